"""bla_conv2d_gathered_bf16_chained (include/bla.h): what can be checked without a device.

1. The written set and the value rule of include/bla.h, restated element by element from the header's address formula
       dst[((b hp + top + i dilate) wp + left + j dilate) cp + c] = rne(t) for c < rows, +0 for rows <= c < cp;  nothing else touched
   with t = acc, + bias, relu, gate in float32 in that order.  On every device-test geometry (six products x three destination layouts) and every option
   combination it equals, bit for bit, "plain product -> float32 epilogue in numpy -> the pad restatement (slices of a zero map)" on the written set, and
   leaves 0xFFFF everywhere else.  Four mutations of the restatement leave that equality: top off by one, the dilation ignored, the padding channels not
   zeroed, the gate read at the wrong pixel.
2. The kernel's store map (the half exchange by v_permlane32_swap, csrc/bla_conv_bf16.hip), restated on lane numbers: over the 256 threads every
   (pixel, 8-channel chunk) of the 128 x 128 tile is stored exactly once, a lane's 16 bytes are the chunk's channels in ascending order, and every store
   address is 16-byte aligned in a 16-byte aligned map with cp % 8 == 0.  (The tile is not staged through LDS, so there is no bank rule to count.)
3. Every refusal include/bla.h lists answers BLA_ERR_INVALID through the real library, before the device is asked for; sound arguments answer
   BLA_ERR_NO_DEVICE where there is none.
The geometry and the references are restated here; nothing is imported from another test file.
"""
import ctypes

import numpy as np
import pytest

F32, F64, U16, U32 = np.float32, np.float64, np.uint16, np.uint32

#        B   C    F   H  W  k  s
CASES = [(3, 3, 5, 5, 7, 3, 1), (2, 16, 130, 9, 9, 3, 1), (2, 8, 8, 8, 8, 3, 2), (1, 8, 16, 7, 9, 3, 2), (2, 16, 16, 4, 4, 1, 1), (5, 64, 128, 8, 8, 3, 1)]
IDS = ["B%d_C%d_F%d_%dx%d_k%d_s%d" % c for c in CASES]
LAYOUTS = ["next_k3_s1", "next_k3_s2", "dgrad_dilate2"]
OPTIONS = {"none": dict(), "bias": dict(bias=True), "bias_relu": dict(bias=True, relu=True), "gate": dict(gate=True), "bias_relu_gate": dict(bias=True, relu=True, gate=True)}


# ---- geometry, restated ------------------------------------------------------------------------------------------------------------------------------
def same_geometry(h, w, k, s):
    ho, wo = int(np.ceil(F32(h) / F32(s))), int(np.ceil(F32(w) / F32(s)))
    vpad, hpad = max((ho - 1) * s + k - h, 0), max((wo - 1) * s + k - w, 0)
    return ho, wo, vpad // 2, hpad // 2, vpad, hpad


def layout(h, w, k, s, data_gradient):
    ho, wo, pt, pl, vpad, hpad = same_geometry(h, w, k, s)
    if data_gradient:
        return h + k - 1, w + k - 1, k - 1 - pt, k - 1 - pl, s
    return h + vpad, w + hpad, pt, pl, 1


def round8(x):
    return -(-x // 8) * 8


def destination_layout(name, ho, wo):
    """(hp, wp, top, left, dilate) of the map an ho x wo output is written into."""
    if name == "next_k3_s1":
        return layout(ho, wo, 3, 1, False)
    if name == "next_k3_s2":
        return layout(ho, wo, 3, 2, False)                    # asymmetric TF-SAME padding on even maps
    return layout(2 * ho, 2 * wo - 1, 3, 2, True)             # the ho x wo tensor is del_y of a stride-2 layer on a 2 ho x (2 wo - 1) input: dilate = 2


def to_bf16(a):
    u = np.ascontiguousarray(a, F32).view(U32)
    nan = (u & U32(0x7FFFFFFF)) > U32(0x7F800000)
    rne = (u.astype(np.uint64) + 0x7FFF + ((u >> U32(16)) & U32(1))) >> np.uint64(16)
    return np.where(nan, (u >> U32(16)) | U32(0x40), rne).astype(U16)


def from_bf16(h):
    return (np.ascontiguousarray(h, U16).astype(U32) << U32(16)).view(F32)


def plain_product(x, kern, s):
    """float32 [B][F][Ho][Wo] of bf16-rounded operands (any summation order: both sides of every comparison here start from the same array)"""
    B, Cn, h, w = x.shape
    Fn, _, k, _ = kern.shape
    ho, wo, pt, pl, _, _ = same_geometry(h, w, k, s)
    xp = np.zeros((B, Cn, h + 2 * k + s, w + 2 * k + s), F32)
    xp[:, :, pt:pt + h, pl:pl + w] = x
    out = np.zeros((B, Fn, ho, wo), F32)
    for p in range(k):
        for q in range(k):
            out += np.einsum("bchw,fc->bfhw", xp[:, :, p:p + (ho - 1) * s + 1:s, q:q + (wo - 1) * s + 1:s], kern[:, :, p, q]).astype(F32)
    return out


# ---- the two restatements ----------------------------------------------------------------------------------------------------------------------------
def epilogue_f32(acc, bias, relu, gate_values):
    """include/bla.h's order in numpy float32: one add, relu, the gate (both selections answer +0)"""
    t = acc.astype(F32)
    if bias is not None:
        t = (t + bias[:, :acc.shape[1], None, None]).astype(F32)
    if relu:
        t = np.where(t > 0, t, F32(0))
    if gate_values is not None:
        t = np.where(gate_values > 0, t, F32(0))
    return t.astype(F32)


def pad_restatement(t, hp, wp, top, left, d):
    """bla_conv_bf16_pad of t [B][rows][ho][wo]: a zero map with the rounded tensor at its slices; and the set the chained store writes"""
    B, rows, ho, wo = t.shape
    P = np.zeros((B, hp, wp, round8(rows)), U16)
    P[:, top:top + (ho - 1) * d + 1:d, left:left + (wo - 1) * d + 1:d, :rows] = to_bf16(t).transpose(0, 2, 3, 1)
    written = np.zeros(P.shape, bool)
    written[:, top:top + (ho - 1) * d + 1:d, left:left + (wo - 1) * d + 1:d, :] = True
    return P, written


def chained_restatement(acc, bias, relu, gate_map, gate_geom, dst_init, dst_geom, mutate=None):
    """The header's rule, element by element on flat maps: returns (out_f32, dst).  gate_map / dst_init are flat uint16 arrays, geom = (hp, wp, cp, top, left, dilate)."""
    B, rows, ho, wo = acc.shape
    out, dst = np.zeros(acc.shape, F32), dst_init.copy()
    hp, wp, cp, top, left, d = dst_geom
    if mutate == "top_off_by_one":
        top += 1
    if mutate == "dilation_ignored":
        d = 1
    for b in range(B):
        for i in range(ho):
            for j in range(wo):
                t = acc[b, :, i, j].astype(F32)
                if bias is not None:
                    t = (t + bias[b, :rows]).astype(F32)
                if relu:
                    t = np.where(t > 0, t, F32(0)).astype(F32)
                if gate_map is not None:
                    ghp, gwp, gcp, gtop, gleft, gd = gate_geom
                    gj = (j + 1) % wo if mutate == "gate_wrong_pixel" else j
                    g0 = ((b * ghp + gtop + i * gd) * gwp + gleft + gj * gd) * gcp
                    t = np.where(from_bf16(gate_map[g0:g0 + rows]) > 0, t, F32(0)).astype(F32)
                out[b, :, i, j] = t
                a0 = ((b * hp + top + i * d) * wp + left + j * d) * cp
                dst[a0:a0 + rows] = to_bf16(t)
                if mutate != "padding_channels_not_zeroed":
                    dst[a0 + rows:a0 + cp] = 0
    return out, dst


_cache = {}


def case_data(case):
    if case in _cache:
        return _cache[case]
    B, Cn, Fn, h, w, k, s = case
    ho, wo = same_geometry(h, w, k, s)[:2]
    rng = np.random.default_rng(2400 + CASES.index(case))
    x, kern = (from_bf16(to_bf16(rng.uniform(-1, 1, sh).astype(F32))) for sh in ((B, Cn, h, w), (Fn, Cn, k, k)))
    # the gate: the layer's bf16 input activations in a k3 s1 forward layout, wider than dst (cp = round8(rows) + 8); zeros of both signs among the values,
    # NaN in every place the rule must not read
    ghp, gwp, gtop, gleft, gd = layout(ho, wo, 3, 1, False)
    gcp = round8(Fn) + 8
    gv = rng.uniform(-1, 1, (B, Fn, ho, wo)).astype(F32)
    gv[rng.uniform(size=gv.shape) < 0.2] = 0.0
    gv[rng.uniform(size=gv.shape) < 0.1] = -0.0
    gv = from_bf16(to_bf16(gv))
    gmap = np.full((B, ghp, gwp, gcp), 0x7FC0, U16)
    gmap[:, gtop:gtop + ho, gleft:gleft + wo, :Fn] = to_bf16(gv).transpose(0, 2, 3, 1)
    d = dict(acc=plain_product(x, kern, s), bias=rng.uniform(-1, 1, (B, Fn + 3)).astype(F32), gate_values=gv, gate_map=gmap.reshape(-1),
             gate_geom=(ghp, gwp, gcp, gtop, gleft, gd), ho=ho, wo=wo)
    _cache[case] = d
    return d


def both_ways(case, lay, opt, mutate=None):
    d = case_data(case)
    B, Fn = case[0], case[2]
    hp, wp, top, left, dil = destination_layout(lay, d["ho"], d["wo"])
    cp = round8(Fn)
    bias = d["bias"] if opt.get("bias") else None
    t = epilogue_f32(d["acc"], bias, opt.get("relu"), d["gate_values"] if opt.get("gate") else None)
    want, written = pad_restatement(t, hp, wp, top, left, dil)
    init = np.full(B * hp * wp * cp, 0xFFFF, U16)
    out, dst = chained_restatement(d["acc"], bias, opt.get("relu"), d["gate_map"] if opt.get("gate") else None, d["gate_geom"], init, (hp, wp, cp, top, left, dil), mutate)
    dst = dst.reshape(want.shape)
    same = np.array_equal(out.view(U32), t.view(U32)) and np.array_equal(dst[written], want[written]) and (dst[~written] == 0xFFFF).all()
    return same, written


@pytest.mark.parametrize("lay", LAYOUTS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restated_rule_equals_product_epilogue_pad(case, lay):
    for name, opt in OPTIONS.items():
        same, written = both_ways(case, lay, opt)
        assert same, name
        assert written.any() and not written.all()                       # every layout here has a halo


@pytest.mark.parametrize("mutate", ["top_off_by_one", "dilation_ignored", "padding_channels_not_zeroed", "gate_wrong_pixel"])
def test_mutated_rule_leaves_the_equality(mutate):
    """on a case whose rows are no multiple of 8 (padding channels exist), in the dilated layout (the dilation matters), with every option on"""
    same, _ = both_ways(CASES[0], "dgrad_dilate2", OPTIONS["bias_relu_gate"], mutate)
    assert not same


# ---- the kernel's store map, on lane numbers ------------------------------------------------------------------------------------------------------------
def acc_row(thread, i, r):
    return (thread >> 7) * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * ((thread & 63) >> 5)


def acc_col(thread, j):
    return ((thread >> 6) & 1) * 64 + j * 32 + (thread & 31)


def test_store_map_covers_every_pixel_chunk_once():
    """Each lane packs group g = channels acc_row(i, 4 g .. 4 g + 3) of pixel acc_col(j); the swap of pair m gives lanes 0-31 [own group 2 m | partner's
    group 2 m] and lanes 32-63 [partner's group 2 m + 1 | own group 2 m + 1]; the lane stores that at channel 64 (t >> 7) + 32 i + 16 m + 8 (lane >> 5)."""
    seen = np.zeros((128, 16), int)
    for t in range(256):
        lane, partner = t & 63, t ^ 32
        for j in range(2):
            assert acc_col(t, j) == acc_col(partner, j)                     # the two halves of a chunk belong to the same pixel
            for i in range(2):
                group = lambda th, g: [acc_row(th, i, 4 * g + e) for e in range(4)]
                for m in range(2):
                    held = group(t, 2 * m) + group(partner, 2 * m) if lane < 32 else group(partner, 2 * m + 1) + group(t, 2 * m + 1)
                    ch = (t >> 7) * 64 + i * 32 + 16 * m + 8 * (lane >> 5)
                    assert held == list(range(ch, ch + 8))
                    assert ch % 8 == 0 and (ch * 2) % 16 == 0               # with cp % 8 == 0 and an aligned base: a 16-byte aligned store
                    seen[acc_col(t, j), ch // 8] += 1
    assert (seen == 1).all()


# ---- the entry without a device ------------------------------------------------------------------------------------------------------------------------
X = 0x10000   # a non-NULL, 16-byte aligned stand-in address: nothing is launched in these tests


def chained_call(pkg, bad=None, ep_null=False):
    """rows 5 on a 6 x 6 map, k 3, stride 1; dst in the next k3 s1 layout, the gate in the same one.  `bad` breaks one thing."""
    N = pkg.native
    g = dict(A=X, P=X, rows=5, batch=2, hp=8, wp=8, cp=8, k=3, stride=1, ho=6, wo=6, bias_stride=0, out=X,
             dst=dict(d=X, hp=8, wp=8, cp=8, top=1, left=1, dilate=1), gate=dict(d=X, hp=8, wp=8, cp=8, top=1, left=1, dilate=1))
    for key, v in (bad or {}).items():
        if "." in key:
            m, f = key.split(".")
            g[m][f] = v
        else:
            g[key] = v
    ep = N.ConvBf16Epilogue(bias=None, bias_stride=g["bias_stride"], relu=1, gate=N.ConvBf16Map(**g["gate"]), out_f32=g["out"], dst=N.ConvBf16Map(**g["dst"]))
    return pkg.lib().bla_conv2d_gathered_bf16_chained(None, g["A"], g["rows"], g["P"], g["batch"], g["hp"], g["wp"], g["cp"], g["k"], g["stride"], g["ho"], g["wo"],
                                                      None if ep_null else ctypes.byref(ep))


BAD = [{"out": None, "dst.d": None},                                            # no output at all
       {"A": None}, {"P": None}, {"rows": 0}, {"batch": 0}, {"stride": 0}, {"cp": 12}, {"k": 4}, {"A": X + 8}, {"P": X + 2}, {"bias_stride": -1},   # the existing entry's
       {"dst.cp": 16}, {"dst.cp": 5}, {"rows": 9},                              # dst.cp != round8(rows)
       {"gate.cp": 12}, {"gate.cp": 0}, {"rows": 9, "dst.cp": 16},              # gate.cp % 8, gate.cp < rows
       {"dst.d": X + 8}, {"gate.d": X + 2},                                     # a map base off 16-byte alignment
       {"dst.top": -1}, {"dst.left": -1}, {"dst.dilate": 0}, {"gate.top": -1}, {"gate.left": -1}, {"gate.dilate": 0},
       {"dst.top": 3}, {"dst.left": 3}, {"dst.dilate": 2}, {"dst.hp": 6}, {"gate.top": 3}, {"gate.wp": 6}, {"gate.dilate": 2},    # the output does not fit
       {"dst.hp": 1 << 14, "dst.wp": 1 << 14}, {"gate.hp": 1 << 14, "gate.wp": 1 << 14}]   # batch hp wp cp = 2^32 elements


@pytest.mark.parametrize("bad", BAD, ids=["_".join("%s=%s" % kv for kv in b.items()) for b in BAD])
def test_argument_errors_are_refused_before_the_device(pkg, bad):
    assert chained_call(pkg, bad) == 1, pkg.lib().bla_last_error()


def test_null_epilogue_is_refused(pkg):
    assert chained_call(pkg, ep_null=True) == 1, pkg.lib().bla_last_error()


def test_sound_arguments_reach_the_device_check(pkg):
    import torch
    if torch.cuda.is_available() or pkg.lib().bla_device_count() > 0:
        pytest.skip("a device is present")
    L = pkg.lib()
    for variant in (None, {"out": None}, {"dst.d": None}, {"gate.d": None}, {"dst.d": None, "dst.cp": 0}):   # an absent map is not looked at
        assert chained_call(pkg, variant) == 3, (variant, L.bla_last_error())
        assert b"no CPU fallback" in L.bla_last_error() or b"not initialised" in L.bla_last_error()
