"""bla_conv2d_gathered_bf16_chained on the device (include/bla.h): the gathered bf16 product with a channel-last bf16 output.

Six products, each written into three destination layouts: the forward layout of a following k = 3, s = 1 convolution, that of a following k = 3, s = 2
convolution (asymmetric TF-SAME padding), and a data-gradient layout with dilate = 2.
* Bit-equality with the parent composition, no tolerance: dst starts as 0xFFFF between guard words; afterwards its written set (every output pixel's
  position, ALL dst.cp channels) equals bla_conv_bf16_pad applied to bla_conv2d_gathered_bf16's fp32 output with ReLU / gate applied in numpy float32;
  every other element and the guards still hold 0xFFFF; out_f32 equals the same fp32 values bit for bit.  Options: none, bias, bias + relu, gate,
  bias + relu + gate with both outputs; bias + relu with dst only and with out_f32 only.  The gate map is wider than dst (cp = round8(rows) + 8) and
  holds the bf16 NaN wherever the entry must not read into a result.
* Exact integers (operands, bias and gate in -4..4): out_f32 equals the int64 numpy convolution with ReLU and gate, dst its bla_f32_to_bf16 rounding.
* Rounded operands against float64, no element left out:  |from_bf16(dst) - ref| <= E + 2^-8 (|ref| + E),
      E = (K + 8) 2^-23 (|A|.|B|) + 2 2^-24 (|bias| + |ref|),  K = k k Cp                                     
  (ReLU is 1-Lipschitz and the gate an exact selection, so E carries through them; 2^-8 |t| is the bf16 rounding's half ulp).  The worst ratio is printed;
  measured on an MI355X (profiles/r18_conv_bf16_chain_tests.txt): 0.77 .. 0.97, the half ulp of a value at the bottom of a binade.
* Repeatability: a second call gives identical bits; a second pass into a map zero-filled once leaves its halo, holes and nothing else zero.
* The stack: three layers 8 -> 16 (k3 s1) -> 24 (k3 s2) -> 8 (k3 s1) on 6 x 6, batch 2, bias + ReLU after each.  Forward: one bla_conv_bf16_pad of the
  input, then chained products only.  Backward: one pad of the loss gradient into the last layer's data-gradient layout, then per layer the data
  gradient = the chained entry on Q_L with the flipped matrix at stride 1, gated by the layer's input map P_L, writing Q_(L-1) in the layer below's
  data-gradient layout, and the weight gradient = bla_conv2d_weight_gradient_gathered_bf16 on (Q_L, P_L), splits = 1.  Every activation map, every Q and
  every del_kern equals, bit for bit, the same network run layer by layer through fp32 outputs and a bla_conv_bf16_pad in front of every product.
* bla_gemm_last_kernel() answers the _cl name with dst and the old name without; refusals leave pattern-filled outputs untouched.
The geometry and the references are restated here; nothing is imported from another test file.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F32, F64, U16, U32, I64 = np.float32, np.float64, np.uint16, np.uint32, np.int64
GUARD = 64
NAN16 = 0x7FC0

#        B   C    F   H  W  k  s
CASES = [(3, 3, 5, 5, 7, 3, 1),        # rows = 5 -> dst.cp = 8; one ragged tile; short last slab
         (2, 16, 130, 9, 9, 3, 1),     # two row tiles; dst.cp = 136; pixel tile 0 straddles the image boundary
         (2, 8, 8, 8, 8, 3, 2),        # stride 2, even map
         (1, 8, 16, 7, 9, 3, 2),       # stride 2, odd map
         (2, 16, 16, 4, 4, 1, 1),      # 1 x 1, no halo
         (5, 64, 128, 8, 8, 3, 1)]     # whole tiles
IDS = ["B%d_C%d_F%d_%dx%d_k%d_s%d" % c for c in CASES]
LAYOUTS = ["next_k3_s1", "next_k3_s2", "dgrad_dilate2"]
#           name              bias   relu   gate   out_f32 dst
OPTIONS = [("none",           False, False, False, True,  True),
           ("bias",           True,  False, False, True,  True),
           ("bias_relu",      True,  True,  False, True,  True),
           ("gate",           False, False, True,  True,  True),
           ("bias_relu_gate", True,  True,  True,  True,  True),
           ("dst_only",       True,  True,  False, False, True),
           ("out_f32_only",   True,  True,  False, True,  False)]


@pytest.fixture(scope="module")
def dev(pkg):
    pkg.init(0)
    return pkg


# ---- geometry and references, restated -------------------------------------------------------------------------------------------------------------------
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
    if name == "next_k3_s1":
        return layout(ho, wo, 3, 1, False)
    if name == "next_k3_s2":
        return layout(ho, wo, 3, 2, False)
    return layout(2 * ho, 2 * wo - 1, 3, 2, True)             # the ho x wo tensor is del_y of a stride-2 layer on a 2 ho x (2 wo - 1) input: dilate = 2


def forward_reference(x, kern, s):
    """[B][F][Ho][Wo] in the inputs' dtype (float64 or int64): the im2col convolution with TF-SAME padding"""
    B, Cn, h, w = x.shape
    Fn, _, k, _ = kern.shape
    ho, wo, pt, pl, _, _ = same_geometry(h, w, k, s)
    xp = np.zeros((B, Cn, h + 2 * k + s, w + 2 * k + s), x.dtype)
    xp[:, :, pt:pt + h, pl:pl + w] = x
    out = np.zeros((B, Fn, ho, wo), x.dtype)
    for p in range(k):
        for q in range(k):
            out += np.einsum("bchw,fc->bfhw", xp[:, :, p:p + (ho - 1) * s + 1:s, q:q + (wo - 1) * s + 1:s], kern[:, :, p, q])
    return out


def written_set(shape, top, left, d, ho, wo):
    w = np.zeros(shape, bool)
    w[:, top:top + (ho - 1) * d + 1:d, left:left + (wo - 1) * d + 1:d, :] = True
    return w


# ---- device buffers ------------------------------------------------------------------------------------------------------------------------------------
class Out:
    """`shape` elements that start as 0xFF bytes (fp32: a NaN, bf16: 0xFFFF) with GUARD elements of the same pattern on either side."""

    def __init__(self, dev, shape, dtype=F32):
        self.shape, self.dtype = shape, np.dtype(dtype)
        self.bits = {2: U16, 4: U32}[self.dtype.itemsize]
        self.n = int(np.prod(shape))
        self.arr = dev.DeviceArray((self.n + 2 * GUARD,), self.bits).fill_bytes(0xFF)
        self.ptr = self.arr.ptr + GUARD * self.dtype.itemsize          # 128 or 256 bytes behind a 256-byte aligned base

    def read(self):
        """the body; asserts the guards"""
        now = self.arr.numpy()
        ones = self.bits(~self.bits(0))
        assert (now[:GUARD] == ones).all() and (now[GUARD + self.n:] == ones).all(), "a guard element changed"
        return now[GUARD:GUARD + self.n].reshape(self.shape).view(self.dtype).copy()

    def untouched(self):
        return (self.arr.numpy() == self.bits(~self.bits(0))).all()


def last_name(dev):
    return dev.lib().bla_gemm_last_kernel().decode()


# ---- operands and the parent's results, once per (case, kind) ------------------------------------------------------------------------------------------------
_cache = {}


def case_data(dev, case, kind):
    """Operands on the device, the gate map, and the parent's fp32 outputs (bla_conv2d_gathered_bf16 with and without the bias)."""
    key = (case, kind)
    if key in _cache:
        return _cache[key]
    B, Cn, Fn, h, w, k, s = case
    ho, wo = same_geometry(h, w, k, s)[:2]
    rng = np.random.default_rng(1800 + CASES.index(case))
    shapes = dict(x=(B, Cn, h, w), kern=(Fn, Cn, k, k), bias=(B, Fn + 3), gate=(B, Fn, ho, wo))
    if kind == "exact":
        v = {n: rng.integers(-4, 5, sh).astype(F32) for n, sh in shapes.items()}
    else:
        v = {n: dev.from_bf16(dev.to_bf16(rng.uniform(-1, 1, sh).astype(F32))) for n, sh in shapes.items()}
        v["bias"] = rng.uniform(-1, 1, shapes["bias"]).astype(F32)       # the bias stays fp32
        v["gate"][rng.uniform(size=shapes["gate"]) < 0.2] = 0.0          # zeros of both signs: neither passes the gate
        v["gate"][rng.uniform(size=shapes["gate"]) < 0.1] = -0.0
    d = dict(v, ho=ho, wo=wo)
    hp, wp, top, left, dil = layout(h, w, k, s, False)
    cp = round8(Cn)
    d["P"] = dev.conv_bf16_pad(dev.to_device(v["x"]), dev.empty((B, hp, wp, cp), U16), B, Cn, h, w, hp, wp, top, left, dil)
    d["A"] = dev.conv_bf16_prepare_kernels(dev.to_device(v["kern"]), dev.empty((Fn, k * k * cp), U16), Fn, Cn, k)
    d["p_geom"] = (hp, wp, cp)
    d["bias_dev"] = dev.to_device(v["bias"])
    # the gate: activations in a k3 s1 forward layout, wider than dst; NaN in the halo and in the channels from F up
    ghp, gwp, gtop, gleft, _ = layout(ho, wo, 3, 1, False)
    gcp = round8(Fn) + 8
    gmap = np.full((B, ghp, gwp, gcp), NAN16, U16)
    gmap[:, gtop:gtop + ho, gleft:gleft + wo, :Fn] = dev.to_bf16(v["gate"]).transpose(0, 2, 3, 1)
    d["gate_dev"] = dev.to_device(gmap, U16)
    d["gate_map"] = dev.conv_bf16_map(d["gate_dev"], ghp, gwp, gcp, gtop, gleft, 1)
    for name, bias in (("parent_plain", None), ("parent_bias", d["bias_dev"])):
        out = Out(dev, (B, Fn, ho, wo))
        dev.conv2d_gathered_bf16(d["A"], Fn, d["P"], B, hp, wp, cp, k, s, ho, wo, out.ptr, bias, Fn + 3 if bias else 0)
        dev.sync()
        d[name] = out.read()
    _cache[key] = d
    return d


def parent_values(d, bias, relu, gate):
    """the parent's fp32 output with ReLU / gate applied in numpy float32"""
    t = d["parent_bias"] if bias else d["parent_plain"]
    if relu:
        t = np.where(t > 0, t, F32(0))
    if gate:
        t = np.where(d["gate"] > 0, t, F32(0))
    return np.ascontiguousarray(t, F32)


def parent_map(dev, t, geom):
    """bla_conv_bf16_pad of t into the destination layout"""
    B, rows, ho, wo = t.shape
    hp, wp, top, left, dil = geom
    P = dev.conv_bf16_pad(dev.to_device(t), dev.empty((B, hp, wp, round8(rows)), U16), B, rows, ho, wo, hp, wp, top, left, dil)
    dev.sync()
    return P.numpy()


def run_chained(dev, case, d, geom, bias, relu, gate, want_out, want_dst, dst=None):
    """one chained call into fresh pattern-filled outputs (or the given dst address); returns (Out or None, Out or None)"""
    B, Cn, Fn, h, w, k, s = case
    hp, wp, cp = d["p_geom"]
    dhp, dwp, dtop, dleft, ddil = geom
    out = Out(dev, (B, Fn, d["ho"], d["wo"])) if want_out else None
    if want_dst and dst is None:
        dst = Out(dev, (B, dhp, dwp, round8(Fn)), U16)
    dev.conv2d_gathered_bf16_chained(d["A"], Fn, d["P"], B, hp, wp, cp, k, s, d["ho"], d["wo"],
                                     dst=dev.conv_bf16_map(dst.ptr, dhp, dwp, round8(Fn), dtop, dleft, ddil) if want_dst else None,
                                     out_f32=out.ptr if want_out else None, ep_bias=d["bias_dev"] if bias else None, ep_bias_stride=Fn + 3 if bias else 0,
                                     relu=relu, gate=d["gate_map"] if gate else None)
    dev.sync()
    assert last_name(dev) == "conv_bf16_gather128x128x64_s%d%s" % (s, "_cl" if want_dst else "")
    return out, dst


@pytest.mark.parametrize("lay", LAYOUTS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bit_equal_to_the_parent_composition(dev, case, lay):
    d = case_data(dev, case, "rounded")
    geom = destination_layout(lay, d["ho"], d["wo"])
    for name, bias, relu, gate, want_out, want_dst in OPTIONS:
        t = parent_values(d, bias, relu, gate)
        out, dst = run_chained(dev, case, d, geom, bias, relu, gate, want_out, want_dst)
        if want_out:
            assert np.array_equal(out.read().view(U32), t.view(U32)), name
        if want_dst:
            got, want = dst.read(), parent_map(dev, t, geom)
            written = written_set(want.shape, geom[2], geom[3], geom[4], d["ho"], d["wo"])
            assert np.array_equal(got[written], want[written]), name
            assert (got[~written] == 0xFFFF).all() and (~written).any(), name          # halo, holes: not touched
            assert (got[written].reshape(-1, want.shape[3])[:, case[2]:] == 0).all(), name   # padding channels: the literal +0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exact_integers(dev, case):
    d = case_data(dev, case, "exact")
    B, Cn, Fn, h, w, k, s = case
    geom = destination_layout("dgrad_dilate2", d["ho"], d["wo"])
    fwd = forward_reference(d["x"].astype(I64), d["kern"].astype(I64), s)
    for bias, relu, gate in ((False, False, False), (True, True, True)):
        ref = fwd + d["bias"].astype(I64)[:, :Fn, None, None] if bias else fwd
        ref = np.where(ref > 0, ref, 0) if relu else ref
        ref = (np.where(d["gate"] > 0, ref, 0) if gate else ref).astype(F32)
        out, dst = run_chained(dev, case, d, geom, bias, relu, gate, True, True)
        assert np.array_equal(out.read().view(U32), ref.view(U32))
        got = dst.read()[:, geom[2]:geom[2] + (d["ho"] - 1) * geom[4] + 1:geom[4], geom[3]:geom[3] + (d["wo"] - 1) * geom[4] + 1:geom[4], :]
        assert np.array_equal(got[..., :Fn], dev.to_bf16(ref).transpose(0, 2, 3, 1)) and (got[..., Fn:] == 0).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rounded_data_against_float64(dev, case):
    d = case_data(dev, case, "rounded")
    B, Cn, Fn, h, w, k, s = case
    geom = destination_layout("next_k3_s2", d["ho"], d["wo"])
    pre = forward_reference(d["x"].astype(F64), d["kern"].astype(F64), s)
    apre = forward_reference(np.abs(d["x"]).astype(F64), np.abs(d["kern"]).astype(F64), s)
    e, u = 2.0 ** -23, 2.0 ** -24
    for bias, relu, gate in ((False, False, False), (True, True, False), (True, True, True)):
        b64 = d["bias"].astype(F64)[:, :Fn, None, None] if bias else np.zeros((1, 1, 1, 1))
        ref = pre + b64
        E = (k * k * round8(Cn) + 8) * e * apre + 2 * u * (np.abs(b64) + np.abs(ref))
        ref = np.where(ref > 0, ref, 0.0) if relu else ref
        ref = np.where(d["gate"] > 0, ref, 0.0) if gate else ref
        bound = E + 2.0 ** -8 * (np.abs(ref) + E)
        _, dst = run_chained(dev, case, d, geom, bias, relu, gate, False, True)
        got = dst.read()[:, geom[2]:geom[2] + (d["ho"] - 1) * geom[4] + 1:geom[4], geom[3]:geom[3] + (d["wo"] - 1) * geom[4] + 1:geom[4], :Fn]
        got = dev.from_bf16(got).transpose(0, 3, 1, 2).astype(F64)
        assert got.shape == ref.shape and np.isfinite(got).all()
        err = np.abs(got - ref)
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print("conv_bf16_chain %s bias %d relu %d gate %d: worst |err| / bound = %.4f (max |err| %.3e)" % ("B%d_C%d_F%d_%dx%d_k%d_s%d" % case, bias, relu, gate, worst, err.max()))
        assert (err <= bound).all(), worst


@pytest.mark.parametrize("case", [CASES[0], CASES[1]], ids=[IDS[0], IDS[1]])
def test_repeatable_and_the_halo_stays_zero(dev, case):
    d = case_data(dev, case, "rounded")
    B, Fn = case[0], case[2]
    geom = destination_layout("dgrad_dilate2", d["ho"], d["wo"])
    out1, dst1 = run_chained(dev, case, d, geom, True, True, True, True, True)
    out2, dst2 = run_chained(dev, case, d, geom, True, True, True, True, True)
    assert np.array_equal(out1.read().view(U32), out2.read().view(U32)) and np.array_equal(dst1.read(), dst2.read())
    # a map zero-filled once, written by two passes with different epilogues: the second pass's values on the written set, zero everywhere else
    zeroed = dev.zeros((B, geom[0], geom[1], round8(Fn)), U16)
    run_chained(dev, case, d, geom, False, False, False, False, True, dst=zeroed)
    run_chained(dev, case, d, geom, True, True, False, False, True, dst=zeroed)
    got = zeroed.numpy()
    assert np.array_equal(got, parent_map(dev, parent_values(d, True, True, False), geom))


# ---- the stack -------------------------------------------------------------------------------------------------------------------------------------------
def test_three_layer_stack_forward_and_backward(dev):
    B, h0, k = 2, 6, 3
    chans, strides = [8, 16, 24, 8], [1, 2, 1]
    rng = np.random.default_rng(18)
    x = rng.uniform(-1, 1, (B, chans[0], h0, h0)).astype(F32)
    sizes = [h0]
    for s in strides:
        sizes.append(same_geometry(sizes[-1], sizes[-1], k, s)[0])                       # 6, 6, 3, 3
    kerns = [rng.uniform(-0.3, 0.3, (chans[l + 1], chans[l], k, k)).astype(F32) for l in range(3)]
    biases = [dev.to_device(rng.uniform(-0.2, 0.2, (B, chans[l + 1])).astype(F32)) for l in range(3)]
    loss_grad = rng.uniform(-1, 1, (B, chans[3], sizes[3], sizes[3])).astype(F32)
    A = [dev.conv_bf16_prepare_kernels(dev.to_device(kerns[l]), dev.empty((chans[l + 1], k * k * round8(chans[l])), U16), chans[l + 1], chans[l], k) for l in range(3)]
    Af = [dev.conv_bf16_prepare_kernels(dev.to_device(kerns[l]), dev.empty((chans[l], k * k * round8(chans[l + 1])), U16), chans[l + 1], chans[l], k, True) for l in range(3)]
    # P[l]: layer l's input in its forward layout; P[3]: the last output, in the layout of a following k3 s1 layer.  Q[l]: the gradient at layer l's
    # pre-activation output in layer l's data-gradient layout; Q[-1] ("below layer 0"): a k3 s1 layer's
    pgeom = [layout(sizes[l], sizes[l], k, strides[l], False) for l in range(3)] + [layout(sizes[3], sizes[3], k, 1, False)]
    qgeom = {l: layout(sizes[l], sizes[l], k, strides[l], True) for l in range(3)}
    qgeom[-1] = layout(sizes[0], sizes[0], k, 1, True)

    def pad(t, geom):
        Bn, c, hh, ww = t.shape
        return dev.conv_bf16_pad(dev.to_device(t), dev.empty((Bn, geom[0], geom[1], round8(c)), U16), Bn, c, hh, ww, *geom)

    def amap(arr, geom, c):
        return dev.conv_bf16_map(arr, geom[0], geom[1], round8(c), geom[2], geom[3], geom[4])

    # ---- the parent's way: fp32 outputs, numpy epilogues, a pad in front of every product
    rP = [pad(x, pgeom[0])]
    for l in range(3):
        y = dev.empty((B, chans[l + 1], sizes[l + 1], sizes[l + 1]))
        dev.conv2d_gathered_bf16(A[l], chans[l + 1], rP[l], B, pgeom[l][0], pgeom[l][1], round8(chans[l]), k, strides[l], sizes[l + 1], sizes[l + 1], y, biases[l], chans[l + 1])
        y = y.numpy()
        rP.append(pad(np.where(y > 0, y, F32(0)).astype(F32), pgeom[l + 1]))
    rQ, rdK = {2: pad(loss_grad, qgeom[2])}, {}
    for l in (2, 1, 0):
        hq, wq, qtop, qleft, qdil = qgeom[l]
        rdK[l] = dev.empty(kerns[l].shape)
        dev.conv2d_weight_gradient_gathered_bf16(rQ[l], hq, wq, round8(chans[l + 1]), qtop, qleft, qdil, rP[l], pgeom[l][0], pgeom[l][1], round8(chans[l]), B, k, strides[l],
                                                 sizes[l + 1], sizes[l + 1], chans[l + 1], chans[l], rdK[l], splits=1)
        dx = dev.empty((B, chans[l], sizes[l], sizes[l]))
        dev.conv2d_gathered_bf16(Af[l], chans[l], rQ[l], B, hq, wq, round8(chans[l + 1]), k, 1, sizes[l], sizes[l], dx)
        top, left = pgeom[l][2], pgeom[l][3]
        act = dev.from_bf16(rP[l].numpy()[:, top:top + sizes[l], left:left + sizes[l], :chans[l]]).transpose(0, 3, 1, 2)
        rQ[l - 1] = pad(np.where(act > 0, dx.numpy(), F32(0)).astype(F32), qgeom[l - 1])

    # ---- chained: one pad of the input, one of the loss gradient, zero-filled maps, chained products only
    cP = [pad(x, pgeom[0])] + [dev.zeros((B, pgeom[l][0], pgeom[l][1], round8(chans[l])), U16) for l in (1, 2, 3)]
    for l in range(3):
        dev.conv2d_gathered_bf16_chained(A[l], chans[l + 1], cP[l], B, pgeom[l][0], pgeom[l][1], round8(chans[l]), k, strides[l], sizes[l + 1], sizes[l + 1],
                                         dst=amap(cP[l + 1], pgeom[l + 1], chans[l + 1]), ep_bias=biases[l], ep_bias_stride=chans[l + 1], relu=True)
        assert last_name(dev) == "conv_bf16_gather128x128x64_s%d_cl" % strides[l]
    cQ, cdK = {2: pad(loss_grad, qgeom[2])}, {}
    for l in (1, 0, -1):
        cQ[l] = dev.zeros((B, qgeom[l][0], qgeom[l][1], round8(chans[l + 1])), U16)
    for l in (2, 1, 0):
        hq, wq, qtop, qleft, qdil = qgeom[l]
        cdK[l] = dev.empty(kerns[l].shape)
        dev.conv2d_weight_gradient_gathered_bf16(cQ[l], hq, wq, round8(chans[l + 1]), qtop, qleft, qdil, cP[l], pgeom[l][0], pgeom[l][1], round8(chans[l]), B, k, strides[l],
                                                 sizes[l + 1], sizes[l + 1], chans[l + 1], chans[l], cdK[l], splits=1)
        dev.conv2d_gathered_bf16_chained(Af[l], chans[l], cQ[l], B, hq, wq, round8(chans[l + 1]), k, 1, sizes[l], sizes[l],
                                         dst=amap(cQ[l - 1], qgeom[l - 1], chans[l]), gate=amap(cP[l], pgeom[l], chans[l]))
    dev.sync()
    for l in range(4):
        assert np.array_equal(cP[l].numpy(), rP[l].numpy()), "activation map %d" % l
    for l in (2, 1, 0, -1):
        assert np.array_equal(cQ[l].numpy(), rQ[l].numpy()), "gradient map %d" % l
    for l in range(3):
        assert np.array_equal(cdK[l].numpy().view(U32), rdK[l].numpy().view(U32)), "del_kern %d" % l
        assert np.abs(rdK[l].numpy()).max() > 0
    assert (rP[3].numpy() != 0).any() and (rQ[-1].numpy() != 0).any()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(dev):
    B, Fn, h, w, k = 2, 5, 6, 6, 3
    P, A = dev.zeros((B, h + 2, w + 2, 8), U16), dev.zeros((Fn, k * k * 8), U16)
    out, dst, gate = Out(dev, (B, Fn, h, w)), Out(dev, (B, h + 2, w + 2, 8), U16), dev.zeros((B, h + 2, w + 2, 8), U16)
    N = dev.native

    def refused(rows=Fn, a=None, cp=8, stride=1, out_ptr=out.ptr, null_ep=False, d=None, g=None):
        m = dict(d=dst.ptr, hp=h + 2, wp=w + 2, cp=8, top=1, left=1, dilate=1)
        dm, gm = {**m, **(d or {})}, {**m, "d": gate.ptr, **(g or {})}
        ep = N.ConvBf16Epilogue(bias=None, bias_stride=0, relu=1, gate=N.ConvBf16Map(**gm), out_f32=out_ptr, dst=N.ConvBf16Map(**dm))
        st = dev.lib().bla_conv2d_gathered_bf16_chained(None, A.ptr if a is None else a, rows, P.ptr, B, h + 2, w + 2, cp, k, stride, h, w, None if null_ep else ctypes.byref(ep))
        dev.sync()
        return st == 1

    assert refused(null_ep=True)
    assert refused(out_ptr=None, d=dict(d=None))
    assert refused(rows=0) and refused(cp=12) and refused(stride=0) and refused(a=A.ptr + 2) and refused(stride=2)     # the existing entry's
    assert refused(d=dict(cp=16)) and refused(rows=9)                                # dst.cp != round8(rows)
    assert refused(g=dict(cp=12)) and refused(rows=9, d=dict(cp=16))                 # gate.cp % 8, gate.cp < rows
    assert refused(d=dict(d=dst.ptr + 8)) and refused(g=dict(d=gate.ptr + 2))        # alignment
    assert refused(d=dict(top=-1)) and refused(d=dict(left=-1)) and refused(d=dict(dilate=0)) and refused(g=dict(dilate=0))
    assert refused(d=dict(top=3)) and refused(d=dict(dilate=2)) and refused(g=dict(left=3)) and refused(d=dict(wp=6))    # the output does not fit
    assert refused(d=dict(hp=1 << 14, wp=1 << 14))                                   # 2^32 elements
    assert out.untouched() and dst.untouched()
    assert not refused()                                                             # and the same arguments, sound, run
