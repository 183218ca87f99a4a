"""Group norm into a bf16 map and the bf16 ResNet block (include/bla.h), as far as a machine without a GPU can check them.

* The references, the bounds and a numpy float32 restatement of both norm entries.  The bounds are those of tests/test_group_norm_gpu.py, u = 2^-24
  (m, v: the mean and variance the entry returned or was given; v is what `stdevs` holds and what the output is divided by -- quirk Q3):
      mean      within 1 fp32 ulp of the float64 mean
      variance  |v - v*| <= 4u v*,  v* = mean((x - m)^2) in float64
      output    |out - y*| <= 4u |y*| against max(y*, 0), y* = (x - m) / v in float64;  dropped elements exactly +0
      gradient  nv = (data - m) / v, A = mean(s), B = mean(nv s), Bbar = mean|nv s|, r* = (s - A - nv B) / v:  |dest - r*| <= 10u (|s| + |A| + |nv| Bbar) / |v|
      map       exact: on the written set (every pixel's position top + y d, left + x d, ALL cp channels) dst equals bla_f32_to_bf16's rounding of the fp32
                output's bits, channels from C up +0; every other element keeps the 0xFFFF it was filled with.
  `check_forward` / `check_gradient` below drive them; tests/test_norm_bf16_gpu.py imports and drives the same functions on the device's outputs.  Here the
  restatement stays inside every bound and equality, and each mutation leaves one: a padding channel not zeroed, the dropout ignored, a chunk that
  straddles two groups normalised with the first group's statistics, the dilation stride ignored in the store position, the map's last row not written.
* `path_of`: the dispatch rule of the two launches (16-byte or 4-byte loads), and the case table reaches every path.
* Every refusal of the four new entries answers BLA_ERR_INVALID (1) through the real library before the device is asked for; sound arguments answer
  BLA_ERR_NO_DEVICE (3) on a machine without a GPU.
* `block_reference`: the whole ResNet block in float64, once with bla_f32_to_bf16's rounding at the composition's points (the operands of every product:
  p1, p2, Q2, q1, the kernel matrices, and x / del_out / the 1 x 1 kernels of the residual entries) and once with no rounding.  `block_differences` is the
  normwise relative difference ||rounded - exact|| / ||exact|| per tensor; tests/test_resnet_bf16_gpu.py holds the device to twice these values.  Recorded
  (result, del_x, conv1, conv2, time_w, time_b[, res]):
      B2 32->32 8x8:  1.4e-03 1.6e-03 3.4e-03 2.9e-03 2.1e-03 2.7e-03
      B2 16->32 6x6:  2.2e-03 2.4e-03 3.6e-03 3.0e-03 3.0e-03 3.0e-03 2.5e-03
      B3 32->32 5x7:  1.5e-03 4.3e-03 9.4e-03 3.0e-03 1.1e-02 1.1e-02
  (pytest -s prints them.)"""
import ctypes as C

import numpy as np
import pytest

from inputs import uniform

F32, F64, U16, U32 = np.float32, np.float64, np.uint16, np.uint32
U = 2.0 ** -24
FILL = 0xFFFF


# ---- geometry, restated ------------------------------------------------------------------------------------------------------------------------------------
def round8(x):
    return -(-x // 8) * 8


def same_geometry(h, w, k, s):
    ho, wo = int(np.ceil(F32(h) / F32(s))), int(np.ceil(F32(w) / F32(s)))
    vpad, hpad = max((ho - 1) * s + k - h, 0), max((wo - 1) * s + k - w, 0)
    return ho, wo, vpad // 2, hpad // 2, vpad, hpad


def layout(h, w, k, s, data_gradient):
    """(hp, wp, top, left, dilate) of bla_conv_bf16_layout"""
    ho, wo, pt, pl, vpad, hpad = same_geometry(h, w, k, s)
    if data_gradient:
        return h + k - 1, w + k - 1, k - 1 - pt, k - 1 - pl, s
    return h + vpad, w + hpad, pt, pl, 1


FORWARD_LAYOUTS = ["next_k3_s1", "next_k3_s2", "next_k1"]
GRADIENT_LAYOUTS = ["dgrad_dilate1", "dgrad_dilate2"]


def destination_layout(name, h, w):
    """where an h x w tensor sits in the operand of the layer that reads it"""
    if name == "next_k3_s1":
        return layout(h, w, 3, 1, False)
    if name == "next_k3_s2":
        return layout(h, w, 3, 2, False)                      # asymmetric TF-SAME padding on even maps
    if name == "next_k1":
        return layout(h, w, 1, 1, False)                      # no halo
    if name == "dgrad_dilate1":
        return layout(h, w, 3, 1, True)
    return layout(2 * h, 2 * w - 1, 3, 2, True)               # the tensor is del_y of a stride-2 layer on a 2h x (2w - 1) input: dilate = 2


def rne(a):
    """bla_f32_to_bf16's rounding (include/bla.h), on float32 bits"""
    u = np.ascontiguousarray(a, F32).view(U32)
    nan = (u & U32(0x7FFFFFFF)) > U32(0x7F800000)
    r = (u.astype(np.uint64) + 0x7FFF + ((u >> U32(16)) & U32(1))) >> np.uint64(16)
    return np.where(nan, (u >> U32(16)) | U32(0x40), r).astype(U16)


def widen(hb):
    return (np.ascontiguousarray(hb, U16).astype(U32) << U32(16)).view(F32)


# (B, C, group_size, H, W, shift): shift = floats by which every fp32 pointer is moved off its 16-byte alignment
CASES = [(2, 5, 32, 3, 5, 0),        # cp = 8 with three padding channels, one short group, odd width: scalar loads
         (3, 40, 16, 6, 6, 0),       # ragged last group; hw % 4 == 0 but w % 4 != 0: 16-byte statistics, scalar apply
         (2, 36, 12, 4, 8, 0),       # chunks straddle groups, cp = 40
         (2, 64, 32, 8, 8, 0),       # whole chunks, 16-byte loads
         (2, 130, 32, 4, 4, 0),      # a third channel tile with 2 live channels
         (1, 32, 32, 24, 24, 0),     # 18,432 per group: over the fp32 family's 16,384 threshold
         (2, 32, 32, 23, 23, 0),     # 16,928 per group, scalar
         (5, 64, 32, 4, 4, 0),
         (1, 8, 8, 1, 2, 0),
         (2, 64, 32, 8, 8, 1)]       # alignment alone forces the scalar loads
SHIFTED = (2, 64, 32, 8, 8, 0)       # forward only, data in [1000, 1001)


def case_id(c):
    return "B%d_C%d_gs%d_%dx%d_off%d" % c


def path_of(h, w, aligned=True):
    """The dispatch rule of both entries (csrc/bla_norm_bf16.hip): the statistics launch reads 16 bytes at a time when h w % 4 == 0, the apply launch when
    w % 4 == 0, each only with every fp32 pointer it touches 16-byte aligned (and d_drop 4-byte aligned); 4 bytes at a time otherwise.  (w % 4 == 0 implies h w % 4 == 0.)"""
    return ("stats16" if aligned and h * w % 4 == 0 else "stats4") + " " + ("apply16" if aligned and w % 4 == 0 else "apply4")


# ---- float64 references and the bounds -------------------------------------------------------------------------------------------------------------------
def group_slices(C_, gs):
    return [(g * gs, min(C_, (g + 1) * gs)) for g in range(-(-C_ // gs))]


def worst(err, bound):
    """the largest err / bound: <= 1 means every element is inside its bound; inf for a NaN or for an error where the bound is zero"""
    err = np.atleast_1d(np.asarray(err, F64)).ravel(); bound = np.atleast_1d(np.asarray(bound, F64)).ravel()
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isfinite(err) & np.isfinite(bound), r, np.inf)
    return float(r.max())


def written_set(shape, top, left, d, h, w):
    m = np.zeros(shape, bool)
    m[:, top:top + (h - 1) * d + 1:d, left:left + (w - 1) * d + 1:d, :] = True
    return m


def check_map(dst, out_f32, lay, what):
    """dst [B][hp][wp][cp] uint16 that started as 0xFFFF, against the fp32 output [B][C][h][w] it must be the rounding of"""
    hp, wp, top, left, d = lay
    B, C_, h, w = out_f32.shape
    cp = round8(C_)
    assert dst.shape == (B, hp, wp, cp)
    want = np.full(dst.shape, FILL, U16)
    pix = np.zeros((B, h, w, cp), U16)                                        # channels from C up: +0
    pix[..., :C_] = rne(out_f32).transpose(0, 2, 3, 1)
    want[:, top:top + (h - 1) * d + 1:d, left:left + (w - 1) * d + 1:d, :] = pix
    ws = written_set(dst.shape, top, left, d, h, w)
    assert np.array_equal(dst[ws], want[ws]), f"{what}: the written set is not the rounding of the fp32 output"
    assert (dst[~ws] == FILL).all(), f"{what}: an element outside the written set changed"


def check_forward(x, drop, m, v, out, dst, gs, lay, what=""):
    """every bound and equality of the forward entry; returns the worst fractions.  x, out [B][C][h][w] float32, m, v [B][groups], drop bool or None"""
    B, C_, h, w = x.shape
    x64 = x.astype(F64)
    frac = dict(mean=0.0, variance=0.0, output=0.0)
    assert not np.isnan(out).any(), f"{what}: an fp32 output element was left out"
    for b in range(B):
        for g, (lo, hi) in enumerate(group_slices(C_, gs)):
            xs = x64[b, lo:hi]; mg, vg = F64(m[b, g]), F64(v[b, g])
            frac["mean"] = max(frac["mean"], worst(abs(mg - xs.mean()), np.spacing(F32(abs(xs.mean()))).astype(F64)))
            vstar = ((xs - mg) ** 2).mean()
            frac["variance"] = max(frac["variance"], worst(abs(vg - vstar), 4 * U * vstar))
            y = (xs - mg) / vg
            keep = np.ones(y.shape, bool) if drop is None else ~drop[b, lo:hi]
            got = out[b, lo:hi].astype(F64)
            frac["output"] = max(frac["output"], worst(np.abs(got - np.maximum(y, 0))[keep], (4 * U * np.abs(y))[keep]))
            assert (out[b, lo:hi][~keep].view(U32) == 0).all(), f"{what}: a dropped element is not +0"
    if dst is not None:
        check_map(dst, out, lay, what)
    return frac


def check_gradient(source, data, m, v, dest, dst, gs, lay, what=""):
    B, C_, h, w = source.shape
    s64, d64 = source.astype(F64), data.astype(F64)
    frac = 0.0
    assert not np.isnan(dest).any(), f"{what}: an fp32 output element was left out"
    for b in range(B):
        for g, (lo, hi) in enumerate(group_slices(C_, gs)):
            mg, vg = F64(m[b, g]), F64(v[b, g])
            s = s64[b, lo:hi]; nv = (d64[b, lo:hi] - mg) / vg
            A = s.mean(); Bm = (nv * s).mean(); Bbar = np.abs(nv * s).mean()
            r = (s - A - nv * Bm) / vg
            bound = 10 * U * (np.abs(s) + abs(A) + np.abs(nv) * Bbar) / abs(vg)
            frac = max(frac, worst(np.abs(dest[b, lo:hi].astype(F64) - r), bound))
    if dst is not None:
        check_map(dst, dest, lay, what)
    return frac


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------------------
def forward_inputs(case, lo=-1.0, hi=3.0):
    B, C_, gs, h, w, _ = case
    seed = 7000 + 10 * CASES.index(case) + (5 if lo > 0 else 0)
    x = uniform(seed, (B, C_, h, w), lo, hi, F32)
    drop = uniform(seed + 1, (B, C_, h, w), 0.0, 1.0, F32) < 0.3
    return x, drop


def gradient_inputs(case):
    """source in [-0.5, 1.5), data in [-1, 3): non-zero means, so the sums matter; m, v: data's float64 statistics rounded to fp32"""
    B, C_, gs, h, w, _ = case
    seed = 7500 + 10 * CASES.index(case)
    source, data = uniform(seed, (B, C_, h, w), -0.5, 1.5, F32), uniform(seed + 1, (B, C_, h, w), -1.0, 3.0, F32)
    G = group_slices(C_, gs)
    m = np.array([[data[b, lo:hi].astype(F64).mean() for lo, hi in G] for b in range(B)])
    v = np.array([[((data[b, lo:hi].astype(F64) - m[b, g]) ** 2).mean() for g, (lo, hi) in enumerate(G)] for b in range(B)])
    assert (v > 0).all()
    return source, data, m.astype(F32), v.astype(F32)


# ---- numpy float32 restatement of the kernels' formulas (every fp32 operation rounds once) ---------------------------------------------------------------
def store_map(values, lay, pad_garbage=False, ignore_dilate=False, skip_last_row=False):
    hp, wp, top, left, d = lay
    B, C_, h, w = values.shape
    cp = round8(C_)
    dst = np.full((B, hp, wp, cp), FILL, U16)
    pix = np.zeros((B, h, w, cp), U16)
    pix[..., :C_] = rne(values).transpose(0, 2, 3, 1)
    if pad_garbage and cp > C_:
        pix[..., C_:] = pix[..., C_ - 1:C_]                       # the tile's stale contents instead of +0
    step = 1 if ignore_dilate else d
    rows = h - 1 if skip_last_row else h
    dst[:, top:top + (rows - 1) * step + 1:step, left:left + (w - 1) * step + 1:step, :] = pix[:, :rows]
    return dst


def restate_forward(x, drop, gs, lay, ignore_drop=False, first_group_stats=False, **store):
    B, C_, h, w = x.shape
    G = group_slices(C_, gs)
    m = np.zeros((B, len(G)), F32); v = np.zeros((B, len(G)), F32); out = np.full(x.shape, np.nan, F32)
    for b in range(B):
        for g, (lo, hi) in enumerate(G):
            xs = x[b, lo:hi]; n = xs.size
            a = xs.astype(F64).sum(); q = (xs.astype(F64) ** 2).sum()
            m[b, g] = F32(a / n); md = F64(m[b, g])
            v[b, g] = F32((q - 2.0 * md * a + n * md * md) / n)
        for c in range(C_):
            g = c // gs
            if first_group_stats:
                g = (c // 8 * 8) // gs                                # the statistics of the chunk's first channel
            y = (x[b, c] - m[b, g]) / v[b, g]
            assert y.dtype == F32
            y = np.where(y < 0, F32(0), y)
            if drop is not None and not ignore_drop:
                y = np.where(drop[b, c], F32(0), y)
            out[b, c] = y
    return m, v, out, store_map(out, lay, **store)


def restate_gradient(source, data, m, v, gs, lay, first_group_stats=False, **store):
    B, C_, h, w = source.shape
    G = group_slices(C_, gs)
    ga = np.zeros((B, len(G)), F32); gb = np.zeros((B, len(G)), F32); out = np.full(source.shape, np.nan, F32)
    for b in range(B):
        for g, (lo, hi) in enumerate(G):
            nv = (data[b, lo:hi] - m[b, g]) / v[b, g]
            n = nv.size
            ga[b, g] = F32(source[b, lo:hi].astype(F64).sum() / n)
            gb[b, g] = F32((nv.astype(F64) * source[b, lo:hi].astype(F64)).sum() / n)
        for c in range(C_):
            g = (c // 8 * 8) // gs if first_group_stats else c // gs
            nv = (data[b, c] - m[b, g]) / v[b, g]
            out[b, c] = (source[b, c] - ga[b, g] - nv * gb[b, g]) / v[b, g]
            assert out.dtype == F32
    return out, store_map(out, lay, **store)


# ---- the restatement against the bounds, and the mutations ----------------------------------------------------------------------------------------------
HOST_CASES = [c for c in CASES if c[3] * c[4] <= 64]             # the large maps add nothing on the host but time


@pytest.mark.parametrize("case,lo,hi", [(c, -1.0, 3.0) for c in HOST_CASES] + [(SHIFTED, 1000.0, 1001.0)],
                         ids=[case_id(c) for c in HOST_CASES] + ["shifted_" + case_id(SHIFTED)])
def test_restated_forward_is_inside_every_bound(case, lo, hi):
    B, C_, gs, h, w, _ = case
    x, drop = forward_inputs(case, lo, hi)
    for name in FORWARD_LAYOUTS:
        lay = destination_layout(name, h, w)
        m, v, out, dst = restate_forward(x, drop, gs, lay)
        frac = check_forward(x, drop, m, v, out, dst, gs, lay, name)
        assert max(frac.values()) <= 1.0, frac


@pytest.mark.parametrize("case", HOST_CASES, ids=case_id)
def test_restated_gradient_is_inside_its_bound(case):
    B, C_, gs, h, w, _ = case
    source, data, m, v = gradient_inputs(case)
    for name in GRADIENT_LAYOUTS:
        lay = destination_layout(name, h, w)
        dest, dst = restate_gradient(source, data, m, v, gs, lay)
        assert check_gradient(source, data, m, v, dest, dst, gs, lay, name) <= 1.0


def test_mutations_leave_the_bounds_or_the_equalities():
    straddle = CASES[2]                                           # group_size 12: the chunk of channels 8..15 holds groups 0 and 1
    B, C_, gs, h, w, _ = straddle
    x, drop = forward_inputs(straddle)
    lay2 = destination_layout("dgrad_dilate2", h, w)
    lay1 = destination_layout("next_k3_s1", h, w)
    m, v, out, dst = restate_forward(x, drop, gs, lay1, first_group_stats=True)
    assert check_forward(x, drop, m, v, out, None, gs, lay1)["output"] > 1.0
    m, v, out, dst = restate_forward(x, drop, gs, lay1, ignore_drop=True)
    with pytest.raises(AssertionError, match="dropped"):
        check_forward(x, drop, m, v, out, dst, gs, lay1)
    source, data, gm, gv = gradient_inputs(straddle)
    dest, dst = restate_gradient(source, data, gm, gv, gs, lay2, first_group_stats=True)
    assert check_gradient(source, data, gm, gv, dest, None, gs, lay2) > 1.0
    for mutation in ("ignore_dilate", "skip_last_row"):
        dest, dst = restate_gradient(source, data, gm, gv, gs, lay2, **{mutation: True})
        with pytest.raises(AssertionError, match="written set|outside"):
            check_gradient(source, data, gm, gv, dest, dst, gs, lay2)
    m, v, out, dst = restate_forward(x, drop, gs, lay1, skip_last_row=True)
    with pytest.raises(AssertionError, match="written set"):
        check_forward(x, drop, m, v, out, dst, gs, lay1)
    pad = CASES[0]                                                # cp = 8, C = 5
    x, drop = forward_inputs(pad)
    layp = destination_layout("next_k3_s2", pad[3], pad[4])
    m, v, out, dst = restate_forward(x, None, pad[2], layp, pad_garbage=True)
    assert (out[:, 4] > 0).any()                                  # the stale channel is not all zeros
    with pytest.raises(AssertionError, match="written set"):
        check_forward(x, None, m, v, out, dst, pad[2], layp)


def test_case_table_reaches_every_path():
    got = [path_of(h, w, shift == 0) for _, _, _, h, w, shift in CASES]
    assert got == ["stats4 apply4", "stats16 apply4", "stats16 apply16", "stats16 apply16", "stats16 apply16", "stats16 apply16", "stats4 apply4",
                   "stats16 apply16", "stats4 apply4", "stats4 apply4"]
    assert set(got) == {"stats16 apply16", "stats16 apply4", "stats4 apply4"}       # (apply16 implies stats16)
    assert [-(-c[1] // 64) for c in CASES][4] == 3 and 130 - 128 == 2                 # the third channel tile's two live channels
    assert 32 * 24 * 24 == 18432 and 32 * 23 * 23 == 16928
    assert any(c[2] % 8 and c[1] > c[2] for c in CASES)                              # a chunk that straddles two groups


# ---- refusals through the real library -------------------------------------------------------------------------------------------------------------------
PTR, ODD = 0x10000, 0x10004       # never dereferenced: every call below is answered before the device is asked for, or by "no device"


def _map(pkg, d=PTR, hp=10, wp=10, cp=8, top=1, left=1, dilate=1):
    return pkg.native.ConvBf16Map(d, hp, wp, cp, top, left, dilate)


def norm_calls(pkg):
    """(name, status getter) for sound arguments and every listed refusal of the two norm entries: 2 x 5 channels 8 x 8 into a 10 x 10 x 8 map"""
    L = pkg.lib()

    def fwd(batch=2, d_in=PTR, ch=5, gs=32, h=8, w=8, sd=PTR, mu=PTR, out=PTR, m="default"):
        mp = _map(pkg) if m == "default" else m
        return L.bla_group_norm_relu_bf16_map(None, batch, d_in, ch, gs, h, w, None, sd, mu, out, C.byref(mp) if mp is not None else None)

    def ddx(batch=2, src=PTR, data=PTR, mu=PTR, sd=PTR, ch=5, gs=32, h=8, w=8, out=PTR, m="default"):
        mp = _map(pkg) if m == "default" else m
        return L.bla_group_norm_ddx_bf16_map(None, batch, src, data, mu, sd, ch, gs, h, w, out, C.byref(mp) if mp is not None else None)

    bad_maps = dict(cp_not_round8=_map(pkg, cp=16), base_off_alignment=_map(pkg, d=ODD), top_negative=_map(pkg, top=-1), left_negative=_map(pkg, left=-1),
                    dilate_zero=_map(pkg, dilate=0), does_not_fit_rows=_map(pkg, hp=8), does_not_fit_columns=_map(pkg, dilate=2),
                    hp_zero=_map(pkg, hp=0), two_to_the_31=_map(pkg, hp=16384, wp=16384))
    refusals = []
    for name, f, ptrs in (("relu", fwd, ("d_in", "sd", "mu")), ("ddx", ddx, ("src", "data", "mu", "sd"))):
        refusals += [(f"{name}:NULL {p}", lambda f=f, p=p: f(**{p: None})) for p in ptrs]
        refusals += [(f"{name}:NULL dst", lambda f=f: f(m=None)), (f"{name}:no output", lambda f=f: f(out=None, m=_map(pkg, d=None)))]
        refusals += [(f"{name}:{e} <= 0", lambda f=f, e=e, v=v: f(**{e: v})) for e in ("batch", "ch", "gs", "h", "w") for v in (0, -1)]
        refusals += [(f"{name}:{k}", lambda f=f, mp=mp: f(m=mp)) for k, mp in bad_maps.items()]
        refusals += [(f"{name}:2^31 with batch", lambda f=f: f(batch=4, m=_map(pkg, hp=8192, wp=8192)))]
        refusals += [(f"{name}:batch above the grid", lambda f=f: f(batch=65536))]
    sound = [("relu", fwd), ("relu fp32 only", lambda: fwd(m=_map(pkg, d=None))), ("relu map only", lambda: fwd(out=None)), ("ddx", ddx),
             ("ddx map only", lambda: ddx(out=None))]
    return sound, refusals


def block_calls(pkg):
    L, N = pkg.lib(), pkg.native
    params = N.ResnetParams(PTR, PTR, PTR, PTR, PTR); grads = N.ResnetGrads(PTR, PTR, PTR, PTR, PTR)
    ws = N.ResnetWs(PTR, PTR, None, PTR, PTR, PTR, PTR, None, None, PTR, PTR); sc = N.ResnetScratch(PTR, PTR, PTR, None)
    maps = N.ResnetBf16Maps(PTR, PTR, PTR)

    def fwd(batch=2, x=PTR, temb=PTR, p=params, drop=PTR, w_=ws, res=PTR, h=8, cin=16, cout=32, k=3, tdim=16, gs=16, m=maps):
        return L.bla_resnet_forward_batched_bf16(None, batch, x, temb, C.byref(p) if p else None, drop, C.byref(w_) if w_ else None, res, h, 8, cin, cout, k, tdim, gs,
                                                 C.byref(m) if m else None)

    def bwd(batch=2, dy=PTR, x=PTR, temb=PTR, p=params, w_=ws, g=grads, s=sc, dtb=PTR, dx=PTR, h=8, cin=16, cout=32, k=3, tdim=16, gs=16, m=maps, splits=0):
        return L.bla_resnet_backward_batched_bf16(None, batch, dy, x, temb, C.byref(p) if p else None, C.byref(w_) if w_ else None, C.byref(g) if g else None,
                                                  C.byref(s) if s else None, dtb, dx, h, 8, cin, cout, k, tdim, gs, C.byref(m) if m else None, splits)

    refusals = [(f"forward:NULL {n}", lambda n=n: fwd(**{n: None})) for n in ("x", "temb", "p", "drop", "w_", "res", "m")]
    refusals += [(f"forward:{n} <= 0", lambda n=n: fwd(**{n: 0})) for n in ("batch", "h", "cin", "cout", "k", "tdim", "gs")]
    refusals += [("forward:NULL conv1", lambda: fwd(p=N.ResnetParams(None, PTR, PTR, PTR, PTR))), ("forward:no residual kernels", lambda: fwd(p=N.ResnetParams(PTR, PTR, PTR, PTR, None))),
                 ("forward:NULL c1", lambda: fwd(w_=N.ResnetWs(PTR, PTR, None, None, PTR, PTR, PTR, None, None, PTR, PTR))),
                 ("forward:NULL p2", lambda: fwd(m=N.ResnetBf16Maps(PTR, None, PTR))), ("forward:p1 off alignment", lambda: fwd(m=N.ResnetBf16Maps(ODD, PTR, PTR)))]
    refusals += [(f"backward:NULL {n}", lambda n=n: bwd(**{n: None})) for n in ("dy", "x", "temb", "p", "w_", "g", "s", "dtb", "m")]
    refusals += [(f"backward:{n} <= 0", lambda n=n: bwd(**{n: 0})) for n in ("batch", "h", "cin", "cout", "k", "tdim", "gs")]
    refusals += [("backward:splits < 0", lambda: bwd(splits=-1)), ("backward:NULL q1", lambda: bwd(m=N.ResnetBf16Maps(PTR, PTR, None))),
                 ("backward:q1 off alignment", lambda: bwd(m=N.ResnetBf16Maps(PTR, PTR, ODD))),
                 ("backward:no residual gradient", lambda: bwd(g=N.ResnetGrads(PTR, PTR, PTR, PTR, None))),
                 ("backward:NULL g_in", lambda: bwd(s=N.ResnetScratch(PTR, PTR, None, None)))]
    sound = [("forward", fwd), ("forward identity", lambda: fwd(cin=32, p=N.ResnetParams(PTR, PTR, PTR, PTR, None))), ("backward", bwd), ("backward no del_x", lambda: bwd(dx=None))]
    return sound, refusals


def test_refusals_answer_invalid_before_the_device_is_asked_for(pkg):
    for calls in (norm_calls, block_calls):
        _, refusals = calls(pkg)
        assert len(refusals) > 20
        for name, call in refusals:
            assert call() == 1, name


def test_sound_arguments_reach_the_device_check(pkg):
    if pkg.lib().bla_device_count() > 0:
        pytest.skip("a device is present: the sound calls would run on placeholder addresses")
    for calls in (norm_calls, block_calls):
        for name, call in calls(pkg)[0]:
            assert call() == 3, name


# ---- the whole block in float64 --------------------------------------------------------------------------------------------------------------------------
#          B  cin cout h  w  gs
BLOCKS = [(2, 32, 32, 8, 8, 32),     # identity residual
          (2, 16, 32, 6, 6, 16),     # 1 x 1 residual
          (3, 32, 32, 5, 7, 32)]     # odd map
K, TDIM = 3, 16
TENSORS = ["result", "del_x", "conv1", "conv2", "time_w", "time_b", "res"]


def block_id(b):
    return "B%d_%dto%d_%dx%d_gs%d" % b


def block_inputs(block):
    B, cin, cout, h, w, gs = block
    s = 9000 + 100 * BLOCKS.index(block)
    I = dict(x=uniform(s, (B, cin, h, w), -1.0, 3.0, F32), temb=uniform(s + 1, (B, TDIM), -1, 1, F32), del_out=uniform(s + 2, (B, cout, h, w), -1, 1, F32),
             conv1=uniform(s + 3, (cout, cin, K, K), -0.25, 0.25, F32), conv2=uniform(s + 4, (cout, cout, K, K), -0.25, 0.25, F32),
             time_w=uniform(s + 5, (TDIM, cout), -0.5, 0.5, F32), time_b=uniform(s + 6, (cout,), -0.5, 0.5, F32),
             res=uniform(s + 7, (cout, cin, 1, 1), -0.5, 0.5, F32), drop=uniform(s + 8, (B, cout, h, w), 0, 1, F32) < 0.3)
    for a in I.values():
        a.setflags(write=False)
    return I


def conv64(x, kern):
    """stride 1, TF-SAME, float64: [B][F][h][w]"""
    B, Cn, h, w = x.shape
    Fn, _, k, _ = kern.shape
    _, _, pt, pl, _, _ = same_geometry(h, w, k, 1)
    xp = np.zeros((B, Cn, h + k - 1, w + k - 1)); xp[:, :, pt:pt + h, pl:pl + w] = x
    out = np.zeros((B, Fn, h, w))
    for p in range(k):
        for q in range(k):
            out += np.einsum("bchw,fc->bfhw", xp[:, :, p:p + h, q:q + w], kern[:, :, p, q])
    return out


def conv64_gradients(dy, x, kern):
    """(del_kern, del_x) of conv64"""
    B, Cn, h, w = x.shape
    Fn, _, k, _ = kern.shape
    _, _, pt, pl, _, _ = same_geometry(h, w, k, 1)
    xp = np.zeros((B, Cn, h + k - 1, w + k - 1)); xp[:, :, pt:pt + h, pl:pl + w] = x
    dxp = np.zeros_like(xp); dk = np.zeros(kern.shape)
    for p in range(k):
        for q in range(k):
            dk[:, :, p, q] = np.einsum("bfhw,bchw->fc", dy, xp[:, :, p:p + h, q:q + w])
            dxp[:, :, p:p + h, q:q + w] += np.einsum("bfhw,fc->bchw", dy, kern[:, :, p, q])
    return dk, dxp[:, :, pt:pt + h, pl:pl + w]


def norm64(x, gs):
    B, C_ = x.shape[:2]
    y = np.empty_like(x); m = np.zeros((B, -(-C_ // gs))); v = np.zeros_like(m)
    for b in range(B):
        for g, (lo, hi) in enumerate(group_slices(C_, gs)):
            m[b, g] = x[b, lo:hi].mean(); v[b, g] = ((x[b, lo:hi] - m[b, g]) ** 2).mean()
            y[b, lo:hi] = (x[b, lo:hi] - m[b, g]) / v[b, g]
    return y, m, v


def norm64_ddx(src, data, m, v, gs):
    r = np.empty_like(src)
    for b in range(src.shape[0]):
        for g, (lo, hi) in enumerate(group_slices(src.shape[1], gs)):
            nv = (data[b, lo:hi] - m[b, g]) / v[b, g]
            s = src[b, lo:hi]
            r[b, lo:hi] = (s - s.mean() - nv * (nv * s).mean()) / v[b, g]
    return r


def block_reference(block, rounded, want_del_x=True, gate1=True, gate2=True):
    """the composition of include/bla.h in float64; rounded: bla_f32_to_bf16's rounding wherever the composition rounds, else none anywhere.
    gate1 / gate2 = False: the mutations -- the data gradient of conv1 / conv2 not gated"""
    B, cin, cout, h, w, gs = block
    I = {n: a.astype(F64) if a.dtype == F32 else a for n, a in block_inputs(block).items()}
    rnd = (lambda a: widen(rne(a.astype(F32))).astype(F64)) if rounded else (lambda a: a)
    y1, m1, v1 = norm64(I["x"], gs)
    p1 = rnd(np.maximum(y1, 0))
    tdense = I["temb"] @ I["time_w"] + I["time_b"]
    c1 = conv64(p1, rnd(I["conv1"])) + tdense[:, :, None, None]
    y2, m2, v2 = norm64(c1, gs)
    p2 = rnd(np.where(I["drop"], 0.0, np.maximum(y2, 0)))
    c2 = conv64(p2, rnd(I["conv2"]))
    r = I["x"] if cin == cout else conv64(rnd(I["x"]), rnd(I["res"]))
    out = dict(result=c2 + r)
    Q2 = rnd(I["del_out"])
    out["conv2"], g_out_a = conv64_gradients(Q2, p2, rnd(I["conv2"]))
    if gate2:
        g_out_a = np.where(p2 > 0, g_out_a, 0.0)
    g_out_b = norm64_ddx(g_out_a, c1, m2, v2, gs)
    q1 = rnd(g_out_b)
    dtb = g_out_b.sum(axis=(2, 3))
    out["time_b"] = dtb.sum(axis=0); out["time_w"] = I["temb"].T @ dtb
    out["conv1"], g_in = conv64_gradients(q1, p1, rnd(I["conv1"]))
    addend = I["del_out"]
    if cin != cout:
        out["res"], addend = conv64_gradients(Q2, rnd(I["x"]), rnd(I["res"]))
    if want_del_x:
        out["del_x"] = norm64_ddx(np.where(p1 > 0, g_in, 0.0) if gate1 else g_in, I["x"], m1, v1, gs) + addend
    return out


def normwise(a, b):
    return float(np.linalg.norm((np.asarray(a, F64) - b).ravel()) / np.linalg.norm(b.ravel()))


def block_differences(block):
    """per tensor: ||rounded - exact|| / ||exact||, and the exact tensors"""
    exact, rounded = block_reference(block, False), block_reference(block, True)
    return {n: normwise(rounded[n], exact[n]) for n in TENSORS if n in exact}, exact


@pytest.mark.parametrize("block", BLOCKS, ids=block_id)
def test_block_rounding_differences_are_recorded(block):
    """Every tensor is recorded and moved by the roundings (bf16's unit roundoff is 2^-9 per operand), and twice the recorded value still fails what the
    device test must catch: a data gradient that is not gated moves every tensor behind it by far more."""
    diff, exact = block_differences(block)
    print(block_id(block), " ".join(f"{n} {diff[n]:.1e}" for n in TENSORS if n in diff))
    assert set(diff) == set(TENSORS) - ({"res"} if block[1] == block[2] else set())
    assert all(d > 0 for d in diff.values())
    no2, no1 = block_reference(block, True, gate2=False), block_reference(block, True, gate1=False)
    for n in ("conv1", "time_w", "time_b", "del_x"):
        assert normwise(no2[n], exact[n]) > 4 * diff[n], n
    assert normwise(no1["del_x"], exact["del_x"]) > 4 * diff["del_x"]
    assert block_inputs(block)["drop"].mean() > 0.2

