"""Mixed-precision convolution on the device: bla_conv_bf16_pad, bla_conv_bf16_prepare_kernels, bla_conv2d_gathered_bf16 and the two _as_bf16 entries.

* Pad and kernel preparation: bit-equal to a numpy restatement of include/bla.h's layouts built on native.to_bf16, dilation 1 and 2; the destination
  starts as 0xFF bytes, so every halo element, hole and padding channel is seen to be written +0.
* Exact products, no tolerance: operands are integers in -4..4 (exact in bf16), every partial sum is an integer far below 2^24, so forward, data gradient
  and weight gradient must equal an integer numpy convolution bit for bit.
* Rounded data: operands uniform [-1, 1) rounded to bf16 on the host, reference = float64 im2col convolution of the rounded values, per element
      |got - ref| <= (K + 8) 2^-23 (|A|.|B|) + 2 2^-24 (|bias| + |ref|)                                                          
  with K = k k Cp (forward), k k Fp (data gradient), B Ho Wo rounded up to 8 (weight gradient).  No element is left out; the worst ratio is printed.
  Measured on an MI355X (profiles/r13_conv_bf16_tests.txt): worst ratio 0.024 (forward), 0.015 (data gradient), 0.011 (weight gradient).
* Outputs start as the 0xFF NaN pattern between 64 guard floats on either side, which keep their bits; a second run is bit-identical.
* Both _as_bf16 entries equal the composition of the three entries made here (the weight gradient: bla_gemm_bf16 nt on a host-made bf16 im2col), bit for
  bit; the backward entry with either output NULL; the bias epilogue with ep_bias_stride != rows; bla_gemm_last_kernel(); the refusals.
The SAME geometry and the im2col reference are restated here (as in test_conv_bf16_host.py); nothing is imported from another test file.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F32, F64, U16, U32, I64 = np.float32, np.float64, np.uint16, np.uint32, np.int64
GUARD = 64

#        B   C    F   H  W  k  s
CASES = [(3, 3, 5, 5, 7, 3, 1),        # Cp = 8, K = 72: a short last slab, a single ragged tile
         (2, 16, 130, 9, 9, 3, 1),     # two row tiles; 162 columns: pixel tile 0 straddles the image boundary at 81, tile 1 is ragged
         (2, 24, 8, 8, 8, 3, 1),       # slabs that cross tap boundaries
         (2, 12, 20, 6, 6, 3, 1),      # channel padding inside every tap
         (2, 8, 8, 8, 8, 3, 2),        # stride 2, even map; the dilated data gradient
         (1, 8, 16, 7, 9, 3, 2),       # stride 2, odd map
         (2, 16, 16, 4, 4, 1, 1),      # 1 x 1: no halo
         (1, 8, 8, 6, 6, 5, 1),        # k = 5
         (5, 64, 128, 8, 8, 3, 1),     # several whole tiles, K = 576 = nine whole slabs
         (1, 8, 1100, 4, 4, 1, 1)]     # F = 1100: nine row tiles = a group of 8 and a last group of 1 (the tile order's short last group), one ragged pixel tile, K = 8
IDS = ["B%d_C%d_F%d_%dx%d_k%d_s%d" % c for c in CASES]


@pytest.fixture(scope="module")
def dev(pkg):
    pkg.init(0)
    return pkg


# ---- geometry and the im2col reference, restated ---------------------------------------------------------------------------------------------------------
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


def im2col(x, k, s):
    """x [B][C][H][W] -> cols [B][Ho Wo][C k k], cols[b][(i, j)][(c, p, q)] = x[b][c][i s + p - pt][j s + q - pl], 0 outside."""
    B, Cn, h, w = x.shape
    ho, wo, pt, pl, _, _ = same_geometry(h, w, k, s)
    xp = np.zeros((B, Cn, h + 2 * k + s, w + 2 * k + s), x.dtype)
    xp[:, :, pt:pt + h, pl:pl + w] = x
    cols = np.zeros((B, ho, wo, Cn, k, k), x.dtype)
    for p in range(k):
        for q in range(k):
            cols[:, :, :, :, p, q] = xp[:, :, p:p + (ho - 1) * s + 1:s, q:q + (wo - 1) * s + 1:s].transpose(0, 2, 3, 1)
    return cols.reshape(B, ho * wo, Cn * k * k)


def conv_reference(x, kern, del_y, s):
    """forward [B][F][Ho][Wo], del_x [B][C][H][W] (the adjoint of the forward map), del_kern [F][C][k][k], in the inputs' dtype (float64 or int64)."""
    B, Cn, h, w = x.shape
    Fn, _, k, _ = kern.shape
    ho, wo, pt, pl, _, _ = same_geometry(h, w, k, s)
    cols = im2col(x, k, s)
    kmat = kern.reshape(Fn, Cn * k * k)
    fwd = np.einsum("bnk,fk->bfn", cols, kmat).reshape(B, Fn, ho, wo)
    dy = del_y.reshape(B, Fn, ho * wo)
    dkern = np.einsum("bfn,bnk->fk", dy, cols).reshape(kern.shape)
    dcols = np.einsum("bfn,fk->bnk", dy, kmat).reshape(B, ho, wo, Cn, k, k)
    dxp = np.zeros((B, Cn, h + 2 * k + s, w + 2 * k + s), x.dtype)
    for p in range(k):
        for q in range(k):
            dxp[:, :, p:p + (ho - 1) * s + 1:s, q:q + (wo - 1) * s + 1:s] += dcols[:, :, :, :, p, q].transpose(0, 3, 1, 2)
    return fwd, dxp[:, :, pt:pt + h, pl:pl + w].copy(), dkern


def padded_channel_last(dev, src, hp, wp, top, left, d):
    """include/bla.h's P as bf16 bit patterns"""
    B, Cn, h, w = src.shape
    P = np.zeros((B, hp, wp, round8(Cn)), U16)
    P[:, top:top + (h - 1) * d + 1:d, left:left + (w - 1) * d + 1:d, :Cn] = dev.to_bf16(src).transpose(0, 2, 3, 1)
    return P


def kernel_matrix(dev, kern, data_gradient):
    Fn, Cn, k, _ = kern.shape
    k16 = dev.to_bf16(kern)
    if not data_gradient:
        A = np.zeros((Fn, k, k, round8(Cn)), U16)
        A[:, :, :, :Cn] = k16.transpose(0, 2, 3, 1)
        return A.reshape(Fn, -1)
    A = np.zeros((Cn, k, k, round8(Fn)), U16)
    A[:, :, :, :Fn] = k16.transpose(1, 2, 3, 0)[:, ::-1, ::-1, :]
    return A.reshape(Cn, -1)


# ---- device buffers ------------------------------------------------------------------------------------------------------------------------------------
class Out:
    """`shape` elements that start as 0xFF bytes (fp32: a NaN) with GUARD elements of the same pattern on either side."""

    def __init__(self, dev, shape, dtype=F32):
        self.shape, self.dtype = shape, np.dtype(dtype)
        self.bits = {2: U16, 4: U32}[self.dtype.itemsize]
        self.n = int(np.prod(shape))
        self.dev = dev
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


def call(dev, name, *args, want=0):
    st = getattr(dev.lib(), name)(None, *args)
    assert st == want, (name, st, dev.lib().bla_last_error())
    dev.sync()


def p(a):
    return a.ptr


# ---- operands and references, computed once per case ---------------------------------------------------------------------------------------------------
_cache = {}


def case_data(dev, case, kind):
    key = (case, kind)
    if key in _cache:
        return _cache[key]
    B, Cn, Fn, h, w, k, s = case
    ho, wo = same_geometry(h, w, k, s)[:2]
    rng = np.random.default_rng(1000 + CASES.index(case))
    shapes = dict(x=(B, Cn, h, w), kern=(Fn, Cn, k, k), dy=(B, Fn, ho, wo), bias=(B, Fn + 3))
    if kind == "exact":
        v = {n: rng.integers(-4, 5, sh).astype(F32) for n, sh in shapes.items()}
        ref = conv_reference(v["x"].astype(I64), v["kern"].astype(I64), v["dy"].astype(I64), s)
        d = dict(v, fwd=(ref[0] + v["bias"].astype(I64)[:, :Fn, None, None]).astype(F32), dx=ref[1].astype(F32), dkern=ref[2].astype(F32))
    else:
        v = {n: dev.from_bf16(dev.to_bf16(rng.uniform(-1, 1, sh).astype(F32))) for n, sh in shapes.items()}
        v["bias"] = rng.uniform(-1, 1, shapes["bias"]).astype(F32)       # the bias stays fp32
        fwd, dx, dkern = conv_reference(v["x"].astype(F64), v["kern"].astype(F64), v["dy"].astype(F64), s)
        afwd, adx, adkern = conv_reference(np.abs(v["x"]).astype(F64), np.abs(v["kern"]).astype(F64), np.abs(v["dy"]).astype(F64), s)
        bias = v["bias"].astype(F64)[:, :Fn, None, None]
        fwd = fwd + bias
        e, u = 2.0 ** -23, 2.0 ** -24
        d = dict(v, fwd=fwd, dx=dx, dkern=dkern,
                 bound_fwd=(k * k * round8(Cn) + 8) * e * afwd + 2 * u * (np.abs(bias) + np.abs(fwd)),
                 bound_dx=(k * k * round8(Fn) + 8) * e * adx + 2 * u * np.abs(dx),
                 bound_dkern=(round8(B * ho * wo) + 8) * e * adkern + 2 * u * np.abs(dkern))
    d["dev"] = {n: dev.to_device(d[n]) for n in shapes}
    _cache[key] = d
    return d


def run_entries(dev, case, d):
    """forward (bias at stride F + 3), both gradients: three Out buffers"""
    B, Cn, Fn, h, w, k, s = case
    ho, wo = same_geometry(h, w, k, s)[:2]
    g = d["dev"]
    out, dx, dk = Out(dev, (B, Fn, ho, wo)), Out(dev, (B, Cn, h, w)), Out(dev, (Fn, Cn, k, k))
    call(dev, "bla_conv2d_forward_batched_f32_as_bf16", p(g["x"]), p(g["kern"]), out.ptr, B, h, w, k, Cn, Fn, s, p(g["bias"]), Fn + 3)
    name_f = last_name(dev)
    call(dev, "bla_conv2d_backward_batched_f32_as_bf16", p(g["dy"]), p(g["x"]), p(g["kern"]), dk.ptr, dx.ptr, B, h, w, k, Cn, Fn, s)
    return out.read(), dx.read(), dk.read(), name_f, last_name(dev)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exact_products(dev, case):
    d = case_data(dev, case, "exact")
    out, dx, dk, name_f, name_b = run_entries(dev, case, d)
    assert name_f == "conv_bf16_gather128x128x64_s%d" % case[6] and name_b == "conv_bf16_gather128x128x64_s1"
    assert np.array_equal(out.view(U32), d["fwd"].view(U32))
    assert np.array_equal(dx.view(U32), d["dx"].view(U32))
    assert np.array_equal(dk.view(U32), d["dkern"].view(U32))
    again = run_entries(dev, case, d)
    assert all(np.array_equal(a.view(U32), b.view(U32)) for a, b in zip((out, dx, dk), again[:3]))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rounded_data_against_float64(dev, case):
    d = case_data(dev, case, "rounded")
    out, dx, dk, _, _ = run_entries(dev, case, d)
    worst = {}
    for name, got, ref, bound in (("forward", out, d["fwd"], d["bound_fwd"]), ("data gradient", dx, d["dx"], d["bound_dx"]),
                                  ("weight gradient", dk, d["dkern"], d["bound_dkern"])):
        assert got.shape == ref.shape and np.isfinite(got).all(), name
        err = np.abs(got.astype(F64) - ref)
        worst[name] = float((err / np.maximum(bound, 1e-300)).max())
        print("conv_bf16 %s %s: worst |err| / bound = %.4f (max |err| %.3e)" % ("B%d_C%d_F%d_%dx%d_k%d_s%d" % case, name, worst[name], err.max()))
        assert (err <= bound).all(), (name, worst[name])
    again = run_entries(dev, case, d)
    assert all(np.array_equal(a.view(U32), b.view(U32)) for a, b in zip((out, dx, dk), again[:3]))


# ---- pad and kernel preparation ---------------------------------------------------------------------------------------------------------------------------
PAD_CASES = [(3, 3, 5, 7, 7, 9, 1, 1, 1),          # B, C, h, w, hp, wp, top, left, dilate: Cp = 8, 4-byte loads (w % 4 != 0)
             (2, 12, 6, 8, 8, 10, 1, 1, 1),        # channel padding, 16-byte loads
             (2, 20, 4, 5, 9, 11, 1, 2, 2),        # dilation 2: holes, and a halo wider on one side
             (1, 70, 3, 68, 5, 70, 1, 1, 1),       # two channel tiles and two x tiles
             (1, 8, 2, 66, 6, 135, 2, 1, 2)]       # two x tiles under dilation 2


@pytest.mark.parametrize("case", PAD_CASES, ids=lambda c: "B%d_C%d_%dx%d_to_%dx%d_t%d_l%d_d%d" % c)
def test_pad_is_bit_equal_and_writes_every_element(dev, case):
    B, Cn, h, w, hp, wp, top, left, d = case
    src = np.random.default_rng(sum(case)).uniform(-1, 1, (B, Cn, h, w)).astype(F32)
    src[0, 0, 0, :2] = [-0.0, np.inf]
    dst = Out(dev, (B, hp, wp, round8(Cn)), U16)
    call(dev, "bla_conv_bf16_pad", p(dev.to_device(src)), dst.ptr, B, Cn, h, w, hp, wp, top, left, d)
    got, want = dst.read(), padded_channel_last(dev, src, hp, wp, top, left, d)
    assert np.array_equal(got, want)
    written = np.zeros(want.shape, bool)
    written[:, top:top + (h - 1) * d + 1:d, left:left + (w - 1) * d + 1:d, :Cn] = True
    assert (got[~written] == 0).all() and (~written).sum() > 0          # halo, holes, padding channels: +0, none left at 0xFFFF


@pytest.mark.parametrize("data_gradient", [0, 1])
@pytest.mark.parametrize("shape", [(5, 3, 3), (20, 12, 3), (8, 24, 1), (130, 16, 5)], ids=lambda s: "F%d_C%d_k%d" % s)
def test_prepare_kernels_is_bit_equal(dev, shape, data_gradient):
    Fn, Cn, k = shape
    kern = np.random.default_rng(Fn).uniform(-1, 1, (Fn, Cn, k, k)).astype(F32)
    want = kernel_matrix(dev, kern, data_gradient)
    dst = Out(dev, want.shape, U16)
    call(dev, "bla_conv_bf16_prepare_kernels", p(dev.to_device(kern)), dst.ptr, Fn, Cn, k, data_gradient)
    got = dst.read()
    assert np.array_equal(got, want)
    inner, ip = (Fn, round8(Fn)) if data_gradient else (Cn, round8(Cn))
    assert (got.reshape(-1, ip)[:, inner:] == 0).all()


def test_layout_entry(dev):
    for h, w, k, s in [(32, 32, 3, 1), (7, 9, 3, 2), (8, 8, 5, 2), (4, 4, 1, 1)]:
        for dg in (False, True):
            assert dev.conv_bf16_layout(h, w, k, s, dg) == layout(h, w, k, s, dg)


# ---- the entries against their composition ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[1], CASES[3], CASES[5]], ids=[IDS[1], IDS[3], IDS[5]])
def test_as_bf16_entries_equal_the_composition(dev, case):
    B, Cn, Fn, h, w, k, s = case
    ho, wo = same_geometry(h, w, k, s)[:2]
    d = case_data(dev, case, "rounded")
    g = d["dev"]
    out, dx, dk, _, _ = run_entries(dev, case, d)
    # forward: pad + prepare + gathered product, by the Python helpers
    hp, wp, top, left, dil = dev.conv_bf16_layout(h, w, k, s)
    P = dev.conv_bf16_pad(g["x"], dev.empty((B, hp, wp, round8(Cn)), U16), B, Cn, h, w, hp, wp, top, left, dil)
    A = dev.conv_bf16_prepare_kernels(g["kern"], dev.empty((Fn, k * k * round8(Cn)), U16), Fn, Cn, k)
    mine = Out(dev, (B, Fn, ho, wo))
    dev.conv2d_gathered_bf16(A, Fn, P, B, hp, wp, round8(Cn), k, s, ho, wo, mine.ptr, g["bias"], Fn + 3)
    dev.sync()
    assert last_name(dev) == "conv_bf16_gather128x128x64_s%d" % s
    assert np.array_equal(mine.read().view(U32), out.view(U32))
    # data gradient: del_y dilated into its layout, the flipped matrix, the same product at stride 1
    hp, wp, top, left, dil = dev.conv_bf16_layout(h, w, k, s, True)
    assert dil == s
    P = dev.conv_bf16_pad(g["dy"], dev.empty((B, hp, wp, round8(Fn)), U16), B, Fn, ho, wo, hp, wp, top, left, dil)
    A = dev.conv_bf16_prepare_kernels(g["kern"], dev.empty((Cn, k * k * round8(Fn)), U16), Fn, Cn, k, True)
    mine = Out(dev, (B, Cn, h, w))
    dev.conv2d_gathered_bf16(A, Cn, P, B, hp, wp, round8(Fn), k, 1, h, w, mine.ptr)
    dev.sync()
    assert np.array_equal(mine.read().view(U32), dx.view(U32))
    # weight gradient: the materialised operands made on the host, bla_gemm_bf16 nt
    n, n8 = B * ho * wo, round8(B * ho * wo)
    cols = im2col(d["x"], k, s)
    G = np.zeros((Cn * k * k, n8), U16)
    G[:, :n] = dev.to_bf16(cols.transpose(2, 0, 1).reshape(Cn * k * k, n))
    dy16 = np.zeros((Fn, n8), U16)
    dy16[:, :n] = dev.to_bf16(d["dy"].reshape(B, Fn, ho * wo).transpose(1, 0, 2).reshape(Fn, n))
    mine = dev.empty((Fn, Cn * k * k)).fill_bytes(0xFF)
    dev.gemm_bf16(dev.to_device(dy16, U16), dev.to_device(G, U16), mine, transb=True)
    dev.sync()
    assert last_name(dev).startswith("gemm_bf16_mfma128x128x64_nt_f32")
    assert np.array_equal(mine.numpy().reshape(dk.shape).view(U32), dk.view(U32))
    # either output NULL: the other is what the full call gives, and the kernel named last is that gradient's
    only_dk, only_dx = Out(dev, dk.shape), Out(dev, dx.shape)
    call(dev, "bla_conv2d_backward_batched_f32_as_bf16", p(g["dy"]), p(g["x"]), p(g["kern"]), only_dk.ptr, None, B, h, w, k, Cn, Fn, s)
    assert last_name(dev).startswith("gemm_bf16_mfma128x128x64_nt_f32")
    call(dev, "bla_conv2d_backward_batched_f32_as_bf16", p(g["dy"]), None, p(g["kern"]), None, only_dx.ptr, B, h, w, k, Cn, Fn, s)
    assert last_name(dev) == "conv_bf16_gather128x128x64_s1"
    assert np.array_equal(only_dk.read().view(U32), dk.view(U32)) and np.array_equal(only_dx.read().view(U32), dx.view(U32))
    dev.conv2d_backward_as_bf16(g["dy"], g["x"], g["kern"], None, None, B, h, w, k, Cn, Fn, s)      # nothing to do


def test_bias_epilogue_and_plain_product(dev):
    """ep_bias_stride != rows against the same product without a bias: the difference is the one fp32 add"""
    case = CASES[1]
    B, Cn, Fn, h, w, k, s = case
    ho, wo = same_geometry(h, w, k, s)[:2]
    d = case_data(dev, case, "rounded")
    g = d["dev"]
    plain, biased = Out(dev, (B, Fn, ho, wo)), Out(dev, (B, Fn, ho, wo))
    call(dev, "bla_conv2d_forward_batched_f32_as_bf16", p(g["x"]), p(g["kern"]), plain.ptr, B, h, w, k, Cn, Fn, s, None, 0)
    call(dev, "bla_conv2d_forward_batched_f32_as_bf16", p(g["x"]), p(g["kern"]), biased.ptr, B, h, w, k, Cn, Fn, s, p(g["bias"]), Fn + 3)
    want = (plain.read() + d["bias"][:, :Fn, None, None]).astype(F32)
    assert np.array_equal(biased.read().view(U32), want.view(U32))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_argument_refusals_leave_the_outputs_alone(dev):
    B, Cn, Fn, h, w, k = 2, 8, 8, 6, 6, 3
    x, kern, dy = dev.zeros((B, Cn, h, w)), dev.zeros((Fn, Cn, k, k)), dev.zeros((B, Fn, h, w))
    P, A = dev.zeros((B, h + 2, w + 2, 8), U16), dev.zeros((Fn, k * k * 8), U16)
    out, dx, dk, p16 = Out(dev, (B, Fn, h, w)), Out(dev, (B, Cn, h, w)), Out(dev, (Fn, Cn, k, k)), Out(dev, (B, h + 2, w + 2, 8), U16)
    G = "bla_conv2d_gathered_bf16"
    call(dev, G, p(A), Fn, p(P), B, h + 2, w + 2, 12, k, 1, h, w, out.ptr, None, 0, want=1)          # cp % 8
    call(dev, G, p(A), Fn, p(P), B, h + 2, w + 2, 8, k, 0, h, w, out.ptr, None, 0, want=1)           # stride < 1
    call(dev, G, p(A), 0, p(P), B, h + 2, w + 2, 8, k, 1, h, w, out.ptr, None, 0, want=1)            # rows <= 0
    call(dev, G, None, Fn, p(P), B, h + 2, w + 2, 8, k, 1, h, w, out.ptr, None, 0, want=1)           # NULL operand
    call(dev, G, p(A), Fn, p(P), B, h + 2, w + 2, 8, k, 1, h + 1, w, out.ptr, None, 0, want=1)       # taps past the padded map
    call(dev, G, p(A), Fn, p(P), B, h + 2, w + 2, 8, k, 2, h, w, out.ptr, None, 0, want=1)           # the same through the stride
    call(dev, G, p(A) + 2, Fn, p(P), B, h + 2, w + 2, 8, k, 1, h, w, out.ptr, None, 0, want=1)       # off alignment
    call(dev, "bla_conv2d_forward_batched_f32_as_bf16", p(x), p(kern), out.ptr, B, h, w, k, Cn, Fn, 0, None, 0, want=1)
    call(dev, "bla_conv2d_forward_batched_f32_as_bf16", p(x), None, out.ptr, B, h, w, k, Cn, Fn, 1, None, 0, want=1)
    call(dev, "bla_conv2d_backward_batched_f32_as_bf16", p(dy), None, p(kern), dk.ptr, dx.ptr, B, h, w, k, Cn, Fn, 1, want=1)    # weight gradient without x
    call(dev, "bla_conv2d_backward_batched_f32_as_bf16", p(dy), p(x), None, dk.ptr, dx.ptr, B, h, w, k, Cn, Fn, 1, want=1)       # data gradient without kernels
    call(dev, "bla_conv2d_backward_batched_f32_as_bf16", p(dy), p(x), p(kern), dk.ptr, dx.ptr, 0, h, w, k, Cn, Fn, 1, want=1)
    call(dev, "bla_conv_bf16_pad", p(x), p16.ptr, B, Cn, h, w, h + 2, w + 2, 3, 1, 1, want=1)         # the map does not fit
    call(dev, "bla_conv_bf16_pad", p(x), p16.ptr, B, Cn, h, w, h + 2, w + 2, 1, 1, 0, want=1)         # dilation < 1
    call(dev, "bla_conv_bf16_prepare_kernels", p(kern), p16.ptr, Fn, 0, k, 0, want=1)
    assert out.untouched() and dx.untouched() and dk.untouched() and p16.untouched()


def test_strict_reference_refuses_the_dilated_data_gradient():
    """BLA_STRICT_REFERENCE=1 (read once per process): the data gradient at stride != 1 answers BLA_ERR_UNDEFINED (5) and writes nothing, also not the
    weight gradient asked for in the same call; stride 1, and the weight gradient alone at stride 2, run."""
    import os, subprocess, sys
    from conftest import ROOT
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from __graft_entry__ import load_pkg\n"
            "import numpy as np\n"
            "d = load_pkg(); d.init(0); L = d.lib(); z = d.zeros((4096,)); dk = d.empty((4096,)).fill_bytes(0xFF); dx = d.empty((4096,)).fill_bytes(0xFF)\n"
            "f = L.bla_conv2d_backward_batched_f32_as_bf16\n"
            "r = [f(None, z.ptr, z.ptr, z.ptr, dk.ptr, dx.ptr, 2, 8, 8, 3, 8, 8, 2)]\n"
            "d.sync(); r.append(bool(np.isnan(dk.numpy()).all() and np.isnan(dx.numpy()).all()))\n"
            "r += [f(None, z.ptr, z.ptr, z.ptr, dk.ptr, None, 2, 8, 8, 3, 8, 8, 2), f(None, z.ptr, z.ptr, z.ptr, dk.ptr, dx.ptr, 2, 8, 8, 3, 8, 8, 1)]\n"
            "d.sync(); print(r)\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, BLA_STRICT_REFERENCE="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "[5, True, 0, 0]", r.stdout + r.stderr
