"""bla_gemm_bf16_splitk on the device: the K-split of the fast bf16 product and its fixed-order fold (include/bla.h).

* Exact on integers, no tolerance: operands in -4..4 (exact in bf16), k <= 1024, so every partial sum is an integer below 2^24 and the split product
  must equal bla_gemm_bf16 on the same call -- and the integer product -- bit for bit, in every layout; the kernel's name carries _tcopyX as before and
  _splitk<S_eff> with S_eff from the partition rule, restated here:  slabs = ceil(k / 64), S clamped to [1, slabs], sps = ceil(slabs / S),
  S_eff = ceil(slabs / sps).
* The epilogue runs in the fold: alpha 0.5, integer biases, beta 2 on an integer C0, ReLU -- exact arithmetic -- into a fp32 and into a bf16 C.
* S_eff = 1 and calls off the fast path are bla_gemm_bf16's own launch: same bits, same name.
* The partition and the fold order, pinned: the split product equals the numpy float32 sum, in split order, of S_eff separate bla_gemm_bf16 products
  on the K sub-ranges (operand pointers advanced by s sps 64 elements: still 16-byte aligned, so each is the same slab sequence on the fast path).
* Rounded data against float64, the bound of the unsplit product unchanged, per element, no element left out:
      |got - ref| <= (k + 8) 2^-23 |alpha| (|A|.|B|) + 2 2^-24 (|bias_row| + |bias_col| + |beta C0| + |ref|)
  A partial over k_s terms errs by at most (k_s - 1) 2^-23 sum_s |ab|; the fold's S - 1 adds err by at most 2^-24 each of a running sum of at most about
  sum |ab|; for S >= 2 every split is non-empty, so max k_s <= k - 64 (S - 2) - 8 and the total is inside (k + 8) 2^-23 sum |ab|.  The worst ratio is
  printed.  Each such case runs again after a different split product has used the workspace and must give the same bits.
* splits = -1 and the epilogue fields the product does not honour: BLA_ERR_INVALID, C untouched.
Every C is a window at a padded pitch in an image of 0xFF bytes with 64 guard elements behind it; everything outside the window keeps its bits.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F32, F64, U16, U32 = np.float32, np.float64, np.uint16, np.uint32
GUARD = 64
LAYOUTS = ["nn", "nt", "tn", "tt"]
FAST, GENERAL = "gemm_bf16_mfma128x128x64_", "gemm_bf16_general_"
#              m    n    k    S
EXACT_CASES = [(128, 128, 128, 2), (129, 127, 1000, 2), (129, 127, 1000, 3), (129, 127, 1000, 5), (129, 127, 1000, 16),
               (127, 129, 72, 2),            # the second split is a single 8-deep chunk
               (289, 161, 1024, 7), (1, 1, 8, 4),
               (1153, 129, 192, 3)]          # 10 x 2 tiles: the tile order's groups of 8 and of 2 tile rows, ragged both ways


@pytest.fixture(scope="module")
def dev(pkg):
    pkg.init(0)
    return pkg


def partition(k, splits):
    slabs = -(-k // 64)
    s = min(max(splits, 1), slabs)
    sps = -(-slabs // s)
    return -(-slabs // sps), sps


class Buf:
    """A rows x cols window at pitch ld, `off` elements behind the allocation's (256-byte aligned) base, 64 guard elements behind it.  The whole image
    starts as `fill` bytes with `window` laid over the window; read() returns the window and sets outside_ok: everything else still holds its bits."""

    def __init__(self, dev, rows, cols, ld, dtype, off=0, window=None, fill=0xFF):
        self.rows, self.cols, self.ld, self.off, self.dtype = rows, cols, ld, off, np.dtype(dtype)
        self.count = off + rows * ld + GUARD
        bits = {2: U16, 4: U32}[self.dtype.itemsize]
        self.image = np.full(self.count, fill * (0x0101 if bits is U16 else 0x01010101), bits)
        if window is not None:
            body = self.image[off:off + rows * ld].reshape(rows, ld)
            body[:, :cols] = np.ascontiguousarray(window, self.dtype).view(bits)
        self.arr = dev.DeviceArray((self.count,), bits).copy_from(self.image)
        self.ptr = self.arr.ptr + off * self.dtype.itemsize

    def read(self):
        now = self.arr.numpy()
        body = now[self.off:self.off + self.rows * self.ld].reshape(self.rows, self.ld)
        mask = np.ones(self.count, bool)
        mask[self.off:self.off + self.rows * self.ld].reshape(self.rows, self.ld)[:, :self.cols] = False
        self.outside_ok = np.array_equal(now[mask], self.image[mask])
        return body[:, :self.cols].copy().view(self.dtype)

    def reset(self):
        self.arr.copy_from(self.image)

    def untouched(self):
        return np.array_equal(self.arr.numpy(), self.image)


def last_name(dev):
    return dev.lib().bla_gemm_last_kernel().decode()


def round8(x):
    return -(-x // 8) * 8


def operand_bufs(dev, lay, a_op16, b_op16, pad="round8", off_a=0, off_b=0):
    """op(A) [m][k] and op(B) [k][n] as bf16 patterns -> device buffers in the layout's storage order; round8: a pitch that is a multiple of 8"""
    sa = np.ascontiguousarray(a_op16.T if lay[0] == "t" else a_op16)
    sb = np.ascontiguousarray(b_op16.T if lay[1] == "t" else b_op16)
    ld = (lambda cols: round8(cols) + 8) if pad == "round8" else (lambda cols: cols + pad)
    A = Buf(dev, sa.shape[0], sa.shape[1], ld(sa.shape[1]), U16, off=off_a, window=sa, fill=0x3C)
    B = Buf(dev, sb.shape[0], sb.shape[1], ld(sb.shape[1]), U16, off=off_b, window=sb, fill=0x3C)
    return A, B


def run(dev, lay, m, n, k, A, B, Cb, ep=None, splits=None, want=0, a_ptr=None, b_ptr=None):
    """splits None: bla_gemm_bf16; else bla_gemm_bf16_splitk.  Returns the kernel's name."""
    L = dev.lib()
    c_type = dev.C_BF16 if Cb.dtype == U16 else dev.C_F32
    args = [None, int(lay[0] == "t"), int(lay[1] == "t"), m, n, k, a_ptr or A.ptr, A.ld, b_ptr or B.ptr, B.ld, Cb.ptr, Cb.ld, c_type,
            C.byref(ep) if ep is not None else None]
    st = L.bla_gemm_bf16(*args) if splits is None else L.bla_gemm_bf16_splitk(*args, splits)
    assert st == want, (st, L.bla_last_error())
    dev.sync()
    return last_name(dev)


def expected_name(lay, k, splits, out="f32"):
    eff = partition(k, splits)[0]
    return FAST + lay + "_" + out + ("_tcopyA" if lay[0] == "t" else "") + ("_tcopyB" if lay[1] == "n" else "") + ("_splitk%d" % eff if eff > 1 else "")


# ---- operands, made once -------------------------------------------------------------------------------------------------------------------------------
_cache = {}


def int_case(dev, m, n, k):
    key = ("int", m, n, k)
    if key not in _cache:
        rng = np.random.default_rng(m * 7 + n * 3 + k)
        a = rng.integers(-4, 5, (m, k)).astype(F32)
        b = rng.integers(-4, 5, (k, n)).astype(F32)
        assert np.abs(a).astype(F64).sum(1).max() * 4 < 2 ** 24                  # every partial sum, in any order
        _cache[key] = (dev.to_bf16(a), dev.to_bf16(b), (a.astype(F64) @ b.astype(F64)).astype(F32))
    return _cache[key]


def rounded_case(dev, m, n, k):
    """uniform [-1, 1) rounded to bf16: (a [m][k], b [k][n]) as float32, the float64 product and |a|.|b|"""
    key = ("rounded", m, n, k)
    if key not in _cache:
        rng = np.random.default_rng(m + 3 * n + 5 * k)
        a = dev.from_bf16(dev.to_bf16(rng.uniform(-1, 1, (m, k)).astype(F32)))
        b = dev.from_bf16(dev.to_bf16(rng.uniform(-1, 1, (k, n)).astype(F32)))
        _cache[key] = (a, b, a.astype(F64) @ b.astype(F64), np.abs(a).astype(F64) @ np.abs(b).astype(F64))
    return _cache[key]


# ---- exact on integers --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", LAYOUTS)
@pytest.mark.parametrize("m,n,k,splits", EXACT_CASES, ids=["%dx%dx%d_S%d" % c for c in EXACT_CASES])
def test_exact_on_integers(dev, m, n, k, splits, lay):
    a16, b16, ref = int_case(dev, m, n, k)
    A, B = operand_bufs(dev, lay, a16, b16)
    plain, split = Buf(dev, m, n, n + 8, F32), Buf(dev, m, n, n + 8, F32)
    name_plain = run(dev, lay, m, n, k, A, B, plain)
    name = run(dev, lay, m, n, k, A, B, split, splits=splits)
    assert name_plain == expected_name(lay, k, 1) and name == expected_name(lay, k, splits), (name_plain, name)
    got, want = split.read(), plain.read()
    assert split.outside_ok and plain.outside_ok
    assert np.array_equal(got.view(U32), want.view(U32)), f"{name}: {int((got.view(U32) != want.view(U32)).sum())} elements differ from bla_gemm_bf16"
    assert np.array_equal(got.view(U32), ref.view(U32))


@pytest.mark.parametrize("lay", ["nt", "tn"])
def test_epilogue_through_the_fold(dev, lay):
    """alpha 0.5 on an integer, integer biases, ReLU, 2 x an integer C0: every step exact in fp32; C0 in -4..4 is exact in bf16 too."""
    m, n, k, splits = 129, 127, 1000, 3
    a16, b16, prod = int_case(dev, m, n, k)
    rng = np.random.default_rng(77)
    br, bc = rng.integers(-9, 10, m).astype(F32), rng.integers(-9, 10, n).astype(F32)
    c0 = rng.integers(-4, 5, (m, n)).astype(F32)
    want = (np.maximum(0.5 * prod.astype(F64) + br[:, None] + bc[None, :], 0) + 2 * c0).astype(F32)
    d_br, d_bc = dev.to_device(br), dev.to_device(bc)
    ep = dev.Epilogue(alpha=0.5, beta=2.0, bias_row=d_br.ptr, bias_col=d_bc.ptr, act=dev.ACT_RELU)
    A, B = operand_bufs(dev, lay, a16, b16)
    got = {}
    for out in (F32, U16):
        window = dev.to_bf16(c0) if out == U16 else c0
        plain, split = Buf(dev, m, n, n + 8, out, window=window), Buf(dev, m, n, n + 8, out, window=window)
        run(dev, lay, m, n, k, A, B, plain, ep)
        name = run(dev, lay, m, n, k, A, B, split, ep, splits=splits)
        assert name == expected_name(lay, k, splits, "bf16" if out == U16 else "f32"), name
        got[out], ref = split.read(), plain.read()
        assert split.outside_ok and plain.outside_ok
        assert np.array_equal(got[out].view(U32 if out == F32 else U16), ref.view(U32 if out == F32 else U16))
    assert np.array_equal(got[F32].view(U32), want.view(U32))
    assert np.array_equal(got[U16], dev.to_bf16(got[F32]))


# ---- S_eff = 1 and the general path: bla_gemm_bf16's own launch -----------------------------------------------------------------------------------------
SAME_LAUNCH = {                       # m, n, k, splits, pad, off_a, path
    "explicit_S1": (129, 127, 1000, 1, "round8", 0, FAST),
    "k8_S4": (127, 129, 8, 4, "round8", 0, FAST),
    "odd_k_S4": (129, 127, 1001, 4, "round8", 0, GENERAL),
    "off_alignment_S4": (129, 127, 1000, 4, "round8", 1, GENERAL),
    "odd_pitch_S0": (129, 127, 1000, 0, 3, 0, GENERAL),
}


@pytest.mark.parametrize("lay", ["nt", "nn"])
@pytest.mark.parametrize("case", list(SAME_LAUNCH))
def test_one_split_and_the_general_path_are_the_unsplit_launch(dev, case, lay):
    m, n, k, splits, pad, off_a, path = SAME_LAUNCH[case]
    a, b, _, _ = rounded_case(dev, m, n, k)
    A, B = operand_bufs(dev, lay, dev.to_bf16(a), dev.to_bf16(b), pad=pad, off_a=off_a)
    plain, split = Buf(dev, m, n, n + 8, F32), Buf(dev, m, n, n + 8, F32)
    name_plain = run(dev, lay, m, n, k, A, B, plain)
    name = run(dev, lay, m, n, k, A, B, split, splits=splits)
    assert name == name_plain and name.startswith(path + lay) and "_splitk" not in name, (name_plain, name)
    assert np.array_equal(split.read().view(U32), plain.read().view(U32)) and split.outside_ok and not np.isnan(split.read()).any()


# ---- the partition and the fold order, pinned ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splits", [3, 16])
def test_split_product_is_the_ordered_sum_of_the_sub_range_products(dev, splits):
    m, n, k = 129, 127, 1000
    a, b, _, _ = rounded_case(dev, m, n, k)
    A, B = operand_bufs(dev, "nt", dev.to_bf16(a), dev.to_bf16(b))
    eff, sps = partition(k, splits)
    assert (eff, sps) == {3: (3, 6), 16: (16, 1)}[splits]
    acc = None
    for s in range(eff):
        k0 = s * sps * 64
        k1 = min(k, k0 + sps * 64)
        part = Buf(dev, m, n, n + 8, F32)
        name = run(dev, "nt", m, n, k1 - k0, A, B, part, a_ptr=A.ptr + 2 * k0, b_ptr=B.ptr + 2 * k0)
        assert name == FAST + "nt_f32", name                                   # the offset keeps the alignment: the same slab sequence
        p = part.read()
        acc = p if acc is None else (acc + p).astype(F32)
    split = Buf(dev, m, n, n + 8, F32)
    name = run(dev, "nt", m, n, k, A, B, split, splits=splits)
    assert name == FAST + "nt_f32_splitk%d" % eff, name
    got = split.read()
    assert split.outside_ok
    assert np.array_equal(got.view(U32), acc.view(U32)), f"{name}: {int((got.view(U32) != acc.view(U32)).sum())} elements differ from the ordered sum"


# ---- rounded data against float64; reproducible ---------------------------------------------------------------------------------------------------------
TOLERANCE_CASES = [(289, 161, 1024, 7, lay) for lay in LAYOUTS] + [(129, 127, 1000, 3, "nt")]


@pytest.mark.parametrize("m,n,k,splits,lay", TOLERANCE_CASES, ids=["%dx%dx%d_S%d_%s" % c for c in TOLERANCE_CASES])
def test_rounded_data_inside_the_unsplit_bound_and_reproducible(dev, m, n, k, splits, lay):
    a, b, prod, absprod = rounded_case(dev, m, n, k)
    rng = np.random.default_rng(k + splits)
    br, bc = rng.uniform(-1, 1, m).astype(F32), rng.uniform(-1, 1, n).astype(F32)
    c0 = dev.from_bf16(dev.to_bf16(rng.uniform(-1, 1, (m, n)).astype(F32)))
    alpha, beta = 0.5, 0.75
    d_br, d_bc = dev.to_device(br), dev.to_device(bc)
    ep = dev.Epilogue(alpha=alpha, beta=beta, bias_row=d_br.ptr, bias_col=d_bc.ptr, act=dev.ACT_RELU)
    A, B = operand_bufs(dev, lay, dev.to_bf16(a), dev.to_bf16(b))
    Cb = Buf(dev, m, n, n + 8, F32, window=c0)
    name = run(dev, lay, m, n, k, A, B, Cb, ep, splits=splits)
    assert name == expected_name(lay, k, splits), name
    got = Cb.read()
    assert Cb.outside_ok
    ref = np.maximum(alpha * prod + br.astype(F64)[:, None] + bc.astype(F64)[None, :], 0) + beta * c0.astype(F64)
    bound = (k + 8) * 2.0 ** -23 * abs(alpha) * absprod + 2 * 2.0 ** -24 * (
        np.abs(br.astype(F64))[:, None] + np.abs(bc.astype(F64))[None, :] + np.abs(beta * c0.astype(F64)) + np.abs(ref))
    err = np.abs(got.astype(F64) - ref)                     # an element left at the NaN pattern fails the comparison
    ratio = float(np.nanmax(err / bound))
    print(f"{name} {m}x{n}x{k}: worst |got - ref| / bound = {ratio:.4f}")
    assert (err <= bound).all(), f"{name}: worst ratio {ratio:.3f}, unwritten {int(np.isnan(err).sum())}"
    # another split product (other shape, other split count) writes its partial tiles over these; then the same call again
    oa16, ob16, oref = int_case(dev, 289, 161, 1024)
    OA, OB = operand_bufs(dev, "nt", oa16, ob16)
    other = Buf(dev, 289, 161, 161 + 8, F32)
    run(dev, "nt", 289, 161, 1024, OA, OB, other, splits=5)
    assert np.array_equal(other.read().view(U32), oref.view(U32))
    Cb.reset()
    run(dev, lay, m, n, k, A, B, Cb, ep, splits=splits)
    assert np.array_equal(Cb.read().view(U32), got.view(U32)) and Cb.outside_ok


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------------
REFUSED = [("pre_act", "ptr"), ("ld_pre", 8), ("relu_mask", "ptr"), ("ld_mask", 8), ("row_sum_a", "ptr"), ("softmax_y", "ptr"), ("softmax_scale", 1.0),
           ("softmax_grad", "ptr"), ("row_sum_alpha", 1.0), ("row_sum_beta", 1.0), ("softmax_loss_acc", "ptr"), ("softmax_correct_acc", "ptr"), ("act", 2)]


def test_refusals_leave_c_alone(dev):
    m, n, k = 16, 24, 256
    a16, b16, _ = int_case(dev, m, n, k)
    A, B = operand_bufs(dev, "nt", a16, b16)
    scratch = dev.zeros((m * n,), np.float64)
    for out in (F32, U16):
        Cb = Buf(dev, m, n, n + 8, out)
        run(dev, "nt", m, n, k, A, B, Cb, splits=-1, want=1)
        assert b"splits" in dev.lib().bla_last_error()
        for field, value in REFUSED:
            ep = dev.Epilogue(alpha=1.0)
            setattr(ep, field, scratch.ptr if value == "ptr" else value)
            run(dev, "nt", m, n, k, A, B, Cb, ep, splits=2, want=1)
        assert Cb.untouched()


def test_python_helpers(dev):
    m, n, k = 64, 40, 192
    a16, b16, ref = int_case(dev, m, n, k)
    c = dev.gemm_bf16_splitk(dev.to_device(a16, U16), dev.to_device(b16, U16), dev.empty((m, n)), splits=2)
    assert np.array_equal(c.numpy(), ref) and last_name(dev) == FAST + "nn_f32_tcopyB_splitk2"
    # splits = 0, the default: the automatic choice depends on the device's CU count, the integer result does not
    c = dev.gemm_bf16_splitk(dev.to_device(a16, U16), dev.to_device(np.ascontiguousarray(b16.T), U16), dev.empty((m, n)), transb=True)
    assert np.array_equal(c.numpy(), ref) and last_name(dev).startswith(FAST + "nt_f32")
    assert dev.gemm_bf16_splitk_plan(m, n, k, 3) == (3, 1, 3 * 65536)
