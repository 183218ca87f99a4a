"""bla_gemm_bf16 (bf16 operands, fp32 accumulation), its conversions and bla_gemm_f32_as_bf16 on the device.

* Conversions and the 16-bit transpose: bit-equal to the host restatement; pitch padding and 64 guard elements behind every buffer keep their bits.
* Exactness, no tolerance: operands are integers in -4..4 (exact in bf16) and k <= 1024, so every partial sum is an integer below 2^24 in any order and
  under any rounding; C (fp32) must equal the integer product bit for bit, on the fast path (which must be the path reported for aligned calls, all four
  layouts) and on the general path, reached three ways (k = 1001, an operand one element off alignment, a pitch padded by 3).
* Rounded data against float64: operands uniform [-1, 1) rounded to bf16 on the host, reference = float64 product of the same rounded values,
      |got - ref| <= (k + 8) 2^-23 |alpha| (|A|.|B|) + 2 2^-24 (|bias_row| + |bias_col| + |beta C0| + |ref|)
  (products of bf16 values are exact in fp32, so only the k fp32 adds err: at most (k - 1) 2^-23 sum |ab| in any order and rounding mode; the second term
  is the epilogue's roundings, as in test_conv_paths_gpu.py).  The worst ratio to the bound is printed per path.
* bf16 output = RNE of the fp32 output of the same call, bit for bit.
* bla_gemm_f32_as_bf16 = bla_f32_to_bf16 x 2 + bla_gemm_bf16, bit for bit.
* Every epilogue field the product does not honour is refused and leaves C alone.
Outputs start as the 0xFF byte pattern; a second run is bit-identical.
"""
import ctypes as C

import numpy as np
import pytest

from inputs import uniform

pytestmark = pytest.mark.gpu
F32, F64, U16, U32 = np.float32, np.float64, np.uint16, np.uint32
GUARD = 64
LAYOUTS = ["nn", "nt", "tn", "tt"]
EXACT_SHAPES = [(1, 1, 8), (127, 129, 72), (128, 128, 64), (129, 127, 1000), (289, 161, 1024), (384, 640, 128), (768, 768, 256),
                (1153, 129, 64)]             # 10 x 2 tiles: the tile order's groups of 8 and of 2 tile rows, ragged both ways
FAST, GENERAL = "gemm_bf16_mfma128x128x64_", "gemm_bf16_general_"


@pytest.fixture(scope="module")
def dev(pkg):
    pkg.init(0)
    return pkg


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


def last_name(dev):
    return dev.lib().bla_gemm_last_kernel().decode()


def stored(op, trans):
    """op(X) -> X as stored."""
    return np.ascontiguousarray(op.T if trans else op)


def run_bf16(dev, lay, m, n, k, a_buf, b_buf, c_buf, ep=None, want=0):
    c_type = dev.C_BF16 if c_buf.dtype == U16 else dev.C_F32
    st = dev.lib().bla_gemm_bf16(None, int(lay[0] == "t"), int(lay[1] == "t"), m, n, k, a_buf.ptr, a_buf.ld, b_buf.ptr, b_buf.ld, c_buf.ptr, c_buf.ld,
                                 c_type, C.byref(ep) if ep is not None else None)
    assert st == want, (st, dev.lib().bla_last_error())
    dev.sync()


def operand_bufs(dev, lay, a_op16, b_op16, pad=8, off_a=0, off_b=0):
    """op(A) [m][k] and op(B) [k][n] as uint16 bf16 patterns -> device buffers in the layout's storage order."""
    sa, sb = stored(a_op16, lay[0] == "t"), stored(b_op16, lay[1] == "t")
    ld = (lambda cols: -(-cols // 8) * 8 + 8) if pad == "round8" else (lambda cols: cols + pad)      # round8: the next multiple of 8, then 8 more
    A = Buf(dev, sa.shape[0], sa.shape[1], ld(sa.shape[1]), U16, off=off_a, window=sa, fill=0x3C)
    B = Buf(dev, sb.shape[0], sb.shape[1], ld(sb.shape[1]), U16, off=off_b, window=sb, fill=0x3C)
    return A, B


def takes_fast_path(A, B, k):
    """The dispatch rule of include/bla.h."""
    return k > 0 and k % 8 == 0 and A.ptr % 16 == 0 and B.ptr % 16 == 0 and A.ld % 8 == 0 and B.ld % 8 == 0


# ---- conversions -------------------------------------------------------------------------------------------------------------------------------------
def test_conversions_edge_set(dev):
    from test_bf16_host import EDGE_BITS
    n = len(EDGE_BITS)
    src = Buf(dev, 1, n, n, F32, window=EDGE_BITS.view(F32)[None, :])
    dst = Buf(dev, 1, n, n, U16)
    assert dev.lib().bla_f32_to_bf16(None, src.ptr, n, dst.ptr, n, 1, n) == 0
    dev.sync()
    got = dst.read()[0]
    assert np.array_equal(got, dev.to_bf16(EDGE_BITS.view(F32))) and dst.outside_ok
    back = Buf(dev, 1, n, n, F32)
    assert dev.lib().bla_bf16_to_f32(None, dst.ptr, n, back.ptr, n, 1, n) == 0
    dev.sync()
    assert np.array_equal(back.read()[0].view(U32), got.astype(U32) << 16) and back.outside_ok


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off_by_one"])
def test_conversions_padded_window(dev, off):
    rows, cols = 37, 130
    bits = np.random.default_rng(5).integers(0, 2 ** 32, (rows, cols), dtype=np.uint64).astype(U32)
    src = Buf(dev, rows, cols, 136, F32, off=off, window=bits.view(F32))
    dst = Buf(dev, rows, cols, 144, U16, off=off)
    assert dev.lib().bla_f32_to_bf16(None, src.ptr, 136, dst.ptr, 144, rows, cols) == 0
    dev.sync()
    got = dst.read()
    assert np.array_equal(got, dev.to_bf16(bits.view(F32))) and dst.outside_ok
    h = np.random.default_rng(6).integers(0, 2 ** 16, (rows, cols)).astype(U16)
    src16 = Buf(dev, rows, cols, 136, U16, off=off, window=h)
    dst32 = Buf(dev, rows, cols, 144, F32, off=off)
    assert dev.lib().bla_bf16_to_f32(None, src16.ptr, 136, dst32.ptr, 144, rows, cols) == 0
    dev.sync()
    assert np.array_equal(dst32.read().view(U32), h.astype(U32) << 16) and dst32.outside_ok


@pytest.mark.parametrize("pad", [8, 3, "round8"], ids=["pitch+8", "pitch+3", "pitch_multiple_of_8"])
@pytest.mark.parametrize("rows,cols", [(1, 1), (33, 65), (130, 257)])
def test_transpose_b16(dev, rows, cols, pad):
    """pitch+8 and pitch+3 leave odd pitches (2-byte accesses); a pitch that is a multiple of 8 takes the 16-byte accesses, edges included."""
    h = np.random.default_rng(rows).integers(0, 2 ** 16, (rows, cols)).astype(U16)
    ld = (lambda c: -(-c // 8) * 8 + 8) if pad == "round8" else (lambda c: c + pad)
    src = Buf(dev, rows, cols, ld(cols), U16, window=h)
    dst = Buf(dev, cols, rows, ld(rows), U16)
    assert dev.lib().bla_transpose_b16(None, src.ptr, src.ld, dst.ptr, dst.ld, rows, cols) == 0
    dev.sync()
    assert np.array_equal(dst.read(), h.T) and dst.outside_ok


# ---- exact integer products ------------------------------------------------------------------------------------------------------------------------
_int_cache = {}


def int_case(dev, m, n, k):
    if (m, n, k) not in _int_cache:
        rng = np.random.default_rng(m * 7 + n * 3 + k)
        a = rng.integers(-4, 5, (m, k)).astype(F32)
        b = rng.integers(-4, 5, (k, n)).astype(F32)
        ref = (a.astype(F64) @ b.astype(F64)).astype(F32)
        assert np.abs(a).astype(F64).sum(1).max() * 4 < 2 ** 24
        _int_cache[(m, n, k)] = (dev.to_bf16(a), dev.to_bf16(b), ref)
    return _int_cache[(m, n, k)]


def exact_run(dev, lay, m, n, k, want_prefix, pad=8, off_a=0, off_b=0):
    a16, b16, ref = int_case(dev, m, n, k)
    A, B = operand_bufs(dev, lay, a16, b16, pad=pad, off_a=off_a, off_b=off_b)
    Cb = Buf(dev, m, n, n + 8, F32)
    run_bf16(dev, lay, m, n, k, A, B, Cb)
    name = last_name(dev)
    if want_prefix is None:
        want_prefix = FAST if takes_fast_path(A, B, k) else GENERAL
    assert name.startswith(want_prefix + lay + "_f32"), name
    got = Cb.read()
    assert np.array_equal(got.view(U32), ref.view(U32)), f"{name}: {int((got != ref).sum())} elements differ"
    assert Cb.outside_ok
    Cb.reset()
    run_bf16(dev, lay, m, n, k, A, B, Cb)
    assert np.array_equal(Cb.read().view(U32), got.view(U32))
    return name


@pytest.mark.parametrize("lay", LAYOUTS)
@pytest.mark.parametrize("m,n,k", EXACT_SHAPES)
def test_exact_pitches_padded_by_8(dev, m, n, k, lay):
    """Every aligned nt case is on the fast path; another layout is there when its m- or n-long rows, padded by 8, still have a pitch that is a multiple of 8."""
    name = exact_run(dev, lay, m, n, k, FAST if lay == "nt" else None)
    if name.startswith(FAST):
        assert ("_tcopyA" in name) == (lay[0] == "t") and ("_tcopyB" in name) == (lay[1] == "n")


@pytest.mark.parametrize("lay", ["nn", "tn", "tt"])
@pytest.mark.parametrize("m,n,k", EXACT_SHAPES)
def test_exact_fast_path_through_the_transposed_copy(dev, m, n, k, lay):
    """Pitches rounded up to a multiple of 8 (and padded by 8 more): every layout takes the fast path, odd m and n included."""
    name = exact_run(dev, lay, m, n, k, FAST, pad="round8")
    assert ("_tcopyA" in name) == (lay[0] == "t") and ("_tcopyB" in name) == (lay[1] == "n")


@pytest.mark.parametrize("lay", LAYOUTS)
@pytest.mark.parametrize("m,n", [s[:2] for s in EXACT_SHAPES])
def test_exact_general_path_odd_k(dev, m, n, lay):
    exact_run(dev, lay, m, n, 1001, GENERAL)


@pytest.mark.parametrize("lay", LAYOUTS)
@pytest.mark.parametrize("which", ["a", "b"])
def test_exact_general_path_operand_off_alignment(dev, lay, which):
    exact_run(dev, lay, 129, 127, 1000, GENERAL, off_a=int(which == "a"), off_b=int(which == "b"))


@pytest.mark.parametrize("lay", LAYOUTS)
@pytest.mark.parametrize("m,n,k", [(127, 129, 72), (129, 127, 1000)])
def test_exact_general_path_odd_pitch(dev, m, n, k, lay):
    exact_run(dev, lay, m, n, k, GENERAL, pad=3)


# ---- rounded data against float64 ------------------------------------------------------------------------------------------------------------------
_worst = {}


def rounded_case(dev, lay, m, n, k, path, alpha=1.0, beta=0.0, bias_row=False, bias_col=False, relu=False, out=F32, seed=1):
    """Runs one product; returns (got fp32 view of the result, ref float64, bound, C buffer)."""
    a = dev.from_bf16(dev.to_bf16(uniform(seed, (m, k), dtype=F32)))
    b = dev.from_bf16(dev.to_bf16(uniform(seed + 1, (k, n), dtype=F32)))
    A, B = operand_bufs(dev, lay, dev.to_bf16(a), dev.to_bf16(b), pad=3 if path == "general_pitch" else "round8")
    br = uniform(seed + 2, (m,), dtype=F32) if bias_row else None
    bc = uniform(seed + 3, (n,), dtype=F32) if bias_col else None
    c0 = dev.from_bf16(dev.to_bf16(uniform(seed + 4, (m, n), dtype=F32))) if beta != 0 else None      # exact in either output type
    d_br = dev.to_device(br) if bias_row else None
    d_bc = dev.to_device(bc) if bias_col else None
    window = None if c0 is None else (dev.to_bf16(c0) if out == U16 else c0)
    Cb = Buf(dev, m, n, n + 8, out, window=window)
    ep = dev.Epilogue(alpha=alpha, beta=beta, bias_row=d_br.ptr if bias_row else None, bias_col=d_bc.ptr if bias_col else None,
                      act=dev.ACT_RELU if relu else dev.ACT_NONE)
    run_bf16(dev, lay, m, n, k, A, B, Cb, ep)
    name = last_name(dev)
    assert name.startswith((FAST if path == "fast" else GENERAL) + lay), name
    got = Cb.read()
    assert Cb.outside_ok
    ref = alpha * (a.astype(F64) @ b.astype(F64))
    zero = np.zeros(1)
    if bias_row:
        ref = ref + br.astype(F64)[:, None]
    if bias_col:
        ref = ref + bc.astype(F64)[None, :]
    if relu:
        ref = np.maximum(ref, 0)
    if beta != 0:
        ref = ref + beta * c0.astype(F64)
    absprod = np.abs(a).astype(F64) @ np.abs(b).astype(F64)
    bound = (k + 8) * 2.0 ** -23 * abs(alpha) * absprod + 2 * 2.0 ** -24 * (
        (np.abs(br.astype(F64))[:, None] if bias_row else zero) + (np.abs(bc.astype(F64))[None, :] if bias_col else zero) +
        (np.abs(beta * c0.astype(F64)) if beta != 0 else zero) + np.abs(ref))
    return got, ref, bound, name


def check_bound(got, ref, bound, name, path):
    err = np.abs(got.astype(F64) - ref)          # an element left at the NaN pattern fails the comparison
    ratio = float(np.nanmax(err / bound))
    key = "fast" if path == "fast" else "general"
    _worst[key] = max(_worst.get(key, 0.0), ratio)
    print(f"{name}: worst |got - ref| / bound = {ratio:.4f} (worst so far on the {key} path: {_worst[key]:.4f})")
    assert (err <= bound).all(), f"{name}: worst ratio {ratio:.3f}, unwritten {int(np.isnan(err).sum())}"


def shape_for(path):
    return (129, 127, 1001) if path == "general_k" else (129, 127, 1000)


EPILOGUES = {
    "alpha": dict(alpha=0.5),
    "beta": dict(beta=0.75),
    "bias_row": dict(bias_row=True),
    "bias_col": dict(bias_col=True),
    "relu": dict(relu=True),
    "all": dict(alpha=0.5, beta=0.75, bias_row=True, bias_col=True, relu=True),
}


@pytest.mark.parametrize("path", ["fast", "general_k", "general_pitch"])
@pytest.mark.parametrize("lay", LAYOUTS)
def test_rounded_every_layout_and_path(dev, lay, path):
    m, n, k = shape_for(path)
    got, ref, bound, name = rounded_case(dev, lay, m, n, k, path, **EPILOGUES["all"])
    check_bound(got, ref, bound, name, path)


@pytest.mark.parametrize("path,lay", [("fast", "nt"), ("fast", "tn"), ("general_k", "nn")])
@pytest.mark.parametrize("epi", [e for e in EPILOGUES if e != "all"])
def test_rounded_each_epilogue_field(dev, epi, path, lay):
    m, n, k = (127, 129, 72) if path == "fast" else (127, 129, 73)
    got, ref, bound, name = rounded_case(dev, lay, m, n, k, path, seed=11, **EPILOGUES[epi])
    check_bound(got, ref, bound, name, path)


@pytest.mark.parametrize("m,n,k", EXACT_SHAPES)
def test_rounded_edge_shapes(dev, m, n, k):
    got, ref, bound, name = rounded_case(dev, "nt", m, n, k, "fast", alpha=0.5, bias_row=True, seed=21)
    check_bound(got, ref, bound, name, "fast")


# ---- bf16 output: one rounding, after the whole epilogue ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["fast", "general_k"])
@pytest.mark.parametrize("lay", ["nt", "nn"])
@pytest.mark.parametrize("epi", ["alpha", "all"])
def test_bf16_output_is_the_rounded_fp32_output(dev, lay, path, epi):
    m, n, k = (129, 127, 136) if path == "fast" else (129, 127, 137)
    got32, _, _, _ = rounded_case(dev, lay, m, n, k, path, seed=31, out=F32, **EPILOGUES[epi])
    got16, _, _, name = rounded_case(dev, lay, m, n, k, path, seed=31, out=U16, **EPILOGUES[epi])
    assert name.endswith("bf16") or "_bf16_tcopy" in name, name
    assert np.array_equal(got16, dev.to_bf16(got32)), f"{name}: {int((got16 != dev.to_bf16(got32)).sum())} elements differ"


# ---- bla_gemm_f32_as_bf16 is the composition --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1000, 1001], ids=["fast", "general"])
@pytest.mark.parametrize("lay", LAYOUTS)
def test_f32_as_bf16_is_the_composition(dev, lay, k):
    m, n = 129, 127
    L = dev.lib()
    a = uniform(41, (m, k), dtype=F32)
    b = uniform(42, (k, n), dtype=F32)
    sa, sb = stored(a, lay[0] == "t"), stored(b, lay[1] == "t")
    A32 = Buf(dev, sa.shape[0], sa.shape[1], sa.shape[1] + 5, F32, window=sa, fill=0x3C)
    B32 = Buf(dev, sb.shape[0], sb.shape[1], sb.shape[1] + 5, F32, window=sb, fill=0x3C)
    br = dev.to_device(uniform(43, (m,), dtype=F32))
    ep = dev.Epilogue(alpha=0.5, bias_row=br.ptr, act=dev.ACT_RELU)
    ta, tb = int(lay[0] == "t"), int(lay[1] == "t")
    C1 = Buf(dev, m, n, n + 8, F32)
    assert L.bla_gemm_f32_as_bf16(None, ta, tb, m, n, k, A32.ptr, A32.ld, B32.ptr, B32.ld, C1.ptr, C1.ld, C.byref(ep)) == 0, L.bla_last_error()
    dev.sync()
    name1 = last_name(dev)
    assert name1.startswith((FAST if k % 8 == 0 else GENERAL) + lay + "_f32"), name1
    # the same by hand: both operands rounded into 16-byte aligned buffers at a pitch rounded up to 8, then the bf16 product
    lda, ldb = -(-sa.shape[1] // 8) * 8, -(-sb.shape[1] // 8) * 8
    A16 = Buf(dev, sa.shape[0], sa.shape[1], lda, U16)
    B16 = Buf(dev, sb.shape[0], sb.shape[1], ldb, U16)
    assert L.bla_f32_to_bf16(None, A32.ptr, A32.ld, A16.ptr, lda, sa.shape[0], sa.shape[1]) == 0
    assert L.bla_f32_to_bf16(None, B32.ptr, B32.ld, B16.ptr, ldb, sb.shape[0], sb.shape[1]) == 0
    C2 = Buf(dev, m, n, n + 8, F32)
    run_bf16(dev, lay, m, n, k, A16, B16, C2, ep)
    assert last_name(dev) == name1
    got1, got2 = C1.read(), C2.read()
    assert np.array_equal(got1.view(U32), got2.view(U32)) and C1.outside_ok and C2.outside_ok
    assert np.array_equal(A16.read(), dev.to_bf16(sa)) and A32.read() is not None and A32.outside_ok
    # and against float64 on the rounded operands
    ar, brd = dev.from_bf16(dev.to_bf16(a)).astype(F64), dev.from_bf16(dev.to_bf16(b)).astype(F64)
    bias = br.numpy().astype(F64)[:, None]
    ref = np.maximum(0.5 * (ar @ brd) + bias, 0)
    bound = (k + 8) * 2.0 ** -23 * 0.5 * (np.abs(ar) @ np.abs(brd)) + 2 * 2.0 ** -24 * (np.abs(bias) + np.abs(ref))
    check_bound(got1, ref, bound, name1 + " (from fp32)", "fast" if k % 8 == 0 else "general")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------
REFUSED = [("pre_act", "ptr"), ("ld_pre", 8), ("relu_mask", "ptr"), ("ld_mask", 8), ("row_sum_a", "ptr"), ("softmax_y", "ptr"), ("softmax_scale", 1.0),
           ("softmax_grad", "ptr"), ("row_sum_alpha", 1.0), ("row_sum_beta", 1.0), ("softmax_loss_acc", "ptr"), ("softmax_correct_acc", "ptr"), ("act", 2)]


@pytest.mark.parametrize("field,value", REFUSED, ids=[f for f, _ in REFUSED])
def test_unsupported_epilogue_fields_are_refused(dev, field, value):
    m, n, k = 16, 24, 32
    a16, b16, _ = int_case(dev, m, n, k)
    A, B = operand_bufs(dev, "nt", a16, b16)
    scratch = dev.zeros((m * n,), np.float64)
    L = dev.lib()
    for out in (F32, U16):
        Cb = Buf(dev, m, n, n + 8, out)
        ep = dev.Epilogue(alpha=1.0)
        setattr(ep, field, scratch.ptr if value == "ptr" else value)
        L.bla_gemm_set_config(-1, 0)
        before = last_name(dev)
        run_bf16(dev, "nt", m, n, k, A, B, Cb, ep, want=1)
        assert last_name(dev) == before
        Cb.read()
        assert Cb.outside_ok and np.array_equal(Cb.arr.numpy(), Cb.image)
    A32 = dev.to_device(np.ones((m, k), F32))
    B32 = dev.to_device(np.ones((n, k), F32))
    Cb = Buf(dev, m, n, n + 8, F32)
    assert L.bla_gemm_f32_as_bf16(None, 0, 1, m, n, k, A32.ptr, k, B32.ptr, k, Cb.ptr, Cb.ld, C.byref(ep)) == 1
    dev.sync()
    assert np.array_equal(Cb.arr.numpy(), Cb.image)


def test_python_helper(dev):
    m, n, k = 64, 40, 48
    a16, b16, ref = int_case(dev, m, n, k)
    c = dev.gemm_bf16(dev.to_device(a16, U16), dev.to_device(b16, U16), dev.empty((m, n)))
    assert np.array_equal(c.numpy(), ref) and last_name(dev).startswith(FAST + "nn_f32_tcopyB")
    c16 = dev.gemm_bf16(dev.to_device(a16, U16), dev.to_device(np.ascontiguousarray(b16.T), U16), dev.empty((m, n), U16), transb=True)
    assert np.array_equal(c16.numpy(), dev.to_bf16(ref)) and last_name(dev) == FAST + "nt_bf16"
