"""bla_f32_to_mxfp8 / bla_mxfp8_to_f32 / bla_gemm_mxfp8 / bla_gemm_f32_as_mxfp8 on the device (include/bla.h "MXFP8").

* Quantiser and dequantiser: bit-equal to the host restatement (native.to_mxfp8 / from_mxfp8, which test_mxfp8_host.py holds to torch), both trans forms,
  bases aligned and one element off, pitches that do and do not allow the wide accesses; pitch padding and 64 guard elements keep their bits.
* Exact product, no tolerance: elements are integers in -4 .. 4, scale bytes 125 .. 129 per block, both random.  Every product is a multiple of 2^-4 and
  with k <= 1024 every partial sum stays below 2^22 such units (|a| <= 16, |b| <= 16, k <= 1024: 2^18, in units of 2^-4), so the result is exact in fp32
  in any order and C must equal the float64 product bit for bit -- on the fast path (the path reported for aligned calls) and on the general path,
  reached three ways: an element base one byte off, a pitch padded by 3, a scale pitch of k / 32 + 1.
* One-hot A with a distinct scale per (row, block) against random integer B: C is a scaled copy of B^T, so a wrong lane, byte or opsel map fails with a
  readable pattern.  Scale range: +-1 elements under scale bytes 87 .. 167.  0xFF in the scale arrays' pitch padding must not reach C.
* Rounded data against float64 (test_mxfp8_host.py's cases, bound and derivation), the worst ratio printed per path.
* bf16 output = RNE of the same call's fp32 output; bla_gemm_f32_as_mxfp8 = quantise x 2 + bla_gemm_mxfp8, bit for bit, all four layouts; refusals
  leave C's bytes alone; a second run is bit-identical; the kernel names are those of include/bla.h.
"""
import ctypes as C

import numpy as np
import pytest

from inputs import uniform
from test_mxfp8_host import RANDOM_CASES, cached_case, edge_row, random_operand

pytestmark = pytest.mark.gpu
F32, F64, U8, U16, U32 = np.float32, np.float64, np.uint8, np.uint16, np.uint32
GUARD = 64
FAST, GENERAL = "gemm_mxfp8_mfma128x128x128_", "gemm_mxfp8_general_"
EXACT_SHAPES = [(1, 1, 32), (127, 129, 96), (128, 128, 128), (129, 127, 992), (289, 161, 1024), (384, 640, 256),
                (1153, 129, 128)]            # 10 x 2 tiles: the tile order's groups of 8 and of 2 tile rows, ragged both ways


@pytest.fixture(scope="module")
def dev(pkg):
    pkg.init(0)
    return pkg


class Buf:
    """test_bf16_gpu.py's Buf for 1-, 2- and 4-byte elements: a rows x cols window at pitch ld, `off` elements behind the allocation's (256-byte aligned)
    base, 64 guard elements behind it.  The whole image starts as `fill` bytes with `window` laid over the window; read() returns the window and sets
    outside_ok: everything else still holds its bits."""

    def __init__(self, dev, rows, cols, ld, dtype, off=0, window=None, fill=0xFF):
        self.rows, self.cols, self.ld, self.off, self.dtype = rows, cols, ld, off, np.dtype(dtype)
        self.count = off + rows * ld + GUARD
        bits = {1: U8, 2: U16, 4: U32}[self.dtype.itemsize]
        self.image = np.full(self.count, fill * {1: 0x01, 2: 0x0101, 4: 0x01010101}[self.dtype.itemsize], bits)
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

    def untouched(self):
        return np.array_equal(self.arr.numpy(), self.image)


def last_name(dev):
    return dev.lib().bla_gemm_last_kernel().decode()


def up(x, to):
    return -(-x // to) * to


# ---- quantiser and dequantiser ---------------------------------------------------------------------------------------------------------------------
def quantise_on_device(dev, v, trans, off=0, wide=True):
    """v [rows][cols] (the values; stored transposed for trans) -> device elements and scales, with the outside of both windows checked."""
    rows, cols = v.shape
    st = np.ascontiguousarray(v.T if trans else v)
    ld_src = up(st.shape[1], 4) + (4 if wide else 3)
    src = Buf(dev, st.shape[0], st.shape[1], ld_src, F32, off=off, window=st, fill=0x3C)
    kp, nb = up(cols, 32), -(-cols // 32)
    el = Buf(dev, rows, kp, kp + (16 if wide else 5), U8, off=off)
    sc = Buf(dev, rows, nb, nb + (4 if wide else 1), U8, off=off)
    stt = dev.lib().bla_f32_to_mxfp8(None, src.ptr, src.ld, int(trans), rows, cols, el.ptr, el.ld, sc.ptr, sc.ld)
    assert stt == 0, dev.lib().bla_last_error()
    dev.sync()
    got_el, got_sc = el.read(), sc.read()
    assert el.outside_ok and sc.outside_ok and src.untouched()
    return got_el, got_sc


@pytest.mark.parametrize("trans", [False, True], ids=["rows", "trans"])
def test_quantiser_edge_set(dev, trans):
    v = edge_row()
    got_el, got_sc = quantise_on_device(dev, v, trans)
    want_el, want_sc = dev.to_mxfp8(v)
    assert np.array_equal(got_sc, want_sc) and (want_sc == 127).all()
    assert np.array_equal(got_el, want_el), np.flatnonzero(got_el != want_el)[:8]


@pytest.mark.parametrize("wide", [True, False], ids=["wide_accesses", "narrow_accesses"])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off_by_one"])
@pytest.mark.parametrize("trans", [False, True], ids=["rows", "trans"])
@pytest.mark.parametrize("rows,cols", [(1, 32), (37, 130), (130, 257)])
def test_quantiser_matches_the_host_restatement(dev, rows, cols, trans, off, wide):
    """Random bit patterns with mild exponents, a few NaN / Inf / zero blocks and fp32 subnormals among them."""
    rng = np.random.default_rng(rows + cols)
    v = (rng.standard_normal((rows, cols)) * 2.0 ** rng.integers(-12, 12, (rows, cols))).astype(F32)
    flat = v.reshape(-1)
    flat[rng.integers(0, flat.size, 3)] = [np.nan, np.inf, -np.inf][:3]
    flat[rng.integers(0, flat.size, 2)] = np.array([1, 0x80000005], U32).view(F32)
    if cols > 64:
        v[0, 32:64] = 0
        v[rows - 1, :32] *= F32(2.0 ** 100)
    got_el, got_sc = quantise_on_device(dev, v, trans, off=off, wide=wide)
    want_el, want_sc = dev.to_mxfp8(v)
    assert np.array_equal(got_sc, want_sc), np.argwhere(got_sc != want_sc)[:8]
    assert np.array_equal(got_el, want_el), np.argwhere(got_el != want_el)[:8]


@pytest.mark.parametrize("wide", [True, False], ids=["wide_accesses", "narrow_accesses"])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "off_by_one"])
@pytest.mark.parametrize("rows,cols", [(1, 32), (37, 130), (130, 257)])
def test_dequantiser_matches_the_host_restatement(dev, rows, cols, off, wide):
    """Every element byte and every scale byte, NaNs included: the result is specified to the bit."""
    rng = np.random.default_rng(rows * 3 + cols)
    nb = -(-cols // 32)
    el = rng.integers(0, 256, (rows, cols)).astype(U8)
    sc = rng.integers(0, 256, (rows, nb)).astype(U8)
    sc[0, 0] = 0
    E = Buf(dev, rows, cols, up(cols, 4) + (4 if wide else 3), U8, off=off, window=el, fill=0x3C)
    S = Buf(dev, rows, nb, nb + (4 if wide else 1), U8, off=off, window=sc, fill=0x3C)
    D = Buf(dev, rows, cols, up(cols, 4) + (4 if wide else 3), F32, off=off)
    assert dev.lib().bla_mxfp8_to_f32(None, E.ptr, E.ld, S.ptr, S.ld, D.ptr, D.ld, rows, cols) == 0, dev.lib().bla_last_error()
    dev.sync()
    got = D.read()
    want = dev.from_mxfp8(el, sc)
    assert D.outside_ok and np.array_equal(got.view(U32), want.view(U32)), np.argwhere(got.view(U32) != want.view(U32))[:8]


# ---- the product ---------------------------------------------------------------------------------------------------------------------------------------
def operand_bufs(dev, el, sc, path="fast", fill=0x3C, scale_fill=0xFF):
    """elements [rows][k] and scales [rows][k / 32] -> device buffers on the asked path: fast (16-byte aligned bases, pitches of 16 and 4 bytes more than
    the rounded-up rows), or general by one of: base (elements one byte off), pitch (element pitch k + 3), scale_pitch (scale pitch k / 32 + 1)."""
    rows, k = el.shape
    nb = sc.shape[1]
    ld = k + 3 if path == "pitch" else up(k, 16) + 16
    ld_s = nb + 1 if path == "scale_pitch" else up(nb, 4) + 4
    E = Buf(dev, rows, k, ld, U8, off=1 if path == "base" else 0, window=el, fill=fill)
    S = Buf(dev, rows, nb, ld_s, U8, window=sc, fill=scale_fill)
    return E, S


def takes_fast_path(A, SA, B, SB, k):
    """The dispatch rule of include/bla.h."""
    return (k > 0 and A.ptr % 16 == 0 and B.ptr % 16 == 0 and A.ld % 16 == 0 and B.ld % 16 == 0 and SA.ptr % 4 == 0 and SB.ptr % 4 == 0 and
            SA.ld % 4 == 0 and SB.ld % 4 == 0)


def run_mx(dev, m, n, k, A, SA, B, SB, Cb, ep=None, want=0):
    c_type = dev.C_BF16 if Cb.dtype == U16 else dev.C_F32
    st = dev.lib().bla_gemm_mxfp8(None, m, n, k, A.ptr, A.ld, SA.ptr, SA.ld, B.ptr, B.ld, SB.ptr, SB.ld, Cb.ptr, Cb.ld, c_type, C.byref(ep) if ep is not None else None)
    assert st == want, (st, dev.lib().bla_last_error())
    dev.sync()


_int_cache = {}


def int_case(dev, m, n, k):
    if (m, n, k) not in _int_cache:
        rng = np.random.default_rng(m * 7 + n * 3 + k)
        ea, eb = dev.native.e4m3_round(rng.integers(-4, 5, (m, k)).astype(F32)), dev.native.e4m3_round(rng.integers(-4, 5, (n, k)).astype(F32))
        sa, sb = rng.integers(125, 130, (m, k // 32)).astype(U8), rng.integers(125, 130, (n, k // 32)).astype(U8)
        a, b = dev.from_mxfp8(ea, sa).astype(F64), dev.from_mxfp8(eb, sb).astype(F64)
        assert (np.abs(a).sum(1).max() * np.abs(b).max()) * 16 < 2 ** 24           # every partial sum, in units of 2^-4
        ref = (a @ b.T).astype(F32)
        assert np.array_equal(ref.astype(F64), a @ b.T)
        _int_cache[(m, n, k)] = (ea, sa, eb, sb, ref)
    return _int_cache[(m, n, k)]


def exact_run(dev, m, n, k, path):
    ea, sa, eb, sb, ref = int_case(dev, m, n, k)
    A, SA = operand_bufs(dev, ea, sa, path)
    B, SB = operand_bufs(dev, eb, sb, "fast" if path == "base" else path)            # base: A alone is off alignment
    Cb = Buf(dev, m, n, n + 8, F32)
    run_mx(dev, m, n, k, A, SA, B, SB, Cb)
    name = last_name(dev)
    assert name == (FAST if takes_fast_path(A, SA, B, SB, k) else GENERAL) + "f32", name
    assert takes_fast_path(A, SA, B, SB, k) == (path == "fast" or (path == "scale_pitch" and (k // 32 + 1) % 4 == 0))      # k = 96, 992: a pitch of k / 32 + 1 is a multiple of 4
    got = Cb.read()
    assert np.array_equal(got.view(U32), ref.view(U32)), f"{name}: {int((got != ref).sum())} elements differ, first at {np.argwhere(got != ref)[:4].tolist()}"
    assert Cb.outside_ok and A.untouched() and SA.untouched() and B.untouched() and SB.untouched()
    Cb.arr.copy_from(Cb.image)
    run_mx(dev, m, n, k, A, SA, B, SB, Cb)
    assert np.array_equal(Cb.read().view(U32), got.view(U32))            # a second run is bit-identical


@pytest.mark.parametrize("m,n,k", EXACT_SHAPES)
def test_exact_fast_path(dev, m, n, k):
    exact_run(dev, m, n, k, "fast")


@pytest.mark.parametrize("path", ["base", "pitch", "scale_pitch"])
@pytest.mark.parametrize("m,n,k", EXACT_SHAPES)
def test_exact_general_path(dev, m, n, k, path):
    exact_run(dev, m, n, k, path)


def test_one_hot_a_gives_a_scaled_copy_of_b(dev):
    m = n = k = 128
    rng = np.random.default_rng(5)
    ea = np.zeros((m, k), U8)
    ea[np.arange(m), np.arange(m)] = 0x38                                  # A[r][r] = 1
    sa = (120 + (np.arange(m)[:, None] * 4 + np.arange(4)[None, :]) % 15).astype(U8)      # distinct per (row, block) within any 3 neighbouring rows
    eb = dev.native.e4m3_round(rng.integers(-4, 5, (n, k)).astype(F32))
    eb[eb == 0] = 0x38                                                      # no zeros: every element of C tells its scale
    sb = rng.integers(125, 130, (n, 4)).astype(U8)
    A, SA = operand_bufs(dev, ea, sa)
    B, SB = operand_bufs(dev, eb, sb)
    Cb = Buf(dev, m, n, n + 8, F32)
    run_mx(dev, m, n, k, A, SA, B, SB, Cb)
    assert last_name(dev) == FAST + "f32"
    got = Cb.read()
    want = (dev.from_mxfp8(eb, sb).T * 2.0 ** (sa[np.arange(m), np.arange(m) // 32].astype(F64) - 127)[:, None]).astype(F32)      # C[r][c] = 2^sa[r][r / 32] B[c][r]
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{len(bad)} elements differ; first (row, col, got, want): {[(int(r), int(c), float(got[r, c]), float(want[r, c])) for r, c in bad[:6]]}"


@pytest.mark.parametrize("path", ["fast", "pitch"])
def test_scale_range(dev, path):
    """+-1 elements under scale bytes 87 .. 167 (every product 2^(sa + sb - 254) is a normal fp32).  Column c of B is non-zero in block c % 4 alone, so an
    element of C is a sum of 32 terms +-2^(sa + sb - 254) of ONE magnitude (and exact zeros): exact in fp32 in any order."""
    m, n, k = 130, 131, 128
    rng = np.random.default_rng(8)
    ea = np.where(rng.integers(0, 2, (m, k)) == 1, 0x38, 0xB8).astype(U8)
    eb = np.where(rng.integers(0, 2, (n, k)) == 1, 0x38, 0xB8).astype(U8)
    eb[(np.arange(k)[None, :] // 32) != (np.arange(n)[:, None] % 4)] = 0
    sa, sb = rng.integers(87, 168, (m, 4)).astype(U8), rng.integers(87, 168, (n, 4)).astype(U8)
    sa[0, :], sb[0, 0], sa[1, :], sb[1, 1] = 87, 87, 167, 167            # the corners
    A, SA = operand_bufs(dev, ea, sa, path)
    B, SB = operand_bufs(dev, eb, sb, path)
    Cb = Buf(dev, m, n, n + 8, F32)
    run_mx(dev, m, n, k, A, SA, B, SB, Cb)
    assert last_name(dev) == (FAST if path == "fast" else GENERAL) + "f32"
    ref64 = dev.from_mxfp8(ea, sa).astype(F64) @ dev.from_mxfp8(eb, sb).astype(F64).T
    ref = ref64.astype(F32)
    assert np.array_equal(ref.astype(F64), ref64) and np.isfinite(ref).all()
    got = Cb.read()
    assert np.array_equal(got.view(U32), ref.view(U32)), np.argwhere(got != ref)[:6].tolist()


@pytest.mark.parametrize("k", [96, 160, 32])
def test_scale_pitch_padding_does_not_reach_c(dev, k):
    """k / 32 = 3, 5, 1: the last slab's scale dword holds 1 to 3 bytes of pitch padding, here 0xFF (NaN); so do whole dwords behind them."""
    m, n = 70, 133
    ea, sa, eb, sb, ref = int_case(dev, m, n, k)
    A, SA = operand_bufs(dev, ea, sa, scale_fill=0xFF, fill=0xFF)
    B, SB = operand_bufs(dev, eb, sb, scale_fill=0xFF, fill=0xFF)
    Cb = Buf(dev, m, n, n + 8, F32)
    run_mx(dev, m, n, k, A, SA, B, SB, Cb)
    assert last_name(dev) == FAST + "f32"
    got = Cb.read()
    assert np.isfinite(got).all() and np.array_equal(got.view(U32), ref.view(U32))


@pytest.mark.parametrize("path", ["fast", "pitch"], ids=["fast", "general"])
def test_nan_operands_stay_in_their_rows_and_columns(dev, path):
    """What a NaN in a GEMM operand gives is unspecified beyond "no fault, and only the affected rows or columns of C": every other element is still exact.
    (Observed, and printed: the affected rows and columns are NaN throughout, on both paths.)"""
    m, n, k = 130, 131, 160
    ea, sa, eb, sb, ref = int_case(dev, m, n, k)
    ea, sa, eb, sb = ea.copy(), sa.copy(), eb.copy(), sb.copy()
    sa[3, 0], ea[129, 159], sb[5, 4], eb[128, 40] = 0xFF, 0x7F, 0xFF, 0xFF            # rows 3 and 129, columns 5 and 128
    A, SA = operand_bufs(dev, ea, sa, path)
    B, SB = operand_bufs(dev, eb, sb, path)
    Cb = Buf(dev, m, n, n + 8, F32, fill=0x3C)
    run_mx(dev, m, n, k, A, SA, B, SB, Cb)
    got = Cb.read()
    hit = np.zeros((m, n), bool)
    hit[[3, 129], :] = True
    hit[:, [5, 128]] = True
    print(f"{last_name(dev)}: {int(np.isnan(got[hit]).sum())} of {int(hit.sum())} elements of the affected rows and columns are NaN")
    assert np.array_equal(got[~hit].view(U32), ref[~hit].view(U32)) and Cb.outside_ok


# ---- rounded data against float64 -----------------------------------------------------------------------------------------------------------------------
_worst = {}


def rounded_run(dev, c, path, out=F32):
    m, n, k = c["m"], c["n"], c["k"]
    A, SA = operand_bufs(dev, c["ea"], c["sa"], path)
    B, SB = operand_bufs(dev, c["eb"], c["sb"], path)
    d_br, d_bc = dev.to_device(c["br"]), dev.to_device(c["bc"])
    c0 = dev.from_bf16(dev.to_bf16(c["c0"])) if out == U16 else c["c0"]
    Cb = Buf(dev, m, n, n + 8, out, window=dev.to_bf16(c0) if out == U16 else c0)
    ep = dev.Epilogue(alpha=c["alpha"], beta=c["beta"], bias_row=d_br.ptr, bias_col=d_bc.ptr, act=dev.ACT_RELU)
    run_mx(dev, m, n, k, A, SA, B, SB, Cb, ep)
    name = last_name(dev)
    assert name == (FAST if path == "fast" else GENERAL) + ("bf16" if out == U16 else "f32"), name
    got = Cb.read()
    assert Cb.outside_ok
    return got, name


@pytest.mark.parametrize("path", ["fast", "pitch"], ids=["fast", "general"])
@pytest.mark.parametrize("kind,m,n,k", RANDOM_CASES)
def test_rounded_data_against_float64(dev, kind, m, n, k, path):
    c = cached_case(kind, m, n, k)
    got, name = rounded_run(dev, c, path)
    err = np.abs(got.astype(F64) - c["ref"])                  # an element left at the NaN pattern fails the comparison
    ratio = float(np.nanmax(err / c["bound"]))
    key = "fast" if path == "fast" else "general"
    _worst[key] = max(_worst.get(key, 0.0), ratio)
    print(f"{name} {kind} {m}x{n}x{k}: worst |got - ref| / bound = {ratio:.4f} (worst so far on the {key} path: {_worst[key]:.4f})")
    assert (err <= c["bound"]).all(), f"{name}: worst ratio {ratio:.3f}, unwritten {int(np.isnan(err).sum())}"


@pytest.mark.parametrize("path", ["fast", "pitch"], ids=["fast", "general"])
def test_bf16_output_is_the_rounded_fp32_output(dev, path):
    """beta C0 with C0 exact in bf16, so both calls read the same value."""
    c = dict(cached_case("normal_rows", 130, 257, 160))
    c["c0"] = dev.from_bf16(dev.to_bf16(c["c0"]))
    got32, _ = rounded_run(dev, c, path, F32)
    got16, name = rounded_run(dev, c, path, U16)
    assert np.array_equal(got16, dev.to_bf16(got32)), f"{name}: {int((got16 != dev.to_bf16(got32)).sum())} elements differ"


# ---- bla_gemm_f32_as_mxfp8 is the composition ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,k", [(129, 127, 1000), (128, 128, 128)])
@pytest.mark.parametrize("lay", ["nn", "nt", "tn", "tt"])
def test_f32_as_mxfp8_is_the_composition(dev, lay, m, n, k):
    L = dev.lib()
    ta, tb = lay[0] == "t", lay[1] == "t"
    a, b = random_operand("normal_rows", 41, m, k), random_operand("uniform", 42, n, k)            # op(A) [m][k], op(B)^T [n][k]
    sa_, sb_ = np.ascontiguousarray(a.T if ta else a), np.ascontiguousarray(b if tb else b.T)      # as stored: A m x k (k x m), B k x n (n x k)
    A32 = Buf(dev, sa_.shape[0], sa_.shape[1], sa_.shape[1] + 5, F32, window=sa_, fill=0x3C)
    B32 = Buf(dev, sb_.shape[0], sb_.shape[1], sb_.shape[1] + 5, F32, window=sb_, fill=0x3C)
    br = dev.to_device(uniform(43, (m,), dtype=F32))
    ep = dev.Epilogue(alpha=0.5, bias_row=br.ptr, act=dev.ACT_RELU)
    C1 = Buf(dev, m, n, n + 8, F32)
    assert L.bla_gemm_f32_as_mxfp8(None, int(ta), int(tb), m, n, k, A32.ptr, A32.ld, B32.ptr, B32.ld, C1.ptr, C1.ld, C.byref(ep)) == 0, L.bla_last_error()
    dev.sync()
    assert last_name(dev) == FAST + "f32"
    # the same by hand: both operands quantised into 16-byte aligned buffers, pitches k rounded up to 32 and k / 32 rounded up to 4, then the product
    kp = up(k, 32)
    ld_s = up(kp // 32, 4)
    EA, SA, EB, SB = Buf(dev, m, kp, kp, U8), Buf(dev, m, kp // 32, ld_s, U8), Buf(dev, n, kp, kp, U8), Buf(dev, n, kp // 32, ld_s, U8)
    assert L.bla_f32_to_mxfp8(None, A32.ptr, A32.ld, int(ta), m, k, EA.ptr, kp, SA.ptr, ld_s) == 0, L.bla_last_error()
    assert L.bla_f32_to_mxfp8(None, B32.ptr, B32.ld, int(not tb), n, k, EB.ptr, kp, SB.ptr, ld_s) == 0, L.bla_last_error()
    C2 = Buf(dev, m, n, n + 8, F32)
    run_mx(dev, m, n, kp, EA, SA, EB, SB, C2, ep)
    assert last_name(dev) == FAST + "f32"
    got1, got2 = C1.read(), C2.read()
    assert np.array_equal(got1.view(U32), got2.view(U32)) and C1.outside_ok and C2.outside_ok and A32.untouched() and B32.untouched()
    (ea, sa), (eb, sb) = dev.to_mxfp8(a), dev.to_mxfp8(b)
    assert np.array_equal(EA.read(), ea) and np.array_equal(SA.read(), sa) and np.array_equal(EB.read(), eb) and np.array_equal(SB.read(), sb)
    # and against float64 on the dequantised operands
    da, db = dev.from_mxfp8(ea, sa).astype(F64), dev.from_mxfp8(eb, sb).astype(F64)
    bias = br.numpy().astype(F64)[:, None]
    ref = np.maximum(0.5 * (da @ db.T) + bias, 0)
    bound = (kp + 8) * 2.0 ** -23 * 0.5 * (np.abs(da) @ np.abs(db).T) + 2 * 2.0 ** -24 * (np.abs(bias) + np.abs(ref))
    assert (np.abs(got1.astype(F64) - ref) <= bound).all()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------
REFUSED = [("pre_act", "ptr"), ("ld_pre", 8), ("relu_mask", "ptr"), ("ld_mask", 8), ("row_sum_a", "ptr"), ("softmax_y", "ptr"), ("softmax_scale", 1.0),
           ("softmax_grad", "ptr"), ("row_sum_alpha", 1.0), ("row_sum_beta", 1.0), ("softmax_loss_acc", "ptr"), ("softmax_correct_acc", "ptr"), ("act", 2)]


def test_refusals_leave_c_alone(dev):
    m, n, k = 16, 24, 64
    ea, sa, eb, sb, _ = int_case(dev, m, n, k)
    A, SA = operand_bufs(dev, ea, sa)
    B, SB = operand_bufs(dev, eb, sb)
    scratch = dev.zeros((m * n,), np.float64)
    L = dev.lib()
    A32, B32 = dev.to_device(np.ones((m, k), F32)), dev.to_device(np.ones((n, k), F32))
    for out in (F32, U16):
        Cb = Buf(dev, m, n, n + 8, out)
        L.bla_gemm_set_config(-1, 0)
        before = last_name(dev)
        for field, value in REFUSED:
            ep = dev.Epilogue(alpha=1.0)
            setattr(ep, field, scratch.ptr if value == "ptr" else value)
            run_mx(dev, m, n, k, A, SA, B, SB, Cb, ep, want=1)
            if out == F32:
                assert L.bla_gemm_f32_as_mxfp8(None, 0, 1, m, n, k, A32.ptr, k, B32.ptr, k, Cb.ptr, Cb.ld, C.byref(ep)) == 1
        c_type = dev.C_BF16 if out == U16 else dev.C_F32

        def call(mm=m, nn=n, kk=k, a=A.ptr, lda=A.ld, s_a=SA.ptr, ldsa=SA.ld, b=B.ptr, ldb=B.ld, s_b=SB.ptr, ldsb=SB.ld, c=Cb.ptr, ldc=Cb.ld, ct=c_type):
            return L.bla_gemm_mxfp8(None, mm, nn, kk, a, lda, s_a, ldsa, b, ldb, s_b, ldsb, c, ldc, ct, None)
        assert call(kk=48) == 1 and call(kk=33) == 1 and call(mm=-1) == 1 and call(nn=-1) == 1 and call(kk=-32) == 1
        assert call(a=None) == 1 and call(b=None) == 1 and call(s_a=None) == 1 and call(s_b=None) == 1 and call(c=None) == 1
        assert call(lda=k - 1) == 1 and call(ldb=k - 1) == 1 and call(ldsa=1) == 1 and call(ldsb=1) == 1 and call(ldc=n - 1) == 1 and call(ct=2) == 1
        dev.sync()
        assert last_name(dev) == before and Cb.untouched()
        assert call() == 0
        dev.sync()
        assert not Cb.untouched()
