"""MXFP8 (e4m3 elements, E8M0 block scales, fp32 accumulation): what can be checked without a device.

1. The host restatement of the conversions (native.to_mxfp8 / from_mxfp8, which the GPU tests hold bla_f32_to_mxfp8 / bla_mxfp8_to_f32 to bit for bit)
   against an independent implementation: torch's CPU float8_e4m3fn cast of the pre-clamped scaled value, torch's decode of all 256 element bytes and of
   all 256 float8_e8m0fnu scale bytes.
2. The quantisation rule of include/bla.h: |dequantised - v| <= max(|v| / 8, 2^(e - 10)) per element (1/8: scaled magnitudes in (448, 512) saturate to
   448; 2^(e - 10): half a subnormal step), a block's largest element never decodes to zero, trans = 1 equals trans = 0 of the transposed array, tail
   padding is +0, NaN / Inf blocks come out as scale 0xFF with elements 0x7F.
3. A float32 restatement of the product (dequantised values, a k-ascending fp32 chain, the epilogue) against float64 on the GPU tests' random cases,
   inside the bound the GPU tests use

       bound = (k + 8) 2^-23 |alpha| (|A|.|B|) + 2 2^-24 (|bias_row| + |bias_col| + |beta C0| + |ref|)

   (a product of two dequantised values has 4 + 4 significant bits and is exact in fp32; at most one ulp per add, in any order) -- and OUTSIDE it under
   four mutations: A's scale taken from the neighbouring block, the scale decoded as 2^(s - 126), the last k-block dropped, saturation replaced by
   wrap-around to NaN.  The neighbouring-block mutation changes nothing where all of a row's scale bytes are equal, which is the case for every row of
   the uniform [-1, 1) operands (a block's maximum is in [0.5, 1) unless all 32 values are below 0.5): there the test asserts exactly that instead.
4. Without a device the four entries answer BLA_ERR_NO_DEVICE; an unsupported epilogue field and k % 32 != 0 are refused before the device is asked for.
"""
import ctypes as C

import numpy as np
import pytest

from inputs import uniform

F32, F64, U8, U32 = np.float32, np.float64, np.uint8, np.uint32


# ---- the edge set: scaled values (the block scale is pinned to 1 by a 300.0 in front of every block of 32) ----------------------------------------------
def _e4m3_value(b):
    e, m = (b >> 3) & 15, b & 7
    return (1 + m / 8) * 2.0 ** (e - 7) if e else m * 2.0 ** -9


def edge_values():
    """Every tie between two neighbouring e4m3 magnitudes (all binades, subnormals included) with its fp32 neighbours, 448 / 464 / 465 and the values
    around them, the smallest subnormal, half of it and its neighbours, +-0, fp32 subnormals -- and all of them negated."""
    v = []
    for b in range(0x7E):
        tie = F32((_e4m3_value(b) + _e4m3_value(b + 1)) / 2)
        v += [F32(_e4m3_value(b)), np.nextafter(tie, F32(0)), tie, np.nextafter(tie, F32(1000))]
    v += [F32(448), F32(464), np.nextafter(F32(464), F32(0)), np.nextafter(F32(464), F32(1000)), F32(465), F32(480), F32(496), np.nextafter(F32(512), F32(0))]
    v += [F32(2.0 ** -9), F32(2.0 ** -10), np.nextafter(F32(2.0 ** -10), F32(0)), np.nextafter(F32(2.0 ** -10), F32(1)), F32(3 * 2.0 ** -10), F32(2.0 ** -11)]
    v += [F32(0.0), np.array(1, U32).view(F32), np.array(0x007FFFFF, U32).view(F32), np.array(0x00800000, U32).view(F32), F32(1e-30)]
    v = np.array(v, F32)
    return np.concatenate([v, -v])


def edge_row():
    """The edge set as one row of whole blocks: 300.0 in front of every 31 edge values pins every block's scale byte to 127 (floor(log2 300) = 8)."""
    v = edge_values()
    v = np.concatenate([v, np.zeros(-len(v) % 31, F32)]).reshape(-1, 31)
    return np.concatenate([np.full((len(v), 1), 300.0, F32), v], axis=1).reshape(1, -1)


def torch_e4m3_bytes(x):
    """torch's CPU cast of the pre-clamped value (its own cast gives NaN above 464: the saturation is the contract's choice)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, F32)).clamp(-448, 448).to(torch.float8_e4m3fn)
    return t.view(torch.uint8).numpy()


def test_element_rounding_edge_set_matches_torch(pkg):
    v = edge_values()
    assert np.array_equal(pkg.native.e4m3_round(v), torch_e4m3_bytes(v))
    by = dict(zip(v.tolist(), pkg.native.e4m3_round(v).tolist()))
    assert by[448.0] == 0x7E and by[464.0] == 0x7E and by[465.0] == 0x7E and by[-465.0] == 0xFE            # the tie goes to even, above it saturates
    assert by[2.0 ** -9] == 0x01 and by[2.0 ** -10] == 0x00 and by[3 * 2.0 ** -10] == 0x02                   # ties among the subnormals go to even
    z = pkg.native.e4m3_round(np.array([0.0, -0.0], F32))
    assert z.tolist() == [0x00, 0x80]
    # and through the quantiser: the scale of every block is 1
    el, sc = pkg.to_mxfp8(edge_row())
    assert (sc == 127).all() and np.array_equal(el, torch_e4m3_bytes(edge_row()))


def test_element_rounding_random_bit_patterns_match_torch(pkg):
    bits = np.random.default_rng(22).integers(0, 2 ** 32, 2 ** 21, dtype=np.uint64).astype(U32)
    x = bits.view(F32)
    x = x[np.abs(x) < 512][:2 ** 20]            # finite scaled values: what the quantiser hands to the rounding
    assert len(x) == 2 ** 20
    # most random patterns are far outside [2^-10, 512): add the same mantissas at exponents inside it
    inside = ((bits[:2 ** 20] & U32(0x807FFFFF)) | ((U32(116) + (bits[:2 ** 20] >> U32(23)) % U32(20)) << U32(23))).view(F32)
    for part in (x, inside):
        assert np.array_equal(pkg.native.e4m3_round(part), torch_e4m3_bytes(part))


def test_all_element_bytes_decode_as_torch_decodes_them(pkg):
    import torch
    b = np.arange(256, dtype=np.int32).astype(U8)
    got = pkg.native.e4m3_decode(b)
    want = torch.from_numpy(b.copy()).view(torch.float8_e4m3fn).to(torch.float32).numpy()
    nan = np.isnan(want)
    assert nan.sum() == 2 and nan[0x7F] and nan[0xFF]
    assert np.array_equal(got.view(U32)[~nan], want.view(U32)[~nan]) and np.isnan(got[nan]).all()
    fin = ~nan
    assert np.array_equal(pkg.native.e4m3_round(got[fin]), b[fin])        # and back, -0 included


def test_all_scale_bytes_decode_as_torch_decodes_them(pkg):
    import torch
    s = np.arange(256, dtype=np.int32).astype(U8)
    got = pkg.native.e8m0_decode(s)
    want = torch.from_numpy(s.copy()).view(torch.float8_e8m0fnu).to(torch.float32).numpy()
    assert np.isnan(want[255]) and np.isnan(got[255])
    assert np.array_equal(got.view(U32)[:255], want.view(U32)[:255])
    assert np.array_equal(got[:255].astype(F64), 2.0 ** (np.arange(255) - 127.0))


# ---- the random operands of the GPU tests (shared with test_mxfp8_gpu.py) -------------------------------------------------------------------------------
def random_operand(kind, seed, rows, k):
    """uniform [-1, 1), or standard normal values times 1e-3, 1 or 37 by row."""
    if kind == "uniform":
        return uniform(seed, (rows, k), -1.0, 1.0, F32)
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows, k)) * np.array([1e-3, 1.0, 37.0])[rng.integers(0, 3, rows)][:, None]).astype(F32)


RANDOM_CASES = [("uniform", 129, 127, 992), ("normal_rows", 129, 127, 992), ("uniform", 128, 128, 128), ("normal_rows", 130, 257, 160)]
EPILOGUE = dict(alpha=0.5, beta=0.75, relu=True)


def random_case(kind, m, n, k, seed=61):
    """Operands quantised on the host, the epilogue's inputs, the float64 reference on the dequantised values and the bound."""
    from conftest import load_pkg
    pkg = load_pkg()
    a, b = random_operand(kind, seed, m, k), random_operand(kind, seed + 1, n, k)
    (ea, sa), (eb, sb) = pkg.to_mxfp8(a), pkg.to_mxfp8(b)
    br, bc = uniform(seed + 2, (m,), dtype=F32), uniform(seed + 3, (n,), dtype=F32)
    c0 = uniform(seed + 4, (m, n), dtype=F32)
    da, db = pkg.from_mxfp8(ea, sa).astype(F64), pkg.from_mxfp8(eb, sb).astype(F64)
    alpha, beta = EPILOGUE["alpha"], EPILOGUE["beta"]
    ref = np.maximum(alpha * (da @ db.T) + br.astype(F64)[:, None] + bc.astype(F64)[None, :], 0) + beta * c0.astype(F64)
    bound = (k + 8) * 2.0 ** -23 * abs(alpha) * (np.abs(da) @ np.abs(db).T) + 2 * 2.0 ** -24 * (
        np.abs(br.astype(F64))[:, None] + np.abs(bc.astype(F64))[None, :] + np.abs(beta * c0.astype(F64)) + np.abs(ref))
    return dict(a=a, b=b, ea=ea, sa=sa, eb=eb, sb=sb, br=br, bc=bc, c0=c0, ref=ref, bound=bound, m=m, n=n, k=k, alpha=alpha, beta=beta)


_cases = {}


def cached_case(kind, m, n, k):
    if (kind, m, n, k) not in _cases:
        _cases[(kind, m, n, k)] = random_case(kind, m, n, k)
    return _cases[(kind, m, n, k)]


# ---- the quantisation rule --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "normal_rows", "wide"])
def test_quantisation_error_rule(pkg, kind):
    if kind == "wide":
        rng = np.random.default_rng(3)
        v = (rng.standard_normal((64, 256)) * 2.0 ** rng.integers(-40, 40, (64, 256))).astype(F32)      # widely scaled within a block
    else:
        v = random_operand(kind, 7, 64, 256)
    el, sc = pkg.to_mxfp8(v)
    d = pkg.from_mxfp8(el, sc).astype(F64)
    e = np.repeat(sc.astype(np.int64) - 127, 32, axis=1)
    limit = np.maximum(np.abs(v.astype(F64)) / 8, 2.0 ** (e - 10.0))
    err = np.abs(d - v.astype(F64))
    print(f"{kind}: worst |dequantised - v| / limit = {(err / limit).max():.4f}")
    assert (err <= limit).all()
    # the block's largest element never decodes to zero, and the scale follows the rule
    blocks = np.abs(v).reshape(64, 8, 32)
    top = np.take_along_axis(np.abs(d).reshape(64, 8, 32), blocks.argmax(2)[:, :, None], 2)[:, :, 0]
    assert (top > 0).all()
    assert np.array_equal(sc.astype(np.int64) - 127, np.clip(np.floor(np.log2(blocks.max(2).astype(F64))) - 8, -127, 127))


def test_scale_clamps_and_zero_blocks(pkg):
    v = np.zeros((4, 32), F32)
    v[1, 3] = np.array(1, U32).view(F32)          # an fp32 subnormal: floor(log2) - 8 is below -127
    v[2, 5] = -3.0e38                             # near the largest fp32: e = 127 - 8 = 119
    v[3, 0] = 2.0 ** -118                         # floor(log2) - 8 = -126
    el, sc = pkg.to_mxfp8(v)
    assert sc[:, 0].tolist() == [127, 0, 246, 1]
    assert not el[0].any() and not el[1].any()                      # 2^-149 2^127 = 2^-22 is below half of 2^-9
    assert el[2, 5] == 0xFE and el[3, 0] == 0x78                # -3e38 2^-119 = -451.4 -> -448;  2^-118 2^126 = 256
    assert np.array_equal(pkg.from_mxfp8(el, sc)[3, :1], np.array([2.0 ** -118], F32))


def test_trans_equals_the_transposed_array(pkg):
    v = random_operand("normal_rows", 9, 37, 130)
    el, sc = pkg.to_mxfp8(v)
    el_t, sc_t = pkg.to_mxfp8(np.ascontiguousarray(v.T), trans=True)
    assert el.shape == (37, 160) and sc.shape == (37, 5)
    assert np.array_equal(el, el_t) and np.array_equal(sc, sc_t)


def test_tail_padding_is_plus_zero(pkg):
    v = -np.abs(random_operand("uniform", 10, 5, 70)) - F32(0.01)
    el, sc = pkg.to_mxfp8(v)
    assert el.shape == (5, 96) and not el[:, 70:].any() and (el[:, :70] & 0x80).all()
    assert np.array_equal(pkg.to_mxfp8(np.pad(v, ((0, 0), (0, 26))))[0], el)      # +0 values, quantised with the block


def test_nan_and_inf_blocks(pkg):
    v = random_operand("uniform", 11, 3, 96)
    v[0, 40] = np.nan
    v[1, 5] = np.inf
    v[2, 95] = -np.inf
    el, sc = pkg.to_mxfp8(v)
    assert sc.tolist() == [[127 - 9, 255, 127 - 9], [255, 127 - 9, 127 - 9], [127 - 9, 127 - 9, 255]]
    for r, g in ((0, 1), (1, 0), (2, 2)):
        assert (el[r, 32 * g:32 * g + 32] == 0x7F).all()
    d = pkg.from_mxfp8(el, sc)
    nan = np.isnan(d)
    assert nan.sum() == 96 and nan[0, 32:64].all() and nan[1, :32].all() and nan[2, 64:].all()
    assert (d.view(U32)[nan] == 0x7FC00000).all()
    e = np.full((1, 32), 0x38, U8)
    e[0, 3] = 0xFF
    assert np.isnan(pkg.from_mxfp8(e, np.array([[127]], U8))).sum() == 1            # a NaN element alone


# ---- the accumulation model ---------------------------------------------------------------------------------------------------------------------------
def restated_product(pkg, c, mutation=None):
    """float32: dequantised values, a k-ascending chain of exact products, then alpha, bias_row, bias_col, ReLU, beta C0 in bla_gemm_bf16's order."""
    ea, sa, eb, sb, k = c["ea"], c["sa"], c["eb"], c["sb"], c["k"]
    if mutation == "neighbour_scale":
        sa = np.roll(sa, 1, axis=1)
    if mutation == "wrap_to_nan":            # what an unsaturated rounding gives above 464: the NaN byte
        scaled = np.abs(c["a"].astype(F64)) * 2.0 ** -(np.repeat(sa.astype(F64), 32, axis=1) - 127)
        ea = np.where(scaled > 464, U8(0x7F), ea)
    a, b = pkg.from_mxfp8(ea, sa), pkg.from_mxfp8(eb, sb)
    if mutation == "scale_126":
        a = (a * F32(2)).astype(F32)
    if mutation == "drop_last_block":
        k -= 32
    acc = np.zeros((c["m"], c["n"]), F32)
    with np.errstate(invalid="ignore"):
        for kk in range(k):
            acc = (acc + a[:, kk, None] * b[None, :, kk]).astype(F32)
        v = (F32(c["alpha"]) * acc).astype(F32)
        v = (v + c["br"][:, None]).astype(F32)
        v = (v + c["bc"][None, :]).astype(F32)
        v = np.where(v < 0, F32(0), v)
        return (v + (F32(c["beta"]) * c["c0"]).astype(F32)).astype(F32)


@pytest.mark.parametrize("kind,m,n,k", RANDOM_CASES)
def test_restated_product_stays_inside_the_bound(pkg, kind, m, n, k):
    c = cached_case(kind, m, n, k)
    prod = pkg.from_mxfp8(c["ea"], c["sa"])[:5, None, :] * pkg.from_mxfp8(c["eb"], c["sb"])[None, :7, :]
    assert np.array_equal(prod.astype(F64), pkg.from_mxfp8(c["ea"], c["sa"]).astype(F64)[:5, None, :] * pkg.from_mxfp8(c["eb"], c["sb"]).astype(F64)[None, :7, :])
    err = np.abs(restated_product(pkg, c).astype(F64) - c["ref"])
    print(f"{kind} {m}x{n}x{k}: worst |restated - ref| / bound = {(err / c['bound']).max():.4f}")
    assert (err <= c["bound"]).all()


@pytest.mark.parametrize("mutation", ["neighbour_scale", "scale_126", "drop_last_block", "wrap_to_nan"])
@pytest.mark.parametrize("kind,m,n,k", RANDOM_CASES)
def test_mutated_product_leaves_the_bound(pkg, kind, m, n, k, mutation):
    c = cached_case(kind, m, n, k)
    if mutation == "neighbour_scale" and np.array_equal(np.roll(c["sa"], 1, axis=1), c["sa"]):
        assert kind == "uniform" and (c["sa"] == 127 - 9).all()      # every block's maximum is in [0.5, 1): the mutation changes no byte (docstring, 3.)
        return
    err = np.abs(restated_product(pkg, c, mutation).astype(F64) - c["ref"])
    assert not (err <= c["bound"]).all(), mutation


# ---- without a device ---------------------------------------------------------------------------------------------------------------------------------
def no_device(pkg):
    import torch
    return not torch.cuda.is_available() and pkg.lib().bla_device_count() <= 0


def test_entries_refuse_without_a_device(pkg):
    """Extents and the epilogue are checked first, the device second, the pointers third: without a device these NULL calls answer BLA_ERR_NO_DEVICE (3);
    with one they launch nothing either -- 3 while the library is not initialised, BLA_ERR_INVALID (1) for the NULL pointers once it is."""
    L = pkg.lib()
    want = (3,) if no_device(pkg) else (1, 3)
    assert L.bla_f32_to_mxfp8(None, None, 32, 0, 1, 32, None, 32, None, 1) in want
    assert L.bla_f32_to_mxfp8(None, None, 32, 1, 1, 32, None, 32, None, 1) in want
    assert L.bla_mxfp8_to_f32(None, None, 32, None, 1, None, 32, 1, 32) in want
    assert L.bla_gemm_mxfp8(None, 8, 8, 32, None, 32, None, 1, None, 32, None, 1, None, 8, pkg.C_F32, None) in want
    assert L.bla_gemm_mxfp8(None, 8, 8, 32, None, 32, None, 1, None, 32, None, 1, None, 8, pkg.C_BF16, None) in want
    assert L.bla_gemm_f32_as_mxfp8(None, 0, 1, 8, 8, 8, None, 8, None, 8, None, 8, None) in want
    ep = pkg.Epilogue(alpha=0.5, beta=0.75, act=pkg.ACT_RELU)          # a supported epilogue changes nothing about that
    st = L.bla_gemm_mxfp8(None, 8, 8, 32, None, 32, None, 1, None, 32, None, 1, None, 8, pkg.C_F32, C.byref(ep))
    assert st in want
    if st == 3:
        assert b"no CPU fallback" in L.bla_last_error() or b"not initialised" in L.bla_last_error()


def test_pure_argument_checks_come_before_the_device(pkg):
    """BLA_ERR_INVALID whether or not a device is there (nothing is launched: the operands are NULL)."""
    L = pkg.lib()
    ep = pkg.Epilogue(alpha=1.0, pre_act=0x1000, ld_pre=8)
    assert L.bla_gemm_mxfp8(None, 8, 8, 32, None, 32, None, 1, None, 32, None, 1, None, 8, pkg.C_F32, C.byref(ep)) == 1
    assert b"epilogue" in L.bla_last_error()
    assert L.bla_gemm_f32_as_mxfp8(None, 0, 1, 8, 8, 8, None, 8, None, 8, None, 8, C.byref(ep)) == 1
    ep2 = pkg.Epilogue(alpha=1.0, act=2)
    assert L.bla_gemm_mxfp8(None, 8, 8, 32, None, 32, None, 1, None, 32, None, 1, None, 8, pkg.C_F32, C.byref(ep2)) == 1
    for k in (1, 31, 33, 48):
        assert L.bla_gemm_mxfp8(None, 8, 8, k, None, 64, None, 2, None, 64, None, 2, None, 8, pkg.C_F32, None) == 1
        assert b"multiple of 32" in L.bla_last_error()
    assert L.bla_gemm_mxfp8(None, -1, 8, 32, None, 32, None, 1, None, 32, None, 1, None, 8, pkg.C_F32, None) == 1
    assert L.bla_gemm_mxfp8(None, 8, 8, 32, None, 32, None, 1, None, 32, None, 1, None, 8, 7, None) == 1
    assert L.bla_f32_to_mxfp8(None, None, 32, 0, -1, 32, None, 32, None, 1) == 1
    assert L.bla_mxfp8_to_f32(None, None, 32, None, 1, None, 32, 1, -32) == 1
    assert L.bla_gemm_f32_as_mxfp8(None, 0, 1, 8, -8, 8, None, 8, None, 8, None, 8, None) == 1
