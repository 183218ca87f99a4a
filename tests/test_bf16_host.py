"""bf16 operands, fp32 accumulation: what can be checked without a device.

1. The host restatement of the conversions (native.to_bf16 / from_bf16, which the GPU tests hold bla_f32_to_bf16 / bla_bf16_to_f32 to bit for bit)
   against torch's CPU bfloat16.
2. A numpy float32 restatement of the fast kernel's accumulation (64-deep slabs, 16-deep MFMA steps, the two 8-element fragment halves of a step, exact
   products, one fp32 add per product) against float64, inside the bound the GPU tests use -- and OUTSIDE it under four mutations, so the bound is tight
   enough to catch a dropped slab, a doubled k-group, swapped fragment halves and a misplaced bias.

   bound = (k + 8) 2^-23 |alpha| (|A|.|B|) + 2 2^-24 (|bias_row| + |bias_col| + |beta C0| + |ref|)
   A product of two bf16 values has 16 significant bits and is exact in fp32, so the only error of the product is that of k fp32 adds: any order, rounded
   to nearest or toward zero, stays within (k - 1) 2^-23 sum |ab|.  The second term is the epilogue's roundings.
3. Without a device every new entry returns BLA_ERR_NO_DEVICE; an epilogue field the bf16 product does not honour is refused before the device is asked for.
"""
import ctypes as C

import numpy as np
import pytest

F32, F64, U16, U32 = np.float32, np.float64, np.uint16, np.uint32

EDGE_BITS = np.array([
    0x00000000, 0x80000000, 0x7F800000, 0xFF800000,            # +-0, +-inf
    0x00000001, 0x007FFFFF, 0x80000001, 0x807FFFFF,            # smallest and largest subnormals
    0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,            # exact ties: down to even, up to even, both signs
    0x00008000, 0x00018000, 0x007F8000,                        # ties among subnormals; the last one rounds up into the normals
    0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,            # one ulp to either side of a tie
    0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF,            # the largest finite value -> inf, the tie below inf -> inf, just under it stays finite
    0x7FC00000, 0x7F800001, 0xFFFFFFFF, 0x7F80FFFF, 0x7FFF0000,  # NaNs, among them patterns whose upper half alone would read as inf
    0x3F800000, 0x40490FDB, 0xC2F6E979, 0x00800000,
], dtype=U32)


def torch_bf16_bits(bits):
    import torch
    t = torch.from_numpy(bits.view(np.int32).copy()).view(torch.float32).to(torch.bfloat16)
    return t.view(torch.int16).numpy().view(U16)


def check_against_torch(pkg, bits):
    got = pkg.to_bf16(bits.view(F32))
    want = torch_bf16_bits(bits)
    nan = np.isnan(bits.view(F32))
    assert np.array_equal(got[~nan], want[~nan])
    assert np.isnan(pkg.from_bf16(got[nan])).all() and np.isnan(pkg.from_bf16(want[nan])).all()
    # the restatement of the issue, where no NaN is involved
    u = bits[~nan].astype(np.uint64)
    assert np.array_equal(got[~nan], ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(U16))


def test_conversion_edge_set_matches_torch(pkg):
    check_against_torch(pkg, EDGE_BITS)
    got = pkg.to_bf16(EDGE_BITS.view(F32))
    by = dict(zip(EDGE_BITS.tolist(), got.tolist()))
    assert by[0x7F7FFFFF] == 0x7F80 and by[0xFF7FFFFF] == 0xFF80          # above the largest bf16: inf
    assert by[0x3F808000] == 0x3F80 and by[0x3F818000] == 0x3F82          # ties to even, down and up
    assert by[0x00000000] == 0x0000 and by[0x80000000] == 0x8000 and by[0x7F800000] == 0x7F80 and by[0xFF800000] == 0xFF80
    assert by[0x00000001] == 0x0000 and by[0x007FFFFF] == 0x0080          # subnormals round like everything else, nothing is flushed
    assert by[0x00018000] == 0x0002


def test_conversion_random_bit_patterns_match_torch(pkg):
    bits = np.random.default_rng(20).integers(0, 2 ** 32, 100_000, dtype=np.uint64).astype(U32)
    check_against_torch(pkg, bits)


def test_widening_is_exact(pkg):
    import torch
    h = np.arange(65536, dtype=np.uint32).astype(U16)
    got = pkg.from_bf16(h)
    assert np.array_equal(got.view(U32), h.astype(U32) << 16)
    want = torch.from_numpy(h.view(np.int16).copy()).view(torch.bfloat16).to(torch.float32).numpy()
    ok = ~np.isnan(want)
    assert np.array_equal(got.view(U32)[ok], want.view(U32)[ok]) and np.isnan(got[~ok]).all()
    fin = np.isfinite(got)
    assert np.array_equal(pkg.to_bf16(got[fin]), h[fin])                 # and back


# ---- the kernel's accumulation, restated ----------------------------------------------------------------------------------------------------------
def restated_product(a, b, bias_row, bias_col, relu, mutation=None):
    """a [m][k], b [n][k]: float32 arrays holding bf16 values.  The fast kernel's order: slabs of 64, MFMA steps of 16, per step the fragment half
    h = 0 (k = 0..7 of the step) then h = 1 (k = 8..15), one fp32 add per exact product.  Epilogue: bias_row, bias_col, ReLU (alpha 1, beta 0)."""
    m, k = a.shape
    n = b.shape[0]
    acc = np.zeros((m, n), F32)
    slabs = list(range(0, k, 64))
    if mutation == "drop_last_slab":
        slabs = slabs[:-1]
    for kb in slabs:
        for s in range(0, min(64, k - kb), 16):
            for h in (0, 1):
                k0 = kb + s + 8 * h
                if k0 >= k:
                    continue
                ka = kb + s + 8 * (1 - h) if mutation == "swap_a_halves" and kb + s + 16 <= k else k0
                times = 2 if mutation == "double_group" and k0 == 8 else 1
                for _ in range(times):
                    for j in range(8):
                        prod = a[:, ka + j, None] * b[None, :, k0 + j]       # exact: 8 + 8 significant bits
                        acc = (acc + prod).astype(F32)
    v = acc
    if mutation == "bias_after_relu":
        v = np.maximum(v, F32(0))
    v = (v + bias_row[:, None]).astype(F32)
    v = (v + bias_col[None, :]).astype(F32)
    if relu and mutation != "bias_after_relu":
        v = np.maximum(v, F32(0))
    return v


def half_to_one(rng, shape):
    """bf16 values with magnitudes in [0.5, 1) and random signs, as float32."""
    from conftest import load_pkg
    pkg = load_pkg()
    x = rng.uniform(0.5, 1.0, shape).astype(F32)
    x = np.minimum(pkg.from_bf16(pkg.to_bf16(x)), F32(0.99609375))           # rounding may reach 1.0: the largest bf16 below it
    return (x * rng.choice(np.array([-1, 1], F32), shape)).astype(F32)


@pytest.fixture(scope="module")
def restated_case():
    rng = np.random.default_rng(31)
    m, n, k = 40, 33, 200                                # three whole slabs and one of 8
    a, b = half_to_one(rng, (m, k)), half_to_one(rng, (n, k))
    br, bc = half_to_one(rng, m), half_to_one(rng, n)
    exact = a.astype(F64) @ b.astype(F64).T
    ref = np.maximum(exact + br[:, None] + bc[None, :], 0)
    absprod = np.abs(a).astype(F64) @ np.abs(b).astype(F64).T
    bound = (k + 8) * 2.0 ** -23 * absprod + 2 * 2.0 ** -24 * (np.abs(br)[:, None] + np.abs(bc)[None, :] + np.abs(ref))
    return dict(a=a, b=b, br=br, bc=bc, ref=ref, bound=bound, k=k)


def test_products_of_bf16_values_are_exact_in_fp32(restated_case):
    a, b = restated_case["a"], restated_case["b"]
    p32 = a[:, None, :] * b[None, :, :]
    assert np.array_equal(p32.astype(F64), a.astype(F64)[:, None, :] * b.astype(F64)[None, :, :])


def test_restated_accumulation_stays_inside_the_bound(restated_case):
    c = restated_case
    got = restated_product(c["a"], c["b"], c["br"], c["bc"], True)
    err = np.abs(got.astype(F64) - c["ref"])
    assert (err <= c["bound"]).all(), (err / c["bound"]).max()


def test_every_product_exceeds_the_bound(restated_case):
    """Operands in [0.5, 1): one product is at least 0.25, the bound at most (k + 8) k 2^-23 + 2^-23 (2 + k + 2) -- so one lost or doubled product shows."""
    c = restated_case
    for k in (c["k"], 1024):
        assert (k + 8) * k * 2.0 ** -23 + 2.0 ** -23 * (k + 4) < 0.25
    assert (k + 8) * k * 2.0 ** -23 < 0.13
    assert c["bound"].max() < 0.25
    assert np.abs(c["a"]).min() >= 0.5 and np.abs(c["b"]).min() >= 0.5 and np.abs(c["a"]).max() < 1 and np.abs(c["b"]).max() < 1


@pytest.mark.parametrize("mutation", ["drop_last_slab", "double_group", "swap_a_halves", "bias_after_relu"])
def test_mutated_accumulation_leaves_the_bound(restated_case, mutation):
    c = restated_case
    got = restated_product(c["a"], c["b"], c["br"], c["bc"], True, mutation)
    err = np.abs(got.astype(F64) - c["ref"])
    assert (err > c["bound"]).any(), mutation


# ---- workgroup -> tile, restated (csrc/bla_bf16_tile.h: xcd_tile, then groups of 8 tile rows walked column by column) -----------------------------------
def tile_of(bid, tiles_m, tiles_n):
    nwg = tiles_m * tiles_n
    q, r, x, i = nwg >> 3, nwg & 7, bid & 7, bid >> 3
    pid = (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + i
    gsz = 8 * tiles_n
    first = pid // gsz * 8
    gm = min(tiles_m - first, 8)
    return first + (pid % gsz) % gm, (pid % gsz) // gm


@pytest.mark.parametrize("tiles_m,tiles_n", [(6, 6), (10, 2), (9, 1), (8, 3), (17, 5), (1, 1)])
def test_tile_order_hits_every_tile_once(tiles_m, tiles_n):
    """6 x 6: the largest grid the GPU tests had; 10 x 2 and 9 x 1: a last group of fewer than 8 tile rows (the GPU cases 1153 x 129 and F = 1100)."""
    hit = sorted(tile_of(bid, tiles_m, tiles_n) for bid in range(tiles_m * tiles_n))
    assert hit == [(tm, tn) for tm in range(tiles_m) for tn in range(tiles_n)]


# ---- without a device ---------------------------------------------------------------------------------------------------------------------------------
def no_device(pkg):
    import torch
    return not torch.cuda.is_available() and pkg.lib().bla_device_count() <= 0


def test_new_entries_refuse_without_a_device(pkg):
    if not no_device(pkg):
        pytest.skip("a device is present")
    L = pkg.lib()
    assert L.bla_f32_to_bf16(None, None, 8, None, 8, 1, 8) == 3
    assert L.bla_bf16_to_f32(None, None, 8, None, 8, 1, 8) == 3
    assert L.bla_transpose_b16(None, None, 8, None, 8, 8, 8) == 3
    assert L.bla_gemm_bf16(None, 0, 1, 8, 8, 8, None, 8, None, 8, None, 8, pkg.C_F32, None) == 3
    assert L.bla_gemm_bf16(None, 0, 0, 8, 8, 8, None, 8, None, 8, None, 8, pkg.C_BF16, None) == 3
    assert L.bla_gemm_f32_as_bf16(None, 0, 1, 8, 8, 8, None, 8, None, 8, None, 8, None) == 3
    assert b"no CPU fallback" in L.bla_last_error() or b"not initialised" in L.bla_last_error()
    ep = pkg.Epilogue(alpha=0.5, beta=0.75, act=pkg.ACT_RELU)          # a supported epilogue changes nothing about that
    assert L.bla_gemm_bf16(None, 0, 1, 8, 8, 8, None, 8, None, 8, None, 8, pkg.C_F32, C.byref(ep)) == 3


def test_unsupported_epilogue_field_is_refused_before_the_device(pkg):
    """The field check is a pure argument check: it answers BLA_ERR_INVALID whether or not a device is there (nothing is launched: the operands are NULL)."""
    L = pkg.lib()
    ep = pkg.Epilogue(alpha=1.0, pre_act=0x1000, ld_pre=8)
    assert L.bla_gemm_bf16(None, 0, 1, 8, 8, 8, None, 8, None, 8, None, 8, pkg.C_F32, C.byref(ep)) == 1
    assert b"epilogue" in L.bla_last_error()
    assert L.bla_gemm_f32_as_bf16(None, 0, 1, 8, 8, 8, None, 8, None, 8, None, 8, C.byref(ep)) == 1
