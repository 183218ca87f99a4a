"""The K-split of the bf16 product (bla_gemm_bf16_splitk): what can be checked without a device.

1. bla_gemm_bf16_splitk_plan against a Python restatement of include/bla.h's partition rule:
       slabs = ceil(k / 64);  S = clamp(requested, 1, slabs);  sps = ceil(slabs / S);  S_eff = ceil(slabs / sps);
       partial_bytes = S_eff > 1 ? S_eff tiles_m tiles_n 65536 : 0
   and of its automatic rule (slots = 3 cus; S = 1 when tiles >= slots or slabs < 2 MIN_SLABS, else min(slots // tiles, slabs // MIN_SLABS)), with the
   constant read from bla.h, plus the structural facts that hold whatever the constant is.
2. A numpy float32 restatement of the split accumulation (per split the slab-ordered accumulation of test_bf16_host.py's restated product, restated here,
   then the fold acc = P[0]; acc += P[1]; ...) against float64 inside the bound of the unsplit product,
       (k + 8) 2^-23 |alpha| (|A|.|B|) + 2 2^-24 (|bias_row| + |bias_col| + |beta C0| + |ref|),
   and OUTSIDE it under four mutations of the partition and the fold.  Why the unsplit bound holds: a partial over k_s terms errs by at most
   (k_s - 1) 2^-23 sum_s |ab|; the fold's S - 1 adds err by at most 2^-24 each of a running sum that is at most about sum |ab|; for S >= 2 every split is
   non-empty, so max k_s <= k - 64 (S - 2) - 8 and the total stays inside (k + 8) 2^-23 sum |ab|.
3. Without a device the plan entry answers (it is host only) and the two launching entries refuse: BLA_ERR_INVALID for a pure argument error,
   BLA_ERR_NO_DEVICE otherwise.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

F32, F64 = np.float32, np.float64
KS = [8, 64, 72, 1000, 1024, 65536]
SPLITS = [1, 2, 3, 5, 7, 16, 100]
MNS = [(1, 1), (129, 127), (289, 161), (128, 1152)]


def ceil_div(a, b):
    return -(-a // b)


def partition(k, splits):
    """include/bla.h's partition rule -> (S_eff, sps)"""
    slabs = ceil_div(k, 64)
    s = min(max(splits, 1), slabs)
    sps = ceil_div(slabs, s)
    return ceil_div(slabs, sps), sps


def min_slabs():
    from conftest import ROOT
    txt = open(os.path.join(ROOT, "include", "bla.h")).read()
    return int(re.search(r"#define\s+BLA_GEMM_BF16_SPLITK_MIN_SLABS\s+(\d+)", txt).group(1))


def automatic(m, n, k, cus, ms):
    """include/bla.h's automatic rule -> the S handed to the partition rule"""
    tiles, slabs = ceil_div(m, 128) * ceil_div(n, 128), ceil_div(k, 64)
    slots = 3 * (cus if cus > 0 else 256)
    if tiles >= slots or slabs < 2 * ms:
        return 1
    return min(slots // tiles, slabs // ms)


def plan(pkg, m, n, k, splits, cus=0):
    return pkg.gemm_bf16_splitk_plan(m, n, k, splits, cus)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("splits", SPLITS)
def test_plan_entry_is_the_partition_rule(pkg, k, splits):
    for m, n in MNS:
        eff, sps = partition(k, splits)
        tiles = ceil_div(m, 128) * ceil_div(n, 128)
        assert plan(pkg, m, n, k, splits) == (eff, sps, eff * tiles * 65536 if eff > 1 else 0), (m, n, k, splits)
        assert (eff - 1) * sps < ceil_div(k, 64) <= eff * sps                     # every split holds a slab, together they hold all of them


def test_plan_entry_named_cases(pkg):
    assert plan(pkg, 129, 127, 1000, 5)[:2] == (4, 4)
    assert plan(pkg, 129, 127, 1000, 3)[:2] == (3, 6)
    assert plan(pkg, 289, 161, 1024, 7)[:2] == (6, 3)
    assert plan(pkg, 129, 127, 1000, 100)[:2] == (16, 1) and plan(pkg, 129, 127, 72, 100)[:2] == (2, 1)       # clamped to the slabs
    for s in SPLITS:
        assert plan(pkg, 129, 127, 8, s) == (1, 1, 0)
    assert plan(pkg, 289, 161, 1024, 7)[2] == 6 * 3 * 2 * 65536
    assert plan(pkg, 129, 127, 1000, 1)[2] == 0
    L = pkg.lib()
    assert L.bla_gemm_bf16_splitk_plan(128, 128, 128, 2, 0, None, None, None) == 0      # any out pointer may be NULL
    assert L.bla_gemm_bf16_splitk_plan(128, 128, 128, -1, 0, None, None, None) == 1
    assert L.bla_gemm_bf16_splitk_plan(-1, 128, 128, 2, 0, None, None, None) == 1
    assert plan(pkg, 0, 128, 128, 4) == (1, 2, 0) and plan(pkg, 128, 128, 0, 4) == (1, 0, 0)


AUTO_M = [1, 128, 129, 256, 1024, 4096, 12000]
AUTO_N = [1, 127, 1152, 2304, 4096]
AUTO_K = [8, 64, 512, 1000, 1024, 4096, 8192, 16384, 65536]


@pytest.mark.parametrize("cus", [256, 8, 0])
def test_automatic_rule(pkg, cus):
    ms = min_slabs()
    assert ms >= 1
    eff_cus = cus if cus > 0 else 256
    for m in AUTO_M:
        for n in AUTO_N:
            for k in AUTO_K:
                eff, sps = partition(k, automatic(m, n, k, cus, ms))
                tiles = ceil_div(m, 128) * ceil_div(n, 128)
                got = plan(pkg, m, n, k, 0, cus)
                assert got == (eff, sps, eff * tiles * 65536 if eff > 1 else 0), (m, n, k, cus)
                if got[0] > 1:                                                    # whatever the constant is
                    assert tiles * got[0] <= 3 * eff_cus and got[1] >= ms, (m, n, k, cus, got)
    assert plan(pkg, 4096, 4096, 4096, 0, cus) == (1, 64, 0)                             # 1024 tiles: more than 3 x 256 slots


# ---- the split accumulation, restated ------------------------------------------------------------------------------------------------------------
def slab_ordered_partial(a, b, k0, k1):
    """The fast kernel's accumulation over k in [k0, k1) (k0 a multiple of 64): slabs of 64, steps of 16, fragment halves of 8, one fp32 add per exact
    product, from a zero accumulator."""
    acc = np.zeros((a.shape[0], b.shape[0]), F32)
    for kb in range(k0, k1, 64):
        for s in range(0, min(64, k1 - kb), 16):
            for h in (0, 1):
                g = kb + s + 8 * h
                for j in range(8):
                    if g + j < k1:
                        acc = (acc + a[:, g + j, None] * b[None, :, g + j]).astype(F32)
    return acc


def restated_split_product(a, b, alpha, bias_row, splits, mutation=None):
    """a [m][k], b [n][k]: float32 arrays of bf16 values.  S_eff partials over the partition's ranges, the split-ascending fold, then alpha and bias_row."""
    k = a.shape[1]
    eff, sps = partition(k, splits)
    ranges = [(s * sps * 64, min(k, (s + 1) * sps * 64)) for s in range(eff)]
    if mutation == "drop_a_range":
        del ranges[1]
    if mutation == "shared_slab":                                    # split 1 starts one slab early: that slab is counted by both neighbours
        ranges[1] = (ranges[1][0] - 64, ranges[1][1])
    if mutation == "drop_last_short_slab":
        assert k % 64 != 0
        ranges[-1] = (ranges[-1][0], k - k % 64)
    parts = [slab_ordered_partial(a, b, k0, k1) for k0, k1 in ranges]
    if mutation == "epilogue_per_partial":                           # alpha AND the bias applied to every partial: the bias arrives S times
        parts = [((F32(alpha) * p).astype(F32) + bias_row[:, None]).astype(F32) for p in parts]
    acc = parts[0]
    for p in parts[1:]:
        acc = (acc + p).astype(F32)
    if mutation == "epilogue_per_partial":
        return acc
    return ((F32(alpha) * acc).astype(F32) + bias_row[:, None]).astype(F32)


def half_to_one(pkg, rng, shape):
    """bf16 values with magnitudes in [0.5, 1) and random signs, as float32"""
    x = rng.uniform(0.5, 1.0, shape).astype(F32)
    x = np.minimum(pkg.from_bf16(pkg.to_bf16(x)), F32(0.99609375))
    return (x * rng.choice(np.array([-1, 1], F32), shape)).astype(F32)


@pytest.fixture(scope="module")
def split_case(pkg):
    rng = np.random.default_rng(47)
    m, n, k = 24, 17, 328                                 # five whole slabs and one of 8
    a, b, br = half_to_one(pkg, rng, (m, k)), half_to_one(pkg, rng, (n, k)), half_to_one(pkg, rng, m)
    alpha = 0.5
    ref = alpha * (a.astype(F64) @ b.astype(F64).T) + br.astype(F64)[:, None]
    absprod = np.abs(a).astype(F64) @ np.abs(b).astype(F64).T
    bound = (k + 8) * 2.0 ** -23 * alpha * absprod + 2 * 2.0 ** -24 * (np.abs(br).astype(F64)[:, None] + np.abs(ref))
    return dict(a=a, b=b, br=br, alpha=alpha, ref=ref, bound=bound, k=k)


@pytest.mark.parametrize("splits", [1, 2, 3, 4, 6])
def test_restated_split_accumulation_stays_inside_the_bound(split_case, splits):
    c = split_case
    got = restated_split_product(c["a"], c["b"], c["alpha"], c["br"], splits)
    err = np.abs(got.astype(F64) - c["ref"])
    assert (err <= c["bound"]).all(), (err / c["bound"]).max()


def test_one_product_exceeds_the_bound(split_case):
    """Operands in [0.5, 1): a lost or doubled product moves the result by alpha 0.25 at least, a bias added once more by 0.5; the bound is far below."""
    c = split_case
    assert c["bound"].max() < 0.5 * 0.25 / 4


@pytest.mark.parametrize("splits", [3, 6])
@pytest.mark.parametrize("mutation", ["drop_a_range", "shared_slab", "drop_last_short_slab", "epilogue_per_partial"])
def test_mutated_split_accumulation_leaves_the_bound(split_case, splits, mutation):
    c = split_case
    got = restated_split_product(c["a"], c["b"], c["alpha"], c["br"], splits, mutation)
    err = np.abs(got.astype(F64) - c["ref"])
    assert (err > c["bound"]).any(), mutation


# ---- without a device ---------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_are_refused_before_the_device(pkg):
    """Pure argument checks: BLA_ERR_INVALID whether or not a device is there (nothing is launched: the operands are NULL)."""
    L = pkg.lib()
    assert L.bla_gemm_bf16_splitk(None, 0, 1, 8, 8, 8, None, 8, None, 8, None, 8, pkg.C_F32, None, -1) == 1
    assert b"splits" in L.bla_last_error()
    ep = pkg.Epilogue(alpha=1.0, pre_act=0x1000, ld_pre=8)
    assert L.bla_gemm_bf16_splitk(None, 0, 1, 8, 8, 8, None, 8, None, 8, None, 8, pkg.C_F32, C.byref(ep), 2) == 1
    assert b"epilogue" in L.bla_last_error()
    W = L.bla_conv2d_weight_gradient_batched_f32_as_bf16
    assert W(None, None, None, None, 2, 8, 8, 3, 8, 8, 1, 0) == 1
    assert W(None, 0x1000, 0x1000, 0x1000, 2, 8, 8, 3, 8, 8, 1, -1) == 1
    assert W(None, 0x1000, 0x1000, 0x1000, 0, 8, 8, 3, 8, 8, 1, 0) == 1


def test_new_entries_refuse_without_a_device(pkg):
    import torch
    if torch.cuda.is_available() or pkg.lib().bla_device_count() > 0:
        pytest.skip("a device is present")
    L = pkg.lib()
    assert plan(pkg, 128, 1152, 65536, 64) == (64, 16, 64 * 9 * 65536)                   # host only
    for splits in (0, 1, 4):
        assert L.bla_gemm_bf16_splitk(None, 0, 1, 8, 8, 128, None, 8, None, 8, None, 8, pkg.C_F32, None, splits) == 3
        assert L.bla_conv2d_weight_gradient_batched_f32_as_bf16(None, 0x1000, 0x1000, 0x1000, 2, 8, 8, 3, 8, 8, 1, splits) == 3
    assert b"no CPU fallback" in L.bla_last_error() or b"not initialised" in L.bla_last_error()
