"""Several products in one launch (bla_gemm_group_f32, bla_gemm_pair_f32, bla_gemm_batched_f32 on the wave-split-K kernels) and the
epilogue fields that only the MNIST step used to set, each against a float64 numpy product of the same operands.

Tolerances (header of test_gemm_gpu.py / DESIGN.md "tolerances"): fp32 MFMA against float64,
    elementwise |got - ref| <= 1e-5 * (|alpha| |A||B| + |bias| + |beta C0|)
    normwise    ||got - ref||_F <= 1e-5 * ||ref||_F
Outputs written with beta == 0 start as the 0xFF byte pattern (a NaN): every element of the window must be written, and the padding
behind a padded pitch must still hold its bits afterwards.
"""
import ctypes as C
import re

import numpy as np
import pytest

from inputs import uniform

pytestmark = pytest.mark.gpu
RTOL = 1e-5
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def dev(pkg):
    pkg.init(0)
    pkg.lib().bla_gemm_set_config(-1, 0)
    return pkg


def nan_fill(shape):
    return np.full(shape, 0xFFFFFFFF, np.uint32).view(F32)


def same_bits(x, y):
    return x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32))


def last_name(dev):
    return dev.lib().bla_gemm_last_kernel().decode()


def check_close(got, ref, bound, tag):
    err = np.abs(got.astype(F64) - ref)      # an element left at the NaN pattern fails both comparisons
    assert (err <= RTOL * bound + 1e-30).all(), f"{tag}: elementwise excess {np.nanmax(err - RTOL * bound):.3e}, unwritten {int(np.isnan(err).sum())}"
    nr = np.linalg.norm(ref)
    if nr > 0:
        assert np.linalg.norm(err) / nr <= RTOL, f"{tag}: normwise {np.linalg.norm(err) / nr:.3e}"


def softmax_cols64(z):
    e = np.exp(z - z.max(0, keepdims=True))
    return e / e.sum(0, keepdims=True)


class Product:
    """One product op(A) op(B) with its epilogue: host operands (uploaded once), the float64 expectation of every output, and fresh
    device outputs for every run.  pad_* widen a pitch beyond the extent; *_pad = None leaves the field out of the epilogue."""

    def __init__(self, dev, seed, m, n, k, ta=False, tb=True, pad_a=0, pad_b=0, pad_c=0, alpha=1.0, beta=0.0, bias_row=False, bias_col=False,
                 pre_pad=None, relu=False, mask_pad=None, row_sum=None, softmax=False):
        self.dev, self.m, self.n, self.k, self.ta, self.tb = dev, m, n, k, ta, tb
        self.alpha, self.beta, self.relu, self.softmax, self.row_sum = alpha, beta, relu, softmax, row_sum
        ar, ac = (k, m) if ta else (m, k)
        br, bc = (n, k) if tb else (k, n)
        a = uniform(seed, (ar, ac + pad_a), dtype=F32)
        b = uniform(seed + 1, (br, bc + pad_b), dtype=F32)
        self.lda, self.ldb, self.ldc = ac + pad_a, bc + pad_b, n + pad_c
        self.d_a, self.d_b = dev.to_device(a), dev.to_device(b)
        op_a = (a[:, :ac].T if ta else a[:, :ac]).astype(F64)
        op_b = (b[:, :bc].T if tb else b[:, :bc]).astype(F64)
        z = alpha * (op_a @ op_b)
        bound = abs(alpha) * (np.abs(op_a) @ np.abs(op_b))
        self.d_br = self.d_bc = self.d_mask = self.d_y = None
        if bias_row:
            v = uniform(seed + 2, (m,), dtype=F32)
            self.d_br = dev.to_device(v); z = z + v.astype(F64)[:, None]; bound = bound + np.abs(v)[:, None]
        if bias_col:
            v = uniform(seed + 3, (n,), dtype=F32)
            self.d_bc = dev.to_device(v); z = z + v.astype(F64)[None, :]; bound = bound + np.abs(v)[None, :]
        self.z, self.bound_z = z, bound
        self.pre0 = nan_fill((m, n + pre_pad)) if pre_pad is not None else None
        want = np.maximum(z, 0) if relu else z
        if mask_pad is not None:
            mask = uniform(seed + 4, (m, n + mask_pad), dtype=F32)
            self.d_mask = dev.to_device(mask); self.ld_mask = n + mask_pad
            want = want * (mask[:, :n] > 0)
        if beta != 0.0:
            self.c0 = uniform(seed + 5, (m, n + pad_c), dtype=F32)
            want = want + beta * self.c0[:, :n].astype(F64); bound = bound + np.abs(beta * self.c0[:, :n].astype(F64))
        else:
            self.c0 = nan_fill((m, n + pad_c))
        self.want_c, self.bound_c = want, bound
        if softmax:   # C = column softmax of Z, grad = (C - Y) * scale, Y and grad at pitch ldc
            self.scale = 1.0 / 784
            y = np.full((m, n + pad_c), 7.0, F32); y[:, :n] = 0; y[np.arange(n) % m, np.arange(n)] = 1
            self.d_y = dev.to_device(y)
            self.want_c = softmax_cols64(z)
            self.want_g = (self.want_c - y[:, :n]) * self.scale
        if row_sum is not None:
            rs_alpha, rs_beta = row_sum
            eff = 1.0 if rs_alpha == 0.0 and rs_beta == 0.0 else rs_alpha      # both 0 = plain store of the sum
            self.rs0 = uniform(seed + 6, (m,), dtype=F32) if rs_beta != 0.0 else nan_fill((m,))
            old = rs_beta * self.rs0.astype(F64) if rs_beta != 0.0 else np.zeros(m)
            self.want_rs = old + eff * op_a.sum(1)
            self.tol_rs = 2e-6 * (abs(eff) * np.abs(op_a).sum(1) + np.abs(old))

    def fresh(self):
        """Device outputs in their initial state, the epilogue and the descriptor that point at them."""
        dev, nat = self.dev, self.dev.native
        r = {"c": dev.to_device(self.c0)}
        ptr = lambda x: x.ptr if x is not None else None
        if self.pre0 is not None: r["pre"] = dev.to_device(self.pre0)
        if self.row_sum is not None: r["rs"] = dev.to_device(self.rs0)
        if self.softmax: r["grad"] = dev.to_device(nan_fill(self.c0.shape))
        rs_alpha, rs_beta = self.row_sum if self.row_sum is not None else (0.0, 0.0)
        r["ep"] = nat.Epilogue(self.alpha, self.beta, ptr(self.d_br), ptr(self.d_bc), ptr(r.get("pre")), self.pre0.shape[1] if self.pre0 is not None else 0,
                               nat.ACT_RELU if self.relu else nat.ACT_NONE, ptr(self.d_mask), self.ld_mask if self.d_mask is not None else 0,
                               ptr(r.get("rs")), ptr(self.d_y), self.scale if self.softmax else 0.0, ptr(r.get("grad")), rs_alpha, rs_beta, None, None)
        r["desc"] = nat.GemmDesc(int(self.ta), int(self.tb), self.m, self.n, self.k, self.d_a.ptr, self.lda, self.d_b.ptr, self.ldb, r["c"].ptr, self.ldc,
                                 C.pointer(r["ep"]))
        return r

    def solo(self, r):
        """The same product through bla_gemm_f32; returns the kernel name it reports."""
        d = r["desc"]
        self.dev.native.check(self.dev.lib().bla_gemm_f32(None, d.transa, d.transb, d.m, d.n, d.k, d.A, d.lda, d.B, d.ldb, d.C, d.ldc, d.ep))
        return last_name(self.dev)

    @staticmethod
    def read(r):
        return {key: r[key].numpy() for key in ("c", "pre", "rs", "grad") if key in r}

    def check(self, out, tag):
        n = self.n
        if self.softmax:
            assert np.allclose(out["c"][:, :n], self.want_c, rtol=1e-4, atol=1e-7), tag
            assert np.allclose(out["grad"][:, :n], self.want_g, rtol=1e-4, atol=1e-9), tag
            assert same_bits(out["grad"][:, n:], nan_fill((self.m, self.ldc - n))), f"{tag}: softmax_grad padding written"
        else:
            check_close(out["c"][:, :n], self.want_c, self.bound_c, tag + " C")
        assert same_bits(out["c"][:, n:], self.c0[:, n:]), f"{tag}: C padding written"
        if "pre" in out:
            check_close(out["pre"][:, :n], self.z, self.bound_z, tag + " pre_act")
            assert same_bits(out["pre"][:, n:], self.pre0[:, n:]), f"{tag}: pre_act padding written"
        if "rs" in out:
            err = np.abs(out["rs"].astype(F64) - self.want_rs)
            assert (err <= self.tol_rs).all(), f"{tag}: row sums off by {np.nanmax(err / self.tol_rs):.2f} x the tolerance"

    @staticmethod
    def assert_equal(o1, o2, tag):
        assert o1.keys() == o2.keys()
        for key in o1:
            assert same_bits(o1[key], o2[key]), f"{tag}: {key} differs from the separate bla_gemm_f32 call"


def run_group(dev, prods):
    runs = [p.fresh() for p in prods]
    dev.native.gemm_group([r["desc"] for r in runs])
    return last_name(dev), [Product.read(r) for r in runs]


def run_solo(prods):
    runs = [p.fresh() for p in prods]
    names = [p.solo(r) for p, r in zip(prods, runs)]
    return names, [Product.read(r) for r in runs]


def tiles_of(m, n, tile):
    return -(-m // tile) * -(-n // tile)


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. bla_gemm_group_f32
# ----------------------------------------------------------------------------------------------------------------------------------
TRIOS = {
    "mnist": [(10, 128, 256), (128, 256, 256), (256, 784, 256)],      # the three weight gradients of the MNIST step (m, n, k)
    "ragged": [(33, 40, 64), (70, 36, 132), (5, 17, 8)],
    "mixed": [(64, 64, 128), (256, 784, 256), (37, 50, 20)],          # 4 tiles of 32x32 -> 16x16 tiles; 200 -> 32x32 tiles; ragged
}
TRIPLE_NAME = re.compile(r"gemm_f32_wsk_triple_nt_(\d+)x(\d+)\+(\d+)x(\d+)\+(\d+)x(\d+)")


def trio_products(dev, shapes, row_sum):
    (m0, n0, k0), (m1, n1, k1), (m2, n2, k2) = shapes
    return [Product(dev, 100, m0, n0, k0, row_sum=row_sum),
            Product(dev, 200, m1, n1, k1, bias_row=True, pre_pad=0, relu=True),
            Product(dev, 300, m2, n2, k2, alpha=-0.5, beta=2.0, bias_col=True, pre_pad=5, mask_pad=1, pad_c=3)]


@pytest.mark.parametrize("row_sum", [(0.0, 0.0), (0.05, 1.0)], ids=["rowsum_plain", "rowsum_scaled"])
@pytest.mark.parametrize("trio", sorted(TRIOS))
def test_group_three_nt_products_share_one_launch(dev, trio, row_sum):
    """Three NT products, each with another epilogue, in one launch of gemm_f32_wsk_triple_nt_kernel: the workgroup ranges of the name cover
    each product's tiles, results within the bound of float64 and bit-equal to three separate calls (same body, same tile choice)."""
    shapes = TRIOS[trio]
    prods = trio_products(dev, shapes, row_sum)
    name, outs = run_group(dev, prods)
    mt = TRIPLE_NAME.fullmatch(name)
    assert mt, name
    f = [int(x) for x in mt.groups()]
    for i, (m, n, _) in enumerate(shapes):
        assert f[2 * i + 1] in (16, 32) and f[2 * i] == tiles_of(m, n, f[2 * i + 1]), (i, name)
    if trio == "mixed":
        assert (f[1], f[3]) == (16, 32), name
    for i, (p, o) in enumerate(zip(prods, outs)):
        p.check(o, f"{trio} product {i} ({name})")
    _, solo = run_solo(prods)
    for i in range(3):
        Product.assert_equal(outs[i], solo[i], f"{trio} product {i} ({name})")


def plain_trio(dev):
    return [Product(dev, 400, 33, 40, 64), Product(dev, 410, 70, 36, 132, pad_c=3), Product(dev, 420, 5, 17, 8, pad_c=1)]


FALLBACKS = {   # id: (index of the replaced descriptor, its replacement, forced (config, split) or None)
    "tn": (0, lambda d: Product(d, 500, 36, 40, 64, ta=True, tb=False), None),
    "nn": (1, lambda d: Product(d, 510, 70, 36, 132, ta=False, tb=False, pad_c=3), None),
    "k_not_multiple_of_4": (0, lambda d: Product(d, 520, 33, 40, 6), None),
    "pitch_not_multiple_of_4": (1, lambda d: Product(d, 530, 70, 36, 132, pad_a=1, pad_c=3), None),
    "k_cut_over_workgroups": (0, lambda d: Product(d, 540, 32, 32, 2304), None),
    "not_latency_bound": (0, lambda d: Product(d, 550, 768, 768, 64), None),
    "softmax_tail": (1, lambda d: Product(d, 560, 10, 40, 64, bias_row=True, pre_pad=0, pad_c=4, softmax=True), None),
    "forced_config": (None, None, (1, 0)),
    "forced_split": (None, None, (-1, 2)),
}


@pytest.mark.parametrize("case", sorted(FALLBACKS))
def test_group_fallbacks(dev, case):
    """A trio that cannot share the launch is issued product by product: same results, the same float64 check, bit-equal to separate calls, and
    bla_gemm_last_kernel() names the launch this call issued last -- the third product's, exactly as a separate call names it -- not the triple
    launch that ran just before, nor the sibling product that launched while the others were still waiting for a shared launch."""
    idx, make, forced = FALLBACKS[case]
    name0, _ = run_group(dev, plain_trio(dev))
    assert name0.startswith("gemm_f32_wsk_triple_nt_"), name0        # a stale name would show below
    prods = plain_trio(dev)
    if idx is not None:
        prods[idx] = make(dev)
    try:
        if forced:
            dev.native.check(dev.lib().bla_gemm_set_config(*forced))
        name, outs = run_group(dev, prods)
        solo_names, solo = run_solo(prods)
    finally:
        dev.lib().bla_gemm_set_config(-1, 0)
    for i, (p, o) in enumerate(zip(prods, outs)):
        p.check(o, f"{case} product {i} ({name})")
        Product.assert_equal(o, solo[i], f"{case} product {i} ({name})")
    assert "triple" not in name, name
    assert name == solo_names[2], (name, solo_names)
    if idx is not None and case != "softmax_tail":      # (the softmax product's own name equals its neighbours': there the stale name is the witness)
        assert solo_names[idx] != solo_names[2], solo_names
    if forced == (1, 0):
        assert "t64x64x16" in name, name
    if forced == (-1, 2):
        assert solo_names[0].endswith("ksplit2"), solo_names


def test_group_counts_and_errors(dev):
    nat, L = dev.native, dev.lib()
    prods = plain_trio(dev)
    # count 1 is bla_gemm_f32
    r = prods[1].fresh()
    nat.gemm_group([r["desc"]])
    name, out = last_name(dev), Product.read(r)
    prods[1].check(out, "count 1")
    solo_names, solo = run_solo(prods[1:2])
    assert name == solo_names[0] and "triple" not in name and "pair" not in name, (name, solo_names)
    Product.assert_equal(out, solo[0], "count 1")
    # count 2 goes through the pair entry
    runs = [p.fresh() for p in prods[:2]]
    nat.gemm_group([x["desc"] for x in runs])
    assert "_pair_" in last_name(dev), last_name(dev)
    for p, x in zip(prods[:2], runs):
        p.check(Product.read(x), "count 2")
    # count 0, count 4 and a NULL array are refused before anything is launched
    runs = [p.fresh() for p in prods] + [prods[0].fresh()]
    for descs in ([], [x["desc"] for x in runs]):
        with pytest.raises(dev.BlaError) as e:
            nat.gemm_group(descs)
        assert e.value.status == 1
    assert L.bla_gemm_group_f32(None, None, 3) == 1
    # a descriptor whose lda is too small
    runs[2]["desc"].lda = prods[2].k - 1
    with pytest.raises(dev.BlaError) as e:
        nat.gemm_group([x["desc"] for x in runs[2:3]])
    assert e.value.status == 1
    for p, x in zip(prods + [prods[0]], runs):
        assert same_bits(x["c"].numpy(), p.c0), "a refused call wrote to C"
    with pytest.raises(dev.BlaError) as e:      # ... also as the last of three
        nat.gemm_group([x["desc"] for x in runs[:3]])
    assert e.value.status == 1
    assert same_bits(runs[2]["c"].numpy(), prods[2].c0)


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. bla_gemm_pair_f32
# ----------------------------------------------------------------------------------------------------------------------------------
PAIR_NAME = re.compile(r"gemm_f32_wsk_pair_([nt]{2})\+([nt]{2})_(\d+)x(\d+)\+(\d+)x(\d+)")


def run_pair(dev, prods):
    runs = [p.fresh() for p in prods]
    dev.native.gemm_pair(runs[0]["desc"], runs[1]["desc"])
    return last_name(dev), [Product.read(r) for r in runs]


def check_pair(dev, prods, tag):
    name, outs = run_pair(dev, prods)
    solo_names, solo = run_solo(prods)
    for i in range(2):
        prods[i].check(outs[i], f"{tag} member {i} ({name})")
        Product.assert_equal(outs[i], solo[i], f"{tag} member {i} ({name})")
    return name, solo_names


@pytest.mark.parametrize("order", [0, 1])
def test_pair_mixed_tiles_with_epilogues(dev, order):
    """A product on 16x16 tiles (4 tiles of 32x32) beside one on 32x32 tiles (132 of them) in one launch, each with its own wsk_tile; bias_row +
    ReLU + pre_act on one side, alpha / beta / bias_col with padded pitches on the other."""
    small = Product(dev, 600, 40, 52, 72, ta=False, tb=True, bias_row=True, relu=True, pre_pad=0)
    large = Product(dev, 610, 92, 1380, 36, ta=True, tb=False, alpha=-0.5, beta=2.0, bias_col=True, pad_a=4, pad_b=8, pad_c=3)
    prods = [small, large] if order == 0 else [large, small]
    name, _ = check_pair(dev, prods, "mixed tiles")
    mt = PAIR_NAME.fullmatch(name)
    assert mt, name
    want = [("nt", tiles_of(40, 52, 16), 16), ("tn", tiles_of(92, 1380, 32), 32)]
    if order == 1:
        want.reverse()
    got = [(mt.group(1), int(mt.group(3)), int(mt.group(4))), (mt.group(2), int(mt.group(5)), int(mt.group(6)))]
    assert got == want, name


@pytest.mark.parametrize("order", [0, 1])
def test_pair_planned_member_beside_unplanned(dev, order):
    """One member fits the shared launch, the other (k = 6: scalar loads) launches on its own; the planned one then goes alone, last, and gives
    the call its name."""
    planned = Product(dev, 620, 33, 40, 64, bias_row=True, pre_pad=2, pad_c=3)
    scalar = Product(dev, 630, 20, 24, 6, alpha=0.5, beta=-1.0, pad_c=1)
    shared, _ = run_pair(dev, [Product(dev, 640, 33, 40, 64), Product(dev, 650, 70, 36, 132)])
    assert PAIR_NAME.fullmatch(shared), shared
    prods = [planned, scalar] if order == 0 else [scalar, planned]
    name, solo_names = check_pair(dev, prods, "planned + unplanned")
    assert "_ss_" in solo_names[1 - order] and "_vv_" in solo_names[order], solo_names
    assert name == solo_names[order], (name, solo_names)     # either way the planned member is the last launch of the call


@pytest.mark.parametrize("order", [0, 1])
def test_pair_member_with_softmax_tail(dev, order):
    """The fused softmax tail keeps a planned product out of the shared launch: both planned products launch alone, one after the other."""
    sm = Product(dev, 660, 10, 40, 64, tb=False, bias_row=True, pre_pad=0, pad_c=4, softmax=True)     # NN, as the output layer
    other = Product(dev, 670, 70, 36, 132, bias_row=True, relu=True, pre_pad=1, pad_c=3)
    shared, _ = run_pair(dev, [Product(dev, 640, 33, 40, 64), Product(dev, 650, 70, 36, 132)])
    assert PAIR_NAME.fullmatch(shared), shared
    prods = [sm, other] if order == 0 else [other, sm]
    name, solo_names = check_pair(dev, prods, "softmax member")
    assert "pair" not in name and name == solo_names[1], (name, solo_names)
    assert solo_names[0] != solo_names[1], solo_names


# ----------------------------------------------------------------------------------------------------------------------------------
# 3. bla_gemm_batched_f32 on the wave-split-K batched kernel
# ----------------------------------------------------------------------------------------------------------------------------------
BATCHED_NAME = re.compile(r"gemm_f32_wsk_batched_([nt]{2})_(\d+)x(\d+)_x(\d+)")


def up4(x):
    return (x + 3) // 4 * 4


class Batched:
    """`batch` operand sets at fixed strides with the full epilogue the batched entry takes: alpha, beta, bias_row, bias_col, ReLU and pre_act,
    ldc > n, stride_c > m * ldc and another stride for pre_act."""

    def __init__(self, dev, seed, batch, m, n, k, ta, tb, share=None, odd_stride_a=False):
        self.dev, self.batch, self.m, self.n, self.k, self.ta, self.tb = dev, batch, m, n, k, ta, tb
        ar, ac = (k, m) if ta else (m, k)
        br, bc = (n, k) if tb else (k, n)
        self.lda, self.ldb, self.ldc, self.ld_pre = ac, bc, n + 3, n + 1
        self.sa = 0 if share == "a" else ar * ac + (1 if odd_stride_a else 4)
        self.sb = 0 if share == "b" else br * bc + 8
        self.sc, self.spre = up4(m * self.ldc) + 8, up4(m * self.ld_pre) + 4
        assert self.sc > m * self.ldc and self.spre != self.sc
        a = uniform(seed, ((batch - 1) * self.sa + ar * ac,), dtype=F32)
        b = uniform(seed + 1, ((batch - 1) * self.sb + br * bc,), dtype=F32)
        self.bias_r, self.bias_c = uniform(seed + 2, (m,), dtype=F32), uniform(seed + 3, (n,), dtype=F32)
        self.c0 = uniform(seed + 4, (batch * self.sc,), dtype=F32)
        self.pre0 = nan_fill((batch * self.spre,))
        self.alpha, self.beta = 0.75, -1.5
        self.d_a, self.d_b, self.d_br, self.d_bc = (dev.to_device(x) for x in (a, b, self.bias_r, self.bias_c))
        self.want_c, self.want_pre = self.c0.astype(F64), np.zeros(batch * self.spre)
        self.bound_c, self.bound_pre = np.zeros(batch * self.sc), np.zeros(batch * self.spre)
        self.win_c, self.win_pre = np.zeros(batch * self.sc, bool), np.zeros(batch * self.spre, bool)
        for i in range(batch):
            op_a = a[i * self.sa:i * self.sa + ar * ac].reshape(ar, ac).astype(F64)
            op_b = b[i * self.sb:i * self.sb + br * bc].reshape(br, bc).astype(F64)
            op_a = op_a.T if ta else op_a
            op_b = op_b.T if tb else op_b
            z = self.alpha * (op_a @ op_b) + self.bias_r.astype(F64)[:, None] + self.bias_c.astype(F64)[None, :]
            bz = self.alpha * (np.abs(op_a) @ np.abs(op_b)) + np.abs(self.bias_r)[:, None] + np.abs(self.bias_c)[None, :]
            ci = (i * self.sc + np.arange(m)[:, None] * self.ldc + np.arange(n)[None, :]).ravel()
            pi = (i * self.spre + np.arange(m)[:, None] * self.ld_pre + np.arange(n)[None, :]).ravel()
            old = self.beta * self.c0[ci].astype(F64)
            self.want_c[ci] = np.maximum(z, 0).ravel() + old
            self.bound_c[ci] = bz.ravel() + np.abs(old)
            self.want_pre[pi], self.bound_pre[pi] = z.ravel(), bz.ravel()
            self.win_c[ci] = True; self.win_pre[pi] = True

    def epilogue(self, pre):
        nat = self.dev.native
        return nat.Epilogue(self.alpha, self.beta, self.d_br.ptr, self.d_bc.ptr, pre.ptr if pre is not None else None, self.ld_pre, nat.ACT_RELU,
                            None, 0, None, None, 0.0, None, 0.0, 0.0, None, None)

    def run(self):
        dev = self.dev
        c, pre = dev.to_device(self.c0), dev.to_device(self.pre0)
        dev.native.gemm_batched(self.d_a, self.d_b, c, self.batch, self.m, self.n, self.k, self.lda, self.sa, self.ldb, self.sb, self.ldc, self.sc,
                                transa=self.ta, transb=self.tb, epilogue=self.epilogue(pre), stride_pre=self.spre)
        return last_name(dev), c.numpy(), pre.numpy()

    def run_set_by_set(self):
        """Per-set bla_gemm_f32 calls on the same operands, pre_act of set i at i * stride_pre."""
        dev, L = self.dev, self.dev.lib()
        c, pre = dev.to_device(self.c0), dev.to_device(self.pre0)
        ep = self.epilogue(pre)
        for i in range(self.batch):
            ep.pre_act = pre.ptr + 4 * i * self.spre
            dev.native.check(L.bla_gemm_f32(None, int(self.ta), int(self.tb), self.m, self.n, self.k, self.d_a.ptr + 4 * i * self.sa, self.lda,
                                            self.d_b.ptr + 4 * i * self.sb, self.ldb, c.ptr + 4 * i * self.sc, self.ldc, C.byref(ep)))
        return c.numpy(), pre.numpy()

    def check(self, c, pre, tag):
        check_close(c[self.win_c], self.want_c[self.win_c], self.bound_c[self.win_c], tag + " C")
        check_close(pre[self.win_pre], self.want_pre[self.win_pre], self.bound_pre[self.win_pre], tag + " pre_act")
        for i in range(self.batch):   # every set's pre_act at its own offset (a set written to another's place leaves this one at the NaN pattern)
            w = slice(i * self.spre, (i + 1) * self.spre)
            assert not np.isnan(pre[w][self.win_pre[w]]).any(), f"{tag}: pre_act of set {i} not written"
        assert same_bits(c[~self.win_c], self.c0[~self.win_c]), f"{tag}: C written outside the windows"
        assert same_bits(pre[~self.win_pre], self.pre0[~self.win_pre]), f"{tag}: pre_act written outside the windows"


# (batch, m, n, k, tile): tiles32 * batch = 6 and 28 stay below 129 -> 16x16 tiles; 4 * 33 = 132 does not -> 32x32 tiles
BATCHED_SHAPES = [(3, 36, 20, 44, 16), (7, 64, 64, 16, 16), (33, 64, 64, 16, 32)]


@pytest.mark.parametrize("batch,m,n,k,tile", BATCHED_SHAPES)
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_batched_wsk_kernel_full_epilogue(dev, ta, tb, batch, m, n, k, tile):
    for share in (None, "a", "b"):
        job = Batched(dev, 700, batch, m, n, k, bool(ta), bool(tb), share=share)
        name, c, pre = job.run()
        mt = BATCHED_NAME.fullmatch(name)
        assert mt, name
        assert (mt.group(1), int(mt.group(2)), int(mt.group(3)), int(mt.group(4))) == ("nt"[ta] + "nt"[tb], tiles_of(m, n, tile), tile, batch), name
        job.check(c, pre, f"batched {name} share={share}")


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("route", ["odd_stride_a", "forced_config"])
def test_batched_set_by_set_route(dev, route, ta, tb):
    """A stride that is no multiple of 4, or a forced configuration, sends the sets out one by one: the first by the planning call, the others with
    pre_act moved along by hand.  Bit-equal to per-set bla_gemm_f32 calls, every set's pre_act at its own offset."""
    job = Batched(dev, 720, 3, 36, 20, 44, bool(ta), bool(tb), odd_stride_a=route == "odd_stride_a")
    try:
        if route == "forced_config":
            dev.native.check(dev.lib().bla_gemm_set_config(1, 0))
        name, c, pre = job.run()
        c2, pre2 = job.run_set_by_set()
        name2 = last_name(dev)
    finally:
        dev.lib().bla_gemm_set_config(-1, 0)
    assert "batched" not in name and name == name2, (name, name2)
    if route == "forced_config":
        assert "t64x64x16" in name, name
    job.check(c, pre, f"set by set ({route}, {name})")
    assert same_bits(c, c2) and same_bits(pre, pre2), name


def test_batched_refusals(dev):
    nat, L = dev.native, dev.lib()
    job = Batched(dev, 740, 3, 36, 20, 44, False, True)
    c, pre, aux = dev.to_device(job.c0), dev.to_device(job.pre0), dev.zeros((job.batch * job.sc,))
    for field in ("relu_mask", "row_sum_a", "softmax_grad"):
        ep = job.epilogue(pre)
        setattr(ep, field, aux.ptr)
        if field == "relu_mask":
            ep.ld_mask = job.ldc
        if field == "softmax_grad":
            ep.softmax_y = aux.ptr
        st = L.bla_gemm_batched_f32(None, 0, 1, job.m, job.n, job.k, job.d_a.ptr, job.lda, job.sa, job.d_b.ptr, job.ldb, job.sb, c.ptr, job.ldc, job.sc,
                                    job.batch, C.byref(ep), job.spre)
        assert st == 1, field
    ep = job.epilogue(pre)
    st = L.bla_gemm_batched_f32(None, 0, 1, job.m, job.n, job.k, job.d_a.ptr, job.lda, job.sa, job.d_b.ptr, job.ldb, job.sb, c.ptr, job.ldc, job.sc,
                                0, C.byref(ep), job.spre)
    assert st == 1
    assert same_bits(c.numpy(), job.c0) and same_bits(pre.numpy(), job.pre0) and not aux.numpy().any()


# ----------------------------------------------------------------------------------------------------------------------------------
# 4. Epilogue fields
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [6, 16, -1])
def test_scaled_row_sum_accumulates_over_two_calls(dev, cfg):
    """row_sum_a[r] = row_sum_beta * row_sum_a[r] + row_sum_alpha * sum_k A[r][k] on the wave-split-K kernels (three tile rows, the last ragged;
    only the first tile column writes).  Each call is checked against the vector the device held before it."""
    m, k, n = (72 if cfg == 16 else 70), 96, 40
    a = uniform(31, (m, k), dtype=F32); b = uniform(32, (n, k), dtype=F32)
    sums, mags = a.astype(F64).sum(1), np.abs(a.astype(F64)).sum(1)
    da, db = dev.to_device(a), dev.to_device(b)
    try:
        dev.native.check(dev.lib().bla_gemm_set_config(cfg, 0))
        for rs_alpha, rs_beta in [(0.05, 1.0), (-2.0, 0.5), (0.05, 0.0)]:
            old = uniform(33, (m,), dtype=F32) if rs_beta != 0.0 else nan_fill((m,))     # beta == 0 must not read the vector
            rs = dev.to_device(old)
            for call in range(2):
                c = dev.to_device(nan_fill((m, n + 3)))
                dev.gemm(da, db, c, transb=True, n=n, row_sum_a=rs, row_sum_alpha=rs_alpha, row_sum_beta=rs_beta)
                assert "wsk" in last_name(dev), last_name(dev)
                got = rs.numpy()
                prev = rs_beta * old.astype(F64) if rs_beta != 0.0 else np.zeros(m)
                err = np.abs(got.astype(F64) - (prev + rs_alpha * sums))
                tol = 2e-6 * (abs(rs_alpha) * mags + np.abs(prev))
                assert (err <= tol).all(), (cfg, rs_alpha, rs_beta, call, np.nanmax(err / tol))
                out = c.numpy()
                check_close(out[:, :n], a.astype(F64) @ b.astype(F64).T, np.abs(a.astype(F64)) @ np.abs(b.astype(F64)).T, f"cfg {cfg}")
                assert same_bits(out[:, n:], nan_fill((m, 3)))
                old = got
    finally:
        dev.lib().bla_gemm_set_config(-1, 0)


@pytest.mark.parametrize("cfg", [1, 4])
def test_tiled_configurations_refuse_scaled_row_sum(dev, cfg):
    """The tiled kernels run the row sum as a pass of its own behind the product: the plain form only."""
    m, k, n = 70, 96, 40
    a = uniform(31, (m, k), dtype=F32); b = uniform(32, (n, k), dtype=F32)
    da, db = dev.to_device(a), dev.to_device(b)
    try:
        dev.native.check(dev.lib().bla_gemm_set_config(cfg, 0))
        for rs_alpha, rs_beta in [(0.05, 1.0), (0.05, 0.0), (0.0, 1.0)]:
            rs, c = dev.to_device(nan_fill((m,))), dev.to_device(nan_fill((m, n)))
            with pytest.raises(dev.BlaError) as e:
                dev.gemm(da, db, c, transb=True, row_sum_a=rs, row_sum_alpha=rs_alpha, row_sum_beta=rs_beta)
            assert e.value.status == 1
            assert same_bits(rs.numpy(), nan_fill((m,))) and same_bits(c.numpy(), nan_fill((m, n)))
        rs, c = dev.to_device(nan_fill((m,))), dev.to_device(nan_fill((m, n + 3)))
        dev.gemm(da, db, c, transb=True, n=n, row_sum_a=rs)
        assert ("t64x64x16" if cfg == 1 else "glds64x64x16") in last_name(dev), last_name(dev)
    finally:
        dev.lib().bla_gemm_set_config(-1, 0)
    assert (np.abs(rs.numpy().astype(F64) - a.astype(F64).sum(1)) <= 2e-6 * np.abs(a.astype(F64)).sum(1)).all()
    out = c.numpy()
    check_close(out[:, :n], a.astype(F64) @ b.astype(F64).T, np.abs(a.astype(F64)) @ np.abs(b.astype(F64)).T, f"cfg {cfg}")
    assert same_bits(out[:, n:], nan_fill((m, 3)))


@pytest.mark.parametrize("cfg,m,k,n,seed", [(6, 10, 128, 300, 41), (6, 32, 64, 70, 81), (6, 1, 8, 33, 41), (16, 16, 96, 44, 41)])
def test_softmax_tail_with_bookkeeping(dev, cfg, m, k, n, seed):
    """Z = alpha W X + b (kept), P = column softmax, grad = (P - Y) * scale with Y and grad at pitch ldc = n + 4, and the per-column loss /
    accuracy accumulators, called twice on the same accumulators.

    softmax_correct_acc must equal the float64 count exactly: the test first asserts on the reference alone that every column's top-two
    probability margin exceeds 4e-5 * max_r bound[r, c], so the device's argmax cannot legitimately differ.
    softmax_loss_acc: per column within 2 * max_r(1e-5 * bound[r, c]) + 1e-5 of -sum y log(p + 1e-15): |d loss| <= 2 max|dz|, plus fp32 expf,
    the subtraction at |z - max| up to ~20, the sum over at most 32 terms and the divide.  The largest observed ratio is printed."""
    alpha, scale, ldc = 0.75, 1.0 / 784, n + 4
    w = uniform(seed, (m, k), dtype=F32); x = uniform(seed + 1, (k, n), -2, 2, F32); b = uniform(seed + 2, (m, 1), dtype=F32)
    w64, x64, b64 = w.astype(F64), x.astype(F64), b.astype(F64)
    z64 = alpha * (w64 @ x64) + b64
    bound = alpha * (np.abs(w64) @ np.abs(x64)) + np.abs(b64)
    p64 = softmax_cols64(z64)
    top = np.sort(p64, axis=0)
    margin = top[-1] - (top[-2] if m > 1 else 0.0)
    assert (margin > 4e-5 * bound.max(0)).all(), (margin.min(), (4e-5 * bound.max(0)).max())
    am, cols = p64.argmax(0), np.arange(n)
    y = np.full((m, ldc), 7.0, F32); y[:, :n] = 0        # the padding would spoil grad, loss and count if it were read as a label
    y[am[::2], cols[::2]] = 1                            # every second column labelled with the prediction ...
    if m > 1:
        y[(am[1::2] + 1) % m, cols[1::2]] = 1            # ... the others with its neighbour (one row only: no label at all)
    correct = (y[am, cols] == 1).astype(np.uint32)
    assert correct.min() == 0 and correct.max() == 1
    loss64 = -(y[:, :n].astype(F64) * np.log(p64 + 1e-15)).sum(0)
    tol_loss = 2 * (1e-5 * bound).max(0) + 1e-5
    dw, dx, db, dy = (dev.to_device(v) for v in (w, x, b, y))
    d_loss, d_corr = dev.zeros((n,), F64), dev.zeros((n,), np.uint32)
    seen = []
    try:
        dev.native.check(dev.lib().bla_gemm_set_config(cfg, 0))
        for call in range(2):
            z, p, g = (dev.to_device(nan_fill(s)) for s in ((m, n + 1), (m, ldc), (m, ldc)))
            dev.gemm(dw, dx, p, n=n, alpha=alpha, bias_row=db, pre_act=z, softmax_y=dy, softmax_scale=scale, softmax_grad=g,
                     softmax_loss_acc=d_loss, softmax_correct_acc=d_corr)
            assert f"wsk{32 if cfg == 6 else 16}x" in last_name(dev), last_name(dev)
            seen.append((z.numpy(), p.numpy(), g.numpy(), d_loss.numpy(), d_corr.numpy()))
    finally:
        dev.lib().bla_gemm_set_config(-1, 0)
    for call, (z, p, g, loss, corr) in enumerate(seen):
        check_close(z[:, :n], z64, bound, f"Z call {call}")
        assert np.allclose(p[:, :n], p64, rtol=1e-4, atol=1e-7)
        assert np.allclose(g[:, :n], (p64 - y[:, :n]) * scale, rtol=1e-4, atol=1e-9)
        assert same_bits(z[:, n:], nan_fill((m, 1))) and same_bits(p[:, n:], nan_fill((m, 4))) and same_bits(g[:, n:], nan_fill((m, 4)))
    assert same_bits(dy.numpy(), y)
    loss1, corr1 = seen[0][3], seen[0][4]
    assert np.array_equal(corr1, correct), np.flatnonzero(corr1 != correct)
    ratio = np.abs(loss1 - loss64) / tol_loss
    print(f"softmax_loss_acc cfg {cfg} {m}x{k}x{n}: largest |loss - ref| / tolerance = {ratio.max():.3e}")
    assert (ratio <= 1).all(), ratio.max()
    assert np.array_equal(seen[1][3], 2 * loss1) and np.array_equal(seen[1][4], 2 * corr1)       # exactly twice after the second call
    for i in range(3):
        assert same_bits(seen[0][i], seen[1][i])


def test_softmax_bookkeeping_validation(dev):
    m, k, n = 10, 16, 12
    w, x, y, p, g = (dev.zeros(s) for s in ((m, k), (k, n), (m, n), (m, n), (m, n)))
    loss, corr = dev.zeros((n,), F64), dev.zeros((n,), np.uint32)
    bad = [dict(softmax_y=y, softmax_grad=g, softmax_loss_acc=loss),                       # one accumulator without the other
           dict(softmax_y=y, softmax_grad=g, softmax_correct_acc=corr),
           dict(softmax_loss_acc=loss, softmax_correct_acc=corr)]                         # accumulators without the softmax tail
    for kw in bad:
        with pytest.raises(dev.BlaError) as e:
            dev.gemm(w, x, p, **kw)
        assert e.value.status == 1, kw.keys()
    w33, y33, p33, g33 = (dev.zeros(s) for s in ((33, k), (33, n), (33, n), (33, n)))
    with pytest.raises(dev.BlaError) as e:                                                 # m = 33: a column no longer fits one tile
        dev.gemm(w33, x, p33, softmax_y=y33, softmax_grad=g33, softmax_loss_acc=loss, softmax_correct_acc=corr)
    assert e.value.status == 1
    dev.gemm(w, x, p, softmax_y=y, softmax_grad=g, softmax_loss_acc=loss, softmax_correct_acc=corr)   # the complete form is accepted
    assert np.allclose(p.numpy(), 1.0 / m) and not corr.numpy().any()
