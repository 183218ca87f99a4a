"""bla_conv2d_weight_gradient_batched_f32_as_bf16 on the device: the materialised bf16 weight gradient with its product K-split (include/bla.h).

For every case and splits in {0, 1, 2, 3}:
* integer operands (-4..4, exact in bf16; every partial sum far below 2^24): del_kern equals an int64 numpy weight gradient bit for bit;
* operands uniform [-1, 1) rounded to bf16: per element, against float64, with Np = B Ho Wo rounded up to 8,
      |got - ref| <= (Np + 8) 2^-23 (|del_y| * |x|) + 2 2^-24 |ref|
  -- the bound of the unsplit product (the fold's S - 1 adds are paid for by the shorter partial sums, see test_bf16_splitk_gpu.py); worst ratio printed;
* splits = 1 equals del_kern of bla_conv2d_backward_batched_f32_as_bf16 bit for bit;
* every splits equals bla_gemm_bf16_splitk (nt, the same splits) on a host-made dY16 [F][Np] and bf16 im2col G [C k k][Np], bit for bit, and names the
  same kernel; the name ends in _splitk<S_eff> exactly when S_eff > 1 (partition rule restated; splits = 0: the plan entry for the device's CU count);
* the output starts as 0xFF bytes between guards, which keep their bits; a second run is bit-identical.
NULL pointers, negative splits and bad extents are refused with the output untouched.
The SAME geometry and the im2col are restated here; nothing is imported from another test file.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F32, F64, U16, U32, I64 = np.float32, np.float64, np.uint16, np.uint32, np.int64
GUARD = 64
SPLITS = [0, 1, 2, 3]
#        B   C    F   H  W  k  s
CASES = [(2, 16, 130, 9, 9, 3, 1),     # n = 162 -> pitch 168, 3 slabs; two row tiles
         (5, 64, 128, 8, 8, 3, 1),     # n = 320 -> 5 slabs; several column tiles
         (2, 8, 8, 8, 8, 3, 2),        # stride 2, n = 32 -> one slab: S_eff = 1 whatever is asked
         (1, 8, 8, 6, 6, 5, 1)]        # k = 5
IDS = ["B%d_C%d_F%d_%dx%d_k%d_s%d" % c for c in CASES]
UNSPLIT = "gemm_bf16_mfma128x128x64_nt_f32"


@pytest.fixture(scope="module")
def dev(pkg):
    pkg.init(0)
    return pkg


# ---- geometry and im2col, restated ---------------------------------------------------------------------------------------------------------------------
def same_geometry(h, w, k, s):
    ho, wo = int(np.ceil(F32(h) / F32(s))), int(np.ceil(F32(w) / F32(s)))
    vpad, hpad = max((ho - 1) * s + k - h, 0), max((wo - 1) * s + k - w, 0)
    return ho, wo, vpad // 2, hpad // 2


def round8(x):
    return -(-x // 8) * 8


def partition(k, splits):
    slabs = -(-k // 64)
    s = min(max(splits, 1), slabs)
    sps = -(-slabs // s)
    return -(-slabs // sps), sps


def im2col(x, k, s):
    """x [B][C][H][W] -> cols [B][Ho Wo][C k k], cols[b][(i, j)][(c, p, q)] = x[b][c][i s + p - pt][j s + q - pl], 0 outside."""
    B, Cn, h, w = x.shape
    ho, wo, pt, pl = same_geometry(h, w, k, s)
    xp = np.zeros((B, Cn, h + 2 * k + s, w + 2 * k + s), x.dtype)
    xp[:, :, pt:pt + h, pl:pl + w] = x
    cols = np.zeros((B, ho, wo, Cn, k, k), x.dtype)
    for p in range(k):
        for q in range(k):
            cols[:, :, :, :, p, q] = xp[:, :, p:p + (ho - 1) * s + 1:s, q:q + (wo - 1) * s + 1:s].transpose(0, 2, 3, 1)
    return cols.reshape(B, ho * wo, Cn * k * k)


def weight_gradient(x, dy, k, s):
    """del_kern [F][C][k][k] in the inputs' dtype (float64 or int64)"""
    B, Fn = dy.shape[:2]
    return np.einsum("bfn,bnk->fk", dy.reshape(B, Fn, -1), im2col(x, k, s)).reshape(Fn, x.shape[1], k, k)


class Out:
    """`shape` elements that start as 0xFF bytes (fp32: a NaN) with GUARD elements of the same pattern on either side."""

    def __init__(self, dev, shape):
        self.shape, self.n = shape, int(np.prod(shape))
        self.arr = dev.DeviceArray((self.n + 2 * GUARD,), U32).fill_bytes(0xFF)
        self.ptr = self.arr.ptr + GUARD * 4

    def read(self):
        now = self.arr.numpy()
        assert (now[:GUARD] == 0xFFFFFFFF).all() and (now[GUARD + self.n:] == 0xFFFFFFFF).all(), "a guard element changed"
        return now[GUARD:GUARD + self.n].reshape(self.shape).view(F32).copy()

    def untouched(self):
        return (self.arr.numpy() == 0xFFFFFFFF).all()


def last_name(dev):
    return dev.lib().bla_gemm_last_kernel().decode()


def wgrad(dev, g, case, out, splits, want=0):
    B, Cn, Fn, h, w, k, s = case
    st = dev.lib().bla_conv2d_weight_gradient_batched_f32_as_bf16(None, g["dy"].ptr, g["x"].ptr, out.ptr, B, h, w, k, Cn, Fn, s, splits)
    assert st == want, (st, dev.lib().bla_last_error())
    dev.sync()
    return last_name(dev)


_cache = {}


def case_data(dev, case, kind):
    key = (case, kind)
    if key in _cache:
        return _cache[key]
    B, Cn, Fn, h, w, k, s = case
    ho, wo = same_geometry(h, w, k, s)[:2]
    rng = np.random.default_rng(2000 + CASES.index(case))
    shapes = dict(x=(B, Cn, h, w), dy=(B, Fn, ho, wo))
    if kind == "exact":
        v = {n: rng.integers(-4, 5, sh).astype(F32) for n, sh in shapes.items()}
        d = dict(v, dkern=weight_gradient(v["x"].astype(I64), v["dy"].astype(I64), k, s).astype(F32))
    else:
        v = {n: dev.from_bf16(dev.to_bf16(rng.uniform(-1, 1, sh).astype(F32))) for n, sh in shapes.items()}
        dkern = weight_gradient(v["x"].astype(F64), v["dy"].astype(F64), k, s)
        adkern = weight_gradient(np.abs(v["x"]).astype(F64), np.abs(v["dy"]).astype(F64), k, s)
        d = dict(v, dkern=dkern, bound=(round8(B * ho * wo) + 8) * 2.0 ** -23 * adkern + 2 * 2.0 ** -24 * np.abs(dkern))
    d["dev"] = {n: dev.to_device(d[n]) for n in shapes}
    # the product's operands, made on the host: dY16 [F][Np], G [C k k][Np], tails zero
    n, n8 = B * ho * wo, round8(B * ho * wo)
    G = np.zeros((Cn * k * k, n8), U16)
    G[:, :n] = dev.to_bf16(im2col(d["x"], k, s).transpose(2, 0, 1).reshape(Cn * k * k, n))
    dy16 = np.zeros((Fn, n8), U16)
    dy16[:, :n] = dev.to_bf16(d["dy"].reshape(B, Fn, ho * wo).transpose(1, 0, 2).reshape(Fn, n))
    d["dev"]["G"], d["dev"]["dy16"] = dev.to_device(G, U16), dev.to_device(dy16, U16)
    d["np"] = n8
    _cache[key] = d
    return d


def device_cus(dev):
    """the context's CU count, as bla_device_name reports it: "<arch> (<n> CUs)" """
    import ctypes
    import re
    buf = ctypes.create_string_buffer(128)
    assert dev.lib().bla_device_name(buf, 128) == 0
    return int(re.search(rb"\((\d+) CUs\)", buf.value).group(1))


def expected_eff(dev, case, d, splits):
    B, Cn, Fn, h, w, k, s = case
    if splits == 0:
        return dev.gemm_bf16_splitk_plan(Fn, Cn * k * k, d["np"], 0, device_cus(dev))[0]
    return partition(d["np"], splits)[0]


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_integer_operands_are_exact(dev, case, splits):
    d = case_data(dev, case, "exact")
    out = Out(dev, d["dkern"].shape)
    name = wgrad(dev, d["dev"], case, out, splits)
    eff = expected_eff(dev, case, d, splits)
    assert name == UNSPLIT + ("_splitk%d" % eff if eff > 1 else ""), (name, eff)
    got = out.read()
    assert np.array_equal(got.view(U32), d["dkern"].view(U32)), f"{name}: {int((got != d['dkern']).sum())} elements differ"


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rounded_operands_against_float64_and_the_composition(dev, case, splits):
    B, Cn, Fn, h, w, k, s = case
    d = case_data(dev, case, "rounded")
    g = d["dev"]
    out = Out(dev, d["dkern"].shape)
    name = wgrad(dev, g, case, out, splits)
    got = out.read()
    err = np.abs(got.astype(F64) - d["dkern"])                  # an element left at the NaN pattern fails the comparison
    ratio = float(np.nanmax(err / np.maximum(d["bound"], 1e-300)))
    print("conv_bf16 weight gradient %s splits %d %s: worst |err| / bound = %.4f" % ("B%d_C%d_F%d_%dx%d_k%d_s%d" % case, splits, name, ratio))
    assert (err <= d["bound"]).all(), (name, ratio, int(np.isnan(err).sum()))
    # the composition: bla_gemm_bf16_splitk, nt, the same splits, on the host-made operands
    mine = Out(dev, (Fn, Cn * k * k))
    st = dev.lib().bla_gemm_bf16_splitk(None, 0, 1, Fn, Cn * k * k, d["np"], g["dy16"].ptr, d["np"], g["G"].ptr, d["np"], mine.ptr, Cn * k * k, dev.C_F32, None, splits)
    assert st == 0, dev.lib().bla_last_error()
    dev.sync()
    assert last_name(dev) == name
    eff = expected_eff(dev, case, d, splits)
    assert name.endswith("_splitk%d" % eff) if eff > 1 else name == UNSPLIT, (name, eff)
    assert np.array_equal(mine.read().reshape(got.shape).view(U32), got.view(U32))
    if splits == 1:                                             # the backward entry's own weight gradient
        theirs = Out(dev, d["dkern"].shape)
        st = dev.lib().bla_conv2d_backward_batched_f32_as_bf16(None, g["dy"].ptr, g["x"].ptr, None, theirs.ptr, None, B, h, w, k, Cn, Fn, s)
        assert st == 0, dev.lib().bla_last_error()
        dev.sync()
        assert last_name(dev) == name and np.array_equal(theirs.read().view(U32), got.view(U32))
    # again, after the products above have used the workspace
    again = Out(dev, d["dkern"].shape)
    assert wgrad(dev, g, case, again, splits) == name
    assert np.array_equal(again.read().view(U32), got.view(U32))


def test_python_helper(dev):
    case = CASES[0]
    B, Cn, Fn, h, w, k, s = case
    d = case_data(dev, case, "exact")
    out = dev.conv2d_weight_gradient_as_bf16(d["dev"]["dy"], d["dev"]["x"], dev.empty((Fn, Cn, k, k)), B, h, w, k, Cn, Fn, s, splits=3)
    dev.sync()
    assert last_name(dev) == UNSPLIT + "_splitk3" and np.array_equal(out.numpy(), d["dkern"])


def test_argument_refusals_leave_the_output_alone(dev):
    case = (2, 8, 8, 6, 6, 3, 1)
    B, Cn, Fn, h, w, k, s = case
    g = dict(x=dev.zeros((B, Cn, h, w)), dy=dev.zeros((B, Fn, h, w)))
    out = Out(dev, (Fn, Cn, k, k))
    W = dev.lib().bla_conv2d_weight_gradient_batched_f32_as_bf16
    assert W(None, None, g["x"].ptr, out.ptr, B, h, w, k, Cn, Fn, s, 0) == 1
    assert W(None, g["dy"].ptr, None, out.ptr, B, h, w, k, Cn, Fn, s, 0) == 1
    assert W(None, g["dy"].ptr, g["x"].ptr, None, B, h, w, k, Cn, Fn, s, 0) == 1
    assert W(None, g["dy"].ptr, g["x"].ptr, out.ptr, B, h, w, k, Cn, Fn, s, -1) == 1
    assert W(None, g["dy"].ptr, g["x"].ptr, out.ptr, 0, h, w, k, Cn, Fn, s, 0) == 1
    assert W(None, g["dy"].ptr, g["x"].ptr, out.ptr, B, h, w, k, Cn, Fn, 0, 2) == 1
    dev.sync()
    assert out.untouched()
    wgrad(dev, g, case, out, 2)                                  # and the same arguments, valid, run
    assert (out.read() == 0).all()
