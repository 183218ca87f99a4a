"""The implicit bf16 weight gradient on the device (include/bla.h): bla_conv2d_weight_gradient_gathered_bf16 on padded copies and
bla_conv2d_backward_gathered_f32_as_bf16, the backward pass that pads del_y once for both gradients.

For every case and splits in {0, 1, 2, 3}:
* integer operands (-4..4, exact in bf16; every partial sum far below 2^24): del_kern of both entries equals an int64 numpy weight gradient bit for bit,
  and bla_conv2d_weight_gradient_batched_f32_as_bf16's; the kernel name carries S_eff by the partition rule restated here (splits = 0: the plan entry for
  the device's CU count, on m = F, n = k k Cp, k = N);
* operands uniform [-1, 1) rounded to bf16: per element, against float64 on the same values, with N = B Ho Wo and nothing left out,
      |got - ref| <= (N + 8) 2^-23 (|del_y| * |x|) + 2 2^-24 |ref|                                  (DESIGN 3.20's bound with k = N); worst ratio printed
  (measured on an MI355X: 0.027 at k = 4, stride 2; 0.0008 .. 0.0023 at the cases with several slabs);
* the first entry runs on HOST-made copies full of junk in every place it must not read into a written element: Q holds the bf16 NaN 0x7FC0 at every
  position that is not (top + i d, left + j d) and in the channels F .. Fp, P holds it in the channels C .. Cp (its halo is +0): del_kern is NaN-free
  and meets the assertions above;
* the second entry equals its stated composition of public entries (pad x, pad del_y once, the first entry, prepare_kernels + the gathered product at
  stride 1) bit for bit in del_kern and del_x, also with either output NULL, and its del_x is the existing backward entry's bit for bit;
* outputs start as 0xFF bytes between guards, which keep their bits; a second run after other products have used the workspace is bit-identical.
The partition and the fold order: at (6,64,128,8,8,3,1), splits = 3, a split is exactly two images, and the result equals bit for bit the float32 sum,
in ascending order, of three splits = 1 calls on the images [0:2], [2:4], [4:6].
Refusals (NULL pointer, splits < 0, cp or fp not a multiple of 8, a misaligned base, top + (ho-1) dilate >= hq, taps past hp) leave the output untouched.
The SAME geometry, the im2col and the partition are restated here; nothing is imported from another test file.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F32, F64, U16, U32, I64 = np.float32, np.float64, np.uint16, np.uint32, np.int64
GUARD = 64
NAN16 = 0x7FC0
SPLITS = [0, 1, 2, 3]
#        B   C    F   H  W  k  s
CASES = [(2, 16, 130, 9, 9, 3, 1),     # N = 162: 3 slabs with a short last one; two row tiles; tiles straddling taps (Cp = 16)
         (6, 64, 128, 8, 8, 3, 1),     # N = 384: 6 slabs, 5 column tiles
         (2, 8, 8, 8, 8, 3, 2),        # stride 2: Q dilated; one short slab
         (2, 8, 8, 7, 7, 3, 2),        # stride 2 on an odd map
         (1, 8, 8, 6, 6, 5, 1),        # k = 5
         (1, 8, 16, 6, 6, 4, 2),       # k = 4 at stride 2
         (2, 8, 8, 4, 4, 1, 1),        # k = 1
         (3, 3, 20, 7, 5, 3, 1),       # C and F not multiples of 8; a non-square map
         (2, 24, 8, 8, 8, 3, 2)]       # Cp = 24
IDS = ["B%d_C%d_F%d_%dx%d_k%d_s%d" % c for c in CASES]
NAME = "conv_bf16_wgrad128x128x64_s%d_splitk%d"


@pytest.fixture(scope="module")
def dev(pkg):
    pkg.init(0)
    return pkg


# ---- geometry, im2col and partition, restated ------------------------------------------------------------------------------------------------------------
def same_geometry(h, w, k, s):
    ho, wo = int(np.ceil(F32(h) / F32(s))), int(np.ceil(F32(w) / F32(s)))
    vpad, hpad = max((ho - 1) * s + k - h, 0), max((wo - 1) * s + k - w, 0)
    return ho, wo, vpad // 2, hpad // 2, vpad, hpad


def layout(h, w, k, s, data_gradient):
    """(hp, wp, top, left, dilate) of include/bla.h"""
    ho, wo, pt, pl, vpad, hpad = same_geometry(h, w, k, s)
    return (h + k - 1, w + k - 1, k - 1 - pt, k - 1 - pl, s) if data_gradient else (h + vpad, w + hpad, pt, pl, 1)


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
    ho, wo, pt, pl = same_geometry(h, w, k, s)[:4]
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


def junk_copies(dev, x, dy, k, s):
    """host-made P (halo +0, NaN in the channels C .. Cp) and Q (NaN everywhere but at the del_y positions' channels below F), as bf16 bit patterns"""
    B, Cn, h, w = x.shape
    Fn, ho, wo = dy.shape[1:]
    hp, wp, top, left, _ = layout(h, w, k, s, False)
    P = np.zeros((B, hp, wp, round8(Cn)), U16)
    P[:, :, :, Cn:] = NAN16
    P[:, top:top + h, left:left + w, :Cn] = dev.to_bf16(x).transpose(0, 2, 3, 1)
    hq, wq, top, left, d = layout(h, w, k, s, True)
    Q = np.full((B, hq, wq, round8(Fn)), NAN16, U16)
    Q[:, top:top + (ho - 1) * d + 1:d, left:left + (wo - 1) * d + 1:d, :Fn] = dev.to_bf16(dy).transpose(0, 2, 3, 1)
    return P, Q


class Out:
    """`shape` fp32 elements that start as 0xFF bytes (a NaN) with GUARD elements of the same pattern on either side."""

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


def call(dev, name, *args, want=0):
    st = getattr(dev.lib(), name)(None, *args)
    assert st == want, (name, st, dev.lib().bla_last_error())
    dev.sync()


def device_cus(dev):
    """the context's CU count, as bla_device_name reports it: "<arch> (<n> CUs)" """
    import ctypes
    import re
    buf = ctypes.create_string_buffer(128)
    assert dev.lib().bla_device_name(buf, 128) == 0
    return int(re.search(rb"\((\d+) CUs\)", buf.value).group(1))


_cache = {}


def case_data(dev, case, kind):
    key = (case, kind)
    if key in _cache:
        return _cache[key]
    B, Cn, Fn, h, w, k, s = case
    ho, wo = same_geometry(h, w, k, s)[:2]
    rng = np.random.default_rng(1600 + CASES.index(case))
    shapes = dict(x=(B, Cn, h, w), dy=(B, Fn, ho, wo), kern=(Fn, Cn, k, k))
    if kind == "exact":
        v = {n: rng.integers(-4, 5, sh).astype(F32) for n, sh in shapes.items()}
        d = dict(v, dkern=weight_gradient(v["x"].astype(I64), v["dy"].astype(I64), k, s).astype(F32))
    else:
        v = {n: dev.from_bf16(dev.to_bf16(rng.uniform(-1, 1, sh).astype(F32))) for n, sh in shapes.items()}
        dkern = weight_gradient(v["x"].astype(F64), v["dy"].astype(F64), k, s)
        adkern = weight_gradient(np.abs(v["x"]).astype(F64), np.abs(v["dy"]).astype(F64), k, s)
        d = dict(v, dkern=dkern, bound=(B * ho * wo + 8) * 2.0 ** -23 * adkern + 2 * 2.0 ** -24 * np.abs(dkern))
    d["dev"] = {n: dev.to_device(d[n]) for n in shapes}
    P, Q = junk_copies(dev, d["x"], d["dy"], k, s)
    d["dev"]["P"], d["dev"]["Q"] = dev.to_device(P, U16), dev.to_device(Q, U16)
    _cache[key] = d
    return d


def entry1_args(case, q_ptr, p_ptr, out_ptr, splits, batch=None):
    B, Cn, Fn, h, w, k, s = case
    ho, wo = same_geometry(h, w, k, s)[:2]
    hp, wp, _, _, _ = layout(h, w, k, s, False)
    hq, wq, top, left, d = layout(h, w, k, s, True)
    return (q_ptr, hq, wq, round8(Fn), top, left, d, p_ptr, hp, wp, round8(Cn), batch or B, k, s, ho, wo, Fn, Cn, out_ptr, splits)


def entry1(dev, case, g, out, splits, want=0):
    call(dev, "bla_conv2d_weight_gradient_gathered_bf16", *entry1_args(case, g["Q"].ptr, g["P"].ptr, out.ptr, splits), want=want)
    return last_name(dev)


def entry2(dev, case, g, dk, dx, splits, want=0):
    B, Cn, Fn, h, w, k, s = case
    call(dev, "bla_conv2d_backward_gathered_f32_as_bf16", g["dy"].ptr, g["x"].ptr, g["kern"].ptr, dk.ptr if dk else None, dx.ptr if dx else None, B, h, w, k, Cn, Fn, s,
         splits, want=want)
    return last_name(dev)


def expected_name(dev, case, splits):
    B, Cn, Fn, h, w, k, s = case
    ho, wo = same_geometry(h, w, k, s)[:2]
    n = B * ho * wo
    eff = dev.gemm_bf16_splitk_plan(Fn, k * k * round8(Cn), n, 0, device_cus(dev))[0] if splits == 0 else partition(n, splits)[0]
    return NAME % (s, eff)


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_integer_operands_are_exact(dev, case, splits):
    B, Cn, Fn, h, w, k, s = case
    d = case_data(dev, case, "exact")
    g = d["dev"]
    one, two, theirs = Out(dev, d["dkern"].shape), Out(dev, d["dkern"].shape), Out(dev, d["dkern"].shape)
    want = expected_name(dev, case, splits)
    assert entry1(dev, case, g, one, splits) == want
    assert entry2(dev, case, g, two, None, splits) == want
    call(dev, "bla_conv2d_weight_gradient_batched_f32_as_bf16", g["dy"].ptr, g["x"].ptr, theirs.ptr, B, h, w, k, Cn, Fn, s, splits)
    for got in (one.read(), two.read(), theirs.read()):
        assert np.array_equal(got.view(U32), d["dkern"].view(U32)), f"{want}: {int((got != d['dkern']).sum())} elements differ"


@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rounded_operands_against_float64_and_the_composition(dev, case, splits):
    B, Cn, Fn, h, w, k, s = case
    ho, wo = same_geometry(h, w, k, s)[:2]
    d = case_data(dev, case, "rounded")
    g = d["dev"]
    want = expected_name(dev, case, splits)
    one, two, dx = Out(dev, d["dkern"].shape), Out(dev, d["dkern"].shape), Out(dev, (B, Cn, h, w))
    assert entry1(dev, case, g, one, splits) == want                        # on the junk-filled host copies
    entry2(dev, case, g, two, dx, splits)
    assert last_name(dev) == "conv_bf16_gather128x128x64_s1"
    got1, got2, got_dx = one.read(), two.read(), dx.read()
    for who, got in (("gathered", got1), ("backward", got2)):
        assert not np.isnan(got).any(), who
        err = np.abs(got.astype(F64) - d["dkern"])
        ratio = float((err / np.maximum(d["bound"], 1e-300)).max())
        print("conv_bf16 implicit weight gradient %s %s splits %d %s: worst |err| / bound = %.4f" % (who, "B%d_C%d_F%d_%dx%d_k%d_s%d" % case, splits, want, ratio))
        assert (err <= d["bound"]).all(), (who, want, ratio)
    assert np.array_equal(got1.view(U32), got2.view(U32))                   # junk or zeros in the unread places: the same bits
    # the composition, by the public entries and the Python helpers
    cp, fp = round8(Cn), round8(Fn)
    hp, wp, top, left, dil = dev.conv_bf16_layout(h, w, k, s)
    assert (hp, wp, top, left, dil) == layout(h, w, k, s, False)
    P = dev.conv_bf16_pad(g["x"], dev.empty((B, hp, wp, cp), U16), B, Cn, h, w, hp, wp, top, left, dil)
    hq, wq, qtop, qleft, qdil = dev.conv_bf16_layout(h, w, k, s, True)
    assert (hq, wq, qtop, qleft, qdil) == layout(h, w, k, s, True)
    Q = dev.conv_bf16_pad(g["dy"], dev.empty((B, hq, wq, fp), U16), B, Fn, ho, wo, hq, wq, qtop, qleft, qdil)
    mine = Out(dev, d["dkern"].shape)
    dev.conv2d_weight_gradient_gathered_bf16(Q, hq, wq, fp, qtop, qleft, qdil, P, hp, wp, cp, B, k, s, ho, wo, Fn, Cn, mine.ptr, splits=splits)
    dev.sync()
    assert last_name(dev) == want
    assert np.array_equal(mine.read().view(U32), got2.view(U32))
    if splits == 0:                                                         # the data gradient does not depend on splits
        A = dev.conv_bf16_prepare_kernels(g["kern"], dev.empty((Cn, k * k * fp), U16), Fn, Cn, k, True)
        mine_dx, theirs_dx = Out(dev, (B, Cn, h, w)), Out(dev, (B, Cn, h, w))
        dev.conv2d_gathered_bf16(A, Cn, Q, B, hq, wq, fp, k, 1, h, w, mine_dx.ptr)
        dev.sync()
        assert np.array_equal(mine_dx.read().view(U32), got_dx.view(U32))
        call(dev, "bla_conv2d_backward_batched_f32_as_bf16", g["dy"].ptr, None, g["kern"].ptr, None, theirs_dx.ptr, B, h, w, k, Cn, Fn, s)
        assert np.array_equal(theirs_dx.read().view(U32), got_dx.view(U32))
    # either output NULL; these runs come after other products have used the workspace
    only_dk, only_dx = Out(dev, d["dkern"].shape), Out(dev, (B, Cn, h, w))
    assert entry2(dev, case, g, only_dk, None, splits) == want
    assert entry2(dev, case, g, None, only_dx, splits) == "conv_bf16_gather128x128x64_s1"
    assert np.array_equal(only_dk.read().view(U32), got2.view(U32)) and np.array_equal(only_dx.read().view(U32), got_dx.view(U32))
    entry2(dev, case, g, None, None, splits)                                # nothing to do
    again = Out(dev, d["dkern"].shape)
    assert entry1(dev, case, g, again, splits) == want
    assert np.array_equal(again.read().view(U32), got1.view(U32))


def test_partition_and_fold_order(dev):
    case = CASES[1]
    B, Cn, Fn, h, w, k, s = case
    assert same_geometry(h, w, k, s)[:2] == (8, 8) and partition(B * 64, 3) == (3, 2)      # a split = 2 slabs = 128 pixels = two images
    d = case_data(dev, case, "rounded")
    g = d["dev"]
    whole = Out(dev, d["dkern"].shape)
    assert entry1(dev, case, g, whole, 3) == NAME % (s, 3)
    hp, wp = layout(h, w, k, s, False)[:2]
    hq, wq = layout(h, w, k, s, True)[:2]
    parts = []
    for first in (0, 2, 4):
        part = Out(dev, d["dkern"].shape)
        call(dev, "bla_conv2d_weight_gradient_gathered_bf16",
             *entry1_args(case, g["Q"].ptr + first * hq * wq * round8(Fn) * 2, g["P"].ptr + first * hp * wp * round8(Cn) * 2, part.ptr, 1, batch=2))
        assert last_name(dev) == NAME % (s, 1)
        parts.append(part.read())
    acc = parts[0].copy()
    acc += parts[1]
    acc += parts[2]
    assert acc.dtype == F32 and np.array_equal(acc.view(U32), whole.read().view(U32))


def test_python_helpers(dev):
    case = CASES[0]
    B, Cn, Fn, h, w, k, s = case
    d = case_data(dev, case, "exact")
    g = d["dev"]
    dk, dx = dev.empty((Fn, Cn, k, k)), dev.empty((B, Cn, h, w))
    dev.conv2d_backward_gathered_as_bf16(g["dy"], g["x"], g["kern"], dk, dx, B, h, w, k, Cn, Fn, s, splits=3)
    dev.sync()
    assert np.array_equal(dk.numpy(), d["dkern"])
    dev.conv2d_backward_gathered_as_bf16(g["dy"], g["x"], None, dk, None, B, h, w, k, Cn, Fn, s, splits=3)
    dev.sync()
    assert last_name(dev) == NAME % (s, 3)


def test_argument_refusals_leave_the_output_alone(dev):
    case = (2, 8, 8, 6, 6, 3, 1)
    B, Cn, Fn, h, w, k, s = case
    hp, wp = layout(h, w, k, s, False)[:2]
    hq, wq, top, left, dil = layout(h, w, k, s, True)
    Q, P = dev.zeros((B, hq, wq, 16), U16), dev.zeros((B, hp, wp, 16), U16)     # room for the bad extents tried below
    out = Out(dev, (Fn, Cn, k, k))
    good = list(entry1_args(case, Q.ptr, P.ptr, out.ptr, 0))
    names = ["q", "hq", "wq", "fp", "top", "left", "dilate", "p", "hp", "wp", "cp", "batch", "k", "stride", "ho", "wo", "f_n", "c_n", "out", "splits"]

    def refused(**changed):
        args = [changed.get(n, v) for n, v in zip(names, good)]
        call(dev, "bla_conv2d_weight_gradient_gathered_bf16", *args, want=1)

    refused(q=None), refused(p=None), refused(out=None)
    refused(splits=-1)
    refused(cp=12), refused(fp=12)
    refused(q=Q.ptr + 2), refused(p=P.ptr + 8)
    refused(top=hq - (h - 1) * dil), refused(left=wq - (w - 1) * dil)                 # top + (ho-1) dilate >= hq
    refused(hp=h + k - 2), refused(wp=w + k - 2)                                      # taps past the padded map
    refused(batch=0), refused(stride=0), refused(dilate=0), refused(fp=0), refused(cp=0)
    g = dict(x=dev.zeros((B, Cn, h, w)), dy=dev.zeros((B, Fn, h, w)), kern=dev.zeros((Fn, Cn, k, k)))
    entry2(dev, case, g, out, None, -1, want=1)
    call(dev, "bla_conv2d_backward_gathered_f32_as_bf16", None, g["x"].ptr, g["kern"].ptr, out.ptr, None, B, h, w, k, Cn, Fn, s, 0, want=1)
    call(dev, "bla_conv2d_backward_gathered_f32_as_bf16", g["dy"].ptr, None, g["kern"].ptr, out.ptr, None, B, h, w, k, Cn, Fn, s, 0, want=1)
    call(dev, "bla_conv2d_backward_gathered_f32_as_bf16", g["dy"].ptr, g["x"].ptr, None, None, out.ptr, B, h, w, k, Cn, Fn, s, 0, want=1)
    assert out.untouched()
    call(dev, "bla_conv2d_weight_gradient_gathered_bf16", *good)                     # and the same arguments, valid, run
    assert (out.read() == 0).all()
