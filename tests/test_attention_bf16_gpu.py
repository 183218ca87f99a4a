"""bla_attention_{forward,backward}_batched_bf16 and the model's attention switch on the device, against tests/test_attention_bf16_host.py:
cases, inputs, the float64 blocks and the recorded rounded-against-exact values are that file's.

* Every output and saved tensor is a view between guard elements in an allocation filled with 0xFF bytes; the guards must come back untouched.  GUARD is
  odd, so every such tensor starts 4 bytes off a 16-byte boundary: the entries ask for float alignment only.  scores_raw is NULL throughout.
* Per tensor ||device - exact|| / ||exact|| <= 2 x the host-recorded value (the device shares the roundings; fp32 accumulation, expf and the elements that
  round the other way do not show beside a unit roundoff of 2^-9: DESIGN 3.25 / 3.26's margin).  Device and host values are printed side by side
  (profiles/r21_attention_bf16_tests.txt).
* weights' rows sum to 1 within 4 S 2^-24; saved q, k, v lie within the accumulation bound of r(Z) r(W) in float64: C 2^-23 sum |r(z)| |r(w)| per element
  (twice the bound of C additions rounded to nearest: the matrix pipe's own summation inside an instruction is not specified to round each addition).
* The exact forward case: d_out and ws->attention equal the host restatement bit for bit.
* Two runs give the same bits in every tensor; image b of a batch equals a batch-1 run of image b.
* Refusals leave pattern-filled outputs untouched.
* Model: the attention matrices zero => both modes give the same prediction and gradients (each block then returns its bias, and every attention
  gradient is an exact zero, in either arithmetic); with the real parameters BF16 mode changes the pass, F32 mode afterwards reproduces the first bits."""
import ctypes as C

import numpy as np
import pytest

import test_attention_bf16_host as host
import test_unet_bf16_host as unet_host

pytestmark = pytest.mark.gpu
F32, U32 = np.float32, np.uint32
GUARD = 61
SAVED = ["q", "k", "v", "weights", "attention"]
GRADS = ["del_q", "del_k", "del_v", "del_wq", "del_wk", "del_wv", "del_w", "del_x"]


@pytest.fixture(scope="module")
def dev(pkg):
    pkg.init(0)
    return pkg


class Out:
    """`shape` floats filled with 0xFF bytes, with GUARD elements of the same pattern on either side"""

    def __init__(self, dev, shape):
        self.shape, self.n = tuple(shape), int(np.prod(shape))
        self.arr = dev.DeviceArray((self.n + 2 * GUARD,), U32).fill_bytes(0xFF)
        self.ptr = self.arr.ptr + 4 * GUARD

    def bits(self):
        now = self.arr.numpy()
        assert (now[:GUARD] == 0xFFFFFFFF).all() and (now[GUARD + self.n:] == 0xFFFFFFFF).all(), "a guard element changed"
        return now[GUARD:GUARD + self.n].reshape(self.shape).copy()

    def untouched(self):
        return (self.arr.numpy() == 0xFFFFFFFF).all()


def shapes(case):
    b, c, s, d = case
    return dict(q=(b, s, d), k=(b, s, d), v=(b, s, d), weights=(b, s, s), attention=(b, s, d), out=(b, c, s), del_q=(b, s, d), del_k=(b, s, d), del_v=(b, s, d),
                del_wq=(c, d), del_wk=(c, d), del_wv=(c, d), del_w=(d, c), del_x=(b, c, s), partials=(b, 4 * c * d))


def run(dev, case, I, backward=True):
    """both entries on fresh guarded buffers -> {tensor: its bit patterns}"""
    b, c, s, d = case
    D = {n: dev.to_device(np.ascontiguousarray(a, F32)) for n, a in I.items()}
    O = {n: Out(dev, shp) for n, shp in shapes(case).items()}
    fws = dev.attention_ws(**{n: O[n].ptr for n in SAVED})
    dev.attention_forward_batched_bf16(b, D["x"], D["wq"], D["wk"], D["wv"], D["w"], D["bias"], fws, O["out"].ptr, c, s, d)
    if backward:
        gws = dev.attention_ws(q=O["del_q"].ptr, k=O["del_k"].ptr, v=O["del_v"].ptr)
        dev.attention_backward_batched_bf16(b, D["del_y"], D["x"], D["wq"], D["wk"], D["wv"], D["w"], fws, gws, O["partials"].ptr, O["del_wq"].ptr, O["del_wk"].ptr,
                                            O["del_wv"].ptr, O["del_w"].ptr, O["del_x"].ptr, c, s, d)
    dev.sync()
    return {n: O[n].bits() for n in SAVED + ["out"] + (GRADS if backward else [])}


@pytest.fixture(scope="module")
def passes(dev):
    """one device pass per case, shared by the tests that only read it"""
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = run(dev, case, host.recorded(case)[0])
        return cache[case]
    return get


@pytest.mark.parametrize("case", host.CASES, ids=str)
def test_against_the_unrounded_float64_block(passes, case):
    """Measured on an MI355X (profiles/r21_attention_bf16_tests.txt; the nine cases, nine of the backward core's sixteen instantiations:
    profiles/r23_unet_paths_tests.txt): device / recorded 1.00 in all 54 tensors, and the device within 2e-4 normwise of the rounded restatement itself."""
    I, exact, rounded, diff = host.recorded(case)
    got = passes(case)
    for n in host.OUTPUTS:
        v = host.normwise(got[n].view(F32), exact[n])
        print(f"{str(case):22s} {n:8s} device vs exact {v:.3e}   host rounded vs exact {diff[n]:.3e}   ratio {v / diff[n]:.2f}   device vs rounded {host.normwise(got[n].view(F32), rounded[n]):.1e}")
    for n in host.OUTPUTS:
        assert host.normwise(got[n].view(F32), exact[n]) <= 2 * diff[n], (n, host.normwise(got[n].view(F32), exact[n]), diff[n])
    for n in ("del_q", "del_k", "del_v"):       # what grad->q, k, v receive
        assert host.normwise(got[n].view(F32), exact[n]) <= 2 * host.normwise(rounded[n], exact[n]), n


@pytest.mark.parametrize("case", host.CASES, ids=str)
def test_saved_tensors(passes, case):
    b, c, s, d = case
    I, _, rounded, _ = host.recorded(case)
    got = passes(case)
    p = got["weights"].view(F32).astype(np.float64)
    assert np.isfinite(p).all() and (p >= 0).all()
    assert np.abs(p.sum(axis=2) - 1).max() <= 4 * 2.0 ** -24 * s, np.abs(p.sum(axis=2) - 1).max()
    z = host.rnd(np.swapaxes(I["x"].astype(np.float64), 1, 2))
    for n, w in (("q", "wq"), ("k", "wk"), ("v", "wv")):
        rw = host.rnd(I[w].astype(np.float64))
        err = np.abs(got[n].view(F32) - z @ rw)
        bound = c * 2.0 ** -23 * (np.abs(z) @ np.abs(rw))
        assert (err <= bound).all(), (n, float((err / np.maximum(bound, 1e-300)).max()))
    assert host.normwise(got["weights"].view(F32), rounded["weights"]) < 1e-2 and host.normwise(got["attention"].view(F32), rounded["attention"]) < 1e-2


@pytest.mark.parametrize("s", [32, 256])
def test_exact_forward_case_bit_for_bit(dev, s):
    I = host.exact_inputs(s)
    want = host.block(I, True, np.float32, backward=False)
    got = run(dev, (2, 16, s, 16), I, backward=False)
    for n in ("out", "attention", "weights", "v", "k"):
        assert np.array_equal(got[n], np.ascontiguousarray(want[n], F32).view(U32)), n
    assert not got["q"].view(F32).any()


def test_second_run_and_batch_one(dev, passes):
    case = host.CASES[1]
    b, c, s, d = case
    I = host.recorded(case)[0]
    first, again = passes(case), run(dev, case, I)
    for n in first:
        assert np.array_equal(first[n], again[n]), n
    for img in range(b):
        one = run(dev, (1, c, s, d), dict(I, x=I["x"][img:img + 1], del_y=I["del_y"][img:img + 1]), backward=False)
        for n in SAVED + ["out"]:
            assert np.array_equal(one[n][0], first[n][img]), (img, n)


def test_refusals_leave_the_outputs_untouched(dev):
    L = dev.lib()
    case = (2, 64, 64, 16)
    b, c, s, d = case
    I = host.make_inputs(case)
    D = {n: dev.to_device(np.ascontiguousarray(a, F32)) for n, a in I.items()}
    big = (2, 64, 288, 72)        # buffers large enough for every refused shape
    O = {n: Out(dev, shp) for n, shp in shapes(big).items()}
    fws = dev.attention_ws(**{n: O[n].ptr for n in SAVED})
    gws = dev.attention_ws(q=O["del_q"].ptr, k=O["del_k"].ptr, v=O["del_v"].ptr)

    def fwd(c_, s_, d_, x=D["x"].ptr, ws=fws):
        return L.bla_attention_forward_batched_bf16(None, b, x, D["wq"].ptr, D["wk"].ptr, D["wv"].ptr, D["w"].ptr, D["bias"].ptr, C.byref(ws) if ws else None, O["out"].ptr,
                                                    c_, s_, d_)

    def bwd(c_, s_, d_, dy=D["del_y"].ptr, partials=O["partials"].ptr, grad=gws):
        return L.bla_attention_backward_batched_bf16(None, b, dy, D["x"].ptr, D["wq"].ptr, D["wk"].ptr, D["wv"].ptr, D["w"].ptr, C.byref(fws), C.byref(grad), partials,
                                                     O["del_wq"].ptr, O["del_wk"].ptr, O["del_wv"].ptr, O["del_w"].ptr, O["del_x"].ptr, c_, s_, d_)
    for shape in [(c, 16, d), (c, 288, d), (c, s, 4), (c, s, 72), (12, s, d)]:
        assert fwd(*shape) == 1 and bwd(*shape) == 1, shape
    assert fwd(c, s, d, x=None) == 1 and bwd(c, s, d, dy=None) == 1 and bwd(c, s, d, partials=None) == 1
    assert fwd(c, s, d, ws=dev.attention_ws(q=O["q"].ptr, k=O["k"].ptr, v=O["v"].ptr, attention=O["attention"].ptr)) == 1      # weights NULL
    assert bwd(c, s, d, grad=dev.attention_ws(q=O["del_q"].ptr, k=O["del_k"].ptr)) == 1                                       # grad->v NULL
    assert L.bla_attention_forward_batched_bf16(None, 0, *([D["x"].ptr] * 6), C.byref(fws), O["out"].ptr, c, s, d) == 1      # batch 0
    dev.sync()
    assert all(o.untouched() for o in O.values())


# ---- the model ----------------------------------------------------------------------------------------------------------------------------------------
def test_model_attention_switch(dev):
    """tests/test_unet_bf16_host.py's configuration: the four attention blocks of the 8 x 8 level (C = 64, S = 64, key_dim 8) qualify, the 2 x 2 mid block does
    not and stays on the fp32 entries in both modes."""
    import test_unet_bf16_gpu as ug
    pkg, L = dev, dev.lib()
    cfg, B = unet_host.CFG, unet_host.B
    assert pkg.attention_bf16_applies(cfg["dims"][1], 64, cfg["key_dim"]) and not pkg.attention_bf16_applies(cfg["dims"][3], 4, cfg["key_dim"])
    x, temb, noise, drop = unet_host.make_inputs()
    dd = unet_host.device_drop_layout(drop)
    data = dict(x=pkg.to_device(x), temb=pkg.to_device(temb), noise=pkg.to_device(noise), drop=pkg.DeviceArray((dd.size,), np.uint8).copy_from(dd))
    P = unet_host.make_params()
    Z = {n: (np.zeros_like(v) if "attention" in n and not n.endswith("biases") else v) for n, v in P.items()}      # (the biases stay: a block that returned
    # zeros would hand the next group norm a zero variance to divide by)
    for products in (ug.F32, ug.BF16):
        # attention matrices zero: the same values in both attention modes (compared as numbers: a zero's sign is not part of the claim)
        m = ug.Model(pkg, cfg, B, products, Z)
        assert L.bla_unet_attention(m.h) == pkg.UNET_ATTENTION_F32 == pkg.unet_attention(m.h)
        o0, g0 = ug.one_pass(m, data)
        pkg.unet_set_attention(m.h, pkg.UNET_ATTENTION_BF16)
        assert L.bla_unet_attention(m.h) == pkg.UNET_ATTENTION_BF16
        for bad in (2, -1, 7):
            assert L.bla_unet_set_attention(m.h, bad) == 1 and L.bla_unet_attention(m.h) == pkg.UNET_ATTENTION_BF16
        o1, g1 = ug.one_pass(m, data)
        assert np.isfinite(g0).all() and np.abs(g0).max() > 0
        assert np.array_equal(o0, o1) and np.array_equal(g0, g1)
        m.destroy()
        # the real parameters: BF16 mode is another arithmetic in the blocks that qualify, F32 mode afterwards is the first pass again
        m = ug.Model(pkg, cfg, B, products, P)
        o0, g0 = ug.one_pass(m, data)
        pkg.unet_set_attention(m.h, pkg.UNET_ATTENTION_BF16)
        o1, g1 = ug.one_pass(m, data)
        o1b, g1b = ug.one_pass(m, data)
        pkg.unet_set_attention(m.h, pkg.UNET_ATTENTION_F32)
        assert L.bla_unet_attention(m.h) == pkg.UNET_ATTENTION_F32
        o2, g2 = ug.one_pass(m, data)
        assert np.array_equal(o0.view(U32), o2.view(U32)) and np.array_equal(g0.view(U32), g2.view(U32))
        assert np.array_equal(o1.view(U32), o1b.view(U32)) and np.array_equal(g1.view(U32), g1b.view(U32))
        assert np.isfinite(o1).all() and np.isfinite(g1).all()
        assert not np.array_equal(o0, o1) and not np.array_equal(g0, g1)
        att = [(off, cnt) for name, off, cnt in m.tensors if "attention" in name and not name.startswith("mid") and not name.endswith("biases")]
        assert len(att) == 16
        for off, cnt in att:        # every routed block's gradients moved, by a rounding's worth and no more
            a, b_ = g1[off:off + cnt].astype(np.float64), g0[off:off + cnt].astype(np.float64)
            assert 0 < np.linalg.norm(a - b_) <= 0.25 * np.linalg.norm(b_)
        m.destroy()
