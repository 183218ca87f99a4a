"""bla_attention_{forward,backward}_batched_f32_heads on the device, against tests/test_attention_f32_heads_host.py: cases, inputs, the float64
composed multi-head block and the tolerance are that file's.

* Every output and saved tensor is a view between guard elements in an allocation filled with 0xFF bytes (tests/test_unet_glue_paths_gpu.py's Guarded); the
  guards must come back untouched.  With heads > 1 scores_raw (both workspaces) and the gradient workspace's weights are NULL throughout.
* Every saved tensor (q, k, v, weights = P, attention), out, the five gradients and the gradient workspace (del_P, del_Q, del_K, del_V) against the float64
  reference: |got - ref| <= t |ref| + t mean|ref|, t = 2e-5 forward and 5e-5 for gradients (tests/test_attention_paths_gpu.py's form and rule).  What that
  leaves the device is measured on the host, never on the device: the float32 NumPy restatement stays at or below 0.081 of the limit on these cases
  (`python tests/test_attention_f32_heads_host.py`), below the 0.25 at which a tensor's t would widen, so WIDER is empty.  The device's own ratios are printed
  before anything is asserted.
* Two runs give the same bits in every tensor; image b of a batch equals a batch-1 run of image b.
* heads == 1 is bla_attention_{forward,backward}_batched_f32 (jacobian_from_raw = 0) bit for bit in every tensor, scores_raw and del_I included.
* Refusals (s = 65, d = 65, heads d = 264, heads = 0, NULLs, batch 0 and 65536) leave pattern-filled outputs untouched."""
import ctypes as C

import numpy as np
import pytest

import test_attention_f32_heads_host as host
from test_unet_glue_paths_gpu import Guarded

pytestmark = pytest.mark.gpu
F32 = np.float32
WIDER = host.WIDER          # {} -- measured on the host, see above
PER_IMAGE = host.FWD + ["del_x"] + host.WORK


@pytest.fixture(scope="module")
def dev(pkg):
    pkg.init(0)
    return pkg


def shapes(case):
    b, c, s, heads, d = case
    D = heads * d
    act = (b, s, D)
    return dict(q=act, k=act, v=act, attention=act, weights=(b, heads, s, s), out=(b, c, s), del_p=act, del_q=act, del_k=act, del_v=act, del_wq=(c, D), del_wk=(c, D),
                del_wv=(c, D), del_w=(D, c), del_x=(b, c, s), partials=(b, c * D), scores_raw=(b, s, s), del_i=(b, s, s), del_s=(b, s, s))


def buffers(dev, case, single):
    names = host.ALL + ["partials"] + (["scores_raw", "del_i", "del_s"] if single else [])
    shp = shapes(case)
    O = {n: Guarded(dev, shp[n]) for n in names}
    ptr = lambda n: O[n].ptr if n in O else None
    fws = dev.attention_ws(q=O["q"].ptr, k=O["k"].ptr, v=O["v"].ptr, weights=O["weights"].ptr, attention=O["attention"].ptr, scores_raw=ptr("scores_raw"))
    gws = dev.attention_ws(q=O["del_q"].ptr, k=O["del_k"].ptr, v=O["del_v"].ptr, attention=O["del_p"].ptr, scores_raw=ptr("del_i"), weights=ptr("del_s"))
    return O, fws, gws


def run(dev, case, I, single=False):
    """both entries on fresh guarded buffers -> {tensor: its bit patterns}; single: bla_attention_*_batched_f32 itself (heads == 1 only)"""
    L, chk = dev.lib(), dev.native.check
    b, c, s, heads, d = case
    assert heads == 1 or not single
    D = {n: dev.to_device(np.ascontiguousarray(a, F32)) for n, a in I.items()}
    O, fws, gws = buffers(dev, case, heads == 1)
    P = [D[n].ptr for n in ("wq", "wk", "wv", "w")]
    G = [O[n].ptr for n in host.GRADS]
    if single:
        chk(L.bla_attention_forward_batched_f32(None, b, D["x"].ptr, *P, D["bias"].ptr, C.byref(fws), O["out"].ptr, c, s, d))
        chk(L.bla_attention_backward_batched_f32(None, b, D["del_y"].ptr, D["x"].ptr, *P, C.byref(fws), C.byref(gws), O["partials"].ptr, *G, c, s, d, 0))
    else:
        chk(L.bla_attention_forward_batched_f32_heads(None, b, D["x"].ptr, *P, D["bias"].ptr, C.byref(fws), O["out"].ptr, c, s, heads, d))
        chk(L.bla_attention_backward_batched_f32_heads(None, b, D["del_y"].ptr, D["x"].ptr, *P, C.byref(fws), C.byref(gws), O["partials"].ptr, *G, c, s, heads, d))
    dev.sync()
    return {n: o.bits() for n, o in O.items()}


@pytest.fixture(scope="module")
def passes(dev):
    """one device pass per case, shared by the tests that only read it"""
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = run(dev, case, host.reference(case)[0])
        return cache[case]
    return get


@pytest.mark.parametrize("case", host.CASES, ids=str)
def test_against_the_composed_float64_block(passes, case):
    _, ref = host.reference(case)
    got = {n: a.view(F32) for n, a in passes(case).items()}
    rs = host.ratios(case, got, ref)
    print(f"{str(case):22s} device  " + "  ".join(f"{n} {v:.3f}" for n, v in rs.items()))
    assert all(np.isfinite(got[n]).all() for n in host.ALL)
    worst = {n: v for n, v in rs.items() if not v <= 1}
    assert not worst, worst


@pytest.mark.parametrize("case", host.CASES, ids=str)
def test_second_run_and_batch_one(dev, passes, case):
    b, c, s, heads, d = case
    I = host.reference(case)[0]
    first, again = passes(case), run(dev, case, I)
    for n in first:
        assert np.array_equal(first[n], again[n]), n
    for img in range(b):
        one = run(dev, (1, c, s, heads, d), dict(I, x=I["x"][img:img + 1], del_y=I["del_y"][img:img + 1]))
        for n in PER_IMAGE:
            assert np.array_equal(one[n][0], first[n][img]), (img, n)


@pytest.mark.parametrize("case", [(3, 24, 16, 1, 16), (1, 7, 33, 1, 5), (9, 16, 9, 1, 8)], ids=str)
def test_one_head_is_the_fp32_batched_block(dev, case):
    I = host.inputs(case)
    one, got = run(dev, case, I, single=True), run(dev, case, I)
    assert set(one) == set(got) and "scores_raw" in got and "del_i" in got
    for n in one:
        assert np.array_equal(one[n], got[n]), n


def test_refusals_leave_the_outputs_untouched(dev):
    L = dev.lib()
    b, c, s, heads, d = case = (2, 16, 16, 4, 16)
    I = host.inputs(case)
    D = {n: dev.to_device(np.ascontiguousarray(a, F32)) for n, a in I.items()}
    O, fws, gws = buffers(dev, (2, 16, 65, 33, 8), False)          # buffers large enough for every refused shape: S = 65, 33 heads, D = 264 >= 4 x 65
    P = [D[n].ptr for n in ("wq", "wk", "wv", "w")]
    G = [O[n].ptr for n in host.GRADS]

    def fwd(c_, s_, heads_, d_, x=D["x"].ptr, ws=fws, batch=b):
        return L.bla_attention_forward_batched_f32_heads(None, batch, x, *P, D["bias"].ptr, C.byref(ws) if ws else None, O["out"].ptr, c_, s_, heads_, d_)

    def bwd(c_, s_, heads_, d_, dy=D["del_y"].ptr, partials=O["partials"].ptr, fw=fws, grad=gws, batch=b):
        return L.bla_attention_backward_batched_f32_heads(None, batch, dy, D["x"].ptr, *P, C.byref(fw), C.byref(grad), partials, *G, c_, s_, heads_, d_)
    for shape in [(c, 65, heads, d), (c, s, heads, 65), (c, s, 33, 8), (c, s, 0, d), (c, s, -1, d), (c, 0, heads, d), (c, s, heads, 0), (0, s, heads, d)]:
        assert fwd(*shape) == 1 and bwd(*shape) == 1, shape
    assert fwd(c, s, heads, d, x=None) == 1 and bwd(c, s, heads, d, dy=None) == 1 and bwd(c, s, heads, d, partials=None) == 1 and fwd(c, s, heads, d, ws=None) == 1
    no_p = dev.attention_ws(q=O["q"].ptr, k=O["k"].ptr, v=O["v"].ptr, attention=O["attention"].ptr)                                           # ws->weights NULL
    assert fwd(c, s, heads, d, ws=no_p) == 1 and bwd(c, s, heads, d, fw=no_p) == 1
    assert bwd(c, s, heads, d, grad=dev.attention_ws(q=O["del_q"].ptr, k=O["del_k"].ptr, v=O["del_v"].ptr)) == 1                              # grad->attention NULL
    assert fwd(c, s, 1, d) == 1 and bwd(c, s, 1, d) == 1                                                                # one head: scores_raw is required
    assert fwd(c, s, heads, d, batch=0) == 1 and bwd(c, s, heads, d, batch=0) == 1 and fwd(c, s, heads, d, batch=65536) == 1 and bwd(c, s, heads, d, batch=65536) == 1
    dev.sync()
    assert all(o.untouched() for o in O.values())
