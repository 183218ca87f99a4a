"""bla_attention_{forward,backward}_batched_online_bf16_heads on the device, against tests/test_attention_heads_host.py: cases, inputs, the
materialised float64 multi-head block, the restatement and the recorded rounded-against-exact values are that file's.

* Every output and saved tensor is a view between guard elements in an allocation filled with 0xFF bytes (tests/test_attention_online_gpu.py's Out); the
  guards must come back untouched, and every tensor starts 4 bytes off a 16-byte boundary.  `weights` is NULL throughout.
* Per tensor of OUTPUTS ||device - exact|| / ||exact|| <= 2 x the host-recorded value (DESIGN 3.25 - 3.29's margin for device-shared roundings); device and
  host values are printed side by side (profiles/r26_attention_heads_tests.txt).
* Per head, BIT FOR BIT: q, k, v, attention, lse, del_p, dots, del_q, del_k, del_v in the head's columns (head row) and the head's slices of del_wq, del_wk,
  del_wv, del_w equal what bla_attention_*_batched_online_bf16 gives on contiguous copies of the head's slices of the weights.
* The two sums across heads, bounded from the device's own tensors: out within D 2^-23 sum |r A| |r W| + 2^-23 |ref| of the float64 r(A_dev) r(W) + bias
  (the fp32 accumulation of D products; the bias addition), del_x within 3 D 2^-23 (sum |r Wq| |r del_q| + sum |r Wk| |r del_k| + sum |r Wv| |r del_v|) of the
  float64 sum of the three products of the device's own del_q, del_k, del_v (3 D products accumulated in fp32).  The worst ratio is printed.
* heads == 1 is the single-head online entry bit for bit in every tensor.
* The exact forward case: out, attention, k, v are the host's bits, q is zero, every head's lse is log(S) within 4 ulp.
* Two runs give the same bits in every tensor; image b of a batch equals a batch-1 run of image b.
* Refusals leave pattern-filled outputs untouched."""
import ctypes as C

import numpy as np
import pytest

import test_attention_heads_host as host
import test_attention_online_gpu as single
import test_attention_online_host as single_host
from test_attention_online_gpu import Out

pytestmark = pytest.mark.gpu
F32, U32 = np.float32, np.uint32
SAVED, GRADS, PER_IMAGE = single.SAVED, single.GRADS, single.PER_IMAGE
COLUMNS = ["q", "k", "v", "attention", "del_p", "del_q", "del_k", "del_v"]     # [B][S][D]: a head is d columns
ROWS = ["lse", "dots"]                                                         # [B][heads][S]: a head is a row


@pytest.fixture(scope="module")
def dev(pkg):
    pkg.init(0)
    return pkg


def shapes(case):
    b, c, s, heads, d = case
    D = heads * d
    return dict(single.shapes((b, c, s, D)), lse=(b, heads, s), dots=(b, heads, s))


def run(dev, case, I, backward=True):
    """both entries on fresh guarded buffers -> {tensor: its bit patterns}"""
    b, c, s, heads, d = case
    D = {n: dev.to_device(np.ascontiguousarray(a, F32)) for n, a in I.items()}
    O = {n: Out(dev, shp) for n, shp in shapes(case).items()}
    fws, gws = single.workspaces(dev, O)
    dev.attention_forward_batched_online_bf16_heads(b, D["x"], D["wq"], D["wk"], D["wv"], D["w"], D["bias"], fws, O["out"].ptr, c, s, heads, d)
    if backward:
        dev.attention_backward_batched_online_bf16_heads(b, D["del_y"], D["x"], D["wq"], D["wk"], D["wv"], D["w"], fws, gws, O["partials"].ptr, O["del_wq"].ptr,
                                                         O["del_wk"].ptr, O["del_wv"].ptr, O["del_w"].ptr, O["del_x"].ptr, c, s, heads, d)
    dev.sync()
    got = {n: O[n].bits() for n in SAVED + ["out"] + (GRADS if backward else [])}
    assert backward or all(O[n].untouched() for n in GRADS + ["partials"])
    return got


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
def test_against_the_materialised_float64_block(passes, case):
    I, exact, rounded, want = host.recorded(case)
    got = passes(case)
    have = {n: host.normwise(got[n].view(F32), exact[n]) for n in host.OUTPUTS}
    for n in host.OUTPUTS:
        print(f"{str(case):22s} {n:8s} device vs exact {have[n]:.3e}   host rounded vs exact {want[n]:.3e}   ratio {have[n] / want[n]:.2f}   "
              f"device vs rounded {host.normwise(got[n].view(F32), rounded[n]):.1e}")
    assert all(np.isfinite(got[n].view(F32)).all() for n in got)
    for n in host.OUTPUTS:
        assert have[n] <= 2 * want[n], (n, have[n], want[n])


@pytest.mark.parametrize("case", host.CASES, ids=str)
def test_a_head_is_the_single_head_entry_bit_for_bit(dev, passes, case):
    b, c, s, heads, d = case
    I = host.recorded(case)[0]
    got = passes(case)
    for h in range(heads):
        sl = slice(h * d, (h + 1) * d)
        one = single.run(dev, (b, c, s, d), host.head_inputs(I, h, d))
        for n in COLUMNS:
            assert np.array_equal(got[n][:, :, sl], one[n]), (h, n)
        for n in ROWS:
            assert np.array_equal(got[n][:, h], one[n]), (h, n)
        for n in ("del_wq", "del_wk", "del_wv"):
            assert np.array_equal(got[n][:, sl], one[n]), (h, n)
        assert np.array_equal(got["del_w"][sl], one["del_w"]), h


@pytest.mark.parametrize("case", host.CASES, ids=str)
def test_the_sums_across_heads_from_the_devices_own_tensors(passes, case):
    b, c, s, heads, d = case
    D = heads * d
    I = host.recorded(case)[0]
    got = passes(case)
    r64 = lambda a: host.rnd(np.asarray(a, np.float64))
    dev64 = lambda n: r64(got[n].view(F32))
    ra, rw = dev64("attention"), r64(I["w"])
    ref = np.swapaxes(ra @ rw + I["bias"].astype(np.float64), 1, 2)
    bound = D * 2.0 ** -23 * np.swapaxes(np.abs(ra) @ np.abs(rw), 1, 2) + 2.0 ** -23 * np.abs(ref)
    err = np.abs(got["out"].view(F32) - ref)
    worst_out = float((err / np.maximum(bound, 1e-300)).max())
    ref, bound = 0.0, 0.0
    for wn, gn in (("wq", "del_q"), ("wk", "del_k"), ("wv", "del_v")):
        rwm, rg = r64(I[wn]), np.swapaxes(dev64(gn), 1, 2)
        ref = ref + rwm @ rg
        bound = bound + np.abs(rwm) @ np.abs(rg)
    bound = 3 * D * 2.0 ** -23 * bound
    err_x = np.abs(got["del_x"].view(F32) - ref)
    worst_x = float((err_x / np.maximum(bound, 1e-300)).max())
    print(f"{str(case):22s} out error / bound {worst_out:.3f}   del_x error / bound {worst_x:.3f}")
    assert worst_out <= 1 and worst_x <= 1, (worst_out, worst_x)


@pytest.mark.parametrize("case", [(3, 64, 96, 16), (1, 16, 288, 16)], ids=str)
def test_one_head_is_the_single_head_entry(dev, case):
    b, c, s, d = case
    I = single_host.inputs(case)
    one, got = single.run(dev, case, I), run(dev, (b, c, s, 1, d), I)
    assert set(one) == set(got)
    for n in one:
        assert np.array_equal(one[n], got[n][:, 0] if n in ROWS else got[n]), n


@pytest.mark.parametrize("shape", host.EXACT, ids=str)
def test_exact_forward_case_bit_for_bit(dev, shape):
    s, c, heads, d = shape
    I = host.exact_inputs(s, c, heads * d)
    want = host.heads_block(I, heads, d, True, np.float32, backward=False)
    got = run(dev, (2, c, s, heads, d), I, backward=False)
    for n in ("out", "attention", "v", "k"):
        assert np.array_equal(got[n], np.ascontiguousarray(want[n], F32).view(U32)), n
    assert not got["q"].view(F32).any()
    log_s = np.float32(np.log(float(s)))
    assert (np.abs(got["lse"].view(F32).astype(np.float64) - np.log(float(s))) <= 4 * float(np.spacing(log_s))).all()


def test_second_run_and_batch_one(dev, passes):
    case = host.CASES[6]
    b, c, s, heads, d = case
    I = host.recorded(case)[0]
    first, again = passes(case), run(dev, case, I)
    for n in first:
        assert np.array_equal(first[n], again[n]), n
    for img in range(b):
        one = run(dev, (1, c, s, heads, d), dict(I, x=I["x"][img:img + 1], del_y=I["del_y"][img:img + 1]))
        for n in SAVED + ["out"] + PER_IMAGE:
            assert np.array_equal(one[n][0], first[n][img]), (img, n)


def test_refusals_leave_the_outputs_untouched(dev):
    L = dev.lib()
    case = (2, 64, 64, 4, 16)
    b, c, s, heads, d = case
    I = host.inputs(case)
    D = {n: dev.to_device(np.ascontiguousarray(a, F32)) for n, a in I.items()}
    O = {n: Out(dev, shp) for n, shp in shapes((2, 64, 4128, 4, 66)).items()}        # buffers large enough for every refused shape
    fws, gws = single.workspaces(dev, O)

    def fwd(c_, s_, heads_, d_, x=D["x"].ptr, ws=fws, batch=b):
        return L.bla_attention_forward_batched_online_bf16_heads(None, batch, x, D["wq"].ptr, D["wk"].ptr, D["wv"].ptr, D["w"].ptr, D["bias"].ptr,
                                                                 C.byref(ws) if ws else None, O["out"].ptr, c_, s_, heads_, d_)

    def bwd(c_, s_, heads_, d_, dy=D["del_y"].ptr, partials=O["partials"].ptr, fw=fws, grad=gws, batch=b):
        return L.bla_attention_backward_batched_online_bf16_heads(None, batch, dy, D["x"].ptr, D["wq"].ptr, D["wk"].ptr, D["wv"].ptr, D["w"].ptr, C.byref(fw),
                                                                  C.byref(grad), partials, O["del_wq"].ptr, O["del_wk"].ptr, O["del_wv"].ptr, O["del_w"].ptr,
                                                                  O["del_x"].ptr, c_, s_, heads_, d_)
    for shape in [(c, s, 33, 8), (c, s, 11, 24), (c, s, 0, d), (c, s, -1, d), (c, s, heads, 4), (c, 16, heads, d), (c, 4128, heads, d), (12, s, heads, d)]:
        assert fwd(*shape) == 1 and bwd(*shape) == 1, shape                           # heads d = 264 twice, no head, d = 4, s = 16, s = 4128, c = 12
    assert fwd(c, s, heads, d, x=None) == 1 and bwd(c, s, heads, d, dy=None) == 1 and bwd(c, s, heads, d, partials=None) == 1 and fwd(c, s, heads, d, ws=None) == 1
    no_lse = dev.attention_ws(q=O["q"].ptr, k=O["k"].ptr, v=O["v"].ptr, attention=O["attention"].ptr)                                         # ws->scores_raw NULL
    assert fwd(c, s, heads, d, ws=no_lse) == 1 and bwd(c, s, heads, d, fw=no_lse) == 1
    assert bwd(c, s, heads, d, grad=dev.attention_ws(q=O["del_q"].ptr, k=O["del_k"].ptr, v=O["del_v"].ptr, attention=O["del_p"].ptr)) == 1    # grad->scores_raw NULL
    assert bwd(c, s, heads, d, grad=dev.attention_ws(q=O["del_q"].ptr, k=O["del_k"].ptr, v=O["del_v"].ptr, scores_raw=O["dots"].ptr)) == 1    # grad->attention NULL
    assert fwd(c, s, heads, d, batch=0) == 1 and bwd(c, s, heads, d, batch=0) == 1 and fwd(c, s, heads, d, batch=65536) == 1
    dev.sync()
    assert all(o.untouched() for o in O.values())
