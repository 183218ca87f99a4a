"""bla_attention_{forward,backward}_batched_online_bf16 and the model's mode 3 on the device, against tests/test_attention_online_host.py:
cases, inputs, the materialised float64 block, the online restatement and the recorded rounded-against-exact values are that file's.

* Every output and saved tensor is a view between guard elements in an allocation filled with 0xFF bytes; the guards must come back untouched.  GUARD is
  odd, so every such tensor starts 4 bytes off a 16-byte boundary: the entries ask for float alignment only.  `weights` is NULL throughout.
* Per tensor ||device - exact|| / ||exact|| <= 2 x the host-recorded value, `exact` being the MATERIALISED float64 block (DESIGN 3.25 - 3.27's margin for
  device-shared roundings).  Device and host values are printed side by side (profiles/r25_attention_online_tests.txt).
* Saved tensors: q, k, v are the materialising bf16 entry's bits where that entry applies, and inside its accumulation bound everywhere; lse lies within
      max_j(inv d 2^-23 sum |r q_i| |r k_j|) + (S / KB + 16) 2^-23 + 2^-23 |lse_i|
  of the float64 log-sum-exp of inv r(q_dev) r(k_dev)^T (the fp32 accumulation of T; one rounding of l per key block plus exp and log; the final sum);
  the row dots lie within d 2^-23 sum |del_P| |A| of the float64 dot of the device's own del_P and A; del_P within C 2^-23 sum |r dy| |r w|.
* The exact forward case: out, attention, k, v are the host's bits, q is zero, lse is log(S) within 4 ulp.
* Two runs give the same bits in every tensor; image b of a batch equals a batch-1 run of image b.
* Refusals leave pattern-filled outputs untouched.
* Model at 40 x 48 images: the 20 x 24 level (S = 480) runs the online entries under mode 3 and nothing else can; the 5 x 6 mid block stays fp32."""
import ctypes as C

import numpy as np
import pytest

import test_attention_bf16_host as old_host
import test_attention_online_host as host
import test_unet_bf16_host as unet_host

pytestmark = pytest.mark.gpu
F32, U32 = np.float32, np.uint32
GUARD = 61
SAVED = ["q", "k", "v", "lse", "attention"]
GRADS = ["del_q", "del_k", "del_v", "del_p", "dots", "del_wq", "del_wk", "del_wv", "del_w", "del_x"]
PER_IMAGE = ["del_q", "del_k", "del_v", "del_p", "dots", "del_x"]


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


def shapes(shape):
    b, c, s, d = shape
    return dict(q=(b, s, d), k=(b, s, d), v=(b, s, d), lse=(b, s), attention=(b, s, d), out=(b, c, s), del_q=(b, s, d), del_k=(b, s, d), del_v=(b, s, d),
                del_p=(b, s, d), dots=(b, s), del_wq=(c, d), del_wk=(c, d), del_wv=(c, d), del_w=(d, c), del_x=(b, c, s), partials=(b, 4 * c * d))


def workspaces(dev, O):
    fws = dev.attention_ws(q=O["q"].ptr, k=O["k"].ptr, v=O["v"].ptr, scores_raw=O["lse"].ptr, attention=O["attention"].ptr)
    gws = dev.attention_ws(q=O["del_q"].ptr, k=O["del_k"].ptr, v=O["del_v"].ptr, scores_raw=O["dots"].ptr, attention=O["del_p"].ptr)
    return fws, gws


def run(dev, shape, I, backward=True):
    """both entries on fresh guarded buffers -> {tensor: its bit patterns}"""
    b, c, s, d = shape
    D = {n: dev.to_device(np.ascontiguousarray(a, F32)) for n, a in I.items()}
    O = {n: Out(dev, shp) for n, shp in shapes(shape).items()}
    fws, gws = workspaces(dev, O)
    dev.attention_forward_batched_online_bf16(b, D["x"], D["wq"], D["wk"], D["wv"], D["w"], D["bias"], fws, O["out"].ptr, c, s, d)
    if backward:
        dev.attention_backward_batched_online_bf16(b, D["del_y"], D["x"], D["wq"], D["wk"], D["wv"], D["w"], fws, gws, O["partials"].ptr, O["del_wq"].ptr, O["del_wk"].ptr,
                                                   O["del_wv"].ptr, O["del_w"].ptr, O["del_x"].ptr, c, s, d)
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
            cache[case] = run(dev, host.shape_of(case), host.recorded(case)[0])
        return cache[case]
    return get


@pytest.mark.parametrize("case", host.ALL, ids=str)
def test_against_the_materialised_float64_block(passes, case):
    """Measured on an MI355X (profiles/r25_attention_online_tests.txt): device / recorded 1.00 in all 81 tensors of the nine inputs, and the
    device within 2e-4 normwise of the rounded restatement itself."""
    I, exact, rounded, diff = host.recorded(case)
    got = passes(case)
    names = host.OUTPUTS + ["del_q", "del_k", "del_v"]
    want = dict(diff, **{n: host.normwise(rounded[n], exact[n]) for n in ("del_q", "del_k", "del_v")})
    have = {n: host.normwise(got[n].view(F32), exact[n]) for n in names}
    for n in names:
        print(f"{str(case):22s} {n:8s} device vs exact {have[n]:.3e}   host rounded vs exact {want[n]:.3e}   ratio {have[n] / want[n]:.2f}   "
              f"device vs rounded {host.normwise(got[n].view(F32), rounded[n]):.1e}")
    assert all(np.isfinite(got[n].view(F32)).all() for n in got)
    for n in (["out"] if case == host.LARGE else names):      # at logits of +-60 and beyond: finite everywhere, and `out` held to its bound
        assert have[n] <= 2 * want[n], (n, have[n], want[n])


@pytest.mark.parametrize("case", host.ALL, ids=str)
def test_saved_tensors(dev, passes, case):
    b, c, s, d = shape = host.shape_of(case)
    I, _, rounded, _ = host.recorded(case)
    got = passes(case)
    z = host.rnd(np.swapaxes(I["x"].astype(np.float64), 1, 2))
    for n, w in (("q", "wq"), ("k", "wk"), ("v", "wv")):
        rw = host.rnd(I[w].astype(np.float64))
        err = np.abs(got[n].view(F32) - z @ rw)
        bound = c * 2.0 ** -23 * (np.abs(z) @ np.abs(rw))
        assert (err <= bound).all(), (n, float((err / np.maximum(bound, 1e-300)).max()))
    if old_host_applies(dev, shape):      # the same kernel: the same bits
        D = {n: dev.to_device(np.ascontiguousarray(a, F32)) for n, a in I.items()}
        O = {n: Out(dev, shp) for n, shp in dict(shapes(shape), weights=(b, s, s)).items()}
        ws = dev.attention_ws(q=O["q"].ptr, k=O["k"].ptr, v=O["v"].ptr, weights=O["weights"].ptr, attention=O["attention"].ptr)
        dev.attention_forward_batched_bf16(b, D["x"], D["wq"], D["wk"], D["wv"], D["w"], D["bias"], ws, O["out"].ptr, c, s, d)
        dev.sync()
        for n in ("q", "k", "v"):
            assert np.array_equal(O[n].bits(), got[n]), n
    # lse against the float64 log-sum-exp of the device's own q and k
    inv = float(np.float32(1.0 / np.sqrt(float(d))))
    dp, att = got["del_p"].view(F32).astype(np.float64), got["attention"].view(F32).astype(np.float64)
    worst = 0.0
    for img in range(b):      # (one image at a time: S x S float64)
        rq, rk = host.rnd(got["q"][img].view(F32).astype(np.float64)), host.rnd(got["k"][img].view(F32).astype(np.float64))
        t = inv * (rq @ rk.T)
        mx = t.max(axis=1)
        want = mx + np.log(np.exp(t - mx[:, None]).sum(axis=1))
        bound = (inv * d * 2.0 ** -23 * (np.abs(rq) @ np.abs(rk).T)).max(axis=1) + (s / host.KB + 16) * 2.0 ** -23 + 2.0 ** -23 * np.abs(want)
        err = np.abs(got["lse"][img].view(F32) - want)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (img, float((err / bound).max()))
    want = (dp * att).sum(axis=2)
    bound = d * 2.0 ** -23 * (np.abs(dp) * np.abs(att)).sum(axis=2)
    err = np.abs(got["dots"].view(F32) - want)
    print(f"{str(case):22s} lse error / bound {worst:.3f}   row dots error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    dyt, rw = host.rnd(np.swapaxes(I["del_y"].astype(np.float64), 1, 2)), host.rnd(I["w"].astype(np.float64))
    assert (np.abs(dp - dyt @ rw.T) <= c * 2.0 ** -23 * (np.abs(dyt) @ np.abs(rw.T))).all()
    assert host.normwise(got["attention"].view(F32), rounded["attention"]) < 1e-2 and host.normwise(got["lse"].view(F32), rounded["lse"][..., 0]) < 1e-2


def old_host_applies(dev, shape):
    return dev.attention_bf16_applies(shape[1], shape[2], shape[3])


def test_the_cases_reach_both_sides_of_the_old_limit(dev):
    assert [old_host_applies(dev, host.shape_of(c)) for c in host.CASES] == [True, True] + [False] * 5
    assert all(dev.attention_online_bf16_applies(*host.shape_of(c)[1:]) for c in host.ALL)


@pytest.mark.parametrize("s", [32, 512, 1024])
def test_exact_forward_case_bit_for_bit(dev, s):
    I = host.exact_inputs(s)
    want = host.online_block(I, True, np.float32, backward=False)
    got = run(dev, (2, 16, s, 16), I, backward=False)
    for n in ("out", "attention", "v", "k"):
        assert np.array_equal(got[n], np.ascontiguousarray(want[n], F32).view(U32)), n
    assert not got["q"].view(F32).any()
    log_s = np.float32(np.log(float(s)))
    assert (np.abs(got["lse"].view(F32).astype(np.float64) - np.log(float(s))) <= 4 * float(np.spacing(log_s))).all()


def test_second_run_and_batch_one(dev, passes):
    case = host.CASES[1]
    b, c, s, d = case
    I = host.recorded(case)[0]
    first, again = passes(case), run(dev, case, I)
    for n in first:
        assert np.array_equal(first[n], again[n]), n
    for img in range(b):
        one = run(dev, (1, c, s, d), dict(I, x=I["x"][img:img + 1], del_y=I["del_y"][img:img + 1]))
        for n in SAVED + ["out"] + PER_IMAGE:
            assert np.array_equal(one[n][0], first[n][img]), (img, n)


def test_refusals_leave_the_outputs_untouched(dev):
    L = dev.lib()
    case = (2, 64, 64, 16)
    b, c, s, d = case
    I = host.make_inputs(case)
    D = {n: dev.to_device(np.ascontiguousarray(a, F32)) for n, a in I.items()}
    big = (2, 64, 4128, 72)        # buffers large enough for every refused shape
    O = {n: Out(dev, shp) for n, shp in shapes(big).items()}
    fws, gws = workspaces(dev, O)

    def fwd(c_, s_, d_, x=D["x"].ptr, ws=fws, batch=b):
        return L.bla_attention_forward_batched_online_bf16(None, batch, x, D["wq"].ptr, D["wk"].ptr, D["wv"].ptr, D["w"].ptr, D["bias"].ptr, C.byref(ws) if ws else None,
                                                           O["out"].ptr, c_, s_, d_)

    def bwd(c_, s_, d_, dy=D["del_y"].ptr, partials=O["partials"].ptr, fw=fws, grad=gws, batch=b):
        return L.bla_attention_backward_batched_online_bf16(None, batch, dy, D["x"].ptr, D["wq"].ptr, D["wk"].ptr, D["wv"].ptr, D["w"].ptr, C.byref(fw), C.byref(grad),
                                                            partials, O["del_wq"].ptr, O["del_wk"].ptr, O["del_wv"].ptr, O["del_w"].ptr, O["del_x"].ptr, c_, s_, d_)
    for shape in [(c, 16, d), (c, 4128, d), (c, s, 4), (c, s, 72), (12, s, d)]:
        assert fwd(*shape) == 1 and bwd(*shape) == 1, shape
    assert fwd(c, s, d, x=None) == 1 and bwd(c, s, d, dy=None) == 1 and bwd(c, s, d, partials=None) == 1 and fwd(c, s, d, ws=None) == 1
    no_lse = dev.attention_ws(q=O["q"].ptr, k=O["k"].ptr, v=O["v"].ptr, attention=O["attention"].ptr)                                             # ws->scores_raw NULL
    assert fwd(c, s, d, ws=no_lse) == 1 and bwd(c, s, d, fw=no_lse) == 1
    assert bwd(c, s, d, grad=dev.attention_ws(q=O["del_q"].ptr, k=O["del_k"].ptr, v=O["del_v"].ptr, scores_raw=O["dots"].ptr)) == 1             # grad->attention NULL
    assert bwd(c, s, d, grad=dev.attention_ws(q=O["del_q"].ptr, k=O["del_k"].ptr, v=O["del_v"].ptr, attention=O["del_p"].ptr)) == 1             # grad->scores_raw NULL
    assert fwd(c, s, d, batch=0) == 1 and bwd(c, s, d, batch=0) == 1 and fwd(c, s, d, batch=65536) == 1
    dev.sync()
    assert all(o.untouched() for o in O.values())


# ---- the model ----------------------------------------------------------------------------------------------------------------------------------------
def test_model_online_attention_switch(dev):
    """tests/test_unet_bf16_host.py's configuration on 40 x 48 images, batch 2: the four attention blocks of the 20 x 24 level (C = 64, S = 480, key_dim 8)
    run the online entries under mode 3 and are refused by the materialising bf16 entry; the 5 x 6 mid block (S = 30) stays on the fp32 entries."""
    import test_unet_bf16_gpu as ug
    pkg, L = dev, dev.lib()
    cfg, B = dict(unet_host.CFG, image_h=40, image_w=48), 2
    ONLINE = pkg.UNET_ATTENTION_BF16_ONLINE
    assert pkg.attention_online_bf16_applies(cfg["dims"][1], 480, cfg["key_dim"]) and not pkg.attention_bf16_applies(cfg["dims"][1], 480, cfg["key_dim"])
    assert not pkg.attention_online_bf16_applies(cfg["dims"][3], 30, cfg["key_dim"])
    x, temb, noise, drop = unet_host.make_inputs(cfg, B)
    dd = unet_host.device_drop_layout(drop, cfg)
    data = dict(x=pkg.to_device(x), temb=pkg.to_device(temb), noise=pkg.to_device(noise), drop=pkg.DeviceArray((dd.size,), np.uint8).copy_from(dd))
    P = unet_host.make_params(cfg)
    Z = {n: (np.zeros_like(v) if "attention" in n and not n.endswith("biases") else v) for n, v in P.items()}
    for products in (ug.F32, ug.BF16):
        # attention matrices zero: the same values in both attention modes (compared as numbers: a zero's sign is not part of the claim)
        m = ug.Model(pkg, cfg, B, products, Z)
        assert L.bla_unet_attention(m.h) == pkg.UNET_ATTENTION_F32
        o0, g0 = ug.one_pass(m, data)
        pkg.unet_set_attention(m.h, ONLINE)
        assert L.bla_unet_attention(m.h) == ONLINE == pkg.unet_attention(m.h)
        for bad in (2, -1, 7):
            assert L.bla_unet_set_attention(m.h, bad) == 1 and L.bla_unet_attention(m.h) == ONLINE
        o1, g1 = ug.one_pass(m, data)
        assert np.isfinite(g0).all() and np.abs(g0).max() > 0
        assert np.array_equal(o0, o1) and np.array_equal(g0, g1)
        m.destroy()
        # the real parameters: mode 3 is another arithmetic in the blocks that qualify, mode 0 afterwards is the first pass again, mode 1 is mode 0 here
        m = ug.Model(pkg, cfg, B, products, P)
        o0, g0 = ug.one_pass(m, data)
        pkg.unet_set_attention(m.h, ONLINE)
        o1, g1 = ug.one_pass(m, data)
        o1b, g1b = ug.one_pass(m, data)
        pkg.unet_set_attention(m.h, pkg.UNET_ATTENTION_F32)
        assert L.bla_unet_attention(m.h) == pkg.UNET_ATTENTION_F32
        o2, g2 = ug.one_pass(m, data)
        pkg.unet_set_attention(m.h, pkg.UNET_ATTENTION_BF16)
        o3, g3 = ug.one_pass(m, data)
        assert np.array_equal(o0.view(U32), o2.view(U32)) and np.array_equal(g0.view(U32), g2.view(U32))
        assert np.array_equal(o0.view(U32), o3.view(U32)) and np.array_equal(g0.view(U32), g3.view(U32))      # nothing qualifies for the materialising entry
        assert np.array_equal(o1.view(U32), o1b.view(U32)) and np.array_equal(g1.view(U32), g1b.view(U32))
        assert np.isfinite(o1).all() and np.isfinite(g1).all()
        assert not np.array_equal(o0, o1) and not np.array_equal(g0, g1)
        att = [(off, cnt) for name, off, cnt in m.tensors if "attention" in name and not name.startswith("mid") and not name.endswith("biases")]
        assert len(att) == 16
        for off, cnt in att:        # every routed block's gradients moved, by a rounding's worth and no more
            a, b_ = g1[off:off + cnt].astype(np.float64), g0[off:off + cnt].astype(np.float64)
            moved = np.linalg.norm(a - b_) / np.linalg.norm(b_)
            print(f"products {products}: attention gradient tensor at {off} moved by {moved:.2e}")
            assert 0 < moved <= 0.25, moved
        m.destroy()
