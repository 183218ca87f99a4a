"""The fp32 self-attention block (bla_attention_{forward,backward}[_batched]_f32, csrc/bla_attention_f32.hip) at shapes off the three golden ones, against float64.

The reference is always oracle.attention_forward / attention_backward in float64, image by image; a batch's weight gradients are the float64 sums over its
images.  The single-image device block is never the reference.  Checked: every saved forward tensor (q, k, v, scores_raw, weights, attention, out), the five
gradients, and -- the only window on the softmax-Jacobian kernel and its fused scale -- the gradient workspace's scores_raw against float64 del_I.  Both
jacobian_from_raw values wherever a backward runs.  Every output is a view between guard elements in an allocation of 0xFF bytes.

Single image (C, S, d): (7, 33, 5) everything odd; (24, 49, 8); (40, 100, 12); (96, 64, 16); (64, 1024, 16) -- 4 MB of scores, softmax rows of 1024, products
that leave the latency-bound pair kernel.
Batch (B, C, S, d): (7, 8, 9, 4) batch_sum's scalar tail alone; (8, 24, 49, 8) exactly one unrolled group of eight; (11, 40, 100, 12) a group of eight and
a tail of three, del_X through three beta = 1 products; (17, 32, 64, 16); (16, 256, 256, 16) del_X through the three-part thin launch (asserted).

Tolerance, tests/test_attention.py's form: |got - ref| <= t |ref| + t mean|ref| (the mean over the compared tensor), t = 2e-5 for forward tensors and 5e-5
for gradients and del_I.  What that leaves the device is measured on the host, never on the device: restate_f32() below is the block in NumPy fp32 (the
kernels' composition, NumPy's summation order), and `python tests/test_attention_paths_gpu.py` prints its worst |err| / limit per case, Jacobian mode and
tensor.  Rule: where the restatement stays within 0.25 of the limit, t as it stands; where it exceeds that, t for that tensor = 4 x (the restatement's worst
ratio) x the base t -- the 4 covers the MFMA and split-K summation order and expf.  Measured (both modes):
  * the five single-image cases and the first four batches: at most 0.12 (del_x of (17, 32, 64, 16), raw-scores Jacobian), except del_I of (64, 1024, 16) at
    0.221; all below 0.25, t unchanged.
  * (16, 256, 256, 16): weights 0.278, attention 0.449, out 0.483 (means over 256 keys that nearly cancel), del_x 0.270, del_I 1.167 (weights times a
    difference that cancels: fp32 itself misses the base limit there); every other tensor at most 0.18.  Hence t = 2.23e-5, 3.60e-5, 3.87e-5 for the three
    forward tensors, 5.40e-5 for del_x and 2.34e-4 for del_I (WIDER below).
The device's own ratios are printed before anything is asserted (profiles/r23_unet_paths_tests.txt: at most 0.11 of the limit on the nine unchanged cases,
0.13 ... 0.19 of the widened limits at (16, 256, 256, 16))."""
import ctypes as C

import numpy as np
import pytest

import conftest  # noqa: F401  (as a script too: the search path of the oracle and the input generators)
from inputs import uniform
from test_unet_glue_paths_gpu import Guarded

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
T_FWD, T_BWD = 2e-5, 5e-5
SAVED = ["q", "k", "v", "scores_raw", "weights", "attention"]
FWD = SAVED + ["out"]
ORA = dict(q="q", k="k", v="v", scores_raw="raw", weights="wts", attention="att", out="out")
GRADS = ["del_wq", "del_wk", "del_wv", "del_w", "del_x"]
PER_IMAGE = FWD + ["del_x", "del_i"]

SINGLE = [(7, 33, 5), (24, 49, 8), (40, 100, 12), (96, 64, 16), (64, 1024, 16)]
BATCHED = [(7, 8, 9, 4), (8, 24, 49, 8), (11, 40, 100, 12), (17, 32, 64, 16), (16, 256, 256, 16)]
# {case: {tensor: worst |err| / limit of restate_f32() at the base t}} where that exceeds 0.25 (`python tests/test_attention_paths_gpu.py` prints all of them);
# t for that tensor = 4 x ratio x base t
WIDER = {(16, 256, 256, 16): {"weights": 0.278, "attention": 0.449, "out": 0.483, "del_x": 0.270, "del_i": 1.167}}


def tol(case, name):
    base = T_FWD if name in FWD else T_BWD
    r = WIDER.get(case, {}).get(name)
    return base if r is None else 4 * r * base


def make_inputs(case):
    b, c, s, d = case
    u = lambda k, shape, lo, hi: uniform(8900 + 100 * b + c + k, shape, lo, hi, F32)      # tests/test_unet_batched.py's ranges
    return dict(x=u(0, (b, c, s), -1, 1), del_y=u(1, (b, c, s), -1, 1), wq=u(2, (c, d), -0.3, 0.3), wk=u(3, (c, d), -0.3, 0.3), wv=u(4, (c, d), -0.3, 0.3),
                w=u(5, (d, c), -0.3, 0.3), bias=u(6, (c,), -0.1, 0.1))


_REF = {}


def reference(ora, case):
    """{jacobian_from_raw: {tensor: float64}} -- per-image tensors stacked over the batch, weight gradients summed over it; computed once per case"""
    if case in _REF:
        return _REF[case]
    b, c, s, d = case
    I = {n: a.astype(F64) for n, a in make_inputs(case).items()}
    P = [I[n] for n in ("wq", "wk", "wv", "w")]
    inv = 1.0 / np.sqrt(float(d))
    fwd = [ora.attention_forward(I["x"][i], *P, I["bias"]) for i in range(b)]
    out = {}
    for jr in (0, 1):
        R = {n: np.stack([f[ORA[n]] for f in fwd]) for n in FWD}
        bwd = [ora.attention_backward(I["del_y"][i], I["x"][i], *P, fwd[i], jacobian_from_raw=bool(jr)) for i in range(b)]
        R["del_x"] = np.stack([g["del_x"] for g in bwd])
        for n in GRADS[:4]:
            R[n] = np.sum([g[n] for g in bwd], axis=0)
        di = []
        for i in range(b):          # del_I = J(del_P V^T) / sqrt(d), J from the softmax output or (jacobian_from_raw) from the scaled scores
            del_s = (I["del_y"][i].T @ I["w"].T) @ fwd[i]["v"].T
            src = fwd[i]["raw"] if jr else fwd[i]["wts"]
            di.append(src * (del_s - (src * del_s).sum(axis=1, keepdims=True)) * inv)
        R["del_i"] = np.stack(di)
        out[jr] = R
    _REF[case] = out
    return out


def restate_f32(case, jr):
    """the device's composition in NumPy fp32 (dot of the Jacobian in double, rounded once, as the kernel has it) -- what fp32 itself costs against float64"""
    b, c, s, d = case
    I = make_inputs(case)
    inv = F32(1.0 / np.sqrt(float(d)))
    R = {n: [] for n in PER_IMAGE}
    G = {n: np.zeros((d, c) if n == "del_w" else (c, d), F32) for n in GRADS[:4]}
    for i in range(b):
        x, dy = I["x"][i], I["del_y"][i]
        z = x.T
        q, k, v = z @ I["wq"], z @ I["wk"], z @ I["wv"]
        raw = (q @ k.T) * inv
        e = np.exp(raw - raw.max(axis=1, keepdims=True))
        wts = e / e.sum(axis=1, keepdims=True, dtype=F32)
        att = wts @ v
        outp = (att @ I["w"] + I["bias"]).T
        dyp = dy.T
        G["del_w"] += att.T @ dyp
        del_p = dyp @ I["w"].T
        del_s = del_p @ v.T
        del_v = wts.T @ del_p
        src = raw if jr else wts
        dot = (src.astype(F64) * del_s).sum(axis=1, keepdims=True).astype(F32)
        del_i = (src * (del_s - dot)) * inv
        del_q, del_k = del_i @ k, del_i.T @ q
        G["del_wk"] += x @ del_k; G["del_wq"] += x @ del_q; G["del_wv"] += x @ del_v
        del_x = (I["wq"] @ del_q.T + I["wk"] @ del_k.T) + I["wv"] @ del_v.T
        for n, a in dict(q=q, k=k, v=v, scores_raw=raw, weights=wts, attention=att, out=outp, del_x=del_x, del_i=del_i).items():
            assert a.dtype == F32
            R[n].append(a)
    R = {n: np.stack(a) for n, a in R.items()}
    R.update(G)
    return R


def ratios(case, got, ref, names):
    """{tensor: worst |got - ref| / (t |ref| + t mean|ref|)} at this case's t"""
    out = {}
    for n in names:
        r = ref[n].reshape(np.shape(got[n]))
        t = tol(case, n)
        out[n] = float((np.abs(got[n].astype(F64) - r) / (t * np.abs(r) + t * np.abs(r).mean())).max())
    return out


def report(case, tag, rs):
    print(f"{str(case):20s} {tag:10s} " + "  ".join(f"{n} {v:.3f}" for n, v in rs.items()))


@pytest.fixture(scope="module")
def dev(pkg):
    pkg.init(0)
    return pkg


def device_block(dev, case, batched):
    """forward once, backward in both Jacobian modes, on fresh guarded buffers -> {jr: {tensor: fp32 array}}, {jr: name of the last product's kernel}"""
    L, chk, N = dev.lib(), dev.native.check, dev.native
    b, c, s, d = case
    I = make_inputs(case)
    D = {n: dev.to_device(a) for n, a in I.items()}
    shp = dict(q=(b, s, d), k=(b, s, d), v=(b, s, d), scores_raw=(b, s, s), weights=(b, s, s), attention=(b, s, d))

    def ws():
        bufs = {n: Guarded(dev, shp[n]) for n in SAVED}
        return bufs, N.AttentionWs(*[bufs[n].ptr for n in SAVED])
    fb, fws = ws()
    out = Guarded(dev, (b, c, s))
    P = [D[n].ptr for n in ("wq", "wk", "wv", "w")]
    if batched:
        chk(L.bla_attention_forward_batched_f32(None, b, D["x"].ptr, *P, D["bias"].ptr, C.byref(fws), out.ptr, c, s, d))
    else:
        chk(L.bla_attention_forward_f32(None, D["x"].ptr, *P, D["bias"].ptr, C.byref(fws), out.ptr, c, s, d))
    fwd = {n: fb[n].f32() for n in SAVED}; fwd["out"] = out.f32()
    got, last = {}, {}
    for jr in (0, 1):
        gb, gws = ws()
        O = dict(del_wq=Guarded(dev, (c, d)), del_wk=Guarded(dev, (c, d)), del_wv=Guarded(dev, (c, d)), del_w=Guarded(dev, (d, c)), del_x=Guarded(dev, (b, c, s)))
        part = Guarded(dev, (b, c * d))
        if batched:
            chk(L.bla_attention_backward_batched_f32(None, b, D["del_y"].ptr, D["x"].ptr, *P, C.byref(fws), C.byref(gws), part.ptr,
                                                     *[O[n].ptr for n in GRADS], c, s, d, jr))
        else:
            chk(L.bla_attention_backward_f32(None, D["del_y"].ptr, D["x"].ptr, *P, C.byref(fws), C.byref(gws), *[O[n].ptr for n in GRADS], c, s, d, jr))
        last[jr] = L.bla_gemm_last_kernel().decode()
        got[jr] = dict(fwd, del_i=gb["scores_raw"].f32(), **{n: O[n].f32() for n in GRADS})
        part.bits()                                                              # (its guards)
        for n in SAVED:                                                          # the backward leaves the saved tensors as they were
            assert np.array_equal(fb[n].f32(), fwd[n]), n
    return got, last


def hold(case, got, ref):
    worst = {}
    for jr in (0, 1):
        rs = ratios(case, got[jr], ref[jr], (FWD if jr == 0 else []) + GRADS + ["del_i"])
        report(case, f"device j{jr}", rs)
        worst.update({(jr, n): v for n, v in rs.items() if not v <= 1})
    assert not worst, worst


@pytest.mark.parametrize("cfg", SINGLE, ids=str)
def test_single_image_block_against_float64(dev, ora, cfg):
    case = (1,) + cfg
    got, _ = device_block(dev, case, batched=False)
    hold(case, got, reference(ora, case))


@pytest.mark.parametrize("case", BATCHED, ids=str)
def test_batched_block_against_float64(dev, ora, case):
    b, c, s, d = case
    got, last = device_block(dev, case, batched=True)
    thin = d % 8 == 0 and 8 <= d <= 64 and c % 32 == 0 and s % 32 == 0 and b * c * s >= 1 << 20      # gemm_thin_applies(c, s, d, batch)
    assert thin == (case == (16, 256, 256, 16))
    for jr in (0, 1):       # del_X is the last product: three-part thin launch, or three products with beta = 1
        assert last[jr].startswith("gemm_f32_thin") == thin, (jr, last[jr])
    hold(case, got, reference(ora, case))


if __name__ == "__main__":          # the host measurement the tolerances rest on (no device involved)
    import oracle
    oracle.build()
    for case in [(1,) + cfg for cfg in SINGLE] + BATCHED:
        ref = reference(oracle, case)
        for jr in (0, 1):
            saved, WIDER = WIDER, {}          # ratios at the base t
            rs = ratios(case, restate_f32(case, jr), ref[jr], (FWD if jr == 0 else []) + GRADS + ["del_i"])
            WIDER = saved
            report(case, f"fp32 j{jr}", rs)
