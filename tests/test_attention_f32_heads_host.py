"""The fp32 multi-head attention block for short sequences (bla_attention_{forward,backward}_batched_f32_heads) restated in numpy, on the host.

f32_heads_block() is include/bla.h's arithmetic line by line: Q, K, V at the block's width D = heads d; per head h (columns h d .. h d + d - 1) the materialised
softmax of inv Q_h K_h^T with inv from the HEAD's width, A_h = P_h V_h, and backwards del_S_h, the row dot <P_h, del_S_h> (double, rounded once), del_I_h,
del_V_h, del_Q_h, del_K_h; out, del_P, the weight gradients and del_X across all D columns.  In float64 it is the device's reference restated; in float32 it is
what fp32 itself costs against that reference (NumPy's summation order), which is what the device tolerance rests on.

reference(case) is the float64 multi-head block COMPOSED from tests/test_attention_bf16_host.py's block(I_h, False) on each head's slices of the weights
(tests/test_attention_heads_host.py's compose / head_inputs), plus P as [B][heads][S][S] and del_P = del_Y' W^T.  tests/test_attention_f32_heads_gpu.py reads
cases, inputs, reference and tolerance here.

Tolerance, tests/test_attention_paths_gpu.py's form and rule: |got - ref| <= t |ref| + t mean|ref| (the mean over the compared tensor), t = 2e-5 for forward
tensors and 5e-5 for gradients; where the float32 restatement exceeds 0.25 of that limit, t for that tensor = 4 x its ratio x the base t (WIDER).  Measured here
(`python tests/test_attention_f32_heads_host.py` prints every ratio): the worst is 0.081 (attention of (2, 48, 64, 4, 64)); per case at most 0.006, 0.031,
0.040, 0.027, 0.081, 0.025 in CASES' order.  Nothing widens: WIDER is empty.

Host-only requirements:
  * the float64 restatement IS the composed reference (1e-12 normwise in every tensor);
  * the float32 restatement stays within 0.25 of the limit (or inside WIDER's entry);
  * three wrong multi-head blocks -- inv from D, the row dot over all D, del_P from the next head's rows of W -- each break the device tolerance;
  * bla_attention_f32_heads_applies over its boundary values, heads = 1 included; the entries refuse bad shapes and NULLs without touching a device."""
import ctypes as C
import functools

import numpy as np
import pytest

import conftest  # noqa: F401  (as a script too: the search path of the input generators)
from test_attention_bf16_host import make_inputs, block
from test_attention_heads_host import compose, head_inputs

F32, F64 = np.float32, np.float64
# (B, C, S, heads, d)
CASES = [(2, 8, 1, 2, 4),             # one key: softmax of a single element
         (3, 24, 16, 4, 16),          # the model's mid block
         (2, 40, 30, 3, 12),          # the 40 x 48 model's mid block; odd heads; d off 8
         (1, 7, 33, 2, 5),            # everything odd
         (2, 48, 64, 4, 64),          # every limit at once, D = 256, the LDS attribute
         (9, 16, 9, 2, 8)]            # batch past eight: batch_sum's unrolled group and its tail
T_FWD, T_BWD = 2e-5, 5e-5
FWD = ["q", "k", "v", "weights", "attention", "out"]
GRADS = ["del_wq", "del_wk", "del_wv", "del_w", "del_x"]
WORK = ["del_p", "del_q", "del_k", "del_v"]                    # the gradient workspace: attention (= del_P), q, k, v
ALL = FWD + GRADS + WORK
MUTATIONS = ["inv_from_width", "rowdot_over_width", "del_p_from_next_head"]
# {case: {tensor: worst |err| / limit of the float32 restatement at the base t}} where that exceeds 0.25; t for that tensor = 4 x ratio x base t
WIDER = {}
T = lambda a: np.swapaxes(a, 1, 2)


def tol(case, name):
    base = T_FWD if name in FWD else T_BWD
    r = WIDER.get(case, {}).get(name)
    return base if r is None else 4 * r * base


def ratios(case, got, ref, names=ALL, base=False):
    """{tensor: worst |got - ref| / (t |ref| + t mean|ref|)} at this case's t (base: at the base t, whatever WIDER says)"""
    out = {}
    for n in names:
        r = np.asarray(ref[n], F64)
        t = (T_FWD if n in FWD else T_BWD) if base else tol(case, n)
        err, lim = np.abs(np.asarray(got[n], F64).reshape(r.shape) - r), t * np.abs(r) + t * np.abs(r).mean()
        with np.errstate(divide="ignore", invalid="ignore"):        # a tensor that is exactly zero (del_Q, del_K of a single key) must come back exactly zero
            out[n] = float(np.where(err == 0, 0.0, err / lim).max())
    return out


def normwise(a, b):
    """||a - b|| / ||b||, the plain ||a - b|| where b is exactly zero"""
    nb = float(np.linalg.norm(np.asarray(b, F64).ravel()))
    return float(np.linalg.norm((np.asarray(a, F64) - b).ravel())) / (nb if nb else 1.0)


def inputs(case):
    b, c, s, heads, d = case
    return make_inputs((b, c, s, heads * d))


def f32_heads_block(I, heads, d, dtype=F64, inv_from_width=False, rowdot_over_width=False, del_p_from_next_head=False):
    """include/bla.h's arithmetic in `dtype`; the keyword mutations are the wrong blocks"""
    T_ = dtype
    x, wq, wk, wv, w, bias, dy = (np.asarray(I[n], T_) for n in ("x", "wq", "wk", "wv", "w", "bias", "del_y"))
    B, _, S = x.shape
    D = heads * d
    assert wq.shape[1] == D and w.shape[0] == D
    inv = T_(np.float32(1.0 / np.sqrt(float(D if inv_from_width else d))))
    sl = lambda h: slice(h * d, (h + 1) * d)
    z = T(x)                                                              # [B][S][C]
    o = dict(q=z @ wq, k=z @ wk, v=z @ wv)
    P, A = np.zeros((B, heads, S, S), T_), np.zeros((B, S, D), T_)
    for h in range(heads):
        t = (o["q"][:, :, sl(h)] @ T(o["k"][:, :, sl(h)])) * inv
        e = np.exp(t - t.max(axis=2, keepdims=True))
        P[:, h] = e / e.sum(axis=2, keepdims=True, dtype=T_)
        A[:, :, sl(h)] = P[:, h] @ o["v"][:, :, sl(h)]
    o["weights"], o["attention"] = P, A
    o["out"] = T(A @ w + bias)
    dyt = T(dy)                                                           # del_Y' [B][S][C]
    o["del_w"] = (T(A) @ dyt).sum(axis=0, dtype=T_)
    dp = dyt @ w.T
    if del_p_from_next_head:
        dp = np.concatenate([dp[:, :, sl((h + 1) % heads)] for h in range(heads)], axis=2)
    o["del_p"] = dp
    ds = [dp[:, :, sl(h)] @ T(o["v"][:, :, sl(h)]) for h in range(heads)]
    dots = [(P[:, h].astype(F64) * ds[h]).sum(axis=2, keepdims=True).astype(T_) for h in range(heads)]     # in double, rounded once
    dq, dk, dv = np.zeros((B, S, D), T_), np.zeros((B, S, D), T_), np.zeros((B, S, D), T_)
    for h in range(heads):
        dot = sum(dots) if rowdot_over_width else dots[h]
        di = (P[:, h] * (ds[h] - dot)) * inv
        dv[:, :, sl(h)] = T(P[:, h]) @ dp[:, :, sl(h)]
        dq[:, :, sl(h)] = di @ o["k"][:, :, sl(h)]
        dk[:, :, sl(h)] = T(di) @ o["q"][:, :, sl(h)]
    o["del_q"], o["del_k"], o["del_v"] = dq, dk, dv
    for n, g in (("del_wq", dq), ("del_wk", dk), ("del_wv", dv)):
        o[n] = (x @ g).sum(axis=0, dtype=T_)                              # Z^T = X
    o["del_x"] = (wq @ T(dq) + wk @ T(dk)) + wv @ T(dv)
    assert all(o[n].dtype == T_ for n in ALL)
    return o


@functools.lru_cache(maxsize=None)
def reference(case):
    """(inputs, the float64 composed multi-head block) -- once per process, shared with the device tests; nobody writes into it"""
    _, _, _, heads, d = case
    I = inputs(case)
    per_head = [block(head_inputs(I, h, d), False) for h in range(heads)]
    ref = compose(per_head, I["bias"])
    ref["weights"] = np.stack([p["weights"] for p in per_head], axis=1)
    ref["del_p"] = T(I["del_y"].astype(F64)) @ I["w"].astype(F64).T
    return I, ref


@pytest.mark.parametrize("case", CASES, ids=str)
def test_float64_restatement_is_the_composed_block(case):
    I, ref = reference(case)
    got = f32_heads_block(I, case[3], case[4])
    diff = {n: normwise(got[n], ref[n]) for n in ALL}
    print(case, {n: f"{v:.1e}" for n, v in diff.items()})
    assert all(got[n].shape == ref[n].shape for n in ALL)
    assert max(diff.values()) <= 1e-12, diff


@pytest.mark.parametrize("case", CASES, ids=str)
def test_float32_restatement_leaves_the_device_three_quarters_of_the_limit(case):
    I, ref = reference(case)
    rs = ratios(case, f32_heads_block(I, case[3], case[4], F32), ref, base=True)
    print(case, {n: round(v, 3) for n, v in rs.items()})
    wide = {n: v for n, v in rs.items() if v > 0.25}
    assert set(wide) == set(WIDER.get(case, {})), wide
    assert all(v <= 1.01 * WIDER[case][n] for n, v in wide.items()), wide


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_the_device_tolerance_catches_a_wrong_block(mutation):
    """on (3, 24, 16, 4, 16) and (2, 40, 30, 3, 12), in float64: nothing but the mutation separates the block from its reference"""
    caught = {}
    for case in (CASES[1], CASES[2]):
        I, ref = reference(case)
        rs = ratios(case, f32_heads_block(I, case[3], case[4], **{mutation: True}), ref)
        caught[case] = {n: round(v, 1) for n, v in rs.items() if not v <= 1}
        print(mutation, case, caught[case])
    assert all(caught.values()), caught


# ---- the entries that need no device ---------------------------------------------------------------------------------------------------------------------
def test_applies_over_the_boundary_values(pkg):
    f = pkg.attention_f32_heads_applies
    want = lambda c, s, heads, d: 1 <= s <= 64 and 1 <= d <= 64 and heads >= 1 and heads * d <= 256 and c > 0
    for c in (-8, -1, 0, 1, 7, 256, 1000):
        for s in (-1, 0, 1, 2, 16, 31, 33, 63, 64, 65, 128):
            for heads in (-1, 0, 1, 2, 3, 4, 5, 16, 32, 64, 128, 256, 257, 2 ** 30):
                for d in (-1, 0, 1, 2, 4, 5, 16, 51, 52, 63, 64, 65, 128, 256):
                    assert f(c, s, heads, d) == want(c, s, heads, d), (c, s, heads, d)
    assert f(256, 16, 4, 16) and f(64, 30, 3, 12) and f(7, 33, 2, 5) and f(48, 64, 4, 64) and f(1, 1, 256, 1)
    assert not f(48, 64, 5, 52) and not f(48, 64, 33, 8) and not f(48, 65, 4, 16) and not f(48, 64, 4, 65) and not f(48, 64, 0, 16)      # 260, 264, s, d, no head
    # one head: exactly the formula, nothing of the single-head block's own (any c, s, d > 0) beyond it
    assert all(f(c, s, 1, d) == (1 <= s <= 64 and 1 <= d <= 64 and c > 0) for c in (0, 1, 8) for s in (0, 1, 64, 65, 1024) for d in (0, 1, 64, 65))


def test_entries_refuse_without_touching_the_device(pkg):
    """shape and NULL refusals come back as BLA_ERR_INVALID (1) on a machine with a device and as 'no device' (3) on one without: never a crash"""
    L = pkg.lib()
    ws = pkg.attention_ws()
    for c, s, heads, d in [(64, 65, 4, 16), (64, 0, 4, 16), (64, 16, 4, 65), (64, 16, 4, 0), (64, 16, 33, 8), (64, 16, 0, 16), (64, 16, -2, 16), (0, 16, 4, 16),
                           (64, 16, 4, 16), (64, 16, 1, 16)]:
        assert L.bla_attention_forward_batched_f32_heads(None, 2, None, None, None, None, None, None, C.byref(ws), None, c, s, heads, d) in (1, 3)
        assert L.bla_attention_backward_batched_f32_heads(None, 2, *([None] * 6), C.byref(ws), C.byref(ws), *([None] * 6), c, s, heads, d) in (1, 3)
        assert L.bla_attention_forward_batched_f32_heads(None, 2, *([None] * 8), c, s, heads, d) in (1, 3)
        assert L.bla_attention_backward_batched_f32_heads(None, 0, *([None] * 14), c, s, heads, d) in (1, 3)


if __name__ == "__main__":          # the host measurement the tolerances rest on (no device involved)
    for case_ in CASES:
        I_, ref_ = reference(case_)
        rs_ = ratios(case_, f32_heads_block(I_, case_[3], case_[4], F32), ref_, base=True)
        print(f"{str(case_):22s} worst {max(rs_.values()):.3f}  " + "  ".join(f"{n} {v:.3f}" for n, v in rs_.items()))
