"""The multi-head online bf16 attention block (bla_attention_{forward,backward}_batched_online_bf16_heads) restated in numpy, on the host.

heads_block() is include/bla.h's arithmetic line by line: Q, K, V at the block's width D = heads d; per head h (columns h d .. h d + d - 1) the online
recurrence of tests/test_attention_online_host.py with inv from the HEAD's width and the head's own m, l, Acc, lse and row dot; out, del_P, the weight
gradients and del_X across all D columns.  Both operands of every matrix product are rounded with bla_f32_to_bf16's rounding immediately before the
product (rounded=True) or not at all.

`exact` is the MATERIALISED float64 multi-head block, composed from tests/test_attention_bf16_host.py's block(I_h, False) on each head's slices of the
weights: out = sum_h (out_h - bias) + bias, del_x = sum_h del_x_h, the weight gradients and the per-head tensors side by side.  What this file RECORDS,
per case and tensor of OUTPUTS, is ||rounded - exact|| / ||exact||; tests/test_attention_heads_gpu.py holds the device inside twice that.

Inputs are make_inputs((B, C, S, heads d)): the gains of Wq, Wk, Wv depend on C only, so a head's logits keep the documented spread.

Host-only requirements:
  * the unrounded restatement IS `exact` (1e-12 in every tensor), and the rounded restatement is the same composition of online_block per head (1e-12):
    heads change the addressing and two sums, nothing else;
  * the recorded values are a few unit roundoffs of bf16;
  * seven wrong multi-head blocks are each caught at 4 times the recorded values;
  * the exact forward case (Wq = 0, small integers) has the same bits in float32 and float64."""
import ctypes as C
import functools

import numpy as np
import pytest

from test_attention_bf16_host import rnd, make_inputs, exact_inputs, normwise, OUTPUTS, block
from test_attention_online_host import online_block, KB

# (B, C, S, heads, d)
CASES = [(2, 24, 32, 2, 8),           # one key block, the smallest d
         (1, 64, 96, 4, 16),          # the model's d, D = 64
         (2, 40, 64, 3, 24),          # an odd number of heads, head boundaries off 16 and 32; 3 D = 216: two qkv column groups, a matrix boundary inside a tile
         (1, 32, 128, 8, 32),         # D = 256, the limit: 24 column tiles
         (1, 16, 288, 2, 64),         # ND = 4, S past the materialising entry's limit
         (1, 8, 1024, 4, 16),         # 32 key blocks
         (3, 256, 64, 4, 64)]         # the model's width with 4 heads of 64, batch 3
EXACT = [(s, c, heads, d) for s in (32, 512, 1024) for c, heads, d in ((16, 4, 16), (24, 2, 24), (16, 8, 32))]
MUTATIONS = ["inv_from_width", "out_from_head_0", "del_x_from_head_0", "del_p_from_next_head", "rowdot_over_width", "lse_of_head_0", "interleaved_heads"]
PER_HEAD = ["q", "k", "v", "attention", "del_q", "del_k", "del_v"]       # [B][S][D], a head's columns
T = lambda a: np.swapaxes(a, 1, 2)


def inputs(case):
    b, c, s, heads, d = case
    return make_inputs((b, c, s, heads * d))


def head_inputs(I, h, d):
    sl = slice(h * d, (h + 1) * d)
    return dict(I, wq=I["wq"][:, sl], wk=I["wk"][:, sl], wv=I["wv"][:, sl], w=I["w"][sl])


def compose(per_head, bias):
    """the multi-head block from single-head blocks on the heads' slices"""
    bias = np.asarray(bias, np.float64)[None, :, None]
    o = dict(out=sum(p["out"] - bias for p in per_head) + bias, del_x=sum(p["del_x"] for p in per_head),
             del_w=np.concatenate([p["del_w"] for p in per_head], axis=0))
    for n in ("del_wq", "del_wk", "del_wv"):
        o[n] = np.concatenate([p[n] for p in per_head], axis=1)
    for n in PER_HEAD:
        o[n] = np.concatenate([p[n] for p in per_head], axis=2)
    return o


def heads_block(I, heads, d, rounded=True, dtype=np.float64, backward=True, inv_from_width=False, out_from_head_0=False, del_x_from_head_0=False,
                del_p_from_next_head=False, rowdot_over_width=False, lse_of_head_0=False, interleaved_heads=False):
    """include/bla.h's arithmetic; the keyword mutations are the wrong blocks.  lse and dots come back as [B][heads][S]."""
    T_ = dtype
    r = rnd if rounded else (lambda a: a)
    prod = lambda a, b: np.matmul(r(a), r(b))
    x, wq, wk, wv, w, bias, dy = (np.asarray(I[n], T_) for n in ("x", "wq", "wk", "wv", "w", "bias", "del_y"))
    B, _, S = x.shape
    D = heads * d
    assert wq.shape[1] == D and w.shape[0] == D
    inv = T_(np.float32(1.0 / np.sqrt(float(D if inv_from_width else d))))
    sl = lambda h: slice(h * d, (h + 1) * d)                              # a head's columns of A and del_P, its rows of W
    cols = (lambda h: slice(h, D, heads)) if interleaved_heads else sl    # a head's columns of Q, K, V and their gradients
    z = T(x)                                                              # [B][S][C]
    o = dict(q=prod(z, wq), k=prod(z, wk), v=prod(z, wv))
    A, lse = np.zeros((B, S, D), T_), np.zeros((B, heads, S), T_)
    for h in range(heads):
        q, k, v = (o[n][:, :, cols(h)] for n in "qkv")
        m, l, acc = np.full((B, S, 1), -np.inf, T_), np.zeros((B, S, 1), T_), np.zeros((B, S, d), T_)
        with np.errstate(over="ignore", invalid="ignore"):
            for j in range(0, S, KB):
                t = inv * prod(q, T(k[:, j:j + KB]))
                m2 = np.maximum(m, t.max(axis=2, keepdims=True))
                a = np.exp(m - m2)                                        # the first block: exp(-inf) = 0
                p = np.exp(t - m2)
                l = l * a + p.sum(axis=2, keepdims=True)
                acc = acc * a + prod(p, v[:, j:j + KB])
                m = m2
            A[:, :, sl(h)] = (acc / l).astype(T_)
            lse[:, h] = (m + np.log(l)).astype(T_)[..., 0]
    o["attention"], o["lse"] = A, lse
    o["out"] = T((prod(A[:, :, sl(0)], w[sl(0)]) if out_from_head_0 else prod(A, w)) + bias)
    if not backward:
        return o
    dyt = T(dy)                                                           # del_Y' [B][S][C]
    o["del_w"] = prod(T(A), dyt).sum(axis=0)
    dp = prod(dyt, w.T)
    if del_p_from_next_head:
        dp = np.concatenate([dp[:, :, sl((h + 1) % heads)] for h in range(heads)], axis=2)
    o["del_p"] = dp
    dots = np.zeros((B, heads, S), T_)
    dq, dk, dv = np.zeros((B, S, D), T_), np.zeros((B, S, D), T_), np.zeros((B, S, D), T_)
    for h in range(heads):
        q, k, v = (o[n][:, :, cols(h)] for n in "qkv")
        dph = dp[:, :, sl(h)]
        dots[:, h] = (dp * A).sum(axis=2) if rowdot_over_width else (dph * A[:, :, sl(h)]).sum(axis=2)
        L, dot = lse[:, 0 if lse_of_head_0 else h][..., None], dots[:, h][..., None]
        gq = np.zeros((B, S, d), T_)
        with np.errstate(over="ignore", invalid="ignore"):
            for j in range(0, S, KB):
                kj, vj = k[:, j:j + KB], v[:, j:j + KB]
                p = np.exp(inv * prod(q, T(kj)) - L)
                di = (p * (prod(dph, T(vj)) - dot)) * inv
                dv[:, j:j + KB, cols(h)] = prod(T(p), dph)
                dk[:, j:j + KB, cols(h)] = prod(T(di), q)
                gq = gq + prod(di, kj)
        dq[:, :, cols(h)] = gq
    o["dots"], o["del_q"], o["del_k"], o["del_v"] = dots, dq, dk, dv
    for n, g in (("del_wq", dq), ("del_wk", dk), ("del_wv", dv)):
        o[n] = prod(x, g).sum(axis=0)                                     # Z^T = X
    c0 = sl(0) if del_x_from_head_0 else slice(0, D)
    o["del_x"] = prod(wq[:, c0], T(dq[:, :, c0])) + prod(wk[:, c0], T(dk[:, :, c0])) + prod(wv[:, c0], T(dv[:, :, c0]))
    return o


@functools.lru_cache(maxsize=None)
def recorded(case):
    """(inputs, exact materialised multi-head block, rounded restatement, {tensor: ||rounded - exact|| / ||exact||}) -- once per process;
    tests/test_attention_heads_gpu.py reads it here.  The S x S tensors of `exact` are dropped head by head."""
    _, _, _, heads, d = case
    I = inputs(case)
    exact = compose([block(head_inputs(I, h, d), False) for h in range(heads)], I["bias"])
    rounded = heads_block(I, heads, d, True)
    return I, exact, rounded, {n: normwise(rounded[n], exact[n]) for n in OUTPUTS}


@pytest.mark.parametrize("case", CASES, ids=str)
def test_unrounded_restatement_is_the_composed_materialised_block(case):
    I, exact, _, _ = recorded(case)
    got = heads_block(I, case[3], case[4], False)
    diff = {n: normwise(got[n], exact[n]) for n in OUTPUTS + PER_HEAD}
    print(case, {n: f"{v:.1e}" for n, v in diff.items()})
    assert max(diff.values()) <= 1e-12, diff


@pytest.mark.parametrize("case", CASES, ids=str)
def test_rounded_restatement_is_the_composed_online_block(case):
    """a head of the multi-head block is the single-head online block on the head's slices; out and del_x are its sums over the heads"""
    _, _, _, heads, d = case
    I, _, rounded, _ = recorded(case)
    per_head = [online_block(head_inputs(I, h, d), True) for h in range(heads)]
    want = compose(per_head, I["bias"])
    diff = {n: normwise(rounded[n], want[n]) for n in OUTPUTS + PER_HEAD}
    for n in ("lse", "dots"):
        diff[n] = normwise(rounded[n], np.stack([p[n][..., 0] for p in per_head], axis=1))
    diff["del_p"] = normwise(rounded["del_p"], np.concatenate([p["del_p"] for p in per_head], axis=2))
    print(case, {n: f"{v:.1e}" for n, v in diff.items()})
    assert max(diff.values()) <= 1e-12, diff


@pytest.mark.parametrize("case", CASES, ids=str)
def test_rounding_differences_are_recorded(case):
    _, _, rounded, diff = recorded(case)
    print(f"{case}: lse {rounded['lse'].min():.1f} .. {rounded['lse'].max():.1f}; " + ", ".join(f"{n} {v:.2e}" for n, v in diff.items()))
    assert all(2.0 ** -12 < v < 2.0 ** -4 for v in diff.values()), diff


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_four_times_the_recorded_value_catches_a_wrong_block(mutation):
    """on (1, 64, 96, 4, 16) and (2, 40, 64, 3, 24)"""
    caught = {}
    for case in (CASES[1], CASES[2]):
        I, exact, _, diff = recorded(case)
        wrong = heads_block(I, case[3], case[4], True, **{mutation: True})
        beyond = {n: normwise(wrong[n], exact[n]) / diff[n] for n in OUTPUTS if not np.isfinite(wrong[n]).all() or normwise(wrong[n], exact[n]) > 4 * diff[n]}
        print(mutation, case, {n: round(float(v), 1) for n, v in beyond.items()})
        caught[case] = beyond
    assert all(caught.values()), caught


@pytest.mark.parametrize("shape", EXACT, ids=str)
def test_exact_forward_case_is_the_same_in_float32_and_float64(shape):
    s, c, heads, d = shape
    I = exact_inputs(s, c, heads * d)
    o32, o64 = heads_block(I, heads, d, True, np.float32, backward=False), heads_block(I, heads, d, True, np.float64, backward=False)
    for n in ("q", "k", "v", "attention", "out"):
        a = o64[n]
        assert np.array_equal(a * 65536, np.round(a * 65536)) and np.abs(a).max() < 128, (n, np.abs(a).max())     # multiples of 2^-16 below 2^7
        assert o32[n].dtype == np.float32 and np.array_equal(o32[n].astype(np.float64), a), n
    assert not np.any(o64["q"]) and np.abs(o64["lse"] - np.log(s)).max() < 1e-12
    assert len(np.unique(o64["attention"])) > 8 and len(np.unique(o64["out"])) > 8        # not a trivial tensor


# ---- the entries that need no device ---------------------------------------------------------------------------------------------------------------------
def test_applies_over_the_boundary_values(pkg):
    f = pkg.attention_online_bf16_heads_applies
    want = lambda c, s, heads, d: (s % 32 == 0 and 32 <= s <= 4096 and d % 8 == 0 and 8 <= d <= 64 and heads >= 1 and heads * d <= 256 and c % 8 == 0
                                   and c > 0)
    for c in (-8, 0, 4, 8, 12, 256, 264):
        for s in (-32, 0, 16, 31, 32, 33, 288, 4096, 4097, 4128):
            for heads in (-1, 0, 1, 2, 3, 4, 5, 8, 11, 16, 32, 33, 2 ** 30):
                for d in (-8, 0, 4, 8, 12, 16, 24, 32, 56, 64, 68, 72, 128):
                    assert f(c, s, heads, d) == want(c, s, heads, d), (c, s, heads, d)
    assert f(256, 1024, 4, 64) and f(256, 1024, 32, 8) and f(256, 1024, 8, 32) and f(256, 1024, 4, 16)
    assert not f(256, 1024, 33, 8) and not f(256, 1024, 11, 24) and not f(256, 1024, 5, 56) and not f(256, 1024, 0, 16)       # 264, 264, 280, no head
    assert all(f(c, s, 1, d) == pkg.attention_online_bf16_applies(c, s, d) for c in (8, 12) for s in (32, 48, 4096, 4128) for d in (4, 8, 64, 72))


def test_entries_refuse_without_touching_the_device(pkg):
    """shape and NULL refusals come back as BLA_ERR_INVALID (1) on a machine with a device and as 'no device' (3) on one without: never a crash"""
    L = pkg.lib()
    ws = pkg.attention_ws()
    for c, s, heads, d in [(64, 16, 4, 16), (64, 4128, 4, 16), (64, 64, 4, 4), (64, 64, 1, 72), (12, 64, 4, 16), (64, 64, 0, 16), (64, 64, 33, 8), (64, 64, -2, 16),
                           (64, 64, 4, 16)]:
        assert L.bla_attention_forward_batched_online_bf16_heads(None, 2, None, None, None, None, None, None, C.byref(ws), None, c, s, heads, d) in (1, 3)
        assert L.bla_attention_backward_batched_online_bf16_heads(None, 2, *([None] * 6), C.byref(ws), C.byref(ws), *([None] * 6), c, s, heads, d) in (1, 3)
        assert L.bla_attention_forward_batched_online_bf16_heads(None, 2, *([None] * 8), c, s, heads, d) in (1, 3)
        assert L.bla_attention_backward_batched_online_bf16_heads(None, 0, *([None] * 14), c, s, heads, d) in (1, 3)
