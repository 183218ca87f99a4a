"""The online-softmax attention block in fp32 (bla_attention_{forward,backward}_batched_online_f32) restated in numpy, on the host.

online_f32_block() is include/bla.h's arithmetic line by line in a chosen dtype: Q, K, V at the block's width D = heads d; per head the recurrence over blocks
of 32 keys in ascending order (m, l, Acc, the rescale a = exp(m - m'), inv from the HEAD's width), A = Acc / l, lse = m + log l; backwards del_P, the row dot
<del_P, A> over the head's d columns, and per key block P_j = exp(T_j - lse), del_S_j, del_I_j, del_V_j, del_K_j, del_Q += del_I_j K_j; out, del_W, the weight
gradients and del_X across all D columns.  A ragged last block is simply shorter here (the device pads it to 32 and masks: the `tail_unmasked` mutation is that
padding without the mask).

The float64 reference is the MATERIALISED composed multi-head block of tests/test_attention_f32_heads_host.py (block / compose / head_inputs on make_inputs), with
lse = the float64 log-sum-exp of the reference's own q and k, and dots = <del_P, A> in float64.  tests/test_attention_online_f32_gpu.py reads cases, inputs,
reference and tolerance here.

Tolerance: the project's form and numbers for fp32 attention, |got - ref| <= t |ref| + t mean|ref| per tensor, t = 2e-5 for q, k, v, attention, lse, out and
5e-5 for the gradients, del_p, del_q / k / v and the dots.  Measured here (`python tests/test_attention_online_f32_host.py` prints every ratio): the float32
restatement's worst tensor per case is 0.02 .. 0.07 of the limit (del_k), lse <= 0.012, dots <= 0.016; nothing widens.

The one-key case (S = 1): P = 1, so del_S = <del_P, v> = dot in exact arithmetic and del_q, del_k, del_wq, del_wk are EXACTLY zero in the reference, where the
form above would demand exact zeros.  The online identity leaves a rounding residue instead: del_S and the dot are two fp32 sums of the same d products, each
within d u sum_dd |del_P v| of the exact sum (u = 2^-24), so |del_S - dot| <= 2 d u sum_dd |del_P[dd] v[dd]| =: E per (image, head).  Carried through:
  |del_I| <= E inv;  |del_q[dd]| <= E inv |k[dd]|;  |del_k[dd]| <= E inv |q[dd]|;  |del_wq[c][col]| <= sum_b |x[b][c]| |del_q[b][col]|, del_wk likewise,
each times (1 + 1e-3) for the roundings of the two or three products behind it (second order in u).  one_key_bounds() writes that out; those four tensors of
that case are held to it, every other tensor of the case to the form above.

Host-only requirements:
  * the float64 restatement IS the materialised reference (1e-12 normwise in every tensor, lse and dots included);
  * the float32 restatement stays within 0.25 of the limit, and inside the derived bound on the one-key case's four zero tensors;
  * seven wrong blocks -- no rescale of Acc, no rescale of l, lse without log l, the row dot over all D, inv from D, the tail keys not masked, the backward key
    blocks at the wrong offset -- each leave the device tolerance, in float64;
  * bla_attention_online_f32_applies over its boundary values; the entries refuse bad shapes and NULLs without touching a device; bla_unet_set_attention(NULL, 4)
    reports the null; the C program accepts BLA_UNET_ATTENTION=online-f32 and still refuses `bogus`."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import conftest  # noqa: F401  (as a script too: the search path of the input generators)
import test_attention_f32_heads_host as heads_host          # the materialised composed reference: block, compose, head_inputs on make_inputs

F32, F64 = np.float32, np.float64
KB = 32                                   # BLA_ATTENTION_ONLINE_KEYS
# (B, C, S, heads, d)
CASES = [(2, 8, 1, 2, 4),                 # one key
         (1, 7, 33, 2, 5),                # everything odd; the second key block holds one key
         (2, 40, 95, 3, 12),              # three blocks, a ragged tail, odd heads
         (2, 24, 64, 2, 17),              # d across 16
         (1, 16, 160, 4, 64),             # D = 256, d = 64, five blocks
         (9, 16, 65, 1, 8),               # batch past eight, one head
         (1, 8, 400, 2, 16)]              # the 40 x 40 model's S
ONE_KEY = CASES[0]
T_FWD, T_BWD = 2e-5, 5e-5
FWD = ["q", "k", "v", "attention", "lse", "out"]
GRADS = ["del_wq", "del_wk", "del_wv", "del_w", "del_x"]
WORK = ["del_p", "del_q", "del_k", "del_v", "dots"]        # the gradient workspace: attention (= del_P), q, k, v, scores_raw (= the row dots)
ALL = FWD + GRADS + WORK
ZERO_AT_ONE_KEY = ["del_q", "del_k", "del_wq", "del_wk"]
MUTATIONS = ["acc_not_rescaled", "l_not_rescaled", "lse_without_log_l", "rowdot_over_width", "inv_from_width", "tail_unmasked", "bwd_blocks_shifted"]
T = lambda a: np.swapaxes(a, 1, 2)


def ratios(got, ref, names=ALL):
    """{tensor: worst |got - ref| / (t |ref| + t mean|ref|)}"""
    out = {}
    for n in names:
        r = np.asarray(ref[n], F64)
        t = T_FWD if n in FWD else T_BWD
        err, lim = np.abs(np.asarray(got[n], F64).reshape(r.shape) - r), t * np.abs(r) + t * np.abs(r).mean()
        with np.errstate(divide="ignore", invalid="ignore"):
            out[n] = float(np.where(err == 0, 0.0, err / lim).max())
    return out


def normwise(a, b):
    nb = float(np.linalg.norm(np.asarray(b, F64).ravel()))
    return float(np.linalg.norm((np.asarray(a, F64) - b).ravel())) / (nb if nb else 1.0)


def inputs(case):
    return heads_host.inputs(case)


def online_f32_block(I, heads, d, dtype=F64, acc_not_rescaled=False, l_not_rescaled=False, lse_without_log_l=False, rowdot_over_width=False, inv_from_width=False,
                     tail_unmasked=False, bwd_blocks_shifted=False):
    """include/bla.h's arithmetic in `dtype`; the keyword mutations are the wrong blocks.  lse and dots come back as [B][heads][S]."""
    T_ = dtype
    x, wq, wk, wv, w, bias, dy = (np.asarray(I[n], T_) for n in ("x", "wq", "wk", "wv", "w", "bias", "del_y"))
    B, _, S = x.shape
    D = heads * d
    assert wq.shape[1] == D and w.shape[0] == D
    inv = T_(np.float32(1.0 / np.sqrt(float(D if inv_from_width else d))))
    sl = lambda h: slice(h * d, (h + 1) * d)
    z = T(x)                                                              # [B][S][C]
    o = dict(q=z @ wq, k=z @ wk, v=z @ wv)
    pad = (-S) % KB if tail_unmasked else 0                               # the wrong block: the last key block padded with zero rows that count as keys
    padded = lambda a: np.concatenate([a, np.zeros((B, pad, a.shape[2]), T_)], axis=1)
    A, lse = np.zeros((B, S, D), T_), np.zeros((B, heads, S), T_)
    for h in range(heads):
        q, k, v = o["q"][:, :, sl(h)], padded(o["k"][:, :, sl(h)]), padded(o["v"][:, :, sl(h)])
        m, l, acc = np.full((B, S, 1), -np.inf, T_), np.zeros((B, S, 1), T_), np.zeros((B, S, d), T_)
        for j in range(0, S, KB):
            t = (q @ T(k[:, j:j + KB])) * inv
            m2 = np.maximum(m, t.max(axis=2, keepdims=True))
            a = np.exp(m - m2)                                            # the first block: exp(-inf) = 0
            p = np.exp(t - m2)
            l = l * (1 if l_not_rescaled else a) + p.sum(axis=2, keepdims=True, dtype=T_)
            acc = acc * (1 if acc_not_rescaled else a) + p @ v[:, j:j + KB]
            m = m2
        A[:, :, sl(h)] = acc / l
        lse[:, h] = (m if lse_without_log_l else m + np.log(l))[:, :, 0]
    o["attention"], o["lse"] = A, lse
    o["out"] = T(A @ w + bias)
    dyt = T(dy)                                                           # del_Y' [B][S][C]
    o["del_w"] = (T(A) @ dyt).sum(axis=0, dtype=T_)
    o["del_p"] = dp = dyt @ w.T
    dots = np.stack([(dp[:, :, sl(h)] * A[:, :, sl(h)]).sum(axis=2, dtype=T_) for h in range(heads)], axis=1)
    if rowdot_over_width:
        dots = np.repeat(dots.sum(axis=1, keepdims=True, dtype=T_), heads, axis=1)
    o["dots"] = dots
    dq, dk, dv = np.zeros((B, S, D), T_), np.zeros((B, S, D), T_), np.zeros((B, S, D), T_)
    for h in range(heads):
        q, k, v, g = o["q"][:, :, sl(h)], o["k"][:, :, sl(h)], o["v"][:, :, sl(h)], dp[:, :, sl(h)]
        L, dot = lse[:, h][:, :, None], dots[:, h][:, :, None]
        for j in range(0, S, KB):
            jp = (j + KB) % (KB * ((S + KB - 1) // KB)) if bwd_blocks_shifted else j      # the wrong block: P from the NEXT key block's K
            kj = k[:, jp:jp + KB][:, :k[:, j:j + KB].shape[1]]
            if kj.shape[1] < k[:, j:j + KB].shape[1]:
                kj = np.concatenate([kj, np.zeros((B, k[:, j:j + KB].shape[1] - kj.shape[1], d), T_)], axis=1)
            with np.errstate(over="ignore"):
                p = np.exp((q @ T(kj)) * inv - L)
            ds = g @ T(v[:, j:j + KB])
            di = (p * (ds - dot)) * inv
            dv[:, j:j + KB, sl(h)] = T(p) @ g
            dk[:, j:j + KB, sl(h)] = T(di) @ q
            dq[:, :, sl(h)] += di @ k[:, j:j + KB]
    o["del_q"], o["del_k"], o["del_v"] = dq, dk, dv
    for n, g in (("del_wq", dq), ("del_wk", dk), ("del_wv", dv)):
        o[n] = (x @ g).sum(axis=0, dtype=T_)                              # Z^T = X
    o["del_x"] = (wq @ T(dq) + wk @ T(dk)) + wv @ T(dv)
    assert all(o[n].dtype == T_ for n in ALL), {n: o[n].dtype for n in ALL}
    return o


@functools.lru_cache(maxsize=None)
def reference(case):
    """(inputs, the float64 materialised multi-head block + lse + dots) -- once per process, shared with the device tests; nobody writes into it"""
    _, _, _, heads, d = case
    I, ref = heads_host.reference(case)
    ref = dict(ref)
    inv = F64(np.float32(1.0 / np.sqrt(float(d))))
    lse, dots = [], []
    for h in range(heads):
        sl = slice(h * d, (h + 1) * d)
        t = (ref["q"][:, :, sl] @ T(ref["k"][:, :, sl])) * inv
        mx = t.max(axis=2, keepdims=True)
        lse.append((mx + np.log(np.exp(t - mx).sum(axis=2, keepdims=True)))[:, :, 0])
        dots.append((ref["del_p"][:, :, sl] * ref["attention"][:, :, sl]).sum(axis=2))
    ref["lse"], ref["dots"] = np.stack(lse, axis=1), np.stack(dots, axis=1)
    return I, ref


def one_key_bounds(case=ONE_KEY):
    """the derived absolute bounds of the four tensors that are exactly zero at S = 1 (module docstring), from the float64 reference"""
    b, c, s, heads, d = case
    assert s == 1
    I, ref = reference(case)
    u, slack = 2.0 ** -24, 1 + 1e-3
    inv = F64(np.float32(1.0 / np.sqrt(float(d))))
    bq, bk = np.zeros((b, 1, heads * d)), np.zeros((b, 1, heads * d))
    for h in range(heads):
        sl = slice(h * d, (h + 1) * d)
        E = 2 * d * u * np.abs(ref["del_p"][:, :, sl] * ref["v"][:, :, sl]).sum(axis=2, keepdims=True)     # |del_S - dot| per (image, head)
        bq[:, :, sl] = E * inv * np.abs(ref["k"][:, :, sl]) * slack
        bk[:, :, sl] = E * inv * np.abs(ref["q"][:, :, sl]) * slack
    ax = np.abs(np.asarray(I["x"], F64))                                                                      # [B][C][1]
    return dict(del_q=bq, del_k=bk, del_wq=(ax @ bq).sum(axis=0) * slack, del_wk=(ax @ bk).sum(axis=0) * slack)


def check_names(case):
    """the tensors held to the relative form (the one-key case's four zero tensors are held to one_key_bounds instead)"""
    return [n for n in ALL if not (case == ONE_KEY and n in ZERO_AT_ONE_KEY)]


def inside_one_key_bounds(got):
    bounds = one_key_bounds()
    return {n: float((np.abs(np.asarray(got[n], F64).reshape(bounds[n].shape)) / bounds[n]).max()) for n in ZERO_AT_ONE_KEY}


@pytest.mark.parametrize("case", CASES, ids=str)
def test_float64_restatement_is_the_materialised_block(case):
    I, ref = reference(case)
    got = online_f32_block(I, case[3], case[4])
    diff = {n: normwise(got[n], ref[n]) for n in ALL}
    print(case, {n: f"{v:.1e}" for n, v in diff.items()})
    assert all(got[n].shape == ref[n].shape for n in ALL)
    assert max(diff.values()) <= 1e-12, diff


@pytest.mark.parametrize("case", CASES, ids=str)
def test_float32_restatement_leaves_the_device_three_quarters_of_the_limit(case):
    I, ref = reference(case)
    got = online_f32_block(I, case[3], case[4], F32)
    rs = ratios(got, ref, check_names(case))
    print(case, {n: round(v, 3) for n, v in rs.items()})
    assert max(rs.values()) <= 0.25, rs
    if case == ONE_KEY:
        assert all(not np.asarray(ref[n]).any() for n in ZERO_AT_ONE_KEY)          # exactly zero in the reference
        inside = inside_one_key_bounds(got)
        print(case, "residue / derived bound", {n: round(v, 3) for n, v in inside.items()}, {n: float(np.abs(got[n]).max()) for n in ZERO_AT_ONE_KEY})
        assert max(inside.values()) <= 1, inside


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_the_device_tolerance_catches_a_wrong_block(mutation):
    """on (1, 7, 33, 2, 5) and (2, 40, 95, 3, 12), in float64: nothing but the mutation separates the block from its reference.  Every wrong block must be caught
    at S = 95 (three key blocks); at S = 33 the second block is ONE key, which raises no row's maximum with these inputs, so the two missing rescales multiply
    by a = 1 there and are invisible by construction -- every other wrong block must be caught there too, the unmasked tail first of all."""
    caught = {}
    for case in (CASES[1], CASES[2]):
        I, ref = reference(case)
        rs = ratios(online_f32_block(I, case[3], case[4], **{mutation: True}), ref)
        caught[case] = {n: round(v, 1) for n, v in rs.items() if not v <= 1}
        print(mutation, case, caught[case])
    assert caught[CASES[2]], caught
    assert caught[CASES[1]] or mutation in ("acc_not_rescaled", "l_not_rescaled"), caught


# ---- the entries that need no device ---------------------------------------------------------------------------------------------------------------------
def test_applies_over_the_boundary_values(pkg):
    f = pkg.attention_online_f32_applies
    want = lambda c, s, heads, d: 1 <= s <= 4096 and 1 <= d <= 64 and heads >= 1 and heads * d <= 256 and c > 0
    for c in (-8, -1, 0, 1, 7, 256, 1000):
        for s in (-1, 0, 1, 2, 31, 32, 33, 64, 65, 324, 400, 4095, 4096, 4097, 2 ** 20):
            for heads in (-1, 0, 1, 2, 3, 4, 5, 16, 32, 64, 128, 256, 257, 2 ** 30):
                for d in (-1, 0, 1, 2, 4, 5, 16, 17, 51, 52, 63, 64, 65, 128, 256):
                    assert f(c, s, heads, d) == want(c, s, heads, d), (c, s, heads, d)
    assert f(256, 1024, 4, 16) and f(7, 33, 2, 5) and f(16, 160, 4, 64) and f(1, 1, 256, 1) and f(8, 400, 2, 16) and f(3, 4096, 1, 64)
    assert not f(48, 64, 5, 52) and not f(48, 64, 33, 8) and not f(48, 4097, 4, 16) and not f(48, 64, 4, 65) and not f(48, 64, 0, 16) and not f(0, 64, 1, 16)


def test_entries_refuse_without_touching_the_device(pkg):
    """shape and NULL refusals come back as BLA_ERR_INVALID (1) on a machine with a device and as 'no device' (3) on one without: never a crash"""
    L = pkg.lib()
    ws = pkg.attention_ws()
    for c, s, heads, d in [(64, 4097, 4, 16), (64, 0, 4, 16), (64, 16, 4, 65), (64, 16, 4, 0), (64, 16, 33, 8), (64, 16, 0, 16), (64, 16, -2, 16), (0, 16, 4, 16),
                           (64, 400, 4, 16), (64, 16, 1, 16)]:
        assert L.bla_attention_forward_batched_online_f32(None, 2, None, None, None, None, None, None, C.byref(ws), None, c, s, heads, d) in (1, 3)
        assert L.bla_attention_backward_batched_online_f32(None, 2, *([None] * 6), C.byref(ws), C.byref(ws), *([None] * 6), c, s, heads, d) in (1, 3)
        assert L.bla_attention_forward_batched_online_f32(None, 2, *([None] * 8), c, s, heads, d) in (1, 3)
        assert L.bla_attention_backward_batched_online_f32(None, 0, *([None] * 14), c, s, heads, d) in (1, 3)


def test_set_attention_null_reports_the_null_not_the_mode(pkg):
    L = pkg.lib()
    assert pkg.UNET_ATTENTION_F32_ONLINE == 4
    assert L.bla_unet_set_attention(None, 4) == 1 and "null" in L.bla_last_error().decode()
    for mode in (2, -1, 7):
        assert L.bla_unet_set_attention(None, mode) == 1 and "mode" in L.bla_last_error().decode()
    assert L.bla_unet_device_bytes(None) == 0


def test_c_program_reads_online_f32(pkg, tmp_path):
    """BLA_UNET_ATTENTION is checked in main before any sub-command opens the device: `online-f32` passes it (the unknown command is what stops the program),
    `bogus` is still refused with a message that names the variable and the online values"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg.build_native()
    subprocess.run(["make", "-s", "-C", os.path.join(root, "examples"), "cifar_unet_gpu"], check=True, timeout=600)
    prog = os.path.join(root, "examples", "cifar_unet_gpu")

    def run(value):
        r = subprocess.run([prog, "no-such-command"], cwd=str(tmp_path), env=dict(os.environ, BLA_UNET_ATTENTION=value), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, timeout=60)
        return r.returncode, r.stdout + r.stderr
    code, text = run("online-f32")
    assert code != 0 and "Unrecognized argument" in text and "BLA_UNET_ATTENTION" not in text, (code, text)
    code, text = run("bogus")
    assert code != 0 and "BLA_UNET_ATTENTION" in text and "online" in text and "online-f32" in text and "Unrecognized" not in text, (code, text)


if __name__ == "__main__":          # the host measurement the tolerances rest on (no device involved)
    for case_ in CASES + [(1, 8, 1024, 1, 16)]:
        I_, ref_ = reference(case_)
        d64 = max(normwise(v, ref_[n]) for n, v in online_f32_block(I_, case_[3], case_[4]).items() if n in ALL)
        got_ = online_f32_block(I_, case_[3], case_[4], F32)
        rs_ = ratios(got_, ref_, check_names(case_))
        print(f"{str(case_):22s} float64 {d64:.1e}  float32 worst {max(rs_.values()):.3f}  " + "  ".join(f"{n} {v:.3f}" for n, v in rs_.items()))
        if case_ == ONE_KEY:
            print("   one key: residue / derived bound", {n: round(v, 3) for n, v in inside_one_key_bounds(got_).items()})
