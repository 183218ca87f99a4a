"""The online-softmax bf16 attention block (bla_attention_{forward,backward}_batched_online_bf16) restated in numpy, on the host.

online_block() is include/bla.h's arithmetic line by line: key blocks of KB keys in ascending order, a running maximum m, a running sum l and the
unnormalised accumulator Acc; both operands of every matrix product rounded with bla_f32_to_bf16's rounding immediately before the product
(rounded=True) or not at all; everything else in the working precision.  The backward pass recomputes P_j = exp(T_j - lse) and uses the row dots
<del_P, A> where the materialised block uses <P, del_S>.

What this file RECORDS, per case and tensor, is ||rounded online block - exact|| / ||exact||, where `exact` is the MATERIALISED float64 block of
tests/test_attention_bf16_host.py (block(I, False)): the online block is held to the block it replaces, not to itself.
tests/test_attention_online_gpu.py holds the device inside twice the recorded values.

Host-only requirements:
  * the unrounded online block IS the materialised block (1e-12 in every tensor): the online recurrence and the row-dot identity are exact;
  * the recorded values are a few unit roundoffs of bf16 in every ordinary case and on the ramp (x's pixel columns scaled by 0.25 .. 2 along S, so
    that the running maximum keeps moving);
  * they are a property of the arithmetic, not of one draw of the roundings (a relative 2^-23 perturbation of every product moves none by more than
    half of itself), and fp32 in place of float64 for everything that is not a product stays within 1.25 times them -- the large-logit input
    (logits beyond +-60, lse up to about 137) included;
  * seven wrong blocks are each caught at 4 times the recorded values;
  * the exact forward case (Wq = 0, small integers) has the same bits in float32 and float64."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from test_attention_bf16_host import rnd, make_inputs, exact_inputs, normwise, OUTPUTS, block, EX

KB = 32                               # BLA_ATTENTION_ONLINE_KEYS
# (B, C, S, d)
CASES = [(2, 24, 32, 8),              # one key block
         (3, 64, 96, 16),
         (1, 16, 288, 16),            # the first S the materialising bf16 entry refuses
         (2, 40, 320, 24),            # d off 16
         (1, 8, 1024, 64),            # the largest d
         (1, 256, 1024, 16),          # the model's shape on 64 x 64 images
         (1, 16, 4096, 8)]            # the limit (the float64 S x S tensors of `exact`: about 1 GB for seconds; one image)
RAMP, LARGE = "ramp", "large-logit"   # two more inputs, named: a variant of (2, 40, 320, 24) and make_inputs((2, 64, 320, 16), logit_gain=40)
ORDINARY = CASES + [RAMP]
ALL = ORDINARY + [LARGE]
MUTATIONS = ["no_acc_rescale", "no_l_rescale", "lse_without_log", "drop_rowdot", "drop_inv", "untransposed_dk", "wrong_key_offset"]


def shape_of(case):
    return {RAMP: (2, 40, 320, 24), LARGE: (2, 64, 320, 16)}.get(case, case)


def inputs(case):
    if case == LARGE:
        return make_inputs(shape_of(case), logit_gain=40.0)
    I = make_inputs(shape_of(case))
    if case == RAMP:
        I = dict(I, x=(I["x"] * np.linspace(0.25, 2, shape_of(case)[2]).astype(np.float32)).astype(np.float32))
    return I


def online_block(I, rounded=True, dtype=np.float64, KB=KB, backward=True, eps_seed=None, no_acc_rescale=False, no_l_rescale=False, lse_without_log=False,
                 drop_rowdot=False, drop_inv=False, untransposed_dk=False, wrong_key_offset=False):
    """include/bla.h's arithmetic; the keyword mutations are the wrong blocks; eps_seed: the 2^-23 perturbation of every product."""
    T_ = dtype
    r = rnd if rounded else (lambda a: a)
    rng = np.random.default_rng(eps_seed) if eps_seed is not None else None

    def prod(a, b):
        p = np.matmul(r(a), r(b))
        return p if rng is None else p * (1 + 2.0 ** -23 * rng.choice([-1.0, 1.0], p.shape))
    x, wq, wk, wv, w, bias, dy = (np.asarray(I[n], T_) for n in ("x", "wq", "wk", "wv", "w", "bias", "del_y"))
    B, _, S = x.shape
    d = wq.shape[1]
    inv = T_(np.float32(1.0 / np.sqrt(float(d))))
    T = lambda a: np.swapaxes(a, 1, 2)
    z = T(x)                                                      # [B][S][C]
    o = dict(q=prod(z, wq), k=prod(z, wk), v=prod(z, wv))
    q, k, v = o["q"], o["k"], o["v"]
    m, l, acc = np.full((B, S, 1), -np.inf, T_), np.zeros((B, S, 1), T_), np.zeros((B, S, d), T_)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(0, S, KB):
            t = inv * prod(q, T(k[:, j:j + KB]))
            m2 = np.maximum(m, t.max(axis=2, keepdims=True))
            a = np.exp(m - m2)                                    # the first block: exp(-inf) = 0
            p = np.exp(t - m2)
            l = l * (1 if no_l_rescale else a) + p.sum(axis=2, keepdims=True)
            acc = acc * (1 if no_acc_rescale else a) + prod(p, v[:, j:j + KB])
            m = m2
        o["attention"] = A = (acc / l).astype(T_)
        o["lse"] = lse = (m + (0 if lse_without_log else np.log(l))).astype(T_)
    o["out"] = T(prod(A, w) + bias)
    if not backward:
        return o
    dyt = T(dy)                                                   # del_Y' [B][S][C]
    o["del_w"] = prod(T(A), dyt).sum(axis=0)
    o["del_p"] = dp = prod(dyt, w.T)
    o["dots"] = dot = 0 * lse if drop_rowdot else (dp * A).sum(axis=2, keepdims=True)
    dq, dk, dv = np.zeros((B, S, d), T_), np.zeros((B, S, d), T_), np.zeros((B, S, d), T_)
    tiles = []
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(0, S, KB):
            jj = (j + KB) % S if wrong_key_offset else j
            kj, vj = k[:, jj:jj + KB], v[:, jj:jj + KB]
            p = np.exp(inv * prod(q, T(kj)) - lse)
            ds = prod(dp, T(vj))
            di = (p * (ds - dot)) * (1 if drop_inv else inv)
            dv[:, j:j + KB] = prod(T(p), dp)
            dk[:, j:j + KB] = prod(T(di), q)
            dq = dq + prod(di, kj)
            tiles.append(di)
    if untransposed_dk:                                           # del_I where del_I^T is meant (the tiles side by side are del_I)
        dk = prod(np.concatenate(tiles, axis=2), q)
    o["del_q"], o["del_k"], o["del_v"] = dq, dk, dv
    for n, g in (("del_wq", dq), ("del_wk", dk), ("del_wv", dv)):
        o[n] = prod(x, g).sum(axis=0)                             # Z^T = X
    o["del_x"] = prod(wq, T(dq)) + prod(wk, T(dk)) + prod(wv, T(dv))
    return o


@functools.lru_cache(maxsize=None)
def recorded(case):
    """(inputs, exact materialised block, rounded online block, {tensor: ||rounded - exact|| / ||exact||}) -- once per process;
    tests/test_attention_online_gpu.py reads it here.  The S x S tensors of `exact` are dropped at once."""
    I = inputs(case)
    exact = block(I, False)
    del exact["weights"]
    rounded = online_block(I, True)
    return I, exact, rounded, {n: normwise(rounded[n], exact[n]) for n in OUTPUTS}


@pytest.mark.parametrize("case", ALL, ids=str)
def test_unrounded_online_block_is_the_materialised_block(case):
    I, exact, _, _ = recorded(case)
    got = online_block(I, False)
    diff = {n: normwise(got[n], exact[n]) for n in OUTPUTS + ["q", "k", "v", "attention", "del_q", "del_k", "del_v"]}
    print(case, {n: f"{v:.1e}" for n, v in diff.items()})
    assert max(diff.values()) <= 1e-12, diff


@pytest.mark.parametrize("case", ORDINARY, ids=str)
def test_rounding_differences_are_recorded(case):
    _, _, rounded, diff = recorded(case)
    print(f"{case}: lse {rounded['lse'].min():.1f} .. {rounded['lse'].max():.1f}; " + ", ".join(f"{n} {v:.2e}" for n, v in diff.items()))
    assert all(2.0 ** -12 < v < 2.0 ** -4 for v in diff.values()), diff


def test_the_large_logit_input_has_large_logits():
    I, exact, rounded, diff = recorded(LARGE)
    t = exact["q"] @ np.swapaxes(exact["k"], 1, 2) / 4
    print(f"logits {t.min():.1f} .. {t.max():.1f}, lse up to {rounded['lse'].max():.1f}; " + ", ".join(f"{n} {v:.2e}" for n, v in diff.items()))
    assert t.max() > 60 and t.min() < -60 and rounded["lse"].max() > 100
    assert all(np.isfinite(rounded[n]).all() for n in rounded)


@pytest.mark.parametrize("case", ORDINARY, ids=str)
def test_recorded_values_do_not_depend_on_the_draw(case):
    I, _, rounded, diff = recorded(case)
    other = online_block(I, True, eps_seed=0)
    moved = {n: normwise(other[n], rounded[n]) / diff[n] for n in OUTPUTS}
    print(case, {n: round(v, 3) for n, v in moved.items()})
    assert max(moved.values()) <= 0.5, moved


@pytest.mark.parametrize("case", ALL, ids=str)
def test_float32_restatement_stays_at_the_recorded_values(case):
    I, exact, _, diff = recorded(case)
    got = online_block(I, True, np.float32)
    ratio = {n: normwise(got[n], exact[n]) / diff[n] for n in OUTPUTS}
    print(case, {n: round(v, 4) for n, v in ratio.items()})
    assert all(got[n].dtype == np.float32 and np.isfinite(got[n]).all() for n in OUTPUTS)
    assert max(ratio.values()) <= 1.25, ratio


def test_another_block_size_is_the_same_arithmetic_up_to_its_roundings():
    """KB = 64 instead of 32 moves the tensors by a fraction of the recorded value: what is recorded does not hinge on the block size"""
    case = CASES[3]
    I, _, rounded, diff = recorded(case)
    other = online_block(I, True, KB=64)
    moved = {n: normwise(other[n], rounded[n]) / diff[n] for n in OUTPUTS}
    print(case, {n: round(v, 3) for n, v in moved.items()})
    assert max(moved.values()) <= 0.5, moved


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_four_times_the_recorded_value_catches_a_wrong_block(mutation):
    """on the ramp, where the running maximum moves in most blocks, and on (3, 64, 96, 16)"""
    caught = {}
    for case in (RAMP, CASES[1]):
        I, exact, _, diff = recorded(case)
        wrong = online_block(I, True, **{mutation: True})
        beyond = {n: normwise(wrong[n], exact[n]) / diff[n] for n in OUTPUTS if not np.isfinite(wrong[n]).all() or normwise(wrong[n], exact[n]) > 4 * diff[n]}
        print(mutation, case, {n: round(float(v), 1) for n, v in beyond.items()})
        caught[case] = beyond
    assert all(caught.values()), caught


@pytest.mark.parametrize("s", [32, 512, 1024])
def test_exact_forward_case_is_the_same_in_float32_and_float64(s):
    I = exact_inputs(s)
    o32, o64 = online_block(I, True, np.float32, backward=False), online_block(I, True, np.float64, backward=False)
    for n in ("q", "k", "v", "attention", "out"):
        a = o64[n]
        assert np.array_equal(a * 65536, np.round(a * 65536)) and np.abs(a).max() < 128, (n, np.abs(a).max())     # multiples of 2^-16 below 2^7
        assert o32[n].dtype == np.float32 and np.array_equal(o32[n].astype(np.float64), a), n
    assert not np.any(o64["q"]) and np.abs(o64["lse"] - np.log(s)).max() < 1e-12
    assert np.array_equal(o64["out"], block(I, True, np.float64, backward=False)["out"])
    assert len(np.unique(o64["attention"])) > 8 and len(np.unique(o64["out"])) > 8        # not a trivial tensor


# ---- the entries that need no device ---------------------------------------------------------------------------------------------------------------------
def test_applies_over_the_boundary_values(pkg):
    f = pkg.attention_online_bf16_applies
    want = lambda c, s, d: s % 32 == 0 and 32 <= s <= 4096 and d % 8 == 0 and 8 <= d <= 64 and c % 8 == 0 and c > 0
    for c in (0, 4, 8, 12, 16, 24, 256, 260, 264):
        for s in (0, 16, 31, 32, 33, 256, 288, 4064, 4096, 4097, 4128, 8192):
            for d in (0, 4, 8, 12, 16, 24, 56, 64, 68, 72, 128):
                assert f(c, s, d) == want(c, s, d), (c, s, d)
    assert f(256, 1024, 16) and f(256, 4096, 16) and not f(256, 16, 16)       # 64 x 64 images at the reference's widths; its 4 x 4 mid block stays fp32
    assert not f(-8, 32, 8) and not f(8, -32, 8) and not f(8, 32, -8)
    assert KB == 32      # include/bla.h's BLA_ATTENTION_ONLINE_KEYS
    with open(os.path.join(os.path.dirname(EX), "include", "bla.h")) as h:
        assert "#define BLA_ATTENTION_ONLINE_KEYS 32" in h.read()


def test_entries_refuse_without_touching_the_device(pkg):
    """shape and NULL refusals come back as BLA_ERR_INVALID (1) on a machine with a device and as 'no device' (3) on one without: never a crash"""
    L = pkg.lib()
    ws = pkg.attention_ws()
    for c, s, d in [(64, 16, 16), (64, 4128, 16), (64, 64, 4), (64, 64, 72), (12, 64, 16), (64, 64, 16)]:
        assert L.bla_attention_forward_batched_online_bf16(None, 2, None, None, None, None, None, None, C.byref(ws), None, c, s, d) in (1, 3)
        assert L.bla_attention_backward_batched_online_bf16(None, 2, *([None] * 6), C.byref(ws), C.byref(ws), *([None] * 6), c, s, d) in (1, 3)
        assert L.bla_attention_forward_batched_online_bf16(None, 2, *([None] * 8), c, s, d) in (1, 3)
        assert L.bla_attention_backward_batched_online_bf16(None, 0, *([None] * 14), c, s, d) in (1, 3)


def test_online_mode_by_name(pkg):
    L = pkg.lib()
    assert pkg.UNET_ATTENTION_BF16_ONLINE == 3 == pkg.UNET_ATTENTION_BF16 | 2
    assert L.bla_unet_set_attention(None, pkg.UNET_ATTENTION_BF16_ONLINE) == 1 and b"null" in L.bla_last_error() and b"mode" not in L.bla_last_error()
    assert L.bla_unet_set_attention(None, 2) == 1 and b"mode" in L.bla_last_error()      # an online softmax on fp32 products does not exist


@pytest.fixture(scope="module")
def prog(pkg):
    pkg.build_native()
    subprocess.check_call(["make", "-s", "-C", EX, "cifar_unet_gpu"])
    return os.path.join(EX, "cifar_unet_gpu")


def test_program_accepts_online_before_any_device_is_opened(prog, tmp_path):
    """an unknown sub-command is refused after the environment is read and needs no device: `online` gets that far, an unknown value does not"""
    def go(value):
        r = subprocess.run([prog, "no-such-command"], cwd=str(tmp_path), env=dict(os.environ, BLA_UNET_ATTENTION=value), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           text=True, timeout=60)
        return r.returncode, r.stdout + r.stderr
    code, text = go("online")
    assert code != 0 and "Unrecognized argument" in text and "BLA_UNET_ATTENTION" not in text, (code, text)
    code, text = go("on-line")
    assert code != 0 and "BLA_UNET_ATTENTION" in text and "online" in text and "Unrecognized" not in text, (code, text)
    assert not os.listdir(tmp_path)
