"""The bf16 self-attention block (bla_attention_{forward,backward}_batched_bf16) restated in numpy, on the host.

block() is include/bla.h's arithmetic line by line: both operands of every matrix product rounded with bla_f32_to_bf16's rounding immediately before
the product (rounded=True) or not at all (rounded=False: the exact float64 block); everything else in the working precision.  What this file RECORDS, per
case and tensor, is ||rounded - exact|| / ||exact||: what the mixed-precision arithmetic costs on these inputs.  tests/test_attention_bf16_gpu.py holds the
device inside twice that (the device shares the roundings; fp32 accumulation, expf and the few elements that round the other way do not show beside a
unit roundoff of 2^-9 -- DESIGN 3.25 / 3.26's practice).

Inputs (make_inputs): x, del_y uniform in [-1, 1); Wq, Wk uniform with gain 1.5 sqrt(3 / C), Wv and W with gain sqrt(3 / C) resp. sqrt(3 / d); bias in
[-0.5, 0.5).  That makes Q and K elements of standard deviation 0.87 and logits of standard deviation 0.75, i.e. spread over about +-2.5: a softmax that is
neither uniform nor one-hot.  (Q and K at 0.2 - 0.5 per element give logits within +-0.3 at d = 16 -- an almost uniform softmax whose gradient through the
scores is noise; the logit spread is the requirement that was kept.)

Two host-only requirements on the recorded values, as in tests/test_unet_bf16_host.py:
  (a) they are a property of the arithmetic, not of one draw of the roundings: a relative 2^-23 perturbation of every product's result in front of its
      next rounding moves no recorded value by more than half of itself;
  (b) they catch wiring errors: each of six wrong blocks puts some tensor more than 4 times its recorded value away from exact.
The exact forward case (Wq = 0, small integers) has the same bits in float32 and in float64, whatever the order of summation: the device must hit them.

The nine CASES reach nine of the backward core's sixteen instantiations att_bf16_bwd_core_kernel<S / 32, ceil(d / 32)>: <1, 1>, <2, 1>, <3, 1>, <4, 1>, <5, 1>,
<8, 1> and <6, 2>, <7, 2>, <8, 2> -- among them every S / 32 in {5, 6, 7}, where the second round of row blocks has active and parked waves side by side, d = 32
(the last on one d tile) and d = 40, 48 (two d tiles, off and on a multiple of 16); batch 11 takes the fold's unrolled loop and its tail."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import test_norm_bf16_host as tnb
from conftest import ROOT
from inputs import uniform

# (B, C, S, d)
CASES = [(2, 24, 32, 8),       # one wave, padded contraction, C off 16 and 32
         (3, 64, 96, 16),      # three row blocks, S not a power of two
         (2, 40, 64, 24),      # d off 16
         (1, 256, 256, 16),    # the model's shape, largest S
         (2, 32, 256, 64),     # largest d
         # appended (seeds go by index; CASES[1] is named elsewhere): S / 32 in {5, 6, 7} -- the second round of row blocks of the backward core has some waves
         # active and the others parked on row block 0 -- and the d classes the five above leave out
         (11, 16, 160, 8),     # S / 32 = 5: one wave active in the second round; batch 8 + 3 through the fold's unrolled loop and its tail; C < 32
         (2, 72, 128, 32),     # S / 32 = 4; d = 32, the last d on one 32-wide d tile; C off 16 and 32
         (1, 48, 192, 48),     # S / 32 = 6, two d tiles
         (1, 8, 224, 40)]      # S / 32 = 7, two d tiles, d off 16, smallest C
OUTPUTS = ["out", "del_x", "del_wq", "del_wk", "del_wv", "del_w"]
EX = os.path.join(ROOT, "examples")


def rnd(a):
    """bla_f32_to_bf16's rounding of the fp32 value, back in the array's own precision"""
    a = np.asarray(a)
    return tnb.widen(tnb.rne(a.astype(np.float32))).astype(a.dtype)


def make_inputs(case, logit_gain=1.0):
    b, c, s, d = case
    seed = 9100 + 10 * CASES.index(case) if case in CASES else 9900 + s
    gc, gd = float(np.sqrt(3.0 / c)), float(np.sqrt(3.0 / d))
    return dict(x=uniform(seed, (b, c, s), -1, 1, np.float32), wq=uniform(seed + 1, (c, d), -1.5 * gc * logit_gain, 1.5 * gc * logit_gain, np.float32),
                wk=uniform(seed + 2, (c, d), -1.5 * gc, 1.5 * gc, np.float32), wv=uniform(seed + 3, (c, d), -gc, gc, np.float32),
                w=uniform(seed + 4, (d, c), -gd, gd, np.float32), bias=uniform(seed + 5, (c,), -0.5, 0.5, np.float32),
                del_y=uniform(seed + 6, (b, c, s), -1, 1, np.float32))


def exact_inputs(s, c=16, d=16, b=2):
    """Wq = 0, so T = 0 and P = 1 / S exactly; x, Wv, W, bias small integers (sparse, so that sums stay small)"""
    def ints(seed, shape, keep):
        return (np.sign(uniform(seed, shape, -1, 1)) * (uniform(seed + 50, shape, 0, 1) < keep)).astype(np.float32)
    return dict(x=ints(9800 + s, (b, c, s), 0.5), wq=np.zeros((c, d), np.float32), wk=ints(9801 + s, (c, d), 0.5), wv=ints(9802 + s, (c, d), 0.5),
                w=ints(9803 + s, (d, c), 0.5), bias=ints(9804 + s, (c,), 1.0) * 3, del_y=np.zeros((b, c, s), np.float32))


def block(I, rounded=True, dtype=np.float64, backward=True, eps_seed=None, drop_inv=False, untransposed_dk=False, drop_rowdot=False, drop_wk_term=False,
          untransposed_dv=False, no_row_max=False):
    """include/bla.h's arithmetic; the keyword mutations are the wrong blocks of requirement (b).  eps_seed: requirement (a)'s perturbation."""
    T_ = dtype
    r = rnd if rounded else (lambda a: a)
    rng = np.random.default_rng(eps_seed) if eps_seed is not None else None

    def prod(a, b):
        p = np.matmul(r(a), r(b))
        return p if rng is None else p * (1 + 2.0 ** -23 * rng.choice([-1.0, 1.0], p.shape))
    x, wq, wk, wv, w, bias, dy = (np.asarray(I[n], T_) for n in ("x", "wq", "wk", "wv", "w", "bias", "del_y"))
    d = wq.shape[1]
    inv = T_(np.float32(1.0 / np.sqrt(float(d))))
    z = np.swapaxes(x, 1, 2)                                      # [B][S][C]
    o = dict(q=prod(z, wq), k=prod(z, wk), v=prod(z, wv))
    t = inv * prod(o["q"], np.swapaxes(o["k"], 1, 2))
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(t if no_row_max else t - t.max(axis=2, keepdims=True))
        o["weights"] = p = (e / e.sum(axis=2, keepdims=True)).astype(T_)
    o["attention"] = a = prod(p, o["v"])
    o["out"] = np.swapaxes(prod(a, w) + bias, 1, 2)
    if not backward:
        return o
    dyt = np.swapaxes(dy, 1, 2)                                   # del_Y' [B][S][C]
    o["del_w"] = prod(np.swapaxes(a, 1, 2), dyt).sum(axis=0)
    dp = prod(dyt, w.T)
    ds = prod(dp, np.swapaxes(o["v"], 1, 2))
    o["del_v"] = dv = prod(p if untransposed_dv else np.swapaxes(p, 1, 2), dp)
    dot = 0 if drop_rowdot else (p * ds).sum(axis=2, keepdims=True)
    di = (p * (ds - dot)) * (1 if drop_inv else inv)
    o["del_q"] = dq = prod(di, o["k"])
    o["del_k"] = dk = prod(di if untransposed_dk else np.swapaxes(di, 1, 2), o["q"])
    for n, g in (("del_wq", dq), ("del_wk", dk), ("del_wv", dv)):
        o[n] = prod(x, g).sum(axis=0)                             # Z^T = X
    o["del_x"] = prod(wq, np.swapaxes(dq, 1, 2)) + (0 if drop_wk_term else prod(wk, np.swapaxes(dk, 1, 2))) + prod(wv, np.swapaxes(dv, 1, 2))
    return o


def normwise(a, b):
    return float(np.linalg.norm((np.asarray(a, np.float64) - b).ravel()) / np.linalg.norm(np.asarray(b, np.float64).ravel()))


@functools.lru_cache(maxsize=None)
def recorded(case):
    """(inputs, exact block, rounded block, {tensor: ||rounded - exact|| / ||exact||}) -- once per process; tests/test_attention_bf16_gpu.py reads it here"""
    I = make_inputs(case)
    exact, rounded = block(I, False), block(I, True)
    return I, exact, rounded, {n: normwise(rounded[n], exact[n]) for n in OUTPUTS}


@pytest.mark.parametrize("case", CASES, ids=str)
def test_rounding_differences_are_recorded(case):
    I, exact, rounded, diff = recorded(case)
    t = exact["q"] @ np.swapaxes(exact["k"], 1, 2) / np.sqrt(case[3])
    print(f"{case}: Q std {exact['q'].std():.2f}, logits std {t.std():.2f}, range {t.min():.1f} .. {t.max():.1f}; " + ", ".join(f"{n} {v:.2e}" for n, v in diff.items()))
    assert all(2.0 ** -12 < v < 2.0 ** -4 for v in diff.values()), diff      # a few unit roundoffs of bf16, in every tensor
    assert 0.4 < t.std() < 1.5 and t.max() - t.min() > 3                      # logits spread over a few units


def test_unrounded_block_is_attention_and_its_gradient():
    """the exact block against the closed form of the forward pass, and its del_x against central differences of <out, del_y>"""
    I, exact, _, _ = recorded(CASES[0])
    for b in range(CASES[0][0]):
        z = I["x"][b].astype(np.float64).T
        q, k, v = z @ I["wq"], z @ I["wk"], z @ I["wv"]
        t = q @ k.T * float(np.float32(1 / np.sqrt(CASES[0][3])))
        p = np.exp(t - t.max(1, keepdims=True)); p /= p.sum(1, keepdims=True)
        assert normwise(exact["out"][b], ((p @ v) @ I["w"] + I["bias"]).T) < 1e-12
    I1 = {n: (a[:1] if n in ("x", "del_y") else a) for n, a in I.items()}
    g = block(I1, False)["del_x"][0]
    for (ci, si) in [(0, 0), (5, 17), (23, 31)]:
        h = 1e-6
        xp = I1["x"].astype(np.float64).copy(); xp[0, ci, si] += h
        xm = I1["x"].astype(np.float64).copy(); xm[0, ci, si] -= h
        fd = ((block(dict(I1, x=xp), False, backward=False)["out"] - block(dict(I1, x=xm), False, backward=False)["out"]) * I1["del_y"]).sum() / (2 * h)
        assert abs(fd - g[ci, si]) <= 1e-6 * max(1, abs(fd)), (ci, si, fd, g[ci, si])


@pytest.mark.parametrize("case", CASES, ids=str)
@pytest.mark.parametrize("draw", [0, 1])
def test_recorded_values_do_not_depend_on_the_draw(case, draw):
    """requirement (a)"""
    I, exact, rounded, diff = recorded(case)
    other = block(I, True, eps_seed=draw)
    moved = {n: normwise(other[n], rounded[n]) / diff[n] for n in OUTPUTS}
    print(case, draw, {n: round(v, 3) for n, v in moved.items()})
    assert max(moved.values()) <= 0.5, moved


MUTATIONS = ["drop_inv", "untransposed_dk", "drop_rowdot", "drop_wk_term", "untransposed_dv"]


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_four_times_the_recorded_value_catches_a_wiring_error(mutation):
    """requirement (b), the five backward mutations, on the square case (S = C = 64 makes the untransposed products well-formed)"""
    case = (2, 64, 64, 16)
    I = make_inputs(case)
    exact, rounded = block(I, False), block(I, True)
    diff = {n: normwise(rounded[n], exact[n]) for n in OUTPUTS}
    wrong = block(I, True, **{mutation: True})
    beyond = {n: normwise(wrong[n], exact[n]) / diff[n] for n in OUTPUTS if normwise(wrong[n], exact[n]) > 4 * diff[n]}
    print(mutation, {n: round(v, 1) for n, v in beyond.items()})
    assert beyond and all(np.isfinite(wrong[n]).all() for n in OUTPUTS)


def test_softmax_without_the_row_maximum_is_caught_at_large_logits():
    """requirement (b), sixth mutation: at logits of +-60 the block stays finite in float32 only because the row maximum is subtracted"""
    case = (2, 64, 64, 16)
    I = make_inputs(case, logit_gain=40.0)
    good = block(I, True, np.float32)
    t = block(I, False)
    logits = t["q"] @ np.swapaxes(t["k"], 1, 2) / 4
    assert logits.max() > 60 and logits.min() < -60
    assert all(np.isfinite(good[n]).all() for n in OUTPUTS)
    diff = {n: normwise(good[n], t[n]) for n in OUTPUTS}
    wrong = block(I, True, np.float32, no_row_max=True)
    assert any(not np.isfinite(wrong[n]).all() or normwise(wrong[n], t[n]) > 4 * diff[n] for n in OUTPUTS)
    assert not np.isfinite(wrong["out"]).all()           # exp(60 ..) overflows float32's 3.4e38 at 88.7: here logits reach past it


@pytest.mark.parametrize("s", [32, 256])
def test_exact_forward_case_is_the_same_in_float32_and_float64(s):
    I = exact_inputs(s)
    o32, o64 = block(I, True, np.float32, backward=False), block(I, True, np.float64, backward=False)
    for n in ("q", "k", "v", "weights", "attention", "out"):
        a = o64[n]
        assert np.array_equal(a * 65536, np.round(a * 65536)) and np.abs(a).max() < 128, (n, np.abs(a).max())     # multiples of 2^-16 below 2^7
        assert o32[n].dtype == np.float32 and np.array_equal(o32[n].astype(np.float64), a), n
    assert np.all(o64["weights"] == 1.0 / s) and not np.any(o64["q"])
    assert len(np.unique(o64["attention"])) > 8 and len(np.unique(o64["out"])) > 8        # not a trivial tensor


# ---- the entries that need no device ---------------------------------------------------------------------------------------------------------------------
def test_applies_over_the_boundary_values(pkg):
    f = pkg.attention_bf16_applies
    want = lambda c, s, d: s % 32 == 0 and 32 <= s <= 256 and d % 8 == 0 and 8 <= d <= 64 and c % 8 == 0 and c > 0
    for c in (0, 4, 8, 12, 16, 24, 256, 260, 264):
        for s in (0, 16, 31, 32, 33, 48, 64, 96, 224, 256, 257, 288, 512):
            for d in (0, 4, 8, 12, 16, 24, 56, 64, 68, 72, 128):
                assert f(c, s, d) == want(c, s, d), (c, s, d)
    assert f(256, 256, 16) and f(256, 64, 16) and not f(256, 16, 16)       # the reference's constants: 16 x 16 and 8 x 8 qualify, the 4 x 4 mid block does not
    assert not f(-8, 32, 8) and not f(8, -32, 8) and not f(8, 32, -8)


def test_entries_refuse_without_touching_the_device(pkg):
    """shape and NULL refusals come back as BLA_ERR_INVALID (1) on a machine with a device and as 'no device' (3) on one without: never a crash"""
    L = pkg.lib()
    ws = pkg.attention_ws()
    for c, s, d in [(64, 16, 16), (64, 288, 16), (64, 64, 4), (64, 64, 72), (12, 64, 16)]:
        assert L.bla_attention_forward_batched_bf16(None, 2, None, None, None, None, None, None, C.byref(ws), None, c, s, d) in (1, 3)
        assert L.bla_attention_backward_batched_bf16(None, 2, *([None] * 6), C.byref(ws), C.byref(ws), *([None] * 6), c, s, d) in (1, 3)


def test_attention_mode_defaults_and_refusals(pkg):
    L = pkg.lib()
    assert pkg.UNET_ATTENTION_F32 == 0 and pkg.UNET_ATTENTION_BF16 == 1
    assert L.bla_unet_attention(None) == pkg.UNET_ATTENTION_F32            # what every model starts with
    for mode in (2, -1, 7):
        assert L.bla_unet_set_attention(None, mode) == 1 and b"mode" in L.bla_last_error()
    assert L.bla_unet_set_attention(None, pkg.UNET_ATTENTION_BF16) == 1 and b"null" in L.bla_last_error()


@pytest.fixture(scope="module")
def prog(pkg):
    pkg.build_native()
    subprocess.check_call(["make", "-s", "-C", EX, "cifar_unet_gpu"])
    return os.path.join(EX, "cifar_unet_gpu")


@pytest.mark.parametrize("args", [["run"], ["train", "1"], ["init"], ["draws", "1", "out"], ["fit", "1"], ["eval"], ["sample"]], ids=lambda a: a[0])
def test_program_refuses_an_unknown_attention_value(prog, tmp_path, args):
    r = subprocess.run([prog] + args, cwd=str(tmp_path), env=dict(os.environ, BLA_UNET_ATTENTION="bogus"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode != 0 and "BLA_UNET_ATTENTION" in r.stdout + r.stderr, (r.returncode, r.stdout, r.stderr)
    assert not os.listdir(tmp_path)      # (init wrote nothing)
