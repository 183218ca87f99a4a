"""Training objectives without a device (include/bla.h, "training objectives"): the cosine betas against a float64 restatement, the float64 identities
between the three parametrisations (eps, x0, v) and their Min-SNR weights, a numpy float32 restatement of the target, conversion and loss kernels
inside the rounding bounds that tests/test_objective_gpu.py holds the device to -- and outside them under six plausible mistakes -- and the example
program's refusal of malformed or contradictory BLA_UNET_SCHEDULE / BLA_UNET_PREDICT / BLA_UNET_MIN_SNR before it needs a device.

u = 2^-24.  The bounds count roundings, one per fp32 coefficient and one per multiply, fma or divide:
  v target  fmaf(a, eps, -(c x0)):   a, c, the product, the fma              4 u (|a eps| + |c x0|)
  v -> eps  fmaf(a, v, c x):         the same count                          4 u (|a v| + |c x|)
  x0 -> eps fmaf(-a, x0, x) / c:     a, c, the fma, the division (+ 2nd order) 5 u (|x| + |a x0|) / c
  loss      w sum d^2 in double:     d, d^2, F - 1 additions at most, the product with w      (F + 4) 2^-53 loss"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from inputs import uniform
from test_dpmpp_host import BIN, SAMPLE_ENV, fmaf, prog, schedule  # noqa: F401  (prog is a fixture)

U = 2.0 ** -24
EPS, X0, V = 0, 1, 2
BLA_ERR_INVALID = 1
T = 1000
TS = (0, 1, 49, 499, 979, 998, 999)
B, FL = 3, 75


# ---- the float64 restatement ---------------------------------------------------------------------------------------------------------------

def cosine_betas(steps, s=0.008, max_beta=0.999):
    """bla_diffusion_cosine_betas operation for operation (math.cos is the C library's)"""
    f = []
    for i in range(steps + 1):
        c = math.cos((i / steps + s) / (1 + s) * math.pi / 2)
        f.append(c * c)
    return np.array([min(1.0 - f[i + 1] / f[i], max_beta) for i in range(steps)]), np.array(f)


def schedule_from_betas(beta):
    """bla_diffusion_create_from_betas' doubles, [T][beta, alpha_bar]"""
    beta = np.asarray(beta, np.float64)
    return np.stack([beta, np.cumprod(1.0 - beta)], axis=1)


def schedules():
    return {"linear": schedule(T), "cosine": schedule_from_betas(cosine_betas(T)[0])}


def loss_weights(ab, prediction, gamma):
    """w_t of bla_diffusion_set_objective in its order of operations"""
    ab = np.asarray(ab, np.float64)
    if gamma == 0:
        return np.ones_like(ab)
    snr = ab / (1.0 - ab)
    m = np.minimum(snr, gamma)
    if prediction == EPS:
        return np.where(snr > 0, m / np.where(snr > 0, snr, 1.0), 1.0)          # abar underflown to 0: the limit, not 0 / 0
    return m if prediction == X0 else m / (snr + 1.0)


def coef(sched, t):
    """a = sqrt(abar_t), c = sqrt(1 - abar_t) in double; t an int or an array of one int per image (then columns)"""
    ab = sched[np.asarray(t), 1]
    a, c = np.sqrt(ab), np.sqrt(1.0 - ab)
    return (a[:, None], c[:, None]) if np.ndim(t) else (a, c)


def v_of(a, c, x0, eps):
    return a * eps - c * x0


def eps_from_v(a, c, v, x):
    return a * v + c * x


def eps_from_x0(a, c, x0, x):
    return (x - a * x0) / c


# ---- the kernels' arithmetic in numpy float32 ----------------------------------------------------------------------------------------------

def f32(v):
    return np.asarray(v, np.float64).astype(np.float32)


def f32_target(a, c, x0, eps, prediction, mutate=None):
    a, c = f32(a), f32(c)
    if mutate == "swap_ac":
        a, c = c, a
    if prediction == EPS:
        return eps.copy()
    if prediction == X0:
        return x0.copy()
    p = c * x0
    return fmaf(a, eps, p if mutate == "v_sign" else -p)


def f32_to_eps(a, c, pred, x, prediction, mutate=None, x0=None):
    a, c = f32(a), f32(c)
    if mutate == "swap_ac":
        a, c = c, a
    if mutate == "x0_for_xt":
        x = x0
    if prediction == V:
        return fmaf(a, pred, c * x)
    if prediction == X0:
        return fmaf(-a, pred, x) / c
    return pred.copy()


def f32_weights(ab, prediction, gamma, mutate=None):
    if mutate == "eps_weight_for_v" and prediction == V:
        prediction = EPS
    if mutate == "gamma_ignored":
        gamma = 0
    return loss_weights(ab, prediction, gamma).astype(np.float32)


def f32_loss(out, target, w, mutate=None):
    """g in float32 and the per-image loss in double, as bla_diffusion_loss_f32 forms them"""
    w = np.ones(out.shape[0], np.float32) if w is None else np.asarray(w, np.float32)
    g = (np.float32(2) * w)[:, None] * (out - target)
    d = out.astype(np.float64) - target.astype(np.float64)
    wd = w.astype(np.float64)
    return g, (wd * wd if mutate == "w_squared" else wd) * (d * d).sum(axis=1)


def inputs(seed, shape=(B, FL)):
    return uniform(seed, shape, -1, 1, np.float32), uniform(seed + 1, shape, -2, 2, np.float32)      # x0, eps


def noised(a, c, x0, eps):
    """x_t as the noising kernels leave it in fp32 (either rounding: the bounds below take x_t as given)"""
    return fmaf(f32(a), x0, f32(c) * eps)


# ---- 1: the cosine betas -------------------------------------------------------------------------------------------------------------------

def device_cosine_betas(L, steps, s=0.008, max_beta=0.999):
    out = np.full(max(steps, 1), -7.0)
    return L.bla_diffusion_cosine_betas(steps, s, max_beta, out.ctypes.data), out


def test_cosine_betas(pkg):
    L = pkg.lib()
    for steps in (20, 50, 1000):
        st, got = device_cosine_betas(L, steps)
        want, f = cosine_betas(steps)
        assert st == 0
        err = np.abs(got - want).max()
        print(f"cosine betas, T = {steps}: worst |difference| {err:.1e} (bound {4 * 2.0 ** -53:.1e})")
        assert err <= 4 * 2.0 ** -53                       # absolute: beta = 1 - ratio cancels
        assert (got > 0).all() and (got < 1).all()
        assert (got == 0.999).sum() == 1 and got[-1] == 0.999 and (got[:-1] < 0.999).all()
        ab = np.cumprod(1.0 - got)
        free = np.arange(steps) < steps - 1                # no cap acts before the last step
        assert np.abs(ab[free] / (f[1:][free] / f[0]) - 1).max() <= 1e-12
    assert abs(np.cumprod(1.0 - device_cosine_betas(L, 1000)[1])[-1] - 2.4e-9) < 1e-10      # DESIGN.md 3.16 quotes it
    st, got = device_cosine_betas(L, 7, 0.0, 0.5)          # s = 0 is allowed: f(0) = 1; the cap moves
    assert st == 0 and (got <= 0.5).all() and got[-1] == 0.5
    for steps, s, mb in ((0, 0.008, 0.999), (-3, 0.008, 0.999), (10, -1e-9, 0.999), (10, float("nan"), 0.999), (10, 0.008, 0.0), (10, 0.008, 1.0),
                         (10, 0.008, -0.1), (10, 0.008, 1.5), (10, 0.008, float("nan"))):
        st, out = device_cosine_betas(L, steps, s, mb)
        assert st == BLA_ERR_INVALID and (out == -7).all(), (steps, s, mb)
    assert L.bla_diffusion_cosine_betas(10, 0.008, 0.999, None) == BLA_ERR_INVALID


# ---- 2: float64 identities -----------------------------------------------------------------------------------------------------------------

def test_float64_identities():
    x0, eps = (v.astype(np.float64) for v in inputs(31))
    sign = np.where(uniform(33, (B, FL), -1, 1, np.float32) < 0, -1.0, 1.0)
    delta = sign * uniform(34, (B, FL), 0.5, 2, np.float32).astype(np.float64)         # x0_hat - x0, |delta| >= 0.5
    checked, skipped = 0, []
    for name, sched in schedules().items():
        for t in TS:
            a, c = coef(sched, t)
            x = a * x0 + c * eps
            tol = 1e-12 * (np.abs(x) + np.abs(eps)) / c
            assert (np.abs(eps_from_v(a, c, v_of(a, c, x0, eps), x) - eps) <= tol).all(), (name, t)
            assert (np.abs(eps_from_x0(a, c, x0, x) - eps) <= tol).all(), (name, t)
            # one prediction three ways: x0_hat, the eps_hat and the v_hat it implies at this x_t
            x0h = x0 + delta
            eh = eps_from_x0(a, c, x0h, x)
            vh = v_of(a, c, x0h, eh)
            v = v_of(a, c, x0, eps)
            sq = {EPS: ((eh - eps) ** 2).sum(), X0: ((x0h - x0) ** 2).sum(), V: ((vh - v) ** 2).sum()}
            ab = sched[t, 1]
            snr = ab / (1.0 - ab)
            # eh - eps = -(a / c) delta is formed as a difference of two numbers of size |eps| <= 2.  eh carries about three roundings of that size, so
            # with |delta| >= 0.5 each element of the difference is off by up to 3 x 2^-53 x 2 / ((a / c) 0.5) = 12 x 2^-53 c / a of its value, and the
            # squared norm by twice that.  24 x 2^-53 c / a reaches 1e-12 at c / a = 375: beyond it (the cosine schedule's last two steps, c / a = 640 and 2e4)
            # double arithmetic does not resolve the identity to 1e-12 and it is not asserted
            if c / a > 375:
                skipped.append((name, t))
                continue
            for gamma in (0.5, 5.0):
                w = {p: float(loss_weights(ab, p, gamma)) for p in (EPS, X0, V)}
                assert abs(w[X0] / w[EPS] / snr - 1) <= 1e-15 and abs(w[X0] / w[V] / (snr + 1.0) - 1) <= 1e-15      # they differ exactly by SNR and SNR + 1
                le, lx, lv = (w[p] * sq[p] for p in (EPS, X0, V))
                assert abs(le / lx - 1) <= 1e-12 and abs(lv / lx - 1) <= 1e-12, (name, t, gamma, le, lx, lv)
                checked += 1
            for p in (EPS, X0, V):
                assert float(loss_weights(ab, p, 0.0)) == 1.0
    assert skipped == [("cosine", 998), ("cosine", 999)] and checked == 2 * (2 * len(TS) - 2)
    sched = schedules()["cosine"]
    w = loss_weights(sched[:, 1], EPS, 5.0)
    assert (w <= 1).all() and w[-1] == 1.0 and w[0] < 1e-3 and (np.diff(w) >= 0).all()                           # the clamp acts at high SNR only


# ---- 3: the float32 restatement inside its bounds, six mistakes outside ---------------------------------------------------------------------

def fractions(sched, t, gamma=5.0, mutate=None):
    """worst fraction of its bound for the v target, v -> eps, x0 -> eps, and the loss of each prediction type, at timestep t"""
    a, c = coef(sched, t)
    x0, eps = inputs(41 + t)
    x0d, epsd = x0.astype(np.float64), eps.astype(np.float64)
    x = noised(a, c, x0, eps)
    xd = x.astype(np.float64)
    out = {}
    # target
    got = f32_target(a, c, x0, eps, V, mutate)
    out["v target"] = (np.abs(got - v_of(a, c, x0d, epsd)) / (4 * U * (np.abs(a * epsd) + np.abs(c * x0d)))).max()
    assert np.array_equal(f32_target(a, c, x0, eps, EPS, mutate), eps) and np.array_equal(f32_target(a, c, x0, eps, X0, mutate), x0)
    # conversion of an arbitrary model output, against float64 on the same fp32 inputs
    vh, x0h = uniform(51 + t, (B, FL), -2, 2, np.float32), uniform(52 + t, (B, FL), -1.5, 1.5, np.float32)
    got = f32_to_eps(a, c, vh, x, V, mutate, x0)
    out["v -> eps"] = (np.abs(got - eps_from_v(a, c, vh.astype(np.float64), xd)) / (4 * U * (np.abs(a * vh) + np.abs(c * xd)))).max()
    got = f32_to_eps(a, c, x0h, x, X0, mutate, x0)
    out["x0 -> eps"] = (np.abs(got - eps_from_x0(a, c, x0h.astype(np.float64), xd)) / (5 * U * (np.abs(xd) + np.abs(a * x0h)) / c)).max()
    assert np.array_equal(f32_to_eps(a, c, vh, x, EPS, mutate, x0), vh)
    # loss: the fp32 weight is within u of the double, the sum within (F + 4) 2^-53
    ab = np.full(B, sched[t, 1])
    for p in (EPS, X0, V):
        w = f32_weights(ab, p, gamma, mutate)
        target = f32_target(a, c, x0, eps, p)
        loss = f32_loss(vh, target, w, mutate)[1]
        d = vh.astype(np.float64) - target.astype(np.float64)
        want = loss_weights(ab, p, gamma) * np.array([math.fsum(r) for r in d * d])
        out["loss", p] = (np.abs(loss - want) / ((U + (FL + 4) * 2.0 ** -53) * want)).max()
    return out


def test_rounding_bound_and_mutations():
    worst = {}
    scheds = schedules()
    for name, sched in scheds.items():
        for t in TS:
            for k, v in fractions(sched, t).items():
                worst[k] = max(worst.get(k, 0), v)
    print("float32 restatement, worst fraction of its bound over both schedules and t in %s: " % (TS,) + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1, worst
    broken = {"v_sign": ["v target"], "swap_ac": ["v target", "v -> eps", "x0 -> eps"], "x0_for_xt": ["v -> eps", "x0 -> eps"],
              "eps_weight_for_v": [("loss", V)], "gamma_ignored": [("loss", EPS), ("loss", V), ("loss", X0)], "w_squared": [("loss", EPS), ("loss", V)]}
    for mutate, keys in broken.items():
        for key in keys:
            over = max(fractions(sched, t, mutate=mutate)[key] for sched in scheds.values() for t in TS)
            assert over > 1, (mutate, key, over)


# ---- 4: the example program ------------------------------------------------------------------------------------------------------------------

OBJECTIVE_ENV = ("BLA_UNET_SCHEDULE", "BLA_UNET_PREDICT", "BLA_UNET_MIN_SNR", "BLA_UNET_EVAL_EMA", "BLA_CIFAR_EVAL_FILE", "BLA_UNET_EVAL_STEPS")


def run_program(args, cwd, env, timeout=120):
    e = dict(os.environ, **env)
    for k in SAMPLE_ENV + OBJECTIVE_ENV:
        if k not in env:
            e.pop(k, None)
    return subprocess.run([BIN] + args, cwd=str(cwd), env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)


VERBS = (["fit", "1", "4"], ["sample", "2", "out"], ["eval"])


def test_program_refuses_bad_objective_options(prog, tmp_path):
    for env, named in (({"BLA_UNET_SCHEDULE": "quadratic"}, "BLA_UNET_SCHEDULE=quadratic"), ({"BLA_UNET_SCHEDULE": "Cosine"}, "BLA_UNET_SCHEDULE=Cosine"),
                       ({"BLA_UNET_PREDICT": "V"}, "BLA_UNET_PREDICT=V"), ({"BLA_UNET_PREDICT": "noise"}, "BLA_UNET_PREDICT=noise"),
                       ({"BLA_UNET_MIN_SNR": "-1"}, "BLA_UNET_MIN_SNR=-1"), ({"BLA_UNET_MIN_SNR": "nan"}, "BLA_UNET_MIN_SNR=nan"),
                       ({"BLA_UNET_MIN_SNR": "inf"}, "BLA_UNET_MIN_SNR=inf"), ({"BLA_UNET_MIN_SNR": "5x"}, "BLA_UNET_MIN_SNR=5x"),
                       ({"BLA_UNET_MIN_SNR": "five"}, "BLA_UNET_MIN_SNR=five"),
                       ({"BLA_UNET_SCHEDULE": "cosine", "BLA_UNET_PREDICT": "v", "BLA_UNET_MIN_SNR": "1e999"}, "BLA_UNET_MIN_SNR=1e999")):
        for args in VERBS:
            r = run_program(args, tmp_path, env)
            assert r.returncode == 1, (args, env, r.stdout + r.stderr)
            assert named in r.stderr, (args, env, r.stderr)
    assert os.listdir(tmp_path) == []


def test_program_refuses_options_that_contradict_the_file(prog, tmp_path):
    w = tmp_path / "w"
    (w / "ema").mkdir(parents=True)
    (w / "objective.txt").write_text("schedule=cosine predict=v min_snr=5\n")
    (w / "ema" / "objective.txt").write_text("schedule=linear predict=x0 min_snr=0\n")
    base = {"BLA_UNET_WEIGHTS": str(w)}
    for env in ({"BLA_UNET_PREDICT": "eps"}, {"BLA_UNET_PREDICT": "x0"}, {"BLA_UNET_SCHEDULE": "linear"}, {"BLA_UNET_MIN_SNR": "4"}, {"BLA_UNET_MIN_SNR": "0"},
                {"BLA_UNET_SCHEDULE": "cosine", "BLA_UNET_PREDICT": "v", "BLA_UNET_MIN_SNR": "0.5"}):
        for args in (["sample", "2", "out"], ["eval"], ["fit", "1", "4"]):
            r = run_program(args, tmp_path, dict(base, BLA_UNET_RESUME="1", **env))      # fit reads the file when it resumes
            assert r.returncode == 1, (args, env, r.stdout + r.stderr)
            assert "objective.txt" in r.stderr and "schedule=cosine predict=v min_snr=5" in r.stderr, (args, env, r.stderr)
    # options that agree with the file (5.0 is 5) pass this check: the program stops later, at the weights or records that are not there
    for env in ({}, {"BLA_UNET_PREDICT": "v"}, {"BLA_UNET_SCHEDULE": "cosine", "BLA_UNET_PREDICT": "v", "BLA_UNET_MIN_SNR": "5.0"}):
        for args in (["sample", "2", "out"], ["eval"]):
            r = run_program(args, tmp_path, dict(base, **env))
            assert r.returncode == 1 and "objective.txt" not in r.stderr and "cannot open" in r.stderr, (args, env, r.stderr)
    # the averaged set has a file of its own
    r = run_program(["eval"], tmp_path, dict(base, BLA_UNET_EVAL_EMA="1", BLA_UNET_PREDICT="v"))
    assert r.returncode == 1 and "ema/objective.txt" in r.stderr and "predict=x0" in r.stderr, r.stderr
    # a file that does not hold fit's line
    for text, named in (("schedule=cosine predict=v\n", "objective.txt"), ("", "objective.txt"), ("schedule=sigmoid predict=v min_snr=5\n", "BLA_UNET_SCHEDULE=sigmoid"),
                        ("schedule=cosine predict=v min_snr=-2\n", "BLA_UNET_MIN_SNR=-2")):
        (w / "objective.txt").write_text(text)
        r = run_program(["sample", "2", "out"], tmp_path, base)
        assert r.returncode == 1 and named in r.stderr, (text, r.stderr)
    assert not (tmp_path / "out").exists()
