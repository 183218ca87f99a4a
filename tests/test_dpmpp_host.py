"""CPU side of DPM-Solver++(2M) sampling (include/bla.h: bla_diffusion_sample_timesteps, bla_diffusion_dpmpp_coefficients,
bla_diffusion_dpmpp_step_f32): the float64 restatement of the timestep spacing, the step coefficients and the step that tests/test_dpmpp_gpu.py
holds the device to, validated here without a device -- against DDIM, against the exact solution of a Gaussian model, against the values the
spacing rule must give, and, for the rounding bound the GPU tests use, against a float32 emulation of the kernel and four wrong kernels -- and
the example program's refusal of bad BLA_UNET_SAMPLER / BLA_UNET_SPACING settings before the device is opened."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from inputs import uniform
from test_ddim_gpu import ddim_ts, numpy_ddim

EX = os.path.join(ROOT, "examples")
BIN = os.path.join(EX, "cifar_unet_gpu")
TRAILING, LOGSNR = 0, 1
U = 2.0 ** -24


# ---- the float64 restatement ---------------------------------------------------------------------------------------------------------------

def schedule(T, b0=1e-4, b1=0.02):
    """bla_diffusion_create's doubles, [T][beta, alpha_bar] (what test_diffusion_gpu.diffusion reads back from the object)"""
    b0, b1 = float(np.float32(b0)), float(np.float32(b1))
    beta = np.array([b0 if T == 1 else b0 + (b1 - b0) * t / (T - 1) for t in range(T)])
    return np.stack([beta, np.cumprod(1.0 - beta)], axis=1)


def log_snr(sched):
    ab = sched[:, 1]
    return 0.5 * np.log(ab / (1.0 - ab))


def lam_diff(sched, a, b):
    """lambda_a - lambda_b as one logarithm of one ratio (no cancellation between two logarithms)"""
    xa, xb = sched[a, 1], sched[b, 1]
    return 0.5 * np.log((xa * (1.0 - xb)) / (xb * (1.0 - xa)))


def sample_ts(sched, S, spacing):
    T = len(sched)
    if spacing == TRAILING:
        return ddim_ts(T, S)
    if S == 1:
        return [T - 1]
    lam = log_snr(sched)
    out = []
    for i in range(S):
        g = lam[0] + (lam[T - 1] - lam[0]) * i / (S - 1)
        dist = np.abs(lam - g)
        out.append(int(np.argmin(dist)))                 # the first minimum: a tie takes the lower t
    for i in range(1, S):
        out[i] = max(out[i], out[i - 1] + 1)
    for i in range(S - 1, -1, -1):
        out[i] = min(out[i], T - 1 - (S - 1 - i))
    return out


def coefficients(sched, t_last, t, t_prev):
    """{inv_sab, s1m, c_x, c_d, w1, w0} in float64"""
    ab = sched[t, 1]
    c = [1.0 / np.sqrt(ab), np.sqrt(1.0 - ab), 0.0, 1.0, 1.0, 0.0]
    if t_prev >= 0:
        abp, h = sched[t_prev, 1], lam_diff(sched, t_prev, t)
        c[2] = np.sqrt(1.0 - abp) / np.sqrt(1.0 - ab)
        c[3] = -np.sqrt(abp) * np.expm1(-h)
        if t_last >= 0:
            r = lam_diff(sched, t, t_last) / h
            c[4], c[5] = 1.0 + 1.0 / (2.0 * r), -1.0 / (2.0 * r)
    return np.array(c, np.float64)


def second_order(t_last, t_prev):
    return t_last >= 0 and t_prev >= 0


def numpy_dpmpp(x, e, hist, c, clip, second):
    """the step in float64 on the inputs as they are: (new x, new hist, unclamped x0, D)"""
    x, e, hist = (np.asarray(v, np.float64) for v in (x, e, hist))
    x0u = (x - c[1] * e) * c[0]
    x0 = np.clip(x0u, -1, 1) if clip else x0u
    D = c[4] * x0 + c[5] * hist if second else x0
    return c[2] * x + c[3] * D, x0, x0u, D


def bounds(x, e, hist, c, clip, second):
    """B_x and B_h per element: one coefficient rounding and one result rounding (2^-24 relative each) per multiply or fmaf, the clamp
    1-Lipschitz, hist an exact fp32 input.  With u = 2^-24 and A = |x| + s1m |e|: x0 is off by at most 4 u inv_sab A (s1m, the fmaf, inv_sab, the
    product) = B_h; w1 x0 adds 2 u w1 |x0u| and the fmaf behind it u |D| <= u (w1 |x0u| + |w0 hist|) plus w0's own u |w0 hist|; c_d D adds
    2 u c_d |D| and the last fmaf u |c_x x + c_d D| beside c_x's u c_x |x|."""
    _, _, x0u, D = numpy_dpmpp(x, e, hist, c, clip, second)
    x, e, hist = (np.abs(np.asarray(v, np.float64)) for v in (x, e, hist))
    A = x + c[1] * e
    Bh = 4 * U * c[0] * A
    Bx = U * (c[3] * (c[4] * (4 * c[0] * A + 3 * np.abs(x0u)) + 2 * abs(c[5]) * hist + 3 * np.abs(D)) + 2 * c[2] * x)
    return Bx, Bh


def fmaf(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def f32_dpmpp(x, e, hist, c, clip, second, mutate=None):
    """the kernel's arithmetic in numpy float32 (every product and fmaf rounded once); `mutate` names one of the wrong kernels of
    test_rounding_bound_and_mutations"""
    c = np.asarray(c, np.float64).astype(np.float32)
    x, e, hist = (np.asarray(v, np.float32) for v in (x, e, hist))
    x0u = fmaf(-c[1], e, x) * c[0]
    x0 = np.clip(x0u, np.float32(-1), np.float32(1)) if clip else x0u
    w0 = -c[5] if mutate == "w0_sign" else c[5]
    D = fmaf(w0, hist, c[4] * x0) if second else x0
    return fmaf(c[2], x, c[3] * D), (x0u if mutate == "hist_before_clamp" else x0)


# the exact model of the issue: x0 ~ N(0, 0.25 I), so every sampler is a scalar gain on x_T

def v_of(ab):
    return 0.25 * ab + 1.0 - ab


def eps_star(x, sched, t):
    ab = sched[t, 1]
    return np.sqrt(1.0 - ab) * x / v_of(ab)


def exact_gain(sched):
    return np.sqrt(0.25 / v_of(sched[-1, 1]))


def gain_dpmpp(sched, S, spacing, first_order_only=False):
    ts = sample_ts(sched, S, spacing)
    x, hist, t_last = np.ones(1), np.zeros(1), -1
    for i in range(S - 1, -1, -1):
        t, t_prev = ts[i], ts[i - 1] if i else -1
        tl = -1 if first_order_only else t_last
        x, hist, _, _ = numpy_dpmpp(x, eps_star(x, sched, t), hist, coefficients(sched, tl, t, t_prev), 0, second_order(tl, t_prev))
        t_last = t
    return float(x[0])


def gain_ddim(sched, S):
    ts = ddim_ts(len(sched), S)
    x = np.ones(1)
    for i in range(S - 1, -1, -1):
        x = numpy_ddim(x, eps_star(x, sched, ts[i]), ts[i], ts[i - 1] if i else -1, 0.0, 0, sched, 0.0)
    return float(x[0])


# ---- 1: first order is DDIM ----------------------------------------------------------------------------------------------------------------

def test_first_order_is_ddim():
    """without clipping: a clamped x0 prediction enters DDIM's update beside the eps_hat it was given, and this solver's through the eps that the
    clamped prediction implies, so with clip the two differ wherever the clamp acts"""
    sched = schedule(1000)
    worst = 0.0
    for t, t_prev in ((999, 979), (431, 411), (49, 24), (999, 499)):
        x, e = uniform(3 + t, (225,), -2, 2, np.float32), uniform(4 + t, (225,), -2, 2, np.float32).astype(np.float64)
        got = numpy_dpmpp(x, e, np.zeros(225), coefficients(sched, -1, t, t_prev), 0, False)[0]
        want = numpy_ddim(x, e, t, t_prev, 0.0, 0, sched, 0.0)
        err = np.abs(got - want).max() / np.abs(want).max()
        worst = max(worst, err)
        assert err <= 1e-13, (t, t_prev, err)
    print(f"first-order step vs numpy_ddim at eta 0: worst {worst:.1e} of max |result|")


def test_lam_diff_against_extended_precision():
    """one logarithm of one ratio against lambda_a - lambda_b formed with 40 digits: 1e-14 relative at every kind of pair the tests use (the
    float64 difference of two logarithms loses ulp(lambda) / |difference| and is not)"""
    import decimal
    sched = schedule(1000)
    with decimal.localcontext() as ctx:
        ctx.prec = 40
        lam = [(decimal.Decimal(ab) / (1 - decimal.Decimal(ab))).ln() / 2 for ab in sched[:, 1]]
        for a, b in ((979, 999), (959, 979), (998, 999), (0, 1), (411, 431), (249, 499), (0, 999), (499, 500)):
            want = lam[a] - lam[b]
            assert abs(decimal.Decimal(float(lam_diff(sched, a, b))) - want) <= decimal.Decimal(1e-14) * abs(want), (a, b)


# ---- 2: solver order on the Gaussian model -----------------------------------------------------------------------------------------------

def test_solver_order_on_the_gaussian_model():
    sched = schedule(1000)
    exact = exact_gain(sched)
    ddim = {S: abs(gain_ddim(sched, S) - exact) for S in (5, 10, 20, 40, 80)}
    m_log = {S: abs(gain_dpmpp(sched, S, LOGSNR) - exact) for S in (5, 10, 20, 40)}
    m_trail = {S: abs(gain_dpmpp(sched, S, TRAILING) - exact) for S in (5, 10, 20, 40)}
    fmt = lambda d: ", ".join("S = %d: %.4f" % kv for kv in d.items())
    print("|gain - exact|  DDIM trailing: %s;  2M trailing: %s;  2M log-SNR: %s" % (fmt(ddim), fmt(m_trail), fmt(m_log)))
    assert m_log[10] < ddim[40]
    assert m_log[20] < ddim[80]
    assert m_trail[20] < ddim[40]
    for S in (5, 10, 20, 40):
        first = abs(gain_dpmpp(sched, S, TRAILING, first_order_only=True) - exact)
        assert abs(first - ddim[S]) <= 1e-12, (S, first, ddim[S])


# ---- 3: the spacing rule -----------------------------------------------------------------------------------------------------------------

def test_spacing_rule():
    sched = schedule(1000)
    assert sample_ts(sched, 1, LOGSNR) == [999]
    assert sample_ts(sched, 2, LOGSNR) == [0, 999]
    assert sample_ts(sched, 5, LOGSNR) == [0, 30, 302, 722, 999]
    assert sample_ts(sched, 10, LOGSNR)[:6] == [0, 5, 22, 73, 202, 410]
    assert sample_ts(sched, 1000, LOGSNR) == list(range(1000))
    for T, sizes in ((1000, (2, 3, 5, 10, 20, 50, 333, 999)), (50, (2, 7, 49, 50)), (7, (2, 6, 7)), (2, (1, 2)), (1, (1,))):
        s = schedule(T)
        assert (np.diff(log_snr(s)) < 0).all()
        for S in sizes:
            ts = sample_ts(s, S, LOGSNR)
            assert len(ts) == S and ts[-1] == T - 1 and (S < 2 or ts[0] == 0) and (np.diff(ts) > 0).all(), (T, S, ts)
            assert sample_ts(s, S, TRAILING) == ddim_ts(T, S)
    assert sample_ts(schedule(50), 50, LOGSNR) == list(range(50))


# ---- 4: the rounding bound -----------------------------------------------------------------------------------------------------------------

BOUND_CASES = [(-1, 999, 979), (999, 979, 959), (999, 499, 249), (-1, 999, -1), (451, 431, 411), (99, 49, -1), (3, 1, 0), (1, 0, -1),
               (999, 998, 997), (500, 250, 0), (-1, 1, 0), (20, 10, 5)]


def bound_inputs(t, n=225):
    return uniform(11 + t, (n,), -2, 2, np.float32), uniform(12 + t, (n,), -2, 2, np.float32), uniform(13 + t, (n,), -1, 1, np.float32)


def fractions(sched, t_last, t, t_prev, clip, mutate=None, c32=None, second=None):
    x, e, hist = bound_inputs(t)
    c = coefficients(sched, t_last, t, t_prev)
    sec = second_order(t_last, t_prev)
    want_x, want_h, _, _ = numpy_dpmpp(x, e, hist, c, clip, sec)
    Bx, Bh = bounds(x, e, hist, c, clip, sec)
    got_x, got_h = f32_dpmpp(x, e, hist, c if c32 is None else c32, clip, sec if second is None else second, mutate)
    return (np.abs(got_x - want_x) / Bx).max(), (np.abs(got_h - want_h) / Bh).max()


def test_rounding_bound_and_mutations():
    sched = schedule(1000)
    worst = np.zeros(2)
    for t_last, t, t_prev in BOUND_CASES:
        for clip in (0, 1):
            f = fractions(sched, t_last, t, t_prev, clip)
            worst = np.maximum(worst, f)
            assert f[0] <= 1 and f[1] <= 1, (t_last, t, t_prev, clip, f)
    print("float32 restatement vs float64: worst %.2f of B_x, %.2f of B_h" % tuple(worst))
    # four wrong kernels, each caught by the bound
    assert fractions(sched, 999, 979, 959, 0, mutate="w0_sign")[0] > 1
    assert fractions(sched, 999, 979, 959, 1, mutate="hist_before_clamp")[1] > 1
    c = coefficients(sched, 3, 1, 0)                                # c_d = alpha_p (1 - expf(-h)) formed in fp32 from the fp32 abar, at t = 1, where
    ab32 = sched[:2, 1].astype(np.float32)                          # 1 - abar_1 = 2.2e-4 keeps 12 of abar's 24 bits
    lam32 = np.float32(0.5) * np.log(ab32 / (np.float32(1) - ab32))
    bad = c.copy()
    bad[3] = np.sqrt(ab32[0]) * (np.float32(1) - np.exp(-(lam32[0] - lam32[1])))
    assert bad.dtype == np.float64 and lam32.dtype == np.float32
    f = fractions(sched, 3, 1, 0, 0, c32=bad)
    print("c_d from 1 - expf(-h) in fp32 at t = 1: relative error %.1e, %.2f of B_x" % (abs(bad[3] - c[3]) / c[3], f[0]))
    assert f[0] > 1
    bad = coefficients(sched, 99, 49, -1)                           # second order at t_prev = -1: the weights of a step to t = 0, c_x = 0, c_d = 1
    bad[4:] = coefficients(sched, 99, 49, 0)[4:]
    assert fractions(sched, 99, 49, -1, 0, c32=bad, second=True)[0] > 1


# ---- 5: the example program refuses bad options ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def prog(pkg):
    pkg.build_native()
    subprocess.check_call(["make", "-s", "-C", EX, "cifar_unet_gpu"])
    return BIN


SAMPLE_ENV = ("BLA_CIFAR_DIR", "BLA_UNET_WEIGHTS", "BLA_UNET_RESUME", "BLA_UNET_INIT", "BLA_SEED", "BLA_UNET_BATCH", "BLA_UNET_CLASSES", "BLA_UNET_CLASS",
              "BLA_UNET_SAMPLE_STEPS", "BLA_UNET_ETA", "BLA_UNET_CLIP", "BLA_UNET_EMA", "BLA_DIFFUSION_STEPS", "BLA_UNET_SAMPLER", "BLA_UNET_SPACING")


def run_example(args, cwd, env, timeout=120):
    e = dict(os.environ, **env)
    for k in SAMPLE_ENV:
        if k not in env:
            e.pop(k, None)
    return subprocess.run([BIN] + args, cwd=str(cwd), env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)


def test_sample_refuses_bad_sampler_options(prog, tmp_path):
    for env, named in (({"BLA_UNET_SAMPLER": "euler", "BLA_UNET_SAMPLE_STEPS": "5"}, "BLA_UNET_SAMPLER=euler"),
                       ({"BLA_UNET_SAMPLER": "DPMPP", "BLA_UNET_SAMPLE_STEPS": "5"}, "BLA_UNET_SAMPLER=DPMPP"),
                       ({"BLA_UNET_SAMPLER": "dpmpp", "BLA_UNET_SAMPLE_STEPS": "5", "BLA_UNET_SPACING": "uniform"}, "BLA_UNET_SPACING=uniform"),
                       ({"BLA_UNET_SAMPLER": "ddim", "BLA_UNET_SAMPLE_STEPS": "5", "BLA_UNET_SPACING": "x"}, "BLA_UNET_SPACING=x"),
                       ({"BLA_UNET_SAMPLER": "dpmpp"}, "BLA_UNET_SAMPLE_STEPS"),
                       ({"BLA_UNET_SAMPLER": "dpmpp", "BLA_UNET_SAMPLE_STEPS": "5", "BLA_UNET_ETA": "0.5"}, "BLA_UNET_ETA=0.5")):
        r = run_example(["sample", "2", str(tmp_path / "out")], tmp_path, env)
        assert r.returncode == 1, (env, r.stdout + r.stderr)
        assert named in r.stderr, (env, r.stderr)
        assert not (tmp_path / "out").exists()
