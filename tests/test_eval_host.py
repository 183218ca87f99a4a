"""CPU side of the held-out evaluation (include/bla.h: bla_diffusion_vlb_terms_f32, bla_diffusion_prior_kl_f32, bla_diffusion_vlb_weights,
bla_diffusion_eval_timesteps): the float64 restatement of the variational bound of Ho et al. 2020 (eq. 5) that tests/test_eval_gpu.py holds the
device to, and tests that pin the restatement itself -- the eps form of the KL against its definition, the decoder's normalisation, the timestep
list, and that the GPU test's bounds tell the restatement from four near misses of it."""
import math

import numpy as np
import pytest

_erfc = np.frompyfunc(math.erfc, 1, 1)
RS2 = 0.70710678118654752440
EPS53 = 2.0 ** -53


def erfc(z):
    return np.asarray(_erfc(np.asarray(z, np.float64)), np.float64)


def linear_schedule(T, b0=1e-4, b1=0.02):
    """bla_diffusion_create's schedule, [T][2] = (beta_t, alpha_bar_t); the GPU tests take the library's own doubles instead"""
    b0, b1 = float(np.float32(b0)), float(np.float32(b1))
    out, ab = [], 1.0
    for t in range(T):
        b = b0 if T == 1 else b0 + (b1 - b0) * t / (T - 1)
        ab *= 1.0 - b
        out.append((b, ab))
    return np.array(out)


def vlb_weights(sched, t, w_from_posterior=False):
    """c_t, w_t for t >= 1, operation for operation what the library's host code does (python floats are IEEE doubles, math.log is libm's)"""
    b, ab, abp = float(sched[t, 0]), float(sched[t, 1]), float(sched[t - 1, 1])
    bt = b * (1.0 - abp) / (1.0 - ab)
    c = 0.5 * (math.log(b / bt) + bt / b - 1.0)
    w = (bt if w_from_posterior else b) / (2.0 * (1.0 - b) * (1.0 - ab))
    return c, w


def eval_timesteps(T, K):
    return [0] + [1 + ((T - 1) * (2 * i + 1)) // (2 * K) for i in range(K)]


def decoder_probs(x0, mu, sigma, edge=0.999, half=1.0 / 255.0):
    """p of every element under the discretised Gaussian decoder (Ho et al. 3.3), before the floor; Phi through erfc on its small side"""
    x0 = np.asarray(x0, np.float64)
    zp, zm = (x0 + half - mu) / sigma, (x0 - half - mu) / sigma
    lower = 0.5 * (erfc(-zp * RS2) - erfc(-zm * RS2))
    upper = 0.5 * (erfc(zm * RS2) - erfc(zp * RS2))
    p = np.where(zm > 0, upper, lower)
    p = np.where(x0 < -edge, 0.5 * erfc(-zp * RS2), p)
    return np.where(x0 > edge, 0.5 * erfc(zm * RS2), p)


def vlb_terms(sched, t, x0, xt, eps, eps_hat, floor=1e-12, edge=0.999, half=1.0 / 255.0, w_from_posterior=False):
    """One image [F] (fp32 inputs read as they are) at timestep t -> (term in nats, sqerr, the magnitude its GPU bound scales with)"""
    x0, xt, eps, eps_hat = (np.asarray(v, np.float64) for v in (x0, xt, eps, eps_hat))
    F = x0.size
    sqerr = math.fsum((eps - eps_hat) ** 2)
    if t >= 1:
        c, w = vlb_weights(sched, t, w_from_posterior)
        return F * c + w * sqerr, sqerr, F * abs(c) + w * sqerr
    b0, ab0 = float(sched[0, 0]), float(sched[0, 1])
    mu = (xt - b0 / math.sqrt(1.0 - ab0) * eps_hat) / math.sqrt(1.0 - b0)
    p = decoder_probs(x0, mu, math.sqrt(b0), edge, half)
    if floor is not None:
        p = np.maximum(p, floor)
    with np.errstate(divide="ignore"):
        lp = np.log(p)
    return -math.fsum(lp), sqerr, math.fsum(np.abs(lp))


def prior_kl(sched, x0):
    x0 = np.asarray(x0, np.float64)
    ab, F = float(sched[-1, 1]), x0.size
    s = math.fsum(x0 * x0)
    return 0.5 * (ab * s - F * ab - F * math.log(1.0 - ab)), ab * s + F * abs(math.log(1.0 - ab)) + F * ab


def term_bound(t, F, scale):
    """The GPU test's bound on |device - restatement| for a term: the order of F double additions at t >= 1; at t = 0 z carries ~1e-14 from the order of
    operations in mu, divided by sigma = 0.01, |d ln p / dz| <~ 7 down to the floor, a few ulp of erfc: ~1e-13 per element, three orders of slack"""
    return (4 * F * EPS53 if t >= 1 else 1e-10) * scale


TS5 = [0, 1, 2, 500, 999]


def vlb_inputs(sched, F, batch, s, ts=TS5):
    """Test 5's inputs: x0 on the pixel grid with -1 and 1 in every image, eps ~ N(0, 1) as fp32, x_t in fp32 at each image's t, eps_hat = eps + s noise"""
    rng = np.random.default_rng(1000 * F + 10 * batch + int(10 * s))
    pix = rng.integers(0, 256, (batch, F))
    pix[:, 0], pix[:, -1] = 0, 255
    x0 = ((pix - 127.5) / 127.5).astype(np.float32)
    eps = rng.standard_normal((batch, F)).astype(np.float32)
    t = np.array([ts[b % len(ts)] for b in range(batch)], np.int32)
    ab = sched[t, 1][:, None]
    xt = (np.sqrt(ab) * x0 + np.sqrt(1 - ab) * eps).astype(np.float32)
    eps_hat = (eps + np.float32(s) * rng.standard_normal((batch, F)).astype(np.float32)).astype(np.float32)
    return x0, xt, eps, eps_hat, t


# ---- 1: the eps form of the KL is the KL ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,t", [(1000, 1), (1000, 2), (1000, 500), (1000, 999), (2, 1)])
def test_kl_identity(T, t):
    sched = linear_schedule(T)
    F = 3072
    rng = np.random.default_rng(t)
    x0 = (rng.integers(0, 256, F) - 127.5) / 127.5
    eps = rng.standard_normal(F)
    eps_hat = eps + 0.3 * rng.standard_normal(F)
    b, ab, abp = sched[t, 0], sched[t, 1], sched[t - 1, 1]
    xt = math.sqrt(ab) * x0 + math.sqrt(1 - ab) * eps
    bt = b * (1 - abp) / (1 - ab)
    mean_q = math.sqrt(abp) * b / (1 - ab) * x0 + math.sqrt(1 - b) * (1 - abp) / (1 - ab) * xt        # Ho et al. eq. 7
    mean_p = (xt - b / math.sqrt(1 - ab) * eps_hat) / math.sqrt(1 - b)                                  # bla_diffusion_step_f32's mean
    kl = 0.5 * F * (math.log(b / bt) + bt / b - 1) + math.fsum((mean_q - mean_p) ** 2) / (2 * b)
    got, _, _ = vlb_terms(sched, t, x0, xt, eps, eps_hat)
    err = abs(got - kl) / abs(kl)
    print(f"T {T} t {t}: KL {kl:.6f}, eps form off by {err:.1e} relative")
    assert err <= 1e-10


# ---- 2: the decoder is a distribution over the 256 pixel values ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("lo,hi", [(-1.0, 1.0), (-6.0, -2.0), (2.0, 6.0)])
def test_decoder_normalisation(lo, hi):
    grid = (np.arange(256) - 127.5) / 127.5          # in double: rounded to fp32 the bins' edges no longer meet (2e-7 of the sum)
    worst = 0.0
    for mu in np.random.default_rng(5).uniform(lo, hi, 50):
        worst = max(worst, abs(math.fsum(decoder_probs(grid, mu, 0.01)) - 1.0))
    print(f"mu in [{lo}, {hi}]: |sum p - 1| <= {worst:.1e}")
    assert worst <= 1e-12


# ---- 3: the timestep list -----------------------------------------------------------------------------------------------------------------------------

def test_eval_timesteps():
    for T in (2, 20, 1000):
        for K in sorted({0, 1, min(T - 1, 2), min(T - 1, 50), T - 1}):
            ts = eval_timesteps(T, K)
            assert ts[0] == 0 and len(ts) == K + 1
            assert all(a < b for a, b in zip(ts, ts[1:])) and ts[-1] <= T - 1, (T, K)
        assert eval_timesteps(T, T - 1) == list(range(T))
        assert eval_timesteps(T, 0) == [0]


# ---- 4: the GPU test's bounds tell the restatement from its near misses ------------------------------------------------------------------------------

MUTATIONS = {"posterior variance in w_t": dict(w_from_posterior=True), "no floor": dict(floor=None), "edge rule at 0.99": dict(edge=0.99),
             "half-width 1/256": dict(half=1.0 / 256.0)}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
def test_mutations_leave_the_bounds(name):
    sched = linear_schedule(1000)
    caught = []
    for F in (3072, 37):
        for s in (0.0, 0.3, 3.0):
            x0, xt, eps, eps_hat, t = vlb_inputs(sched, F, 5, s)
            for b in range(5):
                want, _, scale = vlb_terms(sched, int(t[b]), x0[b], xt[b], eps[b], eps_hat[b])
                got, _, _ = vlb_terms(sched, int(t[b]), x0[b], xt[b], eps[b], eps_hat[b], **MUTATIONS[name])
                if not abs(got - want) <= term_bound(int(t[b]), F, scale):      # a NaN or an infinity leaves the bound too
                    caught.append((F, s, int(t[b])))
    print(f"{name}: outside the bound at (F, s, t) = {caught}")
    assert caught, name
