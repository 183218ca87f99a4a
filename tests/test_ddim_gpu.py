"""Few-step DDIM sampling (Song, Meng, Ermon 2021) and the exponential moving average of the weights on the device (include/bla.h: bla_ema_f32,
bla_diffusion_ddim_timesteps, bla_diffusion_ddim_step_f32, bla_diffusion_guided_ddim_step_f32, bla_unet_sample_ddim_f32,
bla_unet_sample_guided_ddim_f32) against numpy restatements, on the narrow U-Net configuration of tests/test_diffusion_gpu.py, and the example
program's `fit` with BLA_UNET_EMA / `sample` with BLA_UNET_SAMPLE_STEPS at full size."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from inputs import uniform
from test_diffusion_gpu import CFG, F, csv_files, diffusion, fetch, upload
from test_diffusion_host import time_embedding
from test_guidance_gpu import bmp_ok
from test_unet_model import build as unet_build, load_params

pytestmark = pytest.mark.gpu

EX = os.path.join(ROOT, "examples")
BIN = os.path.join(EX, "cifar_unet_gpu")
BLA_ERR_INVALID = 1
CLASSES = 10


@pytest.fixture(scope="module")
def L(pkg):
    pkg.init(0)
    return pkg.lib()


def chk(pkg, status):
    pkg.native.check(status)


def normal(pkg, L, n, seed, offset):
    z = pkg.empty((n,))
    chk(pkg, L.bla_rand_normal_f32(None, z.ptr, n, 0.0, 1.0, seed, offset))
    return z.numpy().astype(np.float64)


# ---- 1: the moving average ---------------------------------------------------------------------------------------------------------------------

def ema_want(e, p, decay):
    w = np.float32(1.0 - float(np.float32(decay)))       # formed in double from the float decay, rounded once
    return e + w * (p - e)                               # float32, every operation rounded


def test_ema_bit_equal(pkg, L):
    for n in (1, 3, 4097, 2 ** 20 + 5):
        e0, p = uniform(n % 97, (n,), -2, 2, np.float32), uniform(n % 89 + 100, (n,), -2, 2, np.float32)
        de, dp = pkg.empty((n + 4,)), pkg.empty((n + 4,))
        for me, mp in ((0, 0), (1, 1), (2, 2), (3, 3), (0, 3), (2, 1)):   # the same and different offsets of the two buckets, in floats
            upload(pkg, dp.ptr + 4 * mp, p)
            for decay in (0.9999, 0.9, 0.5, 0.0):
                upload(pkg, de.ptr + 4 * me, e0)
                chk(pkg, L.bla_ema_f32(None, de.ptr + 4 * me, dp.ptr + 4 * mp, n, decay))
                assert np.array_equal(fetch(pkg, de.ptr + 4 * me, n, np.float32), ema_want(e0, p, decay)), (n, me, mp, decay)
            upload(pkg, de.ptr + 4 * me, e0)
            chk(pkg, L.bla_ema_f32(None, de.ptr + 4 * me, dp.ptr + 4 * mp, n, 1.0))   # decay 1: e kept bit for bit
            assert np.array_equal(fetch(pkg, de.ptr + 4 * me, n, np.float32), e0), (n, me, mp)
        upload(pkg, dp.ptr, e0); upload(pkg, de.ptr, e0)                              # p == e stays as it is
        chk(pkg, L.bla_ema_f32(None, de.ptr, dp.ptr, n, 0.9))
        assert np.array_equal(fetch(pkg, de.ptr, n, np.float32), e0), n


def test_ema_refuses_bad_decays(pkg, L):
    e, p = pkg.to_device(np.ones(8, np.float32)), pkg.to_device(np.zeros(8, np.float32))
    for bad in (-0.1, 1.5, float("nan"), float("inf"), -float("inf")):
        assert L.bla_ema_f32(None, e.ptr, p.ptr, 8, bad) == BLA_ERR_INVALID, bad
    chk(pkg, L.bla_ema_f32(None, e.ptr, p.ptr, 0, 0.5))                                # n = 0: nothing
    assert (e.numpy() == 1).all()


# ---- 2: the timesteps ------------------------------------------------------------------------------------------------------------------------

def ddim_ts(T, S):
    return [T * (i + 1) // S - 1 for i in range(S)]


def timesteps(pkg, L, d, S):
    out = np.full(max(S, 1), -7, np.int32)
    return L.bla_diffusion_ddim_timesteps(d, S, out.ctypes.data), out


def test_ddim_timesteps(pkg, L):
    for T in (1, 7, 50, 1000):
        d, _ = diffusion(pkg, L, T)
        for S in sorted({min(s, T) for s in (1, 2, 3, max(T // 3, 1), max(T - 1, 1), T)}):
            st, got = timesteps(pkg, L, d, S)
            assert st == 0 and got.tolist() == ddim_ts(T, S), (T, S)
            assert got[-1] == T - 1 and (np.diff(got) > 0).all()
        assert timesteps(pkg, L, d, T)[1].tolist() == list(range(T))
        assert timesteps(pkg, L, d, 1)[1].tolist() == [T - 1]
        for S in (0, -1, T + 1):
            st, out = timesteps(pkg, L, d, S)
            assert st == BLA_ERR_INVALID and (out == -7).all(), (T, S)
        chk(pkg, L.bla_diffusion_destroy(d))


# ---- 3: the step against float64 -------------------------------------------------------------------------------------------------------------

def numpy_ddim(x, e, t, t_prev, eta, clip, sched, z):
    ab = sched[t, 1]
    abp = sched[t_prev, 1] if t_prev >= 0 else 1.0
    sig = eta * np.sqrt((1 - abp) / (1 - ab)) * np.sqrt(1 - ab / abp)
    x0 = (x.astype(np.float64) - np.sqrt(1 - ab) * e) / np.sqrt(ab)
    if clip:
        x0 = np.clip(x0, -1, 1)
    return np.sqrt(abp) * x0 + np.sqrt(max(0.0, 1 - abp - sig * sig)) * e + sig * z


def step_error(got, x, e, t, t_prev, sched, want):
    """|got - want| over the scale an fp32 step can be held to: x0^ = (x - sqrt(1 - abar_t) e) / sqrt(abar_t) cancels terms of size
    |x| + sqrt(1 - abar_t) |e| and multiplies their rounding (2^-24 of them) by sqrt(abar_p / abar_t) on the way to the result -- 156 at
    t = 999, t_prev = -1 -- so a last-place error there is 4e-6 of that product where clipping keeps the result itself at |.| <= 1.
    Returned as a multiple of 4e-6 max(1, max |want|) + 1e-7 sqrt(abar_p / abar_t) max(|x| + sqrt(1 - abar_t) |e|): <= 1 passes."""
    ab = sched[t, 1]
    abp = sched[t_prev, 1] if t_prev >= 0 else 1.0
    terms = np.abs(x.astype(np.float64)) + np.sqrt(1 - ab) * np.abs(e)
    scale = 4e-6 * max(1.0, np.abs(want).max()) + 1e-7 * np.sqrt(abp / ab) * terms.max()
    return np.abs(got - want).max() / scale


STEP_CASES = [(999, 979), (999, 499), (999, -1), (431, 411), (431, -1), (0, -1)]


def test_ddim_step(pkg, L):
    T, B, dim, seed = 1000, 3, 24, 77
    d, sched = diffusion(pkg, L, T)
    worst = {}
    for t, t_prev in STEP_CASES:
        x = uniform(31 + t, (B, F), -2, 2, np.float32); e = uniform(32 + t, (B, F), -2, 2, np.float32)
        z = normal(pkg, L, B * F, seed, (t + 1) << 32).reshape(B, F)
        de = pkg.to_device(e)
        for eta in (0.0, 0.5, 1.0):
            for clip in (0, 1):
                dx, tn = pkg.to_device(x), pkg.to_device(np.full((B, dim), -7, np.float32))
                chk(pkg, L.bla_diffusion_ddim_step_f32(d, None, dx.ptr, de.ptr, B, F, t, t_prev, eta, clip, seed, dim, tn.ptr))
                want = numpy_ddim(x, e.astype(np.float64), t, t_prev, eta, clip, sched, z)
                err = step_error(dx.numpy(), x, e, t, t_prev, sched, want)
                worst[(t, t_prev, eta, clip)] = err
                assert err <= 1, (t, t_prev, eta, clip, err)
                if t_prev >= 0:
                    assert np.abs(tn.numpy() - np.stack([time_embedding(t_prev, dim)] * B)).max() <= 1e-6
                else:
                    assert (tn.numpy() == -7).all()
    print("DDIM step vs float64, worst error as a fraction of step_error's bound: %.2f; by (t, t_prev): %s" % (max(worst.values()), ", ".join(
        "%s %.2f" % (k, max(v for kk, v in worst.items() if kk[:2] == k)) for k in STEP_CASES)))
    # refused: t outside [0, T), t_prev outside [-1, t), eta outside [0, 1] or not finite
    dx = pkg.to_device(np.zeros((B, F), np.float32))
    for t, t_prev, eta in ((T, 10, 0.0), (-1, -1, 0.0), (10, 10, 0.0), (10, 11, 0.0), (10, -2, 0.0), (10, 5, -0.1), (10, 5, 1.5), (10, 5, float("nan"))):
        assert L.bla_diffusion_ddim_step_f32(d, None, dx.ptr, de.ptr, B, F, t, t_prev, eta, 0, seed, dim, None) == BLA_ERR_INVALID, (t, t_prev, eta)
    chk(pkg, L.bla_diffusion_destroy(d))


def test_ddim_noise_only_when_sigma_positive(pkg, L):
    """eta = 0 gives the same x whatever the seed; eta > 0 draws z from (seed, (t + 1) << 32)"""
    T, B, dim = 1000, 2, 24
    d, _ = diffusion(pkg, L, T)
    x = uniform(5, (B, F), -1, 1, np.float32); de = pkg.to_device(uniform(6, (B, F), -1, 1, np.float32))
    out = {}
    for seed in (1, 2):
        for eta in (0.0, 1.0):
            dx = pkg.to_device(x)
            chk(pkg, L.bla_diffusion_ddim_step_f32(d, None, dx.ptr, de.ptr, B, F, 500, 480, eta, 0, seed, dim, None))
            out[seed, eta] = dx.numpy()
    assert np.array_equal(out[1, 0.0], out[2, 0.0]) and not np.array_equal(out[1, 1.0], out[2, 1.0])
    chk(pkg, L.bla_diffusion_destroy(d))


# ---- 4: exact-eps recovery ---------------------------------------------------------------------------------------------------------------------

def test_ddim_recovers_x0_from_the_exact_noise(pkg, L):
    """x_T = sqrt(abar_{T-1}) x0 + sqrt(1 - abar_{T-1}) eps and the same eps fed to every eta = 0 step: each x0^ is x0 again in exact arithmetic,
    so x ends at x0.  In fp32 the first x0^ cancels sqrt(abar_{T-1}) x0 (|.| <= 0.006) out of x_T (|.| ~ 2) and divides the rounding of x_T and of
    the coefficients (~1e-7 of 2) by sqrt(abar_{T-1}) = 0.0064: ~3e-5 in x0^, carried unchanged to the end (each later step hands its x0^ error on
    times sqrt(abar_p) / sqrt(abar_p)) plus the same kind of rounding at every step whose abar is small; at S = T those add up over the last ~100
    steps.  Measured on an MI355X: 1.8e-5 (S = 1), 2.2e-5 (S = 10), 1.8e-4 (S = T); the bounds keep a margin of 2x or more."""
    T, B = 1000, 2
    d, sched = diffusion(pkg, L, T)
    x0 = uniform(5, (B, F), -0.9, 0.9, np.float32).astype(np.float64)
    eps = uniform(6, (B, F), -2, 2, np.float32)
    ab = sched[T - 1, 1]
    xT = (np.sqrt(ab) * x0 + np.sqrt(1 - ab) * eps.astype(np.float64)).astype(np.float32)
    de = pkg.to_device(eps)
    errs = {}
    for S, bound in ((1, 6e-5), (10, 6e-5), (T, 4e-4)):
        ts = ddim_ts(T, S)
        dx = pkg.to_device(xT)
        for i in range(S - 1, -1, -1):
            chk(pkg, L.bla_diffusion_ddim_step_f32(d, None, dx.ptr, de.ptr, B, F, ts[i], ts[i - 1] if i else -1, 0.0, 0, 7, 24, None))
        errs[S] = np.abs(dx.numpy() - x0).max()
        assert errs[S] <= bound, (S, errs[S])
    print("exact-eps recovery, max |x - x0|: " + ", ".join("S = %d: %.2e" % kv for kv in errs.items()))
    chk(pkg, L.bla_diffusion_destroy(d))


# ---- 5: the guided step ----------------------------------------------------------------------------------------------------------------------

def test_guided_ddim_step(pkg, L):
    T, B, dim, seed = 1000, 3, 24, 77
    d, sched = diffusion(pkg, L, T)
    table = uniform(91, (CLASSES + 1, dim), -1, 1, np.float32)
    rows = np.array([3, 10, 7, 10, 10, 10], np.int32)
    dtab, drows = pkg.to_device(table), pkg.to_device(rows, np.int32)
    for t, t_prev in ((999, 949), (431, 381), (431, -1), (0, -1)):
        x = uniform(41 + t, (B, F), -2, 2, np.float32)
        ec = uniform(43 + t, (B, F), -2, 2, np.float32); eu = uniform(44 + t, (B, F), -2, 2, np.float32)
        z = normal(pkg, L, B * F, seed, (t + 1) << 32).reshape(B, F)
        dec, deu = pkg.to_device(ec), pkg.to_device(eu)
        for s, eta, clip in ((0.0, 0.0, 0), (0.0, 1.0, 1), (3.0, 0.5, 0), (3.0, 1.0, 1)):
            dx, dcopy, tn = pkg.to_device(x), pkg.to_device(np.zeros((B, F), np.float32)), pkg.to_device(np.full((2 * B, dim), -7, np.float32))
            chk(pkg, L.bla_diffusion_guided_ddim_step_f32(d, None, dx.ptr, dcopy.ptr, dec.ptr, deu.ptr, s, B, F, t, t_prev, eta, clip, seed, dim, tn.ptr,
                                                          dtab.ptr, CLASSES, drows.ptr))
            got = dx.numpy()
            e = eu.astype(np.float64) + s * (ec.astype(np.float64) - eu.astype(np.float64))
            want = numpy_ddim(x, e, t, t_prev, eta, clip, sched, z)
            assert step_error(got, x, e, t, t_prev, sched, want) <= 1, (t, t_prev, s, eta, clip)
            assert np.array_equal(dcopy.numpy(), got)
            if t_prev >= 0:
                emb = np.stack([time_embedding(t_prev, dim)] * (2 * B))
                assert np.abs(tn.numpy() - (emb + table[rows])).max() <= 2e-6, (t, t_prev)
            else:
                assert (tn.numpy() == -7).all()
            if s == 0.0:                                 # the unguided DDIM step on eps_u, bit for bit
                ref = pkg.to_device(x)
                chk(pkg, L.bla_diffusion_ddim_step_f32(d, None, ref.ptr, deu.ptr, B, F, t, t_prev, eta, clip, seed, dim, None))
                assert np.array_equal(ref.numpy(), got), (t, t_prev, eta, clip)
    chk(pkg, L.bla_diffusion_destroy(d))


# ---- 6: the samplers -------------------------------------------------------------------------------------------------------------------------

def test_ddim_sampler(pkg, L):
    B, T, S, dim = 3, 20, 5, CFG["time_dim"]
    h, tensors = unet_build(pkg, CFG, B)
    load_params(pkg, h, tensors, CFG)
    d, sched = diffusion(pkg, L, T)
    ts = ddim_ts(T, S)
    x = pkg.empty((B, F))

    def sample(seed, eta, clip=0, x_seed=None):
        chk(pkg, L.bla_rand_normal_f32(None, x.ptr, B * F, 0.0, 1.0, seed if x_seed is None else x_seed, 0))
        chk(pkg, L.bla_unet_sample_ddim_f32(h, d, None, x.ptr, S, eta, clip, seed))
        return x.numpy()

    got = sample(5, 0.5, 1)
    assert np.isfinite(got).all()
    assert np.array_equal(sample(5, 0.5, 1), got)
    assert not np.array_equal(sample(6, 0.5, 1), got)
    assert np.array_equal(sample(6, 0.0, x_seed=5), sample(5, 0.0))          # eta = 0: nothing but x_T matters
    assert not np.array_equal(sample(6, 1.0, x_seed=5), sample(5, 1.0))
    # the same loop composed from the public pieces: bit-equal.  Each step also against numpy on the x and eps_hat it was given: carrying a numpy
    # x from step to step instead measures the test network more than the step (measured on an MI355X: 2.4e-4 at max |x_0| = 1 after the 5 steps
    # here, 7e-3 guided at s = 3, where each step on its own is within 1e-5)
    temb = pkg.empty((B, dim))
    worst = 0.0
    for eta, clip in ((0.5, 1), (0.0, 0)):
        want = sample(5, eta, clip)
        chk(pkg, L.bla_rand_normal_f32(None, x.ptr, B * F, 0.0, 1.0, 5, 0))
        chk(pkg, L.bla_time_embedding_f32(None, pkg.to_device(np.full(B, ts[-1], np.int32), np.int32).ptr, B, dim, temb.ptr))
        for i in range(S - 1, -1, -1):
            t, t_prev = ts[i], ts[i - 1] if i else -1
            assert np.abs(temb.numpy() - np.stack([time_embedding(t, dim)] * B)).max() <= 1e-6, (t, eta)
            chk(pkg, L.bla_unet_forward_f32(h, None, x.ptr, temb.ptr, None))
            xb = x.numpy().copy()
            eps_hat = fetch(pkg, L.bla_unet_output(h), B * F, np.float32).reshape(B, F).astype(np.float64)
            chk(pkg, L.bla_diffusion_ddim_step_f32(d, None, x.ptr, L.bla_unet_output(h), B, F, t, t_prev, eta, clip, 5, dim, temb.ptr))
            ref = numpy_ddim(xb, eps_hat, t, t_prev, eta, clip, sched, normal(pkg, L, B * F, 5, (t + 1) << 32).reshape(B, F))
            worst = max(worst, step_error(x.numpy(), xb, eps_hat, t, t_prev, sched, ref))
        assert np.array_equal(x.numpy(), want), (eta, clip)
    print(f"DDIM sampler steps vs numpy on the same x and eps_hat: worst {worst:.2f} of step_error's bound")
    assert worst <= 1, worst
    # refused: S outside [1, T], eta outside [0, 1]
    for s_bad, eta in ((0, 0.0), (T + 1, 0.0), (S, -0.5), (S, 2.0)):
        assert L.bla_unet_sample_ddim_f32(h, d, None, x.ptr, s_bad, eta, 0, 5) == BLA_ERR_INVALID, (s_bad, eta)
    chk(pkg, L.bla_diffusion_destroy(d)); chk(pkg, L.bla_unet_destroy(h))


def test_guided_ddim_sampler(pkg, L):
    n, T, S, dim, s = 2, 20, 5, CFG["time_dim"], 3.0
    h, tensors = unet_build(pkg, CFG, 2 * n)
    load_params(pkg, h, tensors, CFG)
    d, sched = diffusion(pkg, L, T)
    ts = ddim_ts(T, S)
    table = uniform(95, (CLASSES + 1, dim), -0.5, 0.5, np.float32)
    dtab = pkg.to_device(table)
    x = pkg.empty((n, F))

    def sample(seed, labels, eta, host=False, x_seed=None):
        lab = np.array(labels, np.int32)
        dlab = pkg.to_device(lab, np.int32)
        chk(pkg, L.bla_rand_normal_f32(None, x.ptr, n * F, 0.0, 1.0, seed if x_seed is None else x_seed, 0))
        chk(pkg, L.bla_unet_sample_guided_ddim_f32(h, d, None, x.ptr, dtab.ptr, CLASSES, lab.ctypes.data if host else dlab.ptr, s, S, eta, 1, seed))
        return x.numpy()

    got = sample(5, [3, 7], 0.5)
    assert np.isfinite(got).all()
    assert np.array_equal(sample(5, [3, 7], 0.5), got)
    assert np.array_equal(sample(5, [3, 7], 0.5, host=True), got)
    assert not np.array_equal(sample(6, [3, 7], 0.5), got)
    assert not np.array_equal(sample(5, [5, 7], 0.5)[0], got[0])
    assert np.array_equal(sample(6, [3, 7], 0.0, x_seed=5), sample(5, [3, 7], 0.0))
    # composed from the public pieces as in test_guided_sampler: bit-equal
    x2, temb, rows = pkg.empty((2 * n, F)), pkg.empty((2 * n, dim)), pkg.empty((2 * n,), np.int32)
    chk(pkg, L.bla_rand_normal_f32(None, x2.ptr, n * F, 0.0, 1.0, 5, 0))
    chk(pkg, L.bla_rand_normal_f32(None, x2.ptr + 4 * n * F, n * F, 0.0, 1.0, 5, 0))
    dts, dl2 = pkg.to_device(np.full(2 * n, ts[-1], np.int32), np.int32), pkg.to_device(np.array([3, 7, CLASSES, CLASSES], np.int32), np.int32)
    chk(pkg, L.bla_time_embedding_f32(None, dts.ptr, 2 * n, dim, temb.ptr))
    chk(pkg, L.bla_class_embedding_f32(None, dtab.ptr, CLASSES, dl2.ptr, 2 * n, dim, 0.0, 0, 0, rows.ptr, temb.ptr))
    out = L.bla_unet_output(h)
    crow = table[[3, 7, CLASSES, CLASSES]]
    worst = 0.0
    for i in range(S - 1, -1, -1):                       # each step also against numpy (the mix and the step) on the x and outputs it was given
        t, t_prev = ts[i], ts[i - 1] if i else -1
        assert np.abs(temb.numpy() - (np.stack([time_embedding(t, dim)] * (2 * n)) + crow)).max() <= 2e-6, t
        chk(pkg, L.bla_unet_forward_f32(h, None, x2.ptr, temb.ptr, None))
        xb = x2.numpy()[:n].copy()
        o = fetch(pkg, out, 2 * n * F, np.float32).reshape(2 * n, F).astype(np.float64)
        chk(pkg, L.bla_diffusion_guided_ddim_step_f32(d, None, x2.ptr, x2.ptr + 4 * n * F, out, out + 4 * n * F, s, n, F, t, t_prev, 0.5, 1, 5, dim, temb.ptr,
                                                      dtab.ptr, CLASSES, rows.ptr))
        e = o[n:] + s * (o[:n] - o[n:])
        ref = numpy_ddim(xb, e, t, t_prev, 0.5, 1, sched, normal(pkg, L, n * F, 5, (t + 1) << 32).reshape(n, F))
        after = x2.numpy()
        assert np.array_equal(after[:n], after[n:])
        worst = max(worst, step_error(after[:n], xb, e, t, t_prev, sched, ref))
    assert np.array_equal(x2.numpy()[:n], got)
    print(f"guided DDIM sampler steps vs numpy on the same x and outputs: worst {worst:.2f} of step_error's bound")
    assert worst <= 1, worst
    # a device label outside [0, classes] cannot be refused without a round trip: its image is sampled with no class row -- the composed loop at row -1
    want = sample(5, [3, CLASSES + 5], 0.5)
    chk(pkg, L.bla_rand_normal_f32(None, x2.ptr, n * F, 0.0, 1.0, 5, 0))
    chk(pkg, L.bla_rand_normal_f32(None, x2.ptr + 4 * n * F, n * F, 0.0, 1.0, 5, 0))
    chk(pkg, L.bla_time_embedding_f32(None, dts.ptr, 2 * n, dim, temb.ptr))
    dl2 = pkg.to_device(np.array([3, CLASSES + 5, CLASSES, CLASSES], np.int32), np.int32)
    chk(pkg, L.bla_class_embedding_f32(None, dtab.ptr, CLASSES, dl2.ptr, 2 * n, dim, 0.0, 0, 0, rows.ptr, temb.ptr))
    assert rows.numpy().tolist() == [3, -1, CLASSES, CLASSES]
    for i in range(S - 1, -1, -1):
        chk(pkg, L.bla_unet_forward_f32(h, None, x2.ptr, temb.ptr, None))
        chk(pkg, L.bla_diffusion_guided_ddim_step_f32(d, None, x2.ptr, x2.ptr + 4 * n * F, out, out + 4 * n * F, s, n, F, ts[i], ts[i - 1] if i else -1, 0.5, 1, 5, dim,
                                                      temb.ptr, dtab.ptr, CLASSES, rows.ptr))
    assert np.array_equal(x2.numpy()[:n], want)
    # a host label outside [0, classes] is refused before anything touches x
    chk(pkg, L.bla_rand_normal_f32(None, x.ptr, n * F, 0.0, 1.0, 5, 0))
    before = x.numpy()
    for bad in ([3, CLASSES + 1], [-1, 7]):
        lab = np.array(bad, np.int32)
        assert L.bla_unet_sample_guided_ddim_f32(h, d, None, x.ptr, dtab.ptr, CLASSES, lab.ctypes.data, s, S, 0.5, 1, 5) == BLA_ERR_INVALID, bad
        assert np.array_equal(x.numpy(), before), bad
    for s_bad in (0, T + 1):
        assert L.bla_unet_sample_guided_ddim_f32(h, d, None, x.ptr, dtab.ptr, CLASSES, pkg.to_device(np.array([1, 2], np.int32), np.int32).ptr, s, s_bad, 0.0, 0,
                                                 5) == BLA_ERR_INVALID
    chk(pkg, L.bla_diffusion_destroy(d)); chk(pkg, L.bla_unet_destroy(h))
    # an odd model batch has no halves
    h3, _ = unet_build(pkg, CFG, 3)
    d, _ = diffusion(pkg, L, T)
    d1 = pkg.to_device(np.array([1], np.int32), np.int32)
    assert L.bla_unet_sample_guided_ddim_f32(h3, d, None, x.ptr, dtab.ptr, CLASSES, d1.ptr, s, S, 0.0, 0, 5) == BLA_ERR_INVALID
    chk(pkg, L.bla_diffusion_destroy(d)); chk(pkg, L.bla_unet_destroy(h3))


# ---- 7: the example program ---------------------------------------------------------------------------------------------------------------

def run(args, cwd, env):
    e = dict(os.environ, **env)
    for k in ("BLA_CIFAR_DIR", "BLA_UNET_WEIGHTS", "BLA_UNET_RESUME", "BLA_UNET_INIT", "BLA_SEED", "BLA_UNET_BATCH", "BLA_UNET_CLASSES", "BLA_UNET_CLASS",
              "BLA_UNET_SAMPLE_STEPS", "BLA_UNET_ETA", "BLA_UNET_CLIP", "BLA_UNET_EMA", "BLA_DIFFUSION_STEPS"):
        if k not in env:
            e.pop(k, None)
    r = subprocess.run([BIN] + args, cwd=str(cwd), env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def test_example_fit_with_ema_and_ddim_sample(pkg, tmp_path):
    pkg.build_native()
    subprocess.check_call(["make", "-s", "-C", EX, "cifar_unet_gpu"])
    (tmp_path / "data" / "cifar").mkdir(parents=True)
    recs = np.random.default_rng(13).integers(0, 256, (16, 3073), dtype=np.uint8)
    recs[:, 0] = np.arange(16) % 10
    recs.tofile(tmp_path / "data" / "cifar" / "data_batch_1.bin")
    fit = {"BLA_DIFFUSION_STEPS": "50"}
    run(["fit", "1", "4"], tmp_path, dict(fit, BLA_UNET_WEIGHTS=str(tmp_path / "plain")))
    run(["fit", "1", "4"], tmp_path, dict(fit, BLA_UNET_WEIGHTS=str(tmp_path / "w"), BLA_UNET_EMA="0.999"))
    plain, both = csv_files(tmp_path / "plain"), csv_files(tmp_path / "w")
    main = {k: v for k, v in both.items() if not k.startswith("ema" + os.sep)}
    ema = {k[4:]: v for k, v in both.items() if k.startswith("ema" + os.sep)}
    assert len(plain) == 122 and main == plain                                 # the EMA changes nothing of the main set
    assert set(ema) == set(plain)
    changed = sum(ema[k] != plain[k] for k in plain)
    print(f"ema/: {changed} of 122 files differ from the main set")
    assert changed >= 100, changed                                             # the tensors the network does not use are the main set's
    # conditional: the class table's average too
    run(["fit", "1", "4"], tmp_path, dict(fit, BLA_UNET_WEIGHTS=str(tmp_path / "c"), BLA_UNET_EMA="0.999", BLA_UNET_CLASSES="1"))
    cond = csv_files(tmp_path / "c")
    assert len(cond) == 2 * 123 and os.path.join("ema", "class_embedding.csv") in cond
    assert cond[os.path.join("ema", "class_embedding.csv")] != cond["class_embedding.csv"]

    def sample(weights, out, **env):
        run(["sample", "2", str(tmp_path / out)], tmp_path, dict({"BLA_DIFFUSION_STEPS": "50", "BLA_UNET_WEIGHTS": str(weights), "BLA_UNET_SAMPLE_STEPS": "5"}, **env))
        assert sorted(os.listdir(tmp_path / out)) == ["sample_0000.bmp", "sample_0001.bmp"]
        return [open(tmp_path / out / f"sample_{i:04d}.bmp", "rb").read() for i in range(2)]

    a, b = sample(tmp_path / "w" / "ema", "s_a"), sample(tmp_path / "w" / "ema", "s_b")
    c = sample(tmp_path / "w" / "ema", "s_eta1", BLA_UNET_ETA="1")
    assert all(bmp_ok(v) for v in a + c)
    assert a == b and a != c
    g = sample(tmp_path / "c" / "ema", "s_guided", BLA_UNET_CLASS="3", BLA_UNET_CLIP="1")
    assert all(bmp_ok(v) for v in g)
