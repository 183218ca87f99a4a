"""DPM-Solver++(2M) sampling on the device (include/bla.h: bla_diffusion_sample_timesteps, bla_diffusion_dpmpp_coefficients,
bla_diffusion_dpmpp_step_f32, bla_diffusion_guided_dpmpp_step_f32, bla_unet_sample_dpmpp_f32, bla_unet_sample_guided_dpmpp_f32) against the
float64 restatement and the rounding bound that tests/test_dpmpp_host.py validates, on the smallest shapes that reach every path of the step
kernel (16-byte body, scalar tail, all-scalar for a misaligned pointer), and the example program's `sample` with BLA_UNET_SAMPLER=dpmpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from inputs import uniform
from test_ddim_gpu import ddim_ts
from test_diffusion_gpu import CFG, F as UNET_F, diffusion, fetch, upload
from test_diffusion_host import time_embedding
from test_dpmpp_host import (LOGSNR, TRAILING, bounds, coefficients, eps_star, exact_gain, fmaf, numpy_dpmpp, run_example, sample_ts, schedule,
                             second_order)
from test_guidance_gpu import bmp_ok
from test_unet_model import build as unet_build, load_params

pytestmark = pytest.mark.gpu

EX = os.path.join(ROOT, "examples")
BLA_ERR_INVALID = 1
CLASSES = 10
T, B, DIM = 1000, 3, 24
GUARD = 4
CASES = [(-1, 999, 979), (999, 979, 959), (999, 499, 249), (-1, 999, -1), (451, 431, 411), (99, 49, -1), (3, 1, 0), (1, 0, -1)]
SHAPES = [(75, 0), (48, 0), (75, 1)]          # (F, offset of d_x in floats): body + tail, body only, all scalar


@pytest.fixture(scope="module")
def L(pkg):
    pkg.init(0)
    return pkg.lib()


@pytest.fixture(scope="module")
def dif(pkg, L):
    d, sched = diffusion(pkg, L, T)
    assert np.array_equal(sched, schedule(T))            # the host restatement of the schedule is the object's, bit for bit
    yield d, sched
    chk(pkg, L.bla_diffusion_destroy(d))


def chk(pkg, status):
    pkg.native.check(status)


class Guarded:
    """a device array of n elements `offset` elements into its buffer, with GUARD elements of -7 behind it"""

    def __init__(self, pkg, a, offset=0):
        a = np.ascontiguousarray(a)
        self.pkg, self.n, self.dtype, self.shape = pkg, a.size, a.dtype, a.shape
        self.buf = pkg.empty((offset + a.size + GUARD,), a.dtype)
        self.ptr = self.buf.ptr + a.itemsize * offset
        upload(pkg, self.ptr, np.concatenate([a.ravel(), np.full(GUARD, -7, a.dtype)]))

    def numpy(self):
        got = fetch(self.pkg, self.ptr, self.n + GUARD, self.dtype)
        assert (got[self.n:] == -7).all(), "wrote behind the end"
        return got[:self.n].reshape(self.shape)


# ---- 1: timesteps and coefficients -------------------------------------------------------------------------------------------------------

def device_ts(L, d, S, spacing):
    out = np.full(max(S, 1), -7, np.int32)
    return L.bla_diffusion_sample_timesteps(d, S, spacing, out.ctypes.data), out


def test_sample_timesteps(pkg, L):
    for steps in (1, 2, 7, 50, 1000):
        d, sched = diffusion(pkg, L, steps)
        for S in sorted({min(s, steps) for s in (1, 2, 3, 5, 10, 20, max(steps // 3, 1), max(steps - 1, 1), steps)}):
            for spacing in (TRAILING, LOGSNR):
                st, got = device_ts(L, d, S, spacing)
                assert st == 0 and got.tolist() == sample_ts(sched, S, spacing), (steps, S, spacing, got)
                assert got[-1] == steps - 1 and (np.diff(got) > 0).all()
            ddim = np.zeros(S, np.int32)
            chk(pkg, L.bla_diffusion_ddim_timesteps(d, S, ddim.ctypes.data))
            assert np.array_equal(device_ts(L, d, S, TRAILING)[1], ddim)
        for S, spacing in ((0, LOGSNR), (-1, TRAILING), (steps + 1, LOGSNR), (steps + 1, TRAILING), (1, 7), (1, -1), (1, 2)):
            st, out = device_ts(L, d, S, spacing)
            assert st == BLA_ERR_INVALID and (out == -7).all(), (steps, S, spacing)
        chk(pkg, L.bla_diffusion_destroy(d))
    d, _ = diffusion(pkg, L, 1000)
    assert device_ts(L, d, 5, LOGSNR)[1].tolist() == [0, 30, 302, 722, 999]
    assert device_ts(L, d, 10, LOGSNR)[1].tolist()[:6] == [0, 5, 22, 73, 202, 410]
    assert device_ts(L, d, 1000, LOGSNR)[1].tolist() == list(range(1000))
    chk(pkg, L.bla_diffusion_destroy(d))


def device_coefficients(L, d, t_last, t, t_prev):
    out = np.full(6, -7.0)
    return L.bla_diffusion_dpmpp_coefficients(d, t_last, t, t_prev, out.ctypes.data_as(C.POINTER(C.c_double))), out


def test_coefficients(pkg, L, dif):
    d, sched = dif
    worst = 0.0
    for t_last, t, t_prev in CASES + [(999, 998, 997), (500, 250, 0), (-1, 1, 0), (20, 10, 5), (999, 0, -1)]:
        st, got = device_coefficients(L, d, t_last, t, t_prev)
        want = coefficients(sched, t_last, t, t_prev)
        assert st == 0
        rel = np.abs(got - want) / np.where(want == 0, 1.0, np.abs(want))
        worst = max(worst, rel.max())
        assert rel.max() <= 1e-14, (t_last, t, t_prev, got, want)
        if t_prev < 0 or t_last < 0:
            assert got[4] == 1.0 and got[5] == 0.0
        if t_prev < 0:
            assert got[2] == 0.0 and got[3] == 1.0
    print(f"coefficients vs numpy: worst relative difference {worst:.1e}")
    for t_last, t, t_prev in ((-1, T, 10), (-1, -1, -1), (-1, 10, 10), (-1, 10, 11), (-1, 10, -2), (10, 10, 5), (5, 10, 3), (T, 10, 5), (-2, 10, 5)):
        st, out = device_coefficients(L, d, t_last, t, t_prev)
        assert st == BLA_ERR_INVALID and (out == -7).all(), (t_last, t, t_prev)


# ---- 2: the step against float64 ---------------------------------------------------------------------------------------------------------

def step_inputs(Fl, t):
    return (uniform(21 + t, (B, Fl), -2, 2, np.float32), uniform(22 + t, (B, Fl), -2, 2, np.float32), uniform(23 + t, (B, Fl), -1, 1, np.float32),
            uniform(24 + t, (B, Fl), -1, 1, np.float32))


def run_step(pkg, L, d, x, e, hist, t_last, t, t_prev, clip, offset=0):
    dx, de, dh = Guarded(pkg, x, offset), Guarded(pkg, e), Guarded(pkg, hist)
    tn = Guarded(pkg, np.full((B, DIM), -7, np.float32))
    chk(pkg, L.bla_diffusion_dpmpp_step_f32(d, None, dx.ptr, de.ptr, dh.ptr, B, x.shape[1], t_last, t, t_prev, clip, DIM, tn.ptr))
    assert np.array_equal(de.numpy(), e)
    return dx.numpy(), dh.numpy(), tn.numpy()


def test_dpmpp_step(pkg, L, dif):
    d, sched = dif
    worst = {}
    for Fl, offset in SHAPES:
        for t_last, t, t_prev in CASES:
            x, e, hist, hist2 = step_inputs(Fl, t)
            c, sec = coefficients(sched, t_last, t, t_prev), second_order(t_last, t_prev)
            for clip in (0, 1):
                got_x, got_h, tn = run_step(pkg, L, d, x, e, hist, t_last, t, t_prev, clip, offset)
                want_x, want_h, _, _ = numpy_dpmpp(x, e, hist, c, clip, sec)
                Bx, Bh = bounds(x, e, hist, c, clip, sec)
                fx, fh = (np.abs(got_x - want_x) / Bx).max(), (np.abs(got_h - want_h) / Bh).max()
                key = (t_last, t, t_prev)
                worst[key] = np.maximum(worst.get(key, 0), (fx, fh))
                assert fx <= 1 and fh <= 1, (Fl, offset, t_last, t, t_prev, clip, fx, fh)
                if clip:
                    assert np.abs(got_h).max() <= 1
                if t_prev >= 0:
                    assert np.abs(tn - np.stack([time_embedding(t_prev, DIM)] * B)).max() <= 1e-6
                else:
                    assert (tn == -7).all()
                    assert np.array_equal(got_x, got_h)                      # the last step returns the x0 prediction it stores
                again = run_step(pkg, L, d, x, e, hist, t_last, t, t_prev, clip, offset)
                assert np.array_equal(again[0], got_x) and np.array_equal(again[1], got_h)
                other = run_step(pkg, L, d, x, e, hist2, t_last, t, t_prev, clip, offset)
                assert np.array_equal(other[1], got_h)                       # the stored prediction never depends on the old one
                assert np.array_equal(other[0], got_x) == (not sec), (t_last, t, t_prev)   # and x only in the second-order case
    print("DPM-Solver++ step vs float64, worst fraction of (B_x, B_h) by (t_last, t, t_prev): " + ", ".join(
        "%s (%.2f, %.2f)" % (k, v[0], v[1]) for k, v in worst.items()))
    print("worst overall: %.2f of B_x, %.2f of B_h" % tuple(np.max(list(worst.values()), axis=0)))


def test_dpmpp_step_refusals(pkg, L, dif):
    d, _ = dif
    dx, de, dh = (pkg.to_device(np.zeros((B, 48), np.float32)) for _ in range(3))
    for t_last, t, t_prev in ((-1, T, 10), (-1, -1, -1), (-1, 10, 10), (-1, 10, 11), (-1, 10, -2), (10, 10, 5), (5, 10, 3), (T, 10, 5), (-2, 10, 5)):
        assert L.bla_diffusion_dpmpp_step_f32(d, None, dx.ptr, de.ptr, dh.ptr, B, 48, t_last, t, t_prev, 0, DIM, None) == BLA_ERR_INVALID, (t_last, t, t_prev)
        assert L.bla_diffusion_guided_dpmpp_step_f32(d, None, dx.ptr, None, de.ptr, de.ptr, 1.0, dh.ptr, B, 48, t_last, t, t_prev, 0, DIM, None, None, 0,
                                                     None) == BLA_ERR_INVALID, (t_last, t, t_prev)
    assert L.bla_diffusion_dpmpp_step_f32(d, None, dx.ptr, de.ptr, None, B, 48, -1, 10, 5, 0, DIM, None) == BLA_ERR_INVALID     # no history buffer
    assert L.bla_diffusion_dpmpp_step_f32(d, None, None, de.ptr, dh.ptr, B, 48, -1, 10, 5, 0, DIM, None) == BLA_ERR_INVALID
    assert L.bla_diffusion_dpmpp_step_f32(d, None, dx.ptr, de.ptr, dh.ptr, 0, 48, -1, 10, 5, 0, DIM, None) == BLA_ERR_INVALID
    assert L.bla_diffusion_guided_dpmpp_step_f32(d, None, dx.ptr, None, de.ptr, de.ptr, float("nan"), dh.ptr, B, 48, -1, 10, 5, 0, DIM, None, None, 0,
                                                 None) == BLA_ERR_INVALID
    assert L.bla_diffusion_guided_dpmpp_step_f32(d, None, dx.ptr, None, de.ptr, de.ptr, 1.0, None, B, 48, -1, 10, 5, 0, DIM, None, None, 0,
                                                 None) == BLA_ERR_INVALID
    assert (dx.numpy() == 0).all() and (dh.numpy() == 0).all()


# ---- 3: the guided step ------------------------------------------------------------------------------------------------------------------

def test_guided_dpmpp_step(pkg, L, dif):
    d, sched = dif
    table = uniform(91, (CLASSES + 1, DIM), -1, 1, np.float32)
    rows = np.array([3, 10, 7, 10, 10, 10], np.int32)
    dtab, drows = pkg.to_device(table), pkg.to_device(rows, np.int32)
    for Fl, offset in SHAPES:
        for t_last, t, t_prev in ((999, 979, 959), (-1, 431, 381), (99, 49, -1), (3, 1, 0)):
            x, eu, hist, _ = step_inputs(Fl, t)
            ec = uniform(25 + t, (B, Fl), -2, 2, np.float32)
            for s, clip in ((0.0, 0), (0.0, 1), (2.5, 0), (2.5, 1)):
                dx, dcopy, dh = Guarded(pkg, x, offset), Guarded(pkg, np.zeros((B, Fl), np.float32)), Guarded(pkg, hist)
                dec, deu, tn = Guarded(pkg, ec), Guarded(pkg, eu), Guarded(pkg, np.full((2 * B, DIM), -7, np.float32))
                chk(pkg, L.bla_diffusion_guided_dpmpp_step_f32(d, None, dx.ptr, dcopy.ptr, dec.ptr, deu.ptr, s, dh.ptr, B, Fl, t_last, t, t_prev, clip, DIM,
                                                               tn.ptr, dtab.ptr, CLASSES, drows.ptr))
                got_x, got_h = dx.numpy(), dh.numpy()
                assert np.array_equal(dcopy.numpy(), got_x)
                if t_prev >= 0:
                    emb = np.stack([time_embedding(t_prev, DIM)] * (2 * B))
                    assert np.abs(tn.numpy() - (emb + table[rows])).max() <= 2e-6, (t, t_prev)
                else:
                    assert (tn.numpy() == -7).all()
                # the unguided step on eps~ = fmaf(s, eps_c - eps_u, eps_u) formed in float32 (eps_u itself at s = 0), bit for bit
                e = fmaf(np.float32(s), ec - eu, eu)
                if s == 0.0:
                    assert np.array_equal(e, eu)
                ref_x, ref_h, _ = run_step(pkg, L, d, x, e, hist, t_last, t, t_prev, clip, offset)
                assert np.array_equal(ref_x, got_x) and np.array_equal(ref_h, got_h), (Fl, offset, t_last, t, t_prev, s, clip)
        # without a copy and without a table: the same x, the bare embedding
        x, eu, hist, _ = step_inputs(Fl, 431)
        dx, dh, deu, tn = Guarded(pkg, x, offset), Guarded(pkg, hist), Guarded(pkg, eu), Guarded(pkg, np.full((2 * B, DIM), -7, np.float32))
        chk(pkg, L.bla_diffusion_guided_dpmpp_step_f32(d, None, dx.ptr, None, deu.ptr, deu.ptr, 2.5, dh.ptr, B, Fl, 451, 431, 411, 0, DIM, tn.ptr, None, 0, None))
        assert np.array_equal(dx.numpy(), run_step(pkg, L, d, x, eu, hist, 451, 431, 411, 0, offset)[0])
        assert np.abs(tn.numpy() - np.stack([time_embedding(411, DIM)] * (2 * B))).max() <= 1e-6


# ---- 4: solver order on the device -------------------------------------------------------------------------------------------------------

def test_solver_order_on_the_device(pkg, L, dif):
    """the step entries driven with the exact noise predictor of x0 ~ N(0, 0.25 I) (tests/test_dpmpp_host.py), computed in numpy from the x read back:
    every element of x is its x_T times the sampler's gain"""
    d, sched = dif
    Fl = 75
    xT = uniform(61, (B, Fl), 0.5, 2, np.float32) * np.where(uniform(62, (B, Fl), -1, 1, np.float32) < 0, -1, 1).astype(np.float32)
    exact = exact_gain(sched)

    def run(S, spacing, dpmpp):
        st, ts = device_ts(L, d, S, spacing)
        assert st == 0
        dx, de, dh = pkg.to_device(xT), pkg.empty((B, Fl)), pkg.to_device(np.zeros((B, Fl), np.float32))
        t_last = -1
        for i in range(S - 1, -1, -1):
            t, t_prev = int(ts[i]), int(ts[i - 1]) if i else -1
            upload(pkg, de.ptr, eps_star(dx.numpy().astype(np.float64), sched, t).astype(np.float32))
            if dpmpp:
                chk(pkg, L.bla_diffusion_dpmpp_step_f32(d, None, dx.ptr, de.ptr, dh.ptr, B, Fl, t_last, t, t_prev, 0, DIM, None))
            else:
                chk(pkg, L.bla_diffusion_ddim_step_f32(d, None, dx.ptr, de.ptr, B, Fl, t, t_prev, 0.0, 0, 1, DIM, None))
            t_last = t
        return np.abs(dx.numpy().astype(np.float64) / xT - exact).max()      # the worst element

    err = {("2M log-SNR", 10): run(10, LOGSNR, True), ("2M log-SNR", 20): run(20, LOGSNR, True), ("2M trailing", 20): run(20, TRAILING, True),
           ("DDIM trailing", 40): run(40, TRAILING, False), ("DDIM trailing", 80): run(80, TRAILING, False)}
    print("|gain - exact| on the device, worst of %d elements: " % (B * Fl) + ", ".join("%s S = %d: %.4f" % (k[0], k[1], v) for k, v in err.items()))
    assert err["2M log-SNR", 10] < err["DDIM trailing", 40]
    assert err["2M trailing", 20] < err["DDIM trailing", 40]
    assert err["2M log-SNR", 20] < err["DDIM trailing", 80]


# ---- 5: the loops ------------------------------------------------------------------------------------------------------------------------

def test_dpmpp_sampler(pkg, L):
    Bm, steps, S, dim = 3, 20, 4, CFG["time_dim"]
    h, tensors = unet_build(pkg, CFG, Bm)
    load_params(pkg, h, tensors, CFG)
    d, sched = diffusion(pkg, L, steps)
    x = pkg.empty((Bm, UNET_F))
    temb, hist = pkg.empty((Bm, dim)), pkg.empty((Bm, UNET_F))
    results = {}
    for spacing in (LOGSNR, TRAILING):
        for clip in (0, 1):
            chk(pkg, L.bla_rand_normal_f32(None, x.ptr, Bm * UNET_F, 0.0, 1.0, 5, 0))
            chk(pkg, L.bla_unet_sample_dpmpp_f32(h, d, None, x.ptr, S, spacing, clip))
            want = x.numpy()
            assert np.isfinite(want).all()
            chk(pkg, L.bla_rand_normal_f32(None, x.ptr, Bm * UNET_F, 0.0, 1.0, 5, 0))      # again, the workspaces grown: bit-identical
            chk(pkg, L.bla_unet_sample_dpmpp_f32(h, d, None, x.ptr, S, spacing, clip))
            assert np.array_equal(x.numpy(), want), (spacing, clip)
            # composed from the public pieces: forward, then the step with the caller's history and the t_last bookkeeping
            ts = sample_ts(sched, S, spacing)
            chk(pkg, L.bla_rand_normal_f32(None, x.ptr, Bm * UNET_F, 0.0, 1.0, 5, 0))
            upload(pkg, hist.ptr, np.full((Bm, UNET_F), np.nan, np.float32))                # never read before it is written
            chk(pkg, L.bla_time_embedding_f32(None, pkg.to_device(np.full(Bm, ts[-1], np.int32), np.int32).ptr, Bm, dim, temb.ptr))
            t_last = -1
            for i in range(S - 1, -1, -1):
                t, t_prev = ts[i], ts[i - 1] if i else -1
                chk(pkg, L.bla_unet_forward_f32(h, None, x.ptr, temb.ptr, None))
                chk(pkg, L.bla_diffusion_dpmpp_step_f32(d, None, x.ptr, L.bla_unet_output(h), hist.ptr, Bm, UNET_F, t_last, t, t_prev, clip, dim, temb.ptr))
                t_last = t
            assert np.array_equal(x.numpy(), want), (spacing, clip)
            results[spacing, clip] = want
    assert not np.array_equal(results[LOGSNR, 0], results[TRAILING, 0])
    for s_bad, spacing in ((0, LOGSNR), (steps + 1, LOGSNR), (S, 7)):
        assert L.bla_unet_sample_dpmpp_f32(h, d, None, x.ptr, s_bad, spacing, 0) == BLA_ERR_INVALID, (s_bad, spacing)
    chk(pkg, L.bla_diffusion_destroy(d)); chk(pkg, L.bla_unet_destroy(h))


def test_guided_dpmpp_sampler(pkg, L):
    n, steps, S, dim, s = 2, 20, 4, CFG["time_dim"], 3.0
    h, tensors = unet_build(pkg, CFG, 2 * n)
    load_params(pkg, h, tensors, CFG)
    d, sched = diffusion(pkg, L, steps)
    table = uniform(95, (CLASSES + 1, dim), -0.5, 0.5, np.float32)
    dtab = pkg.to_device(table)
    x = pkg.empty((n, UNET_F))
    lab = np.array([3, 7], np.int32)
    dlab = pkg.to_device(lab, np.int32)
    x2, temb, rows, hist = pkg.empty((2 * n, UNET_F)), pkg.empty((2 * n, dim)), pkg.empty((2 * n,), np.int32), pkg.empty((n, UNET_F))
    out = L.bla_unet_output(h)
    # the third case: a device label outside [0, classes] cannot be refused without a round trip, so its image is sampled with no class row (row -1 in the
    # composed loop); the same label on the host is refused before anything touches x
    for spacing, lb in ((LOGSNR, lab), (TRAILING, lab), (LOGSNR, np.array([3, CLASSES + 5], np.int32))):
        dlb = pkg.to_device(lb, np.int32)
        chk(pkg, L.bla_rand_normal_f32(None, x.ptr, n * UNET_F, 0.0, 1.0, 5, 0))
        noise = x.numpy()
        chk(pkg, L.bla_unet_sample_guided_dpmpp_f32(h, d, None, x.ptr, dtab.ptr, CLASSES, dlb.ptr, s, S, spacing, 1))
        want = x.numpy()
        assert np.isfinite(want).all()
        for labels in (dlb.ptr, lb.ctypes.data):                                     # again (workspaces grown), and with host labels
            chk(pkg, L.bla_rand_normal_f32(None, x.ptr, n * UNET_F, 0.0, 1.0, 5, 0))
            status = L.bla_unet_sample_guided_dpmpp_f32(h, d, None, x.ptr, dtab.ptr, CLASSES, labels, s, S, spacing, 1)
            if labels == lb.ctypes.data and lb.max() > CLASSES:
                assert status == BLA_ERR_INVALID and np.array_equal(x.numpy(), noise)
            else:
                chk(pkg, status)
                assert np.array_equal(x.numpy(), want), spacing
        # composed from the public pieces as in test_guided_ddim_sampler
        ts = sample_ts(sched, S, spacing)
        chk(pkg, L.bla_rand_normal_f32(None, x2.ptr, n * UNET_F, 0.0, 1.0, 5, 0))
        chk(pkg, L.bla_rand_normal_f32(None, x2.ptr + 4 * n * UNET_F, n * UNET_F, 0.0, 1.0, 5, 0))
        upload(pkg, hist.ptr, np.full((n, UNET_F), np.nan, np.float32))
        dts, dl2 = pkg.to_device(np.full(2 * n, ts[-1], np.int32), np.int32), pkg.to_device(np.array(list(lb) + [CLASSES, CLASSES], np.int32), np.int32)
        chk(pkg, L.bla_time_embedding_f32(None, dts.ptr, 2 * n, dim, temb.ptr))
        chk(pkg, L.bla_class_embedding_f32(None, dtab.ptr, CLASSES, dl2.ptr, 2 * n, dim, 0.0, 0, 0, rows.ptr, temb.ptr))
        assert rows.numpy().tolist() == [int(r) if r <= CLASSES else -1 for r in lb] + [CLASSES, CLASSES]
        t_last = -1
        for i in range(S - 1, -1, -1):
            t, t_prev = ts[i], ts[i - 1] if i else -1
            chk(pkg, L.bla_unet_forward_f32(h, None, x2.ptr, temb.ptr, None))
            chk(pkg, L.bla_diffusion_guided_dpmpp_step_f32(d, None, x2.ptr, x2.ptr + 4 * n * UNET_F, out, out + 4 * n * UNET_F, s, hist.ptr, n, UNET_F, t_last, t,
                                                           t_prev, 1, dim, temb.ptr, dtab.ptr, CLASSES, rows.ptr))
            t_last = t
        after = x2.numpy()
        assert np.array_equal(after[:n], after[n:]) and np.array_equal(after[:n], want), spacing
    for s_bad, spacing in ((0, LOGSNR), (steps + 1, TRAILING), (S, 7)):
        assert L.bla_unet_sample_guided_dpmpp_f32(h, d, None, x.ptr, dtab.ptr, CLASSES, dlab.ptr, s, s_bad, spacing, 0) == BLA_ERR_INVALID, (s_bad, spacing)
    chk(pkg, L.bla_diffusion_destroy(d)); chk(pkg, L.bla_unet_destroy(h))
    h3, _ = unet_build(pkg, CFG, 3)                                                    # an odd model batch has no halves
    d, _ = diffusion(pkg, L, steps)
    d1 = pkg.to_device(np.array([1], np.int32), np.int32)
    assert L.bla_unet_sample_guided_dpmpp_f32(h3, d, None, x.ptr, dtab.ptr, CLASSES, d1.ptr, s, S, LOGSNR, 0) == BLA_ERR_INVALID
    chk(pkg, L.bla_diffusion_destroy(d)); chk(pkg, L.bla_unet_destroy(h3))


# ---- 6: the example program --------------------------------------------------------------------------------------------------------------

def test_example_dpmpp_sample(pkg, tmp_path):
    pkg.build_native()
    subprocess.check_call(["make", "-s", "-C", EX, "cifar_unet_gpu"])
    (tmp_path / "data" / "cifar").mkdir(parents=True)
    recs = np.random.default_rng(13).integers(0, 256, (16, 3073), dtype=np.uint8)
    recs[:, 0] = np.arange(16) % 10
    recs.tofile(tmp_path / "data" / "cifar" / "data_batch_1.bin")
    r = run_example(["fit", "1", "4"], tmp_path, {"BLA_DIFFUSION_STEPS": "50", "BLA_UNET_WEIGHTS": str(tmp_path / "w"), "BLA_UNET_CLASSES": "1"}, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr

    def sample(out, **env):
        r = run_example(["sample", "2", str(tmp_path / out)], tmp_path,
                        dict({"BLA_DIFFUSION_STEPS": "50", "BLA_UNET_WEIGHTS": str(tmp_path / "w"), "BLA_UNET_SAMPLE_STEPS": "5"}, **env), timeout=900)
        assert r.returncode == 0, r.stdout + r.stderr
        assert sorted(os.listdir(tmp_path / out)) == ["sample_0000.bmp", "sample_0001.bmp"]
        return [open(tmp_path / out / f"sample_{i:04d}.bmp", "rb").read() for i in range(2)]

    a, b = sample("s_a", BLA_UNET_SAMPLER="dpmpp"), sample("s_b", BLA_UNET_SAMPLER="dpmpp")
    ddim, named = sample("s_ddim"), sample("s_named", BLA_UNET_SAMPLER="ddim")
    trailing = sample("s_trailing", BLA_UNET_SAMPLER="dpmpp", BLA_UNET_SPACING="trailing")
    assert all(bmp_ok(v) for v in a + trailing)
    assert a == b and a != ddim and ddim == named
    assert sample("s_logsnr", BLA_UNET_SAMPLER="dpmpp", BLA_UNET_SPACING="logsnr", BLA_UNET_ETA="0") == a and trailing != a
    g = sample("s_guided", BLA_UNET_SAMPLER="dpmpp", BLA_UNET_CLASS="3", BLA_UNET_CLIP="1")
    assert all(bmp_ok(v) for v in g) and g != a
