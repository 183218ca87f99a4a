"""Training objectives on the device (include/bla.h, "training objectives": bla_diffusion_create_from_betas, bla_diffusion_set_objective,
bla_diffusion_loss_weight, bla_diffusion_target_f32, bla_diffusion_to_eps_f32, bla_diffusion_loss_f32, bla_unet_backward_from_f32, and the conversion
inside the sampling and evaluation loops) against the float64 restatement and the rounding bounds that tests/test_objective_host.py validates, on the
smallest shapes that reach every path of the element kernels (16-byte body, scalar tail, all scalar for a misaligned pointer), and the example
program's fit / sample / eval with an objective."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from inputs import uniform
from test_diffusion_gpu import CFG, F as UNET_F, diffusion, fetch, upload
from test_dpmpp_gpu import L, chk  # noqa: F401  (L is a fixture)
from test_dpmpp_host import LOGSNR, TRAILING, coefficients, sample_ts, schedule
from test_guidance_gpu import bmp_ok
from test_objective_host import (EPS, FL, OBJECTIVE_ENV, U, V, X0, coef, cosine_betas, eps_from_v, eps_from_x0, loss_weights, run_program, schedule_from_betas,
                                 v_of)
from test_unet_model import build as unet_build, load_params

pytestmark = pytest.mark.gpu

EX = os.path.join(ROOT, "examples")
BLA_ERR_INVALID = 1
T, B, DIM, GUARD = 1000, 3, 24, 4
SHAPES = [(75, 0), (48, 0), (75, 1)]          # (F, offset of the first buffer in floats): body + tail, body only, all scalar
STEPS = [(0, 499, 999), (1, 998, 499), (999, 0, 1), 979]      # per-image timesteps from {0, 1, 499, 998, 999}, and one uniform t_const
LISTED = (0, 1, 499, 998, 999)


class Guarded:
    """a device array of n elements `offset` elements into its buffer, with GUARD elements of -7 on either side"""

    def __init__(self, pkg, a, offset=0):
        a = np.ascontiguousarray(a)
        self.pkg, self.n, self.dtype, self.shape = pkg, a.size, a.dtype, a.shape
        self.buf = pkg.empty((offset + a.size + 2 * GUARD,), a.dtype)
        self.ptr = self.buf.ptr + a.itemsize * (offset + GUARD)           # GUARD x 4 bytes = 16: the alignment is the offset's
        upload(pkg, self.ptr - a.itemsize * GUARD, np.concatenate([np.full(GUARD, -7, a.dtype), a.ravel(), np.full(GUARD, -7, a.dtype)]))

    def numpy(self):
        got = fetch(self.pkg, self.ptr - self.dtype.itemsize * GUARD, self.n + 2 * GUARD, self.dtype)
        assert (got[:GUARD] == -7).all() and (got[-GUARD:] == -7).all(), "wrote outside the buffer"
        return got[GUARD:-GUARD].reshape(self.shape)


def from_betas(pkg, L, betas):
    betas = np.ascontiguousarray(betas, np.float64)
    d = C.c_void_p()
    chk(pkg, L.bla_diffusion_create_from_betas(C.byref(d), len(betas), betas.ctypes.data))
    return d


def read_schedule(pkg, L, d, steps):
    out = []
    for t in range(steps):
        b, ab = C.c_double(), C.c_double()
        chk(pkg, L.bla_diffusion_schedule(d, t, C.byref(b), C.byref(ab)))
        out.append((b.value, ab.value))
    return np.array(out)


@pytest.fixture(scope="module")
def objects(pkg, L):
    """one diffusion object per schedule at T = 1000 with the float64 restatement of its schedule; the tests set the objective they need"""
    out = {"linear": (from_betas(pkg, L, schedule(T)[:, 0]), schedule(T))}
    cos = schedule_from_betas(cosine_betas(T)[0])
    out["cosine"] = (from_betas(pkg, L, cos[:, 0]), cos)
    for name, (d, sched) in out.items():
        assert np.array_equal(read_schedule(pkg, L, d, T), sched), name          # the restatement is the object's, bit for bit
    yield out
    for d, _ in out.values():
        chk(pkg, L.bla_diffusion_destroy(d))


def steps_arg(pkg, ts):
    """(d_t, t_const, per-image timesteps) of one entry of STEPS"""
    if isinstance(ts, int):
        return None, ts, np.full(B, ts), None
    dt = pkg.to_device(np.array(ts, np.int32), np.int32)
    return dt.ptr, 0, np.array(ts), dt


def objective(L, d):
    p, g = C.c_int(-7), C.c_double(-7)
    assert L.bla_diffusion_objective(d, C.byref(p), C.byref(g)) == 0
    return p.value, g.value


# ---- 1: create_from_betas ------------------------------------------------------------------------------------------------------------------

def test_create_from_betas_equals_create(pkg, L, objects):
    d1, sched = diffusion(pkg, L, T)
    b0, b1 = float(np.float32(1e-4)), float(np.float32(0.02))
    betas = np.array([b0 + (b1 - b0) * t / (T - 1) for t in range(T)])          # bla_diffusion_create's expression, float arguments widened
    d2 = from_betas(pkg, L, betas)
    assert np.array_equal(read_schedule(pkg, L, d2, T), sched)
    Fl, seed = 75, 11
    x0 = pkg.to_device(uniform(3, (B, Fl), -1, 1, np.float32))
    outs = []
    for d in (d1, d2):
        dt, eps, xt, temb = pkg.empty((B,), np.int32), pkg.empty((B, Fl)), pkg.empty((B, Fl)), pkg.empty((B, DIM))
        chk(pkg, L.bla_diffusion_noise_f32(d, None, x0.ptr, B, Fl, DIM, seed, 2, dt.ptr, eps.ptr, xt.ptr, temb.ptr))
        outs.append((dt.numpy(), eps.numpy(), xt.numpy(), temb.numpy()))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*outs))
    for case in ((-1, 999, 979), (999, 979, 959), (99, 49, -1), (3, 1, 0)):
        c1, c2 = np.zeros(6), np.zeros(6)
        chk(pkg, L.bla_diffusion_dpmpp_coefficients(d1, *case, c1.ctypes.data_as(C.POINTER(C.c_double))))
        chk(pkg, L.bla_diffusion_dpmpp_coefficients(d2, *case, c2.ctypes.data_as(C.POINTER(C.c_double))))
        assert c1.tobytes() == c2.tobytes(), case
    assert objective(L, d2) == (EPS, 0.0)
    chk(pkg, L.bla_diffusion_destroy(d1)); chk(pkg, L.bla_diffusion_destroy(d2))
    # nothing assumes a linear schedule: the cosine object at every listed timestep
    d, cos = objects["cosine"]
    for spacing in (TRAILING, LOGSNR):
        ts = np.full(10, -7, np.int32)
        chk(pkg, L.bla_diffusion_sample_timesteps(d, 10, spacing, ts.ctypes.data))
        assert ts.tolist() == sample_ts(cos, 10, spacing) and ts[-1] == T - 1 and (np.diff(ts) > 0).all() and ts[0] >= 0
    x, e = uniform(5, (B, Fl), -2, 2, np.float32), uniform(6, (B, Fl), -2, 2, np.float32)
    for t_last, t, t_prev in ((-1, 999, 998), (999, 998, 499), (998, 499, 1), (499, 1, 0), (1, 0, -1)):
        c = np.zeros(6)
        chk(pkg, L.bla_diffusion_dpmpp_coefficients(d, t_last, t, t_prev, c.ctypes.data_as(C.POINTER(C.c_double))))
        want = coefficients(cos, t_last, t, t_prev)
        assert np.isfinite(c).all() and (np.abs(c - want) <= 1e-13 * np.abs(want)).all(), (t, c, want)
        dx, de = pkg.to_device(x), pkg.to_device(e)
        chk(pkg, L.bla_diffusion_ddim_step_f32(d, None, dx.ptr, de.ptr, B, Fl, t, t_prev, 0.5, 0, 9, DIM, None))
        assert np.isfinite(dx.numpy()).all(), t
    for t in LISTED[1:]:
        c, w = C.c_double(), C.c_double()
        chk(pkg, L.bla_diffusion_vlb_weights(d, t, C.byref(c), C.byref(w)))
        assert math.isfinite(c.value) and math.isfinite(w.value) and w.value > 0, t
    # refusals
    out = C.c_void_p()
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan"), float("inf")):
        b = np.full(5, 0.01); b[3] = bad
        assert L.bla_diffusion_create_from_betas(C.byref(out), 5, b.ctypes.data) == BLA_ERR_INVALID and out.value is None, bad
    b = np.full(5, 0.01)
    assert L.bla_diffusion_create_from_betas(C.byref(out), 0, b.ctypes.data) == BLA_ERR_INVALID
    assert L.bla_diffusion_create_from_betas(C.byref(out), 5, None) == BLA_ERR_INVALID
    assert L.bla_diffusion_create_from_betas(None, 5, b.ctypes.data) == BLA_ERR_INVALID


# ---- 2: the objective and its weights --------------------------------------------------------------------------------------------------------

def test_objective_and_weights(pkg, L, objects):
    x0, eps = pkg.to_device(uniform(7, (B, 48), -1, 1, np.float32)), pkg.to_device(uniform(8, (B, 48), -1, 1, np.float32))
    ts = np.array([0, 499, 999], np.int32)
    dt = pkg.to_device(ts, np.int32)
    worst = 0.0
    for name, (d, sched) in objects.items():
        for pred in (EPS, X0, V):
            for gamma in (0.0, 0.5, 5.0):
                chk(pkg, L.bla_diffusion_set_objective(d, pred, gamma))
                assert objective(L, d) == (pred, gamma)
                want = loss_weights(sched[:, 1], pred, gamma)
                got = np.zeros(T)
                w = C.c_double()
                for t in range(T):
                    chk(pkg, L.bla_diffusion_loss_weight(d, t, C.byref(w)))
                    got[t] = w.value
                worst = max(worst, (np.abs(got - want) / want).max())
                assert (np.abs(got - want) <= 4 * 2.0 ** -53 * want).all(), (name, pred, gamma)
                if gamma == 0:
                    assert (got == 1).all()
                target, weight = pkg.empty((B, 48)), Guarded(pkg, np.zeros(B, np.float32))
                chk(pkg, L.bla_diffusion_target_f32(d, None, x0.ptr, eps.ptr, dt.ptr, 0, B, 48, target.ptr, weight.ptr))
                assert weight.numpy().tobytes() == got[ts].astype(np.float32).tobytes(), (name, pred, gamma)
        # refused, and nothing changed
        chk(pkg, L.bla_diffusion_set_objective(d, V, 5.0))
        for pred, gamma in ((3, 5.0), (-1, 5.0), (V, -1.0), (V, float("nan")), (V, float("inf")), (EPS, -1e-300)):
            assert L.bla_diffusion_set_objective(d, pred, gamma) == BLA_ERR_INVALID, (pred, gamma)
            assert objective(L, d) == (V, 5.0)
        w = C.c_double(-7)
        for t in (-1, T):
            assert L.bla_diffusion_loss_weight(d, t, C.byref(w)) == BLA_ERR_INVALID and w.value == -7
        chk(pkg, L.bla_diffusion_set_objective(d, EPS, 0.0))
    print(f"loss weights vs numpy: worst relative difference {worst:.1e}")
    # a schedule so long that alpha_bar underflows to 0: SNR 0, the eps weight is the limit 1 (not 0 / 0), the others 0
    d = from_betas(pkg, L, np.full(300, 0.999))
    assert read_schedule(pkg, L, d, 300)[-1, 1] == 0.0
    w = C.c_double()
    for pred, want in ((EPS, 1.0), (X0, 0.0), (V, 0.0)):
        chk(pkg, L.bla_diffusion_set_objective(d, pred, 5.0))
        chk(pkg, L.bla_diffusion_loss_weight(d, 299, C.byref(w)))
        assert w.value == want, (pred, w.value)
    chk(pkg, L.bla_diffusion_destroy(d))
    # a fresh object: eps-prediction, every weight 1, also where target writes it
    d, _ = diffusion(pkg, L, T)
    assert objective(L, d) == (EPS, 0.0)
    w = C.c_double()
    chk(pkg, L.bla_diffusion_loss_weight(d, 0, C.byref(w)))
    target, weight = pkg.empty((B, 48)), pkg.empty((B,))
    chk(pkg, L.bla_diffusion_target_f32(d, None, None, eps.ptr, dt.ptr, 0, B, 48, target.ptr, weight.ptr))
    assert w.value == 1.0 and (weight.numpy() == 1).all() and target.numpy().tobytes() == eps.numpy().tobytes()
    chk(pkg, L.bla_diffusion_destroy(d))


# ---- 3: target -------------------------------------------------------------------------------------------------------------------------------

def run_target(pkg, L, d, x0, eps, ts, offset):
    dt, t_const, _, keep = steps_arg(pkg, ts)
    dx, de = Guarded(pkg, x0, offset), Guarded(pkg, eps)
    target, weight = Guarded(pkg, np.full(x0.shape, -3, np.float32)), Guarded(pkg, np.full(B, -3, np.float32))
    chk(pkg, L.bla_diffusion_target_f32(d, None, dx.ptr, de.ptr, dt, t_const, B, x0.shape[1], target.ptr, weight.ptr))
    assert dx.numpy().tobytes() == x0.tobytes() and de.numpy().tobytes() == eps.tobytes()
    return target.numpy(), weight.numpy()


def test_target(pkg, L, objects):
    worst = {}
    for name, (d, sched) in objects.items():
        for Fl, offset in SHAPES:
            x0, eps = uniform(61, (B, Fl), -1, 1, np.float32), uniform(62, (B, Fl), -2, 2, np.float32)
            for ts in STEPS:
                tb = steps_arg(pkg, ts)[2]
                a, c = coef(sched, tb)
                for pred in (EPS, X0, V):
                    chk(pkg, L.bla_diffusion_set_objective(d, pred, 5.0))
                    got, w = run_target(pkg, L, d, x0, eps, ts, offset)
                    assert w.tobytes() == loss_weights(sched[tb, 1], pred, 5.0).astype(np.float32).tobytes()
                    if pred == EPS:
                        assert got.tobytes() == eps.tobytes()
                    elif pred == X0:
                        assert got.tobytes() == x0.tobytes()
                    else:
                        x0d, epsd = x0.astype(np.float64), eps.astype(np.float64)
                        frac = (np.abs(got - v_of(a, c, x0d, epsd)) / (4 * U * (np.abs(a * epsd) + np.abs(c * x0d)))).max()
                        worst[name] = max(worst.get(name, 0), frac)
                        assert frac <= 1, (name, Fl, offset, ts, frac)
                    again, w2 = run_target(pkg, L, d, x0, eps, ts, offset)
                    assert again.tobytes() == got.tobytes() and w2.tobytes() == w.tobytes()
        # a timestep outside the schedule on the device: a zero target and weight 0 for that image alone
        chk(pkg, L.bla_diffusion_set_objective(d, V, 5.0))
        x0, eps = uniform(61, (B, 75), -1, 1, np.float32), uniform(62, (B, 75), -2, 2, np.float32)
        got, w = run_target(pkg, L, d, x0, eps, (T, 499, -1), 0)
        ref, wr = run_target(pkg, L, d, x0, eps, (499, 499, 499), 0)
        assert (got[[0, 2]] == 0).all() and (w[[0, 2]] == 0).all() and got[1].tobytes() == ref[1].tobytes() and w[1] == wr[1]
        dx = pkg.to_device(x0)
        for t_const in (-1, T):
            assert L.bla_diffusion_target_f32(d, None, dx.ptr, dx.ptr, None, t_const, B, 75, dx.ptr, None) == BLA_ERR_INVALID
        assert L.bla_diffusion_target_f32(d, None, None, dx.ptr, None, 5, B, 75, dx.ptr, None) == BLA_ERR_INVALID            # v needs x0
        assert L.bla_diffusion_target_f32(d, None, dx.ptr, dx.ptr, None, 5, B, 75, None, None) == BLA_ERR_INVALID
        assert L.bla_diffusion_target_f32(d, None, dx.ptr, dx.ptr, None, 5, 0, 75, dx.ptr, None) == BLA_ERR_INVALID
        assert dx.numpy().tobytes() == x0.tobytes()
        chk(pkg, L.bla_diffusion_set_objective(d, EPS, 0.0))
    print("v target vs float64, worst fraction of 4u(|a eps| + |c x0|): " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


# ---- 4: to_eps -------------------------------------------------------------------------------------------------------------------------------

def run_to_eps(pkg, L, d, pred, x, ts, offset):
    dt, t_const, _, keep = steps_arg(pkg, ts)
    dp, dx = Guarded(pkg, pred, offset), Guarded(pkg, x)
    chk(pkg, L.bla_diffusion_to_eps_f32(d, None, dp.ptr, dx.ptr, dt, t_const, B, pred.shape[1]))
    assert dx.numpy().tobytes() == x.tobytes()
    return dp.numpy()


def test_to_eps(pkg, L, objects):
    worst = {}
    for name, (d, sched) in objects.items():
        for Fl, offset in SHAPES:
            out, x = uniform(71, (B, Fl), -2, 2, np.float32), uniform(72, (B, Fl), -2, 2, np.float32)
            outd, xd = out.astype(np.float64), x.astype(np.float64)
            for ts in STEPS:
                a, c = coef(sched, steps_arg(pkg, ts)[2])
                chk(pkg, L.bla_diffusion_set_objective(d, V, 0.0))
                got = run_to_eps(pkg, L, d, out, x, ts, offset)
                fv = (np.abs(got - eps_from_v(a, c, outd, xd)) / (4 * U * (np.abs(a * outd) + np.abs(c * xd)))).max()
                assert run_to_eps(pkg, L, d, out, x, ts, offset).tobytes() == got.tobytes()
                chk(pkg, L.bla_diffusion_set_objective(d, X0, 0.0))
                got = run_to_eps(pkg, L, d, out, x, ts, offset)
                fx = (np.abs(got - eps_from_x0(a, c, outd, xd)) / (5 * U * (np.abs(xd) + np.abs(a * outd)) / c)).max()
                worst[name] = np.maximum(worst.get(name, 0), (fv, fx))
                assert fv <= 1 and fx <= 1, (name, Fl, offset, ts, fv, fx)
                chk(pkg, L.bla_diffusion_set_objective(d, EPS, 0.0))
                assert run_to_eps(pkg, L, d, out, x, ts, offset).tobytes() == out.tobytes()
        # a timestep outside the schedule on the device leaves that image as it is
        chk(pkg, L.bla_diffusion_set_objective(d, V, 0.0))
        out, x = uniform(71, (B, 75), -2, 2, np.float32), uniform(72, (B, 75), -2, 2, np.float32)
        got, ref = run_to_eps(pkg, L, d, out, x, (T, 499, -1), 0), run_to_eps(pkg, L, d, out, x, (499, 499, 499), 0)
        assert got[[0, 2]].tobytes() == out[[0, 2]].tobytes() and got[1].tobytes() == ref[1].tobytes()
        dx, dp = pkg.to_device(x), pkg.to_device(out)
        for t_const in (-1, T):
            assert L.bla_diffusion_to_eps_f32(d, None, dp.ptr, dx.ptr, None, t_const, B, 75) == BLA_ERR_INVALID
        assert L.bla_diffusion_to_eps_f32(d, None, None, dx.ptr, None, 5, B, 75) == BLA_ERR_INVALID
        assert L.bla_diffusion_to_eps_f32(d, None, dp.ptr, None, None, 5, B, 75) == BLA_ERR_INVALID
        assert dp.numpy().tobytes() == out.tobytes()
        chk(pkg, L.bla_diffusion_set_objective(d, EPS, 0.0))
    print("to_eps vs float64, worst fraction of (4u(|a v| + |c x|), 5u(|x| + |a x0|) / c): " + ", ".join(f"{k} ({v[0]:.2f}, {v[1]:.2f})" for k, v in worst.items()))


def test_round_trip_on_the_device(pkg, L, objects):
    """noise_at -> target (v) -> to_eps on that target returns the noise within the sum of the three stages' bounds: x_t carries 4u(|a x0| + |c eps|)
    (three roundings and second order) and enters through c, the target carries 4u(|a eps| + |c x0|) and enters through a, the conversion adds its own"""
    worst = 0.0
    for name, (d, sched) in objects.items():
        chk(pkg, L.bla_diffusion_set_objective(d, V, 0.0))
        for Fl in (75, 48):
            x0 = uniform(81, (B, Fl), -1, 1, np.float32)
            for ts in STEPS:
                dt, t_const, tb, keep = steps_arg(pkg, ts)
                a, c = coef(sched, tb)
                dx0, eps, xt, temb, v = pkg.to_device(x0), pkg.empty((B, Fl)), pkg.empty((B, Fl)), pkg.empty((B, DIM)), pkg.empty((B, Fl))
                chk(pkg, L.bla_diffusion_noise_at_f32(d, None, dx0.ptr, B, Fl, DIM, dt, t_const, 17, 3 << 32, eps.ptr, xt.ptr, temb.ptr))
                chk(pkg, L.bla_diffusion_target_f32(d, None, dx0.ptr, eps.ptr, dt, t_const, B, Fl, v.ptr, None))
                chk(pkg, L.bla_diffusion_to_eps_f32(d, None, v.ptr, xt.ptr, dt, t_const, B, Fl))
                e, x0d = eps.numpy().astype(np.float64), x0.astype(np.float64)
                vd, xd = v_of(a, c, x0d, e), a * x0d + c * e
                bound = 4 * U * (a * (np.abs(a * e) + np.abs(c * x0d)) + c * (np.abs(a * x0d) + np.abs(c * e)) + np.abs(a * vd) + np.abs(c * xd))
                frac = (np.abs(v.numpy() - e) / bound).max()
                worst = max(worst, frac)
                assert frac <= 1, (name, Fl, ts, frac)
        chk(pkg, L.bla_diffusion_set_objective(d, EPS, 0.0))
    print(f"round trip: worst fraction of the summed bound {worst:.2f}")


# ---- 5: loss ---------------------------------------------------------------------------------------------------------------------------------

def test_loss(pkg, L):
    worst = 0.0
    for Fl, offset in SHAPES:
        out, target = uniform(91, (B, Fl), -2, 2, np.float32), uniform(92, (B, Fl), -2, 2, np.float32)
        d = out.astype(np.float64) - target.astype(np.float64)
        sq = np.array([math.fsum(r) for r in d * d])
        for w in (None, np.array([0.37, 1.0, 2.5e-3], np.float32), np.array([5.0, 0.0, 4.9e-5], np.float32)):
            do, dtg, dw = Guarded(pkg, out, offset), Guarded(pkg, target), Guarded(pkg, w) if w is not None else None

            def run(with_g, with_loss):
                g, loss = Guarded(pkg, np.full((B, Fl), -3, np.float32)), Guarded(pkg, np.full(B, -3, np.float64))
                chk(pkg, L.bla_diffusion_loss_f32(None, do.ptr, dtg.ptr, dw.ptr if dw else None, B, Fl, g.ptr if with_g else None, loss.ptr if with_loss else None))
                return g.numpy(), loss.numpy()

            g, loss = run(True, True)
            wf = np.ones(B, np.float32) if w is None else w
            want_g = np.float32(2) * (out - target) if w is None else (np.float32(2) * w)[:, None] * (out - target)
            assert g.tobytes() == want_g.tobytes(), (Fl, offset, w)
            want = wf.astype(np.float64) * sq
            worst = max(worst, (np.abs(loss - want) / np.where(want > 0, (Fl + 4) * 2.0 ** -53 * want, 1)).max())
            assert (np.abs(loss - want) <= (Fl + 4) * 2.0 ** -53 * want).all(), (Fl, offset, w, loss, want)
            g2, loss2 = run(True, True)
            assert g2.tobytes() == g.tobytes() and loss2.tobytes() == loss.tobytes()
            g3, loss3 = run(True, False)
            assert g3.tobytes() == g.tobytes() and (loss3 == -3).all()
            g4, loss4 = run(False, True)
            assert (g4 == -3).all() and loss4.tobytes() == loss.tobytes()
            g5, loss5 = run(False, False)
            assert (g5 == -3).all() and (loss5 == -3).all()
            assert do.numpy().tobytes() == out.tobytes() and dtg.numpy().tobytes() == target.tobytes()
    print(f"loss vs float64: worst fraction of (F + 4) 2^-53 loss {worst:.2f}")
    do = pkg.to_device(np.zeros((B, 48), np.float32))
    assert L.bla_diffusion_loss_f32(None, None, do.ptr, None, B, 48, do.ptr, None) == BLA_ERR_INVALID
    assert L.bla_diffusion_loss_f32(None, do.ptr, None, None, B, 48, do.ptr, None) == BLA_ERR_INVALID
    assert L.bla_diffusion_loss_f32(None, do.ptr, do.ptr, None, 0, 48, do.ptr, None) == BLA_ERR_INVALID
    assert L.bla_diffusion_loss_f32(None, do.ptr, do.ptr, None, B, 0, do.ptr, None) == BLA_ERR_INVALID


# ---- 6: the backward pass from a given output gradient -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("Bm", [3, 1])
def test_backward_from(pkg, L, Bm):
    dim = CFG["time_dim"]
    h, tensors = unet_build(pkg, CFG, Bm)
    _, total = load_params(pkg, h, tensors, CFG)
    x, temb = pkg.to_device(uniform(101, (Bm, UNET_F), -1, 1, np.float32)), pkg.to_device(uniform(102, (Bm, dim), 0, 1, np.float32))
    noise, g, dtemb = pkg.to_device(uniform(103, (Bm, UNET_F), -2, 2, np.float32)), pkg.empty((Bm, UNET_F)), pkg.empty((Bm, dim))
    assert L.bla_unet_backward_from_f32(h, None, g.ptr) == BLA_ERR_INVALID                      # no forward pass so far
    chk(pkg, L.bla_unet_forward_f32(h, None, x.ptr, temb.ptr, None))
    chk(pkg, L.bla_unet_backward_f32(h, None, noise.ptr))
    chk(pkg, L.bla_unet_embedding_grad_f32(h, None, dtemb.ptr))
    want, want_dtemb = fetch(pkg, L.bla_unet_grads(h), total, np.float32), dtemb.numpy()
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    chk(pkg, L.bla_memset(L.bla_unet_grads(h), 0, 4 * total, None))
    chk(pkg, L.bla_unet_forward_f32(h, None, x.ptr, temb.ptr, None))
    assert L.bla_unet_embedding_grad_f32(h, None, dtemb.ptr) == BLA_ERR_INVALID                 # no backward pass since that forward pass
    chk(pkg, L.bla_diffusion_loss_f32(None, L.bla_unet_output(h), noise.ptr, None, Bm, UNET_F, g.ptr, None))
    seed = g.numpy()
    assert L.bla_unet_backward_from_f32(h, None, None) == BLA_ERR_INVALID
    chk(pkg, L.bla_unet_backward_from_f32(h, None, g.ptr))
    assert fetch(pkg, L.bla_unet_grads(h), total, np.float32).tobytes() == want.tobytes()
    assert g.numpy().tobytes() == seed.tobytes()                                               # only read
    dtemb.fill_bytes(0xff)
    chk(pkg, L.bla_unet_embedding_grad_f32(h, None, dtemb.ptr))
    assert dtemb.numpy().tobytes() == want_dtemb.tobytes()
    chk(pkg, L.bla_unet_destroy(h))


# ---- 7: the loops ----------------------------------------------------------------------------------------------------------------------------

def set_all(pkg, L, d, pred):
    chk(pkg, L.bla_diffusion_set_objective(d, pred, 0.0))


def test_loops_convert_the_output(pkg, L):
    Bm, steps, S, K, dim = 3, 20, 4, 3, CFG["time_dim"]
    h, tensors = unet_build(pkg, CFG, Bm)
    load_params(pkg, h, tensors, CFG)
    d, sched = diffusion(pkg, L, steps)
    x, temb, hist = pkg.empty((Bm, UNET_F)), pkg.empty((Bm, dim)), pkg.empty((Bm, UNET_F))
    x0 = pkg.to_device(uniform(111, (Bm, UNET_F), -1, 1, np.float32))
    ets = [0, 5, 12, 19]
    cts = (C.c_int * (K + 1))(*ets)
    terms = pkg.empty((K + 1, Bm), np.float64)
    out = L.bla_unet_output(h)

    def start():
        chk(pkg, L.bla_rand_normal_f32(None, x.ptr, Bm * UNET_F, 0.0, 1.0, 5, 0))

    def ddim():
        start(); chk(pkg, L.bla_unet_sample_ddim_f32(h, d, None, x.ptr, S, 0.5, 1, 9)); return x.numpy()

    def dpmpp():
        start(); chk(pkg, L.bla_unet_sample_dpmpp_f32(h, d, None, x.ptr, S, LOGSNR, 0)); return x.numpy()

    def evaluate():
        terms.fill_bytes(0xff)
        chk(pkg, L.bla_unet_evaluate_f32(h, d, None, x0.ptr, cts, K + 1, 31, 64, None, 0, None, terms.ptr, None)); return terms.numpy()

    def embed(t):
        chk(pkg, L.bla_time_embedding_f32(None, pkg.to_device(np.full(Bm, t, np.int32), np.int32).ptr, Bm, dim, temb.ptr))

    loops = {"ddim": ddim, "dpmpp": dpmpp, "evaluate": evaluate}
    before = {k: f() for k, f in loops.items()}                  # set_objective has never been called on this object
    set_all(pkg, L, d, V)
    as_v = {k: f() for k, f in loops.items()}
    for k in loops:
        assert np.isfinite(as_v[k]).all() and as_v[k].tobytes() != before[k].tobytes(), k
    # composed from the public pieces: forward, to_eps on the model's output against the buffer it was given, the step or term entry
    ts = sample_ts(sched, S, TRAILING)
    start(); embed(ts[-1])
    for i in range(S - 1, -1, -1):
        t, t_prev = ts[i], ts[i - 1] if i else -1
        chk(pkg, L.bla_unet_forward_f32(h, None, x.ptr, temb.ptr, None))
        chk(pkg, L.bla_diffusion_to_eps_f32(d, None, out, x.ptr, None, t, Bm, UNET_F))
        chk(pkg, L.bla_diffusion_ddim_step_f32(d, None, x.ptr, out, Bm, UNET_F, t, t_prev, 0.5, 1, 9, dim, temb.ptr))
    assert x.numpy().tobytes() == as_v["ddim"].tobytes()
    ts = sample_ts(sched, S, LOGSNR)
    start(); embed(ts[-1])
    t_last = -1
    for i in range(S - 1, -1, -1):
        t, t_prev = ts[i], ts[i - 1] if i else -1
        chk(pkg, L.bla_unet_forward_f32(h, None, x.ptr, temb.ptr, None))
        chk(pkg, L.bla_diffusion_to_eps_f32(d, None, out, x.ptr, None, t, Bm, UNET_F))
        chk(pkg, L.bla_diffusion_dpmpp_step_f32(d, None, x.ptr, out, hist.ptr, Bm, UNET_F, t_last, t, t_prev, 0, dim, temb.ptr))
        t_last = t
    assert x.numpy().tobytes() == as_v["dpmpp"].tobytes()
    eps, xt, t1 = pkg.empty((Bm, UNET_F)), pkg.empty((Bm, UNET_F)), pkg.empty((Bm,), np.float64)
    for i, t in enumerate(ets):
        chk(pkg, L.bla_diffusion_noise_at_f32(d, None, x0.ptr, Bm, UNET_F, dim, None, t, 31, 64 + ((t + 1) << 32), eps.ptr, xt.ptr, temb.ptr))
        chk(pkg, L.bla_unet_forward_f32(h, None, xt.ptr, temb.ptr, None))
        chk(pkg, L.bla_diffusion_to_eps_f32(d, None, out, xt.ptr, None, t, Bm, UNET_F))
        chk(pkg, L.bla_diffusion_vlb_terms_f32(d, None, x0.ptr, xt.ptr, eps.ptr, out, None, t, Bm, UNET_F, t1.ptr, None))
        assert t1.numpy().tobytes() == as_v["evaluate"][i].tobytes(), t
    # back to eps-prediction: what the loops produced before set_objective was ever called
    set_all(pkg, L, d, EPS)
    for k, f in loops.items():
        assert f().tobytes() == before[k].tobytes(), k
    chk(pkg, L.bla_diffusion_destroy(d)); chk(pkg, L.bla_unet_destroy(h))


def test_guided_loop_converts_the_output(pkg, L):
    n, steps, S, dim, s, classes = 2, 20, 4, CFG["time_dim"], 3.0, 10
    h, tensors = unet_build(pkg, CFG, 2 * n)
    load_params(pkg, h, tensors, CFG)
    d, sched = diffusion(pkg, L, steps)
    dtab = pkg.to_device(uniform(95, (classes + 1, dim), -0.5, 0.5, np.float32))
    dlab = pkg.to_device(np.array([3, 7], np.int32), np.int32)
    x = pkg.empty((n, UNET_F))
    x2, temb, rows, hist = pkg.empty((2 * n, UNET_F)), pkg.empty((2 * n, dim)), pkg.empty((2 * n,), np.int32), pkg.empty((n, UNET_F))
    out = L.bla_unet_output(h)

    def guided():
        chk(pkg, L.bla_rand_normal_f32(None, x.ptr, n * UNET_F, 0.0, 1.0, 5, 0))
        chk(pkg, L.bla_unet_sample_guided_dpmpp_f32(h, d, None, x.ptr, dtab.ptr, classes, dlab.ptr, s, S, LOGSNR, 1))
        return x.numpy()

    before = guided()
    set_all(pkg, L, d, V)
    as_v = guided()
    assert np.isfinite(as_v).all() and as_v.tobytes() != before.tobytes()
    # composed as in tests/test_dpmpp_gpu.py, with to_eps over all 2n images of the model's input
    ts = sample_ts(sched, S, LOGSNR)
    chk(pkg, L.bla_rand_normal_f32(None, x2.ptr, n * UNET_F, 0.0, 1.0, 5, 0))
    chk(pkg, L.bla_rand_normal_f32(None, x2.ptr + 4 * n * UNET_F, n * UNET_F, 0.0, 1.0, 5, 0))
    dts, dl2 = pkg.to_device(np.full(2 * n, ts[-1], np.int32), np.int32), pkg.to_device(np.array([3, 7, classes, classes], np.int32), np.int32)
    chk(pkg, L.bla_time_embedding_f32(None, dts.ptr, 2 * n, dim, temb.ptr))
    chk(pkg, L.bla_class_embedding_f32(None, dtab.ptr, classes, dl2.ptr, 2 * n, dim, 0.0, 0, 0, rows.ptr, temb.ptr))
    t_last = -1
    for i in range(S - 1, -1, -1):
        t, t_prev = ts[i], ts[i - 1] if i else -1
        chk(pkg, L.bla_unet_forward_f32(h, None, x2.ptr, temb.ptr, None))
        chk(pkg, L.bla_diffusion_to_eps_f32(d, None, out, x2.ptr, None, t, 2 * n, UNET_F))
        chk(pkg, L.bla_diffusion_guided_dpmpp_step_f32(d, None, x2.ptr, x2.ptr + 4 * n * UNET_F, out, out + 4 * n * UNET_F, s, hist.ptr, n, UNET_F, t_last, t,
                                                       t_prev, 1, dim, temb.ptr, dtab.ptr, classes, rows.ptr))
        t_last = t
    assert x2.numpy()[:n].tobytes() == as_v.tobytes()
    set_all(pkg, L, d, EPS)
    assert guided().tobytes() == before.tobytes()
    chk(pkg, L.bla_diffusion_destroy(d)); chk(pkg, L.bla_unet_destroy(h))


# ---- 8: the example program ------------------------------------------------------------------------------------------------------------------

def test_example_objective(pkg, tmp_path):
    pkg.build_native()
    subprocess.check_call(["make", "-s", "-C", EX, "cifar_unet_gpu"])
    (tmp_path / "data" / "cifar").mkdir(parents=True)
    recs = np.random.default_rng(13).integers(0, 256, (16, 3073), dtype=np.uint8)
    recs[:, 0] = np.arange(16) % 10
    recs.tofile(tmp_path / "data" / "cifar" / "data_batch_1.bin")
    recs[:8].tofile(tmp_path / "data" / "cifar" / "test_batch.bin")
    base = {"BLA_DIFFUSION_STEPS": "50", "BLA_UNET_WEIGHTS": str(tmp_path / "w")}
    r = run_program(["fit", "1", "8"], tmp_path, dict(base, BLA_UNET_SCHEDULE="cosine", BLA_UNET_PREDICT="v", BLA_UNET_MIN_SNR="5", BLA_UNET_LOG_EVERY="1"), timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "w" / "objective.txt").read_text() == "schedule=cosine predict=v min_snr=5\n"
    losses = [float(l.split("Avg loss:")[1]) for l in r.stdout.splitlines() if "Avg loss:" in l]
    assert len(losses) == 2 and all(math.isfinite(v) and v > 0 for v in losses), r.stdout
    # sample and eval take the objective from the file alone
    r = run_program(["sample", "2", str(tmp_path / "s")], tmp_path, dict(base, BLA_UNET_SAMPLER="dpmpp", BLA_UNET_SAMPLE_STEPS="4"), timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert all(bmp_ok(open(tmp_path / "s" / f"sample_{i:04d}.bmp", "rb").read()) for i in range(2))
    r = run_program(["eval"], tmp_path, dict(base, BLA_UNET_BATCH="4", BLA_UNET_EVAL_STEPS="3"), timeout=900)
    assert r.returncode == 0 and "Bits/dim:" in r.stdout, r.stdout + r.stderr
    r = run_program(["sample", "2", str(tmp_path / "s2")], tmp_path, dict(base, BLA_UNET_PREDICT="eps", BLA_UNET_SAMPLER="dpmpp", BLA_UNET_SAMPLE_STEPS="4"))
    assert r.returncode == 1 and "objective.txt" in r.stderr and not (tmp_path / "s2").exists(), r.stdout + r.stderr
    # without an option, in a fresh directory: no objective file
    r = run_program(["fit", "1", "16"], tmp_path, {"BLA_DIFFUSION_STEPS": "50", "BLA_UNET_WEIGHTS": str(tmp_path / "plain")}, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "plain" / "output_conv.csv").exists() and not (tmp_path / "plain" / "objective.txt").exists()
    # and into the directory of the objective run: the set it overwrites is an eps model now, so the file beside it goes
    r = run_program(["fit", "1", "16"], tmp_path, base, timeout=900)
    assert r.returncode == 0 and not (tmp_path / "w" / "objective.txt").exists(), r.stdout + r.stderr
