#!/usr/bin/env python3
"""The training objectives (cosine schedule, v-prediction, Min-SNR weights) on the reference's U-Net (model/cifar_unet.c:26-37 constants) at batch
--batch, device events on the library's stream, every group from the same build in the same process and alternating, the median of --reps repeats with
their spread (min .. max): (a) each new kernel on its own; (b) bla_diffusion_loss_f32 beside the pair it replaces in fit (bla_mse_accumulate_f32's
one-workgroup reduction + the seed kernel inside bla_unet_backward_f32; the seed kernel has no entry of its own, so by events only a stand-in is timed
here, bla_diffusion_loss_f32 with the gradient alone -- unet_loss_grad_kernel's own time is the one in the kernel trace of the fit passes of (d),
profiles/r10_objective_kernel_stats.csv); (c) one DDIM and one DPM-Solver++ sampler step, forward pass included, with the prediction set
to v beside eps on the same weights; (d) one fit pass with cosine + v + gamma 5 beside the default pass (the launches of examples/cifar_unet_gpu.c
`fit`, which this change leaves as they were).
usage: objective_bench.py [--batch 64] [--reps 7] [--steps 1000]"""
import argparse, ctypes as C, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from __graft_entry__ import load_pkg
import test_unet_model as T

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64); ap.add_argument("--reps", type=int, default=7); ap.add_argument("--steps", type=int, default=1000)
a = ap.parse_args()
bla = load_pkg(); bla.init(0); L = bla.lib(); chk = bla.native.check
cfg = dict(image_h=32, image_w=32, in_channels=3, dims=[128, 256, 256, 256], time_dim=512, kernel=3, group_size=32, key_dim=16)
B, F, dim = a.batch, 3 * 32 * 32, 512
EPS, V = 0, 2
st = L.bla_default_stream()
ev = [C.c_void_p() for _ in range(2)]
for e in ev: chk(L.bla_event_create(C.byref(e)))


def timed_ms(fn, inner=1):
    chk(L.bla_event_record(ev[0], st))
    for _ in range(inner): fn()
    chk(L.bla_event_record(ev[1], st)); bla.sync()
    r = C.c_float(); chk(L.bla_event_elapsed_ms(ev[0], ev[1], C.byref(r))); return r.value / inner


def group(fns, inner=1, scale=1.0):
    """{name: [median, min, max]} of --reps repeats of each function, the functions taking turns within every repeat"""
    for fn in fns.values(): fn()                              # warm-up
    bla.sync()
    got = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, fn in fns.items(): got[k].append(timed_ms(fn, inner) * scale)
    return {k: [round(float(f(v)), 4) for f in (np.median, np.min, np.max)] for k, v in got.items()}


def diffusion(cosine, pred, gamma):
    d = C.c_void_p()
    if cosine:
        betas = np.zeros(a.steps)
        chk(L.bla_diffusion_cosine_betas(a.steps, 0.008, 0.999, betas.ctypes.data))
        chk(L.bla_diffusion_create_from_betas(C.byref(d), a.steps, betas.ctypes.data))
    else:
        chk(L.bla_diffusion_create(C.byref(d), a.steps, 1e-4, 0.02))
    if pred != EPS or gamma: chk(L.bla_diffusion_set_objective(d, pred, gamma))
    return d


h, tensors = T.build(bla, cfg, B)
T.load_params(bla, h, tensors, cfg)
d_eps, d_v, d_fit = diffusion(False, EPS, 0.0), diffusion(False, V, 0.0), diffusion(True, V, 5.0)
params, drops = L.bla_unet_param_count(h), L.bla_unet_dropout_count(h)
data = bla.empty((B, F)); chk(L.bla_rand_normal_f32(st, data.ptr, B * F, 0.0, 0.5, 1, 0))
x, eps, xt, temb, hist = bla.empty((B, F)), bla.empty((B, F)), bla.empty((B, F)), bla.empty((B, dim)), bla.zeros((B, F))
target, g, weight, dt = bla.empty((B, F)), bla.empty((B, F)), bla.empty((B,)), bla.empty((B,), np.int32)
losses, acc = bla.empty((B,), np.float64), bla.zeros((1,), np.float64)
drop, m1, m2 = bla.empty((drops,), np.uint8), bla.zeros((params,)), bla.zeros((params,))
out = L.bla_unet_output(h)
mid, gap = a.steps // 2, max(1, a.steps // 50)
chk(L.bla_diffusion_noise_f32(d_fit, st, data.ptr, B, F, dim, 42, 0, dt.ptr, eps.ptr, xt.ptr, temb.ptr))
chk(L.bla_unet_forward_f32(h, st, xt.ptr, temb.ptr, None)); bla.sync()

# ---- (a), (b) the kernels ------------------------------------------------------------------------------------------------------------------------------
kernel_us = group({
    "target v": lambda: chk(L.bla_diffusion_target_f32(d_fit, st, data.ptr, eps.ptr, dt.ptr, 0, B, F, target.ptr, weight.ptr)),
    "to_eps v": lambda: chk(L.bla_diffusion_to_eps_f32(d_v, st, g.ptr, xt.ptr, None, mid, B, F)),      # on a scratch buffer: it repeats on its own output
    "loss (g + loss)": lambda: chk(L.bla_diffusion_loss_f32(st, out, target.ptr, weight.ptr, B, F, g.ptr, losses.ptr)),
    "loss (g alone: a stand-in for the seed kernel)": lambda: chk(L.bla_diffusion_loss_f32(st, out, target.ptr, None, B, F, g.ptr, None)),
    "mse_accumulate (one workgroup)": lambda: chk(L.bla_mse_accumulate_f32(st, out, eps.ptr, B * F, acc.ptr)),
}, inner=200, scale=1e3)

# ---- (c) one sampler step, forward pass included: v beside eps on the same weights ------------------------------------------------------------------------
chk(L.bla_time_embedding_f32(st, bla.to_device(np.full(B, mid, np.int32), np.int32).ptr, B, dim, temb.ptr))
chk(L.bla_rand_normal_f32(st, xt.ptr, B * F, 0.0, 1.0, 3, 0))


def sampler_step(d, dpmpp):
    def run():
        chk(L.bla_unet_forward_f32(h, st, xt.ptr, temb.ptr, None))
        chk(L.bla_diffusion_to_eps_f32(d, st, out, xt.ptr, None, mid, B, F))                          # nothing is launched for eps
        if dpmpp: chk(L.bla_diffusion_dpmpp_step_f32(d, st, xt.ptr, out, hist.ptr, B, F, mid + gap, mid, mid - gap, 1, dim, temb.ptr))
        else: chk(L.bla_diffusion_ddim_step_f32(d, st, xt.ptr, out, B, F, mid, mid - gap, 0.0, 1, 42, dim, temb.ptr))
    return run


sampler_step_ms = group({"ddim eps": sampler_step(d_eps, False), "ddim v": sampler_step(d_v, False), "dpmpp eps": sampler_step(d_eps, True),
                         "dpmpp v": sampler_step(d_v, True)}, inner=20)

# ---- (d) one fit pass ----------------------------------------------------------------------------------------------------------------------------------
step = [0]


def fit_pass(objective):
    def run():
        step[0] += 1
        d = d_fit if objective else d_eps
        chk(L.bla_diffusion_noise_f32(d, st, data.ptr, B, F, dim, 42, step[0], dt.ptr, eps.ptr, x.ptr, temb.ptr))
        chk(L.bla_rand_bernoulli_u8(st, drop.ptr, drops, 0.1, 42, step[0] << 32))
        if objective:
            chk(L.bla_diffusion_target_f32(d, st, data.ptr, eps.ptr, dt.ptr, 0, B, F, target.ptr, weight.ptr))
            chk(L.bla_unet_forward_f32(h, st, x.ptr, temb.ptr, drop.ptr))
            chk(L.bla_diffusion_loss_f32(st, out, target.ptr, weight.ptr, B, F, g.ptr, losses.ptr))
            chk(L.bla_unet_backward_from_f32(h, st, g.ptr))
        else:
            chk(L.bla_unet_forward_f32(h, st, x.ptr, temb.ptr, drop.ptr))
            chk(L.bla_unet_backward_f32(h, st, eps.ptr))
            chk(L.bla_mse_accumulate_f32(st, out, eps.ptr, B * F, acc.ptr))
        chk(L.bla_adam_f32(st, L.bla_unet_params(h), L.bla_unet_grads(h), m1.ptr, m2.ptr, params, 1e-6, 0.9, 0.999, 1e-8, 0.0, 1.0 / B, step[0]))
    return run


fit_pass_ms = group({"default": fit_pass(False), "cosine + v + gamma 5": fit_pass(True)}, inner=5)
assert np.isfinite(losses.numpy()).all()
for d in (d_eps, d_v, d_fit): chk(L.bla_diffusion_destroy(d))
chk(L.bla_unet_destroy(h))

res = {
    "batch": B, "steps": a.steps, "reps": a.reps, "format": "[median, min, max]",
    "kernel_us": kernel_us, "kernel_bytes": {"target v": 12 * B * F, "to_eps v": 12 * B * F, "loss (g + loss)": 12 * B * F},
    "sampler_step_ms": sampler_step_ms,
    "sampler_step_v_over_eps": {k: round(sampler_step_ms[k + " v"][0] / sampler_step_ms[k + " eps"][0], 4) for k in ("ddim", "dpmpp")},
    "fit_pass_ms": fit_pass_ms, "fit_pass_objective_over_default": round(fit_pass_ms["cosine + v + gamma 5"][0] / fit_pass_ms["default"][0], 4),
}
print(json.dumps(res), flush=True)
