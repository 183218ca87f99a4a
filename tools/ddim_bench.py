#!/usr/bin/env python3
"""Few-step DDIM sampling and the EMA of the weights on the reference's U-Net (model/cifar_unet.c:26-37 constants), device events on the library's
stream: (a) one `fit` pass (noise, dropout draw, forward, backward, loss, Adam) without and with the EMA update after it, alternating, and the EMA
alone back to back; (b) a sampler forward pass, the ancestral step and the DDIM step (eta 0 and 1) back to back, images/s of the ancestral sampler at
T = --steps (the reference point) and of DDIM at each S of --sample-steps with eta 0 and 1, at batch --batch; (c) guided DDIM at n = --n images
(model batch 2n) and S = --guided-steps.
usage: ddim_bench.py [--batch 64] [--iters 20] [--steps 1000] [--sample-steps 250,50,20] [--n 64] [--guided-steps 50]"""
import argparse, ctypes as C, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from __graft_entry__ import load_pkg
from inputs import uniform
import test_unet_model as T

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64); ap.add_argument("--iters", type=int, default=20); ap.add_argument("--steps", type=int, default=1000)
ap.add_argument("--sample-steps", default="250,50,20"); ap.add_argument("--n", type=int, default=64); ap.add_argument("--guided-steps", type=int, default=50)
a = ap.parse_args()
bla = load_pkg(); bla.init(0); L = bla.lib(); chk = bla.native.check
cfg = dict(image_h=32, image_w=32, in_channels=3, dims=[128, 256, 256, 256], time_dim=512, kernel=3, group_size=32, key_dim=16)
B, F, dim, K = a.batch, 3 * 32 * 32, 512, 10
st = L.bla_default_stream()
ev = [C.c_void_p() for _ in range(2)]
for e in ev: chk(L.bla_event_create(C.byref(e)))


def timed_ms(fn, reps=1):
    chk(L.bla_event_record(ev[0], st))
    for _ in range(reps): fn()
    chk(L.bla_event_record(ev[1], st)); bla.sync()
    r = C.c_float(); chk(L.bla_event_elapsed_ms(ev[0], ev[1], C.byref(r))); return r.value / reps


# ---- (a) training passes ------------------------------------------------------------------------------------------------------------------
h, tensors = T.build(bla, cfg, B)
_, n = T.load_params(bla, h, tensors, cfg)
d = C.c_void_p(); chk(L.bla_diffusion_create(C.byref(d), a.steps, 1e-4, 0.02))
x0 = bla.to_device(uniform(1, (B, F), -1, 1, np.float32))
t, eps, xt, temb = bla.empty((B,), np.int32), bla.empty((B, F)), bla.empty((B, F)), bla.empty((B, dim))
drop = bla.empty((L.bla_unet_dropout_count(h),), np.uint8)
m, v, acc = bla.zeros((n,)), bla.zeros((n,)), bla.zeros((1,), np.float64)
P, G = L.bla_unet_params(h), L.bla_unet_grads(h)
ema = bla.empty((n,)); chk(L.bla_memcpy_d2d(ema.ptr, P, 4 * n, st))
step = [0]


def fit_pass(p, with_ema):
    chk(L.bla_diffusion_noise_f32(d, st, x0.ptr, B, F, dim, 42, p, t.ptr, eps.ptr, xt.ptr, temb.ptr))
    chk(L.bla_rand_bernoulli_u8(st, drop.ptr, drop.shape[0], 0.1, 42, p << 32))
    chk(L.bla_unet_forward_f32(h, st, xt.ptr, temb.ptr, drop.ptr)); chk(L.bla_unet_backward_f32(h, st, eps.ptr))
    chk(L.bla_mse_accumulate_f32(st, L.bla_unet_output(h), eps.ptr, B * F, acc.ptr))
    step[0] += 1
    chk(L.bla_adam_f32(st, P, G, m.ptr, v.ptr, n, 2e-4, 0.9, 0.999, 1e-8, 0.0, 1.0 / B, step[0]))
    if with_ema:
        chk(L.bla_ema_f32(st, ema.ptr, P, n, min(0.9999, (1 + p) / (10 + p))))


for p in range(3): fit_pass(p, True)                         # warm-up: code objects, workspaces
bla.sync()
plain, with_ema = [], []
for i in range(a.iters):                                    # alternating, so drift of the clock falls on both alike
    plain.append(timed_ms(lambda: fit_pass(3 + 2 * i, False)))
    with_ema.append(timed_ms(lambda: fit_pass(4 + 2 * i, True)))
ema_us = timed_ms(lambda: chk(L.bla_ema_f32(st, ema.ptr, P, n, 0.9999)), 50) * 1e3

# ---- (b) samplers at batch B on the same model --------------------------------------------------------------------------------------------
x = bla.empty((B, F)); out = L.bla_unet_output(h)
dw = C.c_void_p(); chk(L.bla_diffusion_create(C.byref(dw), 2, 1e-4, 0.02))
chk(L.bla_rand_normal_f32(st, x.ptr, B * F, 0.0, 1.0, 7, 0))
chk(L.bla_unet_sample_f32(h, dw, st, x.ptr, 7)); chk(L.bla_unet_sample_ddim_f32(h, d, st, x.ptr, 1, 1.0, 0, 7)); bla.sync()   # warm-up, d's workspace
t500 = bla.to_device(np.full(B, a.steps // 2, np.int32), np.int32)
chk(L.bla_time_embedding_f32(st, t500.ptr, B, dim, temb.ptr))
chk(L.bla_rand_normal_f32(st, xt.ptr, B * F, 0.0, 1.0, 3, 0))
fwd_ms = timed_ms(lambda: chk(L.bla_unet_forward_f32(h, st, xt.ptr, temb.ptr, None)), a.iters)
mid, gap = a.steps // 2, max(1, a.steps // 50)                # t -> t - gap: the spacing of S = 50
anc_step_us = timed_ms(lambda: chk(L.bla_diffusion_step_f32(d, st, xt.ptr, out, B, F, mid, 42, dim, temb.ptr)), 50) * 1e3
ddim_step_us = {eta: timed_ms(lambda: chk(L.bla_diffusion_ddim_step_f32(d, st, xt.ptr, out, B, F, mid, mid - gap, eta, 1, 42, dim, temb.ptr)), 50) * 1e3
                for eta in (0.0, 1.0)}


def sampler_s(fn, seed):
    chk(L.bla_rand_normal_f32(st, x.ptr, B * F, 0.0, 1.0, seed, 0))
    s = timed_ms(fn) / 1e3
    assert np.isfinite(x.numpy()).all()
    return s


anc_s = sampler_s(lambda: chk(L.bla_unet_sample_f32(h, d, st, x.ptr, 8)), 8)
ddim = []
for S in [int(s) for s in a.sample_steps.split(",") if s]:
    for eta in (0.0, 1.0):
        s = sampler_s(lambda: chk(L.bla_unet_sample_ddim_f32(h, d, st, x.ptr, S, eta, 0, 8)), 8)
        ddim.append({"S": S, "eta": eta, "seconds": round(s, 4), "images_per_s": round(B / s, 2), "ms_per_step": round(s * 1e3 / S, 4)})
chk(L.bla_diffusion_destroy(d)); chk(L.bla_diffusion_destroy(dw)); chk(L.bla_unet_destroy(h))

# ---- (c) guided DDIM at model batch 2n ----------------------------------------------------------------------------------------------------
N = a.n
hg, tg = T.build(bla, cfg, 2 * N)
T.load_params(bla, hg, tg, cfg)
d = C.c_void_p(); chk(L.bla_diffusion_create(C.byref(d), a.steps, 1e-4, 0.02))
table = bla.to_device(uniform(2, (K + 1, dim), -0.1, 0.1, np.float32))
lab = bla.to_device((np.arange(N) % K).astype(np.int32), np.int32)
xg = bla.empty((N, F))
chk(L.bla_rand_normal_f32(st, xg.ptr, N * F, 0.0, 1.0, 7, 0)); chk(L.bla_unet_sample_guided_ddim_f32(hg, d, st, xg.ptr, table.ptr, K, lab.ptr, 3.0, 1, 0.0, 0, 7))
bla.sync()                                                  # warm-up
chk(L.bla_rand_normal_f32(st, xg.ptr, N * F, 0.0, 1.0, 8, 0))
guided_s = timed_ms(lambda: chk(L.bla_unet_sample_guided_ddim_f32(hg, d, st, xg.ptr, table.ptr, K, lab.ptr, 3.0, a.guided_steps, 0.0, 0, 8))) / 1e3
assert np.isfinite(xg.numpy()).all()
chk(L.bla_diffusion_destroy(d)); chk(L.bla_unet_destroy(hg))

pu, pe = float(np.median(plain)), float(np.median(with_ema))
anc_step_ms = anc_s * 1e3 / a.steps
res = {
    "batch": B, "params": n, "steps": a.steps,
    "fit_pass_ms": round(pu, 3), "fit_pass_ema_ms": round(pe, 3), "ema_over_plain": round(pe / pu, 4),
    "ema_us_back_to_back": round(ema_us, 2), "ema_TBps": round(12 * n / (ema_us * 1e-6) / 1e12, 2),
    "sampler_forward_ms": round(fwd_ms, 3), "ancestral_step_us": round(anc_step_us, 2),
    "ddim_step_us_eta0": round(ddim_step_us[0.0], 2), "ddim_step_us_eta1": round(ddim_step_us[1.0], 2),
    "ancestral_sample_seconds": round(anc_s, 3), "ancestral_images_per_s": round(B / anc_s, 2), "ancestral_ms_per_step": round(anc_step_ms, 4),
    "ddim": ddim,
    "ddim_ms_per_step_over_ancestral": round(max(r["ms_per_step"] for r in ddim) / anc_step_ms, 4) if ddim else None,
    "n": N, "model_batch": 2 * N, "guided_sample_steps": a.guided_steps, "guided_ddim_seconds": round(guided_s, 4),
    "guided_ddim_images_per_s": round(N / guided_s, 2),
}
print(json.dumps(res), flush=True)
