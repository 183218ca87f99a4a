#!/usr/bin/env python3
"""DDPM training and sampling on the reference's U-Net (model/cifar_unet.c:26-37 constants) at batch B: what one `fit` pass costs against the bare
forward + backward, what each of its added kernels costs (noising, dropout draw, loss, Adam), Adam's HBM rate on the full parameter bucket, the
sampler step's share of one sampler step, and images/s of bla_unet_sample_f32 at T steps.  Device events on the library's stream.
usage: diffusion_bench.py [--batch 64] [--iters 20] [--steps 1000]"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from __graft_entry__ import load_pkg
from inputs import uniform
import test_unet_model as T

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64); ap.add_argument("--iters", type=int, default=20); ap.add_argument("--steps", type=int, default=1000)
a = ap.parse_args()
bla = load_pkg(); bla.init(0); L = bla.lib(); chk = bla.native.check
cfg = dict(image_h=32, image_w=32, in_channels=3, dims=[128, 256, 256, 256], time_dim=512, kernel=3, group_size=32, key_dim=16)
B, F, dim = a.batch, 3 * 32 * 32, 512
st = L.bla_default_stream()
ev = [C.c_void_p() for _ in range(8)]
for e in ev: chk(L.bla_event_create(C.byref(e)))

h, tensors = T.build(bla, cfg, B)
_, n = T.load_params(bla, h, tensors, cfg)
d = C.c_void_p(); chk(L.bla_diffusion_create(C.byref(d), a.steps, 1e-4, 0.02))
x0 = bla.to_device(uniform(1, (B, F), -1, 1, np.float32))
t, eps, xt, temb = bla.empty((B,), np.int32), bla.empty((B, F)), bla.empty((B, F)), bla.empty((B, dim))
drop = bla.empty((L.bla_unet_dropout_count(h),), np.uint8)
m, v, acc = bla.zeros((n,)), bla.zeros((n,)), bla.zeros((1,), np.float64)
P, G = L.bla_unet_params(h), L.bla_unet_grads(h)
step = [0]

parts = {
    "noise": lambda p: chk(L.bla_diffusion_noise_f32(d, st, x0.ptr, B, F, dim, 42, p, t.ptr, eps.ptr, xt.ptr, temb.ptr)),
    "dropout_draw": lambda p: chk(L.bla_rand_bernoulli_u8(st, drop.ptr, drop.shape[0], 0.1, 42, p << 32)),
    "forward": lambda p: chk(L.bla_unet_forward_f32(h, st, xt.ptr, temb.ptr, drop.ptr)),
    "backward": lambda p: chk(L.bla_unet_backward_f32(h, st, eps.ptr)),
    "loss": lambda p: chk(L.bla_mse_accumulate_f32(st, L.bla_unet_output(h), eps.ptr, B * F, acc.ptr)),
    "adam": lambda p: (step.__setitem__(0, step[0] + 1), chk(L.bla_adam_f32(st, P, G, m.ptr, v.ptr, n, 2e-4, 0.9, 0.999, 1e-8, 0.0, 1.0 / B, step[0]))),
}
names = list(parts)


def ms(e0, e1):
    r = C.c_float(); chk(L.bla_event_elapsed_ms(e0, e1, C.byref(r))); return r.value


for p in range(3):                                          # warm-up: code objects, workspaces
    for k in names: parts[k](p)
bla.sync()
# (1) the pass, each part bracketed by events
acc_ms = dict.fromkeys(names, 0.0); whole = 0.0
for p in range(a.iters):
    chk(L.bla_event_record(ev[0], st))
    for i, k in enumerate(names):
        parts[k](p); chk(L.bla_event_record(ev[1 + i], st))
    bla.sync()
    prev = ev[0]
    for i, k in enumerate(names):
        acc_ms[k] += ms(prev, ev[1 + i]); prev = ev[1 + i]
    whole += ms(ev[0], ev[len(names)])
per = {k: acc_ms[k] / a.iters for k in names}
pass_ms = whole / a.iters
fb = per["forward"] + per["backward"]
extra = per["noise"] + per["dropout_draw"] + per["loss"] + per["adam"]
# (2) Adam alone, back to back
chk(L.bla_event_record(ev[0], st))
for _ in range(a.iters): parts["adam"](0)
chk(L.bla_event_record(ev[1], st)); bla.sync()
adam_us = ms(ev[0], ev[1]) / a.iters * 1e3
# (3) the sampler step against one sampler step (forward without dropout + step)
chk(L.bla_event_record(ev[0], st))
for _ in range(a.iters): chk(L.bla_unet_forward_f32(h, st, xt.ptr, temb.ptr, None))
chk(L.bla_event_record(ev[1], st))
for i in range(a.iters): chk(L.bla_diffusion_step_f32(d, st, xt.ptr, L.bla_unet_output(h), B, F, a.steps // 2, 42, dim, temb.ptr))
chk(L.bla_event_record(ev[2], st)); bla.sync()
fwd_ms, step_us = ms(ev[0], ev[1]) / a.iters, ms(ev[1], ev[2]) / a.iters * 1e3
# (4) the whole sampler
chk(L.bla_rand_normal_f32(st, xt.ptr, B * F, 0.0, 1.0, 7, 0)); chk(L.bla_unet_sample_f32(h, d, st, xt.ptr, 7)); bla.sync()   # eager first run (workspace)
chk(L.bla_rand_normal_f32(st, xt.ptr, B * F, 0.0, 1.0, 8, 0))
chk(L.bla_event_record(ev[0], st)); chk(L.bla_unet_sample_f32(h, d, st, xt.ptr, 8)); chk(L.bla_event_record(ev[1], st)); bla.sync()
sample_s = ms(ev[0], ev[1]) / 1e3
assert np.isfinite(xt.numpy()).all()
res = {
    "batch": B, "params": n, "pass_ms": round(pass_ms, 3), "forward_backward_ms": round(fb, 3), "pass_over_forward_backward": round(pass_ms / fb, 4),
    "added_kernels_ms": round(extra, 4), "parts_ms": {k: round(v, 4) for k, v in per.items()},
    "adam_us": round(adam_us, 1), "adam_TBps": round(28.0 * n / (adam_us * 1e-6) / 1e12, 2),
    "sampler_forward_ms": round(fwd_ms, 3), "sampler_step_us": round(step_us, 2), "step_share_of_sampler_step": round(step_us * 1e-3 / (fwd_ms + step_us * 1e-3), 5),
    "sample_steps": a.steps, "sample_seconds": round(sample_s, 3), "sample_images_per_s": round(B / sample_s, 2),
}
print(json.dumps(res), flush=True)
chk(L.bla_diffusion_destroy(d)); chk(L.bla_unet_destroy(h))
