#!/usr/bin/env python3
"""Class-conditional DDPM training and classifier-free guided sampling on the reference's U-Net (model/cifar_unet.c:26-37 constants): (a) one
conditional `fit` pass (noise, class embedding, dropout draw, forward, backward, embedding gradient, table gradient, loss, Adam on the parameters and on
the table) against the unconditional pass at the same batch, part by part; (b) the guided step's share of a guided sampler step and images/s of
bla_unet_sample_guided_f32 at n images (model batch 2n) and T steps, beside bla_unet_sample_f32 at batch n.  Device events on the library's stream.
usage: guidance_bench.py [--batch 64] [--iters 20] [--steps 1000] [--n 64]"""
import argparse, ctypes as C, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from __graft_entry__ import load_pkg
from inputs import uniform
import test_unet_model as T

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64); ap.add_argument("--iters", type=int, default=20); ap.add_argument("--steps", type=int, default=1000)
ap.add_argument("--n", type=int, default=64)
a = ap.parse_args()
bla = load_pkg(); bla.init(0); L = bla.lib(); chk = bla.native.check
cfg = dict(image_h=32, image_w=32, in_channels=3, dims=[128, 256, 256, 256], time_dim=512, kernel=3, group_size=32, key_dim=16)
B, F, dim, K = a.batch, 3 * 32 * 32, 512, 10
st = L.bla_default_stream()
ev = [C.c_void_p() for _ in range(16)]
for e in ev: chk(L.bla_event_create(C.byref(e)))


def ms(e0, e1):
    r = C.c_float(); chk(L.bla_event_elapsed_ms(e0, e1, C.byref(r))); return r.value


# ---- (a) training passes ------------------------------------------------------------------------------------------------------------------
h, tensors = T.build(bla, cfg, B)
_, n = T.load_params(bla, h, tensors, cfg)
d = C.c_void_p(); chk(L.bla_diffusion_create(C.byref(d), a.steps, 1e-4, 0.02))
x0 = bla.to_device(uniform(1, (B, F), -1, 1, np.float32))
t, eps, xt, temb = bla.empty((B,), np.int32), bla.empty((B, F)), bla.empty((B, F)), bla.empty((B, dim))
drop = bla.empty((L.bla_unet_dropout_count(h),), np.uint8)
m, v, acc = bla.zeros((n,)), bla.zeros((n,)), bla.zeros((1,), np.float64)
labels = bla.to_device((np.arange(B) % K).astype(np.int32), np.int32)
table, gtable = bla.to_device(uniform(2, (K + 1, dim), -0.1, 0.1, np.float32)), bla.zeros((K + 1, dim))
tm, tv, rows, dtemb = bla.zeros((K + 1, dim)), bla.zeros((K + 1, dim)), bla.empty((B,), np.int32), bla.empty((B, dim))
P, G = L.bla_unet_params(h), L.bla_unet_grads(h)
step = [0]
parts = {
    "noise": lambda p: chk(L.bla_diffusion_noise_f32(d, st, x0.ptr, B, F, dim, 42, p, t.ptr, eps.ptr, xt.ptr, temb.ptr)),
    "class_embedding": lambda p: chk(L.bla_class_embedding_f32(st, table.ptr, K, labels.ptr, B, dim, 0.1, 42, (p << 32) + (1 << 31), rows.ptr, temb.ptr)),
    "dropout_draw": lambda p: chk(L.bla_rand_bernoulli_u8(st, drop.ptr, drop.shape[0], 0.1, 42, p << 32)),
    "forward": lambda p: chk(L.bla_unet_forward_f32(h, st, xt.ptr, temb.ptr, drop.ptr)),
    "backward": lambda p: chk(L.bla_unet_backward_f32(h, st, eps.ptr)),
    "embedding_grad": lambda p: chk(L.bla_unet_embedding_grad_f32(h, st, dtemb.ptr)),
    "table_grad": lambda p: chk(L.bla_class_embedding_grad_f32(st, dtemb.ptr, rows.ptr, B, K, dim, gtable.ptr)),
    "loss": lambda p: chk(L.bla_mse_accumulate_f32(st, L.bla_unet_output(h), eps.ptr, B * F, acc.ptr)),
    "adam": lambda p: (step.__setitem__(0, step[0] + 1), chk(L.bla_adam_f32(st, P, G, m.ptr, v.ptr, n, 2e-4, 0.9, 0.999, 1e-8, 0.0, 1.0 / B, step[0]))),
    "adam_table": lambda p: chk(L.bla_adam_f32(st, table.ptr, gtable.ptr, tm.ptr, tv.ptr, (K + 1) * dim, 2e-4, 0.9, 0.999, 1e-8, 0.0, 1.0 / B, max(step[0], 1))),
}
cond = list(parts)
added = ["class_embedding", "embedding_grad", "table_grad", "adam_table"]
uncond = [k for k in cond if k not in added]

for p in range(3):                                          # warm-up: code objects, workspaces
    for k in cond: parts[k](p)
bla.sync()


def timed(names, iters):
    acc_ms, whole = dict.fromkeys(names, 0.0), 0.0
    for p in range(iters):
        chk(L.bla_event_record(ev[0], st))
        for i, k in enumerate(names):
            parts[k](p); chk(L.bla_event_record(ev[1 + i], st))
        bla.sync()
        prev = ev[0]
        for i, k in enumerate(names):
            acc_ms[k] += ms(prev, ev[1 + i]); prev = ev[1 + i]
        whole += ms(ev[0], ev[len(names)])
    return {k: acc_ms[k] / iters for k in names}, whole / iters


per_u, pass_u = timed(uncond, a.iters)
per_c, pass_c = timed(cond, a.iters)
added_ms = sum(per_c[k] for k in added)
# the embedding gradient alone, back to back (it reads every W_k once per tile of 8 images: 18 x 512 x cout floats, B / 8 times)
chk(L.bla_event_record(ev[0], st))
for _ in range(a.iters): parts["embedding_grad"](0)
chk(L.bla_event_record(ev[1], st)); bla.sync()
emb_us = ms(ev[0], ev[1]) / a.iters * 1e3
chk(L.bla_diffusion_destroy(d)); chk(L.bla_unet_destroy(h))

# ---- (b) guided sampling at model batch 2n ------------------------------------------------------------------------------------------------
N = a.n
hg, tg = T.build(bla, cfg, 2 * N)
T.load_params(bla, hg, tg, cfg)
d = C.c_void_p(); chk(L.bla_diffusion_create(C.byref(d), a.steps, 1e-4, 0.02))
dw = C.c_void_p(); chk(L.bla_diffusion_create(C.byref(dw), 2, 1e-4, 0.02))
x, x2, temb2, rows2 = bla.empty((N, F)), bla.empty((2 * N, F)), bla.empty((2 * N, dim)), bla.empty((2 * N,), np.int32)
lab = bla.to_device((np.arange(N) % K).astype(np.int32), np.int32)
chk(L.bla_rand_normal_f32(st, x2.ptr, 2 * N * F, 0.0, 1.0, 3, 0))
t500, lab2 = bla.to_device(np.full(2 * N, 500, np.int32), np.int32), bla.to_device(np.r_[np.arange(N) % K, np.full(N, K)].astype(np.int32), np.int32)
chk(L.bla_time_embedding_f32(st, t500.ptr, 2 * N, dim, temb2.ptr))
chk(L.bla_class_embedding_f32(st, table.ptr, K, lab2.ptr, 2 * N, dim, 0.0, 0, 0, rows2.ptr, temb2.ptr))
out = L.bla_unet_output(hg)
chk(L.bla_rand_normal_f32(st, x.ptr, N * F, 0.0, 1.0, 7, 0)); chk(L.bla_unet_sample_guided_f32(hg, dw, st, x.ptr, table.ptr, K, lab.ptr, 3.0, 7)); bla.sync()   # warm-up
chk(L.bla_event_record(ev[0], st))
for _ in range(a.iters): chk(L.bla_unet_forward_f32(hg, st, x2.ptr, temb2.ptr, None))
chk(L.bla_event_record(ev[1], st))
for _ in range(a.iters):
    chk(L.bla_diffusion_guided_step_f32(d, st, x2.ptr, x2.ptr + 4 * N * F, out, out + 4 * N * F, 3.0, N, F, a.steps // 2, 42, dim, temb2.ptr, table.ptr, K, rows2.ptr))
chk(L.bla_event_record(ev[2], st)); bla.sync()
gfwd_ms, gstep_us = ms(ev[0], ev[1]) / a.iters, ms(ev[1], ev[2]) / a.iters * 1e3
chk(L.bla_rand_normal_f32(st, x.ptr, N * F, 0.0, 1.0, 8, 0))
chk(L.bla_event_record(ev[0], st)); chk(L.bla_unet_sample_guided_f32(hg, d, st, x.ptr, table.ptr, K, lab.ptr, 3.0, 8)); chk(L.bla_event_record(ev[1], st)); bla.sync()
guided_s = ms(ev[0], ev[1]) / 1e3
assert np.isfinite(x.numpy()).all()
chk(L.bla_diffusion_destroy(d)); chk(L.bla_diffusion_destroy(dw)); chk(L.bla_unet_destroy(hg))
# the unguided sampler at batch n, for comparison
hu, tu = T.build(bla, cfg, N)
T.load_params(bla, hu, tu, cfg)
d = C.c_void_p(); chk(L.bla_diffusion_create(C.byref(d), a.steps, 1e-4, 0.02))
xu = bla.empty((N, F))
chk(L.bla_rand_normal_f32(st, xu.ptr, N * F, 0.0, 1.0, 8, 0))
chk(L.bla_event_record(ev[0], st)); chk(L.bla_unet_sample_f32(hu, d, st, xu.ptr, 8)); chk(L.bla_event_record(ev[1], st)); bla.sync()
unguided_s = ms(ev[0], ev[1]) / 1e3
chk(L.bla_diffusion_destroy(d)); chk(L.bla_unet_destroy(hu))

res = {
    "batch": B, "params": n,
    "uncond_pass_ms": round(pass_u, 3), "cond_pass_ms": round(pass_c, 3), "cond_over_uncond": round(pass_c / pass_u, 4),
    "added_kernels_ms": round(added_ms, 4), "added_share_of_cond_pass": round(added_ms / pass_c, 5),
    "parts_ms_uncond": {k: round(v, 4) for k, v in per_u.items()}, "parts_ms_cond": {k: round(v, 4) for k, v in per_c.items()},
    "embedding_grad_us_back_to_back": round(emb_us, 2),
    "n": N, "model_batch": 2 * N, "guided_forward_ms": round(gfwd_ms, 3), "guided_step_us": round(gstep_us, 2),
    "guided_step_share_of_sampler_step": round(gstep_us * 1e-3 / (gfwd_ms + gstep_us * 1e-3), 5),
    "sample_steps": a.steps, "guided_sample_seconds": round(guided_s, 3), "guided_images_per_s": round(N / guided_s, 2),
    "unguided_sample_seconds": round(unguided_s, 3), "unguided_images_per_s": round(N / unguided_s, 2),
}
print(json.dumps(res), flush=True)
