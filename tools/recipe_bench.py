#!/usr/bin/env python3
"""The DDPM training recipe on the reference's U-Net (model/cifar_unet.c:26-37 constants), device events on the library's stream: (a) one `fit` pass
without the options (noise, dropout draw, forward, backward, loss, Adam) and with all four (noise-gather over a shuffled, flipped index; sum of squares,
clip scale, scaled Adam; warmed-up learning rate), alternating, medians; (b) back to back: the sum of squares on the parameter bucket beside the EMA
on the same bucket (time and achieved bandwidth), the gather-noise launch beside the plain one, the permutation at n = --records; (c) what the recipe
buys: the 4-image loop of tests/test_diffusion_gpu.py::test_training_loss_falls at lr 1e-4 and 1e-3, with and without clipping at 1.0 plus a 20-pass
warm-up (first loss, mean of passes 80-99).  --skip-loops leaves (c) out (for a profiler run).
usage: recipe_bench.py [--batch 64] [--iters 20] [--steps 1000] [--records 50000] [--skip-loops]"""
import argparse, ctypes as C, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from __graft_entry__ import load_pkg
from inputs import uniform
import test_unet_model as T

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64); ap.add_argument("--iters", type=int, default=20); ap.add_argument("--steps", type=int, default=1000)
ap.add_argument("--records", type=int, default=50000); ap.add_argument("--skip-loops", action="store_true")
a = ap.parse_args()
bla = load_pkg(); bla.init(0); L = bla.lib(); chk = bla.native.check
cfg = dict(image_h=32, image_w=32, in_channels=3, dims=[128, 256, 256, 256], time_dim=512, kernel=3, group_size=32, key_dim=16)
B, F, dim, R = a.batch, 3 * 32 * 32, 512, a.records
st = L.bla_default_stream()
ev = [C.c_void_p() for _ in range(2)]
for e in ev: chk(L.bla_event_create(C.byref(e)))


def timed_ms(fn, reps=1):
    chk(L.bla_event_record(ev[0], st))
    for _ in range(reps): fn()
    chk(L.bla_event_record(ev[1], st)); bla.sync()
    r = C.c_float(); chk(L.bla_event_elapsed_ms(ev[0], ev[1], C.byref(r))); return r.value / reps


# ---- (a) a fit pass without and with the four options ---------------------------------------------------------------------------------------
h, tensors = T.build(bla, cfg, B)
_, n = T.load_params(bla, h, tensors, cfg)
d = C.c_void_p(); chk(L.bla_diffusion_create(C.byref(d), a.steps, 1e-4, 0.02))
data = bla.empty((R, F)); chk(L.bla_rand_normal_f32(st, data.ptr, R * F, 0.0, 0.5, 3, 0))          # the whole set resident, as fit holds it
t, eps, xt, temb = bla.empty((B,), np.int32), bla.empty((B, F)), bla.empty((B, F)), bla.empty((B, dim))
drop = bla.empty((L.bla_unet_dropout_count(h),), np.uint8)
m, v, acc = bla.zeros((n,)), bla.zeros((n,)), bla.zeros((1,), np.float64)
perm, keys = bla.empty((R,), np.uint32), bla.empty((R,), np.uint32)
sumsq, scratch, scale, norm = bla.zeros((1,), np.float64), bla.empty((1024,), np.float64), bla.empty((1,)), bla.empty((1,))
P, G = L.bla_unet_params(h), L.bla_unet_grads(h)
per_epoch = R // B
chk(L.bla_rand_permutation_u32(st, perm.ptr, keys.ptr, R, 42, 1 << 31))
step = [0]


def fit_pass(p, recipe):
    k = p % per_epoch
    if recipe:
        chk(L.bla_diffusion_noise_gather_f32(d, st, data.ptr, R, perm.ptr + 4 * k * B, 1, 32, None, None, B, F, dim, 42, p, t.ptr, eps.ptr, xt.ptr, temb.ptr, None))
    else:
        chk(L.bla_diffusion_noise_f32(d, st, data.ptr + 4 * k * B * F, B, F, dim, 42, p, t.ptr, eps.ptr, xt.ptr, temb.ptr))
    chk(L.bla_rand_bernoulli_u8(st, drop.ptr, drop.shape[0], 0.1, 42, p << 32))
    chk(L.bla_unet_forward_f32(h, st, xt.ptr, temb.ptr, drop.ptr)); chk(L.bla_unet_backward_f32(h, st, eps.ptr))
    chk(L.bla_mse_accumulate_f32(st, L.bla_unet_output(h), eps.ptr, B * F, acc.ptr))
    step[0] += 1
    if recipe:
        lr = 2e-4 * min(1.0, (p + 1) / 5000)
        chk(L.bla_memset(sumsq.ptr, 0, 8, st))
        chk(L.bla_sumsq_accumulate_f32(st, G, n, sumsq.ptr, scratch.ptr))
        chk(L.bla_clip_scale_f32(st, sumsq.ptr, 1.0 / B, 1.0, scale.ptr, norm.ptr))
        chk(L.bla_adam_scaled_f32(st, P, G, m.ptr, v.ptr, n, lr, 0.9, 0.999, 1e-8, 0.0, scale.ptr, step[0]))
    else:
        chk(L.bla_adam_f32(st, P, G, m.ptr, v.ptr, n, 2e-4, 0.9, 0.999, 1e-8, 0.0, 1.0 / B, step[0]))


for p in range(4): fit_pass(p, p % 2 == 1)                  # warm-up: code objects, workspaces, both forms
bla.sync()
plain, recipe = [], []
for i in range(a.iters):                                    # alternating, so drift of the clock falls on both alike
    plain.append(timed_ms(lambda: fit_pass(4 + 2 * i, False)))
    recipe.append(timed_ms(lambda: fit_pass(5 + 2 * i, True)))

# ---- (b) the added kernels back to back ------------------------------------------------------------------------------------------------------
ema = bla.empty((n,)); chk(L.bla_memcpy_d2d(ema.ptr, P, 4 * n, st))
for fn in (lambda: chk(L.bla_ema_f32(st, ema.ptr, P, n, 0.9999)), lambda: chk(L.bla_sumsq_accumulate_f32(st, G, n, sumsq.ptr, scratch.ptr))): fn()
ema_us, sumsq_us = [], []
for _ in range(5):                                          # alternating again
    ema_us.append(timed_ms(lambda: chk(L.bla_ema_f32(st, ema.ptr, P, n, 0.9999)), 50) * 1e3)
    sumsq_us.append(timed_ms(lambda: chk(L.bla_sumsq_accumulate_f32(st, G, n, sumsq.ptr, scratch.ptr)), 50) * 1e3)
noise_us = timed_ms(lambda: chk(L.bla_diffusion_noise_f32(d, st, data.ptr, B, F, dim, 42, 7, t.ptr, eps.ptr, xt.ptr, temb.ptr)), 50) * 1e3
gather_us = timed_ms(lambda: chk(L.bla_diffusion_noise_gather_f32(d, st, data.ptr, R, perm.ptr, 1, 32, None, None, B, F, dim, 42, 7, t.ptr, eps.ptr, xt.ptr, temb.ptr,
                                                                   None)), 50) * 1e3
clip_us = timed_ms(lambda: chk(L.bla_clip_scale_f32(st, sumsq.ptr, 1.0 / B, 1.0, scale.ptr, norm.ptr)), 50) * 1e3
perm_ms = float(np.median([timed_ms(lambda: chk(L.bla_rand_permutation_u32(st, perm.ptr, keys.ptr, R, 42, (e << 32) + (1 << 31)))) for e in range(1, 6)]))
chk(L.bla_diffusion_destroy(d)); chk(L.bla_unet_destroy(h))

# ---- (c) what the recipe buys: the 4-image loop of test_training_loss_falls -----------------------------------------------------------------
loops = []
if not a.skip_loops:
    import test_diffusion_gpu as D
    for lr in (1e-4, 1e-3):
        for with_recipe in (False, True):
            tr = D.Trainer(bla, L, 4, float(np.float32(lr)))
            x0 = bla.to_device(uniform(51, (4, D.F), -1, 1, np.float32))
            losses, norms = [], []
            for pas in range(100):
                losses.append(tr.grads(x0, pas))
                tr.step += 1
                if with_recipe:
                    chk(L.bla_memset(sumsq.ptr, 0, 8, None))
                    chk(L.bla_sumsq_accumulate_f32(None, L.bla_unet_grads(tr.h), tr.n, sumsq.ptr, scratch.ptr))
                    chk(L.bla_clip_scale_f32(None, sumsq.ptr, 1.0 / 4, 1.0, scale.ptr, norm.ptr))
                    chk(L.bla_adam_scaled_f32(None, L.bla_unet_params(tr.h), L.bla_unet_grads(tr.h), tr.m.ptr, tr.v.ptr, tr.n,
                                              float(np.float32(lr * min(1.0, (pas + 1) / 20))), 0.9, 0.999, 1e-8, 0.0, scale.ptr, tr.step))
                    norms.append(float(norm.numpy()[0]))
                else:
                    chk(L.bla_adam_f32(None, L.bla_unet_params(tr.h), L.bla_unet_grads(tr.h), tr.m.ptr, tr.v.ptr, tr.n, tr.lr, 0.9, 0.999, 1e-8, 0.0, 1.0 / 4, tr.step))
            loops.append({"lr": lr, "clip_1.0_warmup_20": with_recipe, "first_loss": round(losses[0], 4), "mean_loss_80_99": round(float(np.mean(losses[80:])), 4),
                          "every_10th": [round(x, 3) for x in losses[::10]], "grad_norm_first_last": [round(norms[0], 3), round(norms[-1], 3)] if norms else None})
            tr.close()

pu, pr = float(np.median(plain)), float(np.median(recipe))
eu, su = float(np.median(ema_us)), float(np.median(sumsq_us))
res = {
    "batch": B, "params": n, "steps": a.steps, "records": R,
    "fit_pass_ms": round(pu, 3), "fit_pass_recipe_ms": round(pr, 3), "recipe_over_plain": round(pr / pu, 4),
    "fit_pass_ms_spread": [round(min(plain), 3), round(max(plain), 3)], "fit_pass_recipe_ms_spread": [round(min(recipe), 3), round(max(recipe), 3)],
    "sumsq_us_back_to_back": round(su, 2), "sumsq_TBps": round(4 * n / (su * 1e-6) / 1e12, 2),
    "ema_us_back_to_back": round(eu, 2), "ema_TBps": round(12 * n / (eu * 1e-6) / 1e12, 2),
    "noise_us": round(noise_us, 2), "noise_gather_us": round(gather_us, 2), "clip_scale_us": round(clip_us, 2),
    "permutation_ms": round(perm_ms, 3), "permutation_compares": R * R,
    "loss_loops": loops,
}
print(json.dumps(res), flush=True)
