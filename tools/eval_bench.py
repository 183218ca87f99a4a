#!/usr/bin/env python3
"""Held-out evaluation on the reference's U-Net (model/cifar_unet.c:26-37 constants) at batch --batch, device events on the library's stream: one
evaluation step (bla_diffusion_noise_at_f32 + forward without dropout + bla_diffusion_vlb_terms_f32, what bla_unet_evaluate_f32 issues per timestep)
against the bare forward pass of the same run, alternating; the two added launches, the prior term and fit's loss kernel on the same bytes back to
back; and a whole bla_unet_evaluate_f32 + prior of --terms KL terms on synthetic records.  --profile: only warm-up and --iters evaluation steps, for
a kernel trace of its own.
usage: eval_bench.py [--batch 64] [--iters 20] [--steps 1000] [--terms 50] [--profile]"""
import argparse, ctypes as C, json, math, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from __graft_entry__ import load_pkg
import test_unet_model as T

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64); ap.add_argument("--iters", type=int, default=20); ap.add_argument("--steps", type=int, default=1000)
ap.add_argument("--terms", type=int, default=50); ap.add_argument("--profile", action="store_true")
a = ap.parse_args()
bla = load_pkg(); bla.init(0); L = bla.lib(); chk = bla.native.check
cfg = dict(image_h=32, image_w=32, in_channels=3, dims=[128, 256, 256, 256], time_dim=512, kernel=3, group_size=32, key_dim=16)
B, F, dim = a.batch, 3 * 32 * 32, 512
st = L.bla_default_stream()
ev = [C.c_void_p() for _ in range(2)]
for e in ev: chk(L.bla_event_create(C.byref(e)))


def timed_ms(fn, reps=1):
    chk(L.bla_event_record(ev[0], st))
    for _ in range(reps): fn()
    chk(L.bla_event_record(ev[1], st)); bla.sync()
    r = C.c_float(); chk(L.bla_event_elapsed_ms(ev[0], ev[1], C.byref(r))); return r.value / reps


h, tensors = T.build(bla, cfg, B)
T.load_params(bla, h, tensors, cfg)
d = C.c_void_p(); chk(L.bla_diffusion_create(C.byref(d), a.steps, 1e-4, 0.02))
pix = np.random.default_rng(1).integers(0, 256, (B, F))
x0 = bla.to_device(((pix - 127.5) / 127.5).astype(np.float32))
eps, xt, temb = bla.empty((B, F)), bla.empty((B, F)), bla.empty((B, dim))
terms, sqerr, prior, acc = bla.empty((B,), np.float64), bla.empty((B,), np.float64), bla.empty((B,), np.float64), bla.zeros((1,), np.float64)
out = L.bla_unet_output(h)
mid = a.steps // 2


def noise_at(t): chk(L.bla_diffusion_noise_at_f32(d, st, x0.ptr, B, F, dim, None, t, 42, (t + 1) << 32, eps.ptr, xt.ptr, temb.ptr))
def forward(): chk(L.bla_unet_forward_f32(h, st, xt.ptr, temb.ptr, None))
def vlb(t): chk(L.bla_diffusion_vlb_terms_f32(d, st, x0.ptr, xt.ptr, eps.ptr, out, None, t, B, F, terms.ptr, sqerr.ptr))
def eval_step(t): noise_at(t); forward(); vlb(t)


for t in (mid, 0, mid): eval_step(t)                         # warm-up: code objects, workspaces
bla.sync()
if a.profile:
    for i in range(a.iters): eval_step(0 if i % 2 else mid)
    bla.sync(); sys.exit(0)
fwd, step, step0 = [], [], []
for i in range(a.iters):                                     # alternating, so drift of the clock falls on all alike
    fwd.append(timed_ms(forward)); step.append(timed_ms(lambda: eval_step(mid))); step0.append(timed_ms(lambda: eval_step(0)))
us = lambda fn: round(timed_ms(fn, 50) * 1e3, 2)
res = {"batch": B, "steps": a.steps, "forward_ms": round(float(np.median(fwd)), 3), "eval_step_ms": round(float(np.median(step)), 3),
       "eval_step_t0_ms": round(float(np.median(step0)), 3)}
res["eval_step_over_forward"] = round(res["eval_step_ms"] / res["forward_ms"], 4)
res["noise_at_us"] = us(lambda: noise_at(mid)); res["vlb_terms_us"] = us(lambda: vlb(mid)); res["vlb_terms_t0_us"] = us(lambda: vlb(0))
res["prior_kl_us"] = us(lambda: chk(L.bla_diffusion_prior_kl_f32(d, st, x0.ptr, B, F, prior.ptr)))
res["mse_accumulate_us"] = us(lambda: chk(L.bla_mse_accumulate_f32(st, out, eps.ptr, B * F, acc.ptr)))
K = min(a.terms, a.steps - 1)
ts = (C.c_int * (K + 1))(); chk(L.bla_diffusion_eval_timesteps(d, K, ts))
all_terms = bla.empty((K + 1, B), np.float64)


def evaluate():
    chk(L.bla_unet_evaluate_f32(h, d, st, x0.ptr, ts, K + 1, 42, 0, None, 0, None, all_terms.ptr, None))
    chk(L.bla_diffusion_prior_kl_f32(d, st, x0.ptr, B, F, prior.ptr))


evaluate(); bla.sync()
sec = timed_ms(evaluate) / 1e3
tt = all_terms.numpy()
nats = prior.numpy() + tt[0] + tt[1:].sum(0) * (a.steps - 1) / max(K, 1)
res.update({"kl_terms": K, "evaluate_seconds": round(sec, 4), "images_per_s": round(B / sec, 2),
            "bits_per_dim_synthetic_records_untrained_weights": round(float(nats.mean() / (F * math.log(2))), 4)})
chk(L.bla_diffusion_destroy(d)); chk(L.bla_unet_destroy(h))
print(json.dumps(res), flush=True)
