#!/usr/bin/env python3
"""DPM-Solver++(2M) beside DDIM on the reference's U-Net (model/cifar_unet.c:26-37 constants), device events on the library's stream, every pair from
the same build in the same process and alternating, the median of --reps repeats with their spread (min .. max): (a) the two step kernels back to
back; (b) one sampler step of each, forward pass included; (c) images/s of the new loop at each S of --dpmpp-steps beside DDIM's at each S of
--ddim-steps, at batch --batch; (d) the guided pair at n = --n images (model batch 2n) and S = --guided-steps.
usage: dpmpp_bench.py [--batch 64] [--reps 7] [--steps 1000] [--dpmpp-steps 10,20] [--ddim-steps 20,50] [--n 64] [--guided-steps 20]"""
import argparse, ctypes as C, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from __graft_entry__ import load_pkg
from inputs import uniform
import test_unet_model as T

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64); ap.add_argument("--reps", type=int, default=7); ap.add_argument("--steps", type=int, default=1000)
ap.add_argument("--dpmpp-steps", default="10,20"); ap.add_argument("--ddim-steps", default="20,50"); ap.add_argument("--n", type=int, default=64)
ap.add_argument("--guided-steps", type=int, default=20)
a = ap.parse_args()
bla = load_pkg(); bla.init(0); L = bla.lib(); chk = bla.native.check
cfg = dict(image_h=32, image_w=32, in_channels=3, dims=[128, 256, 256, 256], time_dim=512, kernel=3, group_size=32, key_dim=16)
B, F, dim, K = a.batch, 3 * 32 * 32, 512, 10
LOGSNR = 1
st = L.bla_default_stream()
ev = [C.c_void_p() for _ in range(2)]
for e in ev: chk(L.bla_event_create(C.byref(e)))


def timed_ms(fn, inner=1):
    chk(L.bla_event_record(ev[0], st))
    for _ in range(inner): fn()
    chk(L.bla_event_record(ev[1], st)); bla.sync()
    r = C.c_float(); chk(L.bla_event_elapsed_ms(ev[0], ev[1], C.byref(r))); return r.value / inner


def pair(fns, inner=1, scale=1.0):
    """{name: [median, min, max]} of --reps repeats of each function, the functions taking turns within every repeat"""
    for fn in fns.values(): fn()                              # warm-up
    bla.sync()
    got = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, fn in fns.items(): got[k].append(timed_ms(fn, inner) * scale)
    return {k: [round(float(f(v)), 4) for f in (np.median, np.min, np.max)] for k, v in got.items()}


h, tensors = T.build(bla, cfg, B)
T.load_params(bla, h, tensors, cfg)
d = C.c_void_p(); chk(L.bla_diffusion_create(C.byref(d), a.steps, 1e-4, 0.02))
x, xt, hist, temb = bla.empty((B, F)), bla.empty((B, F)), bla.zeros((B, F)), bla.empty((B, dim))
out = L.bla_unet_output(h)
mid, gap = a.steps // 2, max(1, a.steps // 50)
chk(L.bla_time_embedding_f32(st, bla.to_device(np.full(B, mid, np.int32), np.int32).ptr, B, dim, temb.ptr))
chk(L.bla_rand_normal_f32(st, xt.ptr, B * F, 0.0, 1.0, 3, 0))
chk(L.bla_unet_forward_f32(h, st, xt.ptr, temb.ptr, None)); bla.sync()

# ---- (a), (b) the steps: with clip the values stay bounded however often the step repeats on its own output -----------------------------------------
ddim_step = lambda: chk(L.bla_diffusion_ddim_step_f32(d, st, xt.ptr, out, B, F, mid, mid - gap, 0.0, 1, 42, dim, temb.ptr))
dpmpp_step = lambda: chk(L.bla_diffusion_dpmpp_step_f32(d, st, xt.ptr, out, hist.ptr, B, F, mid + gap, mid, mid - gap, 1, dim, temb.ptr))
forward = lambda: chk(L.bla_unet_forward_f32(h, st, xt.ptr, temb.ptr, None))
step_us = pair({"ddim": ddim_step, "dpmpp": dpmpp_step}, inner=200, scale=1e3)
sampler_step_ms = pair({"ddim": lambda: (forward(), ddim_step()), "dpmpp": lambda: (forward(), dpmpp_step())}, inner=20)


# ---- (c) the loops ---------------------------------------------------------------------------------------------------------------------------------
def loop(fn):
    def run():
        chk(L.bla_rand_normal_f32(st, x.ptr, B * F, 0.0, 1.0, 8, 0))
        fn()
    return run


loops = {}
for S in [int(s) for s in a.dpmpp_steps.split(",") if s]:
    loops["dpmpp S=%d" % S] = loop(lambda S=S: chk(L.bla_unet_sample_dpmpp_f32(h, d, st, x.ptr, S, LOGSNR, 0)))
for S in [int(s) for s in a.ddim_steps.split(",") if s]:
    loops["ddim S=%d" % S] = loop(lambda S=S: chk(L.bla_unet_sample_ddim_f32(h, d, st, x.ptr, S, 0.0, 0, 8)))
loop_ms = pair(loops)
assert np.isfinite(x.numpy()).all()
chk(L.bla_diffusion_destroy(d)); chk(L.bla_unet_destroy(h))

# ---- (d) the guided pair at model batch 2n -----------------------------------------------------------------------------------------------------------
N, SG = a.n, a.guided_steps
hg, tg = T.build(bla, cfg, 2 * N)
T.load_params(bla, hg, tg, cfg)
d = C.c_void_p(); chk(L.bla_diffusion_create(C.byref(d), a.steps, 1e-4, 0.02))
table = bla.to_device(uniform(2, (K + 1, dim), -0.1, 0.1, np.float32))
lab = bla.to_device((np.arange(N) % K).astype(np.int32), np.int32)
xg = bla.empty((N, F))


def guided(fn):
    def run():
        chk(L.bla_rand_normal_f32(st, xg.ptr, N * F, 0.0, 1.0, 8, 0))
        fn()
    return run


guided_ms = pair({"ddim": guided(lambda: chk(L.bla_unet_sample_guided_ddim_f32(hg, d, st, xg.ptr, table.ptr, K, lab.ptr, 3.0, SG, 0.0, 0, 8))),
                  "dpmpp": guided(lambda: chk(L.bla_unet_sample_guided_dpmpp_f32(hg, d, st, xg.ptr, table.ptr, K, lab.ptr, 3.0, SG, LOGSNR, 0)))})
assert np.isfinite(xg.numpy()).all()
chk(L.bla_diffusion_destroy(d)); chk(L.bla_unet_destroy(hg))

res = {
    "batch": B, "steps": a.steps, "reps": a.reps, "format": "[median, min, max]",
    "step_us": step_us, "step_bytes": {"ddim": 12 * B * F, "dpmpp": 20 * B * F},
    "sampler_step_ms": sampler_step_ms, "sampler_step_dpmpp_over_ddim": round(sampler_step_ms["dpmpp"][0] / sampler_step_ms["ddim"][0], 4),
    "loop_ms": loop_ms, "loop_images_per_s": {k: round(B / (v[0] * 1e-3), 1) for k, v in loop_ms.items()},
    "loop_ms_per_step": {k: round(v[0] / int(k.split("=")[1]), 4) for k, v in loop_ms.items()},
    "n": N, "model_batch": 2 * N, "guided_sample_steps": SG, "guided_ms": guided_ms,
    "guided_images_per_s": {k: round(N / (v[0] * 1e-3), 1) for k, v in guided_ms.items()},
}
print(json.dumps(res), flush=True)
