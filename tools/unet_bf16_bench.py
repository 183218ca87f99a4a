#!/usr/bin/env python3
"""The U-Net with bf16 products (bla_unet_create_mixed) beside the fp32 model: model-level timing (HIP events), one process, a pre-roll of
4096^3 fp32 products, medians [min .. max] of alternating rounds (DESIGN 3.24's method).
usage: unet_bf16_bench.py [--batch 64] [--rounds 7] [--iters 5] [--warm 1.0]        the reference's constants (model/cifar_unet.c:26-37)
Timed, in alternation: the fp32 model's forward pass and forward + backward pass; the bf16 model's, created with the table launches (default) and created
under BLA_UNET_BF16_PREP=0 (every kernel matrix prepared in front of its product); one DDIM sampler step (S = 1 of a 1000-step schedule) on the fp32 and on
the bf16 model.  Two claims are evaluated as DESIGN 3.24 does -- a difference of medians against the slower side's own min-max spread: the bf16 passes
against the fp32 passes, and the table launches against per-convolution preparation.  Every timed output (prediction, gradient bucket, sample) is checked
as finite in the run, the two bf16 models' buckets as bit-equal; the bf16 prediction's normwise distance from the fp32 model's is printed.  Parameters
are uniform random at sqrt(3 / fan_in), no dropout."""
import argparse, ctypes as C, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from __graft_entry__ import load_pkg
from inputs import uniform
from unet_refconst import CFG, tensor_list

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--warm", type=float, default=1.0, help="seconds of 4096^3 fp32 products before the first measurement (0 = cold)")
ap.add_argument("--trace", type=int, default=0, help="no timing: this many forward + backward passes of the bf16 model alone, for a kernel trace")
a = ap.parse_args()
bla = load_pkg(); bla.init(0); L = bla.lib(); chk = bla.native.check
st = L.bla_default_stream()
e0, e1 = C.c_void_p(), C.c_void_p(); chk(L.bla_event_create(C.byref(e0))); chk(L.bla_event_create(C.byref(e1)))
B = a.batch


class Cfg(C.Structure):
    _fields_ = [("image_h", C.c_int), ("image_w", C.c_int), ("in_channels", C.c_int), ("dims", C.c_int * 4), ("time_dim", C.c_int), ("kernel", C.c_int),
                ("group_size", C.c_int), ("key_dim", C.c_int)]


cfg = Cfg(CFG["image_h"], CFG["image_w"], CFG["in_channels"], (C.c_int * 4)(*CFG["dims"]), CFG["time_dim"], CFG["kernel"], CFG["group_size"], CFG["key_dim"])
flat = []
for i, (name, shp) in enumerate(tensor_list(CFG)):
    fan_in = int(np.prod(shp[1:])) if len(shp) > 1 else shp[0]
    flat.append(uniform(7000 + i, shp, *((-0.05, 0.05) if name.endswith("biases") else (-np.sqrt(3.0 / fan_in), np.sqrt(3.0 / fan_in))), np.float32).ravel())
flat = np.concatenate(flat)


def model(products, prep=None):
    keep = os.environ.pop("BLA_UNET_BF16_PREP", None)
    if prep is not None:
        os.environ["BLA_UNET_BF16_PREP"] = prep          # read at the create call
    try:
        h = bla.unet_create_mixed(cfg, B, products)
    finally:
        os.environ.pop("BLA_UNET_BF16_PREP", None)
        if keep is not None:
            os.environ["BLA_UNET_BF16_PREP"] = keep
    assert L.bla_unet_param_count(h) == flat.size         # (every tensor of the reference's constants is a multiple of 4 floats)
    chk(L.bla_memcpy_h2d(L.bla_unet_params(h), flat.ctypes.data, flat.nbytes, None)); bla.sync()
    return h


if a.trace:      # under `rocprofv3 --kernel-trace --stats -- python tools/unet_bf16_bench.py --trace 10`: where a bf16 pass spends its time, kernel by kernel
    h = bla.unet_create_mixed(cfg, B, bla.UNET_PRODUCTS_BF16)      # (BLA_UNET_BF16_PREP as the environment has it)
    chk(L.bla_memcpy_h2d(L.bla_unet_params(h), flat.ctypes.data, flat.nbytes, None)); bla.sync()
    x = bla.to_device(uniform(7931, (B * 3 * 32 * 32,), -1, 1, np.float32)); temb = bla.to_device(uniform(7932, (B, CFG["time_dim"]), 0, 1, np.float32))
    noise = bla.to_device(uniform(7933, (B * 3 * 32 * 32,), -1, 1, np.float32))
    for _ in range(a.trace):
        chk(L.bla_unet_forward_f32(h, st, x.ptr, temb.ptr, None)); chk(L.bla_unet_backward_f32(h, st, noise.ptr))
    bla.sync()
    g = np.empty(flat.size, np.float32); chk(L.bla_memcpy_d2h(g.ctypes.data, L.bla_unet_grads(h), g.nbytes, None)); bla.sync()
    assert np.isfinite(g).all()
    print(f"{a.trace} forward + backward passes of the bf16 model at batch {B}, gradients finite")
    chk(L.bla_unet_destroy(h))
    sys.exit(0)

M = {"fp32": model(bla.UNET_PRODUCTS_F32), "bf16": model(bla.UNET_PRODUCTS_BF16), "bf16, BLA_UNET_BF16_PREP=0": model(bla.UNET_PRODUCTS_BF16, "0")}
n_img = B * 3 * 32 * 32
x = bla.to_device(uniform(7931, (n_img,), -1, 1, np.float32)); temb = bla.to_device(uniform(7932, (B, CFG["time_dim"]), 0, 1, np.float32))
noise = bla.to_device(uniform(7933, (n_img,), -1, 1, np.float32)); xs = bla.empty((n_img,))
diff = C.c_void_p(); chk(L.bla_diffusion_create(C.byref(diff), 1000, 1e-4, 0.02))
fwd = lambda h: chk(L.bla_unet_forward_f32(h, st, x.ptr, temb.ptr, None))
both = lambda h: (fwd(h), chk(L.bla_unet_backward_f32(h, st, noise.ptr)))
ddim = lambda h: chk(L.bla_unet_sample_ddim_f32(h, diff, st, xs.ptr, 1, 0.0, 1, 5))


def fetch(ptr, n):
    out = np.empty(n, np.float32); chk(L.bla_memcpy_d2h(out.ctypes.data, ptr, out.nbytes, None)); bla.sync()
    return out


for h in M.values():                                       # eagerly once: the workspaces grow here, not inside a timed window
    both(h); chk(L.bla_memcpy_d2d(xs.ptr, x.ptr, n_img * 4, None)); ddim(h)
bla.sync()
if a.warm > 0:
    wa = bla.to_device(uniform(1, (4096, 4096), dtype=np.float32)); wc = bla.empty((4096, 4096))
    t0 = time.time()
    while time.time() - t0 < a.warm:
        for _ in range(20):
            bla.gemm(wa, wa, wc, stream=st)
        bla.sync()
    del wa, wc
    print(f"# warmed up for {a.warm:.1f} s of 4096^3 fp32 products", flush=True)


def timed(call):
    call()
    chk(L.bla_event_record(e0, st))
    for _ in range(a.iters):
        call()
    chk(L.bla_event_record(e1, st))
    ms = C.c_float(); chk(L.bla_event_elapsed_ms(e0, e1, C.byref(ms)))
    return ms.value / a.iters


def rounds(calls):
    res = {name: [] for name in calls}
    for r in range(a.rounds + 1):                          # round 0 is a rehearsal
        for name, call in calls.items():
            ms = timed(call)
            if r > 0:
                res[name].append(ms)
    bla.sync()
    return {n: np.array(v) for n, v in res.items()}


def show(res):
    for n, t in res.items():
        print(f"  {n:<52} median {np.median(t):8.3f} ms  [{t.min():8.3f} .. {t.max():8.3f}]", flush=True)


def claim(res, new, old, what):
    d, spread = np.median(res[old]) - np.median(res[new]), res[old].max() - res[old].min()
    print(f"  {what}: ({old}) - ({new}) = {d:.3f} ms against ({old})'s own min-max spread of {spread:.3f} ms: "
          f"{'FASTER' if d > spread else 'NOT faster'} by more than the spread ({np.median(res[old]) / np.median(res[new]):.2f} x)", flush=True)


print(f"== U-Net at the reference's constants, batch {B}: medians of {a.rounds} alternating rounds of {a.iters} passes", flush=True)
calls = {}
for kind, fn in (("forward", fwd), ("forward + backward", both)):
    for name, h in M.items():
        calls[f"{kind}, {name}"] = (lambda f=fn, hh=h: f(hh))
res = rounds(calls)
outs = {name: fetch(L.bla_unet_output(h), n_img) for name, h in M.items()}
grads = {name: fetch(L.bla_unet_grads(h), flat.size) for name, h in M.items()}
assert all(np.isfinite(v).all() for v in outs.values()) and all(np.isfinite(v).all() and np.abs(v).max() > 0 for v in grads.values())
assert np.array_equal(grads["bf16"], grads["bf16, BLA_UNET_BF16_PREP=0"]) and np.array_equal(outs["bf16"], outs["bf16, BLA_UNET_BF16_PREP=0"])
d = np.linalg.norm(outs["bf16"].astype(np.float64) - outs["fp32"]) / np.linalg.norm(outs["fp32"].astype(np.float64))
print(f" every prediction and gradient bucket finite; the two bf16 models bit-equal; bf16 prediction {d:.2e} normwise from the fp32 model's", flush=True)
show(res)
for kind in ("forward", "forward + backward"):
    claim(res, f"{kind}, bf16", f"{kind}, fp32", "claim 1")
for kind in ("forward", "forward + backward"):
    claim(res, f"{kind}, bf16", f"{kind}, bf16, BLA_UNET_BF16_PREP=0", "claim 2")
dcalls = {}
for name in ("fp32", "bf16"):
    dcalls[f"one DDIM step, {name}"] = (lambda hh=M[name]: (chk(L.bla_memcpy_d2d(xs.ptr, x.ptr, n_img * 4, st)), ddim(hh)))
dres = rounds(dcalls)
assert np.isfinite(xs.numpy()).all()
print(" one DDIM sampler step (the forward pass, the embedding and the step kernel; the sample finite):", flush=True)
show(dres)
claim(dres, "one DDIM step, bf16", "one DDIM step, fp32", "sampler")
for h in M.values():
    chk(L.bla_unet_destroy(h))
chk(L.bla_diffusion_destroy(diff))
