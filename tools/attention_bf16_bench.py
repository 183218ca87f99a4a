#!/usr/bin/env python3
"""The bf16 self-attention block (bla_attention_{forward,backward}_batched_bf16) beside the fp32 entries, and the U-Net with its attention
blocks switched (bla_unet_set_attention): HIP events, one process, a pre-roll of 4096^3 fp32 products, medians [min .. max] of alternating rounds
(DESIGN 3.24's method).
usage: attention_bf16_bench.py [--batch 64] [--rounds 7] [--iters 5] [--warm 1.0] [--c 256 --s 256 --d 16]
Part 1, one block at C x S x d: forward and backward of both entries, in alternation.  Part 2, the U-Net at the reference's constants
(model/cifar_unet.c:26-37) with bf16 products: forward and forward + backward with BLA_UNET_ATTENTION_BF16 against BLA_UNET_ATTENTION_F32 (two models, one of
each).  Each claim is a difference of medians against the fp32 side's own min-max spread; the ratio is printed whatever it is.  Every timed output is
checked as finite; the bf16 block's output is printed normwise against the fp32 block's.
--trace N: no timing, N forward + backward passes of the bf16-products model in BLA_UNET_ATTENTION_BF16, for `rocprofv3 --kernel-trace --stats --`."""
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
ap.add_argument("--c", type=int, default=256); ap.add_argument("--s", type=int, default=256); ap.add_argument("--d", type=int, default=16)
ap.add_argument("--trace", type=int, default=0)
a = ap.parse_args()
bla = load_pkg(); bla.init(0); L = bla.lib(); chk = bla.native.check
st = L.bla_default_stream()
e0, e1 = C.c_void_p(), C.c_void_p(); chk(L.bla_event_create(C.byref(e0))); chk(L.bla_event_create(C.byref(e1)))
B, c, s, d = a.batch, a.c, a.s, a.d


class Cfg(C.Structure):
    _fields_ = [("image_h", C.c_int), ("image_w", C.c_int), ("in_channels", C.c_int), ("dims", C.c_int * 4), ("time_dim", C.c_int), ("kernel", C.c_int),
                ("group_size", C.c_int), ("key_dim", C.c_int)]


cfg = Cfg(CFG["image_h"], CFG["image_w"], CFG["in_channels"], (C.c_int * 4)(*CFG["dims"]), CFG["time_dim"], CFG["kernel"], CFG["group_size"], CFG["key_dim"])
flat = []
for i, (name, shp) in enumerate(tensor_list(CFG)):
    fan_in = int(np.prod(shp[1:])) if len(shp) > 1 else shp[0]
    flat.append(uniform(7000 + i, shp, *((-0.05, 0.05) if name.endswith("biases") else (-np.sqrt(3.0 / fan_in), np.sqrt(3.0 / fan_in))), np.float32).ravel())
flat = np.concatenate(flat)
n_img = B * 3 * 32 * 32


def model(attention):
    h = bla.unet_create_mixed(cfg, B, bla.UNET_PRODUCTS_BF16)
    chk(L.bla_memcpy_h2d(L.bla_unet_params(h), flat.ctypes.data, flat.nbytes, None)); bla.sync()
    bla.unet_set_attention(h, attention)
    return h


x = bla.to_device(uniform(7931, (n_img,), -1, 1, np.float32)); temb = bla.to_device(uniform(7932, (B, CFG["time_dim"]), 0, 1, np.float32))
noise = bla.to_device(uniform(7933, (n_img,), -1, 1, np.float32))
mfwd = lambda h: chk(L.bla_unet_forward_f32(h, st, x.ptr, temb.ptr, None))
mboth = lambda h: (mfwd(h), chk(L.bla_unet_backward_f32(h, st, noise.ptr)))


def fetch(ptr, n):
    out = np.empty(n, np.float32); chk(L.bla_memcpy_d2h(out.ctypes.data, ptr, out.nbytes, None)); bla.sync()
    return out


if a.trace:
    h = model(bla.UNET_ATTENTION_BF16)
    for _ in range(a.trace):
        mboth(h)
    bla.sync()
    assert np.isfinite(fetch(L.bla_unet_grads(h), flat.size)).all()
    print(f"{a.trace} forward + backward passes of the bf16-products model with bf16 attention at batch {B}, gradients finite")
    chk(L.bla_unet_destroy(h))
    sys.exit(0)

# ---- one block ------------------------------------------------------------------------------------------------------------------------------------------
gc, gd = np.sqrt(3.0 / c), np.sqrt(3.0 / d)
I = dict(x=uniform(1, (B, c, s), -1, 1, np.float32), wq=uniform(2, (c, d), -gc, gc, np.float32), wk=uniform(3, (c, d), -gc, gc, np.float32),
         wv=uniform(4, (c, d), -gc, gc, np.float32), w=uniform(5, (d, c), -gd, gd, np.float32), bias=uniform(6, (c,), -0.5, 0.5, np.float32),
         dy=uniform(7, (B, c, s), -1, 1, np.float32))
D = {n: bla.to_device(v) for n, v in I.items()}
sizes = dict(q=B * s * d, k=B * s * d, v=B * s * d, scores_raw=B * s * s, weights=B * s * s, attention=B * s * d)
fw = {n: bla.empty((sz,)) for n, sz in sizes.items()}; gw = {n: bla.empty((sz,)) for n, sz in sizes.items()}
fws, gws = bla.attention_ws(**fw), bla.attention_ws(**gw)
out = {k: bla.empty((B * c * s,)) for k in ("fp32", "bf16")}; dx = bla.empty((B * c * s,)); part = bla.empty((B * 4 * c * d,))
dwq, dwk, dwv, dw = (bla.empty((c * d,)) for _ in range(4))
args_f = lambda o: (st, B, D["x"].ptr, D["wq"].ptr, D["wk"].ptr, D["wv"].ptr, D["w"].ptr, D["bias"].ptr, C.byref(fws), o.ptr, c, s, d)
args_b = (st, B, D["dy"].ptr, D["x"].ptr, D["wq"].ptr, D["wk"].ptr, D["wv"].ptr, D["w"].ptr, C.byref(fws), C.byref(gws), part.ptr, dwq.ptr, dwk.ptr, dwv.ptr, dw.ptr,
          dx.ptr, c, s, d)
block = {"forward, fp32 entry": lambda: chk(L.bla_attention_forward_batched_f32(*args_f(out["fp32"]))),
         "forward, bf16 entry": lambda: chk(L.bla_attention_forward_batched_bf16(*args_f(out["bf16"]))),
         "backward, fp32 entry": lambda: chk(L.bla_attention_backward_batched_f32(*args_b, 0)),
         "backward, bf16 entry": lambda: chk(L.bla_attention_backward_batched_bf16(*args_b))}
M = {"attention fp32": model(bla.UNET_ATTENTION_F32), "attention bf16": model(bla.UNET_ATTENTION_BF16)}
for call in block.values():                                # eagerly once: the workspaces grow here, not inside a timed window
    call()
for h in M.values():
    mboth(h)
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


def timed(call, iters):
    call()
    chk(L.bla_event_record(e0, st))
    for _ in range(iters):
        call()
    chk(L.bla_event_record(e1, st))
    ms = C.c_float(); chk(L.bla_event_elapsed_ms(e0, e1, C.byref(ms)))
    return ms.value / iters


def rounds(calls, iters):
    res = {name: [] for name in calls}
    for r in range(a.rounds + 1):                          # round 0 is a rehearsal
        for name, call in calls.items():
            ms = timed(call, iters)
            if r > 0:
                res[name].append(ms)
    bla.sync()
    return {n: np.array(v) for n, v in res.items()}


def show(res, unit=1.0, name="ms"):
    for n, t in res.items():
        print(f"  {n:<44} median {np.median(t) * unit:9.3f} {name}  [{t.min() * unit:9.3f} .. {t.max() * unit:9.3f}]", flush=True)


def claim(res, new, old, unit=1.0, name="ms"):
    dd, spread = np.median(res[old]) - np.median(res[new]), res[old].max() - res[old].min()
    print(f"  claim: ({old}) - ({new}) = {dd * unit:.3f} {name} against ({old})'s own min-max spread of {spread * unit:.3f} {name}: "
          f"{'FASTER' if dd > spread else 'NOT faster'} by more than the spread ({np.median(res[old]) / np.median(res[new]):.2f} x)", flush=True)


print(f"== one attention block, C = {c}, S = {s}, d = {d}, batch {B}: medians of {a.rounds} alternating rounds of {20 * a.iters} calls", flush=True)
res = rounds(block, 20 * a.iters)
block["forward, fp32 entry"](); block["forward, bf16 entry"](); bla.sync()
o32, o16 = out["fp32"].numpy(), out["bf16"].numpy()
assert np.isfinite(o32).all() and np.isfinite(o16).all() and np.isfinite(dx.numpy()).all() and np.isfinite(dw.numpy()).all()
print(f" outputs finite; the bf16 entry's output {np.linalg.norm(o16.astype(np.float64) - o32) / np.linalg.norm(o32.astype(np.float64)):.2e} normwise from the fp32 entry's", flush=True)
show(res, 1000.0, "us")
claim(res, "forward, bf16 entry", "forward, fp32 entry", 1000.0, "us")
claim(res, "backward, bf16 entry", "backward, fp32 entry", 1000.0, "us")

# ---- the model ------------------------------------------------------------------------------------------------------------------------------------------
print(f"== U-Net at the reference's constants, bf16 products, batch {B}: medians of {a.rounds} alternating rounds of {a.iters} passes", flush=True)
calls = {}
for kind, fn in (("forward", mfwd), ("forward + backward", mboth)):
    for name, h in M.items():
        calls[f"{kind}, {name}"] = (lambda f=fn, hh=h: f(hh))
res = rounds(calls, a.iters)
outs = {name: fetch(L.bla_unet_output(h), n_img) for name, h in M.items()}
grads = {name: fetch(L.bla_unet_grads(h), flat.size) for name, h in M.items()}
assert all(np.isfinite(v).all() for v in outs.values()) and all(np.isfinite(v).all() and np.abs(v).max() > 0 for v in grads.values())
dd = np.linalg.norm(outs["attention bf16"].astype(np.float64) - outs["attention fp32"]) / np.linalg.norm(outs["attention fp32"].astype(np.float64))
print(f" every prediction and gradient bucket finite; prediction with bf16 attention {dd:.2e} normwise from the one with fp32 attention", flush=True)
show(res)
for kind in ("forward", "forward + backward"):
    claim(res, f"{kind}, attention bf16", f"{kind}, attention fp32")
for h in M.values():
    chk(L.bla_unet_destroy(h))
