#!/usr/bin/env python3
"""The online-softmax bf16 attention block (bla_attention_{forward,backward}_batched_online_bf16) beside the entries that exist at the same
shape, and the U-Net on 64 x 64 images with its attention blocks switched to it: HIP events, one process, a pre-roll of 4096^3 fp32 products, medians
[min .. max] of alternating rounds (tools/attention_bf16_bench.py's method).
usage: attention_online_bench.py [--batch 64] [--model-batch 16] [--rounds 7] [--iters 10] [--warm 1.0] [--parts 123]
Part 1, one block at C = 256, S = 1024, d = 16: the fp32 entries (the only other path at that S) and the online entries, forward and backward.
Part 2, one block at C = S = 256, d = 16: the fp32 entries, the materialising bf16 entries and the online entries.
Part 3, the U-Net at the reference's widths (model/cifar_unet.c:26-37) on 64 x 64 images with bf16 products: forward + backward with
BLA_UNET_ATTENTION_BF16_ONLINE against BLA_UNET_ATTENTION_F32 (two models, one of each).
Each claim is a difference of medians against the baseline's own min-max spread; the ratio is printed whatever it is.  Every timed output is checked as
finite; the online block's output is printed normwise against the fp32 block's.
--trace N: no timing, N forward + backward calls of the online entries at part 1's shape, then N forward + backward passes of the part 3 model in
BLA_UNET_ATTENTION_BF16_ONLINE, for `rocprofv3 --kernel-trace --stats --`."""
import argparse, ctypes as C, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from __graft_entry__ import load_pkg
from inputs import uniform
from unet_refconst import CFG, tensor_list

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--model-batch", type=int, default=16)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warm", type=float, default=1.0, help="seconds of 4096^3 fp32 products before the first measurement (0 = cold)")
ap.add_argument("--parts", default="123")
ap.add_argument("--trace", type=int, default=0)
a = ap.parse_args()
bla = load_pkg(); bla.init(0); L = bla.lib(); chk = bla.native.check
st = L.bla_default_stream()
e0, e1 = C.c_void_p(), C.c_void_p(); chk(L.bla_event_create(C.byref(e0))); chk(L.bla_event_create(C.byref(e1)))


class Cfg(C.Structure):
    _fields_ = [("image_h", C.c_int), ("image_w", C.c_int), ("in_channels", C.c_int), ("dims", C.c_int * 4), ("time_dim", C.c_int), ("kernel", C.c_int),
                ("group_size", C.c_int), ("key_dim", C.c_int)]


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
        print(f"  {n:<44} median {np.median(t) * unit:10.3f} {name}  [{t.min() * unit:10.3f} .. {t.max() * unit:10.3f}]", flush=True)


def claim(res, new, old, what, unit=1.0, name="ms"):
    dd, spread = np.median(res[old]) - np.median(res[new]), res[old].max() - res[old].min()
    verdict = "HOLDS" if dd > (spread if what == "faster" else -spread) else "FAILS"
    print(f"  claim ({new}) is {what} than ({old}): difference of medians {dd * unit:.3f} {name} against the baseline's min-max spread of {spread * unit:.3f} {name}: "
          f"{verdict} ({np.median(res[old]) / np.median(res[new]):.2f} x)", flush=True)


def warm_up():
    if a.warm > 0:
        wa = bla.to_device(uniform(1, (4096, 4096), dtype=np.float32)); wc = bla.empty((4096, 4096))
        t0 = time.time()
        while time.time() - t0 < a.warm:
            for _ in range(20):
                bla.gemm(wa, wa, wc, stream=st)
            bla.sync()
        print(f"# warmed up for {a.warm:.1f} s of 4096^3 fp32 products", flush=True)


def one_block(c, s, d, with_bf16):
    B = a.batch
    gc, gd = np.sqrt(3.0 / c), np.sqrt(3.0 / d)
    I = dict(x=uniform(1, (B, c, s), -1, 1, np.float32), wq=uniform(2, (c, d), -1.5 * gc, 1.5 * gc, np.float32), wk=uniform(3, (c, d), -1.5 * gc, 1.5 * gc, np.float32),
             wv=uniform(4, (c, d), -gc, gc, np.float32), w=uniform(5, (d, c), -gd, gd, np.float32), bias=uniform(6, (c,), -0.5, 0.5, np.float32),
             dy=uniform(7, (B, c, s), -1, 1, np.float32))
    D = {n: bla.to_device(v) for n, v in I.items()}
    sizes = dict(q=B * s * d, k=B * s * d, v=B * s * d, scores_raw=B * s * s, weights=B * s * s, attention=B * s * d)
    fw = {n: bla.empty((sz,)) for n, sz in sizes.items()}; gw = {n: bla.empty((sz,)) for n, sz in sizes.items()}
    fws, gws = bla.attention_ws(**fw), bla.attention_ws(**gw)
    kinds = ["fp32"] + (["bf16"] if with_bf16 else []) + ["online"]
    out = {k: bla.empty((B * c * s,)) for k in kinds}; dx = bla.empty((B * c * s,)); part = bla.empty((B * 4 * c * d,))
    dwq, dwk, dwv, dw = (bla.empty((c * d,)) for _ in range(4))
    args_f = lambda o: (st, B, D["x"].ptr, D["wq"].ptr, D["wk"].ptr, D["wv"].ptr, D["w"].ptr, D["bias"].ptr, C.byref(fws), o.ptr, c, s, d)
    args_b = (st, B, D["dy"].ptr, D["x"].ptr, D["wq"].ptr, D["wk"].ptr, D["wv"].ptr, D["w"].ptr, C.byref(fws), C.byref(gws), part.ptr, dwq.ptr, dwk.ptr, dwv.ptr, dw.ptr,
              dx.ptr, c, s, d)
    fwd = {"fp32": lambda: chk(L.bla_attention_forward_batched_f32(*args_f(out["fp32"]))),
           "bf16": lambda: chk(L.bla_attention_forward_batched_bf16(*args_f(out["bf16"]))),
           "online": lambda: chk(L.bla_attention_forward_batched_online_bf16(*args_f(out["online"])))}
    bwd = {"fp32": lambda: chk(L.bla_attention_backward_batched_f32(*args_b, 0)),
           "bf16": lambda: chk(L.bla_attention_backward_batched_bf16(*args_b)),
           "online": lambda: chk(L.bla_attention_backward_batched_online_bf16(*args_b))}
    # a backward call reads what ITS forward call saved (the three entries keep different things in the shared workspace): time forward + backward
    # pairs and the forward calls alone; the backward pass is their difference
    calls = {}
    for k in kinds:
        calls[f"forward, {k} entry"] = fwd[k]
        calls[f"forward + backward, {k} entry"] = (lambda f=fwd[k], b=bwd[k]: (f(), b()))
    if a.trace:
        for _ in range(a.trace):
            calls["forward + backward, online entry"]()
        bla.sync()
        assert np.isfinite(dx.numpy()).all()
        print(f"{a.trace} forward + backward calls of the online entries at C = {c}, S = {s}, d = {d}, batch {B}, del_x finite")
        return
    for call in calls.values():                            # eagerly once: the workspaces grow here, not inside a timed window
        call()
    bla.sync()
    warm_up()
    print(f"== one attention block, C = {c}, S = {s}, d = {d}, batch {B}: medians of {a.rounds} alternating rounds of {a.iters} calls", flush=True)
    res = rounds(calls, a.iters)
    for k in kinds:
        fwd[k]()
    bla.sync()
    o = {k: out[k].numpy() for k in kinds}
    assert all(np.isfinite(v).all() for v in o.values()) and np.isfinite(dx.numpy()).all() and np.isfinite(dw.numpy()).all()
    for k in kinds[1:]:
        print(f" outputs finite; the {k} entry's output {np.linalg.norm(o[k].astype(np.float64) - o['fp32']) / np.linalg.norm(o['fp32'].astype(np.float64)):.2e} "
              "normwise from the fp32 entry's", flush=True)
    show(res, 1000.0, "us")
    for k in kinds:
        print(f"  backward alone, {k} entry (difference of the medians above): {(np.median(res[f'forward + backward, {k} entry']) - np.median(res[f'forward, {k} entry'])) * 1000:10.3f} us")
    flop = 4.0 * s * s * d * B
    print(f"  (S x S arithmetic of a forward pass, 4 S^2 d B = {flop / 1e9:.2f} GFLOP: the online forward runs it at "
          f"{flop / np.median(res['forward, online entry']) / 1e9:.1f} TFLOP/s, qkv and the output product included in the time)")
    for kind in ("forward", "forward + backward"):
        if with_bf16:
            claim(res, f"{kind}, online entry", f"{kind}, bf16 entry", "no slower", 1000.0, "us")
            claim(res, f"{kind}, online entry", f"{kind}, fp32 entry", "faster", 1000.0, "us")
        else:
            claim(res, f"{kind}, online entry", f"{kind}, fp32 entry", "faster", 1000.0, "us")


def model_part():
    B = a.model_batch
    cfg64 = dict(CFG, image_h=64, image_w=64)
    cfg = Cfg(cfg64["image_h"], cfg64["image_w"], cfg64["in_channels"], (C.c_int * 4)(*cfg64["dims"]), cfg64["time_dim"], cfg64["kernel"], cfg64["group_size"],
              cfg64["key_dim"])
    flat = []
    for i, (name, shp) in enumerate(tensor_list(cfg64)):
        fan_in = int(np.prod(shp[1:])) if len(shp) > 1 else shp[0]
        flat.append(uniform(7000 + i, shp, *((-0.05, 0.05) if name.endswith("biases") else (-np.sqrt(3.0 / fan_in), np.sqrt(3.0 / fan_in))), np.float32).ravel())
    flat = np.concatenate(flat)
    n_img = B * 3 * 64 * 64

    def model(attention):
        h = bla.unet_create_mixed(cfg, B, bla.UNET_PRODUCTS_BF16)
        assert L.bla_unet_param_count(h) >= flat.size
        chk(L.bla_memcpy_h2d(L.bla_unet_params(h), flat.ctypes.data, flat.nbytes, None)); bla.sync()
        bla.unet_set_attention(h, attention)
        return h

    def fetch(ptr, n):
        out = np.empty(n, np.float32); chk(L.bla_memcpy_d2h(out.ctypes.data, ptr, out.nbytes, None)); bla.sync()
        return out
    x = bla.to_device(uniform(7931, (n_img,), -1, 1, np.float32)); temb = bla.to_device(uniform(7932, (B, cfg64["time_dim"]), 0, 1, np.float32))
    noise = bla.to_device(uniform(7933, (n_img,), -1, 1, np.float32))
    mfwd = lambda h: chk(L.bla_unet_forward_f32(h, st, x.ptr, temb.ptr, None))
    mboth = lambda h: (mfwd(h), chk(L.bla_unet_backward_f32(h, st, noise.ptr)))
    if a.trace:
        h = model(bla.UNET_ATTENTION_BF16_ONLINE)
        for _ in range(a.trace):
            mboth(h)
        bla.sync()
        assert np.isfinite(fetch(L.bla_unet_grads(h), flat.size)).all()
        print(f"{a.trace} forward + backward passes of the bf16-products model on 64 x 64 images with online attention at batch {B}, gradients finite")
        chk(L.bla_unet_destroy(h))
        return
    M = {"attention fp32": model(bla.UNET_ATTENTION_F32), "attention online": model(bla.UNET_ATTENTION_BF16_ONLINE)}
    for h in M.values():
        mboth(h)
    bla.sync()
    warm_up()
    iters = max(1, a.iters // 3)
    print(f"== U-Net at the reference's widths on 64 x 64 images (attention at S = 1024, C = {cfg64['dims'][1]}, d = {cfg64['key_dim']}), bf16 products, batch {B}: "
          f"medians of {a.rounds} alternating rounds of {iters} passes", flush=True)
    calls = {}
    for kind, fn in (("forward", mfwd), ("forward + backward", mboth)):
        for name, h in M.items():
            calls[f"{kind}, {name}"] = (lambda f=fn, hh=h: f(hh))
    res = rounds(calls, iters)
    outs = {name: fetch(L.bla_unet_output(h), n_img) for name, h in M.items()}
    grads = {name: fetch(L.bla_unet_grads(h), flat.size) for name, h in M.items()}
    assert all(np.isfinite(v).all() for v in outs.values()) and all(np.isfinite(v).all() and np.abs(v).max() > 0 for v in grads.values())
    dd = np.linalg.norm(outs["attention online"].astype(np.float64) - outs["attention fp32"]) / np.linalg.norm(outs["attention fp32"].astype(np.float64))
    print(f" every prediction and gradient bucket finite; prediction with online attention {dd:.2e} normwise from the one with fp32 attention", flush=True)
    show(res)
    for kind in ("forward", "forward + backward"):
        claim(res, f"{kind}, attention online", f"{kind}, attention fp32", "faster")
    for h in M.values():
        chk(L.bla_unet_destroy(h))


if a.trace:
    one_block(256, 1024, 16, with_bf16=False)
    model_part()
    sys.exit(0)
if "1" in a.parts:
    one_block(256, 1024, 16, with_bf16=False)
if "2" in a.parts:
    one_block(256, 256, 16, with_bf16=True)
if "3" in a.parts:
    model_part()
