#!/usr/bin/env python3
"""The online-softmax fp32 attention block (bla_attention_{forward,backward}_batched_online_f32) beside the entries that exist at the same shape:
HIP events, one process, a pre-roll of 4096^3 fp32 products, medians [min .. max] of alternating rounds (tools/attention_online_bench.py's method).
usage: attention_online_f32_bench.py [--batches 64,16] [--model-batch 16] [--rounds 7] [--iters 5] [--warm 1.0] [--parts 123]
Part 1, one block at C = 256, S = 1024, d = 16, one head, at each batch: the materialising fp32 entries (bla_attention_*_batched_f32, the only other fp32 path
at that S), the online bf16 entries and the online fp32 entries, forward and forward + backward.
Part 2, the same C and S with 4 heads of 16: the online bf16 heads entries and the online fp32 entries (no materialising fp32 multi-head path exists at that S).
Part 3, no timing: bla_unet_device_bytes of the reference-width fp32 model on 64 x 64 images, created by bla_unet_create_mixed and by
bla_unet_create_attention(.., BLA_UNET_ATTENTION_F32_ONLINE).
The claim under test: forward + backward of the online fp32 entries is no slower than the materialising fp32 entries, i.e. its median lies below theirs by more
than their own min-max spread; it is printed as HOLDS or FAILS with the ratio, whatever it is.  Every timed output is checked as finite; the online outputs are
printed normwise against the fp32 block's."""
import argparse, ctypes as C, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from __graft_entry__ import load_pkg
from inputs import uniform
from unet_refconst import CFG

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="64,16")
ap.add_argument("--model-batch", type=int, default=16)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--warm", type=float, default=1.0, help="seconds of 4096^3 fp32 products before the first measurement (0 = cold)")
ap.add_argument("--parts", default="123")
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


def show(res, unit=1000.0, name="us"):
    for n, t in res.items():
        print(f"  {n:<44} median {np.median(t) * unit:10.3f} {name}  [{t.min() * unit:10.3f} .. {t.max() * unit:10.3f}]", flush=True)


def claim(res, new, old, unit=1000.0, name="us"):
    dd, spread = np.median(res[old]) - np.median(res[new]), res[old].max() - res[old].min()
    print(f"  claim ({new}) is no slower than ({old}), its median below theirs by more than their spread: difference of medians {dd * unit:.3f} {name} against "
          f"the baseline's min-max spread of {spread * unit:.3f} {name}: {'HOLDS' if dd > spread else 'FAILS'} ({np.median(res[old]) / np.median(res[new]):.2f} x)", flush=True)


def warm_up():
    if a.warm > 0:
        wa = bla.to_device(uniform(1, (4096, 4096), dtype=np.float32)); wc = bla.empty((4096, 4096))
        t0 = time.time()
        while time.time() - t0 < a.warm:
            for _ in range(20):
                bla.gemm(wa, wa, wc, stream=st)
            bla.sync()
        print(f"# warmed up for {a.warm:.1f} s of 4096^3 fp32 products", flush=True)


def one_block(B, c, s, heads, d):
    D_ = heads * d
    gc, gd = np.sqrt(3.0 / c), np.sqrt(3.0 / D_)
    I = dict(x=uniform(1, (B, c, s), -1, 1, np.float32), wq=uniform(2, (c, D_), -1.5 * gc, 1.5 * gc, np.float32), wk=uniform(3, (c, D_), -1.5 * gc, 1.5 * gc, np.float32),
             wv=uniform(4, (c, D_), -gc, gc, np.float32), w=uniform(5, (D_, c), -gd, gd, np.float32), bias=uniform(6, (c,), -0.5, 0.5, np.float32),
             dy=uniform(7, (B, c, s), -1, 1, np.float32))
    D = {n: bla.to_device(v) for n, v in I.items()}
    square = B * s * s if heads == 1 else 1                # only the materialising fp32 entries touch S x S
    sizes = dict(q=B * s * D_, k=B * s * D_, v=B * s * D_, scores_raw=max(square, B * heads * s), weights=square, attention=B * s * D_)
    fw = {n: bla.empty((sz,)) for n, sz in sizes.items()}; gw = {n: bla.empty((sz,)) for n, sz in sizes.items()}
    fws, gws = bla.attention_ws(**fw), bla.attention_ws(**gw)
    kinds = (["fp32"] if heads == 1 else []) + ["online bf16", "online fp32"]
    out = {k: bla.empty((B * c * s,)) for k in kinds}; dx = bla.empty((B * c * s,)); part = bla.empty((B * 4 * c * D_,))
    dwq, dwk, dwv, dw = (bla.empty((c * D_,)) for _ in range(4))
    head = lambda o: (st, B, D["x"].ptr, D["wq"].ptr, D["wk"].ptr, D["wv"].ptr, D["w"].ptr, D["bias"].ptr, C.byref(fws), o.ptr, c, s)
    back = (st, B, D["dy"].ptr, D["x"].ptr, D["wq"].ptr, D["wk"].ptr, D["wv"].ptr, D["w"].ptr, C.byref(fws), C.byref(gws), part.ptr, dwq.ptr, dwk.ptr, dwv.ptr, dw.ptr,
            dx.ptr, c, s)
    fwd = {"fp32": lambda: chk(L.bla_attention_forward_batched_f32(*head(out["fp32"]), d)),
           "online bf16": lambda: chk(L.bla_attention_forward_batched_online_bf16_heads(*head(out["online bf16"]), heads, d)),
           "online fp32": lambda: chk(L.bla_attention_forward_batched_online_f32(*head(out["online fp32"]), heads, d))}
    bwd = {"fp32": lambda: chk(L.bla_attention_backward_batched_f32(*back, d, 0)),
           "online bf16": lambda: chk(L.bla_attention_backward_batched_online_bf16_heads(*back, heads, d)),
           "online fp32": lambda: chk(L.bla_attention_backward_batched_online_f32(*back, heads, d))}
    # a backward call reads what ITS forward call saved: time forward + backward pairs and the forward calls alone; the backward pass is their difference
    calls = {}
    for k in kinds:
        calls[f"forward, {k} entry"] = fwd[k]
        calls[f"forward + backward, {k} entry"] = (lambda f=fwd[k], b=bwd[k]: (f(), b()))
    for call in calls.values():                            # eagerly once: the workspaces grow here, not inside a timed window
        call()
    bla.sync()
    warm_up()
    print(f"== one attention block, C = {c}, S = {s}, {heads} head(s) of {d}, batch {B}: medians of {a.rounds} alternating rounds of {a.iters} calls", flush=True)
    res = rounds(calls, a.iters)
    for k in kinds:
        fwd[k]()
    bla.sync()
    o = {k: out[k].numpy() for k in kinds}
    assert all(np.isfinite(v).all() for v in o.values()) and np.isfinite(dx.numpy()).all() and np.isfinite(dw.numpy()).all()
    base = kinds[0]
    for k in kinds[1:]:
        print(f" outputs finite; the {k} entry's output {np.linalg.norm(o[k].astype(np.float64) - o[base]) / np.linalg.norm(o[base].astype(np.float64)):.2e} "
              f"normwise from the {base} entry's", flush=True)
    show(res)
    for k in kinds:
        print(f"  backward alone, {k} entry (difference of the medians above): {(np.median(res[f'forward + backward, {k} entry']) - np.median(res[f'forward, {k} entry'])) * 1000:10.3f} us")
    flop = 4.0 * s * s * d * heads * B
    print(f"  (S x S arithmetic of a forward pass, 4 S^2 d heads B = {flop / 1e9:.2f} GFLOP: the online fp32 forward runs it at "
          f"{flop / np.median(res['forward, online fp32 entry']) / 1e9:.1f} TFLOP/s, qkv and the output product included in the time)")
    if heads == 1:
        for kind in ("forward", "forward + backward"):
            claim(res, f"{kind}, online fp32 entry", f"{kind}, fp32 entry")
    for kind in ("forward", "forward + backward"):
        r = np.median(res[f"{kind}, online fp32 entry"]) / np.median(res[f"{kind}, online bf16 entry"])
        print(f"  {kind}: the online fp32 entries take {r:.2f} x the online bf16 entries' time (no claim)")


def model_bytes():
    B = a.model_batch
    cfg64 = dict(CFG, image_h=64, image_w=64)
    cfg = Cfg(cfg64["image_h"], cfg64["image_w"], cfg64["in_channels"], (C.c_int * 4)(*cfg64["dims"]), cfg64["time_dim"], cfg64["kernel"], cfg64["group_size"],
              cfg64["key_dim"])
    print(f"== bla_unet_device_bytes, the reference's widths on 64 x 64 images (attention at S = 1024 and S = 64), fp32 products, one head, batch {B}", flush=True)
    got = {}
    for name, make in (("bla_unet_create_mixed", lambda: bla.unet_create_mixed(cfg, B, bla.UNET_PRODUCTS_F32)),
                       ("bla_unet_create_attention, BLA_UNET_ATTENTION_F32_ONLINE", lambda: bla.unet_create_attention(cfg, B, bla.UNET_PRODUCTS_F32, 1, bla.UNET_ATTENTION_F32_ONLINE))):
        h = make()
        got[name] = bla.unet_device_bytes(h)
        chk(L.bla_unet_destroy(h))
        print(f"  {name:<60} {got[name]:>14} bytes  ({got[name] / 2 ** 30:.3f} GiB)", flush=True)
    v = list(got.values())
    print(f"  created in its mode the model owns {v[0] - v[1]} bytes ({(v[0] - v[1]) / 2 ** 30:.3f} GiB) less")


if "1" in a.parts:
    for B_ in (int(t) for t in a.batches.split(",")):
        one_block(B_, 256, 1024, 1, 16)
if "2" in a.parts:
    for B_ in (int(t) for t in a.batches.split(",")):
        one_block(B_, 256, 1024, 4, 16)
if "3" in a.parts:
    model_bytes()
