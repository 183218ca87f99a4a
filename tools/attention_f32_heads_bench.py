#!/usr/bin/env python3
"""The fp32 multi-head attention block for short sequences (bla_attention_{forward,backward}_batched_f32_heads) beside what a caller had before
it, and the multi-head U-Net beside the single-head one: HIP events, one process, a pre-roll of 4096^3 fp32 products, medians [min .. max] of alternating
rounds (tools/attention_heads_bench.py's method).
usage: attention_f32_heads_bench.py [--batches 64,16] [--rounds 7] [--iters 20] [--warm 1.0] [--no-model]
Block, at C = 256, S = 16 (the 4 x 4 mid block of the reference's constants), heads 4 x d 16 and each batch, forward calls and forward + backward pairs of
  heads:    the new entries;
  serial:   four consecutive bla_attention_{forward,backward}_batched_f32 calls on contiguous copies of the heads' slices of the weights, which is what a
            caller could do before, WITHOUT the two sums across heads (out and del_x of the last head stay in the buffers): a lower bound of that workaround.
The claim: heads is faster than serial by more than serial's own min-max spread, at every batch, forward and forward + backward.  The ratio is printed whatever
it is.  Every timed output is checked as finite.
Model, the reference's constants (32 x 32 x 3, dims 128 / 256 / 256 / 256, key_dim 16) with bf16 products under BLA_UNET_ATTENTION_BF16_ONLINE at each batch: a
forward + backward pass at heads = 4 beside heads = 1.  NO CLAIM: four heads do four times the attention work."""
import argparse, ctypes as C, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from __graft_entry__ import load_pkg
from inputs import uniform

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="64,16")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warm", type=float, default=1.0, help="seconds of 4096^3 fp32 products before the first measurement (0 = cold)")
ap.add_argument("--no-model", action="store_true")
a = ap.parse_args()
bla = load_pkg(); bla.init(0); L = bla.lib(); chk = bla.native.check
st = L.bla_default_stream()
e0, e1 = C.c_void_p(), C.c_void_p(); chk(L.bla_event_create(C.byref(e0))); chk(L.bla_event_create(C.byref(e1)))
CH, S, HEADS, DH = 256, 16, 4, 16


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


def show(res):
    for n, t in res.items():
        print(f"  {n:<44} median {np.median(t) * 1000:10.3f} us  [{t.min() * 1000:10.3f} .. {t.max() * 1000:10.3f}]", flush=True)


def claim(res, new, old):
    dd, spread = np.median(res[old]) - np.median(res[new]), res[old].max() - res[old].min()
    verdict = "HOLDS" if dd > spread else "FAILS"
    print(f"  claim ({new}) is faster than ({old}): difference of medians {dd * 1000:.3f} us against the baseline's min-max spread of {spread * 1000:.3f} us: "
          f"{verdict} ({np.median(res[old]) / np.median(res[new]):.2f} x)", flush=True)
    return verdict == "HOLDS"


def warm_up():
    if a.warm > 0:
        wa = bla.to_device(uniform(1, (4096, 4096), dtype=np.float32)); wc = bla.empty((4096, 4096))
        t0 = time.time()
        while time.time() - t0 < a.warm:
            for _ in range(20):
                bla.gemm(wa, wa, wc, stream=st)
            bla.sync()
        print(f"# warmed up for {a.warm:.1f} s of 4096^3 fp32 products", flush=True)


class Block:
    """operands and workspaces of one block of width `width` (heads of width d) at batch B"""

    def __init__(self, B, heads, d, weights=None):
        c, s, width = CH, S, heads * d
        gc, gd = np.sqrt(3.0 / c), np.sqrt(3.0 / width)
        I = weights or dict(wq=uniform(2, (c, width), -1.5 * gc, 1.5 * gc, np.float32), wk=uniform(3, (c, width), -1.5 * gc, 1.5 * gc, np.float32),
                            wv=uniform(4, (c, width), -gc, gc, np.float32), w=uniform(5, (width, c), -gd, gd, np.float32))
        self.I = dict(I, x=uniform(1, (B, c, s), -1, 1, np.float32), bias=uniform(6, (c,), -0.5, 0.5, np.float32), dy=uniform(7, (B, c, s), -1, 1, np.float32))
        self.B, self.heads, self.d = B, heads, d
        self.D = {n: bla.to_device(np.ascontiguousarray(v)) for n, v in self.I.items()}
        sizes = dict(q=B * s * width, k=B * s * width, v=B * s * width, scores_raw=B * heads * s * s, weights=B * heads * s * s, attention=B * s * width)
        self.fw = {n: bla.empty((sz,)) for n, sz in sizes.items()}; self.gw = {n: bla.empty((sz,)) for n, sz in sizes.items()}
        self.fws, self.gws = bla.attention_ws(**self.fw), bla.attention_ws(**self.gw)
        self.out, self.dx, self.part = bla.empty((B * c * s,)), bla.empty((B * c * s,)), bla.empty((B * c * width,))
        self.dwq, self.dwk, self.dwv, self.dw = (bla.empty((c * width,)) for _ in range(4))

    def head(self, h):
        sl = slice(h * self.d, (h + 1) * self.d)
        return Block(self.B, 1, self.d, dict(wq=self.I["wq"][:, sl], wk=self.I["wk"][:, sl], wv=self.I["wv"][:, sl], w=self.I["w"][sl]))

    def entry(self, fused):
        D = self.D
        af = (st, self.B, D["x"].ptr, D["wq"].ptr, D["wk"].ptr, D["wv"].ptr, D["w"].ptr, D["bias"].ptr, C.byref(self.fws), self.out.ptr)
        ab = (st, self.B, D["dy"].ptr, D["x"].ptr, D["wq"].ptr, D["wk"].ptr, D["wv"].ptr, D["w"].ptr, C.byref(self.fws), C.byref(self.gws), self.part.ptr,
              self.dwq.ptr, self.dwk.ptr, self.dwv.ptr, self.dw.ptr, self.dx.ptr)
        if fused:
            tail = (CH, S, self.heads, self.d)
            return (lambda: chk(L.bla_attention_forward_batched_f32_heads(*af, *tail))), (lambda: chk(L.bla_attention_backward_batched_f32_heads(*ab, *tail)))
        return (lambda: chk(L.bla_attention_forward_batched_f32(*af, CH, S, self.d))), (lambda: chk(L.bla_attention_backward_batched_f32(*ab, CH, S, self.d, 0)))

    def finite(self):
        return all(np.isfinite(t.numpy()).all() for t in (self.out, self.dx, self.dw, self.dwq, self.dwk, self.dwv))


def block_part(B):
    blk = Block(B, HEADS, DH)
    per_head = [blk.head(h) for h in range(HEADS)]
    fwd, bwd = blk.entry(True)
    each = [p.entry(False) for p in per_head]
    calls = {"forward, heads": fwd, "forward + backward, heads": lambda: (fwd(), bwd()),
             "forward, serial": lambda: [f() for f, _ in each],
             "forward + backward, serial": lambda: [(f(), b()) for f, b in each]}      # (a head's backward reads what its own forward saved)
    for call in calls.values():
        call()
    bla.sync()
    warm_up()
    print(f"== block: C = {CH}, S = {S}, heads = {HEADS}, d = {DH}, batch {B}: medians of {a.rounds} alternating rounds of {a.iters} calls", flush=True)
    res = rounds(calls, a.iters)
    calls["forward + backward, serial"](); calls["forward + backward, heads"](); bla.sync()
    assert blk.finite() and all(p.finite() for p in per_head)
    close = np.allclose(blk.fw["attention"].numpy().reshape(B, S, HEADS * DH)[:, :, :DH].ravel(), per_head[0].fw["attention"].numpy(), rtol=1e-4, atol=1e-5)
    print(f" outputs finite; head 0's attention of the fused entries {'agrees with' if close else 'DIFFERS FROM'} the single-head block on its slices (1e-4)", flush=True)
    show(res)
    for n in ("heads", "serial"):
        print(f"  backward alone, {n} (difference of the medians above): {(np.median(res[f'forward + backward, {n}']) - np.median(res[f'forward, {n}'])) * 1000:10.3f} us")
    return all([claim(res, f"{kind}, heads", f"{kind}, serial") for kind in ("forward", "forward + backward")]) and close


class Cfg(C.Structure):
    _fields_ = [("image_h", C.c_int), ("image_w", C.c_int), ("in_channels", C.c_int), ("dims", C.c_int * 4), ("time_dim", C.c_int), ("kernel", C.c_int),
                ("group_size", C.c_int), ("key_dim", C.c_int)]


def model_part(B):
    cfg = Cfg(32, 32, 3, (C.c_int * 4)(128, 256, 256, 256), 512, 3, 32, 16)
    x, temb, noise = (bla.to_device(uniform(11 + i, shp, -1, 1, np.float32)) for i, shp in enumerate(((B, 3, 32, 32), (B, 512), (B, 3, 32, 32))))
    calls, models = {}, []
    for heads in (1, 4):
        h = bla.unet_create_heads(cfg, B, bla.UNET_PRODUCTS_BF16, heads)
        bla.unet_set_attention(h, bla.UNET_ATTENTION_BF16_ONLINE)
        n = L.bla_unet_param_count(h)
        rng = np.random.default_rng(5)
        flat = (rng.standard_normal(n) * 0.02).astype(np.float32)
        chk(L.bla_memcpy_h2d(L.bla_unet_params(h), flat.ctypes.data, flat.nbytes, None)); bla.sync()
        models.append(h)
        calls[f"forward + backward, heads = {heads}"] = (lambda h=h: (chk(L.bla_unet_forward_f32(h, st, x.ptr, temb.ptr, None)), chk(L.bla_unet_backward_f32(h, st, noise.ptr))))
    for call in calls.values():
        call()
    bla.sync()
    warm_up()
    print(f"== model: the reference's constants, bf16 products, BLA_UNET_ATTENTION_BF16_ONLINE, batch {B}: medians of {a.rounds} alternating rounds of 3 passes", flush=True)
    res = rounds(calls, 3)
    for h in models:
        g = np.empty(L.bla_unet_param_count(h), np.float32)
        chk(L.bla_memcpy_d2h(g.ctypes.data, L.bla_unet_grads(h), g.nbytes, None)); bla.sync()
        assert np.isfinite(g).all()
        chk(L.bla_unet_destroy(h))
    show(res)
    one, four = np.median(res["forward + backward, heads = 1"]), np.median(res["forward + backward, heads = 4"])
    print(f"  heads = 4 costs {(four - one) * 1000:.1f} us a pass more than heads = 1 ({four / one:.3f} x); no claim")


ok = all([block_part(B) for B in map(int, a.batches.split(","))])
print(f"THE CLAIM (the fused fp32 heads entries beat four serial single-head fp32 calls at every batch, forward and forward + backward): {'HOLDS' if ok else 'FAILS'}")
if not a.no_model:
    for B in map(int, a.batches.split(",")):
        model_part(B)
sys.exit(0)
