#!/usr/bin/env python3
"""The multi-head online bf16 attention block (bla_attention_{forward,backward}_batched_online_bf16_heads) beside what a caller had before
it: HIP events, one process, a pre-roll of 4096^3 fp32 products, medians [min .. max] of alternating rounds (tools/attention_online_bench.py's method).
usage: attention_heads_bench.py [--batches 16,64] [--rounds 7] [--iters 10] [--warm 1.0] [--against OTHER/libbla_hip.so] [--trace N]
At C = 256, S = 1024 and each batch, for (heads, d) = (4, 16) and (4, 64), forward calls and forward + backward pairs of
  heads:    the new entries;
  wide:     for (4, 16) only, the single-head online entry at d = 64: the same projection and score FLOPs, a quarter of the exponentials (context, no claim);
  serial:   `heads` consecutive calls of the single-head online entry on contiguous copies of the heads' slices of the weights, which is what a caller
            could do before, WITHOUT the two sums across heads (out and del_x of the last head stay in the buffers): a lower bound of that workaround.
The claim: heads is faster than serial by more than serial's own min-max spread, at every batch.  The ratio is printed whatever it is.  Every timed output
is checked as finite, and heads' tensors of head 0 are compared with serial's first call (the same bits).
--against: the single-head online entry of THIS build against another build of the library (the parent commit's libbla_hip.so) at C = 256, S = 1024, d = 16,
batch 64, alternating rounds in one process: the walking kernels gained a stride argument and a grid plane, and must not have slowed the entries that exist.
--trace N: no timing, N forward + backward pairs of the new entries at (4, 16) and (4, 64), batch 64, for `rocprofv3 --kernel-trace --stats --`."""
import argparse, ctypes as C, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from __graft_entry__ import load_pkg
from inputs import uniform

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="16,64")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warm", type=float, default=1.0, help="seconds of 4096^3 fp32 products before the first measurement (0 = cold)")
ap.add_argument("--against", default=None)
ap.add_argument("--trace", type=int, default=0)
a = ap.parse_args()
bla = load_pkg(); bla.init(0); L = bla.lib(); chk = bla.native.check
st = L.bla_default_stream()
e0, e1 = C.c_void_p(), C.c_void_p(); chk(L.bla_event_create(C.byref(e0))); chk(L.bla_event_create(C.byref(e1)))
CH, S = 256, 1024


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


def claim(res, new, old, what):
    dd, spread = np.median(res[old]) - np.median(res[new]), res[old].max() - res[old].min()
    verdict = "HOLDS" if dd > (spread if what == "faster" else -spread) else "FAILS"
    print(f"  claim ({new}) is {what} than ({old}): difference of medians {dd * 1000:.3f} us against the baseline's min-max spread of {spread * 1000:.3f} us: "
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
    """operands and workspaces of one block of width `width` at batch B; entry(lib, heads, d) -> (forward call, backward call)"""

    def __init__(self, B, width, weights=None):
        c, s = CH, S
        gc, gd = np.sqrt(3.0 / c), np.sqrt(3.0 / width)
        I = weights or dict(wq=uniform(2, (c, width), -1.5 * gc, 1.5 * gc, np.float32), wk=uniform(3, (c, width), -1.5 * gc, 1.5 * gc, np.float32),
                            wv=uniform(4, (c, width), -gc, gc, np.float32), w=uniform(5, (width, c), -gd, gd, np.float32))
        self.I = dict(I, x=uniform(1, (B, c, s), -1, 1, np.float32), bias=uniform(6, (c,), -0.5, 0.5, np.float32), dy=uniform(7, (B, c, s), -1, 1, np.float32))
        self.B, self.width = B, width
        self.D = {n: bla.to_device(np.ascontiguousarray(v)) for n, v in self.I.items()}
        sizes = dict(q=B * s * width, k=B * s * width, v=B * s * width, scores_raw=B * s * 16, attention=B * s * width)
        self.fw = {n: bla.empty((sz,)) for n, sz in sizes.items()}; self.gw = {n: bla.empty((sz,)) for n, sz in sizes.items()}
        self.fws, self.gws = bla.attention_ws(**self.fw), bla.attention_ws(**self.gw)
        self.out, self.dx, self.part = bla.empty((B * c * s,)), bla.empty((B * c * s,)), bla.empty((B * 4 * c * width,))
        self.dwq, self.dwk, self.dwv, self.dw = (bla.empty((c * width,)) for _ in range(4))

    def head(self, h, d):
        sl = slice(h * d, (h + 1) * d)
        return Block(self.B, d, dict(wq=self.I["wq"][:, sl], wk=self.I["wk"][:, sl], wv=self.I["wv"][:, sl], w=self.I["w"][sl]))

    def entry(self, lib, heads, d):
        D = self.D
        tail = (CH, S, d) if heads is None else (CH, S, heads, d)
        f, b = ((lib.bla_attention_forward_batched_online_bf16, lib.bla_attention_backward_batched_online_bf16) if heads is None else
                (lib.bla_attention_forward_batched_online_bf16_heads, lib.bla_attention_backward_batched_online_bf16_heads))
        af = (st, self.B, D["x"].ptr, D["wq"].ptr, D["wk"].ptr, D["wv"].ptr, D["w"].ptr, D["bias"].ptr, C.byref(self.fws), self.out.ptr) + tail
        ab = (st, self.B, D["dy"].ptr, D["x"].ptr, D["wq"].ptr, D["wk"].ptr, D["wv"].ptr, D["w"].ptr, C.byref(self.fws), C.byref(self.gws), self.part.ptr,
              self.dwq.ptr, self.dwk.ptr, self.dwv.ptr, self.dw.ptr, self.dx.ptr) + tail
        return (lambda: chk(f(*af))), (lambda: chk(b(*ab)))

    def finite(self):
        return all(np.isfinite(t.numpy()).all() for t in (self.out, self.dx, self.dw, self.dwq))


def pairs(calls, name, fwd, bwd):
    calls[f"forward, {name}"] = fwd
    calls[f"forward + backward, {name}"] = lambda: (fwd(), bwd())


def heads_part(B, heads, d):
    blk = Block(B, heads * d)
    per_head = [blk.head(h, d) for h in range(heads)]
    calls = {}
    pairs(calls, "heads", *blk.entry(L, heads, d))
    if heads * d == 64 and d != 64:
        pairs(calls, "wide", *blk.entry(L, None, heads * d))
    each = [p.entry(L, None, d) for p in per_head]
    calls["forward, serial"] = lambda: [f() for f, _ in each]
    calls["forward + backward, serial"] = lambda: [(f(), b()) for f, b in each]      # (a head's backward reads what its own forward saved)
    if a.trace:
        for _ in range(a.trace):
            calls["forward + backward, heads"]()
        bla.sync()
        assert blk.finite()
        print(f"{a.trace} forward + backward pairs of the multi-head entries at C = {CH}, S = {S}, heads = {heads}, d = {d}, batch {B}, outputs finite")
        return True
    for call in calls.values():
        call()
    bla.sync()
    warm_up()
    print(f"== C = {CH}, S = {S}, heads = {heads}, d = {d}, batch {B}: medians of {a.rounds} alternating rounds of {a.iters} calls", flush=True)
    res = rounds(calls, a.iters)
    calls["forward + backward, serial"](); calls["forward + backward, heads"](); bla.sync()
    assert blk.finite() and all(p.finite() for p in per_head)
    same = all(np.array_equal(blk.fw[n].numpy().reshape(B, S, heads * d)[:, :, :d].ravel(), per_head[0].fw[n].numpy()) for n in ("q", "k", "v", "attention"))
    same = same and np.array_equal(blk.dwq.numpy().reshape(CH, heads * d)[:, :d].ravel(), per_head[0].dwq.numpy())
    print(f" outputs finite; head 0 of the multi-head entries {'has the bits of' if same else 'DIFFERS FROM'} the single-head entries on its slices", flush=True)
    show(res)
    for n in ("heads", "serial") + (("wide",) if "forward, wide" in res else ()):
        print(f"  backward alone, {n} (difference of the medians above): {(np.median(res[f'forward + backward, {n}']) - np.median(res[f'forward, {n}'])) * 1000:10.3f} us")
    flop = 4.0 * S * S * heads * d * B
    print(f"  (S x S arithmetic of a forward pass, 4 S^2 D B = {flop / 1e9:.2f} GFLOP: the multi-head forward runs it at "
          f"{flop / np.median(res['forward, heads']) / 1e9:.1f} TFLOP/s, qkv and the output product included in the time)")
    return all([claim(res, f"{kind}, heads", f"{kind}, serial", "faster") for kind in ("forward", "forward + backward")]) and same


def against_part(path):
    """the single-head online entry of this build and of another build of the library, alternating in one process"""
    other = C.CDLL(os.path.abspath(path))
    for name in ("bla_init", "bla_attention_forward_batched_online_bf16", "bla_attention_backward_batched_online_bf16"):
        fn = getattr(other, name)
        fn.restype, fn.argtypes = bla.native.SIGNATURES[name]
    chk(other.bla_init(0))
    blk = Block(64, 16)
    calls = {}
    pairs(calls, "this build", *blk.entry(L, None, 16))
    pairs(calls, "other build", *blk.entry(other, None, 16))
    for call in calls.values():
        call()
    bla.sync()
    warm_up()
    print(f"== the single-head online entries, C = {CH}, S = {S}, d = 16, batch 64, this build against {path}: medians of {a.rounds} alternating rounds of "
          f"{a.iters} calls", flush=True)
    res = rounds(calls, a.iters)
    assert blk.finite()
    show(res)
    return all([claim(res, f"{kind}, this build", f"{kind}, other build", "no slower") for kind in ("forward", "forward + backward")])


if a.against:
    ok = against_part(a.against)
elif a.trace:
    ok = all([heads_part(64, 4, 16), heads_part(64, 4, 64)])
else:
    ok = all([heads_part(B, heads, d) for B in map(int, a.batches.split(",")) for heads, d in ((4, 16), (4, 64))])
    print(f"THE CLAIM (the multi-head entries beat `heads` serial single-head calls at every batch, forward and forward + backward): {'HOLDS' if ok else 'FAILS'}")
sys.exit(0 if ok or a.trace else 1)
