#!/usr/bin/env python3
"""bla_gemm_bf16 beside bla_gemm_f32 on the same shape and layout: kernel-level timing (HIP events), alternating rounds in one process.
usage: gemm_bf16_sweep.py [--sizes 1024,2048,4096,8192] [--layouts nt] [--rounds 7] [--iters 10] [--out f32|bf16]
Operands are uniform random in [-1, 1) (zero-filled operands read high); the bf16 operands are the fp32 ones rounded on the device."""
import argparse, ctypes as C, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from __graft_entry__ import load_pkg
from inputs import uniform

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="1024,2048,4096,8192")
ap.add_argument("--layouts", default="nt")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--out", default="f32", choices=["f32", "bf16"])
ap.add_argument("--warm", type=float, default=1.0, help="seconds of 4096^3 fp32 products before the first measurement (the clocks ramp for about that long; 0 = cold)")
a = ap.parse_args()
bla = load_pkg(); bla.init(0); L = bla.lib(); chk = bla.native.check
st = L.bla_default_stream()
e0, e1 = C.c_void_p(), C.c_void_p(); chk(L.bla_event_create(C.byref(e0))); chk(L.bla_event_create(C.byref(e1)))
chk(L.bla_gemm_set_config(-1, 0))
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
    call()                                   # one untimed launch in front (also grows the workspace before the timed ones)
    chk(L.bla_event_record(e0, st))
    for _ in range(a.iters):
        call()
    chk(L.bla_event_record(e1, st))
    ms = C.c_float(); chk(L.bla_event_elapsed_ms(e0, e1, C.byref(ms)))
    return ms.value / a.iters, L.bla_gemm_last_kernel().decode()


for spec in a.sizes.split(","):
    dims = [int(x) for x in spec.split("x")]
    m, k, n = (dims * 3)[:3] if len(dims) == 1 else dims
    for lay in a.layouts.split(","):
        ta, tb = lay[0] == "t", lay[1] == "t"
        A = bla.to_device(uniform(1, (k, m) if ta else (m, k), dtype=np.float32))
        B = bla.to_device(uniform(2, (n, k) if tb else (k, n), dtype=np.float32))
        A16, B16 = bla.empty(A.shape, np.uint16), bla.empty(B.shape, np.uint16)
        chk(L.bla_f32_to_bf16(st, A.ptr, A.ld, A16.ptr, A16.ld, A.shape[0], A.shape[1]))
        chk(L.bla_f32_to_bf16(st, B.ptr, B.ld, B16.ptr, B16.ld, B.shape[0], B.shape[1]))
        C32 = bla.empty((m, n)); Cb = bla.empty((m, n), np.uint16 if a.out == "bf16" else np.float32)
        calls = {"bf16": lambda: bla.gemm_bf16(A16, B16, Cb, transa=ta, transb=tb, stream=st),
                 "f32": lambda: bla.gemm(A, B, C32, transa=ta, transb=tb, stream=st)}
        res, names = {w: [] for w in calls}, {}
        for r in range(a.rounds + 1):        # round 0 is a rehearsal
            for w, call in calls.items():
                ms, names[w] = timed(call)
                if r > 0:
                    res[w].append(ms)
        fl = 2.0 * m * n * k
        med = {w: float(np.median(res[w])) for w in calls}
        for w in calls:
            t = np.array(res[w])
            print(f"{m}x{k}x{n} {lay} {w:<4} {names[w]:<52} median {med[w]*1e3:9.1f} us  min {t.min()*1e3:9.1f} us  max {t.max()*1e3:9.1f} us  "
                  f"{fl/med[w]/1e9:8.2f} TF/s median  {fl/t.min()/1e9:8.2f} best  {fl/t.max()/1e9:8.2f} worst", flush=True)
        print(f"{m}x{k}x{n} {lay} bf16 / f32 rate (medians of {a.rounds} alternating rounds): {med['f32'] / med['bf16']:.2f}x", flush=True)
        del A, B, A16, B16, C32, Cb
