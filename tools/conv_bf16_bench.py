#!/usr/bin/env python3
"""The bf16 convolution beside the fp32 batched entries on the same shape: kernel-level timing (HIP events), medians of alternating rounds in one process.
usage: conv_bf16_bench.py [--shapes 128x128x32x64,256x256x16x64] [--rounds 7] [--iters 20] [--warm 1.0]        shape = CxFxHWxB, k = 3, stride 1
Per shape:
  (a) bla_conv2d_forward_batched_f32                 the yardstick
  (b) bla_conv2d_gathered_bf16 alone                 operands already padded / prepared
  (c) bla_conv_bf16_pad + (b)                        kernels prepared once outside the loop, as a trainer would
  (d) bla_gemm_bf16 nt on the dense shape of (b)     m = F, n = B Ho Wo, k = k k Cp: the gather kernel's ceiling
  (e) bla_conv2d_backward_batched_f32 beside bla_conv2d_backward_batched_f32_as_bf16, the latter also per gradient, with the passes in front of each
      product timed alone where an entry exists (pad of del_y, kernel preparation) or given as entry - product (the im2col and del_y conversion passes)
Operands are uniform random in [-0.5, 0.5)."""
import argparse, ctypes as C, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from __graft_entry__ import load_pkg
from inputs import uniform

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="128x128x32x64,256x256x16x64")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warm", type=float, default=1.0, help="seconds of 4096^3 fp32 products before the first measurement (the clocks ramp for about that long; 0 = cold)")
a = ap.parse_args()
bla = load_pkg(); bla.init(0); L = bla.lib(); chk = bla.native.check
st = L.bla_default_stream()
e0, e1 = C.c_void_p(), C.c_void_p(); chk(L.bla_event_create(C.byref(e0))); chk(L.bla_event_create(C.byref(e1)))
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
    return ms.value / a.iters


r8 = lambda v: -(-v // 8) * 8
for spec in a.shapes.split(","):
    c, f, hw, B = [int(v) for v in spec.split("x")]
    h = w = hw; k, s = 3, 1
    cp, fp, n = r8(c), r8(f), B * h * w
    x = bla.to_device(uniform(1, (B, c, h, w), dtype=np.float32)); kern = bla.to_device(uniform(2, (f, c, k, k), dtype=np.float32))
    dy = bla.to_device(uniform(3, (B, f, h, w), dtype=np.float32))
    out, dx, dk, scratch = bla.empty((B, f, h, w)), bla.empty((B, c, h, w)), bla.empty((f, c, k, k)), bla.empty((f * c * k * k,))
    hp, wp, top, left, dil = bla.conv_bf16_layout(h, w, k, s)
    P, A = bla.empty((B, hp, wp, cp), np.uint16), bla.empty((f, k * k * cp), np.uint16)
    bla.conv_bf16_pad(x, P, B, c, h, w, hp, wp, top, left, dil, stream=st); bla.conv_bf16_prepare_kernels(kern, A, f, c, k, stream=st)
    hpd, wpd, topd, leftd, dild = bla.conv_bf16_layout(h, w, k, s, True)
    Pd, Ad = bla.empty((B, hpd, wpd, fp), np.uint16), bla.empty((c, k * k * fp), np.uint16)
    bla.conv_bf16_pad(dy, Pd, B, f, h, w, hpd, wpd, topd, leftd, dild, stream=st); bla.conv_bf16_prepare_kernels(kern, Ad, f, c, k, True, stream=st)
    n8 = r8(n)
    # random bf16 operands for the dense products, rounded on the device from one fp32 buffer: (d)'s B [n][k k Cp]; the weight gradient's dY16 and G alone
    counts = (n * k * k * cp, f * n8, c * k * k * n8)
    src = bla.to_device(uniform(4, (max(counts),), dtype=np.float32))
    Bd, Y16, G16 = (bla.empty((cnt,), np.uint16) for cnt in counts)
    for dst, cnt in zip((Bd, Y16, G16), counts):
        chk(L.bla_f32_to_bf16(st, src.ptr, cnt, dst.ptr, cnt, 1, cnt))
    bla.sync(); del src
    Cd = bla.empty((f, n))
    calls = {
        "a  forward f32 (yardstick)": lambda: chk(L.bla_conv2d_forward_batched_f32(st, x.ptr, kern.ptr, out.ptr, B, h, w, k, c, f, s)),
        "b  gathered product alone": lambda: bla.conv2d_gathered_bf16(A, f, P, B, hp, wp, cp, k, s, h, w, out, stream=st),
        "c  pad + gathered product": lambda: (bla.conv_bf16_pad(x, P, B, c, h, w, hp, wp, top, left, dil, stream=st),
                                              bla.conv2d_gathered_bf16(A, f, P, B, hp, wp, cp, k, s, h, w, out, stream=st)),
        "c' forward _as_bf16 entry": lambda: bla.conv2d_forward_as_bf16(x, kern, out, B, h, w, k, c, f, s, stream=st),
        "d  gemm_bf16 nt, dense": lambda: bla.gemm_bf16(A, Bd, Cd, transb=True, m=f, n=n, k=k * k * cp, ldb=k * k * cp, stream=st),
        "e  backward f32": lambda: chk(L.bla_conv2d_backward_batched_f32(st, dy.ptr, x.ptr, kern.ptr, dk.ptr, dx.ptr, scratch.ptr, B, h, w, k, c, f, s)),
        "e  backward _as_bf16, both": lambda: bla.conv2d_backward_as_bf16(dy, x, kern, dk, dx, B, h, w, k, c, f, s, stream=st),
        "e  .. weight gradient only": lambda: bla.conv2d_backward_as_bf16(dy, x, kern, dk, None, B, h, w, k, c, f, s, stream=st),
        "e  .... its gemm_bf16 nt alone": lambda: bla.gemm_bf16(Y16, G16, dk, transb=True, m=f, n=c * k * k, k=n8, lda=n8, ldb=n8, ldc=c * k * k, stream=st),
        "e  .. data gradient only": lambda: bla.conv2d_backward_as_bf16(dy, None, kern, None, dx, B, h, w, k, c, f, s, stream=st),
        "e  .... pad of del_y alone": lambda: bla.conv_bf16_pad(dy, Pd, B, f, h, w, hpd, wpd, topd, leftd, dild, stream=st),
        "e  .... kernel preparation alone": lambda: bla.conv_bf16_prepare_kernels(kern, Ad, f, c, k, True, stream=st),
        "e  .... its gathered product alone": lambda: bla.conv2d_gathered_bf16(Ad, c, Pd, B, hpd, wpd, fp, k, 1, h, w, dx, stream=st),
    }
    res = {name: [] for name in calls}
    for r in range(a.rounds + 1):            # round 0 is a rehearsal
        for name, call in calls.items():
            ms = timed(call)
            if r > 0:
                res[name].append(ms)
    med = {name: float(np.median(v)) for name, v in res.items()}
    fl = 2.0 * f * n * k * k * c
    print(f"== {c}->{f} @{h}x{w} x{B}, k {k}, stride {s}: {fl/1e9:.2f} GFLOP per product; medians of {a.rounds} alternating rounds of {a.iters} launches", flush=True)
    for name in calls:
        t = np.array(res[name])
        rate = f"{fl/med[name]/1e9:8.2f} TF/s" if name[0] in "abcd" else " " * 13
        print(f"  {name:<36} median {med[name]*1e3:9.1f} us  min {t.min()*1e3:9.1f}  max {t.max()*1e3:9.1f}  {rate}", flush=True)
    ya, yb, yc, yd = (med[n_] for n_ in list(calls)[:3] + ["d  gemm_bf16 nt, dense"])
    print(f"  (c) / (a) = {yc/ya:.2f} of the fp32 time ({ya/yc:.2f}x);  (b) / (d) = {yb/yd:.2f};  pad = (c) - (b) = {(yc-yb)*1e3:.1f} us", flush=True)
    wg, wgg = med["e  .. weight gradient only"], med["e  .... its gemm_bf16 nt alone"]
    print(f"  weight gradient: im2col + del_y conversion passes = entry - product = {(wg-wgg)*1e3:.1f} us of {wg*1e3:.1f} us", flush=True)
    print(f"  backward _as_bf16 / backward f32 = {med['e  backward _as_bf16, both']/med['e  backward f32']:.2f} of the fp32 time", flush=True)
    del x, kern, dy, out, dx, dk, scratch, P, A, Pd, Ad, Bd, Cd, Y16, G16
