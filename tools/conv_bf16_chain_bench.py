#!/usr/bin/env python3
"""The channel-last bf16 output of the gathered bf16 product (bla_conv2d_gathered_bf16_chained) beside the parent's way to feed the next
layer: kernel-level timing (HIP events), one process, medians [min .. max] of alternating rounds.
usage: conv_bf16_chain_bench.py [--shapes 128x128x32x64,256x256x16x64] [--rounds 7] [--iters 20] [--warm 1.0]        shape = CxFxHWxB, k = 3, stride 1
Per shape, the destination being the padded map of a following k = 3, stride 1 convolution:
  (1) bla_conv2d_gathered_bf16 alone                          the existing product, fp32 [B][F][H][W] out
  (2) (1) + bla_conv_bf16_pad of its output                   the parent's way to make the next layer's operand
  (3) the chained entry, dst only
  (4) the chained entry, dst + out_f32
  (5) the chained entry, dst with bias + relu
Every timed output is checked in the run: (3) and (4) against (2)'s map and (1)'s fp32 output bit for bit, (5) against the same composition with the bias
in (1) and the ReLU in numpy.  Operands are uniform random in [-0.5, 0.5)."""
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
    call()                                   # one untimed launch in front
    chk(L.bla_event_record(e0, st))
    for _ in range(a.iters):
        call()
    chk(L.bla_event_record(e1, st))
    ms = C.c_float(); chk(L.bla_event_elapsed_ms(e0, e1, C.byref(ms)))
    return ms.value / a.iters


r8 = lambda v: -(-v // 8) * 8
U16, U32 = np.uint16, np.uint32
for spec in a.shapes.split(","):
    c, f, hw, B = [int(v) for v in spec.split("x")]
    h = w = hw; k, s = 3, 1
    cp, fp = r8(c), r8(f)
    x = bla.to_device(uniform(1, (B, c, h, w), dtype=np.float32)); kern = bla.to_device(uniform(2, (f, c, k, k), dtype=np.float32))
    bias_h = uniform(3, (B, f), dtype=np.float32); bias = bla.to_device(bias_h)
    hp, wp, top, left, dil = bla.conv_bf16_layout(h, w, k, s)
    P, A = bla.empty((B, hp, wp, cp), U16), bla.empty((f, k * k * cp), U16)
    bla.conv_bf16_pad(x, P, B, c, h, w, hp, wp, top, left, dil, stream=st); bla.conv_bf16_prepare_kernels(kern, A, f, c, k, stream=st)
    # the next layer (k 3, stride 1 on the h x w output): its padded map, one per row so that every timed output can be checked afterwards
    nhp, nwp, ntop, nleft, ndil = bla.conv_bf16_layout(h, w, k, 1)
    out1, out2, out4 = (bla.empty((B, f, h, w)) for _ in range(3))
    N2 = bla.empty((B, nhp, nwp, fp), U16)
    N3, N4, N5 = (bla.zeros((B, nhp, nwp, fp), U16) for _ in range(3))          # zero-filled once: the chained store never touches the halo
    amap = lambda arr: bla.conv_bf16_map(arr, nhp, nwp, fp, ntop, nleft, ndil)
    gathered = lambda out, b=None: bla.conv2d_gathered_bf16(A, f, P, B, hp, wp, cp, k, s, h, w, out, b, f if b else 0, stream=st)
    chained = lambda dst, **kw: bla.conv2d_gathered_bf16_chained(A, f, P, B, hp, wp, cp, k, s, h, w, dst=amap(dst), stream=st, **kw)
    calls = {
        "1  gathered product alone (fp32 out)": lambda: gathered(out1),
        "2  (1) + pad of its output": lambda: (gathered(out2), bla.conv_bf16_pad(out2, N2, B, f, h, w, nhp, nwp, ntop, nleft, ndil, stream=st)),
        "3  chained, dst only": lambda: chained(N3),
        "4  chained, dst + out_f32": lambda: chained(N4, out_f32=out4),
        "5  chained, dst, bias + relu": lambda: chained(N5, ep_bias=bias, ep_bias_stride=f, relu=True),
    }
    res = {name: [] for name in calls}
    for r in range(a.rounds + 1):            # round 0 is a rehearsal
        for name, call in calls.items():
            ms = timed(call)
            if r > 0:
                res[name].append(ms)
    bla.sync()
    # every timed output, checked
    want = N2.numpy()
    ok = [np.array_equal(N3.numpy(), want), np.array_equal(N4.numpy(), want) and np.array_equal(out4.numpy().view(U32), out1.numpy().view(U32))]
    gathered(out2, bias); bla.sync()
    y = out2.numpy()
    bla.conv_bf16_pad(bla.to_device(np.where(y > 0, y, np.float32(0))), N2, B, f, h, w, nhp, nwp, ntop, nleft, ndil, stream=st); bla.sync()
    ok.append(np.array_equal(N5.numpy(), N2.numpy()))
    assert all(ok) and (want != 0).any(), ok
    med = {name: float(np.median(v)) for name, v in res.items()}
    fl = 2.0 * f * B * h * w * k * k * c
    print(f"== {c}->{f} @{h}x{w} x{B}, k {k}, stride {s}: {fl/1e9:.2f} GFLOP per product; medians of {a.rounds} alternating rounds of {a.iters} launches; "
          f"outputs of (3) (4) (5) bit-equal to the parent composition", flush=True)
    for name in calls:
        t = np.array(res[name])
        print(f"  {name:<38} median {med[name]*1e3:8.1f} us  [{t.min()*1e3:8.1f} .. {t.max()*1e3:8.1f}]  {fl/med[name]/1e9:8.2f} TF/s", flush=True)
    t1, t2, t3 = (med[n_] for n_ in list(calls)[:3])
    spread2 = (max(res[list(calls)[1]]) - min(res[list(calls)[1]])) * 1e3
    print(f"  (2) - (3) = {(t2-t3)*1e3:.1f} us against (2)'s own min-max spread of {spread2:.1f} us: (3) is {'FASTER' if (t2-t3)*1e3 > spread2 else 'NOT faster'} by more than "
          f"the spread;  (3) - (1) = {(t3-t1)*1e3:+.1f} us, the price of the channel-last store against the fp32 store;  pad alone = (2) - (1) = {(t2-t1)*1e3:.1f} us", flush=True)
    del x, kern, bias, P, A, out1, out2, out4, N2, N3, N4, N5
