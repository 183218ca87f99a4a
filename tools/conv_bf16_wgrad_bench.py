#!/usr/bin/env python3
"""The implicit bf16 weight gradient beside the materialised one: kernel-level timing (HIP events), one process, medians and [min ... max]
of alternating rounds on the same buffers; what was timed is checked against float64 in the same run.  The method of gemm_bf16_splitk_bench.py.
usage: conv_bf16_wgrad_bench.py [--convs 128x128x32x64,256x256x16x64] [--rounds 7] [--iters 20] [--warm 1.0]
  conv = CxFxHWxB, k = 3, stride 1
Per convolution, the new code:
  (1) bla_conv2d_weight_gradient_gathered_bf16 on prepared copies (Q, P made once outside the timing), splits = 0;
  (2) bla_conv2d_backward_gathered_f32_as_bf16 with d_del_x = NULL (two pad passes + the product);
  (3) bla_conv2d_backward_gathered_f32_as_bf16 whole;
and beside them the code as it was:
  (4) bla_conv2d_weight_gradient_batched_f32_as_bf16, splits = 0 (the two operand passes + the dense split product);
  (5) that entry followed by bla_conv2d_backward_batched_f32_as_bf16 with d_del_kern = NULL (the whole backward pass);
  (6) bla_gemm_bf16_splitk, nt, splits = 0, on the same m = F, n = C k k, k = N (the dense product alone).
Checks: del_kern of (1), (2), (4) on 4 filters, all channels and taps, against the float64 weight gradient of the bf16 values inside
(N + 8) 2^-23 (|del_y| * |x|) + 2 2^-24 |ref|; del_x of (3) equals (5)'s bit for bit.  Operands are uniform in [-1, 1) rounded to bf16."""
import argparse, ctypes as C, os, re, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from __graft_entry__ import load_pkg
from inputs import uniform

ap = argparse.ArgumentParser()
ap.add_argument("--convs", default="128x128x32x64,256x256x16x64")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warm", type=float, default=1.0, help="seconds of 4096^3 fp32 products before the first measurement (the clocks ramp for about that long; 0 = cold)")
a = ap.parse_args()
bla = load_pkg(); bla.init(0); L = bla.lib(); chk = bla.native.check
st = L.bla_default_stream()
e0, e1 = C.c_void_p(), C.c_void_p(); chk(L.bla_event_create(C.byref(e0))); chk(L.bla_event_create(C.byref(e1)))
buf = C.create_string_buffer(128); chk(L.bla_device_name(buf, 128))
CUS = int(re.search(rb"\((\d+) CUs\)", buf.value).group(1))
print(f"# {buf.value.decode()}; medians of {a.rounds} alternating rounds of {a.iters} launches", flush=True)
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


def rounds(calls):
    """{name: call} -> {name: (array of per-round ms, kernel name)}; round 0 is a rehearsal"""
    res, names = {w: [] for w in calls}, {}
    for r in range(a.rounds + 1):
        for w, call in calls.items():
            ms, names[w] = timed(call)
            if r > 0:
                res[w].append(ms)
    return {w: (np.array(res[w]), names[w]) for w in calls}


def line(label, t, extra=""):
    return f"  {label:<58} median {np.median(t)*1e3:9.1f} us  [{t.min()*1e3:9.1f} ... {t.max()*1e3:9.1f}]  {extra}"


def wgrad_rows_f64(x, dy, fs, k):
    """del_kern[f][c][p][q] for f in fs (stride 1, SAME, odd k) and the same on magnitudes: sums over (b, i, j) of dy[b][f][i][j] x[b][c][i+p-pad][j+q-pad]"""
    Bn, c, h, w = x.shape
    pad = (k - 1) // 2
    xp = np.zeros((Bn, c, h + k - 1, w + k - 1), np.float64); xp[:, :, pad:pad + h, pad:pad + w] = x
    d = dy[:, fs].astype(np.float64).transpose(1, 0, 2, 3).reshape(len(fs), -1)
    ref, mag = np.zeros((len(fs), c, k, k)), np.zeros((len(fs), c, k, k))
    for p in range(k):
        for q in range(k):
            xs = xp[:, :, p:p + h, q:q + w].transpose(1, 0, 2, 3).reshape(c, -1)
            ref[:, :, p, q] = d @ xs.T
            mag[:, :, p, q] = np.abs(d) @ np.abs(xs).T
    return ref, mag


r8 = lambda v: -(-v // 8) * 8
for spec in [s for s in a.convs.split(",") if s]:
    c, f, hw, Bn = [int(v) for v in spec.split("x")]
    h = w = hw; k, s = 3, 1
    n, cp, fp = Bn * h * w, r8(c), r8(f)
    n8 = r8(n)
    xh = bla.from_bf16(bla.to_bf16(uniform(1, (Bn, c, h, w), dtype=np.float32))); dyh = bla.from_bf16(bla.to_bf16(uniform(3, (Bn, f, h, w), dtype=np.float32)))
    x, dy = bla.to_device(xh), bla.to_device(dyh)
    kern = bla.to_device(uniform(2, (f, c, k, k), dtype=np.float32))
    dx, dx_old, dk = bla.empty((Bn, c, h, w)), bla.empty((Bn, c, h, w)), bla.empty((f, c, k, k))
    hp, wp, top, left, dil = bla.conv_bf16_layout(h, w, k, s)
    P = bla.conv_bf16_pad(x, bla.empty((Bn, hp, wp, cp), np.uint16), Bn, c, h, w, hp, wp, top, left, dil, stream=st)
    hq, wq, qtop, qleft, qdil = bla.conv_bf16_layout(h, w, k, s, True)
    Q = bla.conv_bf16_pad(dy, bla.empty((Bn, hq, wq, fp), np.uint16), Bn, f, h, w, hq, wq, qtop, qleft, qdil, stream=st)
    counts = (f * n8, c * k * k * n8)
    src = bla.to_device(uniform(4, (max(counts),), dtype=np.float32))
    Y16, G16 = (bla.empty((cnt,), np.uint16) for cnt in counts)
    for dst, cnt in zip((Y16, G16), counts):
        chk(L.bla_f32_to_bf16(st, src.ptr, cnt, dst.ptr, cnt, 1, cnt))
    bla.sync(); del src
    calls = {
        "1  new: gathered weight gradient on prepared copies": lambda: bla.conv2d_weight_gradient_gathered_bf16(Q, hq, wq, fp, qtop, qleft, qdil, P, hp, wp, cp, Bn, k, s, h, w, f, c,
                                                                                                                dk, splits=0, stream=st),
        "2  new: backward_gathered, del_x = NULL (2 pads + product)": lambda: bla.conv2d_backward_gathered_as_bf16(dy, x, None, dk, None, Bn, h, w, k, c, f, s, splits=0, stream=st),
        "3  new: backward_gathered whole": lambda: bla.conv2d_backward_gathered_as_bf16(dy, x, kern, dk, dx, Bn, h, w, k, c, f, s, splits=0, stream=st),
        "4  old: materialised weight-gradient entry, splits = 0": lambda: bla.conv2d_weight_gradient_as_bf16(dy, x, dk, Bn, h, w, k, c, f, s, splits=0, stream=st),
        "5  old: that entry + backward entry with del_kern = NULL": lambda: (bla.conv2d_weight_gradient_as_bf16(dy, x, dk, Bn, h, w, k, c, f, s, splits=0, stream=st),
                                                                             bla.conv2d_backward_as_bf16(dy, None, kern, None, dx_old, Bn, h, w, k, c, f, s, stream=st)),
        "6  old: bla_gemm_bf16_splitk nt alone, splits = 0": lambda: bla.gemm_bf16_splitk(Y16, G16, dk, transb=True, m=f, n=c * k * k, k=n8, lda=n8, ldb=n8, ldc=c * k * k,
                                                                                          stream=st, splits=0),
    }
    res = rounds(calls)
    eff, sps, _ = bla.gemm_bf16_splitk_plan(f, k * k * cp, n, 0, CUS)
    tiles = -(-f // 128) * -(-(k * k * cp) // 128)
    print(f"== conv {c}->{f} @{h}x{w} x{Bn}, k {k}, stride {s}: implicit product {f} x {k*k*cp} x {n}: {tiles} tiles, plan S_eff {eff} sps {sps}, "
          f"partials {eff*tiles*65536/2**20:.1f} MiB", flush=True)
    fs = [0, 1, f // 2, f - 1]
    ref, mag = wgrad_rows_f64(xh, dyh, fs, k)
    bound = (n + 8) * 2.0 ** -23 * mag + 2 * 2.0 ** -24 * np.abs(ref)
    for w_ in [v for v in calls if v[0] in "124"]:
        dk.fill_bytes(0xFF); calls[w_](); bla.sync()
        err = np.abs(dk.numpy()[fs].astype(np.float64) - ref)
        ratio = float(np.max(np.where(np.isnan(err), np.inf, err) / bound))
        print(f"  check {w_[3:]}: worst err/bound {ratio:.4f} on filters {fs} {'ok' if ratio <= 1 else 'OUTSIDE THE BOUND'}", flush=True)
    dx.fill_bytes(0xFF); dx_old.fill_bytes(0xFF)
    calls["3  new: backward_gathered whole"](); calls["5  old: that entry + backward entry with del_kern = NULL"](); bla.sync()
    same = np.array_equal(dx.numpy().view(np.uint32), dx_old.numpy().view(np.uint32))
    print(f"  check del_x of (3) against (5): {'bit-identical' if same else 'DIFFERENT'}", flush=True)
    for w_ in calls:
        t, name = res[w_]
        print(line(w_, t, name), flush=True)
    t = {w_[0]: res[w_][0] for w_ in calls}
    med = {i: float(np.median(v)) for i, v in t.items()}
    spread = t["4"].max() - t["4"].min()
    gain = med["4"] - med["2"]
    verdict = "faster by more than (4)'s spread" if gain > spread else ("within (4)'s spread" if abs(gain) <= spread else "SLOWER beyond (4)'s spread")
    print(f"  weight gradient: (2) / (4) = {med['2']/med['4']:.2f} of the time ({med['4']/med['2']:.2f}x); (4)'s spread {spread*1e3:.1f} us, gain {gain*1e3:.1f} us: {verdict}", flush=True)
    print(f"  pads = (2) - (1): {(med['2']-med['1'])*1e3:.1f} us; operand passes of the old entry = (4) - (6): {(med['4']-med['6'])*1e3:.1f} us; "
          f"implicit product / dense product = (1) / (6) = {med['1']/med['6']:.2f}", flush=True)
    print(f"  whole backward: (3) / (5) = {med['3']/med['5']:.2f} of the time ({med['5']/med['3']:.2f}x)", flush=True)
    del x, dy, kern, dx, dx_old, dk, P, Q, Y16, G16
