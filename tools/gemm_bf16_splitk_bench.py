#!/usr/bin/env python3
"""The K-split of the bf16 product beside the unsplit kernel, and the weight-gradient entry built on it beside the backward entries: kernel-level timing
(HIP events), one process, medians and [min ... max] of alternating rounds on the same buffers; what was timed is checked against float64 in the same run.
usage: gemm_bf16_splitk_bench.py [--products 128x1152x65536,256x2304x16384,128x1152x4096,1024x1024x8192,4096x4096x4096]
                                 [--convs 128x128x32x64,256x256x16x64] [--rounds 7] [--iters 20] [--warm 1.0]
  product = MxNxK, the nt form (A [M][K], B [N][K]);  conv = CxFxHWxB, k = 3, stride 1
Per product:
  (a) bla_gemm_bf16_splitk with S = 1 (bla_gemm_bf16's own launch: the yardstick) and explicit S = 2, 4, 8, ... up to floor(3 CUs / tiles) and the
      number of slabs; the plan (S_eff, slabs per split) beside each.  This sweep chooses BLA_GEMM_BF16_SPLITK_MIN_SLABS.
  (b) splits = 0, the automatic rule, with the acceptance comparison: faster than S = 1 by more than S = 1's own [min ... max] spread / not slower
      beyond it.
Per convolution:
  (c) bla_conv2d_weight_gradient_batched_f32_as_bf16 at splits = 0 beside bla_conv2d_backward_batched_f32_as_bf16 with d_del_x = NULL; the product
      alone on operands of the same shape, so that the operand passes are entry - product.
  (d) the whole backward pass: the new composition (that entry, then the backward entry with d_del_kern = NULL) beside bla_conv2d_backward_batched_f32
      and beside the unchanged bla_conv2d_backward_batched_f32_as_bf16.
Checks: every timed product against the float64 product of the bf16 values on up to 128 rows (the first and the last 64), all columns, inside
(k + 8) 2^-23 (|A|.|B|) + 2 2^-24 |ref|; the weight gradient the same way on 4 filters, all channels and taps.  Operands are uniform in [-1, 1)."""
import argparse, ctypes as C, os, re, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from __graft_entry__ import load_pkg
from inputs import uniform

ap = argparse.ArgumentParser()
ap.add_argument("--products", default="128x1152x65536,256x2304x16384,128x1152x4096,1024x1024x8192,4096x4096x4096")
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
MIN_SLABS = int(re.search(r"#define\s+BLA_GEMM_BF16_SPLITK_MIN_SLABS\s+(\d+)", open(os.path.join(ROOT, "include", "bla.h")).read()).group(1))
print(f"# {buf.value.decode()}; BLA_GEMM_BF16_SPLITK_MIN_SLABS = {MIN_SLABS}; medians of {a.rounds} alternating rounds of {a.iters} launches", flush=True)
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
    return f"  {label:<44} median {np.median(t)*1e3:9.1f} us  [{t.min()*1e3:9.1f} ... {t.max()*1e3:9.1f}]  {extra}"


def worst_ratio(got, a64, b64, k):
    ref = a64 @ b64.T
    bound = (k + 8) * 2.0 ** -23 * (np.abs(a64) @ np.abs(b64).T) + 2 * 2.0 ** -24 * np.abs(ref)
    err = np.abs(got.astype(np.float64) - ref)
    return float(np.nanmax(np.where(np.isnan(err), np.inf, err) / np.maximum(bound, 1e-300)))


# ---- (a), (b): the product -------------------------------------------------------------------------------------------------------------------------------
for spec in [s for s in a.products.split(",") if s]:
    m, n, k = [int(v) for v in spec.split("x")]
    A = bla.to_device(uniform(1, (m, k), dtype=np.float32)); B = bla.to_device(uniform(2, (n, k), dtype=np.float32))
    A16, B16 = bla.empty((m, k), np.uint16), bla.empty((n, k), np.uint16)
    chk(L.bla_f32_to_bf16(st, A.ptr, k, A16.ptr, k, m, k)); chk(L.bla_f32_to_bf16(st, B.ptr, k, B16.ptr, k, n, k))
    bla.sync(); del A, B
    Cd = bla.empty((m, n))
    tiles, slabs = -(-m // 128) * -(-n // 128), -(-k // 64)
    cand, s = [1], 2
    while s <= (3 * CUS) // tiles and s <= slabs:
        cand.append(s); s *= 2
    calls = {f"S = {s}": (lambda s=s: bla.gemm_bf16_splitk(A16, B16, Cd, transb=True, stream=st, splits=s)) for s in cand}
    calls["S = 0 (automatic)"] = lambda: bla.gemm_bf16_splitk(A16, B16, Cd, transb=True, stream=st, splits=0)
    res = rounds(calls)
    rows = np.unique(np.r_[0:min(m, 64), max(m - 64, 0):m])
    a64 = bla.from_bf16(A16.numpy()[rows]).astype(np.float64); b64 = bla.from_bf16(B16.numpy()).astype(np.float64)
    fl = 2.0 * m * n * k
    print(f"== product nt {m} x {n} x {k}: {tiles} tiles, {slabs} slabs, {3 * CUS} slots; {fl/1e9:.2f} GFLOP", flush=True)
    for w, call in calls.items():
        Cd.fill_bytes(0xFF); call(); bla.sync()
        ratio = worst_ratio(Cd.numpy()[rows], a64, b64, k)
        t, name = res[w]
        eff, sps, pbytes = bla.gemm_bf16_splitk_plan(m, n, k, int(w.split()[2]), CUS)
        print(line(w, t, f"{fl/np.median(t)/1e9:8.2f} TF/s  S_eff {eff:3d} sps {sps:4d} partials {pbytes/2**20:7.1f} MiB  worst err/bound {ratio:.4f} "
                         f"{'ok' if ratio <= 1 else 'OUTSIDE THE BOUND'}  {name}"), flush=True)
    one, auto = res["S = 1"][0], res["S = 0 (automatic)"][0]
    spread = one.max() - one.min()
    best = min(res, key=lambda w: np.median(res[w][0]))
    gain = np.median(one) - np.median(auto)
    verdict = "faster than S = 1 by more than its spread" if gain > spread else ("within S = 1's spread" if abs(gain) <= spread else "SLOWER than S = 1 beyond its spread")
    print(f"  automatic / S = 1 = {np.median(auto)/np.median(one):.3f} of the time ({np.median(one)/np.median(auto):.2f}x); S = 1 spread {spread*1e3:.1f} us, gain {gain*1e3:.1f} us: "
          f"{verdict}; fastest candidate: {best}", flush=True)
    del A16, B16, Cd


# ---- (c), (d): the weight-gradient entry and the whole backward pass -----------------------------------------------------------------------------------
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
    n8 = r8(Bn * h * w)
    xh = bla.from_bf16(bla.to_bf16(uniform(1, (Bn, c, h, w), dtype=np.float32))); dyh = bla.from_bf16(bla.to_bf16(uniform(3, (Bn, f, h, w), dtype=np.float32)))
    x, dy = bla.to_device(xh), bla.to_device(dyh)
    kern = bla.to_device(uniform(2, (f, c, k, k), dtype=np.float32))
    dx, dk, scratch = bla.empty((Bn, c, h, w)), bla.empty((f, c, k, k)), bla.empty((f * c * k * k,))
    counts = (f * n8, c * k * k * n8)
    src = bla.to_device(uniform(4, (max(counts),), dtype=np.float32))
    Y16, G16 = (bla.empty((cnt,), np.uint16) for cnt in counts)
    for dst, cnt in zip((Y16, G16), counts):
        chk(L.bla_f32_to_bf16(st, src.ptr, cnt, dst.ptr, cnt, 1, cnt))
    bla.sync(); del src
    product = lambda sp: bla.gemm_bf16_splitk(Y16, G16, dk, transb=True, m=f, n=c * k * k, k=n8, lda=n8, ldb=n8, ldc=c * k * k, stream=st, splits=sp)
    calls = {
        "c  weight gradient, backward entry (S = 1)": lambda: bla.conv2d_backward_as_bf16(dy, x, kern, dk, None, Bn, h, w, k, c, f, s, stream=st),
        "c  weight gradient entry, splits = 0": lambda: bla.conv2d_weight_gradient_as_bf16(dy, x, dk, Bn, h, w, k, c, f, s, splits=0, stream=st),
        "c  .. its product alone, S = 1": lambda: product(1),
        "c  .. its product alone, splits = 0": lambda: product(0),
        "d  backward f32": lambda: chk(L.bla_conv2d_backward_batched_f32(st, dy.ptr, x.ptr, kern.ptr, dk.ptr, dx.ptr, scratch.ptr, Bn, h, w, k, c, f, s)),
        "d  backward _as_bf16 (unchanged entry)": lambda: bla.conv2d_backward_as_bf16(dy, x, kern, dk, dx, Bn, h, w, k, c, f, s, stream=st),
        "d  weight gradient entry + data gradient": lambda: (bla.conv2d_weight_gradient_as_bf16(dy, x, dk, Bn, h, w, k, c, f, s, splits=0, stream=st),
                                                             bla.conv2d_backward_as_bf16(dy, None, kern, None, dx, Bn, h, w, k, c, f, s, stream=st)),
    }
    res = rounds(calls)
    eff, sps, pbytes = bla.gemm_bf16_splitk_plan(f, c * k * k, n8, 0, CUS)
    print(f"== conv {c}->{f} @{h}x{w} x{Bn}, k {k}, stride {s}: weight-gradient product {f} x {c*k*k} x {n8}, automatic plan S_eff {eff} sps {sps} partials {pbytes/2**20:.1f} MiB", flush=True)
    fs = [0, 1, f // 2, f - 1]
    ref, mag = wgrad_rows_f64(xh, dyh, fs, k)
    bound = (n8 + 8) * 2.0 ** -23 * mag + 2 * 2.0 ** -24 * np.abs(ref)
    for w_ in ("c  weight gradient, backward entry (S = 1)", "c  weight gradient entry, splits = 0"):
        dk.fill_bytes(0xFF); calls[w_](); bla.sync()
        err = np.abs(dk.numpy()[fs].astype(np.float64) - ref)
        ratio = float(np.max(np.where(np.isnan(err), np.inf, err) / bound))
        print(f"  check {w_[3:]}: worst err/bound {ratio:.4f} on filters {fs} {'ok' if ratio <= 1 else 'OUTSIDE THE BOUND'}", flush=True)
    for w_ in calls:
        t, name = res[w_]
        print(line(w_, t, name if w_[0] == "c" else ""), flush=True)
    med = {w_: float(np.median(res[w_][0])) for w_ in calls}
    we, wp = med["c  weight gradient entry, splits = 0"], med["c  .. its product alone, splits = 0"]
    oe, op = med["c  weight gradient, backward entry (S = 1)"], med["c  .. its product alone, S = 1"]
    print(f"  operand passes = entry - product: {(we-wp)*1e3:.1f} us beside the split product, {(oe-op)*1e3:.1f} us beside the unsplit one", flush=True)
    print(f"  weight gradient: new entry / backward entry = {we/oe:.2f} of the time ({oe/we:.2f}x); product alone {op/wp:.2f}x", flush=True)
    nb, f32b, ob = med["d  weight gradient entry + data gradient"], med["d  backward f32"], med["d  backward _as_bf16 (unchanged entry)"]
    print(f"  whole backward: new composition / f32 = {nb/f32b:.2f} of the fp32 time ({'bf16 wins' if nb < f32b else 'fp32 still wins'} by {abs(f32b-nb)*1e3:.1f} us); "
          f"unchanged _as_bf16 entry / f32 = {ob/f32b:.2f}", flush=True)
    del x, dy, kern, dx, dk, scratch, Y16, G16
