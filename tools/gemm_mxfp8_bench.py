#!/usr/bin/env python3
"""The MXFP8 product (bla_gemm_mxfp8) beside the bf16 product (bla_gemm_bf16, nt), its quantiser, and bla_gemm_f32_as_mxfp8 beside
bla_gemm_f32_as_bf16: HIP events, one process, a pre-roll of 4096^3 fp32 products, medians [min .. max] of alternating rounds
(tools/attention_bf16_bench.py's method).
usage: gemm_mxfp8_bench.py [--sizes 1024,2048,4096,8192] [--rounds 7] [--warm 1.0]
Part 1: bla_gemm_mxfp8 against bla_gemm_bf16 (nt, the same m = n = k, uniform [-1, 1) operands converted on the device) in TFLOP/s.  Part 2: both
quantiser forms at 4096 x 4096 in GB/s (4 bytes read, 1 + 1/32 written per element).  Part 3: bla_gemm_f32_as_mxfp8 against bla_gemm_f32_as_bf16 at
4096^3, nn and nt.  Each claim is a difference of medians against the bf16 side's own min-max spread; the ratio is printed whatever it is.
Before anything is timed at a size, the kernel that will be timed runs the exact case of the tests at that m and n (integer elements, scale bytes
125 .. 129, k = min(k, 1024)) and a sample of rows is compared bit for bit with float64; every timed output is checked finite."""
import argparse, ctypes as C, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from __graft_entry__ import load_pkg
from inputs import uniform

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="1024,2048,4096,8192")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--warm", type=float, default=1.0, help="seconds of 4096^3 fp32 products before the first measurement (0 = cold)")
ap.add_argument("--target-ms", type=float, default=20.0, help="length of one timed window")
a = ap.parse_args()
bla = load_pkg(); bla.init(0); L = bla.lib(); chk = bla.native.check
st = L.bla_default_stream()
e0, e1 = C.c_void_p(), C.c_void_p(); chk(L.bla_event_create(C.byref(e0))); chk(L.bla_event_create(C.byref(e1)))
F32, F64, U8, U16 = np.float32, np.float64, np.uint8, np.uint16
last = lambda: L.bla_gemm_last_kernel().decode()


def timed(call, iters):
    call()
    chk(L.bla_event_record(e0, st))
    for _ in range(iters):
        call()
    chk(L.bla_event_record(e1, st))
    ms = C.c_float(); chk(L.bla_event_elapsed_ms(e0, e1, C.byref(ms)))
    return ms.value / iters


def rounds(calls):
    iters = {n: max(3, int(a.target_ms / max(timed(c, 3), 1e-3))) for n, c in calls.items()}      # the rehearsal sizes the windows
    res = {name: [] for name in calls}
    for _ in range(a.rounds):
        for name, call in calls.items():
            res[name].append(timed(call, iters[name]))
    bla.sync()
    return {n: np.array(v) for n, v in res.items()}


def show(res, work, unit):
    for n, t in res.items():
        r = work / (t * 1e-3)
        print(f"  {n:<40} median {np.median(t) * 1000:10.2f} us [{t.min() * 1000:10.2f} .. {t.max() * 1000:10.2f}]   {work / (np.median(t) * 1e-3):9.2f} {unit} "
              f"[{r.min():9.2f} .. {r.max():9.2f}]", flush=True)


def claim(res, new, old):
    dd, spread = np.median(res[old]) - np.median(res[new]), res[old].max() - res[old].min()
    print(f"  claim: ({old}) - ({new}) = {dd * 1000:.2f} us against ({old})'s own min-max spread of {spread * 1000:.2f} us: "
          f"{'FASTER' if dd > spread else 'NOT faster'} by more than the spread ({np.median(res[old]) / np.median(res[new]):.3f} x)", flush=True)


def exact_check(n):
    """The tests' exact case at m = n, k = min(n, 1024), on the fast kernel; 64 strided rows against float64, bit for bit."""
    k = min(n, 1024)
    rng = np.random.default_rng(n)
    ea, eb = bla.native.e4m3_round(rng.integers(-4, 5, (n, k)).astype(F32)), bla.native.e4m3_round(rng.integers(-4, 5, (n, k)).astype(F32))
    sa, sb = rng.integers(125, 130, (n, k // 32)).astype(U8), rng.integers(125, 130, (n, k // 32)).astype(U8)
    dA, dSA, dB, dSB = (bla.to_device(x, U8) for x in (ea, sa, eb, sb))
    c = bla.empty((n, n)).fill_bytes(0xFF)
    bla.gemm_mxfp8(dA, dSA, dB, dSB, c, stream=st); bla.sync()
    assert last() == "gemm_mxfp8_mfma128x128x128_f32", last()
    rows = (np.arange(64) * 2654435761 + 12345) % n
    ref = bla.from_mxfp8(ea[rows], sa[rows]).astype(F64) @ bla.from_mxfp8(eb, sb).astype(F64).T
    got = c.numpy()[rows]
    assert np.array_equal(got.astype(F64), ref), f"{n}: the exact case differs in {int((got != ref).sum())} elements"
    return k


if a.warm > 0:
    wa = bla.to_device(uniform(1, (4096, 4096), dtype=F32)); wc = bla.empty((4096, 4096))
    t0 = time.time()
    while time.time() - t0 < a.warm:
        for _ in range(20):
            bla.gemm(wa, wa, wc, stream=st)
        bla.sync()
    del wa, wc
    print(f"# warmed up for {a.warm:.1f} s of 4096^3 fp32 products", flush=True)

# ---- part 1: the product -----------------------------------------------------------------------------------------------------------------------------
for n in [int(s) for s in a.sizes.split(",")]:
    kx = exact_check(n)
    rng = np.random.default_rng(1000 + n)
    src_a, src_b = bla.to_device(rng.random((n, n), F32) * 2 - 1), bla.to_device(rng.random((n, n), F32) * 2 - 1)
    a8, b8, sa, sb = bla.empty((n, n), U8), bla.empty((n, n), U8), bla.empty((n, n // 32), U8), bla.empty((n, n // 32), U8)
    bla.f32_to_mxfp8(src_a, a8, sa, n, n, stream=st); bla.f32_to_mxfp8(src_b, b8, sb, n, n, stream=st)
    a16, b16 = bla.empty((n, n), U16), bla.empty((n, n), U16)
    chk(L.bla_f32_to_bf16(st, src_a.ptr, n, a16.ptr, n, n, n)); chk(L.bla_f32_to_bf16(st, src_b.ptr, n, b16.ptr, n, n, n))
    del src_a, src_b
    c8, c16 = bla.empty((n, n)), bla.empty((n, n))
    calls = {"bla_gemm_bf16 nt": lambda: bla.gemm_bf16(a16, b16, c16, transb=True, stream=st),
             "bla_gemm_mxfp8": lambda: bla.gemm_mxfp8(a8, sa, b8, sb, c8, stream=st)}
    calls["bla_gemm_bf16 nt"](); name16 = last(); calls["bla_gemm_mxfp8"](); name8 = last(); bla.sync()
    o8, o16 = c8.numpy(), c16.numpy()
    assert np.isfinite(o8).all() and np.isfinite(o16).all()
    rel = np.linalg.norm(o8.astype(F64) - o16) / np.linalg.norm(o16.astype(F64))
    print(f"== {n}^3: {name8} against {name16}; exact case at k = {kx} bit-equal to float64, outputs finite, MXFP8 result {rel:.2e} normwise from the bf16 one", flush=True)
    res = rounds(calls)
    show(res, 2.0 * n ** 3 / 1e12, "TFLOP/s")
    claim(res, "bla_gemm_mxfp8", "bla_gemm_bf16 nt")
    del a8, b8, sa, sb, a16, b16, c8, c16

# ---- part 2: the quantiser ---------------------------------------------------------------------------------------------------------------------------
n = 4096
src = bla.to_device(np.random.default_rng(5).random((n, n), F32) * 2 - 1)
el, sc = bla.empty((n, n), U8), bla.empty((n, n // 32), U8)
calls = {"bla_f32_to_mxfp8 trans = 0": lambda: bla.f32_to_mxfp8(src, el, sc, n, n, stream=st),
         "bla_f32_to_mxfp8 trans = 1": lambda: bla.f32_to_mxfp8(src, el, sc, n, n, trans=True, stream=st)}
print(f"== the quantiser at {n} x {n} (4 bytes read, 1 + 1/32 written per element)", flush=True)
res = rounds(calls)
show(res, n * n * (5 + 1 / 32) / 1e9, "GB/s")
assert (sc.numpy() != 255).all()

# ---- part 3: from fp32 operands ------------------------------------------------------------------------------------------------------------------------
fa, fb = src, bla.to_device(np.random.default_rng(6).random((n, n), F32) * 2 - 1)
c8, c16 = bla.empty((n, n)), bla.empty((n, n))
for lay in ("nn", "nt"):
    tb = lay[1] == "t"
    calls = {f"bla_gemm_f32_as_bf16 {lay}": lambda: chk(L.bla_gemm_f32_as_bf16(st, 0, int(tb), n, n, n, fa.ptr, n, fb.ptr, n, c16.ptr, n, None)),
             f"bla_gemm_f32_as_mxfp8 {lay}": lambda: bla.gemm_f32_as_mxfp8(fa, fb, c8, transb=tb, stream=st)}
    for call in calls.values():
        call()
    bla.sync()
    o8, o16 = c8.numpy(), c16.numpy()
    assert np.isfinite(o8).all() and np.isfinite(o16).all()
    print(f"== from fp32 operands, {n}^3 {lay}: outputs finite, MXFP8 result {np.linalg.norm(o8.astype(F64) - o16) / np.linalg.norm(o16.astype(F64)):.2e} normwise "
          f"from the bf16 one", flush=True)
    res = rounds(calls)
    show(res, 2.0 * n ** 3 / 1e12, "TFLOP/s")
    claim(res, f"bla_gemm_f32_as_mxfp8 {lay}", f"bla_gemm_f32_as_bf16 {lay}")
