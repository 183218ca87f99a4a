#!/usr/bin/env python3
"""Group norm into a bf16 map, and the bf16 ResNet block, beside what they replace: kernel-level timing (HIP events), one process, medians
[min .. max] of alternating rounds.
usage: resnet_bf16_bench.py [--shapes 128x32x64,256x16x64] [--rounds 7] [--iters 20] [--warm 1.0]        shape = CxHWxB; group size 32, k = 3, tdim = 128
Per shape:
  norm      bla_group_norm_relu_bf16_map (x -> the padded map of a k3 s1 layer) beside bla_group_norm_relu_batched_f32 + bla_conv_bf16_pad, and with dropout
            beside bla_group_norm_relu_batched_f32 + bla_dropout_f32 + bla_conv_bf16_pad (the fp32 family's fused dropout form is not public)
  gradient  bla_group_norm_ddx_bf16_map (-> the data-gradient map, dilate 1; map only, and map + fp32) beside bla_group_norm_ddx_gated_batched_f32 + pad
  block     bla_resnet_{forward,backward}_batched_bf16 C -> C beside bla_resnet_{forward,backward}_batched_f32 on the same inputs, and every step of the bf16
            composition timed on its own (the per-launch breakdown)
Every timed output is checked in the run: the maps against the replaced pair's map (the fp32 family forms the variance in a second pass, so a value may
differ in its last fp32 bit and its rounding by one bf16 ulp: at most 1 ulp anywhere, equal bits on more than 99 %), the bf16 block's result and del_x
against the fp32 block's (normwise, printed).  Operands are uniform random."""
import argparse, ctypes as C, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from __graft_entry__ import load_pkg
from inputs import uniform

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="128x32x64,256x16x64")
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warm", type=float, default=1.0, help="seconds of 4096^3 fp32 products before the first measurement (the clocks ramp for about that long; 0 = cold)")
a = ap.parse_args()
bla = load_pkg(); bla.init(0); L = bla.lib(); N = bla.native; chk = N.check
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
F32, U8, U16 = np.float32, np.uint8, np.uint16
r8 = lambda v: -(-v // 8) * 8


def timed(call):
    call()                                   # one untimed launch in front
    chk(L.bla_event_record(e0, st))
    for _ in range(a.iters):
        call()
    chk(L.bla_event_record(e1, st))
    ms = C.c_float(); chk(L.bla_event_elapsed_ms(e0, e1, C.byref(ms)))
    return ms.value / a.iters


def rounds(calls):
    res = {name: [] for name in calls}
    for r in range(a.rounds + 1):            # round 0 is a rehearsal
        for name, call in calls.items():
            ms = timed(call)
            if r > 0:
                res[name].append(ms * 1e3)
    bla.sync()
    return {n: np.array(v) for n, v in res.items()}


def show(res, names=None):
    for n in names or res:
        t = res[n]
        print(f"  {n:<58} median {np.median(t):8.1f} us  [{t.min():8.1f} .. {t.max():8.1f}]", flush=True)


def claim(res, new, old):
    new, old = (next(k for k in res if k.startswith(p)) for p in (new, old))
    d, spread = np.median(res[old]) - np.median(res[new]), res[old].max() - res[old].min()
    print(f"  ({old.split()[0]}) - ({new.split()[0]}) = {d:.1f} us against ({old.split()[0]})'s own min-max spread of {spread:.1f} us: "
          f"{'FASTER' if d > spread else 'NOT faster'} by more than the spread", flush=True)


def same_map(got, want, what):
    g, w = bla.from_bf16(got.numpy()), bla.from_bf16(want.numpy())
    equal = float((got.numpy() == want.numpy()).mean())
    assert (np.abs(g - w) <= 2.0 ** -7 * np.maximum(np.abs(g), np.abs(w)) + 1e-5).all() and equal > 0.99 and (w != 0).any(), (what, equal)   # (1e-5: a value that cancels to nearly zero)
    return equal


for spec in a.shapes.split(","):
    c, hw_, B = [int(v) for v in spec.split("x")]
    h = w = hw_; k, gs, tdim = 3, 32, 128
    cp, G, hw = r8(c), -(-c // gs), h * w
    n = B * c * hw
    print(f"== {c} channels @{h}x{w} x{B}, group size {gs}: {n * 4 / 1e6:.1f} MB per fp32 tensor; medians of {a.rounds} alternating rounds of {a.iters} launches", flush=True)
    x = bla.to_device(uniform(11, (B, c, h, w), -1.0, 3.0, F32)); src = bla.to_device(uniform(12, (B, c, h, w), -0.5, 1.5, F32))
    drop = bla.to_device((uniform(13, (B, c, h, w), 0.0, 1.0, F32) < 0.3).astype(U8), U8)
    hp, wp, top, left, dil = bla.conv_bf16_layout(h, w, k, 1)
    hq, wq, topq, leftq, dq = bla.conv_bf16_layout(h, w, k, 1, True)
    y, z = bla.empty((B, c, h, w)), bla.empty((B, c, h, w))
    mu, sd, mu2, sd2 = (bla.empty((B, G)) for _ in range(4))
    P_old, P_oldd = bla.empty((B, hp, wp, cp), U16), bla.empty((B, hp, wp, cp), U16)
    P_new, P_newd = bla.zeros((B, hp, wp, cp), U16), bla.zeros((B, hp, wp, cp), U16)
    fmap = lambda arr: bla.conv_bf16_map(arr, hp, wp, cp, top, left, dil)
    qmap = lambda arr: bla.conv_bf16_map(arr, hq, wq, cp, topq, leftq, dq)
    gn_f32 = lambda: chk(L.bla_group_norm_relu_batched_f32(st, B, x.ptr, y.ptr, sd2.ptr, mu2.ptr, c, gs, hw))
    calls = {
        "1  norm + relu (fp32) + pad": lambda: (gn_f32(), bla.conv_bf16_pad(y, P_old, B, c, h, w, hp, wp, top, left, dil, stream=st)),
        "2  norm + relu into the map": lambda: bla.group_norm_relu_bf16_map(x, B, c, gs, h, w, sd, mu, dst=fmap(P_new), stream=st),
        "3  norm + relu (fp32) + dropout + pad": lambda: (gn_f32(), chk(L.bla_dropout_f32(st, y.ptr, z.ptr, drop.ptr, n)),
                                                         bla.conv_bf16_pad(z, P_oldd, B, c, h, w, hp, wp, top, left, dil, stream=st)),
        "4  norm + relu + dropout into the map": lambda: bla.group_norm_relu_bf16_map(x, B, c, gs, h, w, sd, mu, dst=fmap(P_newd), drop=drop, stream=st),
        "5  (2) with the fp32 output too": lambda: bla.group_norm_relu_bf16_map(x, B, c, gs, h, w, sd, mu, dst=fmap(P_new), out_f32=z, stream=st),
    }
    res = rounds(calls)
    eq = [same_map(P_new, P_old, "norm"), same_map(P_newd, P_oldd, "norm + dropout")]
    print(f" norm: maps within one bf16 ulp of the replaced pair's, equal bits on {min(eq) * 100:.2f} %;  bytes per element: (1) 4 + 4 + 4 + 2, (2) 4 + 4 + 2, "
          f"(3) 4 + 4 + 4 + 1 + 4 + 4 + 2, (4) 4 + 4 + 1 + 2 (the second read of x from cache)", flush=True)
    show(res); claim(res, "2  norm", "1  norm"); claim(res, "4  norm", "3  norm")
    # the gradient: source = src, data = x, statistics of x
    Q_old, Q_new, Q_new2 = bla.empty((B, hq, wq, cp), U16), bla.zeros((B, hq, wq, cp), U16), bla.zeros((B, hq, wq, cp), U16)
    calls = {
        "6  norm gradient (fp32) + pad": lambda: (chk(L.bla_group_norm_ddx_gated_batched_f32(st, B, src.ptr, y.ptr, x.ptr, mu.ptr, sd.ptr, c, gs, hw, None, None)),
                                                 bla.conv_bf16_pad(y, Q_old, B, c, h, w, hq, wq, topq, leftq, dq, stream=st)),
        "7  norm gradient into the map": lambda: bla.group_norm_ddx_bf16_map(src, x, mu, sd, B, c, gs, h, w, dst=qmap(Q_new), stream=st),
        "8  norm gradient into the map and fp32": lambda: bla.group_norm_ddx_bf16_map(src, x, mu, sd, B, c, gs, h, w, dst=qmap(Q_new2), dest_f32=z, stream=st),
    }
    res = rounds(calls)
    eq = [same_map(Q_new, Q_old, "gradient"), same_map(Q_new2, Q_old, "gradient + fp32")]
    print(f" gradient: maps within one bf16 ulp of the replaced pair's, equal bits on {min(eq) * 100:.2f} %", flush=True)
    show(res); claim(res, "7  norm", "6  norm"); claim(res, "8  norm", "6  norm")
    del P_old, P_oldd, P_newd, Q_old, Q_new2

    # the block, c -> c
    I = dict(temb=uniform(21, (B, tdim), -1, 1, F32), del_out=uniform(22, (B, c, h, w), -1, 1, F32), conv1=uniform(23, (c, c, k, k), -0.05, 0.05, F32),
             conv2=uniform(24, (c, c, k, k), -0.05, 0.05, F32), time_w=uniform(25, (tdim, c), -0.1, 0.1, F32), time_b=uniform(26, (c,), -0.1, 0.1, F32))
    D = {nm: bla.to_device(v) for nm, v in I.items()}
    params = N.ResnetParams(D["conv1"].ptr, D["conv2"].ptr, D["time_w"].ptr, D["time_b"].ptr, None)
    act = lambda: bla.empty((B, c, h, w))
    T = {nm: act() for nm in ("relu1", "c1", "relu2", "dp", "c2", "result", "g_out_a", "g_out_b", "g_in", "del_x", "result16", "del_x16", "c1_16", "c2_16")}
    S = {nm: bla.empty((B, G)) for nm in ("mu1", "sd1", "mu2", "sd2", "mu1_16", "sd1_16", "mu2_16", "sd2_16")}
    tdense, dtb, flip = bla.empty((B, c)), bla.empty((B, c)), bla.empty((c * c * k * k,))
    gr = {nm: bla.empty(D[nm].shape) for nm in ("conv1", "conv2", "time_w", "time_b")}; gr16 = {nm: bla.empty(D[nm].shape) for nm in gr}
    ws32 = N.ResnetWs(S["mu1"].ptr, S["sd1"].ptr, T["relu1"].ptr, T["c1"].ptr, tdense.ptr, S["mu2"].ptr, S["sd2"].ptr, T["relu2"].ptr, T["dp"].ptr, T["c2"].ptr, None)
    ws16 = N.ResnetWs(S["mu1_16"].ptr, S["sd1_16"].ptr, None, T["c1_16"].ptr, tdense.ptr, S["mu2_16"].ptr, S["sd2_16"].ptr, None, None, T["c2_16"].ptr, None)
    g32 = N.ResnetGrads(*[gr[nm].ptr for nm in ("conv1", "conv2", "time_w", "time_b")], None); g16 = N.ResnetGrads(*[gr16[nm].ptr for nm in ("conv1", "conv2", "time_w", "time_b")], None)
    sc = N.ResnetScratch(T["g_out_a"].ptr, T["g_out_b"].ptr, T["g_in"].ptr, flip.ptr)
    p1, p2, q1 = P_new, bla.zeros((B, hp, wp, cp), U16), Q_new
    maps = bla.resnet_bf16_maps(p1, p2, q1)
    fwd32 = lambda: chk(L.bla_resnet_forward_batched_f32(st, B, x.ptr, D["temb"].ptr, C.byref(params), drop.ptr, C.byref(ws32), T["result"].ptr, h, w, c, c, k, tdim, gs))
    bwd32 = lambda: chk(L.bla_resnet_backward_batched_f32(st, B, D["del_out"].ptr, x.ptr, D["temb"].ptr, C.byref(params), C.byref(ws32), C.byref(g32), C.byref(sc), dtb.ptr,
                                                          T["del_x"].ptr, h, w, c, c, k, tdim, gs))
    fwd16 = lambda: bla.resnet_forward_batched_bf16(x, D["temb"], params, drop, ws16, T["result16"], B, h, w, c, c, k, tdim, gs, maps, stream=st)
    bwd16 = lambda: bla.resnet_backward_batched_bf16(D["del_out"], x, D["temb"], params, ws16, g16, sc, dtb, T["del_x16"], B, h, w, c, c, k, tdim, gs, maps, 0, stream=st)
    fwd32(); bwd32(); fwd16(); bwd16(); bla.sync()                       # eagerly once: the workspace grows here, not inside a timed window
    res = rounds({"9  block forward, fp32": fwd32, "10 block forward, bf16 products": fwd16, "11 block backward, fp32": bwd32, "12 block backward, bf16 products": bwd16})
    nw = lambda g, r: float(np.linalg.norm((g.numpy().astype(np.float64) - r.numpy()).ravel()) / np.linalg.norm(r.numpy().astype(np.float64).ravel()))
    d_res, d_dx, d_k1 = nw(T["result16"], T["result"]), nw(T["del_x16"], T["del_x"]), nw(gr16["conv1"], gr["conv1"])
    assert d_res < 5e-2 and d_dx < 5e-2 and d_k1 < 5e-2, (d_res, d_dx, d_k1)
    fl = 2.0 * c * B * hw * k * k * c
    print(f" block {c} -> {c}: bf16 against fp32 block, normwise: result {d_res:.1e}, del_x {d_dx:.1e}, conv1 gradient {d_k1:.1e};  {fl / 1e9:.2f} GFLOP per product "
          f"(2 forward, 4 backward)", flush=True)
    show(res)
    # the bf16 composition step by step (buffers of the block run above; every step reads what the block left)
    A = bla.empty((c * k * k * cp,), U16); Q2 = bla.empty((B, hq, wq, cp), U16); g_tmp = bla.empty(D["conv1"].shape)
    ep = bla.Epilogue(alpha=1.0, bias_col=D["time_b"].ptr)
    steps = {
        "f1 norm + relu x -> p1": lambda: bla.group_norm_relu_bf16_map(x, B, c, gs, h, w, S["sd1_16"], S["mu1_16"], dst=fmap(p1), stream=st),
        "f2 tdense": lambda: chk(L.bla_gemm_f32(st, 0, 0, B, c, tdim, D["temb"].ptr, tdim, D["time_w"].ptr, c, tdense.ptr, c, C.byref(ep))),
        "f3 prepare_kernels (forward)": lambda: bla.conv_bf16_prepare_kernels(D["conv1"], A, c, c, k, stream=st),
        "f4 gathered product + bias (conv1; conv2 the same)": lambda: bla.conv2d_gathered_bf16(A, c, p1, B, hp, wp, cp, k, 1, h, w, T["c1_16"], tdense, c, stream=st),
        "f5 norm + relu + dropout c1 -> p2": lambda: bla.group_norm_relu_bf16_map(T["c1_16"], B, c, gs, h, w, S["sd2_16"], S["mu2_16"], dst=fmap(p2), drop=drop, stream=st),
        "f6 sum": lambda: chk(L.bla_sum_f32(st, T["result16"].ptr, T["c2_16"].ptr, x.ptr, n)),
        "b1 pad del_out -> Q2": lambda: bla.conv_bf16_pad(D["del_out"], Q2, B, c, h, w, hq, wq, topq, leftq, dq, stream=st),
        "b2 implicit weight gradient (Q2, p2)": lambda: bla.conv2d_weight_gradient_gathered_bf16(Q2, hq, wq, cp, topq, leftq, dq, p2, hp, wp, cp, B, k, 1, h, w, c, c, g_tmp, 0, stream=st),
        "b3 prepare_kernels (data gradient)": lambda: bla.conv_bf16_prepare_kernels(D["conv2"], A, c, c, k, True, stream=st),
        "b4 gated data gradient -> g_out_a": lambda: bla.conv2d_gathered_bf16_chained(A, c, Q2, B, hq, wq, cp, k, 1, h, w, out_f32=T["g_out_a"], gate=fmap(p2), stream=st),
        "b5 norm gradient -> g_out_b, q1": lambda: bla.group_norm_ddx_bf16_map(T["g_out_a"], T["c1_16"], S["mu2_16"], S["sd2_16"], B, c, gs, h, w, dst=qmap(q1), dest_f32=T["g_out_b"], stream=st),
        "b6 channel sums": lambda: chk(L.bla_col_sum_f32(st, T["g_out_b"].ptr, B * c, hw, dtb.ptr, 1)),
        "b7 last norm gradient (fp32, + addend)": lambda: chk(L.bla_group_norm_ddx_gated_batched_f32(st, B, T["g_in"].ptr, T["del_x16"].ptr, x.ptr, S["mu1_16"].ptr, S["sd1_16"].ptr, c, gs, hw,
                                                                                               None, D["del_out"].ptr)),
    }
    bla.conv_bf16_pad(D["del_out"], Q2, B, c, h, w, hq, wq, topq, leftq, dq, stream=st); bla.conv_bf16_prepare_kernels(D["conv1"], A, c, c, k, stream=st); bla.sync()
    sres = rounds(steps)
    print(" the bf16 block step by step (each step alone, 20 launches back to back):", flush=True)
    show(sres)
    m = {nm: float(np.median(v)) for nm, v in sres.items()}
    f_sum = m["f1 norm + relu x -> p1"] + m["f2 tdense"] + 2 * m["f3 prepare_kernels (forward)"] + 2 * m["f4 gathered product + bias (conv1; conv2 the same)"] + \
        m["f5 norm + relu + dropout c1 -> p2"] + m["f6 sum"]
    print(f"  forward steps add up to {f_sum:.1f} us against the entry's {np.median(res['10 block forward, bf16 products']):.1f} us", flush=True)
    del x, src, drop, y, z, D, T, S, gr, gr16, p1, p2, q1, P_new, Q_new, A, Q2, maps
