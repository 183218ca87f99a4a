#!/usr/bin/env python3
"""bench.py -- the driver's benchmark contract.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

A plain run measures the primary workload only: set-up, warm-up, K timed steps, the result line.  --full adds
everything else below (secondary and tertiary workloads, CPU baselines and the correctness checks that ride on them).
--dump-outputs DIR writes what the timed primary path computed in its last step as DIR/<name>.npy (see dump_outputs).

Primary workload (BASELINE.json configs[1], the configuration the metric is quoted on):
square fp32 matrix_multiply, N = 4096, both operands and the output resident in HBM, one
"step" = one C = A @ B through the C-ABI (bla_gemm_f32).  With N > 1 ranks every rank runs
its own replica (a square GEMM has no exchange step: "replicas only") and the
value is the aggregate over ranks.

Secondary workload, measured in the same run and reported under "secondary" in the same JSON line (the second
half of BASELINE.json's metric, "MNIST-NN training samples/sec @1/2/4/8 GPUs"): model/mnist_nn.c's 784-256-128-10
SGD step on the device-resident trainer, 256 samples per GPU (weak scaling; global batch = 256 x N), synthetic
pixels/labels resident in HBM, data parallel with ONE SUM exchange of the flat 235,146-float gradient bucket per
step between backward and the update.  Both forms of the exchange are timed and validated through the C-ABI: the
peer-read kernel over xGMI (bla_dp_*) and RCCL's ncclAllReduce (bla_dp_rccl_*); faults are explicit JSON keys
(secondary.exchange_fallback / exchange_fault), and BLA_BENCH_STRICT=1 turns them into a non-zero exit.

Tertiary workload (N = 1): BASELINE configs[4], the U-Net's 128->128 3x3 convolution at 32x32 on a batch of 64 images,
forward + both gradients, with its own roofline and CPU baseline ("tertiary").

Rank 0 prints ONE JSON line carrying, besides the contract keys, `roofline` (dominant kernel vs the
gfx950 fp32 MFMA peak, timed with HIP events on the launch stream) and, with --full, `cpu_baseline` (the
reference's own loop, lib/matrix.c:47-57, timed on this host on a bounded slice of the same product).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")   # numpy's BLAS pool would spin beside the launch thread; nothing timed here uses it

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

PEAK_FP32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: 256 CU x 2.4 GHz x 256 FLOP/clk/CU


def cpu_baseline_gemm(n, target_seconds=12.0):
    """Times the reference's i-j-k loop on a row slice of the same n x n product, 1 core.
    Uses the reference itself (oracle/_ref/libref.so, kind "reference") when that build is
    present, else this repo's restatement (kind "port")."""
    from inputs import uniform
    import oracle
    import ref
    a = uniform(0xB1A5, (n, n)); b = uniform(0xB1A6, (n, n))          # fp64, the reference's element type
    def run(rows):
        a_slice = np.ascontiguousarray(a[:rows])
        if ref.available():
            t0 = time.perf_counter()
            c = ref.matmul_inplace(a_slice, b)                         # matrix_multiply_inplace, lib/matrix.c:47-57
            return c, time.perf_counter() - t0
        c = np.zeros((rows, n))
        t0 = time.perf_counter()
        oracle.matmul_rows(a_slice, b, c, 0, rows)
        return c, time.perf_counter() - t0

    kind = "reference" if ref.available() else "port"
    if kind == "port":
        oracle.build()
    # calibrate on 2 rows (the loop is cache-hostile: the rate falls ~10x between N=1024 and N=4096), then size
    # the sample to ~target_seconds of CPU work
    _, t2 = run(2)
    rows = int(max(2, min(n, target_seconds / (t2 / 2))))
    rows = max(2, (rows // 2) * 2)
    c, dt = run(rows)
    gflops = 2.0 * rows * n * n / dt / 1e9
    return {"value": round(gflops, 4), "unit": "GFLOP/s", "cores": 1, "kind": kind, "dtype": "f64",
            "sample": f"{rows} of {n} output rows of the same {n}^3 product, gcc -O2, {dt:.1f} s",
            "full_product_seconds_extrapolated": round(2.0 * n ** 3 / (gflops * 1e9), 1)}, c, rows


def cpu_baseline_mnist(batch, target_seconds=8.0):
    """The reference's training step on the same synthetic batch shape, fp64, 1 core: every matrix.h call of model/mnist_nn.c:218-315 in its
    order on the reference's own functions (oracle/_ref/libref.so, kind "reference"); this repo's restatement of the same loop (kind "port")
    only where that build is absent."""
    import oracle
    import ref
    from inputs import randint
    z = np.load(os.path.join(ROOT, "tests", "golden", "mnist_nn_params.npz"))
    params = [z[n].astype(np.float64) for n in ["w1", "b1", "w2", "b2", "w3", "b3"]]
    x_raw = randint(7, (784, batch), 256).astype(np.float64)
    lab = randint(8, (batch,), 10); y = np.zeros((10, batch)); y[lab, np.arange(batch)] = 1
    kind = "reference" if ref.available() else "port"
    if kind == "port":
        oracle.build()
    t0 = time.perf_counter(); steps = 0
    while True:
        if kind == "reference":
            params, _, _ = ref.mnist_step(params, x_raw, y, True)
        else:
            params, _, _ = oracle.mnist_step(params, x_raw, y, colsum_intended=True)
        steps += 1
        if time.perf_counter() - t0 > target_seconds:
            break
    dt = time.perf_counter() - t0
    what = "the reference's matrix.h functions called in the order of model/mnist_nn.c:218-315" if kind == "reference" else "model/mnist_nn.c:218-315 restated"
    return {"value": round(steps * batch / dt, 1), "unit": "samples/s", "cores": 1, "kind": kind, "dtype": "f64",
            "sample": f"{steps} SGD steps at batch {batch} ({what}), gcc -O2, {dt:.1f} s"}


FLOP_PER_SAMPLE = 1007104   # GEMMs only, fwd 469,504 + bwd 537,600
PARAM_NAMES = ["w1", "b1", "w2", "b2", "w3", "b3"]


def run_mnist(bla, dist, world, rank, stream, steps, warmup, barrier, per_gpu_batch=256):
    """samples/s of the data-parallel MNIST-NN step; returns the "secondary" object (rank 0) or None.

    N > 1: two exchange legs are timed on the same K steps from the same start -- the hand-written peer-read kernel (bla_dp_*, one launch,
    update fused) and the library collective (bla_dp_rccl_*: ncclAllReduce SUM through the C-ABI) -- and each is validated (finite, status
    word clean, parameters bit-identical on every rank, the two legs equal to 1e-5 normwise).  `value` is the direct leg's when it is
    healthy; otherwise the RCCL leg's, and then `exchange_fallback` is true and `exchange_fault` says what happened (nothing is hidden in
    free text).  BLA_BENCH_EXCHANGE=direct|rccl times one leg only; BLA_BENCH_STRICT=1 makes any fault a non-zero exit."""
    from inputs import randint
    mn = bla.mnist_nn
    L = bla.lib()
    z = np.load(os.path.join(ROOT, "tests", "golden", "mnist_nn_params.npz"))
    start = [z[n] for n in PARAM_NAMES]                # the reference's trained weights (identical on all ranks)
    nn = mn.MnistNN(per_gpu_batch, colsum_mode=mn.COLSUM_INTENDED)
    nn.set_params(start)
    gB = per_gpu_batch * world
    x_raw = randint(7, (784, gB), 256).astype(np.float32)
    lab = randint(8, (gB,), 10); y = np.zeros((10, gB), np.float32); y[lab, np.arange(gB)] = 1
    lo, hi = mn.shard_columns(gB, world, rank)
    nn.load_batch(np.ascontiguousarray(x_raw[:, lo:hi]), np.ascontiguousarray(y[:, lo:hi]))
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    bla.native.check(L.bla_event_create(C.byref(ev0))); bla.native.check(L.bla_event_create(C.byref(ev1)))

    def measure(step):
        """W untimed + K timed steps from the common start; returns (wall seconds max over ranks, device ms per step, parameters)."""
        nn.set_params(start)
        for _ in range(warmup):
            step()
        barrier()
        t0 = time.perf_counter()
        bla.native.check(L.bla_event_record(ev0, stream))
        for _ in range(steps):
            step()
        bla.native.check(L.bla_event_record(ev1, stream))
        barrier()
        wall = time.perf_counter() - t0
        ms = C.c_float(); bla.native.check(L.bla_event_elapsed_ms(ev0, ev1, C.byref(ms)))
        if dist is not None:
            import torch
            t = torch.tensor([wall], device="cuda", dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            wall = float(t.item())
        return wall, ms.value / steps, mn.flatten_params(nn.get_params())

    def leg_result(name, wall, dev_ms):
        sps = steps * gB / wall
        return {"exchange": name, "value": round(sps, 1), "ms_per_step": round(wall / steps * 1e3, 4), "device_ms_per_step": round(dev_ms, 4)}

    legs, fault, detail = {}, None, {}
    if dist is None:
        # one GPU: the fused-update step either replayed as a graph or issued directly (six launches per host call); which is faster
        # depends on the host's launch rate, so both are tried on 100 untimed steps and the faster one is timed
        modes = {"graph replay": lambda: nn.graph_step(stream=stream, with_update=True), "direct launches": lambda: nn.fused_step(stream=stream)}
        trial = {}
        for name, fn in modes.items():
            for _ in range(20):
                fn()
            barrier(); t_0 = time.perf_counter()
            for _ in range(100):
                fn()
            barrier(); trial[name] = time.perf_counter() - t_0
        launch_mode = min(trial, key=trial.get)
        print("[bench] MNIST-NN launch-mode trial: " + ", ".join(f"{k} {v * 1e4:.1f} us/step" for k, v in trial.items()), file=sys.stderr, flush=True)
        wall, dev_ms, p = measure(modes[launch_mode])
        assert np.isfinite(p).all()
        legs["none"] = leg_result("none (one GPU; fused-update step issued as " + launch_mode + ")", wall, dev_ms)
        chosen = "none"
        # The reference's step also builds the batch (:204-217) and keeps loss / accuracy (:237-257).  With the dataset resident in HBM both run on
        # the device (bla_mnist_nn_gather_batch, bla_mnist_nn_metrics_*): the same K steps again, each on a different batch of a 16,384-row
        # synthetic dataset, metrics accumulating in the output layer's launch -- reported beside the kernel loop above, not instead of it.
        try:
            rows = 64 * per_gpu_batch
            dsx = randint(11, (784, rows), 256).astype(np.float32); dsl = randint(12, (rows,), 10).astype(np.float32)
            d_X, d_lab = bla.to_device(dsx), bla.to_device(dsl)
            order = bla.DeviceArray((rows,), np.int32).copy_from(randint(13, (rows,), rows).astype(np.int32))
            bla.native.check(L.bla_mnist_nn_metrics_enable(nn.h, 1))
            counter = [0]

            def full_step():
                j = counter[0] % 64; counter[0] += 1
                bla.native.check(L.bla_mnist_nn_gather_batch(nn.h, stream, d_X.ptr, d_lab.ptr, rows, order.ptr + 4 * j * per_gpu_batch))
                nn.fused_step(stream=stream)
            fwall, fdev, fp = measure(full_step)
            loss, corr = C.c_double(), C.c_longlong()
            bla.native.check(L.bla_mnist_nn_metrics_read(nn.h, C.byref(loss), C.byref(corr), 1))
            bla.native.check(L.bla_mnist_nn_metrics_enable(nn.h, 0))
            assert np.isfinite(fp).all() and np.isfinite(loss.value)
            detail["with_batch_gather_and_metrics"] = {"value": round(steps * gB / fwall, 1), "unit": "samples/s", "ms_per_step": round(fwall / steps * 1e3, 4),
                                                       "what": "gather of a fresh batch from a dataset resident in HBM + fused step + loss / accuracy on the device, per step",
                                                       "mean_loss": round(loss.value / ((steps + warmup) * gB), 5)}
        except Exception as e:
            detail["with_batch_gather_and_metrics"] = {"error": repr(e)}
    else:
        import torch
        which = os.environ.get("BLA_BENCH_EXCHANGE", "both")     # direct | rccl | both

        def all_agree(flag):   # every rank must take the same path
            t = torch.tensor([1 if flag else 0], device="cuda", dtype=torch.int32)
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            return int(t.item()) == 1

        def digests(p):
            d = torch.tensor([float(np.frombuffer(p.tobytes(), np.uint32).astype(np.uint64).sum() % (1 << 40))], device="cuda", dtype=torch.float64)
            lo_, hi_ = d.clone(), d.clone()
            dist.all_reduce(lo_, op=dist.ReduceOp.MIN); dist.all_reduce(hi_, op=dist.ReduceOp.MAX)
            return float(lo_.item()), float(hi_.item())

        params = {}
        # ---- leg 1: csrc/bla_dp.hip -- every rank reads its peers' gradient buckets directly over xGMI, one launch, update fused
        if which in ("direct", "both"):
            ex, stage, err = None, "create", ""
            try:
                ex = mn.Exchange(rank, world, nn.count)          # local: fine-grained buckets + uncached flag words
            except Exception as e:
                err = str(e)
            if all_agree(ex is not None):
                stage = "map"
                handles = [None] * world
                dist.all_gather_object(handles, ex.export())     # 256 bytes per rank, once
                try:
                    ex.connect(handles)                          # local: map the peers' buffers (IPC)
                    mapped = True
                except Exception as e:
                    err, mapped = str(e), False
                if not all_agree(mapped):
                    fault = {"stage": stage, "error": err or "a peer could not map this rank's buffers"}
            else:
                fault = {"stage": stage, "error": err or "a peer could not allocate its exchange buffers"}
            if fault is None:
                algo = os.environ.get("BLA_DP_ALGO") or ("twoshot" if world >= 4 else "oneshot")
                dp_graph = [True]

                def step():
                    nn.dp_step(ex, stream=stream, graph=dp_graph[0])
                step(); step()    # a peer that never shows up costs one 4 s in-kernel time-out here, not inside the timed region
                if not all_agree(ex.status() == 0):
                    fault = {"stage": "first steps", "status": ex.status(), "error": "a wait for a peer's flag timed out (4 s)"}
            if fault is None:
                # graph replay or direct launches: both tried on 60 untimed steps; every rank takes the choice that is faster for the slowest rank
                trial = []
                for g in (True, False):
                    dp_graph[0] = g
                    for _ in range(10):
                        step()
                    barrier(); t_0 = time.perf_counter()
                    for _ in range(60):
                        step()
                    barrier()
                    t = torch.tensor([time.perf_counter() - t_0], device="cuda", dtype=torch.float64)
                    dist.all_reduce(t, op=dist.ReduceOp.MAX)
                    trial.append(float(t.item()))
                dp_graph[0] = trial[0] <= trial[1]
                wall, dev_ms, p = measure(step)
                lo_, hi_ = digests(p)
                status = ex.status()
                if os.environ.get("BLA_BENCH_REHEARSE_FAULT") == "1":   # rehearsal of the fault path below
                    status = 1
                if not all_agree(bool(np.isfinite(p).all()) and status == 0 and lo_ == hi_):
                    fault = {"stage": "timed steps", "status": status, "digest_lo": lo_, "digest_hi": hi_, "finite": bool(np.isfinite(p).all()),
                             "error": "status word raised, non-finite parameters or ranks diverged"}
                else:
                    params["direct"] = p
                    legs["direct"] = leg_result("one-kernel SUM all-reduce + SGD update (" + algo + "): every rank reads its peers' 235146-float gradient buckets "
                                                + ("slice-wise (reduce-scatter, then the reduced slices) " if algo == "twoshot" else "")
                                                + "directly over xGMI (IPC-mapped fine-grained memory, flag-synchronised); step issued as "
                                                + ("one graph launch" if dp_graph[0] else "direct launches"), wall, dev_ms)
            if fault is not None:
                print(f"[bench] rank {rank}: direct exchange FAULT {fault}", file=sys.stderr, flush=True)
            if ex is not None:
                ex.close()
        # ---- leg 2: the library collective through the C-ABI (bla_dp_rccl_*: ncclAllReduce, ncclFloat, ncclSum)
        if which in ("rccl", "both") or fault is not None:
            def bcast(raw):
                box = [raw]
                dist.broadcast_object_list(box, src=0)
                return box[0]
            comm, err = None, ""
            try:
                comm = mn.RcclComm(rank, world, bcast)
            except Exception as e:       # e.g. ranks sharing one device in a rehearsal: RCCL refuses duplicate devices
                err = str(e)
            if all_agree(comm is not None):
                wall, dev_ms, p = measure(lambda: nn.dp_step_rccl(comm, stream=stream))
                lo_, hi_ = digests(p)
                if all_agree(bool(np.isfinite(p).all()) and lo_ == hi_):      # every rank takes the same branch, as on the direct leg
                    params["rccl"] = p
                    legs["rccl"] = leg_result("RCCL ncclAllReduce(SUM) of the flat 235146-float gradient bucket per step, through the C-ABI (bla_mnist_nn_dp_step_rccl)", wall, dev_ms)
                else:
                    detail["rccl_fault"] = {"stage": "timed steps", "digest_lo": lo_, "digest_hi": hi_, "finite": bool(np.isfinite(p).all())}
            else:
                detail["rccl_fault"] = {"stage": "communicator", "error": err or "a peer could not create its communicator"}
            if comm is not None:
                comm.close()
        if "direct" in params and "rccl" in params:     # same start, same data, same number of steps: the two exchanges must agree
            d = float(np.linalg.norm(params["direct"] - params["rccl"]) / np.linalg.norm(params["rccl"]))
            detail["direct_vs_rccl_rel_diff"] = float(f"{d:.3e}")
            if d > 1e-5:
                fault = {"stage": "cross-check", "error": f"direct and RCCL legs differ by {d:.3e} (normwise)"}
                legs.pop("direct")
        chosen = "direct" if "direct" in legs else "rccl"
        if chosen not in legs:     # neither exchange produced a valid measurement: say so instead of inventing a number
            if rank != 0:
                return None, fault or detail.get("rccl_fault")
            return {"metric": "MNIST-NN training samples/sec", "value": None, "unit": "samples/s", "n_gpus": world, "exchange_fallback": True,
                    "exchange_fault": fault, **detail}, fault or detail.get("rccl_fault")
    # A fault of the RCCL leg alone is a fault too (BLA_BENCH_STRICT=1 exits non-zero on it), with one exception: the one-GPU rehearsal
    # (BLA_BENCH_SHARE_GPU=1), where RCCL refuses a communicator over duplicate devices by design.
    rf = detail.get("rccl_fault")
    if fault is None and rf is not None and not (os.environ.get("BLA_BENCH_SHARE_GPU") == "1" and rf.get("stage") == "communicator"):
        fault = {"stage": "rccl leg: " + str(rf.get("stage")), **{k: v for k, v in rf.items() if k != "stage"}}
    if rank != 0:
        return None, fault
    best = legs[chosen]
    sec = {"metric": "MNIST-NN training samples/sec", "value": best["value"], "unit": "samples/s", "n_gpus": world,
           "steps": steps, "warmup": warmup, "ms_per_step": best["ms_per_step"], "scaling": "weak",
           "config": {"workload": "model/mnist_nn.c 784-256-128-10 SGD step, device-resident trainer", "per_gpu_batch": per_gpu_batch,
                      "global_batch": gB, "parallelism": f"dp{world}", "exchange": best["exchange"]},
           "gemm_flop_rate_tflops": round(best["value"] * FLOP_PER_SAMPLE / 1e12, 3)}
    # formal roofline of the step: GEMM FLOPs per GPU per step over the device-side step time (HIP events on the launch stream).
    # AI ~ 60 FLOP/B > the ridge, so the bound is MFMA -- but 0.258 GFLOP is ~2 us of MFMA time: the step is launch/latency-bound.
    ach = per_gpu_batch * FLOP_PER_SAMPLE / (best["device_ms_per_step"] * 1e-3) / 1e12
    sec["roofline"] = {"bound": "mfma", "achieved": round(ach, 3), "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s",
                       "frac": round(ach / PEAK_FP32_MFMA_TFLOPS, 4), "traffic": None, "kernel_ms": best["device_ms_per_step"],
                       "algorithmic_flops_per_launch": per_gpu_batch * FLOP_PER_SAMPLE,
                       "note": "whole step (6-7 dependent launches), per GPU; latency-bound, see profiles/r02_mnist_*"}
    if world == 1 and per_gpu_batch == 256:
        sec["roofline"]["traffic"], src = committed_traffic("mnist")
        if src:
            sec["roofline"]["traffic_source"] = src
    if world > 1:
        sec["exchange_fallback"] = chosen != "direct" and os.environ.get("BLA_BENCH_EXCHANGE", "both") != "rccl"
        sec["exchange_fault"] = fault if (fault is None or not str(fault.get("stage", "")).startswith("rccl leg")) else None
        sec["legs"] = legs
    sec.update(detail)
    return sec, fault


def committed_traffic(target):
    """HBM-side traffic per iteration of a secondary / tertiary workload from the committed rocprofv3 --pmc summary of the same workload
    (profiles/r02/<target>.summary.json: separate FETCH_SIZE / WRITE_SIZE passes, gfx950-corrected; it cannot be collected from inside this process)."""
    for rnd in ("r03", "r02"):          # the newest committed summary of this workload
        try:
            d = json.load(open(os.path.join(ROOT, "profiles", rnd, target + ".summary.json")))
            return int(d["iteration"]["traffic_bytes"]), f"profiles/{rnd}/{target}.summary.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes)"
        except (OSError, KeyError, ValueError):
            continue
    return None, None


def run_conv(bla, stream, barrier, steps=20, warmup=5):
    """Tertiary workload, BASELINE configs[4] (SURVEY 8(d) cfg 5): the U-Net's headline convolution 128->128, k3, s1 at 32x32 on a batch of
    64 images, forward + both gradients (implicit-GEMM path, nothing materialised).  FLOPs = 3 x 2*M*K*N x 64 with (M,K,N) = (1024,1152,128)."""
    L = bla.lib(); chk = bla.native.check
    from inputs import uniform
    B, h, cin, cout, k = 64, 32, 128, 128, 3
    hw, kkc = h * h, k * k * cin
    x = bla.to_device(uniform(31, (B, cin, h, h), -1, 1, np.float32))
    kern = bla.to_device(uniform(32, (cout, cin, k, k), -0.1, 0.1, np.float32))
    dy = bla.to_device(uniform(33, (B, cout, h, h), -1, 1, np.float32))
    out, dk, dx, scr = bla.empty((B, cout, h, h)), bla.empty((cout, cin, k, k)), bla.empty((B, cin, h, h)), bla.empty((cout * kkc,))

    def fwd():
        chk(L.bla_conv2d_forward_batched_f32(stream, x.ptr, kern.ptr, out.ptr, B, h, h, k, cin, cout, 1))

    def bwd():
        chk(L.bla_conv2d_backward_batched_f32(stream, dy.ptr, x.ptr, kern.ptr, dk.ptr, dx.ptr, scr.ptr, B, h, h, k, cin, cout, 1))
    ev = [C.c_void_p() for _ in range(3)]
    for e in ev:
        chk(L.bla_event_create(C.byref(e)))
    for _ in range(warmup):
        fwd(); bwd()
    barrier()
    t0 = time.perf_counter()
    t_f = t_b = 0.0
    for _ in range(steps):        # events around each half so that forward and backward get their own fraction
        chk(L.bla_event_record(ev[0], stream)); fwd(); chk(L.bla_event_record(ev[1], stream)); bwd(); chk(L.bla_event_record(ev[2], stream))
        ms = C.c_float()
        chk(L.bla_event_elapsed_ms(ev[0], ev[1], C.byref(ms))); t_f += ms.value
        chk(L.bla_event_elapsed_ms(ev[1], ev[2], C.byref(ms))); t_b += ms.value
    barrier()
    wall = time.perf_counter() - t0
    fl = 2.0 * hw * kkc * cout * B
    f_ms, b_ms = t_f / steps, t_b / steps
    tf_f, tf_b = fl / (f_ms * 1e-3) / 1e12, 2 * fl / (b_ms * 1e-3) / 1e12
    tf_all = 3 * fl / ((f_ms + b_ms) * 1e-3) / 1e12
    res = {"metric": "conv 128->128 k3 s1 @32x32 x64 images, forward + both gradients", "value": round(steps * B / wall, 1), "unit": "images/s",
           "steps": steps, "warmup": warmup, "ms_per_step": round(wall / steps * 1e3, 4),
           "config": {"workload": "model/cifar_unet.c conv path (lib/conv.c:205-229) on a batch of 64 CIFAR-shaped feature maps, implicit GEMM",
                      "gemm": "(M,K,N) = (1024,1152,128) per image, 3 products"},
           "roofline": {"bound": "mfma", "achieved": round(tf_all, 2), "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s",
                        "frac": round(tf_all / PEAK_FP32_MFMA_TFLOPS, 4), "traffic": None, "kernel_ms": round(f_ms + b_ms, 4),
                        "algorithmic_flops_per_launch": 3 * fl, "forward_ms": round(f_ms, 4), "forward_frac": round(tf_f / PEAK_FP32_MFMA_TFLOPS, 4),
                        "backward_ms": round(b_ms, 4), "backward_frac": round(tf_b / PEAK_FP32_MFMA_TFLOPS, 4)}}
    res["roofline"]["traffic"], src = committed_traffic("conv128")
    if src:
        res["roofline"]["traffic_source"] = src
    return res, (x, kern, dy, out, dk, dx)


def run_unet(bla, stream, barrier, steps=5, warmup=2, batch=64):
    """The whole conv path of BASELINE configs[4] at model level: the reference's U-Net at its own constants (model/cifar_unet.c:26-37: 32x32x3,
    widths 128/256/256/256, time embedding 512, key dimension 16, groups of 32; 23.9 M parameters) on a batch of CIFAR-shaped images,
    forward() + backward() (:1099-1166, :1351-1436) device-resident (bla_unet_create_batched).  The fraction prices the convolution FLOPs of the
    pass (2 MACs forward, twice that backward) against the fp32 MFMA peak; norms, attention and glue ride in the same time."""
    L = bla.lib(); chk = bla.native.check
    from inputs import uniform

    class Cfg(C.Structure):
        _fields_ = [("image_h", C.c_int), ("image_w", C.c_int), ("in_channels", C.c_int), ("dims", C.c_int * 4), ("time_dim", C.c_int), ("kernel", C.c_int),
                    ("group_size", C.c_int), ("key_dim", C.c_int)]
    from unet_refconst import CFG, make_params, make_inputs          # the seeded parameters / inputs the committed fp64 prediction belongs to
    D, k2, c0, hw = CFG["dims"], CFG["kernel"] ** 2, CFG["in_channels"], [1024, 256, 64, 16]
    cfg = Cfg(CFG["image_h"], CFG["image_w"], c0, (C.c_int * 4)(*D), CFG["time_dim"], CFG["kernel"], CFG["group_size"], CFG["key_dim"])
    h = C.c_void_p()
    chk(L.bla_unet_create_batched(C.byref(h), C.byref(cfg), batch))
    total = L.bla_unet_param_count(h)
    flat = np.zeros(total, np.float32)
    P = make_params(CFG)                                  # every tensor uniform in +-sqrt(3 / fan-in) (biases +-0.05): activations stay in range
    for i in range(L.bla_unet_tensor_count(h)):
        off, cnt = C.c_size_t(), C.c_size_t(); name = C.create_string_buffer(96)
        chk(L.bla_unet_tensor_info(h, i, C.byref(off), C.byref(cnt), name, 96))
        flat[off.value:off.value + cnt.value] = P[name.value.decode()].ravel()
    chk(L.bla_memcpy_h2d(L.bla_unet_params(h), flat.ctypes.data, flat.nbytes, None)); bla.sync()
    ins = [make_inputs(b) for b in range(batch)]
    x = bla.to_device(np.stack([i[0] for i in ins])); temb = bla.to_device(np.stack([i[1] for i in ins])); noise = bla.to_device(np.stack([i[2] for i in ins]))
    res = [(c0, D[0], 0), (D[0], D[0], 0), (D[1], D[1], 1), (D[1], D[1], 1), (D[2], D[2], 2), (D[2], D[2], 2)] + [(D[3], D[3], 3)] * 4 + \
          [(2 * D[3], D[3], 3), (D[3], D[3], 3), (2 * D[2], D[2], 2), (D[2], D[2], 2), (2 * D[1], D[1], 1), (D[1], D[1], 1), (2 * D[0], D[0], 0), (D[0], D[0], 0)]
    fl = sum(2 * hw[l] * co * (ci * k2 + co * k2 + (ci if ci != co else 0)) for ci, co, l in res)
    fl += 2 * k2 * (hw[1] * D[0] * D[1] + hw[2] * D[1] * D[2] + hw[3] * D[2] * D[3]) + 2 * k2 * hw[0] * D[1] * D[0] + 2 * k2 * hw[0] * D[0] * c0
    ev = [C.c_void_p() for _ in range(3)]
    for e in ev:
        chk(L.bla_event_create(C.byref(e)))
    for _ in range(warmup):
        chk(L.bla_unet_forward_f32(h, stream, x.ptr, temb.ptr, None)); chk(L.bla_unet_backward_f32(h, stream, noise.ptr))
    barrier()
    t0 = time.perf_counter(); t_f = t_b = 0.0
    for _ in range(steps):
        chk(L.bla_event_record(ev[0], stream)); chk(L.bla_unet_forward_f32(h, stream, x.ptr, temb.ptr, None)); chk(L.bla_event_record(ev[1], stream))
        chk(L.bla_unet_backward_f32(h, stream, noise.ptr)); chk(L.bla_event_record(ev[2], stream))
        ms = C.c_float()
        chk(L.bla_event_elapsed_ms(ev[0], ev[1], C.byref(ms))); t_f += ms.value
        chk(L.bla_event_elapsed_ms(ev[1], ev[2], C.byref(ms))); t_b += ms.value
    barrier()
    wall = time.perf_counter() - t0
    out = np.empty((batch, c0, 32, 32), np.float32)
    chk(L.bla_memcpy_d2h(out.ctypes.data, L.bla_unet_output(h), out.nbytes, None)); bla.sync()
    chk(L.bla_unet_destroy(h))
    f_ms, b_ms = t_f / steps, t_b / steps
    tf = 3 * fl * batch / ((f_ms + b_ms) * 1e-3) / 1e12
    return {"metric": "U-Net (model/cifar_unet.c constants) forward + backward, batch of CIFAR-shaped images", "value": round(steps * batch / wall, 1), "unit": "images/s",
            "batch": batch, "steps": steps, "warmup": warmup, "parameters": int(total), "forward_ms": round(f_ms, 3), "backward_ms": round(b_ms, 3),
            "finite_output": bool(np.isfinite(out).all()), **unet_prediction_check(out[0]),
            "roofline": {"bound": "mfma", "achieved": round(tf, 2), "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": round(tf / PEAK_FP32_MFMA_TFLOPS, 4),
                         "algorithmic_flops_per_launch": 3 * fl * batch, "note": "convolution FLOPs only (2 MACs forward, twice that backward) over the whole pass"},
            "cpu_baseline": {"value": round(1 / 29.3, 4), "unit": "images/s", "cores": 1, "kind": "reference",
                             "sample": "the reference program `cifar_unet train 1`, one image forward + backward: 29.3 s on one core of the build container (BASELINE.md section 2; not re-timed here)"}}


def unet_prediction_check(pred0):
    """Image 0's prediction of the timed batch against the fp64 oracle composition of the same network on the same parameters and inputs
    (tests/golden/unet_refconst.npz, written by tools/unet_conditioning.py; the -m gpu test test_reference_constants_against_the_oracle re-derives
    it).  The reference's own loops evaluated in fp32 sit `reference_fp32_distance` from that fp64 result (group norm divides by the variance,
    SURVEY Q3): the device must be inside that neighbourhood."""
    fx = np.load(os.path.join(ROOT, "tests", "golden", "unet_refconst.npz"))
    want = fx["prediction"]
    err = float(np.linalg.norm(pred0.astype(np.float64) - want) / np.linalg.norm(want))
    ref32 = float(fx["prediction_fp32_distance"])
    assert err <= 2 * ref32, f"batch-64 U-Net, image 0: prediction {err:.3e} from the fp64 oracle (the reference's loops in fp32: {ref32:.3e})"
    return {"prediction_rel_err_vs_oracle_image0": float(f"{err:.3e}"), "reference_fp32_distance": float(f"{ref32:.3e}")}


def cpu_baseline_conv(arrays, target_seconds=6.0):
    """conv() + conv_ddx() of single images of the same shape, fp64, 1 core: the reference's own stages (_im2col, _reshape_kernels_matrix,
    matrix_multiply_inplace, the channel reshapes, matrix_transpose, _col2im: lib/conv.c:205-229) called in the intended order on
    oracle/_ref/libref.so (kind "reference"); this repo's restatement (kind "port") only where that build is absent.  The first image doubles
    as a correctness check of the batched kernels."""
    import oracle
    import ref
    kind = "reference" if ref.available() else "port"
    if kind == "port":
        oracle.build()
    x, kern, dy, out, dk, dx = arrays
    hx, hk, hdy = x.numpy().astype(np.float64), kern.numpy().astype(np.float64), dy.numpy().astype(np.float64)
    t0 = time.perf_counter(); n = 0; err = None
    while True:
        if kind == "reference":
            w_out, _, w_dx = ref.conv_fwd_bwd(hx[n], hk, hdy[n])
        else:
            fw = oracle.conv_intended(hx[n], hk, 1)
            w_out, w_dx = fw["output"], oracle.conv_ddx_intended(hdy[n], fw["im2col"], fw["kmat"], hx.shape[1], hk.shape[2])["del_x"]
        if n == 0:
            got = out.numpy()[0].astype(np.float64)
            err = float(np.linalg.norm(got - w_out) / np.linalg.norm(w_out))
            gdx = dx.numpy()[0].astype(np.float64)
            err = max(err, float(np.linalg.norm(gdx - w_dx) / np.linalg.norm(w_dx)))
        n += 1
        if time.perf_counter() - t0 > target_seconds or n >= hx.shape[0]:
            break
    dt = time.perf_counter() - t0
    what = "the reference's lib/conv.c stages in the intended order" if kind == "reference" else "lib/conv.c:205-229 restated"
    return {"value": round(n / dt, 3), "unit": "images/s", "cores": 1, "kind": kind, "dtype": "f64",
            "sample": f"{n} images, conv() + conv_ddx() each ({what}), gcc -O2, {dt:.1f} s"}, err


DUMP_MAX_ELEMS = 8 << 20     # 32 MiB of float32 per dumped array


def dump_outputs(out_dir, c, stream):
    """What a caller of the timed path receives: C = A @ B of the last timed step (every step computes the same product of the
    same seeded operands).  A product above DUMP_MAX_ELEMS elements is written as a fixed sample of whole rows: the rows
    np.random.default_rng(0) draws without replacement, ascending -- the same rows in every run of the same --size."""
    os.makedirs(out_dir, exist_ok=True)
    full = c.numpy(stream)
    n_rows, n_cols = full.shape
    if full.size > DUMP_MAX_ELEMS:
        rows = np.sort(np.random.default_rng(0).choice(n_rows, size=DUMP_MAX_ELEMS // n_cols, replace=False))
        full = full[rows]
    np.save(os.path.join(out_dir, "gemm_c.npy"), np.ascontiguousarray(full, dtype=np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=50)   # ~50 ms of launches: with 10 the clocks are still ramping inside the timed region (140 vs 143 TFLOP/s)
    ap.add_argument("--size", type=int, default=4096, help="square GEMM size (BASELINE configs[1]: 1024..8192)")
    ap.add_argument("--full", action="store_true", help="also run the secondary and tertiary workloads and the CPU baselines (off: the primary workload only)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the timed primary path computed in its last step to DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--preroll", type=float, default=0.15, help="seconds of untimed launches of the same product before the warm-up steps (clock ramp; 0 = off)")
    ap.add_argument("--mnist-steps", type=int, default=300, help="with --full: timed steps of the secondary MNIST-NN workload (0 = skip)")
    ap.add_argument("--mnist-warmup", type=int, default=30)
    ap.add_argument("--unet-steps", type=int, default=5, help="with --full: timed forward+backward passes of the batch-64 U-Net under the tertiary workload (0 = skip; N = 1 only)")
    ap.add_argument("--conv-steps", type=int, default=20, help="with --full: timed forward+backward passes of the tertiary batched-convolution workload (0 = skip; N = 1 only)")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            sys.exit("bench.py --gpus N>1 must be launched with torch.distributed.run (one rank per GPU)")
    dist = None
    tstream = None
    share_gpu = os.environ.get("BLA_BENCH_SHARE_GPU") == "1"    # rehearsal of the N > 1 code path on a one-GPU box
    device = 0 if share_gpu else local_rank
    if world > 1:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(device)
        backend = os.environ.get("BLA_BENCH_BACKEND", "nccl")    # "nccl" is RCCL on ROCm; "gloo" only for the rehearsal above
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", device))
        else:
            dist.init_process_group(backend)
        # Every launch of ours and every collective goes through ONE explicit torch stream: RCCL orders a collective against
        # the *current* torch stream, and our library treats a NULL stream handle as "use the library's own stream".
        tstream = torch.cuda.Stream()
        torch.cuda.set_stream(tstream)

    from __graft_entry__ import load_pkg
    bla = load_pkg()
    bla.init(device)
    L = bla.lib()
    from inputs import uniform

    n = args.size
    a = uniform(0xB1A5, (n, n), dtype=np.float32)
    b = uniform(0xB1A6, (n, n), dtype=np.float32)
    da, db, dc = bla.to_device(a), bla.to_device(b), bla.empty((n, n))
    stream = L.bla_default_stream()
    if dist is not None:
        stream = tstream.cuda_stream
        assert stream, "need a non-NULL stream handle"

    def step():
        bla.gemm(da, db, dc, stream=stream)

    def barrier():
        if dist is not None:
            dist.barrier()
        bla.sync(stream)
        if dist is not None:
            import torch
            torch.cuda.synchronize()

    # Untimed pre-roll: the clocks of an idle MI355X take some tens of milliseconds of load to ramp (round 1: --warmup 5 read 0.88 of peak, --warmup 50
    # 0.945, same kernel).  The W warm-up steps and the K timed steps below are exactly what the contract asks for; this only makes sure they run on a
    # device that is awake, whatever W is.  Reported as config.preroll_s; --preroll 0 turns it off.
    t_pre = time.perf_counter()
    while args.preroll > 0 and time.perf_counter() - t_pre < args.preroll:
        for _ in range(10):
            step()
        bla.sync(stream)
    for _ in range(args.warmup):
        step()
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    bla.native.check(L.bla_event_create(C.byref(ev0)))
    bla.native.check(L.bla_event_create(C.byref(ev1)))
    barrier()
    t0 = time.perf_counter()
    bla.native.check(L.bla_event_record(ev0, stream))
    for _ in range(args.steps):
        step()
    bla.native.check(L.bla_event_record(ev1, stream))
    barrier()
    wall = time.perf_counter() - t0
    ms = C.c_float()
    bla.native.check(L.bla_event_elapsed_ms(ev0, ev1, C.byref(ms)))
    kernel_ms = ms.value / args.steps                       # HIP events on the launch stream: per-launch duration
    if dist is not None:
        import torch
        t = torch.tensor([wall], device="cuda", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        wall = float(t.item())

    flops = 2.0 * n ** 3
    value = world * args.steps * flops / wall / 1e9          # whole-job GFLOP/s over the barrier-bracketed region
    achieved_tflops = flops / (kernel_ms * 1e-3) / 1e12

    out = {
        "metric": "fp32 GFLOP/s matrix_mul 4096^3" if n == 4096 else f"fp32 GFLOP/s matrix_mul {n}^3",
        "value": round(value, 1), "unit": "GFLOP/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(wall / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"square fp32 matrix_multiply N={n} (BASELINE configs[1]), operands resident in HBM",
                   "kernel": L.bla_gemm_last_kernel().decode(), "parallelism": f"replicas x{world}", "preroll_s": args.preroll},
        "roofline": {"bound": "mfma", "achieved": round(achieved_tflops, 2), "peak": PEAK_FP32_MFMA_TFLOPS,
                     "unit": "TFLOP/s", "frac": round(achieved_tflops / PEAK_FP32_MFMA_TFLOPS, 4), "traffic": None,
                     "kernel_ms": round(kernel_ms, 4), "algorithmic_flops_per_launch": flops,
                     "algorithmic_bytes_per_launch": 3 * n * n * 4},
    }
    # HBM traffic of the dominant kernel comes from a separate rocprofv3 --pmc run (it cannot be collected from
    # inside this process); the committed summary applies when it was taken on this exact kernel and size
    for name in ("r03_gemm4096_traffic.json", "r01_gemm4096_traffic.json"):
        try:
            tr = json.load(open(os.path.join(ROOT, "profiles", name)))
            if n == 4096 and tr["kernel"] == out["config"]["kernel"]:
                out["roofline"]["traffic"] = tr["hbm_bytes_per_launch"]
                out["roofline"]["traffic_source"] = f"profiles/{name} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, gfx950-corrected)"
                break
        except (OSError, KeyError, ValueError):
            continue
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, dc, stream)
    # --full only: the GPU workloads are timed back to back; the CPU baselines (tens of seconds of host work) come after them
    sec, fault, ter, conv_arrays = None, None, None, None
    if args.full and args.mnist_steps > 0:
        try:
            sec, fault = run_mnist(bla, dist, world, rank, stream, args.mnist_steps, args.mnist_warmup, barrier)
        except Exception as e:       # the headline measurement above must still be reported
            import traceback
            traceback.print_exc()
            fault = {"stage": "secondary workload", "error": repr(e)}
            sec = {"metric": "MNIST-NN training samples/sec", "value": None, "unit": "samples/s", "n_gpus": world, "error": repr(e)} if rank == 0 else None
    if args.full and world == 1 and args.conv_steps > 0:
        try:
            ter, conv_arrays = run_conv(bla, stream, barrier, steps=args.conv_steps)
        except Exception as e:
            import traceback
            traceback.print_exc()
            ter, conv_arrays = ({"metric": "conv 128->128 k3 s1 @32x32 x64 images", "value": None, "error": repr(e)} if rank == 0 else None), None
        if ter is not None and args.unet_steps > 0:
            try:
                ter["unet_batch_64"] = run_unet(bla, stream, barrier, steps=args.unet_steps)
            except Exception as e:
                import traceback
                traceback.print_exc()
                ter["unet_batch_64"] = {"value": None, "error": repr(e)}
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        base, c_cpu, rows = cpu_baseline_gemm(n)
        out["cpu_baseline"] = base
        # the same slice doubles as a correctness check of what was just timed
        got = dc.numpy()[:rows].astype(np.float64)
        err = np.linalg.norm(got - c_cpu) / np.linalg.norm(c_cpu)
        out["config"]["rel_err_vs_cpu_slice"] = float(f"{err:.3e}")
        assert err < 1e-5, f"GPU result differs from the CPU reference slice: {err}"
    if sec is not None and rank == 0:
        if world == 1 and not args.no_cpu_baseline and sec.get("value") is not None:
            sec["cpu_baseline"] = cpu_baseline_mnist(256)
        out["secondary"] = sec
    if ter is not None and rank == 0:
        if not args.no_cpu_baseline and conv_arrays is not None:
            ter["cpu_baseline"], cerr = cpu_baseline_conv(conv_arrays)
            ter["config"]["rel_err_vs_cpu_image0"] = float(f"{cerr:.3e}")
            assert cerr < 1e-5, f"batched convolution differs from the CPU reference on image 0: {cerr}"
        out["tertiary"] = ter
    if rank == 0:
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy_process_group()
    if fault is not None and os.environ.get("BLA_BENCH_STRICT") == "1":
        sys.exit(3)      # the JSON line above says what happened (secondary.exchange_fault)


if __name__ == "__main__":
    main()
