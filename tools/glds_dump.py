#!/usr/bin/env python3
"""Bit equality of two builds on everything the fp32 direct-to-LDS kernels compute (csrc/bla_gemm_kernel.h, csrc/bla_gather_kernel.h): one process per
build writes a hash of every output, a third compares the two lists line for line.
    python tools/glds_dump.py dump <root of a built tree> <out.txt>
    python tools/glds_dump.py compare <parent.txt> <new.txt>
Inputs are seeded uniform random, so a change in the order of accumulation would show.  Shapes and operands are those of this tree's GPU tests:
  * every direct-to-LDS GEMM config (3-5, 7-15, 17, 18) x four layouts on two shapes -- one whose row-contiguous pitches are powers of two, one where
    they are not.  For configs 3-5, 7-10 and 18 that selects the global_load_lds (RCG) instantiation and the buffer_load ... lds one; configs 11-15 and
    17 always run the buffer form (bla_gemm.hip sets rc_global = 0 for them: their RCG instantiations exist and nothing launches them), so there the
    two shapes are two shapes of one kernel.  bla_gemm_last_kernel() does not name the form: which one ran follows from the pitch, not from the name;
  * K splits on every config, the persistent kernel at several tiles per workgroup (test_persistent_kernel_many_tiles_per_workgroup's shape);
  * every case of test_every_planned_path and test_operand_forms (tests/test_conv_paths_gpu.py): forward and backward, the fused epilogues at every site,
    the caller's padded copies, the prepared kernel matrices, the pair launch; the window of 16-pixel rows with an epilogue; the parity-class launch
    (tests/test_conv_gpu.py's headline shape).
The last lines name every kernel (bla_gemm_last_kernel) and plan (bla_conv_last_plan) seen."""
import hashlib
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
GLDS_CONFIGS = {3: None, 4: None, 5: 32, 7: None, 8: None, 9: None, 10: 32, 18: 32,      # config -> K must be a multiple of (None: 16)
                11: [(256, 32, 256), (512, 48, 256), (256, 160, 768), (768, 32, 256), (512, 512, 512)], 12: [(256, 64, 256), (512, 96, 256), (256, 160, 768), (768, 64, 256), (512, 512, 512)],
                13: [(128, 32, 512), (256, 48, 512), (128, 160, 1024), (128, 32, 1536), (384, 256, 512)], 14: [(128, 32, 128), (256, 48, 384), (128, 160, 640), (384, 256, 512)],
                15: [(128, 32, 256), (256, 48, 512), (128, 160, 768), (384, 256, 256)], 17: [(192, 32, 192), (384, 48, 192), (192, 160, 576), (384, 256, 384)]}
GENERAL = [(4, 32, 4), (64, 32, 64), (68, 64, 60), (132, 96, 128), (128, 128, 128), (260, 160, 36), (200, 256, 136), (384, 512, 256), (516, 16, 260), (300, 48, 520),
           (256, 80, 128), (132, 112, 140), (128, 144, 128)]


def pow2(v):
    return v & (v - 1) == 0


def two_shapes(cfg, ta, tb):
    """one shape whose row-contiguous pitches (m of a transposed A, n of a plain B) are all powers of two, one where none is (or not all are)"""
    spec = GLDS_CONFIGS[cfg]
    shapes = spec if isinstance(spec, list) else [s for s in GENERAL if s[1] % (spec or 16) == 0]
    rc = lambda s: [v for v, is_rc in ((s[0], ta), (s[2], not tb)) if is_rc]
    if ta == 0 and tb == 1:      # no row-contiguous operand: both forms are the same kernel
        return shapes[1:3]
    yes = [s for s in shapes if all(pow2(v) for v in rc(s))]
    no = [s for s in shapes if not any(pow2(v) for v in rc(s))] or [s for s in shapes if not all(pow2(v) for v in rc(s))]
    if not yes:      # 192-wide tiles: no extent is a power of two
        return [no[0]]
    return [yes[-1], no[0]]


def dump(root, out_path):
    spec = importlib.util.spec_from_file_location("graft_entry_of_the_build", os.path.join(root, "__graft_entry__.py"))
    entry = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(entry)
    dev = entry.load_pkg()
    dev.init(0)
    for d in ("tests", os.path.join("tests", "golden")):
        sys.path.insert(0, os.path.join(HERE, d))
    from inputs import uniform
    import test_conv_paths_gpu as T
    lines, names = [], set()

    def keep(name, array):
        assert np.isfinite(array).all(), "an element nobody wrote: " + name
        lines.append("%s %s %s" % (hashlib.sha256(np.ascontiguousarray(array).tobytes()).hexdigest(), "x".join(map(str, array.shape)), name))

    def gemm(cfg, split, m, k, n, ta, tb, tag, pitch=0):
        """pitch: the row pitch of the row-contiguous operands (0: their own extent); config 17 runs once on a pitch wider than the matrix"""
        a = uniform(10 + m, (k, pitch or m) if ta else (m, k), dtype=F32); b = uniform(50 + n, (n, k) if tb else (k, pitch or n), dtype=F32)
        c = dev.empty((m, n)).fill_bytes(0xFF)
        dev.lib().bla_gemm_set_config(cfg, split)
        try:
            dev.gemm(dev.to_device(a), dev.to_device(b), c, transa=bool(ta), transb=bool(tb), m=m, n=n, k=k, lda=a.shape[1], ldb=b.shape[1], ldc=n)
            kernel = dev.lib().bla_gemm_last_kernel().decode()
        except dev.BlaError as e:      # a forced config the library refuses for this shape: the refusal is the record
            lines.append("refused (status %s) gemm/%s/cfg%d/%s%s/%dx%dx%d" % (e.status, tag, cfg, "nt"[ta], "nt"[tb], m, k, n))
            return
        finally:
            dev.lib().bla_gemm_set_config(-1, 0)
        names.add("kernel " + kernel)
        keep("gemm/%s/cfg%d/%s%s/%dx%dx%d/%s" % (tag, cfg, "nt"[ta], "nt"[tb], m, k, n, kernel), c.numpy())

    for cfg in sorted(GLDS_CONFIGS):
        for ta, tb in ((0, 0), (0, 1), (1, 0), (1, 1)):
            for m, k, n in two_shapes(cfg, ta, tb):
                gemm(cfg, 0, m, k, n, ta, tb, "tile")
            m, k, n = (GLDS_CONFIGS[cfg] if isinstance(GLDS_CONFIGS[cfg], list) else [(200, 256, 136)])[-1]
            gemm(cfg, 2, m, k, n, ta, tb, "split2")
            if cfg == 17:
                gemm(cfg, 0, 192, 32, 192, ta, tb, "pitch256", pitch=256)
    for ta, tb in ((0, 0), (0, 1), (1, 0), (1, 1)):
        gemm(10, 0, 3100, 96, 3148, ta, tb, "persistent")

    def conv(case, forms):
        ops = T.Operands(dev, case); cid = T.case_id(case)
        def fwd(tag, **kw):
            out, out2, plan = T.run_forward(dev, ops, **kw)
            names.add("plan " + plan)
            keep("conv/%s/%s/out/%s" % (cid, tag, plan), out)
            if out2 is not None:
                keep("conv/%s/%s/out2/%s" % (cid, tag, plan), out2)
        def bwd(tag, **kw):
            dk, dx, plan = T.run_backward(dev, ops, **kw)
            names.add("plan " + plan)
            keep("conv/%s/%s/del_kern/%s" % (cid, tag, plan), dk); keep("conv/%s/%s/del_x/%s" % (cid, tag, plan), dx)
        fwd("plain"); bwd("plain")
        if not forms:
            return
        ops.with_epilogue(dev)
        for ep in ((True, False), (False, True), (True, True)):
            fwd("ep%d%d" % ep, ep=ep)
        if ops.with_padded(dev):
            fwd("padded", x_padded=True); bwd("padded", x_padded=True, dy_padded=True)
        mode_f, prep_f = ops.prepare(dev, False)
        mode_b, prep_b = ops.prepare(dev, True)
        if mode_f:
            fwd("prepared", prepared=prep_f)
        if mode_b:
            bwd("prepared", prepared=prep_b)

    window16 = (128, 16, 16, 32, 256, 3, 1, None)      # the window of 16-pixel rows with the tile store's epilogue
    for case in T.CASES:
        conv(case, case in T.FORMS or case == window16)
    for case in T.FORMS:
        if case not in T.CASES:
            conv(case, True)
    conv((64, 32, 32, 128, 256, 3, 2, None), False)      # the four parity classes of a stride-2 data gradient in one launch
    with open(out_path, "w") as f:
        f.write("\n".join(lines + sorted(names)) + "\n")
    print("%d arrays, %d kernel / plan names -> %s" % (len(lines), len(names), out_path))


def compare(a_path, b_path):
    a, b = open(a_path).read().splitlines(), open(b_path).read().splitlines()
    bad = 0
    for n in range(max(len(a), len(b))):
        la, lb = a[n] if n < len(a) else "(no line)", b[n] if n < len(b) else "(no line)"
        if la != lb:
            bad += 1
            print("DIFFERS line %d:\n  %s\n  %s" % (n + 1, la, lb))
    print("%d lines compared, %d differ" % (max(len(a), len(b)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "dump":
        dump(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
