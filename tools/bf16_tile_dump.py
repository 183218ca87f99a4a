#!/usr/bin/env python3
"""Bit equality of two builds on everything the bf16 tile (csrc/bla_bf16_tile.h) computes: one process per build dumps the results, a third compares them.
    python tools/bf16_tile_dump.py dump <root of a built tree> <out.npz>
    python tools/bf16_tile_dump.py compare <parent.npz> <new.npz>
Inputs are uniform random (rounded to bf16 where the entry takes bf16), so a change in the order of accumulation would show.  The shapes, operands and
buffers are those of this tree's GPU tests: bla_gemm_bf16 at EXACT_SHAPES (nt and tn, fp32 and bf16 output, the `all` epilogue), bla_gemm_bf16_splitk at
EXACT_CASES (nt and tn), the forward (with a bias) and backward _as_bf16 convolution entries at the convolution's CASES, the weight-gradient entry at its
CASES x SPLITS."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, U16 = np.float32, np.uint16


def dump(root, out_path):
    spec = importlib.util.spec_from_file_location("graft_entry_of_the_build", os.path.join(root, "__graft_entry__.py"))
    entry = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(entry)
    dev = entry.load_pkg()
    dev.init(0)
    for d in ("tests", os.path.join("tests", "golden")):
        sys.path.insert(0, os.path.join(HERE, d))
    import test_bf16_gpu as G
    import test_bf16_splitk_gpu as S
    import test_conv_bf16_gpu as Cv
    import test_conv_wgrad_bf16_gpu as W
    arrays = {}
    for m, n, k in G.EXACT_SHAPES:
        for lay in ("nt", "tn"):
            for out in (F32, U16):
                got = G.rounded_case(dev, lay, m, n, k, "fast", out=out, **G.EPILOGUES["all"])[0]
                arrays["gemm/%dx%dx%d_%s_%s" % (m, n, k, lay, np.dtype(out).name)] = got
    for m, n, k, splits in S.EXACT_CASES:
        a, b = S.rounded_case(dev, m, n, k)[:2]
        for lay in ("nt", "tn"):
            A, B = S.operand_bufs(dev, lay, dev.to_bf16(a), dev.to_bf16(b))
            Cb = S.Buf(dev, m, n, n + 8, F32)
            name = S.run(dev, lay, m, n, k, A, B, Cb, splits=splits)
            assert name == S.expected_name(lay, k, splits), name
            arrays["splitk/%dx%dx%d_S%d_%s" % (m, n, k, splits, lay)] = Cb.read()
    for case, cid in zip(Cv.CASES, Cv.IDS):
        fwd, dx, dk = Cv.run_entries(dev, case, Cv.case_data(dev, case, "rounded"))[:3]
        arrays["conv_forward/" + cid], arrays["conv_data_gradient/" + cid], arrays["conv_weight_gradient/" + cid] = fwd, dx, dk
    for case, cid in zip(W.CASES, W.IDS):
        g = W.case_data(dev, case, "rounded")["dev"]
        for splits in W.SPLITS:
            out = W.Out(dev, (case[2], case[1], case[5], case[5]))
            W.wgrad(dev, g, case, out, splits)
            arrays["wgrad_entry/%s_S%d" % (cid, splits)] = out.read()
    assert all(np.isfinite(v.astype(F32) if v.dtype != U16 else dev.from_bf16(v)).all() for v in arrays.values()), "an element nobody wrote"
    np.savez(out_path, **arrays)
    print("%d arrays -> %s" % (len(arrays), out_path))


def compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    assert sorted(a.files) == sorted(b.files), "the two dumps hold different arrays"
    groups = {}
    for name in a.files:
        same = a[name].dtype == b[name].dtype and a[name].shape == b[name].shape and a[name].tobytes() == b[name].tobytes()
        n, bad = groups.get(name.split("/")[0], (0, 0))
        groups[name.split("/")[0]] = (n + 1, bad + (not same))
        if not same:
            print("DIFFERS:", name)
    for g, (n, bad) in sorted(groups.items()):
        print("%s: %d arrays, %d differ" % (g, n, bad))
    total, bad = sum(n for n, _ in groups.values()), sum(d for _, d in groups.values())
    print("%d arrays compared, %d differ" % (total, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "dump":
        dump(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
