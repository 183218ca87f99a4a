#!/usr/bin/env python3
"""The main slab loop of the bf16 MFMA kernels in two device listings (no GPU needed):
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -DBLA_BUILDING -I include --cuda-device-only -S big-linear-algebra_amd/csrc/bla_gemm_bf16.hip -o new_gemm.s
    python tools/bf16_tile_asm_compare.py parent_gemm.s new_gemm.s parent_conv.s new_conv.s
For every kernel that issues v_mfma_f32_32x32x16_bf16: the loop around its MFMAs (from the label the loop's backward branch jumps to, to that branch), and in
it the counts the tile's design fixes -- MFMAs, ds_read_b128, global_load_lds_dwordx4, s_barrier, s_waitcnt vmcnt -- any other vector memory load (there
must be none: a vector load in front of a DMA drains every DMA in flight), and the VALU / SALU instruction counts."""
import re, sys

def kernels(path):
    out, name, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
            out[name] = body
        elif name and line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
            name = None
        elif name:
            s = line.split(";")[0].strip()
            if s and not s.startswith((".", "//")) or re.match(r"^\.LBB\w+:", s):
                body.append(s)
    # keyed by the mangled name's own part: gemm_bf16_nt_kernelILb1ELb0EE = gemm_bf16_nt_kernel<true, false>
    return {re.search(r"N_1\d\d(\w+_kernel(I\w+?EE)?)", k).group(1): v for k, v in out.items() if any(i.startswith("v_mfma_f32_32x32x16_bf16") for i in v)}

def slab_loop(body):
    mf = [n for n, i in enumerate(body) if i.startswith("v_mfma")]
    labels = {i[:-1]: n for n, i in enumerate(body) if i.endswith(":")}
    for n in range(mf[-1], len(body)):   # the first backward branch behind the last MFMA whose target lies in front of the first one
        m = re.match(r"s_c?branch\w*\s+(\.LBB\w+)", body[n])
        if m and labels.get(m.group(1), len(body)) < mf[0]:
            return [i for i in body[labels[m.group(1)]:n + 1] if not i.endswith(":")]
    raise SystemExit("no loop around the MFMAs")

def counts(loop):
    mn = [i.split()[0] for i in loop]
    c = lambda f: sum(1 for i in mn if f(i))
    other = sorted(set(i for i in mn if re.match(r"(global|buffer|flat|scratch)_load", i) and not i.startswith("global_load_lds")))
    return {"mfma": c(lambda i: i.startswith("v_mfma_f32_32x32x16_bf16")), "ds_read_b128": c(lambda i: i == "ds_read_b128"),
            "global_load_lds_dwordx4": c(lambda i: i == "global_load_lds_dwordx4"), "s_barrier": c(lambda i: i == "s_barrier"),
            "s_waitcnt vmcnt": sum(1 for i in loop if i.startswith("s_waitcnt") and "vmcnt" in i), "other vector loads": other or "none",
            "valu": c(lambda i: i.startswith("v_") and not i.startswith("v_mfma")), "salu": c(lambda i: i.startswith("s_") and i not in ("s_barrier", "s_waitcnt", "s_nop")),
            "instructions": len(loop)}

for parent, new in zip(sys.argv[1::2], sys.argv[2::2]):
    kp, kn = kernels(parent), kernels(new)
    for name in kp:
        a, b = counts(slab_loop(kp[name])), counts(slab_loop(kn[name]))
        fixed = ("mfma", "ds_read_b128", "global_load_lds_dwordx4", "s_barrier", "s_waitcnt vmcnt", "other vector loads")
        print(f"{name}: {'SAME' if all(a[k] == b[k] for k in fixed) else 'DIFFERENT'} fixed counts")
        for k in a:
            print(f"    {k:<26} parent {a[k]!s:>6}   new {b[k]!s:>6}")
