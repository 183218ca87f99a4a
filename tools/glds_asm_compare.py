#!/usr/bin/env python3
"""Every kernel of the fp32 direct-to-LDS translation units in two device listings, parent against new (no GPU needed):
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -DBLA_BUILDING -I include --cuda-device-only -S big-linear-algebra_amd/csrc/bla_gemm.hip -o new_gemm.s
    python tools/glds_asm_compare.py parent_gemm.s new_gemm.s parent_gather.s new_gather.s
The parent's kernels are all instantiations of one template, gemm_f32_glds_kernel<BM, BN, BK, WM, WN, AKC, BKC, MINW, NBUF, PERSIST, GATHER, RCG, HS, WK, GW>;
the new ones are gemm_f32_glds_kernel<... without GATHER and GW> for GATHER = 0 and gather_kernel<GATHER, HS, GW> for the rest: kernels are paired through
that table, every other kernel by its own name.  A listing is normalised first -- labels renumbered in order of appearance, symbol names dropped, the literal
offsets of scalar loads from the kernarg pointer dropped (the argument block is passed by value: its layout may move) -- and each kernel gets a verdict:
    IDENTICAL    the normalised instruction sequences are the same
    IDENTICAL UP TO SGPR NUMBERS   the same instructions in the same order once the numbers of scalar registers are masked as well (the allocator named
                 a few scalars differently), and, where the note says so, the literal offsets of all scalar loads (a field of a by-value argument
                 block read through a copy of the kernarg pointer); the note counts the instructions that differ before masking
    SAME COUNTS  in every innermost loop around MFMAs the counts the pipelines' design fixes are the parent's -- v_mfma, ds_read by width, LDS-DMA
                 instructions by form, s_barrier, s_waitcnt vmcnt, the set of other vector memory loads -- and for the whole kernel scratch bytes and
                 AGPRs are equal and VGPRs not more
    DIFFERENT    anything else (exit status 1)
A parent kernel without a counterpart must be an RCG = true instantiation that launch_glds can never select (both operands K-contiguous, three buffers, or
persistent); it is listed as UNREACHABLE."""
import re, sys

GLDS = re.compile(r"_ZN3bla20gemm_f32_glds_kernelI((?:L[ib]\d+E)+)E")
GATHER = re.compile(r"_ZN3bla13gather_kernelI((?:L[ib]\d+E)+)E")

def logical(name, parent):
    """The name a kernel is paired under, and (parent only) its template arguments."""
    m = GLDS.match(name)
    if m:
        a = [int(x) for x in re.findall(r"L[ib](\d+)E", m.group(1))]
        if not parent:
            return "gemm_f32_glds_kernel<%s>" % ", ".join(map(str, a)), a
        if a[10]:
            return "gather_kernel<%d, %d, %d>" % (a[10], a[12], a[14]), a
        return "gemm_f32_glds_kernel<%s>" % ", ".join(map(str, a[:10] + a[11:14])), a
    m = GATHER.match(name)
    if m:
        return "gather_kernel<%s>" % ", ".join(re.findall(r"L[ib](\d+)E", m.group(1))), None
    return name.replace("NS_10GatherArgsE", "NS_8GemmArgsE"), None   # gather_pair_kernel: the same name over the new argument block

def kernels(path, parent):
    out, name, body, meta = {}, None, None, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body, meta = m.group(1), [], {}
            continue
        if name is None:
            continue
        k = re.match(r"^; (NumVgprs|NumAgprs|ScratchSize): (\d+)", line)
        if k:
            meta[k.group(1)] = int(k.group(2))
        k = re.match(r"^\s+\.amdhsa_user_sgpr_(private_segment_buffer|dispatch_ptr|queue_ptr) (\d)", line)
        if k:
            meta[k.group(1)] = int(k.group(2))
        if "ScratchSize" in meta:   # the last of the "Kernel info" comments, behind the code and its .amdhsa_kernel block
            out[logical(name, parent)[0]] = (body, meta, logical(name, parent)[1], name)
            name = None
            continue
        s = line.split(";")[0].strip()
        if s and not s.startswith((".", "//")) or re.match(r"^\.LBB\w+:", s):
            body.append(s)
    return out

def normalised(body, meta):
    karg = 4 * meta.get("private_segment_buffer", 0) + 2 * meta.get("dispatch_ptr", 0) + 2 * meta.get("queue_ptr", 0)
    kptr = "s[%d:%d]" % (karg, karg + 1)
    labels, out = {}, []
    for i in body:
        i = re.sub(r"\.LBB\w+", lambda m: labels.setdefault(m.group(0), "L%d" % len(labels)), i)
        i = re.sub(r"_Z\w+", "SYM", i)
        m = re.match(r"(s_load_dword\w*\s+\S+\s+)(s\[\d+:\d+\]), (0x[0-9a-f]+|\d+)(.*)", i)
        if m and m.group(2) == kptr:
            i = m.group(1) + m.group(2) + ", KARG" + m.group(4)
        m = re.match(r"(s_add_u32 s\d+, s%d, )(0x[0-9a-f]+|\d+)$" % karg, i)   # the address of what lies behind the argument block (the implicit arguments)
        if m:
            i = m.group(1) + "KARG"
        out.append(i)
    return out

def masked(body, loads=False):
    """scalar register numbers masked; loads: the literal offsets of every scalar load too"""
    out = []
    for i in body:
        if loads:
            i = re.sub(r"^(s_load_dword\w*\s+\S+\s+\S+,) (0x[0-9a-f]+|\d+)", r"\1 OFF", i)
        out.append(re.sub(r"\bs(\d+|\[\d+:\d+\])", "S", i))
    return out

def mfma_loops(body):
    """Innermost loops (label .. backward branch to it) that hold MFMAs, in order."""
    labels = {i[:-1]: n for n, i in enumerate(body) if i.endswith(":")}
    spans = []
    for n, i in enumerate(body):
        m = re.match(r"s_c?branch\w*\s+(\S+)", i)
        if m and labels.get(m.group(1), n) < n:
            spans.append((labels[m.group(1)], n))
    has = lambda a, b: any(i.startswith("v_mfma") for i in body[a:b])
    spans = [s for s in spans if has(*s)]
    inner = [s for s in spans if not any(t != s and s[0] <= t[0] and t[1] <= s[1] for t in spans)]
    return [[i for i in body[a:b + 1] if not i.endswith(":")] for a, b in inner]

def counts(loop):
    c = {}
    other = set()
    for i in loop:
        mn = i.split()[0]
        lds_dma = mn.startswith("global_load_lds") or (mn.startswith("buffer_load") and re.search(r"\blds\b", i))
        if mn.startswith("v_mfma"): key = "v_mfma"
        elif mn.startswith("ds_read"): key = mn
        elif lds_dma: key = mn + (" lds" if mn.startswith("buffer") else "")
        elif mn == "s_barrier": key = mn
        elif mn == "s_waitcnt" and "vmcnt" in i: key = "s_waitcnt vmcnt"
        elif re.match(r"(global|buffer|flat|scratch)_load", mn):
            other.add(mn); continue
        else: continue
        c[key] = c.get(key, 0) + 1
    c["other vector loads"] = tuple(sorted(other))
    return c

def main(argv):
    bad = 0
    tally = {}
    for parent, new in zip(argv[0::2], argv[1::2]):
        kp, kn = kernels(parent, True), kernels(new, False)
        print("== %s  (%d kernels)  against  %s  (%d kernels)" % (parent, len(kp), new, len(kn)))
        for name, (body, meta, args, _) in kp.items():
            if name not in kn:
                dead = args is not None and args[10] == 0 and args[11] == 1 and ((args[5] and args[6]) or args[8] != 2 or args[9])
                verdict = "UNREACHABLE" if dead else "DIFFERENT (no counterpart)"
                note = "scratch %d" % meta["ScratchSize"]
            else:
                nbody, nmeta = kn[name][0], kn[name][1]
                regs = "vgpr %d -> %d  agpr %d -> %d  scratch %d -> %d" % (meta["NumVgprs"], nmeta["NumVgprs"], meta["NumAgprs"], nmeta["NumAgprs"], meta["ScratchSize"], nmeta["ScratchSize"])
                na, nb = normalised(body, meta), normalised(nbody, nmeta)
                same_regs = all(meta[k] == nmeta[k] for k in ("NumVgprs", "NumAgprs", "ScratchSize"))
                renamed = [loads for loads in (False, True) if same_regs and masked(na, loads) == masked(nb, loads)]
                if na == nb:
                    verdict, note = "IDENTICAL", "vgpr %d agpr %d scratch %d" % (nmeta["NumVgprs"], nmeta["NumAgprs"], nmeta["ScratchSize"])
                elif renamed:
                    verdict = "IDENTICAL UP TO SGPR NUMBERS"
                    note = "%d of %d instructions differ before masking%s; vgpr %d agpr %d scratch %d" % (
                        sum(x != y for x, y in zip(na, nb)), len(na), " (scalar-load offsets masked too)" if renamed[0] else "", nmeta["NumVgprs"], nmeta["NumAgprs"], nmeta["ScratchSize"])
                else:
                    a, b = [counts(l) for l in mfma_loops(body)], [counts(l) for l in mfma_loops(nbody)]
                    ok = a == b and meta["ScratchSize"] == nmeta["ScratchSize"] and meta["NumAgprs"] == nmeta["NumAgprs"] and nmeta["NumVgprs"] <= meta["NumVgprs"]
                    verdict = "SAME COUNTS" if ok else "DIFFERENT"
                    note = regs + "  instructions %d -> %d" % (len(body), len(nbody))
                    if a != b:
                        note += "\n      parent loops: %s\n      new loops:    %s" % (a, b)
            bad += verdict.startswith("DIFFERENT")
            tally[verdict] = tally.get(verdict, 0) + 1
            print("%-12s %s   [%s]" % (verdict, name, note))
        for name in kn:
            if name not in kp:
                bad += 1
                print("DIFFERENT (no parent) %s" % name)
    print("total: " + ", ".join("%d %s" % (n, v) for v, n in sorted(tally.items())))
    return 1 if bad else 0

if __name__ == "__main__":
    if len(sys.argv) < 3 or len(sys.argv) % 2 == 0:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1:]))
