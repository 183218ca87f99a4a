"""Every planned kernel path and operand form of the batched convolution (csrc/bla_conv.hip, bla_gather.hip, bla_conv_thin.hip), driven by name and held
element by element to the project's GEMM bound against a float64 reference.

What ran is read from bla_conv_last_plan() (include/bla.h has the grammar).  `plan_of` below restates the planner -- plan_forward, plan_backward,
use_tiled_gather, gather3_splits, the K splits of the weight gradient, plan_wsk_gather, parity_dgrad_applies, thin_conv_applies -- for a given CU count;
the case table states the plan of every case at 256 CUs (an MI355X), the GPU test asserts table == plan_of == what the library says it launched, and two
host tests pin the table's coverage: every entry of CHECKLIST is reached, and a sweep over about 100,000 shape and shift combinations finds no path outside it.

Reference: numpy float64 im2col products on the fp32 inputs with the SAME geometry restated here (forward and weight gradient), and the adjoint scatter
of kern^T . del_y for the data gradient -- a different formulation from the library's flipped-kernel convolution.  ora.conv_intended / ora.col2im_adjoint
cross-check it on the two smallest cases.

Bound (the project's GEMM bound, elementwise): |got - want| <= 1e-5 * (|A| @ |B|), for the weight gradient summed over the images; behind an epilogue
+ 2u (|conv| + |bias| + |add|), u = 2^-24, one rounding per add.  Index-only work (conv_prepare_kernels modes 1-3) is bit-exact.  Forward and data
gradient are checked in full on the first and last image and on two images whose 128-pixel tiles straddle an image boundary (where the geometry has
that), every image must be finite, and the batch-summed weight gradient covers all images.  Every output is a view inside an allocation of 0xFF bytes
with 64 guard floats on either side which must come back untouched, d_scratch included.  Each case runs twice with the largest other case in between
(which overwrites the grow-only workspace): first and second result agree bit for bit.

The host tests (no gpu marker) run a numpy float32 restatement of a tiled product -- slabs of 16 along K accumulated in fp32, K splits summed in order,
epilogue last -- through the same bound function: inside as written, outside under each mutation a subtly wrong kernel would amount to."""
import ctypes as C
import functools
import itertools
import re

import numpy as np
import pytest

from inputs import uniform

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
GUARD = 64
CUS = 256       # the table below is stated for an MI355X
BLA_ERR_INVALID = 1      # include/bla.h


# ---- the planner, restated ---------------------------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def same_geometry(h, w, k, s):
    """TF "SAME" (lib/conv.c:13-28,55-56): output size, top / left padding"""
    ho, wo = cdiv(h, s), cdiv(w, s)
    return ho, wo, max(0, (ho - 1) * s + k - h) // 2, max(0, (wo - 1) * s + k - w) // 2


def padded_geom(g):
    """rows, row pitch and floats per channel of the zero-padded, stride-split copy (padded_geom, csrc/bla_conv.hip)"""
    hp, wp = (g["ho"] - 1) * g["s"] + g["k"], (g["wo"] - 1) * g["s"] + g["k"]
    hh, wh = cdiv(hp, g["s"]), cdiv(cdiv(wp, g["s"]), 4) * 4
    return hh, wh, g["s"] * g["s"] * hh * wh


def geom(h, w, k, c, s, ho, wo, pt, pl):
    return dict(h=h, w=w, k=k, c=c, s=s, ho=ho, wo=wo, pt=pt, pl=pl)


def fwd_product(batch, h, w, k, cin, f, s, a_aligned=True, img_aligned=True, padded=False):
    ho, wo, pt, pl = same_geometry(h, w, k, s)
    return dict(g=geom(h, w, k, cin, s, ho, wo, pt, pl), M=f, N=ho * wo, K=k * k * cin, lda=k * k * cin, a_stride=0, a_aligned=a_aligned, img_aligned=img_aligned,
                padded=padded)


def wgrad_product(batch, h, w, k, cin, f, s, a_aligned=True, img_aligned=True, padded=False):
    ho, wo, pt, pl = same_geometry(h, w, k, s)
    return dict(g=geom(h, w, k, cin, s, ho, wo, pt, pl), M=f, N=k * k * cin, K=ho * wo, lda=ho * wo, a_stride=f * ho * wo, a_aligned=a_aligned, img_aligned=img_aligned,
                padded=padded)


def dgrad_product(batch, h, w, k, cin, f, s, img_aligned=True, padded=False):
    """the stride-1 convolution of the (zero-dilated) del_y with the flipped kernels; its A is the caller's scratch, always aligned here"""
    ho, wo, pt, pl = same_geometry(h, w, k, s)
    hd, wd = (ho - 1) * s + 1, (wo - 1) * s + 1
    return dict(g=geom(hd, wd, k, f, 1, h, w, k - 1 - pt, k - 1 - pl), M=cin, N=h * w, K=k * k * f, lda=k * k * f, a_stride=0, a_aligned=True, img_aligned=img_aligned,
                padded=padded and s == 1 and k % 2 == 1)


def gather_hs(mode, M, N):
    return M % 128 == 0 and N % 128 == 0 and mode in (3, 4)


def gather3_splits(M, N, K, cus):
    if not gather_hs(3, M, N):
        return 1
    tiles, slabs = (M // 128) * (N // 128), K // 16
    splits = max(1, min(cus // tiles, slabs // 8))
    per = cdiv(slabs, splits)
    return cdiv(slabs, per)


def gather_k_splits(mode, batch, M, N, hwo, cus):
    """K splits of a gathered weight gradient (gather_k_per_split, csrc/bla_gather.hip; M, N as the gathered product has them), off the side lane"""
    K = batch * hwo
    tiles = cdiv(M, 128) * cdiv(N, 128)
    splits, slabs = (2 * cus) // tiles, K // 16
    splits = min(splits, slabs // 8)
    if splits >= 32:
        splits &= ~7
    splits = max(splits, 1)
    return cdiv(K, cdiv(slabs, splits) * 16)


def fits32(a, batch):
    return batch * a["g"]["c"] * padded_geom(a["g"])[2] < 2 ** 29 and batch * a["M"] * a["g"]["ho"] * a["g"]["wo"] < 2 ** 29


def use_tiled_gather(a, batch, mode, cus):
    cols = a["N"] * batch if mode == 1 else a["N"]
    kk = a["K"] if mode == 1 else a["K"] * batch
    tiles = cdiv(a["M"], 128) * cdiv(cols, 128)
    if not (a["lda"] % 4 == 0 and a["a_aligned"]) or a["M"] < 64:
        return False
    if mode == 1:
        return a["K"] % 16 == 0 and (tiles >= 128 or (a["M"] % 128 == 0 and cols % 128 == 0 and a["g"]["wo"] % 4 == 0 and tiles * gather3_splits(a["M"], cols, a["K"], cus) >= 128))
    return a["K"] % 16 == 0 and kk >= 1024 and tiles * batch >= 128


def window_geometry(a, batch, cus):
    g = a["g"]
    return (g["s"] == 1 and g["k"] == 3 and g["pt"] == 1 and g["pl"] == 1 and g["w"] in (16, 32) and g["ho"] == g["h"] and g["wo"] == g["w"] and (g["h"] * g["w"]) % 128 == 0 and
            g["c"] % 16 == 0 and a["M"] % 128 == 0 and gather3_splits(a["M"], a["N"] * batch, a["K"], cus) == 1 and (a["M"] // 128) * (a["N"] * batch // 128) >= 2 * cus)


def plan_forward(a, batch, cus):
    """(path, fuses_epilogue): path one of wsk, m1, m3, m7"""
    if not use_tiled_gather(a, batch, 1, cus):
        return "wsk", batch == 1
    if not fits32(a, batch) or a["g"]["wo"] % 4 != 0:
        return "m1", False
    if window_geometry(a, batch, cus):
        return "m7", True
    return "m3", gather_hs(3, a["M"], a["N"] * batch)


def wsk_plan(a, batch, wgrad, target=768):
    """plan_wsk_gather: (vec, K splits)"""
    tiles = cdiv(a["M"], 32) * cdiv(a["N"], 32)
    splits = cdiv(target, tiles * batch)
    splits = max(1, min(splits, a["K"] // 128))
    splits = min(splits, 32)
    kps = cdiv(cdiv(a["K"], splits), 32) * 32
    splits = cdiv(a["K"], kps)
    vec = a["K"] % 4 == 0 and a["K"] >= 4 and a["lda"] % 4 == 0 and a["a_aligned"] and a["a_stride"] % 4 == 0
    return vec, splits


def wsk_token(a, batch, wgrad, target=768):
    vec, splits = wsk_plan(a, batch, wgrad, target)
    return "wsk/%s/s%d" % ("vec" if vec else "scalar", splits)


def padded_name(a):
    g = a["g"]
    return "caller" if a["padded"] else "image" if g["k"] == 1 and g["s"] == 1 and g["w"] % 4 == 0 and a["img_aligned"] else "copy"


def fixed_offsets(wo):
    return wo in (4, 8) or (wo >= 16 and wo % 16 == 0)


def wgrad_core(a, batch, cus):
    """(mode, half-slab, splits) of a weight gradient on the tiled kernels"""
    mode = 4 if fits32(a, batch) and a["g"]["wo"] % 4 == 0 and a["N"] % 4 == 0 else 2
    M, N = (a["N"], a["M"]) if mode == 4 else (a["M"], a["N"])
    hs = mode == 4 and gather_hs(4, M, N) and fixed_offsets(a["g"]["wo"])
    return mode, hs, gather_k_splits(mode, batch, M, N, a["K"], cus)


def forward_token(role, a, batch, cus, ep=False, prepared=False):
    """one forward-shaped product through launch_implicit<CONV_FWD>"""
    path, fuses = plan_forward(a, batch, cus)
    fused = ep and fuses
    tail = "" if fused else "/ep=pass" if ep else "/ep=none"
    prep = "/A=prep" if prepared else ""
    if path == "wsk":
        return "%s:%s%s%s%s" % (role, wsk_token(a, batch, False), "/ep=wsk" if fused else "", tail, prep)
    if path == "m1":
        return "%s:m1%s%s" % (role, tail, prep)
    if path == "m7":
        return "%s:m7w%d%s%s%s" % (role, a["g"]["w"], "/ep=tile" if fused else "", tail, prep)
    cols = a["N"] * batch
    hs, splits = gather_hs(3, a["M"], cols), gather3_splits(a["M"], cols, a["K"], cus)
    site = ("/ep=tile" if splits == 1 else "/ep=fold") if fused else ""
    return "%s:m3%s/s%d%s%s/pad=%s%s" % (role, "hs" if hs else "", splits, site, tail, padded_name(a), prep)


def thin_conv_applies(k, cin, f, s):
    return s == 1 and k in (1, 3) and (cin <= 4 or (f <= 4 and cin * k * k <= 3584))


def parity_taps(k, pad, r):
    return [(p, (p - pad - r) // 2) for p in range(k) if (p - pad - r) % 2 == 0 and p - pad - r >= 0][:4]


def parity_applies(batch, h, w, k, cin, f, s):
    ho, wo, pt, pl = same_geometry(h, w, k, s)
    if s != 2 or h % 2 or w % 8 or k > 4 or f % 16 or cin % 128 or (batch * (h // 2) * (w // 2)) % 128:
        return False
    a, b, c, d = parity_taps(k, pt, 0), parity_taps(k, pt, 1), parity_taps(k, pl, 0), parity_taps(k, pl, 1)
    if not (a and b and c and d):
        return False
    copy_floats, cls_floats = batch * f * (ho + 2) * (cdiv(wo + 2, 4) * 4), batch * cin * (h // 2) * (w // 2)
    return len(a) + len(b) == k and len(c) + len(d) == k and ho == h // 2 and wo == w // 2 and copy_floats < 2 ** 29 and cls_floats < 2 ** 29


def parity_token(batch, h, w, k, cin, f, cus):
    _, _, pt, pl = same_geometry(h, w, k, 2)
    P, Q = [parity_taps(k, pt, r) for r in (0, 1)], [parity_taps(k, pl, r) for r in (0, 1)]
    N = batch * (h // 2) * (w // 2)
    if gather_hs(3, cin, N) and 4 * (cin // 128) * (N // 128) >= 2 * cus - cus // 2:
        return "dgrad:parity/one[m3hs/x4]"
    each = ["m3%s/s%d" % ("hs" if gather_hs(3, cin, N) else "", gather3_splits(cin, N, f * len(P[c >> 1]) * len(Q[c & 1]), cus)) for c in range(4)]
    return "dgrad:parity/each[%s]" % ",".join(each)


def plan_of(case, cus=CUS, ep=False, x_padded=False, dy_padded=False, prepared_fwd=False, prepared_bwd=False):
    """(forward plan, backward plan) of bla_conv2d_forward_fused_f32 / bla_conv2d_backward_prepared_f32 on (batch, h, w, cin, f, k, s, shift)"""
    batch, h, w, cin, f, k, s, shift = case
    al = lambda name: shift != name
    if thin_conv_applies(k, cin, f, s):
        return "fwd:thin" + ("/ep=thin" if ep else ""), "wgrad:thin dgrad:thin"
    af = fwd_product(batch, h, w, k, cin, f, s, al("kern"), al("x"), x_padded)
    fwd = forward_token("fwd", af, batch, cus, ep, prepared_fwd and plan_forward(af, batch, cus)[0] == "m7")
    aw = wgrad_product(batch, h, w, k, cin, f, s, al("del_y"), al("x"), x_padded)
    ad = dgrad_product(batch, h, w, k, cin, f, s, al("del_y"), dy_padded)
    tw, td = use_tiled_gather(aw, batch, 2, cus), use_tiled_gather(ad, batch, 1, cus)
    if s == 1:
        dpath = plan_forward(ad, batch, cus)[0]
        if not tw and not td:
            return fwd, "wskpair:%s+%s" % (wsk_token(aw, batch, True, 384), wsk_token(ad, batch, False, 384))
        if (ad["N"] * batch <= 2048 and tw and fits32(aw, batch) and fixed_offsets(aw["g"]["wo"]) and aw["N"] % 4 == 0 and gather_hs(4, aw["N"], aw["M"]) and
                (dpath == "m7" or (dpath == "m3" and gather_hs(3, ad["M"], ad["N"] * batch)))):
            _, _, ws = wgrad_core(aw, batch, cus)
            dtok = "m7w%d" % ad["g"]["w"] if dpath == "m7" else "m3hs/s%d" % gather3_splits(ad["M"], ad["N"] * batch, ad["K"], cus)
            return fwd, "pair:m4hs/s%d+%s/ep=none/padw=%s%s%s" % (ws, dtok, padded_name(aw), "" if dpath == "m7" else "/padd=" + padded_name(ad), "/A=prep" if prepared_bwd else "")
    if tw:
        mode, hs, splits = wgrad_core(aw, batch, cus)
        wtok = "wgrad:m%d%s/s%d%s" % (mode, "hs" if hs else "", splits, "/pad=" + padded_name(aw) if mode == 4 else "")
    else:
        wtok = "wgrad:" + wsk_token(aw, batch, True)
    if parity_applies(batch, h, w, k, cin, f, s):
        return fwd, wtok + " " + parity_token(batch, h, w, k, cin, f, cus)
    return fwd, wtok + " " + forward_token("dgrad" if s == 1 else "dgrad.dil", ad, batch, cus, False, prepared_bwd and s == 1)


def prep_mode_of(case, cus, data_gradient):
    """conv_kernel_prep_mode: which prepared form the forward / data-gradient product of this convolution reads (0: none)"""
    batch, h, w, cin, f, k, s, _ = case
    if batch < 2 or thin_conv_applies(k, cin, f, s):
        return 0
    if not data_gradient:
        return 1 if plan_forward(fwd_product(batch, h, w, k, cin, f, s), batch, cus)[0] == "m7" else 0
    if s != 1:
        return 0
    ad = dgrad_product(batch, h, w, k, cin, f, 1)
    if not use_tiled_gather(wgrad_product(batch, h, w, k, cin, f, 1), batch, 2, cus) and not use_tiled_gather(ad, batch, 1, cus):
        return 0
    return 2 if plan_forward(ad, batch, cus)[0] == "m7" else 3


def forms_plans(case, cus=CUS):
    """the plans test_operand_forms must see, in its order: the forward with an epilogue; forward and backward on the caller's padded copies (stride 1, rows of
    whole float4); the forward and the backward on a prepared kernel matrix (where bla_conv_prep_mode names one)"""
    s, w = case[6], case[2]
    out = [plan_of(case, cus, ep=True)[0]]
    if s == 1 and w % 4 == 0:
        out += list(plan_of(case, cus, x_padded=True, dy_padded=True))
    if prep_mode_of(case, cus, False):
        out.append(plan_of(case, cus, prepared_fwd=True)[0])
    if prep_mode_of(case, cus, True):
        out.append(plan_of(case, cus, prepared_bwd=True)[1])
    return tuple(out)


def kinds(plan):
    """the tokens of a plan with their numbers and attributes taken off: role:path, K splits as s1 / sN"""
    out = []
    for tok in plan.split():
        role, path = tok.split(":", 1)
        path = re.sub(r"/(ep|pad|padw|padd|A)=\w+", "", path)
        path = re.sub(r"\[.*\]", "", path)
        path = re.sub(r"/s(\d+)", lambda m: "" if role == "wskpair" else "/s1" if m.group(1) == "1" else "/sN", path)
        out.append(role + ":" + path)
    return out


# ---- the case table ------------------------------------------------------------------------------------------------------------------------------------
# (batch, h, w, c_in, f_n, k, stride, shift) -> (forward plan, backward plan) at 256 CUs.  shift: the one operand moved one float off its 16-byte
# alignment (x, kern, out, del_y, del_kern, del_x) or None.
CASES = {
    # wo = 10: no padded copy -- the bounds-checked forward / data gradient (mode 1) and weight gradient (mode 2); 160-pixel images: tiles straddle
    (104, 16, 10, 128, 128, 3, 1, None):
        ('fwd:m1/ep=none', 'wgrad:m2/s55 dgrad:m1/ep=none'),
    # ... and mode 1 on the zero-dilated del_y (15 x 9 with wo = 10 output columns)
    (104, 16, 10, 128, 128, 3, 2, None):
        ('fwd:wsk/vec/s1/ep=none', 'wgrad:wsk/vec/s1 dgrad.dil:m1/ep=none'),
    # window of 16-pixel rows, two channel groups; weight gradient on the older form (ragged tap tiles)
    (128, 16, 16, 32, 256, 3, 1, None):
        ('fwd:m7w16/ep=none', 'wgrad:m4/s79/pad=copy dgrad:wsk/vec/s1/ep=none'),
    # window 16 for forward and data gradient, 16 groups: the largest case
    (128, 16, 16, 256, 256, 3, 1, None):
        ('fwd:m7w16/ep=none', 'wgrad:m4hs/s14/pad=copy dgrad:m7w16/ep=none'),
    # window of 32-pixel rows, one channel group (no prefetch of a next group)
    (32, 32, 32, 16, 256, 3, 1, None):
        ('fwd:m7w32/ep=none', 'wgrad:m4/s128/pad=copy dgrad:wsk/vec/s1/ep=none'),
    # ... three groups: the prefetch guard taken, then not taken
    (32, 32, 32, 48, 256, 3, 1, None):
        ('fwd:m7w32/ep=none', 'wgrad:m4/s64/pad=copy dgrad:wsk/vec/s1/ep=none'),
    # window 32 as the data gradient (two groups of del_y channels); 32 filters keep forward and weight gradient on the 32x32 kernel
    (64, 32, 32, 128, 32, 3, 1, None):
        ('fwd:wsk/vec/s1/ep=none', 'wgrad:wsk/vec/s1 dgrad:m7w32/ep=none'),
    # half-slab padded copy, one pass over K: the tile store's own epilogue site
    (64, 16, 16, 256, 256, 3, 1, None):
        ('fwd:m3hs/s1/ep=none/pad=copy', 'wgrad:m4hs/s14/pad=copy dgrad:m3hs/s1/ep=none/pad=copy'),
    # taps cut 3 ways; wo = 12: weight gradient on the older form although its tiles are whole; 144-pixel images straddle
    (64, 12, 12, 128, 128, 3, 1, None):
        ('fwd:m3hs/s3/ep=none/pad=copy', 'wgrad:m4/s53/pad=copy dgrad:m3hs/s3/ep=none/pad=copy'),
    # taps cut 7 ways (ragged last split); 288-pixel images straddle
    (16, 9, 32, 128, 128, 3, 1, None):
        ('fwd:m3hs/s7/ep=none/pad=copy', 'wgrad:m4hs/s32/pad=copy dgrad:m3hs/s7/ep=none/pad=copy'),
    # taps cut 8 ways
    (16, 16, 16, 128, 128, 3, 1, None):
        ('fwd:m3hs/s8/ep=none/pad=copy', 'wgrad:m4hs/s32/pad=copy dgrad:m3hs/s8/ep=none/pad=copy'),
    # taps cut 9 ways; both gradients in one launch of the tiled kernels
    (32, 8, 8, 128, 128, 3, 1, None):
        ('fwd:m3hs/s9/ep=none/pad=copy', 'pair:m4hs/s16+m3hs/s9/ep=none/padw=copy/padd=copy'),
    # ... the pair on 4-pixel rows, taps cut 16 ways
    (64, 4, 4, 256, 256, 3, 1, None):
        ('fwd:m3hs/s16/ep=none/pad=copy', 'pair:m4hs/s8+m3hs/s16/ep=none/padw=copy/padd=copy'),
    # ragged M and N tiles: padded copy and weight gradient on the older forms
    (64, 16, 16, 16, 64, 3, 1, None):
        ('fwd:m3/s1/ep=none/pad=copy', 'wgrad:m4/s128/pad=copy dgrad:wsk/vec/s2/ep=none'),
    # 1x1: the image is its own padded copy; the batched weight gradient beside it on the 32x32 kernel (one 128 x 128 tile per image: 64 tiles, under the 128 a tiled launch needs)
    (64, 20, 20, 128, 128, 1, 1, None):
        ('fwd:m3hs/s1/ep=none/pad=image', 'wgrad:wsk/vec/s1 dgrad:m3hs/s1/ep=none/pad=image'),
    # even kernel (padding at the bottom / right only): the data gradient alone on the tiled kernels, older form; weight gradient with its pixels cut over workgroups
    (64, 16, 16, 72, 24, 2, 1, None):
        ('fwd:wsk/vec/s2/ep=none', 'wgrad:wsk/vec/s2 dgrad:m3/s1/ep=none/pad=copy'),
    # stride 2 by parity, class by class, taps cut [4, 2, 2, 1]
    (16, 8, 8, 128, 128, 3, 2, None):
        ('fwd:wsk/vec/s9/ep=none', 'wgrad:wsk/vec/s1 dgrad:parity/each[m3hs/s4,m3hs/s2,m3hs/s2,m3hs/s1]'),
    # ... [8, 4, 4, 2]
    (16, 8, 8, 128, 256, 3, 2, None):
        ('fwd:wsk/vec/s6/ep=none', 'wgrad:wsk/vec/s1 dgrad:parity/each[m3hs/s8,m3hs/s4,m3hs/s4,m3hs/s2]'),
    # ... a 2x2 kernel: one tap per class
    (16, 8, 8, 128, 128, 2, 2, None):
        ('fwd:wsk/vec/s4/ep=none', 'wgrad:wsk/vec/s1 dgrad:parity/each[m3hs/s1,m3hs/s1,m3hs/s1,m3hs/s1]'),
    # a 4x4 kernel is not admitted by parity_dgrad_applies (its taps do not split 2 + 2 with pad 1): zero-dilated on the half-slab kernel, taps cut
    (16, 8, 8, 128, 128, 4, 2, None):
        ('fwd:wsk/vec/s11/ep=none', 'wgrad:wsk/vec/s1 dgrad.dil:m3hs/s16/ep=none/pad=copy'),
    # 192 input channels: zero-dilated on the padded copy, older form
    (64, 16, 16, 192, 128, 3, 2, None):
        ('fwd:m3hs/s8/ep=none/pad=copy', 'wgrad:m4/s32/pad=copy dgrad.dil:m3/s1/ep=none/pad=copy'),
    # zero-dilated on the half-slab kernel in one pass (K = 128)
    (64, 16, 16, 128, 8, 4, 2, None):
        ('fwd:wsk/vec/s6/ep=none', 'wgrad:wsk/vec/s1 dgrad.dil:m3hs/s1/ep=none/pad=copy'),
    # at most four channels on one side: the thin kernels (test_thin_convolutions keeps their numbers)
    (2, 16, 16, 3, 8, 3, 1, None):
        ('fwd:thin', 'wgrad:thin dgrad:thin'),
    # the 32x32 kernel, single image: scalar loads forward and dilated (K = 5)
    (1, 4, 4, 5, 5, 1, 2, None):
        ('fwd:wsk/scalar/s1/ep=none', 'wgrad:wsk/vec/s1 dgrad.dil:wsk/scalar/s1/ep=none'),
    # ... 16-byte loads (K = 20)
    (1, 4, 4, 5, 5, 2, 2, None):
        ('fwd:wsk/vec/s1/ep=none', 'wgrad:wsk/vec/s1 dgrad.dil:wsk/vec/s1/ep=none'),
    # ... dilated with K = 256 cut over two workgroups
    (1, 4, 4, 5, 64, 2, 2, None):
        ('fwd:wsk/vec/s1/ep=none', 'wgrad:wsk/vec/s1 dgrad.dil:wsk/vec/s2/ep=none'),
    # ... weight gradient with scalar loads (9 pixels)
    (1, 5, 5, 5, 5, 1, 2, None):
        ('fwd:wsk/scalar/s1/ep=none', 'wgrad:wsk/scalar/s1 dgrad.dil:wsk/scalar/s1/ep=none'),
    # ... weight gradient with scalar loads, 289 pixels cut over workgroups
    (2, 33, 33, 8, 8, 3, 2, None):
        ('fwd:wsk/vec/s1/ep=none', 'wgrad:wsk/scalar/s2 dgrad.dil:wsk/vec/s1/ep=none'),
    # forward with scalar loads (K = 261) cut over two workgroups
    (1, 8, 8, 29, 24, 3, 1, None):
        ('fwd:wsk/scalar/s2/ep=none', 'wskpair:wsk/vec/s1+wsk/vec/s1'),
    # the pair on the 32x32 kernel: scalar + scalar
    (1, 5, 5, 5, 5, 1, 1, None):
        ('fwd:wsk/scalar/s1/ep=none', 'wskpair:wsk/scalar/s1+wsk/scalar/s1'),
    # ... scalar + 16-byte
    (1, 5, 5, 5, 5, 2, 1, None):
        ('fwd:wsk/vec/s1/ep=none', 'wskpair:wsk/scalar/s1+wsk/vec/s1'),
    # ... 16-byte + scalar
    (1, 4, 4, 5, 5, 1, 1, None):
        ('fwd:wsk/scalar/s1/ep=none', 'wskpair:wsk/vec/s1+wsk/scalar/s1'),
    # ... 16-byte + 16-byte, both cut over workgroups
    (1, 16, 16, 5, 64, 2, 1, None):
        ('fwd:wsk/vec/s1/ep=none', 'wskpair:wsk/vec/s2+wsk/vec/s2'),
    # ... a batch, 289 pixels: scalar weight gradient cut over workgroups + scalar data gradient (K = 54)
    (3, 17, 17, 5, 6, 3, 1, None):
        ('fwd:wsk/scalar/s1/ep=none', 'wskpair:wsk/scalar/s2+wsk/scalar/s1'),
    # the alignment shape on the 32x32 kernel
    (5, 16, 16, 32, 24, 3, 1, None):
        ('fwd:wsk/vec/s2/ep=none', 'wskpair:wsk/vec/s2+wsk/vec/s1'),
    # a shifted image leaves every plan alone
    (5, 16, 16, 32, 24, 3, 1, 'x'):
        ('fwd:wsk/vec/s2/ep=none', 'wskpair:wsk/vec/s2+wsk/vec/s1'),
    # a shifted kernel matrix: the forward falls to the 32x32 kernel with scalar loads; the gradients read a flipped copy
    (5, 16, 16, 32, 24, 3, 1, 'kern'):
        ('fwd:wsk/scalar/s2/ep=none', 'wskpair:wsk/vec/s2+wsk/vec/s1'),
    # a shifted output: scalar stores / the scalar fold
    (5, 16, 16, 32, 24, 3, 1, 'out'):
        ('fwd:wsk/vec/s2/ep=none', 'wskpair:wsk/vec/s2+wsk/vec/s1'),
    # a shifted del_y: the weight gradient falls to the 32x32 kernel with scalar loads
    (5, 16, 16, 32, 24, 3, 1, 'del_y'):
        ('fwd:wsk/vec/s2/ep=none', 'wskpair:wsk/scalar/s2+wsk/vec/s1'),
    # a shifted weight gradient
    (5, 16, 16, 32, 24, 3, 1, 'del_kern'):
        ('fwd:wsk/vec/s2/ep=none', 'wskpair:wsk/vec/s2+wsk/vec/s1'),
    # a shifted data gradient
    (5, 16, 16, 32, 24, 3, 1, 'del_x'):
        ('fwd:wsk/vec/s2/ep=none', 'wskpair:wsk/vec/s2+wsk/vec/s1'),
    # a shifted image leaves every plan alone
    (32, 8, 8, 128, 128, 3, 1, 'x'):
        ('fwd:m3hs/s9/ep=none/pad=copy', 'pair:m4hs/s16+m3hs/s9/ep=none/padw=copy/padd=copy'),
    # a shifted kernel matrix: the forward falls to the 32x32 kernel with scalar loads; the gradients read a flipped copy
    (32, 8, 8, 128, 128, 3, 1, 'kern'):
        ('fwd:wsk/scalar/s3/ep=none', 'pair:m4hs/s16+m3hs/s9/ep=none/padw=copy/padd=copy'),
    # a shifted output: scalar stores / the scalar fold
    (32, 8, 8, 128, 128, 3, 1, 'out'):
        ('fwd:m3hs/s9/ep=none/pad=copy', 'pair:m4hs/s16+m3hs/s9/ep=none/padw=copy/padd=copy'),
    # a shifted del_y: the weight gradient falls to the 32x32 kernel with scalar loads
    (32, 8, 8, 128, 128, 3, 1, 'del_y'):
        ('fwd:m3hs/s9/ep=none/pad=copy', 'wgrad:wsk/scalar/s1 dgrad:m3hs/s9/ep=none/pad=copy'),
    # a shifted weight gradient
    (32, 8, 8, 128, 128, 3, 1, 'del_kern'):
        ('fwd:m3hs/s9/ep=none/pad=copy', 'pair:m4hs/s16+m3hs/s9/ep=none/padw=copy/padd=copy'),
    # a shifted data gradient
    (32, 8, 8, 128, 128, 3, 1, 'del_x'):
        ('fwd:m3hs/s9/ep=none/pad=copy', 'pair:m4hs/s16+m3hs/s9/ep=none/padw=copy/padd=copy'),
    # a shifted image leaves every plan alone
    (32, 32, 32, 48, 256, 3, 1, 'x'):
        ('fwd:m7w32/ep=none', 'wgrad:m4/s64/pad=copy dgrad:wsk/vec/s1/ep=none'),
    # a shifted kernel matrix: the forward falls to the 32x32 kernel with scalar loads; the gradients read a flipped copy
    (32, 32, 32, 48, 256, 3, 1, 'kern'):
        ('fwd:wsk/scalar/s1/ep=none', 'wgrad:m4/s64/pad=copy dgrad:wsk/vec/s1/ep=none'),
    # a shifted output: scalar stores / the scalar fold
    (32, 32, 32, 48, 256, 3, 1, 'out'):
        ('fwd:m7w32/ep=none', 'wgrad:m4/s64/pad=copy dgrad:wsk/vec/s1/ep=none'),
    # a shifted del_y: the weight gradient falls to the 32x32 kernel with scalar loads
    (32, 32, 32, 48, 256, 3, 1, 'del_y'):
        ('fwd:m7w32/ep=none', 'wskpair:wsk/scalar/s1+wsk/vec/s1'),
    # a shifted weight gradient
    (32, 32, 32, 48, 256, 3, 1, 'del_kern'):
        ('fwd:m7w32/ep=none', 'wgrad:m4/s64/pad=copy dgrad:wsk/vec/s1/ep=none'),
    # a shifted data gradient
    (32, 32, 32, 48, 256, 3, 1, 'del_x'):
        ('fwd:m7w32/ep=none', 'wgrad:m4/s64/pad=copy dgrad:wsk/vec/s1/ep=none'),
}

# case -> the plans test_operand_forms sees (forms_plans has their order): one shape per forward path and epilogue site
FORMS = {
    (64, 16, 16, 256, 256, 3, 1, None):
        ('fwd:m3hs/s1/ep=tile/pad=copy', 'fwd:m3hs/s1/ep=none/pad=caller', 'wgrad:m4hs/s14/pad=caller dgrad:m3hs/s1/ep=none/pad=caller', 'wgrad:m4hs/s14/pad=copy dgrad:m3hs/s1/ep=none/pad=copy/A=prep'),
    (32, 32, 32, 48, 256, 3, 1, None):
        ('fwd:m7w32/ep=tile', 'fwd:m7w32/ep=none', 'wgrad:m4/s64/pad=caller dgrad:wsk/vec/s1/ep=none', 'fwd:m7w32/ep=none/A=prep', 'wgrad:m4/s64/pad=copy dgrad:wsk/vec/s1/ep=none/A=prep'),
    (64, 32, 32, 128, 32, 3, 1, None):
        ('fwd:wsk/vec/s1/ep=pass', 'fwd:wsk/vec/s1/ep=none', 'wgrad:wsk/vec/s1 dgrad:m7w32/ep=none', 'wgrad:wsk/vec/s1 dgrad:m7w32/ep=none/A=prep'),
    (32, 8, 8, 128, 128, 3, 1, None):
        ('fwd:m3hs/s9/ep=fold/pad=copy', 'fwd:m3hs/s9/ep=none/pad=caller', 'pair:m4hs/s16+m3hs/s9/ep=none/padw=caller/padd=caller', 'pair:m4hs/s16+m3hs/s9/ep=none/padw=copy/padd=copy/A=prep'),
    (104, 16, 10, 128, 128, 3, 1, None):
        ('fwd:m1/ep=pass', 'wgrad:m2/s55 dgrad:m1/ep=none/A=prep'),
    (64, 16, 16, 16, 64, 3, 1, None):
        ('fwd:m3/s1/ep=pass/pad=copy', 'fwd:m3/s1/ep=none/pad=caller', 'wgrad:m4/s128/pad=caller dgrad:wsk/vec/s2/ep=none', 'wgrad:m4/s128/pad=copy dgrad:wsk/vec/s2/ep=none/A=prep'),
    (64, 20, 20, 128, 128, 1, 1, None):
        ('fwd:m3hs/s1/ep=tile/pad=image', 'fwd:m3hs/s1/ep=none/pad=caller', 'wgrad:wsk/vec/s1 dgrad:m3hs/s1/ep=none/pad=caller', 'wgrad:wsk/vec/s1 dgrad:m3hs/s1/ep=none/pad=image/A=prep'),
    (5, 16, 16, 32, 24, 3, 1, None):
        ('fwd:wsk/vec/s2/ep=pass', 'fwd:wsk/vec/s2/ep=none', 'wskpair:wsk/vec/s2+wsk/vec/s1'),
    (1, 16, 16, 32, 24, 3, 1, None):
        ('fwd:wsk/vec/s2/ep=wsk', 'fwd:wsk/vec/s2/ep=none', 'wskpair:wsk/vec/s2+wsk/vec/s1'),
    (2, 16, 16, 3, 8, 3, 1, None):
        ('fwd:thin/ep=thin', 'fwd:thin', 'wgrad:thin dgrad:thin'),
}

# every path of the family that the default switches can reach, as kinds(): the table reaches each of them (test_table_reaches_the_checklist), and a sweep
# finds nothing outside it (test_no_reachable_path_is_missing_from_the_checklist)
CHECKLIST = [
    'dgrad.dil:m1',
    'dgrad.dil:m3/s1',
    'dgrad.dil:m3hs/s1',
    'dgrad.dil:m3hs/sN',
    'dgrad.dil:wsk/scalar/s1',
    'dgrad.dil:wsk/vec/s1',
    'dgrad.dil:wsk/vec/sN',
    'dgrad:m1',
    'dgrad:m3/s1',
    'dgrad:m3hs/s1',
    'dgrad:m3hs/sN',
    'dgrad:m7w16',
    'dgrad:m7w32',
    'dgrad:parity/each',
    'dgrad:thin',
    'dgrad:wsk/vec/s1',
    'dgrad:wsk/vec/sN',
    'fwd:m1',
    'fwd:m3/s1',
    'fwd:m3hs/s1',
    'fwd:m3hs/sN',
    'fwd:m7w16',
    'fwd:m7w32',
    'fwd:thin',
    'fwd:wsk/scalar/s1',
    'fwd:wsk/scalar/sN',
    'fwd:wsk/vec/s1',
    'fwd:wsk/vec/sN',
    'pair:m4hs/sN+m3hs/sN',
    'wgrad:m2/sN',
    'wgrad:m4/sN',
    'wgrad:m4hs/sN',
    'wgrad:thin',
    'wgrad:wsk/scalar/s1',
    'wgrad:wsk/scalar/sN',
    'wgrad:wsk/vec/s1',
    'wgrad:wsk/vec/sN',
    'wskpair:wsk/scalar+wsk/scalar',
    'wskpair:wsk/scalar+wsk/vec',
    'wskpair:wsk/vec+wsk/scalar',
    'wskpair:wsk/vec+wsk/vec',
]
# reached only at sizes another file already runs (tests/test_conv_gpu.py, test_headline_shapes_batch_64_against_the_oracle: (64, 32, 32, 128, 256, 3, 2))
ELSEWHERE = {"dgrad:parity/one"}
# attribute values the operand-form cases (FORMS) must reach: the four epilogue sites (and the thin kernels' own), the three padded operands, a prepared matrix
ATTRIBUTES = ["ep=tile", "ep=fold", "ep=pass", "ep=wsk", "ep=thin", "pad=caller", "pad=image", "pad=copy", "padw=caller", "padd=caller", "A=prep"]


def case_id(case):
    return "x".join(str(v) for v in case[:7]) + ("" if case[7] is None else "-" + case[7])


# ---- the float64 reference and the bound -------------------------------------------------------------------------------------------------------------------
def gather_cols(img, k, s, pt, pl, ho, wo, halo="zero"):
    """im2col of one image [C][H][W]: [(c, p, q)][(i, j)] = img[c][i*s + p - pt][j*s + q - pl], zero outside (halo="wrap": the mutation that reads data there)"""
    c_n, h, w = img.shape
    hp, wp = (ho - 1) * s + k, (wo - 1) * s + k
    hh, ww = min(h, hp - pt), min(w, wp - pl)
    if halo == "wrap":
        pad = np.pad(img[:, :hh, :ww], ((0, 0), (pt, hp - pt - hh), (pl, wp - pl - ww)), mode="wrap")
    else:
        pad = np.zeros((c_n, hp, wp), img.dtype)
        pad[:, pt:pt + hh, pl:pl + ww] = img[:, :hh, :ww]
    cols = np.stack([pad[:, p:p + s * (ho - 1) + 1:s, q:q + s * (wo - 1) + 1:s] for p in range(k) for q in range(k)], axis=1)
    return cols.reshape(c_n * k * k, ho * wo)


def scatter_cols(dcols, c_n, h, w, k, s, pt, pl, ho, wo):
    """the adjoint of gather_cols: [C][H][W] += dcols[(c, p, q)][(i, j)] at (i*s + p - pt, j*s + q - pl)"""
    hp, wp = (ho - 1) * s + k, (wo - 1) * s + k
    pad = np.zeros((c_n, max(hp, pt + h), max(wp, pl + w)), dcols.dtype)
    d = dcols.reshape(c_n, k, k, ho, wo)
    for p in range(k):
        for q in range(k):
            pad[:, p:p + s * (ho - 1) + 1:s, q:q + s * (wo - 1) + 1:s] += d[:, p, q]
    return pad[:, pt:pt + h, pl:pl + w]


def ref_forward(x, kern, k, s):
    """(want, bound) [F][Ho*Wo] of one image: the product and |A| @ |B|"""
    f_n = kern.shape[0]
    ho, wo, pt, pl = same_geometry(x.shape[1], x.shape[2], k, s)
    cols = gather_cols(x.astype(F64), k, s, pt, pl, ho, wo); a = kern.astype(F64).reshape(f_n, -1)
    return a @ cols, np.abs(a) @ np.abs(cols)


def ref_wgrad(x, del_y, k, s, skip_image=None):
    """(want, bound) [F][C*k*k]: summed over the images, a few images per product"""
    batch, c_n, h, w = x.shape; f_n = del_y.shape[1]
    ho, wo, pt, pl = same_geometry(h, w, k, s)
    want = np.zeros((f_n, c_n * k * k)); bound = np.zeros_like(want)
    step = max(1, (1 << 24) // (c_n * k * k * ho * wo))
    for b0 in range(0, batch, step):
        bs = [b for b in range(b0, min(batch, b0 + step)) if b != skip_image]
        if not bs:
            continue
        cols = np.stack([gather_cols(x[b].astype(F64), k, s, pt, pl, ho, wo) for b in bs])      # [b][K][HWo]
        dy = del_y[bs].astype(F64).reshape(len(bs), f_n, ho * wo)
        want += np.tensordot(dy, cols, axes=([0, 2], [0, 2]))
        bound += np.tensordot(np.abs(dy), np.abs(cols, out=cols), axes=([0, 2], [0, 2]))
    return want, bound


def ref_dgrad(del_y, kern, h, w, k, s):
    """(want, bound) [C][H][W] of one image: the adjoint scatter of kern^T . del_y"""
    f_n, c_n = kern.shape[:2]
    ho, wo, pt, pl = same_geometry(h, w, k, s)
    a = kern.astype(F64).reshape(f_n, -1).T; dy = del_y.astype(F64).reshape(f_n, ho * wo)
    return scatter_cols(a @ dy, c_n, h, w, k, s, pt, pl, ho, wo), scatter_cols(np.abs(a) @ np.abs(dy), c_n, h, w, k, s, pt, pl, ho, wo)


def worst(err, bound):
    """the largest err / bound: <= 1 means every element is inside its bound; inf for a NaN or for an error where the bound is zero"""
    err = np.atleast_1d(np.asarray(err, F64)); bound = np.atleast_1d(np.asarray(bound, F64))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isfinite(err) & np.isfinite(bound), r, np.inf)
    return float(r.max())


def fraction(got, want, bound, ep_terms=None):
    """worst fraction of the bound 1e-5 |A||B| (+ 2u (|conv| + |bias| + |add|) behind an epilogue: ep_terms = that sum of magnitudes)"""
    b = 1e-5 * np.asarray(bound, F64)
    if ep_terms is not None:
        b = b + 2 * U * ep_terms
    with np.errstate(invalid="ignore"):
        return worst(np.abs(np.asarray(got, F64).reshape(np.shape(want)) - want), b)


def epilogue_ref(conv, bound, bias, add):
    """out = conv + bias[f], out2 = out + add with their bounds' epilogue terms; conv, bound, add [F][HWo], bias [F] (either may be None)"""
    bz = np.zeros(conv.shape[0]) if bias is None else bias.astype(F64)
    out = conv + bz[:, None]
    t1 = np.abs(conv) + np.abs(bz)[:, None]
    if add is None:
        return out, t1, None, None
    return out, t1, out + add.astype(F64), t1 + np.abs(add.astype(F64))


def sampled_images(batch, hw):
    """first, last and two images whose 128-pixel tiles straddle an image boundary (where the geometry has that; else the second and the middle one)"""
    if batch <= 4:
        return list(range(batch))
    straddle = [b for b in range(1, batch - 1) if (b * hw) % 128]
    mid = straddle if straddle else list(range(1, batch - 1))
    return sorted({0, mid[0], mid[len(mid) // 2], batch - 1})


# ---- inputs: generated once per shape and shared -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def inputs_for(shape):
    batch, h, w, cin, f, k, s = shape
    ho, wo, _, _ = same_geometry(h, w, k, s)
    seed = 7000 + sum(v * p for v, p in zip(shape, (1, 3, 7, 11, 13, 17, 19)))
    I = dict(x=uniform(seed, (batch, cin, h, w), -1, 1, F32), kern=uniform(seed + 1, (f, cin, k, k), -0.3, 0.3, F32), del_y=uniform(seed + 2, (batch, f, ho, wo), -1, 1, F32),
             bias=uniform(seed + 3, (batch, f + 3), -1, 1, F32), add=uniform(seed + 4, (batch, f, ho, wo), -1, 1, F32))
    for a in I.values():
        a.setflags(write=False)
    return I


# ---- numpy float32 restatement of a tiled product --------------------------------------------------------------------------------------------------------------
def restate_product(a, cols, splits, skip_split=None):
    """C = A . cols in fp32: K cut into `splits` runs of whole 16-deep slabs (the last may be short), a run accumulated slab by slab, the runs summed in order"""
    K = a.shape[1]
    per = cdiv(cdiv(K, 16), splits) * 16
    total = np.zeros((a.shape[0], cols.shape[1]), F32)
    for z in range(cdiv(K, per)):
        if z == skip_split:
            continue
        acc = np.zeros_like(total)
        for k0 in range(z * per, min(K, (z + 1) * per), 16):
            acc = acc + a[:, k0:k0 + 16] @ cols[k0:k0 + 16]
        total = total + acc
    assert total.dtype == F32
    return total


def restate_forward(I, shape, b, splits, bias_stride=0, with_add=False, drop_tap=None, skip_split=None, halo="zero", bias_image=None, drop_add=False):
    """one image of the forward pass with the epilogue last; the keyword arguments are the mutations"""
    batch, h, w, cin, f, k, s = shape
    ho, wo, pt, pl = same_geometry(h, w, k, s)
    cols = gather_cols(I["x"][b], k, s, pt, pl, ho, wo, halo); a = I["kern"].reshape(f, -1).copy()
    if drop_tap is not None:
        a[:, drop_tap] = 0
    out = restate_product(a, cols, splits, skip_split)
    if bias_stride:
        out = out + I["bias"][b if bias_image is None else bias_image, :f][:, None]
    out2 = None
    if with_add:
        out2 = out if drop_add else out + I["add"][b].reshape(f, -1)
    return out, out2


def restate_wgrad(I, shape, splits, skip_image=None):
    """per image a product over its pixels, the images summed in order"""
    batch, h, w, cin, f, k, s = shape
    ho, wo, pt, pl = same_geometry(h, w, k, s)
    total = np.zeros((f, cin * k * k), F32)
    for b in range(batch):
        if b != skip_image:
            total = total + restate_product(I["del_y"][b].reshape(f, -1), np.ascontiguousarray(gather_cols(I["x"][b], k, s, pt, pl, ho, wo).T), splits)
    return total


def restate_dgrad(I, shape, b, splits, flip=True):
    """the library's formulation: the stride-1 convolution of the zero-dilated del_y with the kernels transposed and flipped, pads mirrored"""
    batch, h, w, cin, f, k, s = shape
    ho, wo, pt, pl = same_geometry(h, w, k, s)
    dil = np.zeros((f, (ho - 1) * s + 1, (wo - 1) * s + 1), F32); dil[:, ::s, ::s] = I["del_y"][b]
    kt = I["kern"].transpose(1, 0, 2, 3)
    kt = kt[:, :, ::-1, ::-1] if flip else kt
    cols = gather_cols(dil, k, 1, k - 1 - pt, k - 1 - pl, h, w)
    return restate_product(np.ascontiguousarray(kt).reshape(cin, -1), cols, splits)


HOST_SHAPES = [((4, 8, 8, 32, 32, 3, 1), 3), ((3, 12, 12, 16, 32, 3, 1), 1), ((4, 8, 8, 32, 16, 3, 2), 2), ((3, 8, 8, 16, 32, 2, 1), 2)]      # (shape, K splits)


@pytest.mark.parametrize("shape,splits", HOST_SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_restatement_stays_inside_the_bound(shape, splits):
    batch, h, w, cin, f, k, s = shape; I = inputs_for(shape)
    for b in range(batch):
        conv, bound = ref_forward(I["x"][b], I["kern"], k, s)
        out, out2 = restate_forward(I, shape, b, splits)
        assert fraction(out, conv, bound) <= 1
        out, out2 = restate_forward(I, shape, b, splits, bias_stride=f + 3, with_add=True)
        w1, t1, w2, t2 = epilogue_ref(conv, bound, I["bias"][b, :f], I["add"][b].reshape(f, -1))
        assert fraction(out, w1, bound, t1) <= 1 and fraction(out2, w2, bound, t2) <= 1
        want, bound = ref_dgrad(I["del_y"][b], I["kern"], h, w, k, s)
        assert fraction(restate_dgrad(I, shape, b, splits), want.reshape(cin, -1), bound.reshape(cin, -1)) <= 1
    want, bound = ref_wgrad(I["x"], I["del_y"], k, s)
    assert fraction(restate_wgrad(I, shape, splits), want, bound) <= 1


@pytest.mark.parametrize("shape,splits", HOST_SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_mutations_leave_the_bound(shape, splits):
    """What a subtly wrong kernel would return is outside the bound: one tap dropped, one split's slab left out of the fold, the halo read as data, one
    image left out of the weight-gradient sum, the bias of image b - 1 applied to image b, the addend dropped, the kernel not flipped in the data gradient."""
    batch, h, w, cin, f, k, s = shape; I = inputs_for(shape)
    b = batch - 1
    conv, bound = ref_forward(I["x"][b], I["kern"], k, s)
    w1, t1, w2, t2 = epilogue_ref(conv, bound, I["bias"][b, :f], I["add"][b].reshape(f, -1))
    assert fraction(restate_forward(I, shape, b, splits, drop_tap=k * k * cin // 2)[0], conv, bound) > 1
    if splits > 1:
        assert fraction(restate_forward(I, shape, b, splits, skip_split=splits - 1)[0], conv, bound) > 1
    assert fraction(restate_forward(I, shape, b, splits, halo="wrap")[0], conv, bound) > 1
    out, out2 = restate_forward(I, shape, b, splits, bias_stride=f + 3, with_add=True, bias_image=b - 1)
    assert fraction(out, w1, bound, t1) > 1 and fraction(out2, w2, bound, t2) > 1
    out, out2 = restate_forward(I, shape, b, splits, bias_stride=f + 3, with_add=True, drop_add=True)
    assert fraction(out, w1, bound, t1) <= 1 and fraction(out2, w2, bound, t2) > 1
    want, bound = ref_wgrad(I["x"], I["del_y"], k, s)
    assert fraction(restate_wgrad(I, shape, splits, skip_image=1), want, bound) > 1
    want, bound = ref_dgrad(I["del_y"][b], I["kern"], h, w, k, s)
    assert fraction(restate_dgrad(I, shape, b, splits, flip=False), want.reshape(cin, -1), bound.reshape(cin, -1)) > 1


def test_reference_against_the_oracle(ora):
    """this file's float64 reference against the oracle's conv() / conv_ddx() restatement (and its adjoint col2im at stride 2) on the two smallest cases"""
    for shape in ((1, 4, 4, 5, 5, 1, 2), (1, 5, 5, 5, 5, 2, 1)):
        batch, h, w, cin, f, k, s = shape; I = inputs_for(shape)
        x, kern, dy = I["x"][0].astype(F64), I["kern"].astype(F64), I["del_y"][0].astype(F64)
        ho, wo, _, _ = same_geometry(h, w, k, s)
        assert (ho, wo) == ora.out_hw(h, w, s)
        fw = ora.conv_intended(x, kern, s)
        want, _ = ref_forward(I["x"][0], I["kern"], k, s)
        assert np.allclose(want, fw["output"].reshape(f, -1), rtol=1e-12, atol=1e-14)
        dq = ora.reshape_matrix_channels(dy)
        want, _ = ref_wgrad(I["x"], I["del_y"], k, s)
        assert np.allclose(want.reshape(f, cin, k, k), ora.matrix_to_kernels(ora.matmul(ora.transpose(fw["im2col"]), dq), cin, k), rtol=1e-12, atol=1e-14)
        want, _ = ref_dgrad(I["del_y"][0], I["kern"], h, w, k, s)
        assert np.allclose(want, ora.col2im_adjoint(dq @ fw["kmat"].T, cin, h, w, k, s), rtol=1e-12, atol=1e-14)


# ---- host tests of the table ---------------------------------------------------------------------------------------------------------------------------------
def test_table_states_the_restated_plan():
    """the table's entries are what plan_of gives at 256 CUs (on the device the library's own record is the arbiter of both)"""
    for case, want in CASES.items():
        assert plan_of(case, CUS) == want, case
    for case, want in FORMS.items():
        assert forms_plans(case, CUS) == want, case


def test_table_reaches_the_checklist():
    reached = set()
    for want in CASES.values():
        reached |= set(kinds(want[0]) + kinds(want[1]))
    assert reached == set(CHECKLIST), set(CHECKLIST) ^ reached
    assert not set(CHECKLIST) & ELSEWHERE
    attrs = set()
    for want in FORMS.values():
        attrs |= set(re.findall(r"(?:ep|pad|padw|padd|A)=\w+", " ".join(want)))
    assert set(ATTRIBUTES) <= attrs, set(ATTRIBUTES) - attrs
    # the shapes the table is there for: window channel groups 1, 2, 3 and 16; ragged last splits 3, 7, 8, 9; every shift on the three alignment shapes
    assert {c[3] // 16 for c, p in CASES.items() if p[0].startswith("fwd:m7")} >= {1, 2, 3, 16}
    assert {int(m) for p in CASES.values() for m in re.findall(r"fwd:m3hs/s(\d+)", p[0])} >= {1, 3, 7, 8, 9}
    for shape in ((5, 16, 16, 32, 24, 3, 1), (32, 8, 8, 128, 128, 3, 1), (32, 32, 32, 48, 256, 3, 1)):
        assert {c[7] for c in CASES if c[:7] == shape} == {None, "x", "kern", "out", "del_y", "del_kern", "del_x"}


def test_no_reachable_path_is_missing_from_the_checklist():
    """a sweep over batch sizes, maps, channel counts, kernel sizes, strides and the two shifts that change a plan: every path it finds is on the checklist"""
    known = set(CHECKLIST) | ELSEWHERE
    for batch, (h, w), cin, f, k, s, shift in itertools.product((1, 2, 5, 16, 32, 64, 104, 128), ((4, 4), (8, 8), (16, 16), (32, 32), (16, 10), (12, 12), (9, 32), (20, 20), (7, 9), (17, 17)),
                                                                (3, 5, 16, 32, 48, 72, 128, 192, 256), (3, 6, 24, 64, 128, 256), (1, 2, 3, 4), (1, 2), (None, "kern", "del_y")):
        fwd, bwd = plan_of((batch, h, w, cin, f, k, s, shift), CUS)
        assert set(kinds(fwd) + kinds(bwd)) <= known, ((batch, h, w, cin, f, k, s, shift), fwd, bwd)


# ---- on the device -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev(pkg):
    pkg.init(0)
    return pkg


def device_cus(dev):
    buf = C.create_string_buffer(256)
    dev.native.check(dev.lib().bla_device_name(buf, 256))
    return int(re.search(r"\((\d+) CUs\)", buf.value.decode()).group(1))


class View:
    """A tensor inside a larger allocation pre-filled with 0xFF bytes: GUARD floats before and after it (and one more in front when `shifted`, which moves
    the pointer one float off its 16-byte alignment).  numpy() returns the tensor after checking that every guard byte is still 0xFF."""

    def __init__(self, dev, shape, init=None, shifted=False):
        self.shape = tuple(int(v) for v in np.atleast_1d(shape)); self.n = int(np.prod(self.shape))
        self.lead = GUARD + (1 if shifted else 0)
        total = self.lead + self.n + GUARD
        if init is None:
            self.base = dev.empty((total,)).fill_bytes(0xFF)
        else:
            host = np.full(total * 4, 0xFF, np.uint8).view(F32)
            host[self.lead:self.lead + self.n] = np.asarray(init, F32).ravel()
            self.base = dev.to_device(host)
        self.ptr = self.base.ptr + self.lead * 4
        assert self.ptr % 16 == (4 if shifted else 0)

    def numpy(self):
        a = self.base.numpy(); raw = a.view(np.uint8)
        assert (raw[:self.lead * 4] == 0xFF).all() and (raw[(self.lead + self.n) * 4:] == 0xFF).all(), "a guard element was written"
        return a[self.lead:self.lead + self.n].reshape(self.shape).copy()


def last_plan(dev):
    return dev.lib().bla_conv_last_plan().decode()


def padded_copy(dev, a, h, w, k):
    """[planes][H][W] inside bla_conv_padded_layout: zero halo, row pitch wh (None: this geometry has no such copy)"""
    v = [C.c_int() for _ in range(5)]
    dev.native.check(dev.lib().bla_conv_padded_layout(h, w, k, 1, *[C.byref(i) for i in v]))
    lw, wh, plane, pt, pl = [i.value for i in v]
    if plane == 0:
        return None
    assert lw == w and plane % wh == 0
    planes = a.reshape(-1, h, w)
    out = np.zeros((planes.shape[0], plane // wh, wh), F32)
    out[:, pt:pt + h, pl:pl + w] = planes
    return out


class Operands:
    """the device inputs of one case, uploaded once and shared by its runs"""

    def __init__(self, dev, case):
        batch, h, w, cin, f, k, s, shift = case
        self.case, self.I = case, inputs_for(case[:7])
        self.ho, self.wo, _, _ = same_geometry(h, w, k, s)
        I = self.I
        self.x, self.kern, self.del_y = View(dev, I["x"].shape, I["x"], shift == "x"), View(dev, I["kern"].shape, I["kern"], shift == "kern"), View(dev, I["del_y"].shape, I["del_y"], shift == "del_y")
        self.bias = self.add = self.x_padded = self.dy_padded = None
        self.prepared = {}

    def with_epilogue(self, dev):
        self.bias, self.add = View(dev, self.I["bias"].shape, self.I["bias"]), View(dev, self.I["add"].shape, self.I["add"])

    def with_padded(self, dev):
        batch, h, w, cin, f, k, s, _ = self.case
        px = padded_copy(dev, self.I["x"], h, w, k) if s == 1 else None
        py = padded_copy(dev, self.I["del_y"], h, w, k) if s == 1 else None
        self.x_padded = None if px is None else View(dev, px.shape, px)
        self.dy_padded = None if py is None else View(dev, py.shape, py)
        return self.x_padded is not None

    def prepare(self, dev, data_gradient):
        """the kernel matrix in the form bla_conv_prep_mode names (None: the product takes none), made by bla_conv_prepare_kernels_f32"""
        batch, h, w, cin, f, k, s, _ = self.case
        mode = dev.lib().bla_conv_prep_mode(batch, h, w, k, cin, f, s, int(data_gradient))
        if mode == 0:
            return 0, None
        dst = View(dev, (f * cin * k * k,))
        dev.native.check(dev.lib().bla_conv_prepare_kernels_f32(None, self.kern.ptr, dst.ptr, f, cin, k, mode))
        assert np.array_equal(dst.numpy().view(np.uint32), prepared_ref(self.I["kern"], mode).ravel().view(np.uint32)), (self.case, mode)
        return mode, dst


def prepared_ref(kern, mode):
    """conv_prepare_kernels in numpy: 1 = [F][(g, t, c16)], 2 = [C][(g, t, f16)] flipped, 3 = [C][F][k*k] flipped"""
    f, c, k, _ = kern.shape; kk = k * k
    if mode == 1:
        return kern.reshape(f, c // 16, 16, kk).transpose(0, 1, 3, 2)
    flipped = kern.reshape(f, c, kk)[:, :, ::-1]
    if mode == 3:
        return flipped.transpose(1, 0, 2)
    return flipped.reshape(f // 16, 16, c, kk).transpose(2, 0, 3, 1)


def run_forward(dev, ops, ep=(False, False), x_padded=False, prepared=None, read=True):
    """bla_conv2d_forward_fused_f32 -> (out, out2 or None, the plan)"""
    batch, h, w, cin, f, k, s, shift = ops.case
    out = View(dev, (batch, f, ops.ho * ops.wo), None, shift == "out")
    out2 = View(dev, out.shape) if ep[1] else None
    st = dev.lib().bla_conv2d_forward_fused_f32(None, ops.x.ptr, ops.kern.ptr, out.ptr, batch, h, w, k, cin, f, s, ops.bias.ptr if ep[0] else None, f + 3 if ep[0] else 0,
                                                ops.add.ptr if ep[1] else None, out2.ptr if ep[1] else None, ops.x_padded.ptr if x_padded else None,
                                                prepared.ptr if prepared is not None else None)
    dev.native.check(st)
    if not read:
        return None
    return out.numpy(), (out2.numpy() if ep[1] else None), last_plan(dev)


def run_backward(dev, ops, x_padded=False, dy_padded=False, prepared=None, read=True):
    """bla_conv2d_backward_prepared_f32 -> (del_kern, del_x, the plan); the scratch of F*C*k*k floats is guarded like the outputs"""
    batch, h, w, cin, f, k, s, shift = ops.case
    dk, dx, scratch = View(dev, (f, cin * k * k), None, shift == "del_kern"), View(dev, (batch, cin, h * w), None, shift == "del_x"), View(dev, (f * cin * k * k,))
    st = dev.lib().bla_conv2d_backward_prepared_f32(None, ops.del_y.ptr, ops.x.ptr, ops.kern.ptr, dk.ptr, dx.ptr, scratch.ptr, batch, h, w, k, cin, f, s,
                                                    ops.x_padded.ptr if x_padded else None, prepared.ptr if prepared is not None else None,
                                                    ops.dy_padded.ptr if dy_padded else None)
    dev.native.check(st)
    if not read:
        return None
    scratch.numpy()
    return dk.numpy(), dx.numpy(), last_plan(dev)


FRACTIONS = {}      # (path kind, quantity) -> worst fraction of its bound seen in this run


def record(plan, value, tag):
    """print each figure before it is asserted; keep the worst per path"""
    for kind in kinds(plan):
        FRACTIONS[kind] = max(FRACTIONS.get(kind, 0.0), value)
        print(f"conv bound fraction | {kind} | {value:.3f} | worst so far {FRACTIONS[kind]:.3f} | {tag}")
    assert value <= 1, (plan, value, tag)


def same_bits(a, b):
    return a is b or (a is not None and b is not None and np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def check_forward(ops, out, out2, plan, ep, tag):
    batch, h, w, cin, f, k, s, _ = ops.case; I = ops.I
    assert np.isfinite(out).all() and (out2 is None or np.isfinite(out2).all()), tag
    worst_f = 0.0
    for b in sampled_images(batch, ops.ho * ops.wo):
        conv, bound = ref_forward(I["x"][b], I["kern"], k, s)
        w1, t1, w2, t2 = epilogue_ref(conv, bound, I["bias"][b, :f] if ep[0] else None, I["add"][b].reshape(f, -1) if ep[1] else None)
        worst_f = max(worst_f, fraction(out[b], w1, bound, t1 if ep[0] else None))
        if ep[1]:
            worst_f = max(worst_f, fraction(out2[b], w2, bound, t2))
    record(plan, worst_f, tag)


def check_backward(ops, dk, dx, plan, tag):
    batch, h, w, cin, f, k, s, _ = ops.case; I = ops.I
    assert np.isfinite(dx).all(), tag
    want, bound = wgrad_reference(ops.case[:7])
    fw = fraction(dk, want, bound)
    fd = max(fraction(dx[b], *[a.reshape(cin, -1) for a in ref_dgrad(I["del_y"][b], I["kern"], h, w, k, s)]) for b in sampled_images(batch, h * w))
    toks = plan.split()
    record(toks[0], fw, (tag, "weight gradient"))
    record(toks[-1], fd, (tag, "data gradient"))


@functools.lru_cache(maxsize=2)
def wgrad_reference(shape):
    I = inputs_for(shape)
    return ref_wgrad(I["x"], I["del_y"], shape[5], shape[6])


INTERLOPER = {}


def interloper(dev, case):
    """the largest case of the table (for that case itself the largest other window case), forward and backward: it grows the workspace past what `case`
    asked for, or -- the workspace only grows -- at least overwrites what `case` left in it"""
    big = (128, 16, 16, 256, 256, 3, 1, None)
    other = (128, 16, 16, 32, 256, 3, 1, None) if case[:7] == big[:7] else big
    if other not in INTERLOPER:
        INTERLOPER.clear()
        INTERLOPER[other] = Operands(dev, other)
    run_forward(dev, INTERLOPER[other], read=False); run_backward(dev, INTERLOPER[other], read=False)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES), ids=case_id)
def test_every_planned_path(dev, case):
    """table == plan_of at this device's CU count (the table itself where that is 256) == bla_conv_last_plan(); every element inside its bound; guards intact;
    the second run, behind another case's, returns the same bits"""
    cus = device_cus(dev)
    want = plan_of(case, cus)
    if cus == CUS:
        assert want == CASES[case], (case, want)
    ops = Operands(dev, case)
    if case[7] == "out" and "ep=fold" in plan_of(case, cus, ep=True)[0]:
        # a shifted output behind a fused fold: the 16-byte fold refuses it cleanly (BLA_ERR_INVALID) and writes nothing
        ops.with_epilogue(dev)
        with pytest.raises(dev.BlaError) as e:
            run_forward(dev, ops, ep=(True, True))
        assert e.value.status == BLA_ERR_INVALID and "unaligned convolution output" in str(e.value), e.value
    out, _, pf = run_forward(dev, ops)
    dk, dx, pb = run_backward(dev, ops)
    print(f"conv plan | {case_id(case)} | {pf} | {pb}")
    assert (pf, pb) == want, (case, (pf, pb), want)
    interloper(dev, case)
    out_b, _, pf_b = run_forward(dev, ops)
    dk_b, dx_b, pb_b = run_backward(dev, ops)
    assert (pf_b, pb_b) == (pf, pb)
    assert same_bits(out, out_b) and same_bits(dk, dk_b) and same_bits(dx, dx_b), (case, "not bit-reproducible behind another case")
    check_forward(ops, out, None, pf, (False, False), case_id(case))
    check_backward(ops, dk, dx, pb, case_id(case))


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(FORMS), ids=case_id)
def test_operand_forms(dev, case):
    """The forms the U-Net passes internally, through the entry points that expose them: the fused epilogue (bias only with bias_stride > F; add and second
    output only; both) at whichever site the plan names, the caller's padded copies of x and del_y, and the prepared kernel matrices -- made by
    bla_conv_prepare_kernels_f32 in the mode bla_conv_prep_mode names, bit-exact against numpy, and bit-identical in effect to the call without them."""
    cus = device_cus(dev)
    ops = Operands(dev, case); ops.with_epilogue(dev)
    plain_out, _, plain_pf = run_forward(dev, ops)
    for ep in ((True, False), (False, True), (True, True)):
        out, out2, pf = run_forward(dev, ops, ep=ep)
        assert pf == plan_of(case, cus, ep=True)[0], (case, ep, pf)
        check_forward(ops, out, out2, pf, ep, (case_id(case), "bias" if ep[0] else "-", "add" if ep[1] else "-"))
    plain_dk, plain_dx, plain_pb = run_backward(dev, ops)
    got = [plan_of(case, cus, ep=True)[0]]
    assert ops.with_padded(dev) == (case[6] == 1 and case[2] % 4 == 0)
    if ops.x_padded is not None:
        out, _, pf = run_forward(dev, ops, x_padded=True)
        dk, dx, pb = run_backward(dev, ops, x_padded=True, dy_padded=True)
        assert (pf, pb) == plan_of(case, cus, x_padded=True, dy_padded=True), (case, pf, pb)
        check_forward(ops, out, None, pf, (False, False), (case_id(case), "x_padded"))
        check_backward(ops, dk, dx, pb, (case_id(case), "x_padded, dy_padded"))
        got += [pf, pb]
    mode_f, prep_f = ops.prepare(dev, False)
    mode_b, prep_b = ops.prepare(dev, True)
    print(f"conv prepared modes | {case_id(case)} | forward {mode_f} | data gradient {mode_b}")
    assert (mode_f, mode_b) == (prep_mode_of(case, cus, False), prep_mode_of(case, cus, True)), case
    if mode_f:
        out, _, pf = run_forward(dev, ops, prepared=prep_f)
        assert pf == plan_of(case, cus, prepared_fwd=True)[0] and same_bits(out, plain_out), (case, pf)
        got.append(pf)
    if mode_b:
        dk, dx, pb = run_backward(dev, ops, prepared=prep_b)
        assert pb == plan_of(case, cus, prepared_bwd=True)[1] and same_bits(dk, plain_dk) and same_bits(dx, plain_dx), (case, pb)
        got.append(pb)
    assert tuple(got) == forms_plans(case, cus), (case, got)
    if cus == CUS:
        assert tuple(got) == FORMS[case], (case, got)


PREPARE = [(32, 48, 3, 1), (32, 48, 3, 2), (32, 48, 3, 3),        # mode 1 permutes inside a row; modes 2 and 3 through the 16 x 16 LDS tile
           (32, 72, 3, 2), (24, 72, 3, 3), (24, 48, 3, 1),        # c_n = 72 / f_n = 24: element by element
           (32, 48, 1, 3), (20, 72, 1, 3), (16, 16, 2, 3)]        # 1x1 and 2x2 kernels


@pytest.mark.gpu
@pytest.mark.parametrize("f,c,k,mode", PREPARE, ids=lambda v: str(v))
def test_prepare_kernels_bit_exact(dev, f, c, k, mode):
    kern = uniform(7900 + f + c + k + mode, (f, c, k, k), -1, 1, F32)
    src, dst = View(dev, kern.shape, kern), View(dev, (f * c * k * k,))
    dev.native.check(dev.lib().bla_conv_prepare_kernels_f32(None, src.ptr, dst.ptr, f, c, k, mode))
    assert np.array_equal(dst.numpy().view(np.uint32), np.ascontiguousarray(prepared_ref(kern, mode)).ravel().view(np.uint32))
    assert np.array_equal(src.numpy(), kern)
