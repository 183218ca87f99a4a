"""The implicit bf16 weight gradient, restated on the host with numpy alone: no GPU, nothing imported from another test file.

(a) The LDS maps of bf16_tile_product_kmajor, emulated on a 16 KiB byte array:
    * the DMA placement (wave w, piece i, lane l -> row 4 (4w + i) + (l >> 4), slot l & 15, source chunk slot ^ x(row)) stores every (k-row, chunk) of a
      [64][128] slab exactly once, and a lane's source chunk per piece does not depend on anything but (l, i);
    * the transposed read ds_read_b64_tr_b16, by its definition (a group of 16 lanes reads 4 rows x 16 columns; lane 4q + p addresses row q, columns
      4p .. 4p+3; lane i receives column i, row q in element q), applied to the fragment addresses, delivers to every lane, block, k-step and read exactly
      X[k = 16 s + 8 (L >> 5) + 4 t + e][block column + (L & 31)]; the closed form the header precomputes equals off(r0 + q, c0 + (p >> 1)) + 8 (p & 1);
    * every address is 8-byte aligned;
    * bank conflicts per 32-lane half by the rule bank = (a / 4) % 64 are counted and printed: 0 (lanes that read the same dword are one access).
(b) The kernel's pixel walk: the incremental (i, j, Q offset, P offset) steps with their carries equal the direct index maps for every k-row of every slab,
    in uint32 arithmetic, from any split's first slab.
(c) A float32 restatement of the whole entry -- index maps into the flat padded copies, the partition, slab-by-slab float32 accumulation, the ascending
    fold, the (tap, c) -> [c][p][q] permutation -- stays inside
        |got - ref| <= (N + 8) 2^-23 (|del_y| * |x|) + 2 2^-24 |ref|
    against float64, and leaves it under each mutation: Q's dilation ignored, top off by one, taps run (q, p), the last short slab dropped, a slab counted
    by two neighbouring splits, a fold that does not permute.  Operands lie in [0.5, 1): every term is at least 1/4, the bound is far
    below that, so a dropped, doubled or misplaced term exceeds it by construction.
"""
import numpy as np
import pytest

F32, F64, U16, U32 = np.float32, np.float64, np.uint16, np.uint32
BK = 64


# ---- (a) the LDS image ------------------------------------------------------------------------------------------------------------------------------------
def xor_of(row):
    return ((row & 3) << 2) | ((row >> 2) & 3)


def off(row, ch):
    return 256 * row + 16 * (ch ^ xor_of(row))


def staged_slab():
    """X [64][128] of distinct 16-bit values, staged by the DMA placement -> (X, the LDS image as 8192 uint16)"""
    X = (np.arange(64 * 128, dtype=np.int64).reshape(64, 128) + 1).astype(U16)
    lds = np.zeros(8192, U16)
    written = np.zeros(1024, np.int64)        # per 16-byte slot of the image
    fetched = np.zeros((64, 16), np.int64)    # per (k-row, source chunk)
    for w in range(4):
        for i in range(4):
            for l in range(64):
                pc = 4 * w + i
                r, slot = 4 * pc + (l >> 4), l & 15
                chunk = slot ^ xor_of(r)
                assert chunk == (l & 15) ^ (((l >> 4) << 2) | i), "the lane's column chunk per piece is not a loop constant"
                a = pc * 1024 + 16 * l        # lane-linear DMA
                assert a == 256 * r + 16 * slot == off(r, chunk)
                lds[a // 2:a // 2 + 8] = X[r, 8 * chunk:8 * chunk + 8]
                written[a // 16] += 1
                fetched[r, chunk] += 1
    assert (written == 1).all() and (fetched == 1).all()
    return X, lds


def fragment_address(L, first_col, s, t):
    r0 = 16 * s + 8 * (L >> 5) + 4 * t
    c0 = (first_col >> 3) + 2 * ((L >> 4) & 1)
    q, p = (L & 15) >> 2, L & 3
    return off(r0 + q, c0 + (p >> 1)) + 8 * (p & 1)


def header_address(L, wave_block, i, s, t):
    """the closed form of bla_bf16_tile.h: wave_block = the wave's 64-column half (wm or wn), i = its 32-column block"""
    fh, g16, q, p = L >> 5, (L >> 4) & 1, (L & 15) >> 2, L & 3
    row, x = 8 * fh + 4 * t + q, (q << 2) | (2 * fh + t)
    return 256 * row + 16 * ((wave_block * 8 + i * 4 + 2 * g16 + (p >> 1)) ^ x) + 8 * (p & 1) + 4096 * s


def transposed_read(lds, addr):
    """addr[64] byte addresses -> out[64][4], by the instruction's definition"""
    out = np.zeros((64, 4), U16)
    for g in range(4):
        block = np.zeros((4, 16), U16)
        for q in range(4):
            for p in range(4):
                a = addr[16 * g + 4 * q + p]
                block[q, 4 * p:4 * p + 4] = lds[a // 2:a // 2 + 4]
        for i in range(16):
            out[16 * g + i] = block[:, i]
    return out


def test_dma_placement_and_transposed_fragments():
    X, lds = staged_slab()
    conflicts = 0
    for blk in range(4):                      # the four 32-column blocks of a slab: (wave half, i) = (blk >> 1, blk & 1)
        for s in range(4):
            for t in range(2):
                addr = [fragment_address(L, 32 * blk, s, t) for L in range(64)]
                assert addr == [header_address(L, blk >> 1, blk & 1, s, t) for L in range(64)]
                assert all(a % 8 == 0 and 0 <= a <= 16384 - 8 for a in addr)
                got = transposed_read(lds, addr)
                for L in range(64):
                    k0 = 16 * s + 8 * (L >> 5) + 4 * t
                    assert (got[L] == X[k0:k0 + 4, 32 * blk + (L & 31)]).all(), (blk, s, t, L)
                for half in range(2):
                    banks = {}
                    for a in addr[32 * half:32 * half + 32]:
                        for dw in (a // 4, a // 4 + 1):
                            banks.setdefault(dw % 64, set()).add(dw)
                    conflicts += sum(len(v) - 1 for v in banks.values())
    print("ds_read_b64_tr_b16 on image (b): %d bank conflicts over 4 blocks x 4 k-steps x 2 reads x 2 halves" % conflicts)
    assert conflicts == 0


# ---- geometry, restated -------------------------------------------------------------------------------------------------------------------------------------
def same_geometry(h, w, k, s):
    ho, wo = int(np.ceil(F32(h) / F32(s))), int(np.ceil(F32(w) / F32(s)))
    vpad, hpad = max((ho - 1) * s + k - h, 0), max((wo - 1) * s + k - w, 0)
    return ho, wo, vpad // 2, hpad // 2, vpad, hpad


def round8(x):
    return -(-x // 8) * 8


def layouts(h, w, k, s):
    ho, wo, pt, pl, vpad, hpad = same_geometry(h, w, k, s)
    fwd = dict(hp=h + vpad, wp=w + hpad, top=pt, left=pl)
    dg = dict(hq=h + k - 1, wq=w + k - 1, top=k - 1 - pt, left=k - 1 - pl, d=s)
    return ho, wo, fwd, dg


def partition(n, splits):
    slabs = -(-n // BK)
    s = min(max(splits, 1), slabs)
    sps = -(-slabs // s)
    return -(-slabs // sps), sps


# ---- (b) the pixel walk -------------------------------------------------------------------------------------------------------------------------------------
WALKS = [(2, 9, 9, 3, 1), (3, 10, 10, 3, 2), (70, 1, 1, 1, 1), (5, 3, 1, 3, 1), (2, 6, 6, 4, 2), (1, 40, 3, 5, 1), (9, 7, 5, 3, 2), (1, 3, 70, 3, 1)]


@pytest.mark.parametrize("B,h,w,k,s", WALKS)
def test_incremental_pixel_offsets_equal_the_direct_maps(B, h, w, k, s):
    ho, wo, fwd, dg = layouts(h, w, k, s)
    fp, cp, N = 16, 8, B * ho * wo
    M = 1 << 32
    db, rest = BK // (ho * wo), BK % (ho * wo)
    di, dj = rest // wo, rest % wo
    q_step = ((db * dg["hq"] + di * dg["d"]) * dg["wq"] + dj * dg["d"]) * fp
    q_cj, q_ci = (dg["wq"] - wo) * dg["d"] * fp, (dg["hq"] - ho * dg["d"]) * dg["wq"] * fp
    p_step = ((db * fwd["hp"] + di * s) * fwd["wp"] + dj * s) * cp
    p_cj, p_ci = (fwd["wp"] - wo) * s * cp, (fwd["hp"] - ho * s) * fwd["wp"] * cp

    def direct(n):
        b, pix = divmod(n, ho * wo)
        i, j = divmod(pix, wo)
        return i, j, ((b * dg["hq"] + dg["top"] + i * dg["d"]) * dg["wq"] + dg["left"] + j * dg["d"]) * fp, ((b * fwd["hp"] + i * s) * fwd["wp"] + j * s) * cp

    for first_slab in (0, 1):
        for row in range(BK):                 # every (wave, piece, lane >> 4) of a slab
            n = first_slab * BK + row
            i, j, oq, op = direct(n)
            while n < N:
                assert (i, j, oq % M, op % M) == direct(n)[:2] + tuple(v % M for v in direct(n)[2:]), (n, row)
                j += dj
                cj = j >= wo
                j -= wo if cj else 0
                i += di + (1 if cj else 0)
                ci = i >= ho
                i -= ho if ci else 0
                oq = (oq + q_step + (q_cj if cj else 0) + (q_ci if ci else 0)) % M
                op = (op + p_step + (p_cj if cj else 0) + (p_ci if ci else 0)) % M
                n += BK


# ---- (c) the float32 restatement -----------------------------------------------------------------------------------------------------------------------------
def to_bf16_values(a):
    u = a.astype(F32).view(U32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(U32).view(F32)


def reference(x, dy, k, s):
    """float64 del_kern [F][C][k][k] and the same on magnitudes, by an im2col of its own"""
    B, Cn, h, w = x.shape
    ho, wo, pt, pl = same_geometry(h, w, k, s)[:4]
    xp = np.zeros((B, Cn, h + 2 * k + s, w + 2 * k + s), F64)
    xp[:, :, pt:pt + h, pl:pl + w] = x
    out, mag = np.zeros((dy.shape[1], Cn, k, k)), np.zeros((dy.shape[1], Cn, k, k))
    for p in range(k):
        for q in range(k):
            win = xp[:, :, p:p + (ho - 1) * s + 1:s, q:q + (wo - 1) * s + 1:s]
            out[:, :, p, q] = np.einsum("bfij,bcij->fc", dy.astype(F64), win)
            mag[:, :, p, q] = np.einsum("bfij,bcij->fc", np.abs(dy).astype(F64), np.abs(win))
    return out, mag


def restated(x, dy, k, s, splits, mutate=None):
    """what the entry computes, in float32, through the FLAT padded copies and the kernel's index maps"""
    B, Cn, h, w = x.shape
    Fn = dy.shape[1]
    ho, wo, fwd, dg = layouts(h, w, k, s)
    cp, fp, N = round8(Cn), round8(Fn), B * ho * wo
    hp, wp, hq, wq = fwd["hp"], fwd["wp"], dg["hq"], dg["wq"]
    P = np.zeros((B, hp, wp, cp), F32)
    P[:, fwd["top"]:fwd["top"] + h, fwd["left"]:fwd["left"] + w, :Cn] = x.transpose(0, 2, 3, 1)
    Q = np.zeros((B, hq, wq, fp), F32)
    Q[:, dg["top"]:dg["top"] + (ho - 1) * dg["d"] + 1:dg["d"], dg["left"]:dg["left"] + (wo - 1) * dg["d"] + 1:dg["d"], :Fn] = dy.transpose(0, 2, 3, 1)
    P, Q = P.reshape(-1), Q.reshape(-1)
    d = 1 if mutate == "dilation" else dg["d"]
    top = dg["top"] + (1 if mutate == "top" else 0)
    n = np.arange(N)
    b, pix = n // (ho * wo), n % (ho * wo)
    i, j = pix // wo, pix % wo
    a_rows = Q[(((b * hq + top + i * d) * wq + dg["left"] + j * d) * fp)[:, None] + np.arange(fp)[None, :]]                      # [N][Fp]
    col = np.arange(k * k * cp)
    tap, c = col // cp, col % cp
    tp, tq = (tap % k, tap // k) if mutate == "taps" else (tap // k, tap % k)
    b_rows = P[(((b * hp + i * s) * wp + j * s) * cp)[:, None] + ((tp * wp + tq) * cp + c)[None, :]]                                 # [N][k k Cp]
    eff, sps = partition(N, splits)
    slabs = -(-N // BK)
    partial = np.zeros((eff, fp, k * k * cp), F32)
    for sp in range(eff):
        first, last = sp * sps, min(slabs, (sp + 1) * sps)
        if mutate == "shared" and sp > 0:
            first -= 1
        if mutate == "short" and last == slabs and N % BK:
            last -= 1
        for sl in range(first, last):
            rows = slice(sl * BK, min(N, (sl + 1) * BK))
            partial[sp] += a_rows[rows].T @ b_rows[rows]                                                                          # float32
    acc = partial[0].copy()
    for sp in range(1, eff):
        acc += partial[sp]
    if mutate == "fold":
        return acc[:Fn, :Cn * k * k].reshape(Fn, Cn, k, k)
    return acc[:Fn].reshape(Fn, k, k, cp)[:, :, :, :Cn].transpose(0, 3, 1, 2)


#         B  C   F   H   W  k  s  splits
CLEAN = [(2, 16, 20, 9, 9, 3, 1, 2), (3, 8, 8, 10, 10, 3, 2, 2), (2, 8, 8, 7, 7, 3, 2, 1), (1, 8, 16, 6, 6, 4, 2, 3), (3, 3, 20, 7, 5, 3, 1, 3), (2, 24, 8, 8, 8, 3, 2, 1),
         (1, 8, 8, 6, 6, 5, 1, 0), (2, 8, 8, 4, 4, 1, 1, 1)]
MUTATED = (3, 8, 8, 10, 10, 3, 2, 2)          # stride 2 (Q dilated), N = 75: two slabs, the last one short, one slab per split
_data = {}


def case_data(case):
    if case not in _data:
        B, Cn, Fn, h, w, k, s, _ = case
        ho, wo = same_geometry(h, w, k, s)[:2]
        rng = np.random.default_rng(16)
        x = to_bf16_values(rng.uniform(0.5, 1.0, (B, Cn, h, w)))
        dy = to_bf16_values(rng.uniform(0.5, 1.0, (B, Fn, ho, wo)))
        x, dy = np.minimum(x, F32(0.99609375)), np.minimum(dy, F32(0.99609375))     # rounding may reach 1.0: stay inside [0.5, 1)
        ref, mag = reference(x, dy, k, s)
        _data[case] = x, dy, ref, (B * ho * wo + 8) * 2.0 ** -23 * mag + 2 * 2.0 ** -24 * np.abs(ref)
    return _data[case]


@pytest.mark.parametrize("case", CLEAN)
def test_restatement_is_inside_the_bound(case):
    x, dy, ref, bound = case_data(case)
    got = restated(x, dy, case[5], case[6], case[7])
    ratio = float((np.abs(got.astype(F64) - ref) / bound).max())
    print("restated implicit weight gradient %s: worst |err| / bound = %.4f" % (case, ratio))
    assert ratio <= 1


@pytest.mark.parametrize("mutate", ["dilation", "top", "taps", "short", "shared", "fold"])
def test_every_mutation_leaves_the_bound(mutate):
    x, dy, ref, bound = case_data(MUTATED)
    assert partition(3 * 5 * 5, MUTATED[7]) == (2, 1)
    got = restated(x, dy, MUTATED[5], MUTATED[6], MUTATED[7], mutate)
    assert got.shape == ref.shape
    ratio = float((np.abs(got.astype(F64) - ref) / bound).max())
    assert ratio > 1, (mutate, ratio)
