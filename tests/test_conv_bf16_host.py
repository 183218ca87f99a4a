"""Mixed-precision convolution (bf16 operands, fp32 accumulation): what can be checked without a device.

1. Without a device every new compute entry returns BLA_ERR_NO_DEVICE; pure argument errors (NULL pointers, extents <= 0, stride < 1, cp % 8 != 0)
   answer BLA_ERR_INVALID before the device is asked for.  bla_conv_bf16_layout is a host function and answers without a device.
2. bla_conv_bf16_layout against the TF-SAME formula of lib/conv.c (restated here) on a sweep of (h, w, k, stride).
3. The index maps of include/bla.h -- padded channel-last activations, tap-major kernel matrices (forward; flipped and transposed for the data
   gradient), the (c, p, q) x (b, i, j) im2col of the weight gradient -- restated in numpy, give the float64 im2col convolution, its adjoint and its
   weight gradient, stride 2 and odd maps included.
4. A numpy float32 restatement of the gather kernel's accumulation (64-deep slabs over the tap-major K, 16-deep MFMA steps, two 8-element fragment halves,
   exact products, one fp32 add per product) stays inside

       bound = (K + 8) 2^-23 (|A|.|B|) + 2 2^-24 (|bias| + |ref|)                          (K = k k Cp, k k Fp, or B Ho Wo rounded up to 8)

   and leaves it under five mutations of the index maps: the kernel not flipped in the data gradient, the top pad off by one, the dilation ignored, the
   taps in (q, p) order, the last short slab dropped.  The operands have magnitudes in [0.5, 1), so one misplaced product (>= 0.25) exceeds the bound
   (< 0.001 here); that is asserted too.
"""
import numpy as np
import pytest

F32, F64, U16 = np.float32, np.float64, np.uint16


# ---- geometry, restated ------------------------------------------------------------------------------------------------------------------------------
def same_geometry(h, w, k, s):
    """lib/conv.c:13-28,55-56: ceil on a float quotient; returns ho, wo, pt, pl, vpad, hpad."""
    ho, wo = int(np.ceil(F32(h) / F32(s))), int(np.ceil(F32(w) / F32(s)))
    vpad, hpad = max((ho - 1) * s + k - h, 0), max((wo - 1) * s + k - w, 0)
    return ho, wo, vpad // 2, hpad // 2, vpad, hpad


def layout(h, w, k, s, data_gradient):
    """hp, wp, top, left, dilate as include/bla.h states them."""
    ho, wo, pt, pl, vpad, hpad = same_geometry(h, w, k, s)
    if data_gradient:
        return h + k - 1, w + k - 1, k - 1 - pt, k - 1 - pl, s
    return h + vpad, w + hpad, pt, pl, 1


def round8(x):
    return -(-x // 8) * 8


# ---- the float64 im2col reference (lib/conv.c's maps with a batch in front) ---------------------------------------------------------------------------
def im2col(x, k, s):
    """x [B][C][H][W] -> cols [B][Ho Wo][C k k], cols[b][(i, j)][(c, p, q)] = x[b][c][i s + p - pt][j s + q - pl], 0 outside."""
    B, Cn, h, w = x.shape
    ho, wo, pt, pl, _, _ = same_geometry(h, w, k, s)
    xp = np.zeros((B, Cn, h + 2 * k + s, w + 2 * k + s), x.dtype)
    xp[:, :, pt:pt + h, pl:pl + w] = x
    cols = np.zeros((B, ho, wo, Cn, k, k), x.dtype)
    for p in range(k):
        for q in range(k):
            cols[:, :, :, :, p, q] = xp[:, :, p:p + (ho - 1) * s + 1:s, q:q + (wo - 1) * s + 1:s].transpose(0, 2, 3, 1)
    return cols.reshape(B, ho * wo, Cn * k * k)


def conv_reference(x, kern, del_y, s):
    """forward [B][F][Ho][Wo], del_x [B][C][H][W] (the adjoint of the forward map), del_kern [F][C][k][k] -- in the dtype of the inputs (float64 or int64)."""
    B, Cn, h, w = x.shape
    Fn, _, k, _ = kern.shape
    ho, wo, pt, pl, _, _ = same_geometry(h, w, k, s)
    cols = im2col(x, k, s)
    kmat = kern.reshape(Fn, Cn * k * k)
    fwd = np.einsum("bnk,fk->bfn", cols, kmat).reshape(B, Fn, ho, wo)
    dy = del_y.reshape(B, Fn, ho * wo)
    dkern = np.einsum("bfn,bnk->fk", dy, cols).reshape(kern.shape)
    dcols = np.einsum("bfn,fk->bnk", dy, kmat).reshape(B, ho, wo, Cn, k, k)
    dxp = np.zeros((B, Cn, h + 2 * k + s, w + 2 * k + s), x.dtype)
    for p in range(k):
        for q in range(k):
            dxp[:, :, p:p + (ho - 1) * s + 1:s, q:q + (wo - 1) * s + 1:s] += dcols[:, :, :, :, p, q].transpose(0, 3, 1, 2)
    return fwd, dxp[:, :, pt:pt + h, pl:pl + w].copy(), dkern


# ---- the layouts of include/bla.h, restated (values, not bit patterns: the GPU tests apply native.to_bf16 to the same maps) -----------------------------
def padded_channel_last(src, hp, wp, top, left, d):
    B, Cn, h, w = src.shape
    P = np.zeros((B, hp, wp, round8(Cn)), src.dtype)
    P[:, top:top + (h - 1) * d + 1:d, left:left + (w - 1) * d + 1:d, :Cn] = src.transpose(0, 2, 3, 1)
    return P


def kernel_matrix(kern, data_gradient, tap_order="pq", flip=True):
    Fn, Cn, k, _ = kern.shape
    if not data_gradient:
        A = np.zeros((Fn, k, k, round8(Cn)), kern.dtype)
        src = kern.transpose(0, 2, 3, 1)                                  # [f][p][q][c]
        A[:, :, :, :Cn] = src if tap_order == "pq" else src.transpose(0, 2, 1, 3)
        return A.reshape(Fn, k * k * round8(Cn))
    A = np.zeros((Cn, k, k, round8(Fn)), kern.dtype)
    src = kern.transpose(1, 2, 3, 0)                                      # [c][p][q][f]
    A[:, :, :, :Fn] = src[:, ::-1, ::-1, :] if flip else src
    return A.reshape(Cn, k * k * round8(Fn))


def gathered_operand(P, k, s, ho, wo):
    """The B operand of bla_conv2d_gathered_bf16: G[(b, i, j)][(p k + q) cp + c] = P[b][i s + p][j s + q][c]."""
    B, hp, wp, cp = P.shape
    G = np.zeros((B, ho, wo, k, k, cp), P.dtype)
    for p in range(k):
        for q in range(k):
            G[:, :, :, p, q, :] = P[:, p:p + (ho - 1) * s + 1:s, q:q + (wo - 1) * s + 1:s, :]
    return G.reshape(B * ho * wo, k * k * cp)


def to_output(prod, B, ho, wo):
    """[rows][(b, i, j)] -> [B][rows][ho][wo]"""
    return prod.reshape(prod.shape[0], B, ho, wo).transpose(1, 0, 2, 3)


def forward_operands(x, kern, s, top_shift=0, tap_order="pq"):
    _, _, h, w = x.shape
    k = kern.shape[2]
    ho, wo = same_geometry(h, w, k, s)[:2]
    hp, wp, top, left, d = layout(h, w, k, s, False)
    return kernel_matrix(kern, False, tap_order), gathered_operand(padded_channel_last(x, hp, wp, top + top_shift, left, d), k, s, ho, wo), (ho, wo)


def dgrad_operands(del_y, kern, h, w, s, flip=True, dilate=True):
    k = kern.shape[2]
    hp, wp, top, left, d = layout(h, w, k, s, True)
    return kernel_matrix(kern, True, flip=flip), gathered_operand(padded_channel_last(del_y, hp, wp, top, left, d if dilate else 1), k, 1, h, w), (h, w)


def wgrad_operands(del_y, x, k, s):
    """dY16 [f][n], G [(c, p, q)][n], n = (b, i, j) at the pitch B Ho Wo rounded up to 8, zero tails."""
    B, Fn = del_y.shape[:2]
    cols = im2col(x, k, s)
    n = B * cols.shape[1]
    dy = np.zeros((Fn, round8(n)), x.dtype)
    dy[:, :n] = del_y.reshape(B, Fn, -1).transpose(1, 0, 2).reshape(Fn, n)
    G = np.zeros((cols.shape[2], round8(n)), x.dtype)
    G[:, :n] = cols.transpose(2, 0, 1).reshape(cols.shape[2], n)
    return dy, G


MAP_CASES = [(3, 3, 5, 5, 7, 3, 1), (2, 8, 8, 8, 8, 3, 2), (1, 8, 16, 7, 9, 3, 2), (2, 24, 8, 8, 8, 3, 1), (2, 16, 16, 4, 4, 1, 1), (1, 8, 8, 6, 6, 5, 1),
             (2, 4, 6, 5, 6, 2, 2), (1, 5, 3, 7, 7, 3, 3)]


@pytest.mark.parametrize("case", MAP_CASES, ids=lambda c: "B%d_C%d_F%d_%dx%d_k%d_s%d" % c)
def test_index_maps_equal_the_im2col_reference(case):
    B, Cn, Fn, h, w, k, s = case
    rng = np.random.default_rng(sum(case))
    ho, wo = same_geometry(h, w, k, s)[:2]
    x, kern, dy = rng.standard_normal((B, Cn, h, w)), rng.standard_normal((Fn, Cn, k, k)), rng.standard_normal((B, Fn, ho, wo))
    fwd, dx, dkern = conv_reference(x, kern, dy, s)
    A, G, (oh, ow) = forward_operands(x, kern, s)
    assert np.allclose(to_output(A @ G.T, B, oh, ow), fwd, rtol=0, atol=1e-12 * np.abs(fwd).max())
    A, G, (oh, ow) = dgrad_operands(dy, kern, h, w, s)
    assert np.allclose(to_output(A @ G.T, B, oh, ow), dx, rtol=0, atol=1e-12 * np.abs(dx).max())
    dy16, G = wgrad_operands(dy, x, k, s)
    assert np.allclose((dy16 @ G.T).reshape(kern.shape), dkern, rtol=0, atol=1e-12 * np.abs(dkern).max())


def test_layout_against_the_same_formula(pkg):
    n = 0
    for h in (1, 2, 3, 4, 5, 7, 8, 9, 16, 31, 32):
        for w in (1, 3, 6, 8, 9, 32):
            for k in (1, 2, 3, 4, 5, 7):
                for s in (1, 2, 3, 4):
                    for dg in (False, True):
                        assert pkg.conv_bf16_layout(h, w, k, s, dg) == layout(h, w, k, s, dg), (h, w, k, s, dg)
                        hp, wp, top, left, d = layout(h, w, k, s, dg)
                        ho, wo = same_geometry(h, w, k, s)[:2]
                        sh, sw = (ho, wo) if dg else (h, w)               # the map that is copied in ...
                        oh, ow, st = (h, w, 1) if dg else (ho, wo, s)     # ... and the output the product forms from it
                        assert top >= 0 and left >= 0 and top + (sh - 1) * d < hp and left + (sw - 1) * d < wp
                        assert (oh - 1) * st + k <= hp and (ow - 1) * st + k <= wp
                        n += 1
    assert n == 11 * 6 * 6 * 4 * 2
    L = pkg.lib()
    assert L.bla_conv_bf16_layout(0, 8, 3, 1, 0, *[None] * 5) == 1 and L.bla_conv_bf16_layout(8, 8, 3, 0, 0, *[None] * 5) == 1


# ---- the kernel's accumulation, restated ----------------------------------------------------------------------------------------------------------
def restated_product(a, b, drop_last_slab=False):
    """a [m][K], b [n][K]: float32 arrays holding bf16 values.  Slabs of 64 (the last may be short), MFMA steps of 16, fragment half 0 then 1, one fp32
    add per exact product -- the order of conv_bf16_gather_kernel, which is gemm_bf16_nt_kernel's."""
    K = a.shape[1]
    acc = np.zeros((a.shape[0], b.shape[0]), F32)
    slabs = list(range(0, K, 64))
    for kb in slabs[:-1] if drop_last_slab else slabs:
        for s in range(0, min(64, K - kb), 16):
            for half in (0, 1):
                for j in range(8):
                    kk = kb + s + 8 * half + j
                    if kk < K:
                        acc = (acc + a[:, kk, None] * b[None, :, kk]).astype(F32)
    return acc


def half_to_one(pkg, rng, shape):
    """bf16 values with magnitudes in [0.5, 1) and random signs, as float32."""
    x = rng.uniform(0.5, 1.0, shape).astype(F32)
    x = np.minimum(pkg.from_bf16(pkg.to_bf16(x)), F32(0.99609375))
    return (x * rng.choice(np.array([-1, 1], F32), shape)).astype(F32)


FWD_CASE = (2, 3, 5, 5, 7, 3, 1)      # Cp = 8, K = 72: one whole slab and a short one that holds tap (2, 2)
DGRAD_CASE = (1, 8, 8, 7, 9, 3, 2)    # stride 2 on an odd map: the dilated data gradient, Fp = 8, K = 72


@pytest.fixture(scope="module")
def restated(pkg):
    rng = np.random.default_rng(47)
    out = {}
    for name, (B, Cn, Fn, h, w, k, s) in (("fwd", FWD_CASE), ("dgrad", DGRAD_CASE)):
        ho, wo = same_geometry(h, w, k, s)[:2]
        x, kern, dy = half_to_one(pkg, rng, (B, Cn, h, w)), half_to_one(pkg, rng, (Fn, Cn, k, k)), half_to_one(pkg, rng, (B, Fn, ho, wo))
        bias = half_to_one(pkg, rng, (B, Fn))
        fwd, dx, dkern = conv_reference(x.astype(F64), kern.astype(F64), dy.astype(F64), s)
        afwd, adx, adkern = conv_reference(np.abs(x).astype(F64), np.abs(kern).astype(F64), np.abs(dy).astype(F64), s)
        n8 = round8(B * ho * wo)
        ref_f = fwd + bias[:, :, None, None]
        out[name] = dict(shape=(B, Cn, Fn, h, w, k, s), x=x, kern=kern, dy=dy, bias=bias, fwd=ref_f, dx=dx, dkern=dkern,
                         bound_fwd=(k * k * round8(Cn) + 8) * 2.0 ** -23 * afwd + 2 * 2.0 ** -24 * (np.abs(bias)[:, :, None, None] + np.abs(ref_f)),
                         bound_dx=(k * k * round8(Fn) + 8) * 2.0 ** -23 * adx + 2 * 2.0 ** -24 * np.abs(dx),
                         bound_dkern=(n8 + 8) * 2.0 ** -23 * adkern + 2 * 2.0 ** -24 * np.abs(dkern))
    return out


def restated_forward(c, **mut):
    B = c["shape"][0]
    A, G, (oh, ow) = forward_operands(c["x"], c["kern"], c["shape"][6], mut.get("top_shift", 0), mut.get("tap_order", "pq"))
    out = to_output(restated_product(A, G, mut.get("drop_last_slab", False)), B, oh, ow)
    return (out + c["bias"][:, :, None, None]).astype(F32)


def restated_dgrad(c, **mut):
    B, _, _, h, w, _, s = c["shape"]
    A, G, (oh, ow) = dgrad_operands(c["dy"], c["kern"], h, w, s, mut.get("flip", True), mut.get("dilate", True))
    return to_output(restated_product(A, G, mut.get("drop_last_slab", False)), B, oh, ow)


def restated_wgrad(c):
    dy16, G = wgrad_operands(c["dy"], c["x"], c["shape"][5], c["shape"][6])
    return restated_product(dy16, G).reshape(c["kern"].shape)


def test_one_misplaced_product_exceeds_the_bound(restated):
    for c in restated.values():
        for key in ("x", "kern", "dy"):
            assert np.abs(c[key]).min() >= 0.5 and np.abs(c[key]).max() < 1
        assert max(c["bound_fwd"].max(), c["bound_dx"].max(), c["bound_dkern"].max()) < 1e-3 < 0.25


@pytest.mark.parametrize("name", ["fwd", "dgrad"])
def test_restated_accumulation_stays_inside_the_bound(restated, name):
    c = restated[name]
    for got, ref, bound in ((restated_forward(c), c["fwd"], c["bound_fwd"]), (restated_dgrad(c), c["dx"], c["bound_dx"]),
                            (restated_wgrad(c), c["dkern"], c["bound_dkern"])):
        err = np.abs(got.astype(F64) - ref)
        assert got.shape == ref.shape and (err <= bound).all(), (err / bound).max()


@pytest.mark.parametrize("name,mutation", [("fwd", dict(top_shift=1)), ("fwd", dict(tap_order="qp")), ("fwd", dict(drop_last_slab=True)),
                                           ("dgrad", dict(flip=False)), ("dgrad", dict(dilate=False)), ("dgrad", dict(drop_last_slab=True))],
                         ids=["top_pad_off_by_one", "tap_order_qp", "fwd_last_short_slab_dropped", "kernel_not_flipped", "dilation_ignored",
                              "dgrad_last_short_slab_dropped"])
def test_mutated_index_maps_leave_the_bound(restated, name, mutation):
    c = restated[name]
    got, ref, bound = (restated_forward(c, **mutation), c["fwd"], c["bound_fwd"]) if name == "fwd" else (restated_dgrad(c, **mutation), c["dx"], c["bound_dx"])
    assert (np.abs(got.astype(F64) - ref) > bound).any(), mutation


# ---- the entries without a device ------------------------------------------------------------------------------------------------------------------------
X = 0x10000   # a non-NULL, 16-byte aligned stand-in address: nothing is launched in these tests


def entry_calls(L, bad=None):
    """One call of every compute entry with sound arguments; `bad` names the argument set to break."""
    g = dict(src=X, dst=X, A=X, P=X, out=X, x=X, kern=X, dy=X, dk=X, dx=X, batch=2, c=8, h=6, w=6, k=3, stride=1, cp=8, rows=8)
    if bad:
        g.update(bad)
    return dict(
        pad=lambda: L.bla_conv_bf16_pad(None, g["src"], g["dst"], g["batch"], g["c"], g["h"], g["w"], g["h"] + 2, g["w"] + 2, 1, 1, 1),
        prepare=lambda: L.bla_conv_bf16_prepare_kernels(None, g["kern"], g["dst"], g["rows"], g["c"], g["k"], 0),
        gathered=lambda: L.bla_conv2d_gathered_bf16(None, g["A"], g["rows"], g["P"], g["batch"], g["h"] + 2, g["w"] + 2, g["cp"], g["k"], g["stride"],
                                                    g["h"], g["w"], g["out"], None, 0),
        forward=lambda: L.bla_conv2d_forward_batched_f32_as_bf16(None, g["x"], g["kern"], g["out"], g["batch"], g["h"], g["w"], g["k"], g["c"], g["rows"],
                                                                 g["stride"], None, 0),
        backward=lambda: L.bla_conv2d_backward_batched_f32_as_bf16(None, g["dy"], g["x"], g["kern"], g["dk"], g["dx"], g["batch"], g["h"], g["w"], g["k"],
                                                                   g["c"], g["rows"], g["stride"]))


def no_device(pkg):
    import torch
    return not torch.cuda.is_available() and pkg.lib().bla_device_count() <= 0


def test_new_entries_refuse_without_a_device(pkg):
    if not no_device(pkg):
        pytest.skip("a device is present")
    L = pkg.lib()
    for name, call in entry_calls(L).items():
        assert call() == 3, name
        assert b"no CPU fallback" in L.bla_last_error() or b"not initialised" in L.bla_last_error()
    assert pkg.conv_bf16_layout(32, 32, 3, 1) == (34, 34, 1, 1, 1)        # the host function needs none


BAD = [("pad", dict(src=None)), ("pad", dict(dst=None)), ("pad", dict(batch=0)), ("pad", dict(c=0)), ("pad", dict(h=-1)), ("pad", dict(dst=X + 2)),
       ("prepare", dict(kern=None)), ("prepare", dict(dst=None)), ("prepare", dict(rows=0)), ("prepare", dict(k=0)),
       ("gathered", dict(A=None)), ("gathered", dict(P=None)), ("gathered", dict(out=None)), ("gathered", dict(rows=0)), ("gathered", dict(batch=-2)),
       ("gathered", dict(stride=0)), ("gathered", dict(cp=12)), ("gathered", dict(cp=0)), ("gathered", dict(k=4)), ("gathered", dict(A=X + 8)),
       ("forward", dict(x=None)), ("forward", dict(kern=None)), ("forward", dict(out=None)), ("forward", dict(stride=0)), ("forward", dict(h=0)),
       ("backward", dict(dy=None)), ("backward", dict(x=None)), ("backward", dict(kern=None)), ("backward", dict(stride=-1)), ("backward", dict(c=0))]


@pytest.mark.parametrize("entry,bad", BAD, ids=["%s-%s" % (e, "_".join("%s=%s" % kv for kv in b.items())) for e, b in BAD])
def test_argument_errors_are_refused_before_the_device(pkg, entry, bad):
    """Pure argument checks: BLA_ERR_INVALID whether or not a device is there (k = 4 in a 6+2 padded map: the taps reach past it)."""
    L = pkg.lib()
    assert entry_calls(L, bad)[entry]() == 1, L.bla_last_error()
