"""bla_attention_{forward,backward}_batched_online_f32, BLA_UNET_ATTENTION_F32_ONLINE and bla_unet_create_attention on the device, against
tests/test_attention_online_f32_host.py: cases, inputs, the float64 materialised multi-head block (+ lse, dots) and the tolerance are that file's.

Block entries
* Every output and saved tensor is a view between guard elements in an allocation filled with 0xFF bytes (tests/test_unet_glue_paths_gpu.py's Guarded); the
  guards must come back untouched.  `weights` is NULL in both workspaces throughout.
* q, k, v, attention, lse, out, the five gradients and the gradient workspace (del_P, del_Q, del_K, del_V, the row dots) against the float64 reference:
  |got - ref| <= t |ref| + t mean|ref|, t = 2e-5 forward and 5e-5 for gradients.  What that leaves the device is measured on the host: the float32 NumPy
  restatement stays at or below 0.07 of the limit on these cases.  The one-key case's del_q, del_k, del_wq, del_wk, exactly zero in the reference, are held to
  the host file's derived absolute bound.  The device's own ratios are printed before anything is asserted.
* Two runs give the same bits in every tensor; image b of a batch equals a batch-1 run of image b.
* Refusals (s = 4097, d = 65, heads d = 264, heads = 0, NULLs, batch 0 and 65536) leave pattern-filled outputs untouched.

Model (tests/test_unet_heads_gpu.py's configuration, batch 2)
* (a) 16 x 16 images, 2 heads of 8: no block is longer than 64, so mode 4 is mode 0 bit for bit.
* (b) 40 x 40 images, 2 heads of 8, fp32 products: bla_unet_create_heads refuses, bla_unet_create_attention(.., F32_ONLINE) creates; one forward + backward
  pass against the float64 network (predictions 1e-4 normwise, gradient tensors 1e-2: the all-fp32 model's bounds in tests/test_unet_heads_gpu.py); a second
  pass for bits; set_attention(F32) and (BF16_ONLINE) are refused and the next pass is unchanged.
* (c) 32 x 32 images, one head: a model created in mode 4 and a bla_unet_create_mixed model switched to mode 4 are bit-equal, and the first one's
  bla_unet_device_bytes is smaller by exactly the S x S floats its routing does not own.
* (d) attention = F32 and one head: bla_unet_create_attention is bla_unet_create_mixed, bit for bit and byte for byte."""
import ctypes as C

import numpy as np
import pytest

import test_attention_online_f32_host as host
import test_unet_heads_host as net
import test_unet_bf16_host as bf
from test_unet_glue_paths_gpu import Guarded
from test_unet_bf16_gpu import cfg_struct

pytestmark = pytest.mark.gpu
F32 = np.float32
PER_IMAGE = ["q", "k", "v", "attention", "lse", "out", "del_x", "del_p", "del_q", "del_k", "del_v", "dots"]
P_F32, B, HEADS = 0, net.B, net.HEADS


@pytest.fixture(scope="module")
def dev(pkg):
    pkg.init(0)
    return pkg


def shapes(case):
    b, c, s, heads, d = case
    D = heads * d
    act = (b, s, D)
    return dict(q=act, k=act, v=act, attention=act, lse=(b, heads, s), out=(b, c, s), del_p=act, del_q=act, del_k=act, del_v=act, dots=(b, heads, s), del_wq=(c, D),
                del_wk=(c, D), del_wv=(c, D), del_w=(D, c), del_x=(b, c, s), partials=(b, c * D))


def buffers(dev, case):
    shp = shapes(case)
    O = {n: Guarded(dev, shp[n]) for n in host.ALL + ["partials"]}
    fws = dev.attention_ws(q=O["q"].ptr, k=O["k"].ptr, v=O["v"].ptr, attention=O["attention"].ptr, scores_raw=O["lse"].ptr)
    gws = dev.attention_ws(q=O["del_q"].ptr, k=O["del_k"].ptr, v=O["del_v"].ptr, attention=O["del_p"].ptr, scores_raw=O["dots"].ptr)
    return O, fws, gws


def run(dev, case, I):
    """both entries on fresh guarded buffers -> {tensor: its bit patterns}"""
    L, chk = dev.lib(), dev.native.check
    b, c, s, heads, d = case
    D = {n: dev.to_device(np.ascontiguousarray(a, F32)) for n, a in I.items()}
    O, fws, gws = buffers(dev, case)
    P = [D[n].ptr for n in ("wq", "wk", "wv", "w")]
    G = [O[n].ptr for n in host.GRADS]
    chk(L.bla_attention_forward_batched_online_f32(None, b, D["x"].ptr, *P, D["bias"].ptr, C.byref(fws), O["out"].ptr, c, s, heads, d))
    chk(L.bla_attention_backward_batched_online_f32(None, b, D["del_y"].ptr, D["x"].ptr, *P, C.byref(fws), C.byref(gws), O["partials"].ptr, *G, c, s, heads, d))
    dev.sync()
    return {n: o.bits() for n, o in O.items()}


@pytest.fixture(scope="module")
def passes(dev):
    """one device pass per case, shared by the tests that only read it"""
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = run(dev, case, host.reference(case)[0])
        return cache[case]
    return get


@pytest.mark.parametrize("case", host.CASES, ids=str)
def test_against_the_materialised_float64_block(passes, case):
    _, ref = host.reference(case)
    got = {n: a.view(F32) for n, a in passes(case).items()}
    rs = host.ratios(got, ref, host.check_names(case))
    print(f"{str(case):22s} device  " + "  ".join(f"{n} {v:.3f}" for n, v in rs.items()))
    assert all(np.isfinite(got[n]).all() for n in host.ALL)
    inside = {}
    if case == host.ONE_KEY:
        inside = host.inside_one_key_bounds(got)
        print(f"{str(case):22s} device  residue / derived bound  " + "  ".join(f"{n} {v:.3f}" for n, v in inside.items()))
    worst = {n: v for n, v in {**rs, **inside}.items() if not v <= 1}
    assert not worst, worst


@pytest.mark.parametrize("case", host.CASES, ids=str)
def test_second_run_and_batch_one(dev, passes, case):
    b, c, s, heads, d = case
    I = host.reference(case)[0]
    first, again = passes(case), run(dev, case, I)
    for n in first:
        assert np.array_equal(first[n], again[n]), n
    for img in range(b):
        one = run(dev, (1, c, s, heads, d), dict(I, x=I["x"][img:img + 1], del_y=I["del_y"][img:img + 1]))
        for n in PER_IMAGE:
            assert np.array_equal(one[n][0], first[n][img]), (img, n)


def test_refusals_leave_the_outputs_untouched(dev):
    L = dev.lib()
    b, c, s, heads, d = case = (2, 16, 40, 4, 16)
    I = host.inputs(case)
    D = {n: dev.to_device(np.ascontiguousarray(a, F32)) for n, a in I.items()}
    O, fws, gws = buffers(dev, (2, 16, 40, 33, 8))                  # (no refused call writes: the buffers only have to exist)
    P = [D[n].ptr for n in ("wq", "wk", "wv", "w")]
    G = [O[n].ptr for n in host.GRADS]

    def fwd(c_, s_, heads_, d_, x=D["x"].ptr, ws=fws, batch=b):
        return L.bla_attention_forward_batched_online_f32(None, batch, x, *P, D["bias"].ptr, C.byref(ws) if ws else None, O["out"].ptr, c_, s_, heads_, d_)

    def bwd(c_, s_, heads_, d_, dy=D["del_y"].ptr, partials=O["partials"].ptr, fw=fws, grad=gws, batch=b):
        return L.bla_attention_backward_batched_online_f32(None, batch, dy, D["x"].ptr, *P, C.byref(fw), C.byref(grad), partials, *G, c_, s_, heads_, d_)
    for shape in [(c, 4097, heads, d), (c, s, heads, 65), (c, s, 33, 8), (c, s, 0, d), (c, s, -1, d), (c, 0, heads, d), (c, s, heads, 0), (0, s, heads, d)]:
        assert fwd(*shape) == 1 and bwd(*shape) == 1, shape
    assert fwd(c, s, heads, d, x=None) == 1 and bwd(c, s, heads, d, dy=None) == 1 and bwd(c, s, heads, d, partials=None) == 1 and fwd(c, s, heads, d, ws=None) == 1
    no_lse = dev.attention_ws(q=O["q"].ptr, k=O["k"].ptr, v=O["v"].ptr, attention=O["attention"].ptr)                                         # ws->scores_raw NULL
    assert fwd(c, s, heads, d, ws=no_lse) == 1 and bwd(c, s, heads, d, fw=no_lse) == 1
    assert bwd(c, s, heads, d, grad=dev.attention_ws(q=O["del_q"].ptr, k=O["del_k"].ptr, v=O["del_v"].ptr, attention=O["del_p"].ptr)) == 1      # the dots NULL
    assert fwd(c, s, heads, d, batch=0) == 1 and bwd(c, s, heads, d, batch=0) == 1 and fwd(c, s, heads, d, batch=65536) == 1 and bwd(c, s, heads, d, batch=65536) == 1
    dev.sync()
    assert all(o.untouched() for o in O.values())


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------------------
class Model:
    """a device model from bla_unet_create_attention (attention given), bla_unet_create_heads (heads given) or bla_unet_create_mixed, parameters uploaded"""

    def __init__(self, pkg, cfg, heads, params, attention=None):
        self.pkg, self.L, self.cfg = pkg, pkg.lib(), cfg
        L = self.L
        if attention is not None:
            self.h = pkg.unet_create_attention(cfg_struct(cfg), B, P_F32, heads, attention)
        else:
            self.h = pkg.unet_create_mixed(cfg_struct(cfg), B, P_F32) if heads is None else pkg.unet_create_heads(cfg_struct(cfg), B, P_F32, heads)
        self.tensors = []
        for i in range(L.bla_unet_tensor_count(self.h)):
            off, cnt = C.c_size_t(), C.c_size_t(); name = C.create_string_buffer(96)
            pkg.native.check(L.bla_unet_tensor_info(self.h, i, C.byref(off), C.byref(cnt), name, 96))
            self.tensors.append((name.value.decode(), off.value, cnt.value))
        self.total = L.bla_unet_param_count(self.h)
        flat = np.zeros(self.total, np.float32)
        for name, off, cnt in self.tensors:
            flat[off:off + cnt] = params[name].ravel()
        pkg.native.check(L.bla_memcpy_h2d(L.bla_unet_params(self.h), flat.ctypes.data, flat.nbytes, None)); pkg.sync()

    def one_pass(self, data, mode=None):
        chk, L = self.pkg.native.check, self.L
        if mode is not None:
            self.pkg.unet_set_attention(self.h, mode)
        chk(L.bla_unet_forward_f32(self.h, None, data["x"].ptr, data["temb"].ptr, data["drop"].ptr))
        chk(L.bla_unet_backward_f32(self.h, None, data["noise"].ptr))
        c = self.cfg
        out, g = np.empty((B, c["in_channels"], c["image_h"], c["image_w"]), np.float32), np.empty(self.total, np.float32)
        chk(L.bla_memcpy_d2h(out.ctypes.data, L.bla_unet_output(self.h), out.nbytes, None))
        chk(L.bla_memcpy_d2h(g.ctypes.data, L.bla_unet_grads(self.h), g.nbytes, None)); self.pkg.sync()
        return out, g

    def bytes(self):
        return self.pkg.unet_device_bytes(self.h)

    def destroy(self):
        self.pkg.native.check(self.L.bla_unet_destroy(self.h))


def device_inputs(dev, cfg):
    x, temb, noise, drop = net.make_inputs(cfg)
    dd = bf.device_drop_layout(drop, cfg)
    return dict(x=dev.to_device(x), temb=dev.to_device(temb), noise=dev.to_device(noise), drop=dev.DeviceArray((dd.size,), np.uint8).copy_from(dd))


def same(p, q):
    return np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1])


def test_model_a_16x16_routes_nothing_new(dev):
    cfg = net.cfg_at(16)
    m = Model(dev, cfg, HEADS, net.make_params(cfg))
    data = device_inputs(dev, cfg)
    first = m.one_pass(data)
    online = m.one_pass(data, dev.UNET_ATTENTION_F32_ONLINE)
    assert dev.unet_attention(m.h) == dev.UNET_ATTENTION_F32_ONLINE == 4
    assert np.isfinite(first[1]).all() and np.abs(first[1]).max() > 0 and same(online, first)
    assert same(m.one_pass(data, dev.UNET_ATTENTION_F32), first)
    m.destroy()


def test_model_b_40x40_two_heads_all_fp32(dev):
    cfg, L = net.cfg_at(40), dev.lib()
    h = C.c_void_p(0x1234)
    assert L.bla_unet_create_heads(C.byref(h), C.byref(cfg_struct(cfg)), B, P_F32, HEADS) == 1 and h.value == 0x1234       # S = 400 at level 1: still no path there
    m = Model(dev, cfg, HEADS, net.make_params(cfg), attention=dev.UNET_ATTENTION_F32_ONLINE)
    assert dev.unet_attention(m.h) == dev.UNET_ATTENTION_F32_ONLINE and dev.unet_heads(m.h) == HEADS
    data = device_inputs(dev, cfg)
    out, grads = m.one_pass(data)
    assert np.isfinite(out).all() and np.isfinite(grads).all()
    exact = net.batch_pass(*net._oracle(), cfg)                                # the unrounded float64 network with the float64 multi-head block
    rows = [(f"prediction[{b}]", bf.normwise(out[b], exact[0][b])) for b in range(B)]
    for name, off, cnt in m.tensors:
        w = exact[1][name].ravel()
        if np.linalg.norm(w) == 0:
            assert name.endswith(".biases") and "attention" in name and not grads[off:off + cnt].any(), name
            continue
        rows.append((name, bf.normwise(grads[off:off + cnt].astype(np.float64), w)))
    worst = max(rows[B:], key=lambda t: t[1])
    print(f"40 x 40, mode 4: predictions {[f'{v:.2e}' for _, v in rows[:B]]}, worst gradient {worst[0]} {worst[1]:.2e}")
    assert all(v <= 1e-4 for _, v in rows[:B]), rows[:B]
    assert all(v <= 1e-2 for _, v in rows[B:]), [r for r in rows[B:] if not r[1] <= 1e-2]
    assert same(m.one_pass(data), (out, grads))
    for mode in (dev.UNET_ATTENTION_F32, dev.UNET_ATTENTION_BF16_ONLINE, dev.UNET_ATTENTION_BF16):
        assert L.bla_unet_set_attention(m.h, mode) == 1 and L.bla_unet_attention(m.h) == dev.UNET_ATTENTION_F32_ONLINE, mode
    assert same(m.one_pass(data), (out, grads))
    m.destroy()


def squares_not_owned(cfg, heads=1):
    """floats of S x S buffers that a one-head model created in mode 4 does not allocate, from the configuration: the five attention blocks sit at level 1 (four)
    and level 3 (the mid block); a block with S > 64 keeps B heads S floats (the lse) instead of scores_raw and weights at B S S each, and the shared gradient
    workspace keeps max(the longest dots, the largest materialising block's S x S) for scores_raw and that block's S x S for weights"""
    side = lambda level: (cfg["image_h"] + (1 << level) - 1) >> level
    S = [side(1) ** 2] * 4 + [side(3) ** 2]
    long_ = [s for s in S if s > 64]
    short = [s for s in S if s <= 64]
    assert heads == 1 and long_ and short
    saved = sum(2 * B * s * s - B * s for s in long_)
    smax, sq = max(S), max(short) ** 2
    saved += B * smax * smax - max(B * max(long_), B * sq)      # the gradient workspace's scores_raw
    saved += B * smax * smax - B * sq                           # ... and its weights
    return saved


def test_model_c_32x32_one_head_owns_no_square(dev):
    cfg = net.cfg_at(32)
    P, data = net.make_params(cfg, 1), device_inputs(dev, cfg)
    a, b = Model(dev, cfg, 1, P, attention=dev.UNET_ATTENTION_F32_ONLINE), Model(dev, cfg, None, P)
    pa, pb = a.one_pass(data), b.one_pass(data, dev.UNET_ATTENTION_F32_ONLINE)
    assert np.isfinite(pa[1]).all() and np.abs(pa[1]).max() > 0 and same(pa, pb)
    plain = b.one_pass(data, dev.UNET_ATTENTION_F32)                    # the materialising fp32 block: other bits, the same network
    assert not same(plain, pa) and bf.normwise(pa[0], plain[0].astype(np.float64)) <= 1e-4
    saved = squares_not_owned(cfg)
    print(f"32 x 32, one head, batch {B}: {b.bytes()} bytes as created by bla_unet_create_mixed, {a.bytes()} created in mode 4, {4 * saved} fewer")
    assert b.bytes() - a.bytes() == 4 * saved and saved > 0
    L = dev.lib()
    assert L.bla_unet_set_attention(a.h, dev.UNET_ATTENTION_F32) == 1 and L.bla_unet_set_attention(a.h, dev.UNET_ATTENTION_BF16) == 1      # S x S buffers it lacks
    assert L.bla_unet_set_attention(a.h, dev.UNET_ATTENTION_BF16_ONLINE) == 0 and L.bla_unet_set_attention(a.h, dev.UNET_ATTENTION_F32_ONLINE) == 0   # a float a row: owned
    assert same(a.one_pass(data), pa)
    a.destroy(); b.destroy()


def test_model_d_f32_is_create_mixed(dev):
    cfg = net.cfg_at(16)
    P, data = net.make_params(cfg, 1), device_inputs(dev, cfg)
    a, b = Model(dev, cfg, 1, P, attention=dev.UNET_ATTENTION_F32), Model(dev, cfg, None, P)
    assert a.bytes() == b.bytes() > 0 and a.tensors == b.tensors and dev.unet_attention(a.h) == dev.UNET_ATTENTION_F32
    assert same(a.one_pass(data), b.one_pass(data))
    h = C.c_void_p(0x1234)
    for bad in (2, -1, 7):
        assert dev.lib().bla_unet_create_attention(C.byref(h), C.byref(cfg_struct(cfg)), B, P_F32, 1, bad) == 1 and h.value == 0x1234
    a.destroy(); b.destroy()
