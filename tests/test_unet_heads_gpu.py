"""The multi-head U-Net on the device (bla_unet_create_heads) against tests/test_unet_heads_host.py: configuration (tests/test_unet_bf16_host.py's
CFG, batch 2, 2 heads of width 8), parameters, inputs, the float64 networks and the recorded values are that file's.

* heads == 1 is bla_unet_create_mixed: predictions and the gradient bucket bit for bit, both `products` values, attention modes 0 and 3.
* 16 x 16 images, fp32 products: level-1 S = 64 and mid S = 4 both run the fp32 heads entries under mode 0.  Against the float64 network with the float64
  multi-head block: predictions 1e-4 normwise, gradient tensors 1e-2 (tests/test_unet_model.py's bounds).  Mode 3 moves the level-1 blocks onto the online
  bf16 heads entries: other bits, every gradient tensor within 0.25 normwise of mode 0's (DESIGN 3.29's model bound), bit-reproducible, and mode 0 afterwards
  gives the first bits again.
* The blocks' stored routes follow every switch: mode 0, mode 3, mode 0 gives the first bits again; mode 3's are those of a fresh model put under mode 3
  before its first pass; a refused switch to BLA_UNET_ATTENTION_BF16 changes nothing of the next pass.
* 32 x 32 images, fp32 products: level-1 S = 256 runs the online heads entries in BOTH modes, mid S = 16 the fp32 heads entries in both (the online predicate
  refuses it) -- so the two modes are bit-equal.  Per tensor the device lies within twice the host-recorded ||rounded - exact|| / ||exact|| (DESIGN 3.25 - 3.30's
  margin); the one tensor whose recorded value depends on the draw of the roundings (host.DRAW_DEPENDENT) within 0.25 normwise instead.
* 40 x 48 images: level-1 S = 480 online, the 5 x 6 mid block (S = 30) on the fp32 heads entries: finite and bit-reproducible.
* Refusals: 36 x 36 and 40 x 40 images (S = 400 at level 1: no multi-head path; one head is accepted), heads key_dim = 264, heads = 0: BLA_ERR_INVALID, *out
  untouched.  bla_unet_set_attention(BLA_UNET_ATTENTION_BF16) is refused at 2 heads, the mode unchanged, and accepted at 1."""
import ctypes as C

import numpy as np
import pytest

import test_unet_bf16_host as bf
import test_unet_heads_host as host
from test_unet_bf16_gpu import cfg_struct

pytestmark = pytest.mark.gpu
F32, BF16 = 0, 1
B, HEADS = host.B, host.HEADS


class Model:
    """a device model (heads None: bla_unet_create_mixed) with the parameter bucket uploaded in tensor order"""

    def __init__(self, pkg, cfg, products, heads, params=None, batch=B):
        self.pkg, self.L, self.batch, self.cfg = pkg, pkg.lib(), batch, cfg
        L = self.L
        self.h = pkg.unet_create_mixed(cfg_struct(cfg), batch, products) if heads is None else pkg.unet_create_heads(cfg_struct(cfg), batch, products, heads)
        self.tensors = []
        for i in range(L.bla_unet_tensor_count(self.h)):
            off, cnt = C.c_size_t(), C.c_size_t(); name = C.create_string_buffer(96)
            pkg.native.check(L.bla_unet_tensor_info(self.h, i, C.byref(off), C.byref(cnt), name, 96))
            self.tensors.append((name.value.decode(), off.value, cnt.value))
        self.total = L.bla_unet_param_count(self.h)
        if params is not None:
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
        out, g = np.empty((self.batch, c["in_channels"], c["image_h"], c["image_w"]), np.float32), np.empty(self.total, np.float32)
        chk(L.bla_memcpy_d2h(out.ctypes.data, L.bla_unet_output(self.h), out.nbytes, None))
        chk(L.bla_memcpy_d2h(g.ctypes.data, L.bla_unet_grads(self.h), g.nbytes, None)); self.pkg.sync()
        return out, g

    def destroy(self):
        self.pkg.native.check(self.L.bla_unet_destroy(self.h))


@pytest.fixture(scope="module")
def dev(pkg):
    pkg.init(0)
    return pkg


def device_inputs(dev, cfg):
    x, temb, noise, drop = host.make_inputs(cfg)
    dd = bf.device_drop_layout(drop, cfg)
    return dict(x=dev.to_device(x), temb=dev.to_device(temb), noise=dev.to_device(noise), drop=dev.DeviceArray((dd.size,), np.uint8).copy_from(dd))


def compare(m, out, grads, exact):
    """[(name, ||device - exact|| / ||exact||)]: the predictions per image, then every gradient tensor whose exact gradient is not zero"""
    rows = [(f"prediction[{b}]", bf.normwise(out[b], exact[0][b])) for b in range(B)]
    for name, off, cnt in m.tensors:
        g, w = grads[off:off + cnt].astype(np.float64), exact[1][name].ravel()
        assert g.size == w.size, name
        if np.linalg.norm(w) == 0:
            assert name.endswith(".biases") and "attention" in name and not g.any(), name
            continue
        rows.append((name, bf.normwise(g, w)))
    return rows


@pytest.mark.parametrize("products", [F32, BF16], ids=["f32", "bf16"])
def test_one_head_is_create_mixed(dev, products):
    cfg = host.cfg_at(16)
    P, data = host.make_params(cfg, 1), device_inputs(dev, cfg)
    a, b = Model(dev, cfg, products, 1, P), Model(dev, cfg, products, None, P)
    assert a.tensors == b.tensors and a.total == b.total and dev.unet_heads(a.h) == 1 == dev.unet_heads(b.h) and dev.lib().bla_unet_heads(None) == 1
    assert dev.unet_products(a.h) == products
    for mode in (dev.UNET_ATTENTION_F32, dev.UNET_ATTENTION_BF16_ONLINE):
        (oa, ga), (ob, gb) = a.one_pass(data, mode), b.one_pass(data, mode)
        assert np.isfinite(ga).all() and np.abs(ga).max() > 0
        assert np.array_equal(oa, ob) and np.array_equal(ga, gb), mode
    a.destroy(); b.destroy()


def test_16x16_against_the_float64_network_and_the_online_mode(dev):
    cfg = host.cfg_at(16)
    m = Model(dev, cfg, F32, HEADS, host.make_params(cfg))
    data = device_inputs(dev, cfg)
    D = HEADS * cfg["key_dim"]
    sizes = {n: cnt for n, _, cnt in m.tensors}
    assert dev.unet_heads(m.h) == HEADS and dev.unet_attention(m.h) == dev.UNET_ATTENTION_F32
    assert sizes["mid_self_attention.Q_proj"] == 48 * D and sizes["down_2_self_attention_1.K_proj"] == 64 * D and sizes["up_3_self_attention_2.V_proj"] == 64 * D
    assert sizes["up_3_self_attention_1.weights"] == D * 64 and sizes["mid_self_attention.biases"] == 48
    assert [(n, c) for n, _, c in m.tensors] == [(n, int(np.prod(s))) for n, s in bf.tensor_list(host.wide(cfg))]
    out, grads = m.one_pass(data)
    assert np.isfinite(out).all() and np.isfinite(grads).all()
    rows = compare(m, out, grads, host.exact16())
    worst = max(rows[B:], key=lambda t: t[1])
    print(f"16 x 16, mode 0: predictions {[f'{v:.2e}' for _, v in rows[:B]]}, worst gradient {worst[0]} {worst[1]:.2e}")
    assert all(v <= 1e-4 for _, v in rows[:B]), rows[:B]
    assert all(v <= 1e-2 for _, v in rows[B:]), [r for r in rows[B:] if not r[1] <= 1e-2]
    # mode 3: the level-1 blocks (S = 64) on the online bf16 heads entries
    out3, grads3 = m.one_pass(data, dev.UNET_ATTENTION_BF16_ONLINE)
    assert not np.array_equal(grads3, grads) and not np.array_equal(out3, out)
    moved = {n: bf.normwise(grads3[off:off + cnt], grads[off:off + cnt].astype(np.float64)) for n, off, cnt in m.tensors if grads[off:off + cnt].any()}
    print(f"16 x 16, mode 3 against mode 0: largest move {max(moved.values()):.2e} ({max(moved, key=moved.get)})")
    assert max(moved.values()) <= 0.25, {n: v for n, v in moved.items() if v > 0.25}
    again = m.one_pass(data)
    assert np.array_equal(again[0], out3) and np.array_equal(again[1], grads3)
    back = m.one_pass(data, dev.UNET_ATTENTION_F32)
    assert np.array_equal(back[0], out) and np.array_equal(back[1], grads)
    m.destroy()


def test_stored_routes_follow_every_switch(dev):
    """Every attention block keeps the route bla_unet_set_attention last decided for it: a route left behind by an earlier mode would show as other bits.
    16 x 16, batch 2, 2 heads, fp32 products: the level-1 blocks (S = 64) move between the fp32 heads and the online heads entries, the mid block (S = 4) stays."""
    cfg = host.cfg_at(16)
    P, data, L = host.make_params(cfg), device_inputs(dev, cfg), dev.lib()
    m, fresh = Model(dev, cfg, F32, HEADS, P), Model(dev, cfg, F32, HEADS, P)

    def same(p, q):
        return np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1])
    first = m.one_pass(data)
    second = m.one_pass(data, dev.UNET_ATTENTION_BF16_ONLINE)
    third = m.one_pass(data, dev.UNET_ATTENTION_F32)
    assert np.isfinite(first[1]).all() and np.abs(first[1]).max() > 0 and not same(second, first)
    assert same(third, first)
    assert same(second, fresh.one_pass(data, dev.UNET_ATTENTION_BF16_ONLINE))      # a model that was never under another mode
    assert L.bla_unet_set_attention(m.h, dev.UNET_ATTENTION_BF16) == 1 and b"heads" in L.bla_last_error() and L.bla_unet_attention(m.h) == dev.UNET_ATTENTION_F32
    assert same(m.one_pass(data), third)                                           # the refused switch left mode and routes alone
    m.destroy(); fresh.destroy()


def test_32x32_within_twice_the_recorded_rounding(dev):
    cfg = host.cfg_at(32)
    exact, _, rec = host.recorded32()
    m = Model(dev, cfg, F32, HEADS, host.make_params(cfg))
    data = device_inputs(dev, cfg)
    out, grads = m.one_pass(data)
    assert np.isfinite(out).all() and np.isfinite(grads).all()
    rows = compare(m, out, grads, exact)
    for name, v in rows:
        print(f"{name:44s} device {v:.3e}  host rounded-vs-exact {rec[name]:.3e}  ratio {v / rec[name]:.2f}")
    bad = [(n, v, rec[n]) for n, v in rows if not v <= (0.25 if n in host.DRAW_DEPENDENT else 2 * rec[n])]
    assert not bad, bad
    out3, grads3 = m.one_pass(data, dev.UNET_ATTENTION_BF16_ONLINE)      # the same entries block for block: S = 256 online, S = 16 fp32 heads
    assert np.array_equal(out3, out) and np.array_equal(grads3, grads)
    m.destroy()


def test_40x48_mixes_the_two_paths(dev):
    """level 1 is 20 x 24 (S = 480 = 15 x 32: online), the mid block 5 x 6 (S = 30: fp32 heads)"""
    cfg = dict(host.CFG, image_h=40, image_w=48)
    m = Model(dev, cfg, F32, HEADS, host.make_params(cfg))
    data = device_inputs(dev, cfg)
    (o1, g1), (o2, g2) = m.one_pass(data), m.one_pass(data)
    assert np.isfinite(o1).all() and np.isfinite(g1).all() and np.abs(g1).max() > 0
    assert all(g1[off:off + cnt].any() for n, off, cnt in m.tensors if "attention" in n and not n.endswith(".biases"))
    assert np.array_equal(o1, o2) and np.array_equal(g1, g2)
    m.destroy()


def test_refusals(dev):
    L = dev.lib()

    def create(cfg, heads, products=F32):
        h = C.c_void_p(0x1234)
        st = L.bla_unet_create_heads(C.byref(h), C.byref(cfg_struct(cfg)), B, products, heads)
        return st, h
    for side in (36, 40):                                          # 36: no multiple of 8 either; 40: level 1 is 20 x 20, S = 400 (> 64, no multiple of 32)
        st, h = create(host.cfg_at(side), HEADS)
        assert st == 1 and h.value == 0x1234, side
    assert b"multi-head" in L.bla_last_error()
    st, h = create(host.cfg_at(40), 1)                              # one head: the fp32 block takes any S
    assert st == 0 and L.bla_unet_heads(h) == 1
    dev.native.check(L.bla_unet_destroy(h))
    for heads in (33, 0, -1):                                      # 33 x 8 = 264
        st, h = create(host.cfg_at(16), heads)
        assert st == 1 and h.value == 0x1234 and b"heads" in L.bla_last_error(), heads
    st, h = create(host.cfg_at(16), 32)                             # 32 x 8 = 256: the limit
    assert st == 0
    assert L.bla_unet_set_attention(h, dev.UNET_ATTENTION_BF16) == 1 and b"heads" in L.bla_last_error() and L.bla_unet_attention(h) == dev.UNET_ATTENTION_F32
    assert L.bla_unet_set_attention(h, dev.UNET_ATTENTION_BF16_ONLINE) == 0 and L.bla_unet_set_attention(h, dev.UNET_ATTENTION_F32) == 0
    dev.native.check(L.bla_unet_destroy(h))
    st, h = create(host.cfg_at(16), 1)
    assert st == 0 and L.bla_unet_set_attention(h, dev.UNET_ATTENTION_BF16) == 0 and L.bla_unet_attention(h) == dev.UNET_ATTENTION_BF16
    dev.native.check(L.bla_unet_destroy(h))
