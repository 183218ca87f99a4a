"""bla_resnet_forward_batched_bf16 / bla_resnet_backward_batched_bf16 on the device (include/bla.h).

Three blocks (tests/test_norm_bf16_host.py: BLOCKS), k = 3, tdim = 16, dropout decisions at p = 0.3; the weight gradients' K-split is asked for as 0
(automatic), 2 and 1.
* Both entries equal the composition include/bla.h states, bit for bit, in every output, saved tensor, scratch tensor and map.  The test makes the
  composition from the public entries, with buffers of its own for the kernel matrices, Q2 and the residual's data gradient; the one step no public entry
  performs, g->time_b = the sum of d_dtb's rows in image order, is restated in numpy float32.
* Every output is a view between guard elements in an allocation filled with 0xFF bytes (the three maps: zero-filled once, as their contract asks); guards
  must be untouched.  A second run with d_del_x = NULL gives the same weight gradients and leaves del_x and sc->g_in untouched.
* Against the unrounded float64 block: per tensor, ||device - exact|| / ||exact|| is at most twice the value the host test recorded for the float64
  restatement with the composition's roundings.  The device differs from that restatement only by fp32 accumulation and by roundings that fall the
  other way at a tie; a factor 2 leaves that room and still fails a data gradient that is not gated (the host test asserts that such a block lies more
  than four times the recorded value away).  Host-recorded (rounded float64 against exact) and measured device values on an MI355X
  (profiles/r19_resnet_bf16_tests.txt), tensors result, del_x, conv1, conv2, time_w, time_b[, res]:
      B2 32->32 8x8   host  1.4e-03 1.6e-03 3.4e-03 2.9e-03 2.1e-03 2.7e-03            device  1.4e-03 1.6e-03 3.4e-03 2.9e-03 2.1e-03 2.7e-03
      B2 16->32 6x6   host  2.2e-03 2.4e-03 3.6e-03 3.0e-03 3.0e-03 3.0e-03 2.5e-03    device  2.2e-03 2.4e-03 3.6e-03 3.0e-03 3.0e-03 3.0e-03 2.5e-03
      B3 32->32 5x7   host  1.5e-03 4.3e-03 9.4e-03 3.0e-03 1.1e-02 1.1e-02            device  1.5e-03 4.3e-03 9.4e-03 3.0e-03 1.1e-02 1.1e-02
  (the device's values equal the host's to the two digits printed: both share the bf16 roundings, beside which the fp32 accumulation does not show)
* Refusals (an extent <= 0, splits < 0, a NULL map) leave pattern-filled outputs untouched."""
import ctypes as C

import numpy as np
import pytest

from test_norm_bf16_host import BLOCKS, K, TDIM, TENSORS, block_differences, block_id, block_inputs, group_slices, normwise, round8

pytestmark = pytest.mark.gpu
F32, U8, U16, U32 = np.float32, np.uint8, np.uint16, np.uint32
GUARD = 64
SPLITS = [0, 2, 1]


@pytest.fixture(scope="module")
def dev(pkg):
    pkg.init(0)
    return pkg


class Out:
    """`shape` elements filled with `fill` bytes, with GUARD elements of the same pattern on either side"""

    def __init__(self, dev, shape, dtype=F32, fill=0xFF):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.bits = {2: U16, 4: U32}[self.dtype.itemsize]
        self.n, self.fill = int(np.prod(shape)), self.bits(~self.bits(0)) if fill == 0xFF else self.bits(0)
        self.arr = dev.DeviceArray((self.n + 2 * GUARD,), self.bits).fill_bytes(fill)
        self.ptr = self.arr.ptr + GUARD * self.dtype.itemsize

    def read(self):
        now = self.arr.numpy()
        assert (now[:GUARD] == self.fill).all() and (now[GUARD + self.n:] == self.fill).all(), "a guard element changed"
        return now[GUARD:GUARD + self.n].reshape(self.shape).copy()          # the bit patterns

    def f32(self):
        return self.read().view(F32)

    def untouched(self):
        return (self.arr.numpy() == self.fill).all()


class Buffers:
    """every tensor either way of running the block writes, each in a guarded allocation of its own"""

    def __init__(self, dev, block):
        B, cin, cout, h, w, gs = block
        hp, wp = dev.conv_bf16_layout(h, w, K, 1)[:2]
        hq, wq = dev.conv_bf16_layout(h, w, K, 1, True)[:2]
        g1, g2 = len(group_slices(cin, gs)), len(group_slices(cout, gs))
        shapes = dict(mu1=(B, g1), sd1=(B, g1), c1=(B, cout, h, w), tdense=(B, cout), mu2=(B, g2), sd2=(B, g2), c2=(B, cout, h, w), res=(B, cout, h, w),
                      result=(B, cout, h, w), g_conv1=(cout, cin, K, K), g_conv2=(cout, cout, K, K), g_time_w=(TDIM, cout), g_time_b=(cout,), g_res=(cout, cin, 1, 1),
                      g_out_a=(B, cout, h, w), g_out_b=(B, cout, h, w), g_in=(B, cin, h, w), dtb=(B, cout), del_x=(B, cin, h, w))
        self.t = {n: Out(dev, s) for n, s in shapes.items()}
        self.t.update(p1=Out(dev, (B, hp, wp, round8(cin)), U16, 0), p2=Out(dev, (B, hp, wp, round8(cout)), U16, 0), q1=Out(dev, (B, hq, wq, round8(cout)), U16, 0))

    def __getitem__(self, n):
        return self.t[n].ptr


def device_inputs(dev, block):
    I = block_inputs(block)
    return {n: dev.to_device(a.astype(U8), U8) if a.dtype == bool else dev.to_device(a) for n, a in I.items()}


def structs(dev, block, D, T):
    N = dev.native
    B, cin, cout = block[:3]
    res = cin != cout
    params = N.ResnetParams(D["conv1"].ptr, D["conv2"].ptr, D["time_w"].ptr, D["time_b"].ptr, D["res"].ptr if res else None)
    ws = N.ResnetWs(T["mu1"], T["sd1"], None, T["c1"], T["tdense"], T["mu2"], T["sd2"], None, None, T["c2"], T["res"] if res else None)
    grads = N.ResnetGrads(T["g_conv1"], T["g_conv2"], T["g_time_w"], T["g_time_b"], T["g_res"] if res else None)
    sc = N.ResnetScratch(T["g_out_a"], T["g_out_b"], T["g_in"], None)
    return params, ws, grads, sc, dev.resnet_bf16_maps(T["p1"], T["p2"], T["q1"])


def run_entries(dev, block, D, T, splits, want_del_x=True):
    B, cin, cout, h, w, gs = block
    params, ws, grads, sc, maps = structs(dev, block, D, T)
    dev.resnet_forward_batched_bf16(D["x"], D["temb"], params, D["drop"], ws, T["result"], B, h, w, cin, cout, K, TDIM, gs, maps)
    dev.resnet_backward_batched_bf16(D["del_out"], D["x"], D["temb"], params, ws, grads, sc, T["dtb"], T["del_x"] if want_del_x else None, B, h, w, cin, cout, K, TDIM, gs,
                                     maps, splits)
    dev.sync()


def run_composition(dev, block, D, T, splits):
    """include/bla.h's composition, entry by entry"""
    B, cin, cout, h, w, gs = block
    L, chk = dev.lib(), dev.native.check
    cpi, cpo, hw = round8(cin), round8(cout), h * w
    hp, wp, top, left, dil = dev.conv_bf16_layout(h, w, K, 1)
    hq, wq, topq, leftq, dq = dev.conv_bf16_layout(h, w, K, 1, True)
    p1 = dev.conv_bf16_map(T["p1"], hp, wp, cpi, top, left, dil); p2 = dev.conv_bf16_map(T["p2"], hp, wp, cpo, top, left, dil)
    q1 = dev.conv_bf16_map(T["q1"], hq, wq, cpo, topq, leftq, dq)
    A = dev.empty((max(cin, cout) * K * K * max(cpi, cpo),), U16)
    # forward
    dev.group_norm_relu_bf16_map(D["x"], B, cin, gs, h, w, T["sd1"], T["mu1"], dst=p1)
    ep = dev.Epilogue(alpha=1.0, bias_col=D["time_b"].ptr)
    chk(L.bla_gemm_f32(None, 0, 0, B, cout, TDIM, D["temb"].ptr, TDIM, D["time_w"].ptr, cout, T["tdense"], cout, C.byref(ep)))
    dev.conv_bf16_prepare_kernels(D["conv1"], A, cout, cin, K)
    dev.conv2d_gathered_bf16(A, cout, T["p1"], B, hp, wp, cpi, K, 1, h, w, T["c1"], ep_bias=T["tdense"], ep_bias_stride=cout)
    dev.group_norm_relu_bf16_map(T["c1"], B, cout, gs, h, w, T["sd2"], T["mu2"], dst=p2, drop=D["drop"])
    dev.conv_bf16_prepare_kernels(D["conv2"], A, cout, cout, K)
    dev.conv2d_gathered_bf16(A, cout, T["p2"], B, hp, wp, cpo, K, 1, h, w, T["c2"])
    r = D["x"].ptr
    if cin != cout:
        dev.conv2d_forward_as_bf16(D["x"], D["res"], T["res"], B, h, w, 1, cin, cout, 1)
        r = T["res"]
    chk(L.bla_sum_f32(None, T["result"], T["c2"], r, B * cout * hw))
    # backward
    Q2 = dev.empty((B, hq, wq, cpo), U16)
    dev.conv_bf16_pad(D["del_out"], Q2, B, cout, h, w, hq, wq, topq, leftq, dq)
    dev.conv2d_weight_gradient_gathered_bf16(Q2, hq, wq, cpo, topq, leftq, dq, T["p2"], hp, wp, cpo, B, K, 1, h, w, cout, cout, T["g_conv2"], splits)
    dev.conv_bf16_prepare_kernels(D["conv2"], A, cout, cout, K, True)
    dev.conv2d_gathered_bf16_chained(A, cout, Q2, B, hq, wq, cpo, K, 1, h, w, out_f32=T["g_out_a"], gate=p2)
    dev.group_norm_ddx_bf16_map(T["g_out_a"], T["c1"], T["mu2"], T["sd2"], B, cout, gs, h, w, dst=q1, dest_f32=T["g_out_b"])
    chk(L.bla_col_sum_f32(None, T["g_out_b"], B * cout, hw, T["dtb"], 1))                        # BLA_COLSUM_INTENDED
    dev.sync()
    dtb = T.t["dtb"].f32()
    tb = np.zeros(cout, F32)
    for b in range(B):                                                                         # acc = 0; acc += dtb[b], in image order
        tb = tb + dtb[b]
    chk(L.bla_memcpy_h2d(T["g_time_b"], tb.ctypes.data, tb.nbytes, None)); dev.sync()
    chk(L.bla_gemm_f32(None, 1, 0, TDIM, cout, B, D["temb"].ptr, TDIM, T["dtb"], cout, T["g_time_w"], cout, None))
    dev.conv2d_weight_gradient_gathered_bf16(T["q1"], hq, wq, cpo, topq, leftq, dq, T["p1"], hp, wp, cpi, B, K, 1, h, w, cout, cin, T["g_conv1"], splits)
    addend, g_res = D["del_out"].ptr, None
    if cin != cout:
        g_res = dev.empty((B, cin, h, w))
        dev.conv2d_backward_gathered_as_bf16(D["del_out"], D["x"], D["res"], T["g_res"], g_res, B, h, w, 1, cin, cout, 1, splits)
        addend = g_res.ptr
    dev.conv_bf16_prepare_kernels(D["conv1"], A, cout, cin, K, True)
    dev.conv2d_gathered_bf16_chained(A, cin, T["q1"], B, hq, wq, cpo, K, 1, h, w, out_f32=T["g_in"], gate=p1)
    chk(L.bla_group_norm_ddx_gated_batched_f32(None, B, T["g_in"], T["del_x"], D["x"].ptr, T["mu1"], T["sd1"], cin, gs, hw, None, addend))
    dev.sync()


_runs = {}


def both(dev, block):
    """the entries' and the composition's tensors, once per block"""
    if block not in _runs:
        D = device_inputs(dev, block)
        splits = SPLITS[BLOCKS.index(block)]
        E, Cm = Buffers(dev, block), Buffers(dev, block)
        run_entries(dev, block, D, E, splits)
        run_composition(dev, block, D, Cm, splits)
        _runs[block] = (D, {n: o.read() for n, o in E.t.items()}, {n: o.read() for n, o in Cm.t.items()})
    return _runs[block]


def live(block):
    skip = {"res", "g_res"} if block[1] == block[2] else set()
    return [n for n in ("mu1", "sd1", "c1", "tdense", "mu2", "sd2", "c2", "res", "result", "p1", "p2", "q1", "g_conv1", "g_conv2", "g_time_w", "g_time_b", "g_res",
                        "g_out_a", "g_out_b", "g_in", "dtb", "del_x") if n not in skip]


@pytest.mark.parametrize("block", BLOCKS, ids=block_id)
def test_entries_equal_the_composition_bit_for_bit(dev, block):
    _, got, want = both(dev, block)
    for n in live(block):
        assert np.array_equal(got[n], want[n]), n
        if n not in ("p1", "p2", "q1"):
            assert not np.isnan(got[n].view(F32)).any(), n + ": an element was left out"
    if block[1] == block[2]:
        assert (got["res"] == 0xFFFFFFFF).all() and (got["g_res"] == 0xFFFFFFFF).all()
    assert (got["p1"] != 0).any() and (got["p2"] != 0).any() and (got["q1"] != 0).any()


@pytest.mark.parametrize("block", BLOCKS, ids=block_id)
def test_against_the_unrounded_float64_block(dev, block):
    _, got, _ = both(dev, block)
    recorded, exact = block_differences(block)
    names = dict(result="result", del_x="del_x", conv1="g_conv1", conv2="g_conv2", time_w="g_time_w", time_b="g_time_b", res="g_res")
    measured = {n: normwise(got[names[n]].view(F32), exact[n]) for n in TENSORS if n in exact}
    print(block_id(block), "host", " ".join(f"{recorded[n]:.1e}" for n in measured), " device", " ".join(f"{measured[n]:.1e}" for n in measured))
    for n, d in measured.items():
        assert d <= 2 * recorded[n], (n, d, recorded[n])


@pytest.mark.parametrize("block", BLOCKS, ids=block_id)
def test_without_del_x(dev, block):
    """d_del_x = NULL: the same weight gradients, the residual kernel's included; the data gradients and the last norm gradient are not formed"""
    D, got, _ = both(dev, block)
    T = Buffers(dev, block)
    run_entries(dev, block, D, T, SPLITS[BLOCKS.index(block)], want_del_x=False)
    for n in live(block):
        if n in ("del_x", "g_in"):
            assert T.t[n].untouched(), n
        else:
            assert np.array_equal(T.t[n].read(), got[n]), n


def test_refusals_leave_the_outputs_untouched(dev):
    block = BLOCKS[1]
    B, cin, cout, h, w, gs = block
    D = device_inputs(dev, block)
    T = Buffers(dev, block)
    params, ws, grads, sc, maps = structs(dev, block, D, T)
    L = dev.lib()
    fwd = lambda batch=B, co=cout, m=C.byref(maps): L.bla_resnet_forward_batched_bf16(None, batch, D["x"].ptr, D["temb"].ptr, C.byref(params), D["drop"].ptr, C.byref(ws),
                                                                                     T["result"], h, w, cin, co, K, TDIM, gs, m)
    bwd = lambda batch=B, m=C.byref(maps), splits=0: L.bla_resnet_backward_batched_bf16(None, batch, D["del_out"].ptr, D["x"].ptr, D["temb"].ptr, C.byref(params), C.byref(ws),
                                                                                        C.byref(grads), C.byref(sc), T["dtb"], T["del_x"], h, w, cin, cout, K, TDIM, gs, m, splits)
    odd = dev.native.ResnetBf16Maps(T["p1"] + 2, T["p2"], T["q1"])
    for call in (lambda: fwd(batch=0), lambda: fwd(co=0), lambda: fwd(m=None), lambda: fwd(m=C.byref(odd)), lambda: bwd(batch=0), lambda: bwd(m=None), lambda: bwd(splits=-1),
                 lambda: bwd(m=C.byref(odd))):
        assert call() == 1
    dev.sync()
    for n, o in T.t.items():
        assert o.untouched(), n
