"""The U-Net's glue kernels (csrc/bla_unet.hip) on the paths tests/test_unet_glue.py's one 6 x 8 x 8 tensor never takes.

* Select / add kernels (relu_mask, also in place; dropout; dropout_mask; sum): blocks_for() caps the grid at 2048 blocks of 256 threads, so only above
  524288 elements does a thread take a second trip of its grid-stride loop (524288 + 77: some threads two trips; 3 * 524288 + 1: three and four).  Bit for
  bit against the NumPy fp32 restatement; +0.0, -0.0 and negative values sit in the gates, which `<= 0` and `== 0` decide.
* Nearest-neighbour resize and its gradient: the float2 / float4 kernels of scale 2 (in_w / 2 = 1, 5 and 64; 65 x 128 x 64 pairs are more than the grid
  holds threads), the same shapes one float off their alignment (the general kernels must give the same bits), odd widths, cropped outputs (ragged blocks in
  the gradient), scales 3 and 1.  Forward: NumPy indexing, bit for bit.  Gradient: the fp32 oracle bit for bit (the same adds in the same order), and within
  4 * 2^-24 * sum |block| of the float64 sum.
* softmax_ddx: rows 1, 3, 5, 130 (last workgroup with idle waves; more than one workgroup) x dim 1, 63, 64, 65, 200, 1024 (the lane loop's second and later
  trips).  Reference: float64 s (g - <s, g>).  The kernel forms the dot in double and rounds it once, then one fp32 subtraction and one fp32 product: three
  roundings, |err| <= 4 * 2^-24 * |s| (|g| + |<s, g>|) + 1e-30 per element (derived, not measured).

Every output is a view between guard elements in an allocation filled with 0xFF bytes (tests/test_attention_bf16_gpu.py's pattern); the guards must come
back intact.  Ratios to the bounds are printed (profiles/r23_unet_paths_tests.txt)."""
import numpy as np
import pytest

from inputs import uniform

pytestmark = pytest.mark.gpu
F32, F64, U32 = np.float32, np.float64, np.uint32
GUARD = 64          # elements: 256 bytes, so an unshifted view keeps the allocation's alignment and `shift=1` is exactly one float off it
CAP = 2048 * 256    # blocks_for(): above this many elements (pairs, for the float2 kernels) the grid-stride loops take a second trip


@pytest.fixture(scope="module")
def dev(pkg):
    pkg.init(0)
    return pkg


class Guarded:
    """`shape` 4-byte elements with GUARD (+ shift) elements in front and GUARD behind, all 0xFF bytes; `init` fills the view itself"""

    def __init__(self, dev, shape, init=None, shift=0):
        self.dev, self.shape, self.n, self.lo = dev, tuple(shape), int(np.prod(shape)), GUARD + shift
        self.arr = dev.DeviceArray((self.n + 2 * GUARD + shift,), U32).fill_bytes(0xFF)
        self.ptr = self.arr.ptr + 4 * self.lo
        if init is not None:
            a = np.ascontiguousarray(init).view(U32).ravel()
            assert a.size == self.n
            host = np.full(self.arr.shape, 0xFFFFFFFF, U32); host[self.lo:self.lo + self.n] = a
            self.arr.copy_from(host)

    def bits(self):
        now = self.arr.numpy()
        assert (now[:self.lo] == 0xFFFFFFFF).all() and (now[self.lo + self.n:] == 0xFFFFFFFF).all(), "a guard element changed"
        return now[self.lo:self.lo + self.n].reshape(self.shape).copy()

    def f32(self):
        return self.bits().view(F32)

    def untouched(self):
        return bool((self.arr.numpy() == 0xFFFFFFFF).all())


def same_bits(got_bits, want):
    return np.array_equal(got_bits, np.ascontiguousarray(want, F32).view(U32).reshape(got_bits.shape))


def with_zeros(a, seed):
    """both zeros planted among the values (deterministic places, every size gets some once it has the room)"""
    a = a.copy(); n = a.size
    a[(np.arange(n) + seed) % 7 == 0] = F32(0.0)
    a[(np.arange(n) + seed) % 11 == 3] = F32(-0.0)
    return a


# ---- select and add kernels ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 256, 257, CAP + 77, 3 * CAP + 1])
def test_select_and_add_kernels(dev, n):
    L, chk = dev.lib(), dev.native.check
    zero = F32(0.0)
    src = with_zeros(uniform(4100, (n,), -1, 1, F32), 1)
    gate = with_zeros(uniform(4101, (n,), -1, 1, F32), 0)           # negative, +0.0, -0.0 -> 0; positive -> source
    if n > 256:
        assert (gate == 0).any() and np.signbit(gate[gate == 0]).any() and not np.signbit(gate[gate == 0]).all() and (gate < 0).any() and (gate > 0).any()
        assert np.signbit(src[(src == 0) & (gate > 0)]).any()      # a -0.0 that must come through as -0.0
    d_src, d_gate = dev.to_device(src), dev.to_device(gate)

    want = np.where(gate <= 0, zero, src)
    out = Guarded(dev, (n,))
    chk(L.bla_relu_mask_f32(None, out.ptr, d_src.ptr, d_gate.ptr, n)); assert same_bits(out.bits(), want), "relu_mask"
    inplace = Guarded(dev, (n,), init=src)
    chk(L.bla_relu_mask_f32(None, inplace.ptr, inplace.ptr, d_gate.ptr, n)); assert same_bits(inplace.bits(), want), "relu_mask in place"

    drop = (uniform(4102, (n,), 0, 1) < 0.3).astype(np.uint8) * np.array([1, 255, 2, 128], np.uint8)[np.arange(n) % 4]     # any non-zero byte drops
    d_drop = dev.to_device(drop, np.uint8)
    y = Guarded(dev, (n,))
    chk(L.bla_dropout_f32(None, d_src.ptr, y.ptr, d_drop.ptr, n))
    want_y = np.where(drop != 0, zero, src)
    assert same_bits(y.bits(), want_y), "dropout"

    # dropout_mask: zero where the forward result is +0.0 or -0.0 (want_y holds dropped zeros, planted zeros of both signs and values)
    g = uniform(4103, (n,), -1, 1, F32)
    gm = Guarded(dev, (n,), init=g)
    chk(L.bla_dropout_mask_f32(None, gm.ptr, y.ptr, n)); assert same_bits(gm.bits(), np.where(want_y == 0, zero, g)), "dropout_mask"
    gm2 = Guarded(dev, (n,), init=g)
    chk(L.bla_dropout_mask_f32(None, gm2.ptr, d_gate.ptr, n)); assert same_bits(gm2.bits(), np.where(gate == 0, zero, g)), "dropout_mask on signed values"

    b = with_zeros(uniform(4104, (n,), -1, 1, F32), 1)              # the same places as src: (+0) + (+0) and (-0) + (-0) = -0 among the sums
    total = Guarded(dev, (n,)); d_b = dev.to_device(b)
    chk(L.bla_sum_f32(None, total.ptr, d_src.ptr, d_b.ptr, n)); assert same_bits(total.bits(), src + b), "sum"


# ---- nearest-neighbour resize -------------------------------------------------------------------------------------------------------------------------
#          C   h    w     H    W  scale  fast (float2 / float4 kernels when aligned)
RESIZE = [(3, 1, 2, 2, 4, 2, True),
          (5, 6, 10, 12, 20, 2, True),            # in_w / 2 = 5
          (65, 128, 128, 256, 256, 2, True),      # 532480 pairs: past the grid cap
          (4, 5, 7, 10, 14, 2, False),            # odd width
          (4, 5, 7, 9, 13, 2, False),             # cropped: the gradient's last blocks are 1 high and 1 wide
          (2, 3, 2, 7, 5, 3, False),
          (2, 4, 4, 4, 4, 1, False)]
RESIZE_RUNS = [(cfg, 0) for cfg in RESIZE] + [(cfg, 1) for cfg in RESIZE if cfg[6]]


def shifted_input(dev, a, shift):
    """`a` on the device, `shift` floats behind the start of its allocation -> (array to keep alive, address)"""
    host = np.zeros(a.size + shift, F32); host[shift:] = a.ravel()
    arr = dev.to_device(host)
    return arr, arr.ptr + 4 * shift


@pytest.mark.parametrize("cfg,shift", RESIZE_RUNS, ids=lambda v: "x".join(map(str, v[:6])) if isinstance(v, tuple) else f"off{v}")
def test_nearest_neighbours_and_gradient(dev, ora, cfg, shift):
    """shift = 1: operands one float off their alignment, so the scale-2 shapes run on the general kernels -- and must give the same bits (both are compared
    with the same references)."""
    L, chk = dev.lib(), dev.native.check
    c, h, w, H, W, sc, fast = cfg
    if fast:
        assert (c * h * w // 2 > CAP) == (c == 65)
    x = uniform(4200 + c, (c, h, w), -1, 1, F32)
    keep, x_ptr = shifted_input(dev, x, shift)
    up = Guarded(dev, (c, H, W), shift=shift)
    aligned = x_ptr % 8 == 0 and up.ptr % 16 == 0
    assert aligned == (shift == 0)                      # the claim about which kernel runs rests on this
    chk(L.bla_nearest_neighbours_f32(None, x_ptr, up.ptr, c, h, w, H, W, sc))
    assert same_bits(up.bits(), x[:, (np.arange(H) // sc)[:, None], (np.arange(W) // sc)[None, :]]), "forward"

    gs = uniform(4300 + c, (c, H, W), -1, 1, F32)
    keep2, g_ptr = shifted_input(dev, gs, shift)
    dst = Guarded(dev, (c, h, w), shift=shift)
    assert (g_ptr % 16 == 0 and dst.ptr % 8 == 0) == (shift == 0)
    chk(L.bla_nearest_neighbours_ddx_f32(None, g_ptr, dst.ptr, c, H, W, h, w, sc))
    got = dst.bits()
    assert same_bits(got, ora.nearest_neighbours_ddx(gs, h, w, sc)), "gradient against the fp32 oracle"
    ref = ora.nearest_neighbours_ddx(gs.astype(F64), h, w, sc)
    bound = 4 * 2.0 ** -24 * ora.nearest_neighbours_ddx(np.abs(gs).astype(F64), h, w, sc)
    err = np.abs(got.view(F32).astype(F64) - ref)
    print(f"nearest_ddx {cfg[:6]} shift {shift}: worst |err| / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all()


def test_nearest_neighbours_refusals_leave_the_outputs_untouched(dev):
    L = dev.lib()
    c, h, w, sc = 2, 3, 2, 3
    x = dev.to_device(uniform(4400, (c, 14, 10), -1, 1, F32))
    out = Guarded(dev, (c, 14, 10))
    assert L.bla_nearest_neighbours_f32(None, x.ptr, out.ptr, c, h, w, 7, 5, sc) == 0 and not out.untouched()
    out = Guarded(dev, (c, 14, 10))
    assert L.bla_nearest_neighbours_f32(None, x.ptr, out.ptr, c, h, w, 14, 5, sc) == 1      # rows 9 .. 13 would read input rows 3 and 4
    assert L.bla_nearest_neighbours_f32(None, x.ptr, out.ptr, c, h, w, 7, 7, sc) == 1       # column 6 would read input column 2
    assert L.bla_nearest_neighbours_f32(None, x.ptr, out.ptr, c, h, w, 10, 6, sc) == 1      # one row and one column too many
    assert L.bla_nearest_neighbours_f32(None, x.ptr, out.ptr, c, h, w, 7, 5, 0) == 1
    assert L.bla_nearest_neighbours_ddx_f32(None, x.ptr, out.ptr, c, 14, 5, h, w, sc) == 1  # source rows 9 .. 13 have no destination row
    assert L.bla_nearest_neighbours_ddx_f32(None, x.ptr, out.ptr, c, 7, 7, h, w, sc) == 1
    assert L.bla_nearest_neighbours_ddx_f32(None, None, out.ptr, c, 7, 5, h, w, sc) == 1
    dev.sync()
    assert out.untouched()


# ---- softmax_ddx ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 63, 64, 65, 200, 1024])
@pytest.mark.parametrize("rows", [1, 3, 5, 130])
def test_softmax_ddx(dev, rows, dim):
    L, chk = dev.lib(), dev.native.check
    t = uniform(4500 + rows, (rows, dim), -4, 4)
    e = np.exp(t - t.max(axis=1, keepdims=True))
    s = (e / e.sum(axis=1, keepdims=True)).astype(F32)                  # a real row softmax, as the kernel receives it
    g = uniform(4600 + dim, (rows, dim), -1, 1, F32)
    out = Guarded(dev, (rows, dim)); d_s, d_g = dev.to_device(s), dev.to_device(g)
    chk(L.bla_softmax_ddx_f32(None, d_s.ptr, d_g.ptr, out.ptr, rows, dim))
    s64, g64 = s.astype(F64), g.astype(F64)
    dot = (s64 * g64).sum(axis=1, keepdims=True)
    ref = s64 * (g64 - dot)
    bound = 4 * 2.0 ** -24 * np.abs(s64) * (np.abs(g64) + np.abs(dot)) + 1e-30
    err = np.abs(out.f32().astype(F64) - ref)
    print(f"softmax_ddx {rows} x {dim}: worst |err| / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()


def test_softmax_ddx_of_nothing_writes_nothing(dev):
    L = dev.lib()
    s = dev.to_device(np.full((4, 8), 0.125, F32)); g = dev.to_device(uniform(4700, (4, 8), -1, 1, F32))
    out = Guarded(dev, (4, 8))
    assert L.bla_softmax_ddx_f32(None, s.ptr, g.ptr, out.ptr, 0, 8) == 0 and L.bla_softmax_ddx_f32(None, s.ptr, g.ptr, out.ptr, 4, 0) == 0
    assert L.bla_softmax_ddx_f32(None, s.ptr, g.ptr, out.ptr, 0, 0) == 0
    dev.sync()
    assert out.untouched()
