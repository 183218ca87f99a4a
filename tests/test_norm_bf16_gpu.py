"""bla_group_norm_relu_bf16_map and bla_group_norm_ddx_bf16_map on the device (include/bla.h).

Every output is a view inside an allocation pre-filled with 0xFF bytes (fp32: a NaN, bf16: 0xFFFF) with 64 guard elements on either side; an element the
kernels do not write fails its bound or its equality, and the guards must come back untouched.
* fp32 outputs (mean, variance, output, gradient) against float64 with the derived bounds of tests/test_group_norm_gpu.py -- `check_forward` and
  `check_gradient` of tests/test_norm_bf16_host.py, the functions its numpy restatement and its mutations are held to.  No element is left out.
* The map is exact: on the written set it equals bla_f32_to_bf16's rounding (include/bla.h, computed in numpy) of the fp32 output's bits, padding channels
  +0; every other element and the guards still hold 0xFFFF.  A call without the fp32 output gives the same map bits, a second call the same bits, and a
  second pass into a map zero-filled once leaves halo and holes zero.
* Shapes: the smallest at which each thing can go wrong (the table in the host file), one of them with every fp32 pointer one float off 16-byte
  alignment.  Destinations: the forward layout of a following k3 s1, k3 s2 (asymmetric padding) and k1 layer; for the gradient the data-gradient layouts
  with dilate 1 and 2.  Data: `uniform`, plus one forward case shifted to [1000, 1001).  Dropout decisions at p = 0.3 except in the k1 layout (no d_drop).
The worst fractions of the bounds are printed; measured on an MI355X (profiles/r19_resnet_bf16_tests.txt): mean <= 0.50, variance <= 0.18, output <= 0.43,
gradient <= 0.26."""
import numpy as np
import pytest

from test_norm_bf16_host import (CASES, SHIFTED, FORWARD_LAYOUTS, GRADIENT_LAYOUTS, FILL, case_id, check_forward, check_gradient, destination_layout, forward_inputs,
                                 gradient_inputs, group_slices, round8, written_set)

pytestmark = pytest.mark.gpu
F32, U8, U16, U32 = np.float32, np.uint8, np.uint16, np.uint32
GUARD = 64


@pytest.fixture(scope="module")
def dev(pkg):
    pkg.init(0)
    return pkg


class Out:
    """`shape` elements that start as 0xFF bytes with GUARD elements of the same pattern on either side; shift: elements by which the view is moved"""

    def __init__(self, dev, shape, dtype=F32, shift=0, fill=0xFF):
        self.shape, self.dtype = tuple(shape), np.dtype(dtype)
        self.bits = {2: U16, 4: U32}[self.dtype.itemsize]
        self.n, self.lo, self.fill = int(np.prod(shape)), GUARD + shift, self.bits(~self.bits(0)) if fill == 0xFF else self.bits(0)
        self.arr = dev.DeviceArray((self.n + 2 * GUARD + shift,), self.bits).fill_bytes(fill)
        self.ptr = self.arr.ptr + self.lo * self.dtype.itemsize

    def read(self):
        """the body; asserts the guards"""
        now = self.arr.numpy()
        assert (now[:self.lo] == self.fill).all() and (now[self.lo + self.n:] == self.fill).all(), "a guard element changed"
        return now[self.lo:self.lo + self.n].reshape(self.shape).view(self.dtype).copy()


def shifted_input(dev, a, shift):
    """a device copy of `a` that starts `shift` elements behind a 256-byte aligned base: (owner, address)"""
    flat = np.zeros(a.size + shift, a.dtype); flat[shift:] = a.ravel()
    d = dev.to_device(flat, a.dtype)
    return d, d.ptr + shift * a.dtype.itemsize


def run_forward(dev, case, name, x, drop, with_f32=True, dst=None):
    B, C_, gs, h, w, shift = case
    hp, wp, top, left, d = destination_layout(name, h, w)
    G = len(group_slices(C_, gs))
    keep = [shifted_input(dev, x, shift)]
    if drop is not None:
        keep.append(shifted_input(dev, drop.astype(U8), shift))
    mu, sd = Out(dev, (B, G), shift=shift), Out(dev, (B, G), shift=shift)
    out = Out(dev, x.shape, shift=shift) if with_f32 else None
    dst = dst or Out(dev, (B, hp, wp, round8(C_)), U16)
    dev.group_norm_relu_bf16_map(keep[0][1], B, C_, gs, h, w, sd.ptr, mu.ptr, dst=dev.conv_bf16_map(dst.ptr, hp, wp, round8(C_), top, left, d),
                                 out_f32=out.ptr if out else None, drop=keep[1][1] if drop is not None else None)
    dev.sync()
    return mu.read(), sd.read(), out.read() if out else None, dst


def forward_case(dev, case, name, lo=-1.0, hi=3.0):
    B, C_, gs, h, w, _ = case
    x, drop = forward_inputs(case, lo, hi)
    if name == "next_k1":
        drop = None
    lay = destination_layout(name, h, w)
    m, v, out, dst = run_forward(dev, case, name, x, drop)
    bits = dst.read()
    frac = check_forward(x, drop, m, v, out, bits, gs, lay, name)
    print(f"{case_id(case)} {name} [{lo}, {hi}): " + " ".join(f"{k} {f:.3f}" for k, f in frac.items()))
    assert max(frac.values()) <= 1.0, frac
    # the map alone: the same bits; and again: the same bits
    m2, v2, _, dst2 = run_forward(dev, case, name, x, drop, with_f32=False)
    assert np.array_equal(dst2.read(), bits) and np.array_equal(m2.view(U32), m.view(U32)) and np.array_equal(v2.view(U32), v.view(U32))
    m3, v3, out3, dst3 = run_forward(dev, case, name, x, drop)
    assert np.array_equal(dst3.read(), bits) and np.array_equal(out3.view(U32), out.view(U32)) and np.array_equal(m3.view(U32), m.view(U32))
    # two passes into a map zero-filled once: halo, holes and nothing else stay zero
    zmap = Out(dev, bits.shape, U16, fill=0)
    for _ in range(2):
        run_forward(dev, case, name, x, drop, with_f32=False, dst=zmap)
    z = zmap.read()
    ws = written_set(bits.shape, lay[2], lay[3], lay[4], h, w)
    assert (z[~ws] == 0).all() and np.array_equal(z[ws], bits[ws])


@pytest.mark.parametrize("name", FORWARD_LAYOUTS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_forward(dev, case, name):
    forward_case(dev, case, name)


def test_forward_shifted_data(dev):
    forward_case(dev, SHIFTED, "next_k3_s1", 1000.0, 1001.0)


def run_gradient(dev, case, name, I, with_f32=True, dst=None):
    B, C_, gs, h, w, shift = case
    hp, wp, top, left, d = destination_layout(name, h, w)
    source, data, m, v = I
    keep = [shifted_input(dev, a, shift) for a in (source, data, m, v)]
    dest = Out(dev, source.shape, shift=shift) if with_f32 else None
    dst = dst or Out(dev, (B, hp, wp, round8(C_)), U16)
    dev.group_norm_ddx_bf16_map(keep[0][1], keep[1][1], keep[2][1], keep[3][1], B, C_, gs, h, w, dst=dev.conv_bf16_map(dst.ptr, hp, wp, round8(C_), top, left, d),
                                dest_f32=dest.ptr if dest else None)
    dev.sync()
    return dest.read() if dest else None, dst


@pytest.mark.parametrize("name", GRADIENT_LAYOUTS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gradient(dev, case, name):
    B, C_, gs, h, w, _ = case
    I = gradient_inputs(case)
    lay = destination_layout(name, h, w)
    dest, dst = run_gradient(dev, case, name, I)
    bits = dst.read()
    frac = check_gradient(I[0], I[1], I[2], I[3], dest, bits, gs, lay, name)
    print(f"{case_id(case)} {name}: gradient {frac:.3f}")
    assert frac <= 1.0
    _, dst2 = run_gradient(dev, case, name, I, with_f32=False)
    assert np.array_equal(dst2.read(), bits)
    dest3, dst3 = run_gradient(dev, case, name, I)
    assert np.array_equal(dst3.read(), bits) and np.array_equal(dest3.view(U32), dest.view(U32))
    zmap = Out(dev, bits.shape, U16, fill=0)
    for _ in range(2):
        run_gradient(dev, case, name, I, with_f32=False, dst=zmap)
    z = zmap.read()
    ws = written_set(bits.shape, lay[2], lay[3], lay[4], h, w)
    assert (z[~ws] == 0).all() and np.array_equal(z[ws], bits[ws])


def test_fp32_output_alone(dev):
    """dst->d == NULL: the planar fp32 output only, inside the same bounds"""
    case = CASES[2]
    B, C_, gs, h, w, _ = case
    x, drop = forward_inputs(case)
    G = len(group_slices(C_, gs))
    xd, dd = dev.to_device(x), dev.to_device(drop.astype(U8), U8)
    mu, sd, out = Out(dev, (B, G)), Out(dev, (B, G)), Out(dev, x.shape)
    dev.group_norm_relu_bf16_map(xd, B, C_, gs, h, w, sd.ptr, mu.ptr, out_f32=out.ptr, drop=dd)
    dev.sync()
    assert max(check_forward(x, drop, mu.read(), sd.read(), out.read(), None, gs, None).values()) <= 1.0
    source, data, m, v = gradient_inputs(case)
    dest = Out(dev, x.shape)
    dev.group_norm_ddx_bf16_map(dev.to_device(source), dev.to_device(data), dev.to_device(m), dev.to_device(v), B, C_, gs, h, w, dest_f32=dest.ptr)
    dev.sync()
    assert check_gradient(source, data, m, v, dest.read(), None, gs, None) <= 1.0


def test_refusals_leave_the_outputs_untouched(dev):
    case = CASES[3]
    B, C_, gs, h, w, _ = case
    x, _ = forward_inputs(case)
    hp, wp, top, left, d = destination_layout("next_k3_s1", h, w)
    xd = dev.to_device(x)
    mu, sd, out, dst = Out(dev, (B, 2)), Out(dev, (B, 2)), Out(dev, x.shape), Out(dev, (B, hp, wp, C_), U16)
    for bad in (dict(cp=C_ + 8), dict(top=-1), dict(dilate=0), dict(hp=h), dict(d=dst.ptr + 2)):
        mp = dict(d=dst.ptr, hp=hp, wp=wp, cp=C_, top=top, left=left, dilate=d); mp.update(bad)
        with pytest.raises(dev.BlaError) as e:
            dev.group_norm_relu_bf16_map(xd, B, C_, gs, h, w, sd.ptr, mu.ptr, dst=dev.conv_bf16_map(**mp), out_f32=out.ptr)
        assert e.value.status == 1
        with pytest.raises(dev.BlaError) as e:
            dev.group_norm_ddx_bf16_map(xd, xd, mu.ptr, sd.ptr, B, C_, gs, h, w, dst=dev.conv_bf16_map(**mp), dest_f32=out.ptr)
        assert e.value.status == 1
    dev.sync()
    for o in (mu, sd, out, dst):
        assert (o.read().view(o.bits) == o.fill).all()
