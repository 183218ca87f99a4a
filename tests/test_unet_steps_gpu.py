"""The U-Net's step list (csrc/bla_unet_model.hip: kNetwork and its three walkers) at the smallest configuration that has every kind of step --
tests/test_unet_model.py's: one absent and two present up-convolutions, residual 1 x 1s, all five attention blocks.  What a wrong walk would break and the
parity tests need not see: the tensor table as the create walk lays it out (written out here from tests/test_unet_bf16_host.py's tensor_list), the gradient
buffers' reuse across models and passes (bit-equal repeats, with the side lane's write-once pool and with the three rotating buffers), and the two seeds of
the backward walk."""
import numpy as np
import pytest

import test_unet_bf16_host as host
from test_unet_bf16_gpu import BF16, F32, Model, one_pass

pytestmark = pytest.mark.gpu

CFG = host.CFG
B = 2


def expected_table(cfg=CFG):
    """(name, offset, count): the tensors in forward order, each on a 4-float (16-byte) boundary"""
    table, off = [], 0
    for name, shp in host.tensor_list(cfg):
        cnt = int(np.prod(shp))
        table.append((name, off, cnt)); off += (cnt + 3) // 4 * 4
    return table, off


@pytest.fixture(scope="module")
def data(pkg):
    pkg.init(0)
    x, temb, noise, drop = host.make_inputs(batch=B)
    dd = host.device_drop_layout(drop)
    return dict(P=host.make_params(), x=pkg.to_device(x), temb=pkg.to_device(temb), noise=pkg.to_device(noise), noise_h=noise,
                drop=pkg.DeviceArray((dd.size,), np.uint8).copy_from(dd))


@pytest.mark.parametrize("products", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("batch", [1, 2])
def test_tensor_table_and_dropout_count(pkg, batch, products):
    pkg.init(0)
    m = Model(pkg, CFG, batch, products)
    table, total = expected_table()
    assert len(m.tensors) == len(table)
    for got, want in zip(m.tensors, table):
        assert got == want, (got, want)
    assert m.total == total
    assert pkg.lib().bla_unet_dropout_count(m.h) == sum(host.dropout_block_sizes()) * batch      # the 18 blocks' cout * h * w, image by image inside a block
    m.destroy()


@pytest.mark.parametrize("products", [F32, BF16], ids=["f32_side_lane", "bf16"])
def test_two_models_and_two_passes_give_the_same_bits(pkg, data, products):
    """fp32 at batch 2 runs its weight gradients on the side lane by default (every gradient write its own pool buffer), bf16 on three rotating buffers"""
    a, b = Model(pkg, CFG, B, products, data["P"]), Model(pkg, CFG, B, products, data["P"])
    (oa, ga), (ob, gb) = one_pass(a, data), one_pass(b, data)
    assert np.isfinite(oa).all() and np.isfinite(ga).all() and np.abs(ga).max() > 0
    assert np.array_equal(oa, ob) and np.array_equal(ga, gb)
    again_o, again_g = one_pass(a, data)
    assert np.array_equal(again_o, oa) and np.array_equal(again_g, ga)
    a.destroy(); b.destroy()


def test_backward_from_the_host_seed_is_backward_from_the_noise(pkg, data):
    m = Model(pkg, CFG, B, F32, data["P"])
    out, grads = one_pass(m, data)
    seed = pkg.to_device(np.float32(2) * (out - data["noise_h"]))      # unet_loss_grad_kernel's 2 (prediction - noise), in fp32
    m.forward(data["x"], data["temb"], data["drop"])
    pkg.native.check(pkg.lib().bla_unet_backward_from_f32(m.h, None, seed.ptr))
    assert np.abs(grads).max() > 0 and np.array_equal(m.grads(), grads)
    m.destroy()
