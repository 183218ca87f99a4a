"""The mixed-precision U-Net on the device (bla_unet_create_mixed with BLA_UNET_PRODUCTS_BF16) against the float64 restatement of
tests/test_unet_bf16_host.py: configuration, parameters, inputs and the recorded rounded-against-exact values are that file's.  The bound is twice the
recorded value per tensor (DESIGN 3.25's practice), per image for the prediction and for the gradient summed over the three images."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import test_unet_bf16_host as host
from conftest import ROOT

pytestmark = pytest.mark.gpu

F32, BF16 = 0, 1
CFG, B = host.CFG, host.B


class Cfg(C.Structure):
    _fields_ = [("image_h", C.c_int), ("image_w", C.c_int), ("in_channels", C.c_int), ("dims", C.c_int * 4), ("time_dim", C.c_int), ("kernel", C.c_int),
                ("group_size", C.c_int), ("key_dim", C.c_int)]


def cfg_struct(cfg):
    return Cfg(cfg["image_h"], cfg["image_w"], cfg["in_channels"], (C.c_int * 4)(*cfg["dims"]), cfg["time_dim"], cfg["kernel"], cfg["group_size"], cfg["key_dim"])


class Model:
    """a device model with `flat` (the parameter bucket in tensor order, 16-byte aligned tensors) uploaded"""

    def __init__(self, pkg, cfg, batch, products, params=None, create=None):
        self.pkg, self.L, self.batch, self.cfg = pkg, pkg.lib(), batch, cfg
        L = self.L
        if create == "batched":
            self.h = C.c_void_p(); pkg.native.check(L.bla_unet_create_batched(C.byref(self.h), C.byref(cfg_struct(cfg)), batch))
        else:
            self.h = pkg.unet_create_mixed(cfg_struct(cfg), batch, products)
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

    def forward(self, x, temb, drop):
        self.pkg.native.check(self.L.bla_unet_forward_f32(self.h, None, x.ptr, temb.ptr, drop.ptr if drop is not None else None))

    def backward(self, noise):
        self.pkg.native.check(self.L.bla_unet_backward_f32(self.h, None, noise.ptr))

    def output(self):
        c = self.cfg
        out = np.empty((self.batch, c["in_channels"], c["image_h"], c["image_w"]), np.float32)
        self.pkg.native.check(self.L.bla_memcpy_d2h(out.ctypes.data, self.L.bla_unet_output(self.h), out.nbytes, None)); self.pkg.sync()
        return out

    def grads(self):
        g = np.empty(self.total, np.float32)
        self.pkg.native.check(self.L.bla_memcpy_d2h(g.ctypes.data, self.L.bla_unet_grads(self.h), g.nbytes, None)); self.pkg.sync()
        return g

    def destroy(self):
        self.pkg.native.check(self.L.bla_unet_destroy(self.h))


@pytest.fixture(scope="module")
def data(pkg):
    pkg.init(0)
    x, temb, noise, drop = host.make_inputs()
    dd = host.device_drop_layout(drop)
    return dict(P=host.make_params(), x=pkg.to_device(x), temb=pkg.to_device(temb), noise=pkg.to_device(noise), noise_h=noise,
                drop=pkg.DeviceArray((dd.size,), np.uint8).copy_from(dd))


def one_pass(m, data):
    m.forward(data["x"], data["temb"], data["drop"]); m.backward(data["noise"])
    return m.output(), m.grads()


@pytest.fixture(scope="module")
def bf16_pass(pkg, data):
    """one forward + backward pass of the bf16 model (default: the table launches), shared by the tests that only read it"""
    m = Model(pkg, CFG, B, BF16, data["P"])
    out, grads = one_pass(m, data)
    out.setflags(write=False); grads.setflags(write=False)
    yield m, out, grads
    m.destroy()


def test_symbols_mode_and_kernel(pkg, data, bf16_pass):
    L = pkg.lib()
    m, out, _ = bf16_pass
    assert L.bla_unet_products(m.h) == BF16 == pkg.UNET_PRODUCTS_BF16 and L.bla_unet_batch(m.h) == B
    f = Model(pkg, CFG, 2, F32)
    assert L.bla_unet_products(f.h) == F32 and pkg.unet_products(f.h) == F32
    f.destroy()
    m.forward(data["x"], data["temb"], data["drop"]); pkg.sync()
    assert L.bla_gemm_last_kernel().decode().startswith("conv_bf16_gather128x128x64_s1"), L.bla_gemm_last_kernel()
    assert np.array_equal(m.output(), out)
    m.backward(data["noise"]); pkg.sync()      # (leaves the shared model as the fixture made it)


def test_f32_mode_is_create_batched(pkg, data):
    a, b = Model(pkg, CFG, B, F32, data["P"]), Model(pkg, CFG, B, None, data["P"], create="batched")
    (oa, ga), (ob, gb) = one_pass(a, data), one_pass(b, data)
    assert np.isfinite(ga).all() and np.abs(ga).max() > 0
    assert np.array_equal(oa, ob) and np.array_equal(ga, gb)
    a.destroy(); b.destroy()


def test_against_the_float64_restatement(pkg, bf16_pass):
    """Measured on an MI355X (profiles/r20_unet_bf16_tests.txt): device / recorded 1.00 for the three predictions and 0.93 .. 1.03 (median 1.00)
    for the 103 gradient tensors; the device is 6e-8 (predictions) and 1.5e-7 .. 3.0e-3 (gradients, at most 0.37 of the recorded value) from the ROUNDED
    restatement.  On inputs for which the recorded values depend on the draw of the roundings (test_unet_bf16_host.make_params, requirement 3) four tensors of
    the 2 x 2 level lay at 2.1 .. 3.1 times their recorded value."""
    m, out, grads = bf16_pass
    exact, _, rec = host.recorded()
    assert np.isfinite(out).all() and np.isfinite(grads).all()
    rows = []
    for b in range(B):
        rows.append((f"prediction[{b}]", host.normwise(out[b], exact[0][b]), rec[f"prediction[{b}]"]))
    for name, off, cnt in m.tensors:
        g, w = grads[off:off + cnt].astype(np.float64), exact[1][name].ravel()
        if np.linalg.norm(w) == 0:
            assert name.endswith(".biases") and "attention" in name and not g.any(), name      # exactly zero, as in fp32 mode
            continue
        rows.append((name, host.normwise(g, w), rec[name]))
    for name, dev, hst in rows:
        print(f"{name:44s} device {dev:.3e}  host rounded-vs-exact {hst:.3e}  ratio {dev / hst:.2f}")
    bad = [(n, d, h) for n, d, h in rows if not d <= 2 * h]
    assert not bad, bad


def test_table_launch_in_place(pkg, data, bf16_pass):
    _, out, grads = bf16_pass
    keep = os.environ.get("BLA_UNET_BF16_PREP")
    os.environ["BLA_UNET_BF16_PREP"] = "0"
    try:
        m = Model(pkg, CFG, B, BF16, data["P"])      # the variable is read at this create call
    finally:
        if keep is None:
            del os.environ["BLA_UNET_BF16_PREP"]
        else:
            os.environ["BLA_UNET_BF16_PREP"] = keep
    o, g = one_pass(m, data)
    m.destroy()
    assert np.array_equal(o, out) and np.array_equal(g, grads)


def test_determinism_and_batch_one(pkg, data, bf16_pass):
    m, out, grads = bf16_pass
    for _ in range(2):
        o, g = one_pass(m, data)
        assert np.array_equal(o, out) and np.array_equal(g, grads)
    one = Model(pkg, CFG, 1, BF16, data["P"])
    x, temb, noise, drop = host.make_inputs()
    dx, dt, dn = pkg.to_device(x[0]), pkg.to_device(temb[0]), pkg.to_device(noise[0])
    dd = pkg.DeviceArray((drop.shape[1],), np.uint8).copy_from(drop[0])
    one.forward(dx, dt, dd); one.backward(dn)
    o1, g1 = one.output(), one.grads()
    assert np.isfinite(o1).all() and np.isfinite(g1).all() and np.abs(g1).max() > 0
    exact, _, rec = host.recorded()
    assert host.normwise(o1[0], exact[0][0]) <= 2 * rec["prediction[0]"]      # (the same image: the batch-1 model is the same network)
    one.destroy()


def test_everything_behind_the_pass(pkg, data, bf16_pass):
    L = pkg.lib(); chk = pkg.native.check
    m, out, grads = bf16_pass
    # bla_unet_backward_from_f32 seeded with 2 (output - noise) formed in fp32
    seed = pkg.to_device((np.float32(2) * (out - data["noise_h"])).astype(np.float32))
    m.forward(data["x"], data["temb"], data["drop"])
    chk(L.bla_unet_backward_from_f32(m.h, None, seed.ptr)); pkg.sync()
    assert np.array_equal(m.grads(), grads)
    # bla_unet_embedding_grad_f32 against sum_k W_k . g_tb_k of the restatement
    dtemb = pkg.empty((B, CFG["time_dim"]))
    chk(L.bla_unet_embedding_grad_f32(m.h, None, dtemb.ptr)); pkg.sync()
    exact, _, rec = host.recorded()
    e = host.normwise(dtemb.numpy(), exact[2])
    print(f"embedding gradient: device {e:.3e}  host rounded-vs-exact {rec['embedding_grad']:.3e}")
    assert e <= 2 * rec["embedding_grad"]
    # bla_unet_sample_ddim_f32, S = 2
    d = C.c_void_p(); chk(L.bla_diffusion_create(C.byref(d), 20, 1e-4, 0.02))
    f = Model(pkg, CFG, B, F32, data["P"])
    n = B * CFG["in_channels"] * CFG["image_h"] * CFG["image_w"]
    x = pkg.empty((n,))

    def sample(model):
        chk(L.bla_rand_normal_f32(None, x.ptr, n, 0.0, 1.0, 5, 0))
        chk(L.bla_unet_sample_ddim_f32(model.h, d, None, x.ptr, 2, 0.5, 1, 5))
        return x.numpy()
    got = sample(m)
    assert np.isfinite(got).all() and np.array_equal(sample(m), got) and not np.array_equal(sample(f), got)
    chk(L.bla_diffusion_destroy(d)); f.destroy()
    one_pass(m, data)      # (leaves the shared model as the fixture made it)


# ---- the C program -----------------------------------------------------------------------------------------------------------------------------------------
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from unet_refconst import CFG as REF_CFG, tensor_list as ref_tensor_list  # noqa: E402

EX = os.path.join(ROOT, "examples")


@pytest.fixture(scope="module")
def prog(pkg):
    pkg.build_native()
    subprocess.check_call(["make", "-s", "-C", EX, "cifar_unet_gpu"])
    return os.path.join(EX, "cifar_unet_gpu")


@pytest.mark.parametrize("products", [None, "bf16"])
def test_program_pass_is_the_library_pass(pkg, prog, tmp_path_factory, products):
    """tests/test_c_unet.py's one-training-pass flow (`train 1 2`, unit initialisation, time step 500, synthetic batch file): the gradients the program dumps
    are the library model's of that mode on the dumped parameters, images, embeddings, noise and dropout decisions, bit for bit -- bf16 with
    BLA_UNET_PRODUCTS=bf16, fp32 without the variable (the default, f32)."""
    pkg.init(0)
    tmp = tmp_path_factory.mktemp("c_unet_bf16")
    batch_file = str(tmp / "data_batch_1.bin")
    np.random.default_rng(11).integers(0, 256, (10000, 3073), dtype=np.uint8).tofile(batch_file)
    d = tmp / "dump"; d.mkdir()
    env = dict(os.environ, BLA_CIFAR_BATCH=batch_file, BLA_UNET_DUMP=str(d), BLA_UNET_INIT="unit", BLA_UNET_TIMESTEP="500")
    env.pop("BLA_UNET_PRODUCTS", None)
    if products:
        env["BLA_UNET_PRODUCTS"] = products
    r = subprocess.run([prog, "train", "1", "2"], cwd=str(tmp), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    flat = np.fromfile(d / "params.f32", np.float32)
    P, at = {}, 0
    for name, shp in ref_tensor_list(REF_CFG):
        n = int(np.prod(shp)); P[name] = flat[at:at + n]; at += n
    assert at == flat.size
    m = Model(pkg, REF_CFG, 2, BF16 if products == "bf16" else F32, P)
    x = pkg.to_device(np.fromfile(d / "x.f32", np.float32)); noise = pkg.to_device(np.fromfile(d / "noise.f32", np.float32))
    temb = pkg.to_device(np.fromfile(d / "temb.f32", np.float32))
    drop_h = np.fromfile(d / "drop.u8", np.uint8)
    drop = pkg.DeviceArray((drop_h.size,), np.uint8).copy_from(drop_h)
    m.forward(x, temb, drop); m.backward(noise)
    got = np.concatenate([m.grads()[off:off + cnt] for _, off, cnt in m.tensors])
    pred = m.output().ravel()
    m.destroy()
    assert np.isfinite(got).all() and np.abs(got).max() > 0
    assert np.array_equal(np.fromfile(d / "prediction.f32", np.float32), pred)
    assert np.array_equal(np.fromfile(d / "grads.f32", np.float32), got)
