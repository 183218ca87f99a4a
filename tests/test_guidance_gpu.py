"""Class-conditional diffusion with classifier-free guidance on the device (include/bla.h: bla_unet_embedding_grad_f32, bla_class_embedding_f32,
bla_class_embedding_grad_f32, bla_diffusion_guided_step_f32, bla_unet_sample_guided_f32) against float64 numpy / CPU torch restatements, on the
narrow U-Net configuration of tests/test_diffusion_gpu.py, and the example program's conditional `fit` / guided `sample` at full size."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from inputs import uniform
from test_diffusion_gpu import CFG, F, csv_files, diffusion, fetch, numpy_step, run, torch_adamw, upload
from test_diffusion_host import rand_bernoulli, time_embedding
from test_unet_model import build as unet_build, load_params

pytestmark = pytest.mark.gpu

EX = os.path.join(ROOT, "examples")
BLA_ERR_INVALID = 1
CLASSES = 10


@pytest.fixture(scope="module")
def L(pkg):
    pkg.init(0)
    return pkg.lib()


def chk(pkg, status):
    pkg.native.check(status)


class Net:
    """a U-Net of the narrow configuration with parameters drawn as tests/test_unet_model.py draws them"""

    def __init__(self, pkg, L, B, cfg=CFG):
        self.pkg, self.L, self.B, self.cfg = pkg, L, B, cfg
        self.h, self.tensors = unet_build(pkg, cfg, B)
        self.P, self.n = load_params(pkg, self.h, self.tensors, cfg)
        self.tdim = cfg["time_dim"]
        self.x, self.temb, self.noise = pkg.empty((B, F)), pkg.empty((B, self.tdim)), pkg.empty((B, F))
        self.dtemb = pkg.empty((B, self.tdim))

    def inputs(self, seed):
        upload(self.pkg, self.x.ptr, uniform(seed, (self.B, F), -1, 1, np.float32))
        upload(self.pkg, self.temb.ptr, uniform(seed + 1, (self.B, self.tdim), 0, 1, np.float32))
        upload(self.pkg, self.noise.ptr, uniform(seed + 2, (self.B, F), -1, 1, np.float32))

    def forward(self, drop=None):
        chk(self.pkg, self.L.bla_unet_forward_f32(self.h, None, self.x.ptr, self.temb.ptr, drop))
        return fetch(self.pkg, self.L.bla_unet_output(self.h), self.B * F, np.float32).reshape(self.B, F)

    def backward(self):
        chk(self.pkg, self.L.bla_unet_backward_f32(self.h, None, self.noise.ptr))

    def embedding_grad(self):
        chk(self.pkg, self.L.bla_unet_embedding_grad_f32(self.h, None, self.dtemb.ptr))
        return self.dtemb.numpy().copy()

    def identity(self):
        """sum_k W_k . g_tb_k in float64 from the buckets: what sum_b dtemb[b] must be"""
        p = fetch(self.pkg, self.L.bla_unet_params(self.h), self.n, np.float32).astype(np.float64)
        g = fetch(self.pkg, self.L.bla_unet_grads(self.h), self.n, np.float32).astype(np.float64)
        at = {name: (off, cnt) for name, off, cnt in self.tensors}
        out = np.zeros(self.tdim)
        blocks = [name[:-len(".time_weights")] for name, _, _ in self.tensors if name.endswith(".time_weights")]
        assert len(blocks) == 18
        for b in blocks:
            wo, wc = at[b + ".time_weights"]; bo, bc = at[b + ".time_biases"]
            out += p[wo:wo + wc].reshape(self.tdim, bc) @ g[bo:bo + bc]
        return out

    def close(self):
        chk(self.pkg, self.L.bla_unet_destroy(self.h))


# ---- 1-4: the gradient of the time-embedding input -----------------------------------------------------------------------------------------

def test_embedding_grad_sum_over_images(pkg, L):
    net = Net(pkg, L, 3)
    net.inputs(61)
    drop = pkg.to_device(rand_bernoulli(L.bla_unet_dropout_count(net.h), 0.1, 7, 0), np.uint8)   # (kept alive until the pass has run)
    net.forward(drop.ptr); net.backward()
    got = net.embedding_grad().astype(np.float64).sum(0)
    want = net.identity()
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"sum_b dtemb[b] vs sum_k W_k g_tb_k: {err:.2e} of max |.| = {np.abs(want).max():.3e}")
    assert np.abs(want).max() > 0 and err <= 1e-5, err
    net.close()


def test_embedding_grad_per_image(pkg, L):
    net = Net(pkg, L, 3)
    net.inputs(62)
    pred = net.forward()
    noise = net.noise.numpy().copy()
    for j in range(3):
        n2 = pred.copy(); n2[j] = noise[j]                # del_Y = 2 (pred - noise) is exactly 0 for every image but j
        upload(pkg, net.noise.ptr, n2)
        net.backward()
        d = net.embedding_grad()
        others = [i for i in range(3) if i != j]
        assert (d[others] == 0).all(), j
        want = net.identity()
        err = np.abs(d[j].astype(np.float64) - want).max() / np.abs(want).max()
        assert np.abs(want).max() > 0 and err <= 1e-5, (j, err)
    net.close()


def loss(pred, noise):
    return float(((pred.astype(np.float64) - noise.astype(np.float64)) ** 2).sum())


def test_embedding_grad_finite_difference(pkg, L):
    """Central differences in fp32 on the device, no dropout, B = 1, L = sum (pred - noise)^2, 4 random unit directions v, h = 1e-2.

    The model's backward pass is the reference's intended one, and its group-norm gradient (lib/norm.c:52-93) is the derivative of a norm that
    divides by the standard deviation, while the forward pass divides by the variance.  So no gradient the backward pass forms --
    the parameters' nor this one -- is the derivative of the forward loss: measured on an MI355X, <dtemb, v> against (L(temb + h v) -
    L(temb - h v)) / 2h is off by 0.23 .. 0.71 of |<dtemb, v>| here (printed below; 0.1 .. 16 at B = 3).  What the embedding gradient can be held
    to is the backward pass's own derivative: moving temb by h v moves every block's projection temb . W_k + b_k exactly as moving its time
    biases by h v W_k does, so the central difference along v must equal the one along those bias offsets (the forward passes differ by the
    rounding of the projection only), and <dtemb, v> must equal the backward pass's own directional derivative sum_k <g_tb_k, v W_k>.
    Measured on an MI355X: the two central differences agree to 5.3e-4 of each other (worst of the 4) and the two derivatives to 1.3e-6; the
    bounds (1e-2, 1e-5) keep a margin and fail on an embedding gradient that is off by more than rounding."""
    net = Net(pkg, L, 1)
    net.inputs(63)
    temb0 = net.temb.numpy().copy()
    noise = net.noise.numpy().copy()
    net.forward(); net.backward()
    g = net.embedding_grad().astype(np.float64)[0]
    p0 = fetch(pkg, L.bla_unet_params(net.h), net.n, np.float32)
    grads = fetch(pkg, L.bla_unet_grads(net.h), net.n, np.float32).astype(np.float64)
    at = {name: (off, cnt) for name, off, cnt in net.tensors}
    blocks = [name[:-len(".time_weights")] for name, _, _ in net.tensors if name.endswith(".time_weights")]
    rng = np.random.default_rng(5)
    h, fd_gap, an_gap = 1e-2, [], []
    for _ in range(4):
        v = rng.standard_normal(temb0.shape[1]); v /= np.linalg.norm(v)
        upload(pkg, net.temb.ptr, (temb0 + h * v).astype(np.float32)); lp = loss(net.forward(), noise)
        upload(pkg, net.temb.ptr, (temb0 - h * v).astype(np.float32)); lm = loss(net.forward(), noise)
        upload(pkg, net.temb.ptr, temb0)
        fd_t, an = (lp - lm) / (2 * h), float(g @ v)
        an_b, lb = 0.0, []
        for sign in (1, -1):
            p = p0.copy()
            for b in blocks:
                wo, wc = at[b + ".time_weights"]; bo, bc = at[b + ".time_biases"]
                delta = v @ p0[wo:wo + wc].astype(np.float64).reshape(-1, bc)
                p[bo:bo + bc] = (p0[bo:bo + bc] + sign * h * delta).astype(np.float32)
                if sign == 1:
                    an_b += float(grads[bo:bo + bc] @ delta)
            upload(pkg, L.bla_unet_params(net.h), p)
            lb.append(loss(net.forward(), noise))
        upload(pkg, L.bla_unet_params(net.h), p0)
        fd_b = (lb[0] - lb[1]) / (2 * h)
        fd_gap.append(abs(fd_t - fd_b) / abs(fd_t)); an_gap.append(abs(an - an_b) / abs(an))
        print(f"<dtemb, v> = {an:+.6e} (backward's bias derivative {an_b:+.6e}); central differences along temb {fd_t:+.6e}, along the biases "
              f"{fd_b:+.6e}; <dtemb, v> vs the temb difference: {abs(an - fd_t) / abs(an):.2e}")
    print(f"central differences temb vs biases: worst {max(fd_gap):.2e}; <dtemb, v> vs sum_k <g_tb_k, v W_k>: worst {max(an_gap):.2e}")
    assert max(fd_gap) <= 1e-2 and max(an_gap) <= 1e-5, (fd_gap, an_gap)
    net.close()


def test_embedding_grad_batch1_deterministic_and_needs_backward(pkg, L):
    net = Net(pkg, L, 1)
    assert L.bla_unet_embedding_grad_f32(net.h, None, net.dtemb.ptr) == BLA_ERR_INVALID   # nothing has run
    net.inputs(64)
    net.forward()
    assert L.bla_unet_embedding_grad_f32(net.h, None, net.dtemb.ptr) == BLA_ERR_INVALID   # a forward pass, no backward since
    net.backward()
    a = net.embedding_grad(); b = net.embedding_grad()
    assert np.array_equal(a, b) and np.abs(a).max() > 0
    want = net.identity()
    assert np.abs(a[0].astype(np.float64) - want).max() <= 1e-5 * np.abs(want).max()
    net.forward()
    assert L.bla_unet_embedding_grad_f32(net.h, None, net.dtemb.ptr) == BLA_ERR_INVALID   # a new forward pass invalidates it
    net.close()
    # batched, twice bit-identical
    net = Net(pkg, L, 5)
    net.inputs(65); net.forward(); net.backward()
    assert np.array_equal(net.embedding_grad(), net.embedding_grad())
    net.close()


def test_embedding_grad_wide_time_embedding(pkg, L):
    """time_dim > 1024: the model forms its projections block by block (no one-launch time jobs); the embedding gradient still holds"""
    cfg = dict(CFG, time_dim=1100)
    for B in (1, 2):
        net = Net(pkg, L, B, cfg)
        net.inputs(66); net.forward(); net.backward()
        got = net.embedding_grad().astype(np.float64).sum(0)
        want = net.identity()
        assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max(), B
        net.close()


# ---- 5-6: class embedding and its gradient -------------------------------------------------------------------------------------------------

def test_class_embedding(pkg, L):
    B, dim, seed, off = 37, 24, 0x1234ABCD, (5 << 32) + (1 << 31)
    table = uniform(71, (CLASSES + 1, dim), -1, 1, np.float32)
    labels = np.random.default_rng(3).integers(0, CLASSES + 1, B).astype(np.int32)   # (label == classes: forced unconditional)
    temb0 = uniform(72, (B, dim), 0, 1, np.float32)
    dtab, dlab, rows, temb = pkg.to_device(table), pkg.to_device(labels, np.int32), pkg.empty((B,), np.int32), pkg.empty((B, dim))
    for p in (0.0, 0.3, 1.0):
        want_rows = np.where(rand_bernoulli(B, p, seed, off) == 1, CLASSES, labels).astype(np.int32)
        if p == 0.0:
            assert np.array_equal(want_rows, labels)
        if p == 1.0:
            assert (want_rows == CLASSES).all()
        for lab in (dlab.ptr, labels.ctypes.data):       # labels in device memory, then in host memory
            upload(pkg, temb.ptr, temb0)
            chk(pkg, L.bla_class_embedding_f32(None, dtab.ptr, CLASSES, lab, B, dim, p, seed, off, rows.ptr, temb.ptr)); pkg.sync()
            assert np.array_equal(rows.numpy(), want_rows), p
            assert np.array_equal(temb.numpy(), temb0 + table[want_rows]), p
    # a bad label from the host: refused before anything runs
    upload(pkg, temb.ptr, temb0)
    for bad in (CLASSES + 1, -1):
        lab = labels.copy(); lab[5] = bad
        assert L.bla_class_embedding_f32(None, dtab.ptr, CLASSES, lab.ctypes.data, B, dim, 0.0, seed, off, rows.ptr, temb.ptr) == BLA_ERR_INVALID
    assert np.array_equal(temb.numpy(), temb0)
    # ... from the device: row -1, that image's embedding untouched
    lab = labels.copy(); lab[5] = CLASSES + 3
    dbad = pkg.to_device(lab, np.int32)
    chk(pkg, L.bla_class_embedding_f32(None, dtab.ptr, CLASSES, dbad.ptr, B, dim, 0.0, seed, off, rows.ptr, temb.ptr)); pkg.sync()
    r = rows.numpy()
    assert r[5] == -1 and np.array_equal(np.delete(r, 5), np.delete(labels, 5))
    want = temb0 + table[np.maximum(labels, 0)]; want[5] = temb0[5]
    assert np.array_equal(temb.numpy(), want)


def test_class_embedding_grad_and_adam(pkg, L):
    B, dim = 13, 24
    dtemb = uniform(81, (B, dim), -2, 2, np.float32)
    rows = np.random.default_rng(4).choice([0, 2, 5, CLASSES], B).astype(np.int32)
    want = np.zeros((CLASSES + 1, dim), np.float32)
    for b in range(B):                                   # float32, images in order
        want[rows[b]] = want[rows[b]] + dtemb[b]
    g, dd, dr = pkg.to_device(np.full((CLASSES + 1, dim), 7, np.float32)), pkg.to_device(dtemb), pkg.to_device(rows, np.int32)
    chk(pkg, L.bla_class_embedding_grad_f32(None, dd.ptr, dr.ptr, B, CLASSES, dim, g.ptr)); pkg.sync()
    got = g.numpy()
    assert np.array_equal(got, want)
    unused = [k for k in range(CLASSES + 1) if k not in set(rows.tolist())]
    assert unused and (got[unused] == 0).all()
    # one Adam step on the table, grad_scale = 1 / B, against torch.optim.AdamW
    f32 = lambda v: float(np.float32(v))
    lr = f32(2e-4)
    t0 = uniform(82, (CLASSES + 1, dim), -1, 1, np.float32)
    tab, m, v = pkg.to_device(t0), pkg.zeros((CLASSES + 1, dim)), pkg.zeros((CLASSES + 1, dim))
    chk(pkg, L.bla_adam_f32(None, tab.ptr, g.ptr, m.ptr, v.ptr, t0.size, lr, 0.9, 0.999, 1e-8, 0.0, 1.0 / B, 1)); pkg.sync()
    ref = torch_adamw(t0.ravel(), [(np.float32(1.0 / B) * got.ravel()).astype(np.float32)], lr, (f32(0.9), f32(0.999)), f32(1e-8), 0.0)
    err = np.abs(tab.numpy().ravel() - ref).max() / np.abs(ref).max()
    assert err <= 1e-6, err


# ---- 7: the guided step ---------------------------------------------------------------------------------------------------------------------

def test_guided_step(pkg, L):
    T, B, dim, seed = 1000, 3, 24, 77
    d, sched = diffusion(pkg, L, T)
    table = uniform(91, (CLASSES + 1, dim), -1, 1, np.float32)
    rows = np.array([3, 10, 7, 10, 10, 10], np.int32)
    dtab, drows = pkg.to_device(table), pkg.to_device(rows, np.int32)
    for t in (T - 1, 431, 0):
        x = uniform(31 + t, (B, F), -2, 2, np.float32)
        ec = uniform(33 + t, (B, F), -2, 2, np.float32); eu = uniform(34 + t, (B, F), -2, 2, np.float32)
        z = pkg.empty((B * F,))
        chk(pkg, L.bla_rand_normal_f32(None, z.ptr, B * F, 0.0, 1.0, seed, (t + 1) << 32))
        zz = z.numpy().reshape(B, F).astype(np.float64) if t > 0 else 0.0
        dec, deu = pkg.to_device(ec), pkg.to_device(eu)
        for s in (0.0, 1.0, 3.0):
            dx, dcopy, tn = pkg.to_device(x), pkg.to_device(np.zeros((B, F), np.float32)), pkg.to_device(np.full((2 * B, dim), -7, np.float32))
            chk(pkg, L.bla_diffusion_guided_step_f32(d, None, dx.ptr, dcopy.ptr, dec.ptr, deu.ptr, s, B, F, t, seed, dim, tn.ptr, dtab.ptr, CLASSES, drows.ptr))
            got = dx.numpy()
            e = eu.astype(np.float64) + s * (ec.astype(np.float64) - eu.astype(np.float64))
            want = numpy_step(x, e, t, sched, zz)
            err = np.abs(got - want).max()
            assert err <= 2e-6 * max(1.0, np.abs(want).max()), (t, s, err)
            assert np.array_equal(dcopy.numpy(), got)
            if t > 0:
                emb = np.stack([time_embedding(t - 1, dim)] * (2 * B))
                assert np.abs(tn.numpy() - (emb + table[rows])).max() <= 2e-6, (t, s)
            else:
                assert (tn.numpy() == -7).all()
            if s == 0.0:                                 # the unguided step on eps_u, bit for bit
                ref = pkg.to_device(x)
                chk(pkg, L.bla_diffusion_step_f32(d, None, ref.ptr, deu.ptr, B, F, t, seed, dim, None))
                assert np.array_equal(ref.numpy(), got), t
    chk(pkg, L.bla_diffusion_destroy(d))


# ---- 8: the guided sampler ------------------------------------------------------------------------------------------------------------------

def test_guided_sampler(pkg, L):
    n, T, dim, s = 2, 5, CFG["time_dim"], 3.0
    h, tensors = unet_build(pkg, CFG, 2 * n)
    load_params(pkg, h, tensors, CFG)
    d, _ = diffusion(pkg, L, T)
    table = uniform(95, (CLASSES + 1, dim), -0.5, 0.5, np.float32)
    dtab = pkg.to_device(table)
    x = pkg.empty((n, F))

    def sample(seed, labels, host=False):
        lab = np.array(labels, np.int32)
        dlab = pkg.to_device(lab, np.int32)
        chk(pkg, L.bla_rand_normal_f32(None, x.ptr, n * F, 0.0, 1.0, seed, 0))
        chk(pkg, L.bla_unet_sample_guided_f32(h, d, None, x.ptr, dtab.ptr, CLASSES, lab.ctypes.data if host else dlab.ptr, s, seed))
        return x.numpy()

    got = sample(5, [3, 7])
    assert np.isfinite(got).all()
    assert np.array_equal(sample(5, [3, 7]), got)
    assert np.array_equal(sample(5, [3, 7], host=True), got)
    assert not np.array_equal(sample(6, [3, 7]), got)
    assert not np.array_equal(sample(5, [5, 7])[0], got[0])
    # a host label outside [0, classes] is refused before anything touches x
    chk(pkg, L.bla_rand_normal_f32(None, x.ptr, n * F, 0.0, 1.0, 5, 0))
    before = x.numpy()
    for bad in ([3, CLASSES + 1], [-1, 7]):
        lab = np.array(bad, np.int32)
        assert L.bla_unet_sample_guided_f32(h, d, None, x.ptr, dtab.ptr, CLASSES, lab.ctypes.data, s, 5) == BLA_ERR_INVALID, bad
        assert np.array_equal(x.numpy(), before), bad
    # the same loop composed from the public pieces: one batch-2n forward pass and the guided step per timestep -- bit-equal.  A device label outside
    # [0, classes] cannot be refused without a round trip: its image is sampled with no class row (row -1)
    x2, temb, rows = pkg.empty((2 * n, F)), pkg.empty((2 * n, dim)), pkg.empty((2 * n,), np.int32)
    out = L.bla_unet_output(h)
    for labels, want in (([3, 7], got), ([3, CLASSES + 5], sample(5, [3, CLASSES + 5]))):
        chk(pkg, L.bla_rand_normal_f32(None, x2.ptr, n * F, 0.0, 1.0, 5, 0))
        chk(pkg, L.bla_rand_normal_f32(None, x2.ptr + 4 * n * F, n * F, 0.0, 1.0, 5, 0))
        dts, dl2 = pkg.to_device(np.full(2 * n, T - 1, np.int32), np.int32), pkg.to_device(np.array(labels + [CLASSES, CLASSES], np.int32), np.int32)
        chk(pkg, L.bla_time_embedding_f32(None, dts.ptr, 2 * n, dim, temb.ptr))
        chk(pkg, L.bla_class_embedding_f32(None, dtab.ptr, CLASSES, dl2.ptr, 2 * n, dim, 0.0, 0, 0, rows.ptr, temb.ptr))
        assert rows.numpy().tolist() == [r if r <= CLASSES else -1 for r in labels] + [CLASSES, CLASSES]
        for t in range(T - 1, -1, -1):
            chk(pkg, L.bla_unet_forward_f32(h, None, x2.ptr, temb.ptr, None))
            chk(pkg, L.bla_diffusion_guided_step_f32(d, None, x2.ptr, x2.ptr + 4 * n * F, out, out + 4 * n * F, s, n, F, t, 5, dim, temb.ptr, dtab.ptr, CLASSES, rows.ptr))
        assert np.array_equal(x2.numpy()[:n], want), labels
    chk(pkg, L.bla_diffusion_destroy(d)); chk(pkg, L.bla_unet_destroy(h))
    # an odd model batch has no halves
    h3, _ = unet_build(pkg, CFG, 3)
    d, _ = diffusion(pkg, L, T)
    d1 = pkg.to_device(np.array([1], np.int32), np.int32)
    assert L.bla_unet_sample_guided_f32(h3, d, None, x.ptr, dtab.ptr, CLASSES, d1.ptr, s, 5) == BLA_ERR_INVALID
    chk(pkg, L.bla_diffusion_destroy(d)); chk(pkg, L.bla_unet_destroy(h3))


# ---- 9: the example program ---------------------------------------------------------------------------------------------------------------

def bmp_ok(a):
    return (len(a) == 3126 and a[:2] == b"BM" and int.from_bytes(a[2:6], "little") == 3126 and int.from_bytes(a[18:22], "little") == 32
            and int.from_bytes(a[22:26], "little") == 32 and int.from_bytes(a[28:30], "little") == 24)


def test_example_conditional_fit_and_guided_sample(pkg, tmp_path):
    pkg.build_native()
    subprocess.check_call(["make", "-s", "-C", EX, "cifar_unet_gpu"])
    (tmp_path / "data" / "cifar").mkdir(parents=True)
    recs = np.random.default_rng(12).integers(0, 256, (16, 3073), dtype=np.uint8)
    recs[:, 0] = np.arange(16) % 10
    recs.tofile(tmp_path / "data" / "cifar" / "data_batch_1.bin")
    r = run(["fit", "1", "4"], tmp_path, {"BLA_DIFFUSION_STEPS": "50", "BLA_UNET_LOG_EVERY": "1", "BLA_UNET_CLASSES": "1"})
    lines = [l for l in r.stdout.splitlines() if l.startswith("Pass ")]
    assert len(lines) == 4 and all(np.isfinite(float(l.split()[-1])) for l in lines), r.stdout
    files = csv_files(tmp_path / "data" / "cifar_unet")
    assert len(files) == 123 and "class_embedding.csv" in files
    table = np.array(files["class_embedding.csv"].decode().replace(",", " ").split(), np.float64)
    assert table.size == 11 * 512 and np.abs(table).max() > 0

    def sample(out, k):
        run(["sample", "2", str(tmp_path / out)], tmp_path, {"BLA_DIFFUSION_STEPS": "3", "BLA_UNET_CLASS": str(k)})
        assert sorted(os.listdir(tmp_path / out)) == ["sample_0000.bmp", "sample_0001.bmp"]
        return [open(tmp_path / out / f"sample_{i:04d}.bmp", "rb").read() for i in range(2)]

    a, b, c = sample("c3a", 3), sample("c3b", 3), sample("c5", 5)
    assert all(bmp_ok(v) for v in a + c)
    assert a == b and a != c
