"""The DDPM training recipe on the device (include/bla.h: bla_rand_permutation_u32, bla_diffusion_noise_gather_f32, bla_sumsq_accumulate_f32,
bla_clip_scale_f32, bla_adam_scaled_f32) against numpy / CPU torch restatements and against the entries they extend, and the example program's
`fit` with BLA_UNET_SHUFFLE, BLA_UNET_FLIP, BLA_ADAM_CLIP_NORM and BLA_ADAM_WARMUP."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from inputs import uniform
from test_diffusion_gpu import CFG, F, Trainer, chk, csv_files, diffusion, fetch, torch_adamw, upload
from test_diffusion_host import rand_bernoulli, rand_u32

pytestmark = pytest.mark.gpu

EX = os.path.join(ROOT, "examples")
BIN = os.path.join(EX, "cifar_unet_gpu")
INVALID = 1          # BLA_ERR_INVALID
FLIP_OFFSET = 2 ** 31 + 2 ** 30
UNET_PARAMS = 23_900_000      # the reference U-Net's bucket is this long to three digits; test_sumsq reads the exact count from the device


@pytest.fixture(scope="module")
def L(pkg):
    pkg.init(0)
    return pkg.lib()


# ---- 1: the permutation ---------------------------------------------------------------------------------------------------------------------

def test_permutation(pkg, L):
    seed, off = 42, 5 << 32
    for n in (1, 2, 5, 4099, 50000):
        out, keys = pkg.empty((n + 1,), np.uint32), pkg.empty((n + 1,), np.uint32)
        upload(pkg, out.ptr + 4 * n, np.array([0xABCD], np.uint32)); upload(pkg, keys.ptr + 4 * n, np.array([0xABCD], np.uint32))
        chk(pkg, L.bla_rand_permutation_u32(None, out.ptr, keys.ptr, n, seed, off))
        got, k = out.numpy(), keys.numpy()
        want_k = rand_u32(n, seed, off)
        if n == 50000:
            assert n - len(np.unique(want_k)) >= 1          # tied keys: the tie rule is exercised
        assert np.array_equal(k[:n], want_k), n
        assert np.array_equal(got[:n], np.argsort(want_k, kind="stable").astype(np.uint32)), n
        assert np.array_equal(np.sort(got[:n]), np.arange(n, dtype=np.uint32)), n
        assert got[n] == 0xABCD and k[n] == 0xABCD           # nothing written behind the n elements
        chk(pkg, L.bla_rand_permutation_u32(None, out.ptr, keys.ptr, n, seed, off))
        assert np.array_equal(out.numpy(), got) and np.array_equal(keys.numpy(), k)
    assert L.bla_rand_permutation_u32(None, out.ptr, keys.ptr, 2 ** 20 + 1, seed, off) == INVALID
    chk(pkg, L.bla_rand_permutation_u32(None, out.ptr, keys.ptr, 0, seed, off))
    assert np.array_equal(out.numpy(), got)


# ---- 2: batch assembly inside the noising launch --------------------------------------------------------------------------------------------

def gather(pkg, L, d, data, records, index, flip, width, labels, B, IF, dim, seed, pas, mis=0, with_x0=True):
    """bla_diffusion_noise_gather_f32 into fresh buffers; d_xt starts 4 * mis bytes behind a 16-byte boundary.  Returns t, eps, xt, temb, x0, labels_out"""
    dd = pkg.to_device(data)
    di = pkg.to_device(index, np.uint32) if index is not None else None
    dl = pkg.to_device(labels, np.int32) if labels is not None else None
    t, eps, xt, temb = pkg.empty((B,), np.int32), pkg.empty((B, IF)), pkg.empty((B * IF + 4,)), pkg.empty((B, dim))
    x0, lo = pkg.empty((B, IF)), pkg.to_device(np.full(B, 77, np.int32), np.int32)
    st = L.bla_diffusion_noise_gather_f32(d, None, dd.ptr, records, di.ptr if di else None, flip, width, dl.ptr if dl else None, lo.ptr if dl else None, B, IF, dim,
                                          seed, pas, t.ptr, eps.ptr, xt.ptr + 4 * mis, temb.ptr, x0.ptr if with_x0 else None)
    if st:
        return st
    return t.numpy(), eps.numpy(), fetch(pkg, xt.ptr + 4 * mis, B * IF, np.float32).reshape(B, IF), temb.numpy(), x0.numpy(), lo.numpy()


def plain(pkg, L, d, batch, dim, seed, pas, mis=0):
    """the existing bla_diffusion_noise_f32 on an assembled batch, with the same placement of d_xt"""
    B, IF = batch.shape
    dx = pkg.to_device(batch)
    t, eps, xt, temb = pkg.empty((B,), np.int32), pkg.empty((B, IF)), pkg.empty((B * IF + 4,)), pkg.empty((B, dim))
    chk(pkg, L.bla_diffusion_noise_f32(d, None, dx.ptr, B, IF, dim, seed, pas, t.ptr, eps.ptr, xt.ptr + 4 * mis, temb.ptr))
    return t.numpy(), eps.numpy(), fetch(pkg, xt.ptr + 4 * mis, B * IF, np.float32).reshape(B, IF), temb.numpy()


def assemble(data, index, flips, width):
    rows = data[index]
    mirrored = rows.reshape(len(index), -1, width)[:, :, ::-1].reshape(rows.shape)
    return np.where(flips[:, None] == 1, mirrored, rows).astype(np.float32)


@pytest.mark.parametrize("IF,width,mis", [(3072, 32, 0), (15, 5, 0), (3072, 32, 1)])
def test_noise_gather_equals_noise_on_the_assembled_batch(pkg, L, IF, width, mis):
    T, B, dim, seed, pas, records = 1000, 16, 24, 42, 3, 40
    d, _ = diffusion(pkg, L, T)
    data = uniform(61, (records, IF), -1, 1, np.float32)
    labels = (np.arange(records) * 7 % 10).astype(np.int32)
    index = np.random.default_rng(5).permutation(records)[:B].astype(np.uint32)
    flips = rand_bernoulli(B, 0.5, seed, (pas << 32) + FLIP_OFFSET)
    assert flips.tolist() == [1, 1, 0, 1, 1, 1, 1, 0, 0, 1, 0, 1, 0, 1, 0, 0]
    assert flips.any() and not flips.all()                 # both kinds occur
    batch = assemble(data, index, flips, width)
    got = gather(pkg, L, d, data, records, index, 1, width, labels, B, IF, dim, seed, pas, mis)
    want = plain(pkg, L, d, batch, dim, seed, pas, mis)
    for g, w, name in zip(got[:4], want, ("t", "eps", "xt", "temb")):
        assert np.array_equal(g, w), name
    assert np.array_equal(got[4], batch)
    assert np.array_equal(got[5], labels[index])
    # flip = 0: the same rows, nothing mirrored, the same noise
    got0 = gather(pkg, L, d, data, records, index, 0, width, labels, B, IF, dim, seed, pas, mis)
    want0 = plain(pkg, L, d, data[index], dim, seed, pas, mis)
    assert np.array_equal(got0[2], want0[2]) and np.array_equal(got0[4], data[index]) and np.array_equal(got0[1], got[1]) and np.array_equal(got0[0], got[0])
    chk(pkg, L.bla_diffusion_destroy(d))


def test_noise_gather_properties(pkg, L):
    T, B, dim, seed, pas, IF, width = 1000, 6, 24, 9, 11, 3072, 32
    d, sched = diffusion(pkg, L, T)
    data = uniform(62, (B, IF), -1, 1, np.float32)
    # no index, no flip, no d_x0: bla_diffusion_noise_f32 on d_data itself
    got = gather(pkg, L, d, data, B, None, 0, width, None, B, IF, dim, seed, pas, with_x0=False)
    want = plain(pkg, L, d, data, dim, seed, pas)
    for g, w in zip(got[:4], want):
        assert np.array_equal(g, w)
    assert (got[5] == 77).all()                            # no labels given: d_labels_out is not touched
    # an index equal to `records`: a zero image, pure scaled noise, label -1 -- on both paths
    for IFo, wo in ((3072, 32), (15, 5)):
        datao = uniform(63, (B, IFo), -1, 1, np.float32)
        index = np.array([0, B, 2, 1, B, 5], np.uint32)
        labels = np.arange(B, dtype=np.int32)
        t, eps, xt, temb, x0, lo = gather(pkg, L, d, datao, B, index, 1, wo, labels, B, IFo, dim, seed, pas)
        for b in (1, 4):
            assert not x0[b].any() and lo[b] == -1
            assert np.array_equal(xt[b], (np.float32(np.sqrt(1 - sched[t[b], 1])) * eps[b]).astype(np.float32))
        ok = [0, 2, 3, 5]
        assert np.array_equal(lo[ok], labels[index[ok]])
        flips = rand_bernoulli(B, 0.5, seed, (pas << 32) + FLIP_OFFSET)
        safe = np.where(index < B, index, 0)
        assert np.array_equal(x0[ok], assemble(datao, safe, flips, wo)[ok])
    assert gather(pkg, L, d, uniform(64, (B, 16), -1, 1, np.float32), B, None, 1, 5, None, B, 16, dim, seed, pas) == INVALID
    chk(pkg, L.bla_diffusion_destroy(d))


# ---- 3: the sum of squares ------------------------------------------------------------------------------------------------------------------

def unet_param_count(pkg, L):
    from test_unet_model import build as unet_build
    full = dict(image_h=32, image_w=32, in_channels=3, dims=[128, 256, 256, 256], time_dim=512, kernel=3, group_size=32, key_dim=16)
    h, _ = unet_build(pkg, full, 1)
    n = L.bla_unet_param_count(h)
    chk(pkg, L.bla_unet_destroy(h))
    return n


def test_sumsq(pkg, L):
    n_unet = unet_param_count(pkg, L)
    assert abs(n_unet - UNET_PARAMS) < 100_000
    acc, scratch = pkg.zeros((1,), np.float64), pkg.empty((1024,), np.float64)
    for n in (0, 1, 7, 1000003, n_unet):
        a = uniform(70 + n % 13, (n,), -3, 3, np.float32)
        want = float(np.sum(a.astype(np.float64) ** 2))
        buf = pkg.empty((n + 4,))
        for mis in (0, 1, 3):
            upload(pkg, buf.ptr + 4 * mis, a)
            acc.fill_bytes(0)
            chk(pkg, L.bla_sumsq_accumulate_f32(None, buf.ptr + 4 * mis, n, acc.ptr, scratch.ptr))
            got = float(acc.numpy()[0])
            rel = abs(got - want) / want if want else abs(got)
            print(f"sumsq n {n} misaligned {mis}: relative difference {rel:.2e} (bound {2 * n * 2.0 ** -53:.2e})")
            assert rel <= 2 * n * 2.0 ** -53, (n, mis, rel)
            acc.fill_bytes(0)
            chk(pkg, L.bla_sumsq_accumulate_f32(None, buf.ptr + 4 * mis, n, acc.ptr, scratch.ptr))
            assert float(acc.numpy()[0]) == got                    # run to run: the same bits
    # two buckets into one accumulator
    a, b = uniform(81, (100003,), -2, 2, np.float32), uniform(82, (5632,), -2, 2, np.float32)
    da, db = pkg.to_device(a), pkg.to_device(b)
    acc.fill_bytes(0)
    chk(pkg, L.bla_sumsq_accumulate_f32(None, da.ptr, a.size, acc.ptr, scratch.ptr))
    sa = float(acc.numpy()[0])
    chk(pkg, L.bla_sumsq_accumulate_f32(None, db.ptr, b.size, acc.ptr, scratch.ptr))
    both = float(acc.numpy()[0])
    acc.fill_bytes(0)
    chk(pkg, L.bla_sumsq_accumulate_f32(None, db.ptr, b.size, acc.ptr, scratch.ptr))
    sb = float(acc.numpy()[0])
    assert both == sa + sb
    want = float(np.sum(a.astype(np.float64) ** 2) + np.sum(b.astype(np.float64) ** 2))
    assert abs(both - want) / want <= 2 * (a.size + b.size) * 2.0 ** -53


# ---- 4: the clipping coefficient ------------------------------------------------------------------------------------------------------------

def clip_want(sumsq, gs, max_norm):
    gs, max_norm = np.float64(np.float32(gs)), np.float64(np.float32(max_norm))
    norm = abs(gs) * np.sqrt(np.float64(sumsq))
    return gs * min(1.0, max_norm / (norm + 1e-6)), norm


def within_one_ulp(got, want):
    w = np.float32(want)
    return np.nextafter(w, np.float32(-np.inf)) <= got <= np.nextafter(w, np.float32(np.inf))


def test_clip_scale(pkg, L):
    a = uniform(91, (100003,), -3, 3, np.float32)
    da, acc, scratch = pkg.to_device(a), pkg.zeros((1,), np.float64), pkg.empty((1024,), np.float64)
    chk(pkg, L.bla_sumsq_accumulate_f32(None, da.ptr, a.size, acc.ptr, scratch.ptr))
    sumsq = float(acc.numpy()[0])                                      # the fetched double sum
    scale, norm = pkg.empty((1,)), pkg.empty((1,))
    gs = 1.0 / 64
    for max_norm in (1.0, 0.37, 3.0):                                  # the norm is sqrt(3e5) / 64 = 8.6: above all three
        chk(pkg, L.bla_clip_scale_f32(None, acc.ptr, gs, max_norm, scale.ptr, norm.ptr))
        want, wn = clip_want(sumsq, gs, max_norm)
        got, gn = scale.numpy()[0], norm.numpy()[0]
        assert wn > max_norm and got < np.float32(gs)
        assert within_one_ulp(got, want), (got, want)
        assert within_one_ulp(gn, wn), (gn, wn)
    for max_norm in (9.0, 1e6):                                        # below: nothing is clipped, the scale is grad_scale exactly
        chk(pkg, L.bla_clip_scale_f32(None, acc.ptr, gs, max_norm, scale.ptr, None))
        assert clip_want(sumsq, gs, max_norm)[1] < max_norm and scale.numpy()[0] == np.float32(gs)
    chk(pkg, L.bla_clip_scale_f32(None, acc.ptr, -gs, 1.0, scale.ptr, norm.ptr))   # a negative grad_scale keeps its sign; the norm is |grad_scale| ...
    assert within_one_ulp(scale.numpy()[0], clip_want(sumsq, -gs, 1.0)[0]) and scale.numpy()[0] < 0 and norm.numpy()[0] > 0
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert L.bla_clip_scale_f32(None, acc.ptr, gs, bad, scale.ptr, norm.ptr) == INVALID, bad


# ---- 5: Adam with its grad_scale on the device ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_scaled_bit_equal_to_adam(pkg, L, wd):
    n, steps = 100003, 5
    f32 = lambda v: float(np.float32(v))
    lr, b1, b2, eps, wd = f32(2e-3), f32(0.9), f32(0.999), f32(1e-8), f32(wd)
    p0 = uniform(11, (n,), -1, 1, np.float32)
    grads = [uniform(100 + s, (n,), -3, 3, np.float32) for s in range(steps)]
    acc, scratch, scale = pkg.zeros((1,), np.float64), pkg.empty((1024,), np.float64), pkg.empty((1,))
    for mis in (0, 1):
        A = [pkg.zeros((n + 4,)) for _ in range(4)]       # p, g, m, v of bla_adam_scaled_f32
        Bk = [pkg.zeros((n + 4,)) for _ in range(4)]      # ... of bla_adam_f32
        at = lambda arrs: [x.ptr + 4 * mis for x in arrs]
        upload(pkg, at(A)[0], p0); upload(pkg, at(Bk)[0], p0)
        for s in range(steps):
            upload(pkg, at(A)[1], grads[s]); upload(pkg, at(Bk)[1], grads[s])
            acc.fill_bytes(0)
            chk(pkg, L.bla_sumsq_accumulate_f32(None, at(A)[1], n, acc.ptr, scratch.ptr))
            chk(pkg, L.bla_clip_scale_f32(None, acc.ptr, 1.0 / 64, 1.0, scale.ptr, None))
            fetched = float(scale.numpy()[0])
            assert 0 < fetched < 1.0 / 64
            chk(pkg, L.bla_adam_scaled_f32(None, *at(A), n, lr, b1, b2, eps, wd, scale.ptr, s + 1))
            chk(pkg, L.bla_adam_f32(None, *at(Bk), n, lr, b1, b2, eps, wd, fetched, s + 1))
        for k, name in ((0, "p"), (2, "m"), (3, "v")):
            assert np.array_equal(fetch(pkg, at(A)[k], n, np.float32), fetch(pkg, at(Bk)[k], n, np.float32)), (name, mis)
        assert np.abs(fetch(pkg, at(A)[0], n, np.float32) - p0).max() > 0


def test_clipped_training_pass_equals_cpu_clip_grad_norm_and_adamw(pkg, L):
    import torch
    lr = float(np.float32(2e-4))
    tr = Trainer(pkg, L, 3, lr)
    x0 = pkg.to_device(uniform(41, (3, F), -1, 1, np.float32))
    p0 = tr.params()
    tr.grads(x0, 0)
    g = fetch(pkg, L.bla_unet_grads(tr.h), tr.n, np.float32)
    mean_g = (np.float32(1.0 / 3) * g).astype(np.float32)
    measured = float(np.sqrt(np.sum(mean_g.astype(np.float64) ** 2)))
    max_norm = float(np.float32(measured / 4))                      # below the measured norm: the pass is clipped
    acc, scratch, scale, norm = pkg.zeros((1,), np.float64), pkg.empty((1024,), np.float64), pkg.empty((1,)), pkg.empty((1,))
    chk(pkg, L.bla_sumsq_accumulate_f32(None, L.bla_unet_grads(tr.h), tr.n, acc.ptr, scratch.ptr))
    chk(pkg, L.bla_clip_scale_f32(None, acc.ptr, 1.0 / 3, max_norm, scale.ptr, norm.ptr))
    chk(pkg, L.bla_adam_scaled_f32(None, L.bla_unet_params(tr.h), L.bla_unet_grads(tr.h), tr.m.ptr, tr.v.ptr, tr.n, lr, 0.9, 0.999, 1e-8, 0.0, scale.ptr, 1))
    got = tr.params()
    assert abs(float(norm.numpy()[0]) - measured) <= 1e-5 * measured
    gt = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    gt.grad = torch.from_numpy(mean_g.copy())
    torch.nn.utils.clip_grad_norm_([gt], max_norm)
    want = torch_adamw(p0, [gt.grad.numpy()], lr, (float(np.float32(0.9)), float(np.float32(0.999))), float(np.float32(1e-8)), 0.0)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"clipped pass vs clip_grad_norm_ + AdamW: {err:.2e} of max|p| (norm {measured:.4f}, max_norm {max_norm:.4f})")
    assert err <= 1e-6 and np.abs(got - p0).max() > 0, err
    tr.close()


# ---- 6: the example program -----------------------------------------------------------------------------------------------------------------

RECIPE = {"BLA_UNET_SHUFFLE": "1", "BLA_UNET_FLIP": "1", "BLA_ADAM_CLIP_NORM": "1.0", "BLA_ADAM_WARMUP": "3"}


def run(args, cwd, env):
    e = dict(os.environ, **env)
    for k in ("BLA_CIFAR_DIR", "BLA_UNET_WEIGHTS", "BLA_UNET_RESUME", "BLA_UNET_INIT", "BLA_SEED", "BLA_UNET_BATCH", "BLA_UNET_CLASSES", "BLA_UNET_EMA",
              "BLA_DIFFUSION_STEPS", "BLA_ADAM_LR", "BLA_UNET_LOG_EVERY") + tuple(RECIPE):
        if k not in env:
            e.pop(k, None)
    r = subprocess.run([BIN] + args, cwd=str(cwd), env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def test_example_fit_with_the_recipe(pkg, tmp_path):
    pkg.build_native()
    subprocess.check_call(["make", "-s", "-C", EX, "cifar_unet_gpu"])
    (tmp_path / "data" / "cifar").mkdir(parents=True)
    recs = np.random.default_rng(17).integers(0, 256, (16, 3073), dtype=np.uint8)
    recs[:, 0] = np.arange(16) % 10
    recs.tofile(tmp_path / "data" / "cifar" / "data_batch_1.bin")
    base = {"BLA_DIFFUSION_STEPS": "50", "BLA_UNET_LOG_EVERY": "1"}
    outs = {}
    for name, env in (("a", RECIPE), ("b", RECIPE), ("plain", {})):
        r = run(["fit", "2", "4"], tmp_path, dict(base, BLA_UNET_WEIGHTS=str(tmp_path / name), **env))
        losses = [l for l in r.stdout.splitlines() if l.startswith("Pass ")]
        norms = [l for l in r.stdout.splitlines() if l.startswith("Grad norm")]
        assert len(losses) == 8 and len(norms) == (8 if env else 0), r.stdout
        assert all(np.isfinite(float(l.split()[-1])) for l in losses + norms), r.stdout
        if env:
            assert all(float(l.split()[-1]) > 0 for l in norms), r.stdout
        outs[name] = (csv_files(tmp_path / name), r.stdout)
    assert len(outs["a"][0]) == 122
    assert outs["a"][0] == outs["b"][0] and outs["a"][1] == outs["b"][1]          # two runs: byte-identical sets (and logs)
    assert set(outs["a"][0]) == set(outs["plain"][0])
    changed = sum(outs["a"][0][k] != outs["plain"][0][k] for k in outs["plain"][0])
    assert changed >= 100, changed                                                 # the options are not ignored
    # each option on its own changes the result as well
    for k, v in RECIPE.items():
        run(["fit", "2", "4"], tmp_path, dict(base, BLA_UNET_WEIGHTS=str(tmp_path / k), **{k: v}))
        one = csv_files(tmp_path / k)
        assert sum(one[f] != outs["plain"][0][f] for f in one) >= 100, k
    # conditional: labels travel with the shuffled, flipped batch
    r = run(["fit", "2", "4"], tmp_path, dict(base, BLA_UNET_WEIGHTS=str(tmp_path / "c"), BLA_UNET_CLASSES="1", **RECIPE))
    cond = csv_files(tmp_path / "c")
    assert len(cond) == 123 and "class_embedding.csv" in cond
    lines = [l for l in r.stdout.splitlines() if l.startswith(("Pass ", "Grad norm"))]
    assert len(lines) == 16 and all(np.isfinite(float(l.split()[-1])) for l in lines), r.stdout
