"""Held-out evaluation on the device (include/bla.h: bla_diffusion_noise_at_f32, bla_diffusion_vlb_terms_f32, bla_diffusion_prior_kl_f32,
bla_diffusion_vlb_weights, bla_diffusion_eval_timesteps, bla_unet_evaluate_f32) against the float64 restatement of tests/test_eval_host.py, with the
schedule taken from bla_diffusion_schedule, and the example program's `eval` verb and fit's BLA_UNET_EVAL_EVERY at full size."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_diffusion_gpu import CFG, csv_files, diffusion, fetch, upload
from test_diffusion_host import time_embedding
from test_eval_host import EPS53, TS5, eval_timesteps, prior_kl, term_bound, vlb_inputs, vlb_terms, vlb_weights
from test_unet_model import build as unet_build, load_params

pytestmark = pytest.mark.gpu

EX = os.path.join(ROOT, "examples")
BIN = os.path.join(EX, "cifar_unet_gpu")
INVALID = 1
GUARD = -12345.678


@pytest.fixture(scope="module")
def L(pkg):
    pkg.init(0)
    return pkg.lib()


@pytest.fixture(scope="module")
def d1000(pkg, L):
    d, sched = diffusion(pkg, L, 1000)
    yield d, sched
    pkg.native.check(L.bla_diffusion_destroy(d))


def chk(pkg, status):
    pkg.native.check(status)


def put(pkg, a, mis=0):
    """a on the device, `mis` floats behind a 16-byte boundary; returns (the owning array, the data pointer)"""
    a = np.ascontiguousarray(a)
    buf = pkg.empty((a.size + 4,), a.dtype)
    upload(pkg, buf.ptr + a.itemsize * mis, a)
    return buf, buf.ptr + a.itemsize * mis


def guarded(pkg, n):
    buf = pkg.to_device(np.full(n + 2, GUARD), np.float64)
    return buf, buf.ptr + 8


def read_guarded(buf, n):
    v = buf.numpy()
    assert v[0] == GUARD and v[n + 1] == GUARD, "a guard double around the output was overwritten"
    return v[1:n + 1]


def run_terms(pkg, L, d, arrays, t_dev, t_const, mis, with_sqerr=True):
    x0, xt, eps, eps_hat = arrays
    B, F = x0.shape
    keep = [put(pkg, a, mis) for a in (x0, xt, eps, eps_hat)]
    dt = pkg.to_device(np.asarray(t_dev, np.int32), np.int32) if t_dev is not None else None
    tb, tp = guarded(pkg, B)
    sb, sp = guarded(pkg, B)
    chk(pkg, L.bla_diffusion_vlb_terms_f32(d, None, keep[0][1], keep[1][1], keep[2][1], keep[3][1], dt.ptr if dt is not None else None, t_const, B, F, tp,
                                           sp if with_sqerr else None))
    pkg.sync()
    return read_guarded(tb, B).copy(), read_guarded(sb, B).copy()


def compare_terms(sched, arrays, ts, terms, sqerr, s, tag):
    x0, xt, eps, eps_hat = arrays
    F = x0.shape[1]
    for b, t in enumerate(ts):
        want, want_sq, scale = vlb_terms(sched, int(t), x0[b], xt[b], eps[b], eps_hat[b])
        e_sq, e_t = abs(sqerr[b] - want_sq), abs(terms[b] - want)
        print(f"{tag} image {b} t {t}: term {terms[b]:.9g} off by {e_t:.2e} (bound {term_bound(int(t), F, scale):.2e}), sqerr off by {e_sq:.2e}")
        assert e_sq <= 2 * F * EPS53 * want_sq, (tag, b, t)
        assert e_t <= term_bound(int(t), F, scale), (tag, b, t)
        if s == 0:
            assert sqerr[b] == 0.0
            if t >= 1:
                c, _ = vlb_weights(sched, int(t))
                assert abs(terms[b] - F * c) <= 4 * EPS53 * abs(F * c), (tag, b, t)


# ---- 5: one term of the bound per image --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", [0.0, 0.3, 3.0])
@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("F,mis", [(3072, 0), (37, 0), (3072, 1)])
def test_vlb_terms(pkg, L, d1000, F, mis, batch, s):
    d, sched = d1000
    x0, xt, eps, eps_hat, t = vlb_inputs(sched, F, batch, s)
    arrays = (x0, xt, eps, eps_hat)
    terms, sqerr = run_terms(pkg, L, d, arrays, t, -5, mis)                      # the device timesteps win over t_const
    compare_terms(sched, arrays, t, terms, sqerr, s, "mixed")
    again, again_sq = run_terms(pkg, L, d, arrays, t, -5, mis)
    assert terms.tobytes() == again.tobytes() and sqerr.tobytes() == again_sq.tobytes()
    only, untouched = run_terms(pkg, L, d, arrays, t, 0, mis, with_sqerr=False)   # d_sqerr NULL
    assert only.tobytes() == terms.tobytes() and (untouched == GUARD).all()
    for tc in TS5:
        x0, xt, eps, eps_hat, t = vlb_inputs(sched, F, batch, s, ts=[tc])
        arrays = (x0, xt, eps, eps_hat)
        terms, sqerr = run_terms(pkg, L, d, arrays, None, tc, mis)
        compare_terms(sched, arrays, t, terms, sqerr, s, f"t_const {tc}")


def test_vlb_terms_floor_and_decoder_level(pkg, L, d1000):
    """What the issue measured on the CPU, on the device's own numbers: at s = 3 about 1 % of the t = 0 elements sit on the 1e-12 floor (the comparison
    above leaves none of them out), at s = 0 the decoder term is about 1.7 bits/dim"""
    d, sched = d1000
    x0, xt, eps, eps_hat, t = vlb_inputs(sched, 3072, 1, 0.0)
    terms, _ = run_terms(pkg, L, d, (x0, xt, eps, eps_hat), t, 0, 0)
    bpd = terms[0] / (3072 * math.log(2))
    print(f"decoder term at s = 0: {bpd:.3f} bits/dim")
    assert 1.5 <= bpd <= 1.9


def test_vlb_terms_bad_timesteps(pkg, L, d1000):
    d, sched = d1000
    x0, xt, eps, eps_hat, _ = vlb_inputs(sched, 3072, 5, 0.3)
    arrays = (x0, xt, eps, eps_hat)
    t = np.array([0, -1, 2, 1000, 999], np.int32)
    terms, sqerr = run_terms(pkg, L, d, arrays, t, 0, 0)
    assert np.isnan(terms[[1, 3]]).all() and (sqerr[[1, 3]] == 0).all()
    good = [0, 2, 4]
    compare_terms(sched, tuple(a[good] for a in arrays), t[good], terms[good], sqerr[good], 0.3, "beside bad t")
    keep = [put(pkg, a) for a in arrays]
    out = pkg.empty((5,), np.float64)
    for tc in (-1, 1000):
        assert L.bla_diffusion_vlb_terms_f32(d, None, keep[0][1], keep[1][1], keep[2][1], keep[3][1], None, tc, 5, 3072, out.ptr, None) == INVALID


# ---- 6: the prior term -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("batch", [1, 5])
@pytest.mark.parametrize("F,mis", [(3072, 0), (37, 0), (3072, 1)])
def test_prior_kl(pkg, L, d1000, F, mis, batch):
    d, sched = d1000
    x0 = vlb_inputs(sched, F, batch, 0.0)[0]
    keep, ptr = put(pkg, x0, mis)
    kb, kp = guarded(pkg, batch)
    chk(pkg, L.bla_diffusion_prior_kl_f32(d, None, ptr, batch, F, kp)); pkg.sync()
    got = read_guarded(kb, batch).copy()
    chk(pkg, L.bla_diffusion_prior_kl_f32(d, None, ptr, batch, F, kp)); pkg.sync()
    assert read_guarded(kb, batch).tobytes() == got.tobytes()
    for b in range(batch):
        want, scale = prior_kl(sched, x0[b])
        print(f"prior image {b}: {got[b]:.9g} off by {abs(got[b] - want):.2e} (bound {4 * F * EPS53 * scale:.2e})")
        assert abs(got[b] - want) <= 4 * F * EPS53 * scale


# ---- 7: noising at given timesteps -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F", [768, 7])
@pytest.mark.parametrize("mis", [0, 1])
def test_noise_at_equals_the_training_noise(pkg, L, d1000, F, mis):
    d, sched = d1000
    B, dim, seed, pas = 3, 24, 99, 5
    x0 = np.random.default_rng(3).uniform(-1, 1, (B, F)).astype(np.float32)
    keep, px0 = put(pkg, x0, mis)
    dt = pkg.empty((B,), np.int32)
    bufs = [pkg.to_device(np.full(B * F + 4, -7.0, np.float32)) for _ in range(4)]
    ptrs = [b.ptr + 4 * mis for b in bufs]
    temb, temb_at = pkg.empty((B, dim)), pkg.empty((B, dim))
    chk(pkg, L.bla_diffusion_noise_f32(d, None, px0, B, F, dim, seed, pas, dt.ptr, ptrs[0], ptrs[1], temb.ptr))
    chk(pkg, L.bla_diffusion_noise_at_f32(d, None, px0, B, F, dim, dt.ptr, -1, seed, pas << 32, ptrs[2], ptrs[3], temb_at.ptr))
    eps, xt, eps_at, xt_at = (fetch(pkg, p, B * F, np.float32) for p in ptrs)
    assert eps.tobytes() == eps_at.tobytes() and xt.tobytes() == xt_at.tobytes() and temb.numpy().tobytes() == temb_at.numpy().tobytes()
    for b in bufs[2:]:                                                            # nothing written outside [mis, mis + B F)
        v = b.numpy()
        assert (v[:mis] == -7).all() and (v[mis + B * F:] == -7).all()


@pytest.mark.parametrize("mis", [0, 1])
def test_noise_at_constant_timestep(pkg, L, d1000, mis):
    d, sched = d1000
    B, F, dim, seed, off = 3, 768, 24, 7, (4 << 32) + 11
    x0 = np.random.default_rng(4).uniform(-1, 1, (B, F)).astype(np.float32)
    keep, px0 = put(pkg, x0, mis)
    e_buf, x_buf, temb = pkg.empty((B * F + 4,)), pkg.empty((B * F + 4,)), pkg.empty((B, dim))
    pe, px = e_buf.ptr + 4 * mis, x_buf.ptr + 4 * mis
    ref = pkg.empty((B * F,))
    chk(pkg, L.bla_rand_normal_f32(None, ref.ptr, B * F, 0.0, 1.0, seed, off))
    for t in (0, 431, 999):
        chk(pkg, L.bla_diffusion_noise_at_f32(d, None, px0, B, F, dim, None, t, seed, off, pe, px, temb.ptr))
        e = fetch(pkg, pe, B * F, np.float32)
        assert e.tobytes() == ref.numpy().tobytes()
        a, c = np.float32(np.sqrt(sched[t, 1])), np.float32(np.sqrt(1 - sched[t, 1]))
        cz = c * e                                                                # fp32, rounded
        if mis:    # one element per lane: both products rounded
            want = a * x0.ravel() + cz
        else:      # the 16-byte body fuses the first product: a x is exact in double, one rounding of the sum (53 bits hold it: 48-bit product, fp32 addend)
            want = (np.float64(a) * x0.ravel().astype(np.float64) + cz.astype(np.float64)).astype(np.float32)
        assert fetch(pkg, px, B * F, np.float32).tobytes() == want.astype(np.float32).tobytes(), (t, mis)
        assert np.abs(temb.numpy() - np.stack([time_embedding(t, dim)] * B)).max() <= 1e-6
    for t in (-1, 1000):
        assert L.bla_diffusion_noise_at_f32(d, None, px0, B, F, dim, None, t, seed, off, pe, px, temb.ptr) == INVALID
    # a device timestep out of range: zero rows for that image alone
    dt = pkg.to_device(np.array([1000, 5, -1], np.int32), np.int32)
    chk(pkg, L.bla_diffusion_noise_at_f32(d, None, px0, B, F, dim, dt.ptr, 0, seed, off, pe, px, temb.ptr))
    xt, tb = fetch(pkg, px, B * F, np.float32).reshape(B, F), temb.numpy()
    assert (xt[[0, 2]] == 0).all() and (tb[[0, 2]] == 0).all() and np.abs(xt[1]).min() > 0 and np.abs(tb[1]).max() > 0
    assert fetch(pkg, pe, B * F, np.float32).tobytes() == ref.numpy().tobytes()


# ---- 8: the host helpers -----------------------------------------------------------------------------------------------------------------------------

def test_vlb_weights_and_eval_timesteps(pkg, L):
    for T in (2, 20, 1000):
        d, sched = diffusion(pkg, L, T)
        for t in range(1, T):
            c, w = C.c_double(), C.c_double()
            chk(pkg, L.bla_diffusion_vlb_weights(d, t, C.byref(c), C.byref(w)))
            assert (c.value, w.value) == vlb_weights(sched, t), (T, t)
        for t in (0, -1, T):
            assert L.bla_diffusion_vlb_weights(d, t, None, None) == INVALID
        for K in sorted({0, 1, min(T - 1, 4), min(T - 1, 50), T - 1}):
            out = (C.c_int * (K + 1))()
            chk(pkg, L.bla_diffusion_eval_timesteps(d, K, out))
            assert list(out) == eval_timesteps(T, K), (T, K)
        out = (C.c_int * (T + 1))()
        for K in (-1, T):
            assert L.bla_diffusion_eval_timesteps(d, K, out) == INVALID
        chk(pkg, L.bla_diffusion_destroy(d))


# ---- 9: the loop on the model's batch ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("conditional", [False, True])
def test_unet_evaluate_is_the_composition(pkg, L, conditional):
    B, T, dim, classes, seed, base = 4, 20, CFG["time_dim"], 10, 31, 7 * 192
    F = CFG["in_channels"] * CFG["image_h"] * CFG["image_w"]
    ts = [0, 3, 19]
    h, tensors = unet_build(pkg, CFG, B)
    load_params(pkg, h, tensors, CFG)
    d, sched = diffusion(pkg, L, T)
    x0 = pkg.to_device(vlb_inputs(sched, F, B, 0.0, ts=[0])[0])
    table = pkg.to_device(np.random.default_rng(8).uniform(-0.5, 0.5, (classes + 1, dim)).astype(np.float32)) if conditional else None
    rows = pkg.to_device(np.array([0, 3, classes, -1], np.int32), np.int32) if conditional else None    # the null row, and one that adds nothing
    terms, sqerr = pkg.empty((len(ts), B), np.float64), pkg.empty((len(ts), B), np.float64)
    cts = (C.c_int * len(ts))(*ts)

    def evaluate(sq):
        terms.fill_bytes(0xff); sq is None or sq.fill_bytes(0xff)
        chk(pkg, L.bla_unet_evaluate_f32(h, d, None, x0.ptr, cts, len(ts), seed, base, table.ptr if conditional else None, classes,
                                         rows.ptr if conditional else None, terms.ptr, sq.ptr if sq is not None else None))
        return terms.numpy(), sq.numpy() if sq is not None else None

    got, got_sq = evaluate(sqerr)
    assert np.isfinite(got).all() and np.isfinite(got_sq).all() and (got > 0).all()
    again, again_sq = evaluate(sqerr)
    assert got.tobytes() == again.tobytes() and got_sq.tobytes() == again_sq.tobytes()
    assert evaluate(None)[0].tobytes() == got.tobytes()
    # the same calls one by one
    eps, xt, temb, scratch = pkg.empty((B, F)), pkg.empty((B, F)), pkg.empty((B, dim)), pkg.empty((B,), np.int32)
    t1, s1 = pkg.empty((B,), np.float64), pkg.empty((B,), np.float64)
    for i, t in enumerate(ts):
        chk(pkg, L.bla_diffusion_noise_at_f32(d, None, x0.ptr, B, F, dim, None, t, seed, base + ((t + 1) << 32), eps.ptr, xt.ptr, temb.ptr))
        if conditional:
            chk(pkg, L.bla_class_embedding_f32(None, table.ptr, classes, rows.ptr, B, dim, 0.0, seed, 0, scratch.ptr, temb.ptr))
        chk(pkg, L.bla_unet_forward_f32(h, None, xt.ptr, temb.ptr, None))
        chk(pkg, L.bla_diffusion_vlb_terms_f32(d, None, x0.ptr, xt.ptr, eps.ptr, L.bla_unet_output(h), None, t, B, F, t1.ptr, s1.ptr))
        assert t1.numpy().tobytes() == got[i].tobytes() and s1.numpy().tobytes() == got_sq[i].tobytes(), t
    bad = (C.c_int * 2)(0, T)
    assert L.bla_unet_evaluate_f32(h, d, None, x0.ptr, bad, 2, seed, 0, None, 0, None, terms.ptr, None) == INVALID
    chk(pkg, L.bla_diffusion_destroy(d)); chk(pkg, L.bla_unet_destroy(h))


# ---- 10: the program ---------------------------------------------------------------------------------------------------------------------------------

FULL = dict(image_h=32, image_w=32, in_channels=3, dims=[128, 256, 256, 256], time_dim=512, kernel=3, group_size=32, key_dim=16)
# BLA_UNET_FULL_FILES=1: the file set holds every input channel, so the files alone say what the program's model holds
ENV = {"BLA_UNET_BATCH": "4", "BLA_DIFFUSION_STEPS": "20", "BLA_UNET_EVAL_STEPS": "4", "BLA_UNET_FULL_FILES": "1"}


def run(args, cwd, env, ok=True):
    e = dict(os.environ, **env)
    for k in ("BLA_CIFAR_DIR", "BLA_CIFAR_EVAL_FILE", "BLA_UNET_WEIGHTS", "BLA_UNET_RESUME", "BLA_UNET_INIT", "BLA_SEED", "BLA_UNET_BATCH", "BLA_UNET_CLASSES",
              "BLA_UNET_EVAL_EMA", "BLA_UNET_EVAL_EVERY", "BLA_UNET_EVAL_IMAGES", "BLA_UNET_EVAL_STEPS", "BLA_UNET_EMA"):
        if k not in env:
            e.pop(k, None)
    r = subprocess.run([BIN] + args, cwd=str(cwd), env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r


def tensor_file(name):
    """the file of the set that holds the device model's tensor `name` (examples/cifar_unet_gpu.c plan_model with BLA_UNET_FULL_FILES=1)"""
    if name == "output_conv_kernels":
        return "output_conv.csv"
    m = re.fullmatch(r"((?:down|up)_\d)_conv_kernels", name)
    if m:
        return os.path.join(m[1], "conv_0.csv")
    member, part = name.split(".")
    leaf = {"conv_1_kernels": "conv_1", "conv_2_kernels": "conv_2", "time_weights": "time_weight", "time_biases": "time_bias", "residual_conv_kernels": "conv_3",
            "Q_proj": "query", "K_proj": "key", "V_proj": "value", "weights": "weight", "biases": "bias"}[part]
    stage = "mid" if member.startswith("mid_") else member[:member.index("_", member.index("_") + 1)]
    block = member[len(stage) + 1:]
    return os.path.join(stage, "self_attention_0" if block == "self_attention" else block, leaf + ".csv")


@pytest.fixture(scope="module")
def fitted(pkg, tmp_path_factory):
    """`fit` on 16 synthetic records (as test_example_fit_with_ema_and_ddim_sample does it) and a synthetic evaluation file of 11 records"""
    subprocess.check_call(["make", "-s", "-C", EX, "cifar_unet_gpu"])
    tmp = tmp_path_factory.mktemp("eval")
    (tmp / "data" / "cifar").mkdir(parents=True)
    recs = np.random.default_rng(13).integers(0, 256, (16, 3073), dtype=np.uint8)
    recs[:, 0] = np.arange(16) % 10
    recs.tofile(tmp / "data" / "cifar" / "data_batch_1.bin")
    held = np.random.default_rng(14).integers(0, 256, (11, 3073), dtype=np.uint8)
    held[:, 0] = np.arange(11) % 10
    held.tofile(tmp / "data" / "cifar" / "test_batch.bin")
    plain = run(["fit", "1", "4"], tmp, ENV)
    with_eval = run(["fit", "1", "4"], tmp, dict(ENV, BLA_UNET_WEIGHTS=str(tmp / "w2"), BLA_UNET_EVAL_EVERY="1"))
    return tmp, held, plain, with_eval


def parse_eval(out):
    lines = out.splitlines()
    m0 = re.fullmatch(r"eval: (\d+) images, (\d+) steps, (\d+) of (\d+) KL terms", lines[0])
    m1 = re.fullmatch(r"Bits/dim: (\S+) \(prior (\S+), decoder (\S+), KL (\S+)\)", lines[1])
    assert m0 and m1 and lines[2].startswith("Eps MSE by timestep:") and len(lines) == 3, out
    mse = re.findall(r" t=(\d+) (\S+)", lines[2][len("Eps MSE by timestep:"):])
    return [int(v) for v in m0.groups()], [float(v) for v in m1.groups()], [(int(t), float(v)) for t, v in mse]


def test_example_eval(pkg, L, fitted):
    tmp, held, _, _ = fitted
    r = run(["eval", "8"], tmp, ENV)
    head, (total, prior, decoder, kl), mse = parse_eval(r.stdout)
    assert head == [8, 20, 4, 19] and [t for t, _ in mse] == eval_timesteps(20, 4)
    assert math.isfinite(total) and total > 0 and all(math.isfinite(v) and v > 0 for _, v in mse)
    assert abs(prior + decoder + kl - total) <= 2.01e-6               # four numbers printed with six decimals: each within 0.5e-6 of its value
    assert run(["eval", "8"], tmp, ENV).stdout == r.stdout
    assert parse_eval(run(["eval"], tmp, ENV).stdout)[0] == [8, 20, 4, 19]       # all 11 records: the last partial batch is dropped
    # the same number through the library: the same weight files, batch, seed and offsets, hence the same kernels on the same inputs
    B, T, K, F = 4, 20, 4, 3072
    files = csv_files(tmp / "data" / "cifar_unet")
    h, tensors = unet_build(pkg, FULL, B)
    flat = np.zeros(L.bla_unet_param_count(h), np.float32)
    for name, off, cnt in tensors:
        v = np.array(files[tensor_file(name)].decode().replace(",", " ").split(), np.float64).astype(np.float32)     # (float)atof, as the program reads it
        assert v.size == cnt, name
        flat[off:off + cnt] = v
    upload(pkg, L.bla_unet_params(h), flat)
    d, _ = diffusion(pkg, L, T)
    planes = held[:8, 1:].reshape(8, 3, 32, 32)[:, :, ::-1, :]                     # load_example: the planes' rows flipped
    x0 = pkg.to_device(((planes.astype(np.float64) - 127.5) / 127.5).astype(np.float32).reshape(8, F))
    ts = (C.c_int * (K + 1))()
    chk(pkg, L.bla_diffusion_eval_timesteps(d, K, ts))
    terms, pri = pkg.empty((K + 1, B), np.float64), pkg.empty((B,), np.float64)
    nats = np.zeros(3)
    for r0 in (0, 4):
        chk(pkg, L.bla_unet_evaluate_f32(h, d, None, x0.ptr + 4 * r0 * F, ts, K + 1, 42, r0 * F // 4, None, 0, None, terms.ptr, None))
        chk(pkg, L.bla_diffusion_prior_kl_f32(d, None, x0.ptr + 4 * r0 * F, B, F, pri.ptr))
        t = terms.numpy()
        nats += [pri.numpy().sum(), t[0].sum(), t[1:].sum() * (T - 1) / K]
    want = nats / (8 * F * math.log(2))
    print(f"eval 8: {total:.6f} bits/dim (prior {prior:.6f}, decoder {decoder:.6f}, KL {kl:.6f}); through the library {want.sum():.9f}")
    assert f"{want.sum():.6f}" == f"{total:.6f}" or abs(want.sum() - total) <= 1e-6       # (a sum in another order may round the last digit the other way)
    assert np.abs(want - [prior, decoder, kl]).max() <= 1e-6
    chk(pkg, L.bla_diffusion_destroy(d)); chk(pkg, L.bla_unet_destroy(h))


def test_example_eval_refusals(fitted):
    tmp = fitted[0]
    r = run(["eval", "8"], tmp, dict(ENV, BLA_UNET_EVAL_EMA="1"), ok=False)
    assert r.returncode == 1 and os.path.join("ema", "down_1", "resnet_1", "conv_1.csv") in r.stderr, r.stderr
    r = run(["eval", "8"], tmp, dict(ENV, BLA_CIFAR_EVAL_FILE=str(tmp / "nothing.bin")), ok=False)
    assert r.returncode == 1 and "nothing.bin" in r.stderr
    r = run(["eval", "8"], tmp, dict(ENV, BLA_UNET_EVAL_STEPS="20"), ok=False)
    assert r.returncode == 1 and "BLA_UNET_EVAL_STEPS" in r.stderr
    r = run(["eval", "3"], tmp, ENV, ok=False)
    assert r.returncode == 1 and "fewer than one batch" in r.stderr


def test_example_fit_reports_held_out_bits(fitted):
    tmp, _, plain, with_eval = fitted
    lines = with_eval.stdout.splitlines()
    held = [l for l in lines if l.startswith("Held-out bits/dim: ")]
    assert len(held) == 4 and all(math.isfinite(float(l.split()[-1])) and float(l.split()[-1]) > 0 for l in held), with_eval.stdout
    assert lines[-2].startswith("Pass 3:") and lines[-1] == held[-1]                # behind the loss line
    assert [l for l in lines if l not in held] == plain.stdout.splitlines()         # without the variable: fit's output as it is today ...
    assert csv_files(tmp / "w2") == csv_files(tmp / "data" / "cifar_unet")          # ... and the evaluation leaves the training untouched
    assert "Held-out" not in plain.stdout
