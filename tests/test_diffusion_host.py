"""CPU side of the diffusion training / sampling feature: the numpy restatement of the Philox4x32-10 streams include/bla.h defines (pinned to the
Random123 known-answer vectors; tests/test_diffusion_gpu.py holds the device to it), and the example program's two new verbs, `fit` and `sample`,
which must check their input files before any device call (so this runs without a GPU) and leave the reference's usage text alone."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

EX = os.path.join(ROOT, "examples")
BIN = os.path.join(EX, "cifar_unet_gpu")
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
TAG_U32, TAG_NORMAL, TAG_BERNOULLI = 0, 1, 2


def philox4x32_10(ctr, key):
    """ctr: uint32 [..., 4], key: uint32 [..., 2] -> uint32 [..., 4] (Salmon et al., SC'11; Random123's philox4x32 with 10 rounds)"""
    c = [np.asarray(ctr[..., i], np.uint64) for i in range(4)]
    k0, k1 = np.asarray(key[..., 0], np.uint64), np.asarray(key[..., 1], np.uint64)
    mask = np.uint64(0xFFFFFFFF)
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(W0)) & mask; k1 = (k1 + np.uint64(W1)) & mask
        p0 = np.uint64(M0) * c[0]; p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & mask]
    return np.stack(c, -1).astype(np.uint32)


def blocks(seed, offset, tag, first, count):
    """Philox blocks first .. first + count - 1 of the stream (seed, offset, tag): [count][4] words"""
    j = (np.uint64(offset) + np.arange(first, first + count, dtype=np.uint64))
    ctr = np.stack([j & np.uint64(0xFFFFFFFF), j >> np.uint64(32), np.full(count, tag, np.uint64), np.zeros(count, np.uint64)], -1)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)
    return philox4x32_10(ctr, np.broadcast_to(key, (count, 2)))


def stream_words(seed, offset, tag, n):
    return blocks(seed, offset, tag, 0, (n + 3) // 4).reshape(-1)[:n]


def rand_u32(n, seed, offset):
    return stream_words(seed, offset, TAG_U32, n)


def rand_bernoulli(n, p, seed, offset):
    thr = min(max(np.floor(np.float64(np.float32(p)) * 2.0 ** 32), 0), 2.0 ** 32)
    return (stream_words(seed, offset, TAG_BERNOULLI, n).astype(np.float64) < thr).astype(np.uint8)


def rand_normal(n, seed, offset, mean=0.0, stddev=1.0):
    """Box-Muller on (w0, w1), (w2, w3) with u = ((w >> 8) + 0.5) * 2^-24 rounded to fp32 as the device forms it; the rest in double"""
    w = blocks(seed, offset, TAG_NORMAL, 0, (n + 3) // 4)
    u = (((w >> 8).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)).astype(np.float64)
    r01, r23 = np.sqrt(-2 * np.log(u[:, 0])), np.sqrt(-2 * np.log(u[:, 2]))
    a01, a23 = 2 * np.pi * u[:, 1], 2 * np.pi * u[:, 3]
    z = np.stack([r01 * np.cos(a01), r01 * np.sin(a01), r23 * np.cos(a23), r23 * np.sin(a23)], -1).reshape(-1)[:n]
    return mean + stddev * z


def time_embedding(t, dim):
    """examples/cifar_unet_gpu.c time_embedding(): relu(sin / cos(t w_i)), w_i = exp(-ln(1e4) i / half), in double"""
    half = dim // 2
    out = np.zeros(dim)
    for i in range(half):
        w = np.exp(-np.log(10000.0) * i / half)
        out[i] = max(np.sin(t * w), 0.0); out[half + i] = max(np.cos(t * w), 0.0)
    return out.astype(np.float32)


def test_philox_known_answers():
    """Random123's known-answer vectors for philox4x32_10"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = philox4x32_10(np.array([ctr], np.uint64), np.array([key], np.uint64))[0]
        assert [int(v) for v in got] == list(want), [hex(int(v)) for v in got]


def test_stream_layout():
    """element i = word i % 4 of block offset + i / 4; the tags separate the streams; offsets past 2^32 carry into the counter's second word"""
    seed = 0x123456789ABCDEF0
    w = rand_u32(10, seed, 2 ** 32 - 1)
    b0 = philox4x32_10(np.array([[0xFFFFFFFF, 0, TAG_U32, 0]], np.uint64), np.array([[0x9ABCDEF0, 0x12345678]], np.uint64))[0]
    b1 = philox4x32_10(np.array([[0, 1, TAG_U32, 0]], np.uint64), np.array([[0x9ABCDEF0, 0x12345678]], np.uint64))[0]
    assert np.array_equal(w[:4], b0) and np.array_equal(w[4:8], b1)
    assert not np.array_equal(stream_words(seed, 0, TAG_U32, 8), stream_words(seed, 0, TAG_NORMAL, 8))
    z = rand_normal(1 << 16, 7, 0)
    assert abs(z.mean()) < 0.02 and abs(z.var() - 1) < 0.02
    d = rand_bernoulli(1 << 16, 0.1, 7, 0)
    assert abs(d.mean() - 0.1) < 0.01


@pytest.fixture(scope="module")
def prog(pkg):
    pkg.build_native()
    subprocess.check_call(["make", "-s", "-C", EX, "cifar_unet_gpu"])
    return BIN


def run(prog, args, cwd, env=None):
    e = dict(os.environ, **(env or {}))
    for k in ("BLA_CIFAR_DIR", "BLA_UNET_WEIGHTS", "BLA_UNET_RESUME", "BLA_CIFAR_BATCH"):
        if not env or k not in env:
            e.pop(k, None)
    return subprocess.run([prog] + args, cwd=str(cwd), env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def test_example_builds(prog):
    assert os.access(prog, os.X_OK)


def test_fit_names_the_missing_data_file(prog, tmp_path):
    r = run(prog, ["fit", "1", "4"], tmp_path)
    assert r.returncode != 0 and "Unrecognized argument" not in r.stdout
    assert "data/cifar/data_batch_1.bin" in r.stderr, r.stderr
    r = run(prog, ["fit", "1"], tmp_path, {"BLA_CIFAR_DIR": str(tmp_path / "elsewhere")})
    assert r.returncode != 0 and str(tmp_path / "elsewhere" / "data_batch_1.bin") in r.stderr, r.stderr


def test_fit_resume_names_the_missing_parameter_file(prog, tmp_path):
    (tmp_path / "data" / "cifar").mkdir(parents=True)
    np.zeros((4, 3073), np.uint8).tofile(tmp_path / "data" / "cifar" / "data_batch_1.bin")
    r = run(prog, ["fit", "1", "4"], tmp_path, {"BLA_UNET_RESUME": "1"})
    assert r.returncode != 0 and "Unrecognized argument" not in r.stdout
    assert "data/cifar_unet/down_1/resnet_1/conv_1.csv" in r.stderr, r.stderr


def test_sample_names_the_missing_parameter_file(prog, tmp_path):
    r = run(prog, ["sample", "2", str(tmp_path / "out")], tmp_path)
    assert r.returncode != 0 and "Unrecognized argument" not in r.stdout
    assert "data/cifar_unet/down_1/resnet_1/conv_1.csv" in r.stderr, r.stderr


def test_usage_text_is_still_the_references(prog, tmp_path):
    usage = "\trun [<num samples> (default 1)]\n\ttrain <num epochs>\n\tinit\n"
    r = run(prog, [], tmp_path)
    assert r.returncode == 1 and r.stdout == "Please supply an argument, options:\n" + usage
    r = run(prog, ["bogus"], tmp_path)
    assert r.returncode == 1 and r.stdout == "Unrecognized argument, options:\n" + usage
    r = run(prog, ["train"], tmp_path)
    assert r.returncode == 1 and r.stdout == "Please supply a number of epochs, usage:\n\ttrain <num_epochs>\n"
