"""CPU side of the DDPM training recipe: `fit`'s four opt-in options (BLA_UNET_SHUFFLE, BLA_UNET_FLIP, BLA_ADAM_CLIP_NORM, BLA_ADAM_WARMUP) are checked
before any device call, so a bad value ends the program with status 1 and a message naming the variable and its value on a machine without a GPU."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

EX = os.path.join(ROOT, "examples")
BIN = os.path.join(EX, "cifar_unet_gpu")
OPTIONS = ("BLA_UNET_SHUFFLE", "BLA_UNET_FLIP", "BLA_ADAM_CLIP_NORM", "BLA_ADAM_WARMUP")


@pytest.fixture(scope="module")
def prog(pkg):
    pkg.build_native()
    subprocess.check_call(["make", "-s", "-C", EX, "cifar_unet_gpu"])
    return BIN


def run(prog, args, cwd, env):
    e = dict(os.environ, **env)
    for k in ("BLA_CIFAR_DIR", "BLA_UNET_WEIGHTS", "BLA_UNET_RESUME", "BLA_CIFAR_BATCH", "BLA_UNET_CLASSES", "BLA_DIFFUSION_STEPS", "BLA_UNET_EMA") + OPTIONS:
        if k not in env:
            e.pop(k, None)
    return subprocess.run([prog] + args, cwd=str(cwd), env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def cifar(tmp_path):
    (tmp_path / "data" / "cifar").mkdir(parents=True)
    recs = np.zeros((8, 3073), np.uint8)
    recs[:, 0] = np.arange(8)
    recs.tofile(tmp_path / "data" / "cifar" / "data_batch_1.bin")


BAD = {"BLA_UNET_SHUFFLE": ("-1", "nan", "x", "1x", "2", "yes"), "BLA_UNET_FLIP": ("-1", "nan", "x", "1x", "2", "true"),
       "BLA_ADAM_CLIP_NORM": ("0", "-1", "nan", "x", "1x", "inf", "1e60"), "BLA_ADAM_WARMUP": ("0", "-1", "nan", "x", "1x", "2.5")}


@pytest.mark.parametrize("name", OPTIONS)
def test_fit_rejects_bad_values(prog, tmp_path, name):
    cifar(tmp_path)
    good = {"BLA_UNET_SHUFFLE": "1", "BLA_UNET_FLIP": "1", "BLA_ADAM_CLIP_NORM": "1.0", "BLA_ADAM_WARMUP": "20"}
    for bad in BAD[name]:
        for others in ({}, {k: v for k, v in good.items() if k != name}):
            r = run(prog, ["fit", "1", "4"], tmp_path, dict(others, **{name: bad}))
            assert r.returncode == 1, (bad, r.stdout + r.stderr)
            assert f"{name}={bad}" in r.stderr, r.stderr
            assert "bla_init" not in r.stderr, r.stderr                        # stopped before the device was opened
            assert not (tmp_path / "data" / "cifar_unet").exists()


def test_fit_rejects_a_bad_value_before_it_reads_the_data(prog, tmp_path):
    """no data directory at all: the message names the option, not the missing file"""
    r = run(prog, ["fit", "1", "4"], tmp_path, {"BLA_ADAM_WARMUP": "0"})
    assert r.returncode == 1 and "BLA_ADAM_WARMUP=0" in r.stderr and "data_batch_1.bin" not in r.stderr, r.stderr


def test_good_values_pass_the_option_checks(prog, tmp_path):
    """accepted values get past the option checks: a resumed fit without a parameter set then stops at the first missing file (still before the device)"""
    cifar(tmp_path)
    for env in ({"BLA_UNET_SHUFFLE": "0", "BLA_UNET_FLIP": "0"}, {"BLA_UNET_SHUFFLE": "1", "BLA_UNET_FLIP": "1", "BLA_ADAM_CLIP_NORM": "0.5", "BLA_ADAM_WARMUP": "1"},
                {"BLA_ADAM_CLIP_NORM": "1e3", "BLA_ADAM_WARMUP": "5000"}, {"BLA_UNET_SHUFFLE": "", "BLA_ADAM_CLIP_NORM": ""}):
        r = run(prog, ["fit", "1", "4"], tmp_path, dict(env, BLA_UNET_RESUME="1"))
        assert r.returncode == 1 and "data/cifar_unet/down_1/resnet_1/conv_1.csv" in r.stderr, r.stdout + r.stderr
        assert not any(f"{k}=" in r.stderr for k in OPTIONS), r.stderr
