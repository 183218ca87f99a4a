"""CPU side of DDIM sampling and the EMA of the weights: the example program's new options (BLA_UNET_SAMPLE_STEPS and BLA_UNET_ETA for `sample`,
BLA_UNET_EMA for `fit`) and a resumed EMA set are checked before any device call, so a bad value or an incomplete ema/ set ends the program with
status 1 and a message naming the cause on a machine without a GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

EX = os.path.join(ROOT, "examples")
BIN = os.path.join(EX, "cifar_unet_gpu")


@pytest.fixture(scope="module")
def prog(pkg):
    pkg.build_native()
    subprocess.check_call(["make", "-s", "-C", EX, "cifar_unet_gpu"])
    return BIN


def run(prog, args, cwd, env):
    e = dict(os.environ, **env)
    for k in ("BLA_CIFAR_DIR", "BLA_UNET_WEIGHTS", "BLA_UNET_RESUME", "BLA_CIFAR_BATCH", "BLA_UNET_CLASSES", "BLA_UNET_CLASS", "BLA_DIFFUSION_STEPS",
              "BLA_UNET_SAMPLE_STEPS", "BLA_UNET_ETA", "BLA_UNET_CLIP", "BLA_UNET_EMA"):
        if k not in env:
            e.pop(k, None)
    return subprocess.run([prog] + args, cwd=str(cwd), env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def test_sample_rejects_bad_sample_steps(prog, tmp_path):
    for bad, env in (("0", {}), ("-3", {}), ("x", {}), ("5s", {}), ("1001", {}), ("51", {"BLA_DIFFUSION_STEPS": "50"})):
        r = run(prog, ["sample", "2", str(tmp_path / "out")], tmp_path, dict(env, BLA_UNET_SAMPLE_STEPS=bad))
        assert r.returncode == 1, r.stdout + r.stderr
        assert f"BLA_UNET_SAMPLE_STEPS={bad}" in r.stderr, r.stderr
        assert not (tmp_path / "out").exists()


def test_sample_rejects_a_bad_eta(prog, tmp_path):
    for bad in ("-0.1", "1.5", "nan", "inf", "0.5x", "x"):
        for steps in ({"BLA_UNET_SAMPLE_STEPS": "5"}, {}):
            r = run(prog, ["sample", "2", str(tmp_path / "out")], tmp_path, dict(steps, BLA_UNET_ETA=bad))
            assert r.returncode == 1, r.stdout + r.stderr
            assert f"BLA_UNET_ETA={bad}" in r.stderr, r.stderr


def cifar(tmp_path):
    (tmp_path / "data" / "cifar").mkdir(parents=True)
    recs = np.zeros((8, 3073), np.uint8)
    recs[:, 0] = np.arange(8)
    recs.tofile(tmp_path / "data" / "cifar" / "data_batch_1.bin")


def test_fit_rejects_a_bad_decay(prog, tmp_path):
    cifar(tmp_path)
    for bad in ("0", "1", "1.5", "-0.5", "nan", "0.99x", "x"):
        r = run(prog, ["fit", "1", "4"], tmp_path, {"BLA_UNET_EMA": bad})
        assert r.returncode == 1, r.stdout + r.stderr
        assert f"BLA_UNET_EMA={bad}" in r.stderr, r.stderr


def test_fit_resume_names_the_missing_ema_file(prog, tmp_path):
    """`init` (host only) writes a complete set; a copy of it below ema/ with one file removed, or without the class table a conditional run
    needs, stops a resumed `fit` with the missing file's path"""
    cifar(tmp_path)
    w = tmp_path / "w"
    r = run(prog, ["init"], tmp_path, {"BLA_UNET_WEIGHTS": str(w)})
    assert r.returncode == 0, r.stdout + r.stderr
    shutil.copytree(w, tmp_path / "ema")
    shutil.move(str(tmp_path / "ema"), str(w / "ema"))
    env = {"BLA_UNET_WEIGHTS": str(w), "BLA_UNET_RESUME": "1", "BLA_UNET_EMA": "0.999"}
    missing = w / "ema" / "mid" / "resnet_2" / "time_bias.csv"
    missing.unlink()
    r = run(prog, ["fit", "1", "4"], tmp_path, env)
    assert r.returncode == 1, r.stdout + r.stderr
    assert str(missing) in r.stderr, r.stderr
    shutil.copy(w / "mid" / "resnet_2" / "time_bias.csv", missing)      # the set complete again; a conditional run also needs its class table
    r = run(prog, ["fit", "1", "4"], tmp_path, dict(env, BLA_UNET_CLASSES="1"))
    assert r.returncode == 1, r.stdout + r.stderr
    assert str(w / "ema" / "class_embedding.csv") in r.stderr, r.stderr
