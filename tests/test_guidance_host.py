"""CPU side of class-conditional diffusion: the example program's new options (BLA_UNET_CLASSES for `fit`, BLA_UNET_CLASS for `sample`) must
check their inputs before any device call, so a bad label, a class out of range or a missing class table ends the program with status 1 and a
message on a machine without a GPU."""
import os
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
    for k in ("BLA_CIFAR_DIR", "BLA_UNET_WEIGHTS", "BLA_UNET_RESUME", "BLA_CIFAR_BATCH", "BLA_UNET_CLASSES", "BLA_UNET_CLASS"):
        if k not in env:
            e.pop(k, None)
    return subprocess.run([prog] + args, cwd=str(cwd), env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def test_fit_rejects_a_label_above_nine(prog, tmp_path):
    (tmp_path / "data" / "cifar").mkdir(parents=True)
    recs = np.zeros((4, 3073), np.uint8)
    recs[:, 0] = [1, 9, 12, 0]
    recs.tofile(tmp_path / "data" / "cifar" / "data_batch_1.bin")
    r = run(prog, ["fit", "1", "4"], tmp_path, {"BLA_UNET_CLASSES": "1"})
    assert r.returncode == 1, r.stdout + r.stderr
    assert "record 2 has label 12" in r.stderr, r.stderr


def test_sample_rejects_a_class_out_of_range(prog, tmp_path):
    for bad in ("10", "-1", "3x"):
        r = run(prog, ["sample", "2", str(tmp_path / "out")], tmp_path, {"BLA_UNET_CLASS": bad})
        assert r.returncode == 1, r.stdout + r.stderr
        assert f"BLA_UNET_CLASS={bad}" in r.stderr and "0..9" in r.stderr, r.stderr


def test_sample_with_a_class_needs_the_table(prog, tmp_path):
    r = run(prog, ["sample", "2", str(tmp_path / "out")], tmp_path, {"BLA_UNET_CLASS": "3"})
    assert r.returncode == 1, r.stdout + r.stderr
    assert "data/cifar_unet/class_embedding.csv" in r.stderr, r.stderr
    r = run(prog, ["sample", "2", str(tmp_path / "out")], tmp_path, {"BLA_UNET_CLASS": "3", "BLA_UNET_WEIGHTS": str(tmp_path / "w")})
    assert r.returncode == 1 and str(tmp_path / "w" / "class_embedding.csv") in r.stderr, r.stderr
