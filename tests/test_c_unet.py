"""examples/cifar_unet_gpu.c -- the reference's CIFAR U-Net program (model/cifar_unet.c: init / train / run) as a C host program over the
batched device model.  CPU part (against what the reference built as oracle/_ref/libref_unet.so produced, recorded in tests/golden/c_programs.npz):
`init` writes byte for byte the 122 files the reference's own init() writes; the example, noise and dropout draws of `train` are the ones the
reference's own functions (init_parameters, load_example, random_gaussian, _dropout) make when called in train()'s / forward()'s order after srand(42).  GPU part: one
training pass of two images against the oracle composition on exactly the values the program uploaded; `run` from the as-written file set."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from unet_refconst import CFG, tensor_list  # noqa: E402

EX = os.path.join(ROOT, "examples")
BIN = os.path.join(EX, "cifar_unet_gpu")
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libref_unet.so")
IMAGE = 3 * 32 * 32


def needs_ref_build():
    return os.path.isdir("/root/reference") and os.path.exists(REF_SO)


@pytest.fixture(scope="module")
def prog(pkg):
    pkg.build_native()
    subprocess.check_call(["make", "-s", "-C", EX, "cifar_unet_gpu"])
    return BIN


@pytest.fixture(scope="module")
def batch_file(tmp_path_factory):
    """a CIFAR-10 batch file's shape (10,000 records of 1 label + 3,072 pixel bytes), random content"""
    path = tmp_path_factory.mktemp("cifar") / "data_batch_1.bin"
    np.random.default_rng(11).integers(0, 256, (10000, 3073), dtype=np.uint8).tofile(path)
    return str(path)


def run(prog, args, cwd, env=None, check=True):
    r = subprocess.run([prog] + args, cwd=str(cwd), env=dict(os.environ, **(env or {})), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    if check:
        assert r.returncode == 0, r.stdout + r.stderr
    return r


def block_sizes():
    D = CFG["dims"]; side = [32, 16, 8, 4]
    return [D[l] * side[l] * side[l] for l in [0, 0, 1, 1, 2, 2, 3, 3, 3, 3, 3, 3, 2, 2, 1, 1, 0, 0]]


def test_usage_messages_match_the_reference(prog, tmp_path):
    r = run(prog, [], tmp_path, check=False)
    assert r.returncode == 1 and r.stdout == "Please supply an argument, options:\n\trun [<num samples> (default 1)]\n\ttrain <num epochs>\n\tinit\n"
    r = run(prog, ["train"], tmp_path, check=False)
    assert r.returncode == 1 and r.stdout == "Please supply a number of epochs, usage:\n\ttrain <num_epochs>\n"
    r = run(prog, ["bogus"], tmp_path, check=False)
    assert r.returncode == 1 and r.stdout.startswith("Unrecognized argument, options:\n\trun [<num samples> (default 1)]")


REF_INIT = """
import ctypes as C
U = C.CDLL(%r)
U.cifar_unet_main(2, (C.c_char_p * 3)(b"cifar_unet", b"init", None))
"""


def init_tree(d):
    """Every directory and file `init` made under d (sorted relative paths) and the sha256 of each file (zeros for a directory)."""
    paths = sorted(os.path.relpath(os.path.join(r, f), d) for r, ds, fs in os.walk(d) for f in fs + ds)
    digs = [hashlib.sha256(open(os.path.join(d, p), "rb").read()).digest() if os.path.isfile(os.path.join(d, p)) else bytes(32) for p in paths]
    return np.array(paths), np.frombuffer(b"".join(digs), np.uint8).reshape(len(paths), 32)


def reference_init_tree(tmp):
    """model/cifar_unet.c's own main("init") (oracle/_ref/libref_unet.so, compiled from the reference's sources by oracle/Makefile)."""
    a = tmp / "theirs"
    (a / "data").mkdir(parents=True)
    subprocess.check_call([sys.executable, "-c", REF_INIT % REF_SO], cwd=str(a))
    return init_tree(a)


def test_init_writes_the_reference_files(prog, tmp_path):
    """`init` against the reference's own main("init"): the same directories, the same 122 files, the same bytes -- He / Xavier draws in
    init_parameters' order (:1804-1844) and save_parameters' as-written channel counts.  What the reference wrote (paths, sha256 of every
    file) is recorded in tests/golden/c_programs.npz (oracle/gen_golden.py); where the reference build exists it is run here as well and
    must still write exactly that."""
    rec = golden("c_programs")
    b = tmp_path / "ours"
    (b / "data").mkdir(parents=True)
    run(prog, ["init"], b)
    paths, digs = init_tree(b)
    assert list(paths) == list(rec["unet_init:paths"]) and sum(1 for p in paths if p.endswith(".csv")) == 122
    for p, got, want in zip(paths, digs, rec["unet_init:sha256"]):
        assert np.array_equal(got, want), p
    if needs_ref_build():
        tp, td = reference_init_tree(tmp_path)
        assert list(tp) == list(rec["unet_init:paths"]) and np.array_equal(td, rec["unet_init:sha256"]), "tests/golden/c_programs.npz differs from the reference's init"


REF_DRAWS = """
import ctypes as C, sys, numpy as np
sys.path.insert(0, %(oracle)r)
import ref
U = C.CDLL(%(so)r); libc = C.CDLL(None)
libc.rand.restype = C.c_int; U.random_gaussian.restype = C.c_double
libc.srand(42)                                            # main(), :1941
params = C.create_string_buffer(4096)                     # struct ModelParams: 49 pointers
U.allocate_model_params(params); U.init_parameters(params)      # train(), :1889,1900
fd = libc.open(%(batch)r.encode(), 0)
seed = C.c_uint(0)                                        # :1902
images = %(images)d; blocks = %(blocks)r
xs, noises, drops = [], [], [[] for _ in blocks]
for b in range(images):
    x = np.zeros((3, 32, 32)); U.load_example(ref.mats(x), fd)                                   # :1904
    xs.append(x.astype(np.float32))
    noises.append(np.array([U.random_gaussian(C.byref(seed)) for _ in range(3072)]).astype(np.float32))   # :1905-1914
    for k, (ch, side) in enumerate(blocks):                                                     # forward(): one _dropout per ResNet block, :1058
        ones = np.ones((ch, side, side)); y = np.zeros_like(ones)
        U._dropout(ref.mats(ones), ref.mats(y), ch)
        drops[k].append((y == 0).astype(np.uint8).ravel())
np.savez(%(out)r, x=np.stack(xs), noise=np.stack(noises), drop=np.concatenate([np.concatenate(d) for d in drops]), next_rand=libc.rand())
"""


DRAW_BLOCKS = [(c, s) for c, s in zip([128, 128] + [256] * 14 + [128, 128], [32, 32, 16, 16, 8, 8, 4, 4, 4, 4, 4, 4, 8, 8, 16, 16, 32, 32])]


def reference_draws(batch_file, tmp):
    """REF_DRAWS on two images of batch_file: x, noise, drop (one uint8 per dropout decision), next_rand."""
    out = str(tmp / "ref.npz")
    subprocess.check_call([sys.executable, "-c", REF_DRAWS % dict(oracle=os.path.join(ROOT, "oracle"), so=REF_SO, batch=batch_file, images=2, blocks=DRAW_BLOCKS, out=out)])
    z = np.load(out)
    return {k: z[k] for k in z.files}


def recorded_draws():
    rec = golden("c_programs")
    return {"x": rec["unet_draws:x"], "noise": rec["unet_draws:noise"], "next_rand": rec["unet_draws:next_rand"],
            "drop": np.unpackbits(rec["unet_draws:drop_bits"])[:int(rec["unet_draws:drop_len"])]}


def test_draws_are_the_reference_functions_draws(prog, batch_file, tmp_path):
    """What `train 1 2` hands the device against the reference's own functions called in the reference's order (in a fresh process: random_gaussian
    keeps a static spare value): pixels -> [-1, 1], the Gaussian noise of rand_r(&seed), every dropout decision, and the NEXT rand() value --
    so the number of draws agrees as well as their order.  The reference's draws on this batch file are recorded in tests/golden/c_programs.npz
    (oracle/gen_golden.py); where the reference build exists they are drawn again here and must still be those."""
    blocks = DRAW_BLOCKS
    want = recorded_draws()
    if needs_ref_build():
        live = reference_draws(batch_file, tmp_path)
        for k in want:
            assert np.array_equal(live[k], want[k]), f"{k}: tests/golden/c_programs.npz differs from the reference's draws"
    d = tmp_path / "ours"; d.mkdir()
    r = run(prog, ["draws", "2", str(d)], tmp_path, env=dict(BLA_CIFAR_BATCH=batch_file))
    words = r.stdout.split()
    assert int(words[words.index("next_rand") + 1]) == int(want["next_rand"])
    assert int(words[words.index("drop_per_image") + 1]) == sum(block_sizes()) == sum(c * s * s for c, s in blocks)
    x = np.fromfile(d / "x.f32", np.float32).reshape(2, 3, 32, 32); noise = np.fromfile(d / "noise.f32", np.float32).reshape(2, 3072)
    drop = np.fromfile(d / "drop.u8", np.uint8)
    assert np.array_equal(x, want["x"]) and np.abs(x).max() <= 1 and len(np.unique(x)) > 200
    assert np.array_equal(noise, want["noise"])
    assert np.array_equal(drop, want["drop"]) and 0.09 < drop.mean() < 0.11                       # block by block, inside a block image by image
    # the parameters the program would upload: the tensors of the device model, He / Xavier ranges of the reference's fan-in convention
    flat = np.fromfile(d / "params.f32", np.float32)
    names = tensor_list(CFG)
    assert flat.size == sum(int(np.prod(s)) for _, s in names)
    at = 0
    for name, shp in names:
        v = flat[at:at + int(np.prod(shp))]; at += v.size
        stage = name.split("_resnet")[0].split("_self")[0].split("_conv")[0]
        side = {"down_1": 32, "down_2": 16, "down_3": 8, "down_4": 4, "mid": 4, "up_1": 4, "up_2": 8, "up_3": 16, "up_4": 32, "output": 32}[stage]
        if name in ("up_1_conv_kernels", "up_2_conv_kernels", "up_3_conv_kernels"):
            side *= 2                                                                            # drawn at the finer resolution, :1832,1836,1842
        if name.endswith("biases"):
            assert not v.any(), name
            continue
        if name.endswith("time_weights"):
            bound = np.sqrt(6.0 / CFG["time_dim"])
        elif name.endswith(".weights"):
            bound = np.sqrt(6.0 / CFG["key_dim"])
        elif name.endswith("Q_proj") or name.endswith("K_proj"):
            bound = np.sqrt(6.0 / (side * side + CFG["key_dim"]))
        else:
            bound = np.sqrt(6.0 / (side * side))                                                 # kernels and V_proj: fan_in = height x width
        assert 0.98 * bound < np.abs(v).max() <= bound * (1 + 1e-6), (name, np.abs(v).max(), bound)


def split_bucket(flat):
    out = {}; at = 0
    for name, shp in tensor_list(CFG):
        n = int(np.prod(shp)); out[name] = flat[at:at + n].reshape(shp); at += n
    assert at == flat.size
    return out


def read_dump(d, images):
    P = split_bucket(np.fromfile(d / "params.f32", np.float32))
    x = np.fromfile(d / "x.f32", np.float32).reshape(images, 3, 32, 32); noise = np.fromfile(d / "noise.f32", np.float32).reshape(images, 3, 32, 32)
    temb = np.fromfile(d / "temb.f32", np.float32).reshape(images, -1); drop = np.fromfile(d / "drop.u8", np.uint8)
    sizes = block_sizes(); starts = np.concatenate([[0], np.cumsum(sizes)])
    per_image = [np.concatenate([drop[images * starts[k] + b * sizes[k]: images * starts[k] + (b + 1) * sizes[k]] for k in range(18)]) for b in range(images)]
    return P, x, noise, temb, per_image, np.fromfile(d / "prediction.f32", np.float32).reshape(images, 3, 32, 32), split_bucket(np.fromfile(d / "grads.f32", np.float32))


@pytest.mark.gpu
def test_train_is_the_references_train(prog, ora, batch_file, tmp_path):
    """`train 1` = the reference's train() (:1874-1934): init_parameters, one example, noise, forward, loss, backward.  The uploaded values are the
    `draws` verb's (pinned to the reference's functions by the CPU test); the prediction and the printed loss against the oracle composition in
    fp64 on those values.  The gradients are NOT compared at this initialisation: with fan_in = height x width the reference's own fp64 backward
    pass reaches 1e72 (group_norm divides by the variance), which no fp32 evaluation holds -- the next test compares them at BLA_UNET_INIT=unit."""
    d = tmp_path / "dump"; d.mkdir(); h = tmp_path / "host"; h.mkdir()
    env = dict(BLA_CIFAR_BATCH=batch_file, BLA_UNET_DUMP=str(d))
    r = run(prog, ["train", "1"], tmp_path, env)
    run(prog, ["draws", "1", str(h)], tmp_path, env)
    for f in ("x.f32", "noise.f32", "drop.u8", "params.f32"):
        assert open(d / f, "rb").read() == open(h / f, "rb").read(), f
    P, x, noise, temb, drops, got, _ = read_dump(d, 1)
    assert not temb.any()
    want, G = ora.unet(CFG, {k: v.astype(np.float64) for k, v in P.items()}, x[0].astype(np.float64), temb[0].astype(np.float64), noise[0].astype(np.float64), drops[0])
    err = np.linalg.norm(got[0] - want) / np.linalg.norm(want)
    loss = float([l for l in r.stdout.splitlines() if l.startswith("Pass 0:")][0].split("Avg loss: ")[1])
    print(f"C U-Net program at the reference's init: prediction error {err:.2e}, loss {loss:.6f}, fp64 gradient norm {np.sqrt(sum(np.linalg.norm(v) ** 2 for v in G.values())):.2e}")
    assert err <= 5e-3                                   # the reference's loops in fp32 sit 4.9e-4 from fp64 here (tools/unet_conditioning.py's method)
    assert abs(loss - np.mean((want - noise[0]) ** 2)) <= 1e-5 * loss + 1e-6


@pytest.mark.gpu
def test_train_pass_of_two_images_against_the_oracle(prog, ora, batch_file, tmp_path):
    """`train 1 2` at BLA_UNET_INIT=unit and time step 500: prediction, printed loss and the gradient bucket (summed over the two images; dropout
    decisions block by block, image by image inside a block) against the oracle in fp64.  Yardstick: the oracle's own fp32 mode -- the reference's
    loops in float -- on the same values; the device must not sit further from fp64 than twice that (+1e-3)."""
    d = tmp_path / "dump"; d.mkdir()
    env = dict(BLA_CIFAR_BATCH=batch_file, BLA_UNET_DUMP=str(d), BLA_UNET_INIT="unit", BLA_UNET_TIMESTEP="500")
    r = run(prog, ["train", "1", "2"], tmp_path, env)
    P, x, noise, temb, drops, got, grads = read_dump(d, 2)
    assert temb.min() >= 0 and temb.max() > 0.9 and np.array_equal(temb[0], temb[1])
    G64 = G32 = None; losses = []
    for b in range(2):
        w64, g64 = ora.unet(CFG, {k: v.astype(np.float64) for k, v in P.items()}, x[b].astype(np.float64), temb[b].astype(np.float64), noise[b].astype(np.float64), drops[b])
        w32, g32 = ora.unet(CFG, P, x[b], temb[b], noise[b], drops[b])
        ref32 = np.linalg.norm(w32 - w64) / np.linalg.norm(w64); err = np.linalg.norm(got[b] - w64) / np.linalg.norm(w64)
        assert err <= 2 * ref32 + 1e-3, f"image {b}: prediction error {err:.3e}, the reference's loops in fp32 {ref32:.3e}"
        losses.append(np.mean((w64 - noise[b]) ** 2))
        G64 = g64 if G64 is None else {k: G64[k] + g64[k] for k in g64}
        G32 = g32 if G32 is None else {k: G32[k] + g32[k].astype(np.float64) for k in g32}
    loss = float([l for l in r.stdout.splitlines() if l.startswith("Pass 0:")][0].split("Avg loss: ")[1])
    assert abs(loss - np.mean(losses)) <= 2e-3 * np.mean(losses) + 1e-6, (loss, losses)
    total = np.sqrt(sum(np.linalg.norm(v) ** 2 for v in G64.values()))
    worst = ("", 0.0, 0.0)
    for name, w in G64.items():
        scale = max(np.linalg.norm(w), 1e-3 * total)
        e = np.linalg.norm(grads[name] - w) / scale; e32 = np.linalg.norm(G32[name] - w) / scale
        worst = max(worst, (name, e, e32), key=lambda t: t[1])
        assert e <= 2 * e32 + 1e-3, f"{name}: gradient error {e:.3e}, the reference's loops in fp32 {e32:.3e}"
    print(f"C U-Net program, two images: loss {loss:.6f} (oracle {np.mean(losses):.6f}), worst gradient tensor {worst[0]} {worst[1]:.2e} (fp32 loops {worst[2]:.2e})")


@pytest.mark.gpu
def test_run_from_the_file_set(prog, batch_file, tmp_path):
    """init -> run: parameters through the reference's CSV file set (as written: five ResNet blocks lose input channels, SURVEY Q-list) and with
    BLA_UNET_FULL_FILES=1 (every channel); both runs draw the same examples, so only the parameters differ.  (BLA_UNET_INIT=unit: at the reference's
    initialisation the prediction is ~1e-7 and the loss is the noise's own mean square whatever the parameters.)"""
    (tmp_path / "data").mkdir()
    out = {}
    for full in ("0", "1"):
        env = dict(BLA_CIFAR_BATCH=batch_file, BLA_UNET_FULL_FILES=full, BLA_UNET_WEIGHTS=str(tmp_path / "data" / f"w{full}"), BLA_UNET_INIT="unit")
        run(prog, ["init"], tmp_path, env)
        r = run(prog, ["run", "3"], tmp_path, env)
        line = r.stdout.strip().splitlines()[-1]
        assert line.startswith("Predicting the noise of 3 examples...done! Avg loss: "), line
        out[full] = float(line.split("Avg loss: ")[1])
        assert np.isfinite(out[full]) and out[full] > 0
    assert out["0"] != out["1"]
    n_as_written = os.path.getsize(tmp_path / "data" / "w0" / "up_1" / "resnet_1" / "conv_1.csv")
    n_full = os.path.getsize(tmp_path / "data" / "w1" / "up_1" / "resnet_1" / "conv_1.csv")
    assert 1.9 < n_full / n_as_written < 2.1
