"""The multi-head U-Net (bla_unet_create_heads) restated in float64, on the host.

oracle.unet composes the network; this file replaces its two attention functions (monkeypatch, the way tests/test_unet_bf16_host.py's restated_unet replaces
the block and convolution functions; nothing under oracle/ is edited) by tests/test_attention_heads_host.py's heads_block: the multi-head block, unrounded (the
float64 multi-head block itself, which that file pins against the composition of single-head blocks) or with the online bf16 entries' roundings.  Everything
else is the oracle's.  Configuration: tests/test_unet_bf16_host.py's CFG (dims [32, 64, 64, 48], key_dim 8) and its parameter scales, batch 2, 2 heads, so the
attention tensors are C x 16 and 16 x C.

  * 16 x 16 images: level-1 S = 64 and mid S = 4 both run the fp32 heads entries under BLA_UNET_ATTENTION_F32; the reference is the unrounded network.
  * 32 x 32 images: level-1 S = 256 runs the online bf16 heads entries in BOTH attention modes, mid S = 16 the fp32 heads entries.  What this file RECORDS per
    tensor is ||rounded - exact|| / ||exact||, `rounded` = heads_block(.., rounded=True) in the blocks with S > 64 and the unrounded block in the mid block;
    tests/test_unet_heads_gpu.py holds the device (fp32 products, so attention is the only rounding) inside twice that.
  * tests/test_unet_bf16_host.py's draw-independence rule at these inputs: time biases perturbed by 3e-7 may move no tensor of the rounded network by more
    than half its recorded value and none beyond 1.3 times it (three draws).  ONE tensor fails it: down_2_self_attention_2.Q_proj moves by 0.55 of its recorded
    value at draw 0 (its exact gradient is small: the recorded value is 5.7e-2 where its neighbours have 3e-3); every other tensor moves by less than half.
    DRAW_DEPENDENT names it, and the device test bounds it by 0.25 normwise (DESIGN 3.29's model bound) instead of twice the recorded value.
  * The program: `cifar_unet_gpu init` with BLA_UNET_HEADS=2 writes attention files twice as wide; a bad value stops every sub-command with a message."""
import functools
import os
import subprocess

import numpy as np
import pytest

import test_unet_bf16_host as bf
from test_attention_heads_host import heads_block

F64 = np.float64
CFG, B, HEADS = bf.CFG, 2, 2
LONG = 64                      # bla_attention_f32_heads_applies' limit on S: longer blocks are bf16-online in both modes
DRAW_DEPENDENT = {"down_2_self_attention_2.Q_proj"}         # tensors of the 32 x 32 network that fail the draw-independence rule (bounded by 0.25 normwise on the device instead)
EX = bf.EX


def cfg_at(side):
    return dict(CFG, image_h=side, image_w=side)


def wide(cfg, heads=HEADS):
    """the configuration whose key_dim is the attention tensors' width (for tensor_list / make_params)"""
    return dict(cfg, key_dim=cfg["key_dim"] * heads)


def make_params(cfg, heads=HEADS):
    return bf.make_params(wide(cfg, heads))


def make_inputs(cfg):
    return bf.make_inputs(cfg, B)


def heads_unet(ora, monkeypatch, cfg, P, x, temb, noise, drop, rounded_above=None, heads=HEADS):
    """oracle.unet, one image, its attention the multi-head block; rounded_above: blocks with S above it take the online bf16 entries' roundings (None: none)"""
    d = cfg["key_dim"]

    def inputs(xin, wq, wk, wv, w, bias, del_y=None):
        c = xin.shape[0]
        x2 = np.asarray(xin, F64).reshape(1, c, -1)
        return dict(x=x2, wq=wq, wk=wk, wv=wv, w=w, bias=bias, del_y=np.zeros_like(x2) if del_y is None else np.asarray(del_y, F64).reshape(1, c, -1))

    def rounded(I):
        return rounded_above is not None and I["x"].shape[2] > rounded_above

    def attention_forward(xin, wq, wk, wv, w, bias):
        I = inputs(xin, wq, wk, wv, w, bias)
        return dict(I=I, out=heads_block(I, heads, d, rounded(I), backward=False)["out"][0].reshape(xin.shape))

    def attention_backward(del_y, xin, wq, wk, wv, w, f):
        I = dict(f["I"], del_y=np.asarray(del_y, F64).reshape(f["I"]["x"].shape))
        o = heads_block(I, heads, d, rounded(I))
        return dict(del_wq=o["del_wq"], del_wk=o["del_wk"], del_wv=o["del_wv"], del_w=o["del_w"], del_x=o["del_x"][0].reshape(xin.shape))
    monkeypatch.setattr(ora, "attention_forward", attention_forward)
    monkeypatch.setattr(ora, "attention_backward", attention_backward)
    try:
        return ora.unet(cfg, P, x, temb, noise, drop)
    finally:
        monkeypatch.undo()


def batch_pass(ora, monkeypatch, cfg, rounded_above=None, params=None, heads=HEADS):
    """(predictions [B], gradients summed over the images) of the restated network"""
    P = {n: np.asarray(v, F64) for n, v in (params or make_params(cfg, heads)).items()}
    x, temb, noise, drop = make_inputs(cfg)
    outs, G = [], None
    for b in range(B):
        out, g = heads_unet(ora, monkeypatch, cfg, P, x[b].astype(F64), temb[b].astype(F64), noise[b].astype(F64), drop[b], rounded_above, heads)
        outs.append(out)
        G = g if G is None else {n: G[n] + g[n] for n in G}
    return np.stack(outs), G


def differences(exact, other):
    """name -> ||other - exact|| / ||exact||: 'prediction[b]' and every gradient tensor with a non-zero exact gradient"""
    d = {f"prediction[{b}]": bf.normwise(other[0][b], exact[0][b]) for b in range(B)}
    for n, w in exact[1].items():
        if np.linalg.norm(w) > 0:
            d[n] = bf.normwise(other[1][n], w)
    return d


def _oracle():
    import oracle as ora
    ora.build()
    return ora, pytest.MonkeyPatch()


@functools.lru_cache(maxsize=None)
def exact16():
    """the unrounded 16 x 16 network -- once per process; tests/test_unet_heads_gpu.py reads it here"""
    return batch_pass(*_oracle(), cfg_at(16))


@functools.lru_cache(maxsize=None)
def recorded32():
    """(exact pass, rounded pass, recorded differences) of the 32 x 32 network -- once per process; tests/test_unet_heads_gpu.py reads it here"""
    ora, mp = _oracle()
    exact, rounded = batch_pass(ora, mp, cfg_at(32)), batch_pass(ora, mp, cfg_at(32), LONG)
    return exact, rounded, differences(exact, rounded)


def test_the_tensor_list_has_the_attention_tensors_at_width_D():
    shapes = dict(bf.tensor_list(wide(CFG)))
    D = HEADS * CFG["key_dim"]
    assert shapes["mid_self_attention.Q_proj"] == (48, D) and shapes["down_2_self_attention_1.V_proj"] == (64, D) and shapes["up_3_self_attention_2.weights"] == (D, 64)
    assert set(exact16()[1]) == set(shapes)


def test_one_head_restatement_is_the_oracle(ora, monkeypatch):
    """heads_block with one head, unrounded, in place of the oracle's attention: the same network to 1e-7 normwise, not 1e-10 -- the block's
    inv is the DEVICE's (float)(1 / sqrt(d)), the oracle's a double: 3e-8 apart at d = 8, which is what the Q and K projections' gradients differ by"""
    cfg = cfg_at(16)
    P = {n: np.asarray(v, F64) for n, v in make_params(cfg, 1).items()}
    x, temb, noise, drop = make_inputs(cfg)
    a = F64
    want_out, want = ora.unet(cfg, P, x[0].astype(a), temb[0].astype(a), noise[0].astype(a), drop[0])
    out, G = heads_unet(ora, monkeypatch, cfg, P, x[0].astype(a), temb[0].astype(a), noise[0].astype(a), drop[0], heads=1)
    assert bf.normwise(out, want_out) <= 1e-7
    diff = {n: bf.normwise(G[n], w) for n, w in want.items() if np.linalg.norm(w) > 0}
    assert max(diff.values()) <= 1e-7 and len(diff) == len(want) - 5, max(diff.items(), key=lambda t: t[1])


def test_rounding_differences_are_recorded():
    exact, _, diff = recorded32()
    for n, v in diff.items():
        print(f"{n:44s} rounded vs exact {v:.3e}")
    assert len(diff) == B + sum(1 for n, _ in bf.tensor_list(wide(CFG)) if not (n.endswith(".biases") and "attention" in n))
    assert all(0 < v < 0.1 for v in diff.values()), {n: v for n, v in diff.items() if not 0 < v < 0.1}
    assert np.abs(exact[0]).max() > 1e-3


@pytest.mark.parametrize("draw", [0, 1, 2])
def test_recorded_values_do_not_depend_on_the_draw(ora, monkeypatch, draw):
    """tests/test_unet_bf16_host.py's rule (its test of the same name) at these inputs"""
    exact, rounded, diff = recorded32()
    rng = np.random.default_rng(draw)
    cfg = cfg_at(32)
    P = {n: v.astype(F64) * (1 + 3e-7 * rng.choice([-1.0, 1.0], v.shape)) if n.endswith("time_biases") else v for n, v in make_params(cfg).items()}
    other = batch_pass(ora, monkeypatch, cfg, LONG, params=P)
    moved = differences(exact, other)
    mutual = {n: bf.normwise(other[1][n], rounded[1][n]) / diff[n] for n in diff if n in other[1]}
    print(f"draw {draw}: largest move {max(mutual.values()):.2f} of the recorded value ({max(mutual, key=mutual.get)}), largest ratio to it {max(moved[n] / diff[n] for n in diff):.2f}")
    failing = {n for n in diff if mutual.get(n, 0) > 0.5 or moved[n] > 1.3 * diff[n]}
    assert failing <= DRAW_DEPENDENT and max(moved[n] for n in DRAW_DEPENDENT) <= 0.25, {n: (mutual.get(n), moved[n] / diff[n]) for n in failing - DRAW_DEPENDENT}


# ---- the C program: BLA_UNET_HEADS needs no device for `init` and for its refusals -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prog(pkg):
    pkg.build_native()
    subprocess.check_call(["make", "-s", "-C", EX, "cifar_unet_gpu"])
    return os.path.join(EX, "cifar_unet_gpu")


def run(prog, args, cwd, **env):
    return subprocess.run([prog] + args, cwd=str(cwd), env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)


def test_program_init_writes_the_attention_files_at_width_D(prog, tmp_path):
    """the reference's constants (C = 256 in every attention block, key_dim 16), 2 heads: query / key / value [256][32], weight [32][256], bias [256]"""
    r = run(prog, ["init"], tmp_path, BLA_UNET_HEADS="2", BLA_UNET_WEIGHTS="w", BLA_UNET_FULL_FILES="1")
    assert r.returncode == 0, r.stdout + r.stderr
    seen = 0
    for dirpath, _, files in os.walk(os.path.join(str(tmp_path), "w")):
        if "self_attention" not in dirpath:
            continue
        assert sorted(files) == ["bias.csv", "key.csv", "query.csv", "value.csv", "weight.csv"], (dirpath, files)
        for leaf in files:
            with open(os.path.join(dirpath, leaf)) as f:
                rows = [[tok for tok in line.split(",") if tok.strip()] for line in f if line.strip()]
            want = dict(bias=(1, 256), weight=(32, 256)).get(leaf[:-4], (256, 32))
            assert (len(rows), {len(row) for row in rows}) == (want[0], {want[1]}), (dirpath, leaf, len(rows))
            seen += 1
    assert seen == 5 * 5


@pytest.mark.parametrize("value", ["0", "-2", "two", "2x", "1.5", "17", "4096"])
@pytest.mark.parametrize("args", [["run"], ["train", "1"], ["init"], ["fit", "1"], ["eval"], ["sample"]], ids=lambda a: a[0])
def test_program_refuses_a_bad_heads_value(prog, tmp_path, args, value):
    r = run(prog, args, tmp_path, BLA_UNET_HEADS=value)
    assert r.returncode != 0 and "BLA_UNET_HEADS" in r.stdout + r.stderr, (r.returncode, r.stdout, r.stderr)
    assert not os.listdir(tmp_path)      # (init wrote nothing)


def test_program_refuses_heads_on_the_materialising_bf16_attention(prog, tmp_path):
    r = run(prog, ["init"], tmp_path, BLA_UNET_HEADS="2", BLA_UNET_ATTENTION="bf16")
    assert r.returncode != 0 and "BLA_UNET_HEADS" in r.stderr and not os.listdir(tmp_path)
