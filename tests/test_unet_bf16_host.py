"""The mixed-precision U-Net (bla_unet_create_mixed, BLA_UNET_PRODUCTS_BF16) restated in float64, on the host.

oracle.unet composes the network from four functions of the oracle module: resnet_forward, resnet_backward, conv_intended and conv_backward_any_stride.
This file replaces those four (monkeypatch; nothing under oracle/ is edited) and leaves the wiring, attention, the norms of the output head, resizing,
concatenation and the skip additions the oracle's:
  * the two block functions become single-image adapters over block_reference of tests/test_norm_bf16_host.py -- the composition of
    bla_resnet_{forward,backward}_batched_bf16 in float64, with bla_f32_to_bf16's rounding wherever that composition rounds, or with none anywhere;
  * the two convolution functions round exactly where the _as_bf16 compositions round: forward the operands x and kern, the weight gradient del_y and x,
    the data gradient del_y and kern.
The unrounded variant must BE the oracle (1e-10 normwise).  ||rounded - exact|| / ||exact|| of the prediction (per image), of every gradient tensor (summed
over the three images) and of the time-embedding gradient is what the mixed-precision arithmetic costs on these inputs: tests/test_unet_bf16_gpu.py holds
the device inside twice that (DESIGN 3.25's practice: the device shares the roundings, fp32 accumulation does not show beside a unit roundoff of 2^-9).
Three wrong-but-finite networks show that twice the recorded value still catches a wiring error.  Configuration: tests/test_unet_model.py's."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import test_norm_bf16_host as tnb
from conftest import ROOT
from inputs import uniform

CFG = dict(image_h=16, image_w=16, in_channels=3, dims=[32, 64, 64, 48], time_dim=24, kernel=3, group_size=32, key_dim=8)
B = 3
BLOCK_NAMES = ["down_1_resnet_1", "down_1_resnet_2", "down_2_resnet_1", "down_2_resnet_2", "down_3_resnet_1", "down_3_resnet_2", "down_4_resnet_1", "down_4_resnet_2",
               "mid_resnet_1", "mid_resnet_2", "up_1_resnet_1", "up_1_resnet_2", "up_2_resnet_1", "up_2_resnet_2", "up_3_resnet_1", "up_3_resnet_2", "up_4_resnet_1",
               "up_4_resnet_2"]      # forward order = the order of the dropout decisions
EX = os.path.join(ROOT, "examples")


def tensor_list(cfg=CFG):
    """(name, shape) in bucket order: the order forward() first uses them (csrc/bla_unet_model.hip)"""
    D, k, t, d, c0 = cfg["dims"], cfg["kernel"], cfg["time_dim"], cfg["key_dim"], cfg["in_channels"]
    out = []

    def res(name, cin, cout):
        out.extend([(name + ".conv_1_kernels", (cout, cin, k, k)), (name + ".conv_2_kernels", (cout, cout, k, k)), (name + ".time_weights", (t, cout)),
                    (name + ".time_biases", (cout,))])
        if cin != cout:
            out.append((name + ".residual_conv_kernels", (cout, cin, 1, 1)))

    def att(name, c):
        out.extend([(name + ".Q_proj", (c, d)), (name + ".K_proj", (c, d)), (name + ".V_proj", (c, d)), (name + ".weights", (d, c)), (name + ".biases", (c,))])
    res("down_1_resnet_1", c0, D[0]); res("down_1_resnet_2", D[0], D[0]); out.append(("down_1_conv_kernels", (D[1], D[0], k, k)))
    res("down_2_resnet_1", D[1], D[1]); att("down_2_self_attention_1", D[1]); res("down_2_resnet_2", D[1], D[1]); att("down_2_self_attention_2", D[1])
    out.append(("down_2_conv_kernels", (D[2], D[1], k, k)))
    res("down_3_resnet_1", D[2], D[2]); res("down_3_resnet_2", D[2], D[2]); out.append(("down_3_conv_kernels", (D[3], D[2], k, k)))
    res("down_4_resnet_1", D[3], D[3]); res("down_4_resnet_2", D[3], D[3])
    res("mid_resnet_1", D[3], D[3]); att("mid_self_attention", D[3]); res("mid_resnet_2", D[3], D[3])
    res("up_1_resnet_1", 2 * D[3], D[3]); res("up_1_resnet_2", D[3], D[3])
    if D[3] != D[2]:
        out.append(("up_1_conv_kernels", (D[2], D[3], k, k)))
    res("up_2_resnet_1", 2 * D[2], D[2]); res("up_2_resnet_2", D[2], D[2])
    if D[2] != D[1]:
        out.append(("up_2_conv_kernels", (D[1], D[2], k, k)))
    res("up_3_resnet_1", 2 * D[1], D[1]); att("up_3_self_attention_1", D[1]); res("up_3_resnet_2", D[1], D[1]); att("up_3_self_attention_2", D[1])
    if D[1] != D[0]:
        out.append(("up_3_conv_kernels", (D[0], D[1], k, k)))
    res("up_4_resnet_1", 2 * D[0], D[0]); res("up_4_resnet_2", D[0], D[0])
    out.append(("output_conv_kernels", (c0, D[0], k, k)))
    return out


def make_params(cfg=CFG):
    """tests/test_unet_model.py's parameter draws (seed 7000 + bucket index, fp32) at other scales, chosen on the host in float64 alone (nothing of the
    device enters the choice) by three requirements on the restatement below.  With s = that test's sqrt(3 / fan_in): kernels 0.8 s, time weights 8 s,
    biases in [-2, 2], Q / K projections 0.2 s, V projections and attention output weights 0.1 s.
    (1) The rounding difference must be small against a wiring error.  Group norm divides by the variance (lib/norm.c), so this network
        amplifies roundoff and scales gradients by 1 / variance at every norm: at that test's scales bf16's 2^-9 becomes 0.8 (median) to 1.6 normwise in
        the gradient tensors of one image -- twice that holds for any finite gradient.
    (2) A lost skip gradient must show.  With smaller kernels alone (0.6 s) the roundoff is 6e-2 at most, but the gradient along the main path is 1e27
        times the one a skip connection carries.  A larger time embedding puts per-channel offsets in front of every block's second norm, which keeps
        the group variances away from zero.
    (3) The recorded value must be a property of the arithmetic, not of one draw of the roundings.  A bf16 rounding is a step function: a value that an
        fp32-level difference moves across a rounding boundary changes by a whole bf16 ulp, and everything behind it rounds differently.  On the 2 x 2
        level an image is 192 numbers, so one such element weighs much.  With time weights 4 s, biases in [-1, 1] and all attention matrices at 0.8 s,
        perturbing the time biases by 3e-7 moved the rounded restatement by up to 1.55 times the recorded value of a tensor (0 where no element
        crossed), and a device run on those inputs lay at 2.1 .. 3.1 times the recorded value in four tensors of the 2 x 2 level while reproducing the
        rounded block alone to 1e-7: no fp32 implementation can be held to twice one draw there.  At the scales above the same perturbations (six draws,
        with every product and norm stored in fp32 as well) move no tensor by more than 0.28 of its recorded value and none beyond 1.05 times it;
        test_recorded_values_do_not_depend_on_the_draw keeps that true.
    At these scales: 4e-3 in the prediction, 1.5e-3 .. 2.1e-2 in the gradients of three images, a lost skip gradient at 287 times a recorded value.
    Scanned: kernel gains 0.4 .. 3, time gains 0.3 .. 16, biases 0.05 .. 4, attention gains 0.05 .. 0.8."""
    P = {}
    for i, (name, shp) in enumerate(tensor_list(cfg)):
        s = float(np.sqrt(3.0 / (int(np.prod(shp[1:])) if len(shp) > 1 else shp[0])))
        if name.endswith("biases"):
            scale = 2.0
        elif name.endswith(".time_weights"):
            scale = 8.0 * s
        elif name.endswith("Q_proj") or name.endswith("K_proj"):
            scale = 0.2 * s
        elif name.endswith("V_proj") or name.endswith(".weights"):
            scale = 0.1 * s
        else:
            scale = 0.8 * s
        P[name] = uniform(7000 + i, shp, -scale, scale, np.float32)
    return P


def dropout_block_sizes(cfg=CFG):
    D = cfg["dims"]; H = [cfg["image_h"]]; W = [cfg["image_w"]]
    for _ in range(3):
        H.append((H[-1] + 1) // 2); W.append((W[-1] + 1) // 2)
    return [D[l] * H[l] * W[l] for l in [0, 0, 1, 1, 2, 2, 3, 3, 3, 3, 3, 3, 2, 2, 1, 1, 0, 0]]


def make_inputs(cfg=CFG, batch=B):
    """x, temb, noise [batch][..] fp32 and the 10 % dropout draw per image (block after block: what the oracle takes)"""
    x = uniform(7911, (batch, cfg["in_channels"], cfg["image_h"], cfg["image_w"]), -1, 1, np.float32)
    temb = uniform(7912, (batch, cfg["time_dim"]), -1, 1, np.float32)
    noise = uniform(7913, x.shape, -1, 1, np.float32)
    drop = (uniform(7914, (batch, sum(dropout_block_sizes(cfg))), 0, 1, np.float32) < 0.1).astype(np.uint8)
    return x, temb, noise, drop


def device_drop_layout(drop, cfg=CFG):
    """per image, block after block -> the device's layout: block after block, inside a block image by image"""
    parts, o = [], 0
    for sz in dropout_block_sizes(cfg):
        parts.append(drop[:, o:o + sz].ravel()); o += sz
    return np.concatenate(parts)


def rnd(a):
    """bla_f32_to_bf16's rounding of the fp32 value, back in float64"""
    return tnb.widen(tnb.rne(np.asarray(a, np.float64).astype(np.float32))).astype(np.float64)


def run_block(I, gs, rounded, **mutation):
    """block_reference on the inputs I (it draws its own through block_inputs: hand it ours)"""
    _, cin, h, w = I["x"].shape
    keep = tnb.block_inputs
    tnb.block_inputs = lambda block: I
    try:
        return tnb.block_reference((1, cin, I["conv1"].shape[0], h, w, gs), rounded, **mutation)
    finally:
        tnb.block_inputs = keep


def restated_unet(ora, monkeypatch, rounded, P, x, temb, noise, drop, ungated_block=None, dropped_skip=None, unflipped_conv=False):
    """oracle.unet with the four functions replaced (module docstring); one image.  The mutations:
    ungated_block: forward index of a block whose conv2 data gradient is not gated by p2;
    dropped_skip: forward index of the block (16: up_4_resnet_1) whose input gradient loses its skip half (what `+ gs1` adds in front of down_1_resnet_2 is lost);
    unflipped_conv: a stride-2 convolution's data gradient multiplies with the kernels as they are, not flipped (a data-gradient matrix prepared as a forward one)."""
    r = rnd if rounded else (lambda a: np.asarray(a, np.float64))
    conv_fwd, conv_bwd = ora.conv_intended, ora.conv_backward_any_stride
    calls = [0]

    def resnet_forward(xin, te, k1, k2, tw, tb, kres, dr, group_size):
        cout = k1.shape[0]
        I = dict(x=np.asarray(xin, np.float64)[None], temb=np.asarray(te, np.float64)[None], conv1=k1, conv2=k2, time_w=tw, time_b=tb,
                 drop=np.asarray(dr).reshape(1, cout, xin.shape[1], xin.shape[2]) != 0, del_out=np.zeros((1, cout, xin.shape[1], xin.shape[2])))
        if kres is not None:
            I["res"] = kres
        f = dict(I=I, index=calls[0], result=run_block(I, group_size, rounded)["result"][0])
        calls[0] += 1
        return f

    def resnet_backward(del_out, xin, te, k1, k2, kres, f, group_size):
        I = dict(f["I"], del_out=np.asarray(del_out, np.float64)[None])
        o = run_block(I, group_size, rounded, gate2=f["index"] != ungated_block)
        dx = o["del_x"][0]
        if f["index"] == dropped_skip:
            dx = dx.copy(); dx[dx.shape[0] // 2:] = 0
        return dict(dk1=o["conv1"], dk2=o["conv2"], dtw=o["time_w"], dtb=o["time_b"], dkres=o.get("res"), del_x=dx)

    def conv_intended(xin, kern, s):
        return conv_fwd(r(xin), r(kern), s)

    def conv_backward_any_stride(del_y, xin, kern, s):
        dy = r(del_y)
        dk, _ = conv_bwd(dy, r(xin), kern, s)
        kd = r(kern)
        _, dx = conv_bwd(dy, xin, kd[:, :, ::-1, ::-1] if unflipped_conv and s == 2 and kern.shape[0] == CFG["dims"][3] else kd, s)
        return dk, dx
    for name, fn in (("resnet_forward", resnet_forward), ("resnet_backward", resnet_backward), ("conv_intended", conv_intended),
                     ("conv_backward_any_stride", conv_backward_any_stride)):
        monkeypatch.setattr(ora, name, fn)
    try:
        return ora.unet(CFG, P, x, temb, noise, drop)
    finally:
        monkeypatch.undo()


def embedding_grad(P, G):
    """dL/dtemb of one image = sum over the 18 blocks of W_k . g_tb_k (a single image's time-bias gradient is its channel sums)"""
    return sum(P[n + ".time_weights"] @ G[n + ".time_biases"] for n in BLOCK_NAMES)


def normwise(a, b):
    return float(np.linalg.norm((np.asarray(a, np.float64) - b).ravel()) / np.linalg.norm(np.asarray(b).ravel()))


def batch_pass(ora, monkeypatch, rounded, params=None, **mutation):
    """(predictions [B], gradients summed over the images, embedding gradient [B][T]) of the restated network"""
    P = {n: np.asarray(v, np.float64) for n, v in (params or make_params()).items()}
    x, temb, noise, drop = make_inputs()
    outs, G, emb = [], None, []
    for b in range(B):
        out, g = restated_unet(ora, monkeypatch, rounded, P, x[b].astype(np.float64), temb[b].astype(np.float64), noise[b].astype(np.float64), drop[b], **mutation)
        outs.append(out); emb.append(embedding_grad(P, g))
        G = g if G is None else {n: G[n] + g[n] for n in G}
    return np.stack(outs), G, np.stack(emb)


def differences(exact, other):
    """name -> ||other - exact|| / ||exact||: 'prediction[b]', every gradient tensor with a non-zero exact gradient, 'embedding_grad'"""
    d = {f"prediction[{b}]": normwise(other[0][b], exact[0][b]) for b in range(B)}
    for n, w in exact[1].items():
        if np.linalg.norm(w) > 0:
            d[n] = normwise(other[1][n], w)
    d["embedding_grad"] = normwise(other[2], exact[2])
    return d


@functools.lru_cache(maxsize=None)
def _recorded():
    import oracle as ora
    ora.build()
    mp = pytest.MonkeyPatch()
    exact, rounded = batch_pass(ora, mp, False), batch_pass(ora, mp, True)
    return exact, rounded, differences(exact, rounded)


def recorded():
    """(exact pass, rounded pass, recorded differences) -- computed once per process; tests/test_unet_bf16_gpu.py reads it here"""
    return _recorded()


def test_unrounded_restatement_is_the_oracle(ora):
    exact = recorded()[0]
    P = {n: v.astype(np.float64) for n, v in make_params().items()}
    x, temb, noise, drop = make_inputs()
    G = None
    for b in range(B):
        out, g = ora.unet(CFG, P, x[b].astype(np.float64), temb[b].astype(np.float64), noise[b].astype(np.float64), drop[b])
        assert normwise(exact[0][b], out) <= 1e-10, (b, normwise(exact[0][b], out))
        G = g if G is None else {n: G[n] + g[n] for n in G}
    assert set(G) == set(exact[1]) == {n for n, _ in tensor_list()}
    for n, w in G.items():
        if np.linalg.norm(w) == 0:
            assert n.endswith(".biases") and "attention" in n, n
            assert not exact[1][n].any(), n
        else:
            assert normwise(exact[1][n], w) <= 1e-10, (n, normwise(exact[1][n], w))


def test_rounding_differences_are_recorded():
    _, _, diff = recorded()
    for n, v in diff.items():
        print(f"{n:44s} rounded vs exact {v:.3e}")
    assert len(diff) == B + 1 + sum(1 for n, _ in tensor_list() if not (n.endswith(".biases") and "attention" in n))
    assert all(v > 0 for v in diff.values()), {n: v for n, v in diff.items() if not v > 0}
    assert make_inputs()[3].mean() > 0.08


@pytest.mark.parametrize("draw", [0, 1, 2])
def test_recorded_values_do_not_depend_on_the_draw(ora, monkeypatch, draw):
    """make_params' requirement (3): time biases perturbed by 3e-7 (what separates one fp32 evaluation order from another) may move elements across
    bf16 rounding boundaries, but no tensor of the rounded restatement by more than half its recorded value, and none beyond 1.3 times it -- the device
    test's factor of 2 then has room for a device that rounds a few elements the other way."""
    exact, rounded, diff = recorded()
    rng = np.random.default_rng(draw)
    P = {n: v.astype(np.float64) * (1 + 3e-7 * rng.choice([-1.0, 1.0], v.shape)) if n.endswith("time_biases") else v for n, v in make_params().items()}
    other = batch_pass(ora, monkeypatch, True, params=P)
    moved = differences(exact, other)
    mutual = {n: normwise(other[1][n], rounded[1][n]) / diff[n] for n in diff if n in other[1]}
    print(f"draw {draw}: largest move {max(mutual.values()):.2f} of the recorded value ({max(mutual, key=mutual.get)}), largest ratio to it {max(moved[n] / diff[n] for n in diff):.2f}")
    assert max(mutual.values()) <= 0.5 and all(moved[n] <= 1.3 * diff[n] for n in diff)


@pytest.mark.parametrize("mutation", [dict(ungated_block=8), dict(dropped_skip=16), dict(unflipped_conv=True)], ids=["ungated_data_gradient", "dropped_skip", "unflipped_stride2"])
def test_twice_the_recorded_value_catches_a_wiring_error(ora, monkeypatch, mutation):
    """Each wrong-but-finite network moves at least one tensor beyond twice its recorded value (the bound of the device test)."""
    exact, _, diff = recorded()
    moved = differences(exact, batch_pass(ora, monkeypatch, True, **mutation))
    assert all(np.isfinite(v) for v in moved.values())
    beyond = {n: (moved[n], diff[n]) for n in diff if moved[n] > 2 * diff[n]}
    print(mutation, "beyond twice the recorded value:", len(beyond), "tensors; worst", max(beyond.items(), key=lambda t: t[1][0] / t[1][1], default=None))
    assert beyond, moved


# ---- the C program and the create entry: refusals that need no device ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prog(pkg):
    pkg.build_native()
    subprocess.check_call(["make", "-s", "-C", EX, "cifar_unet_gpu"])
    return os.path.join(EX, "cifar_unet_gpu")


@pytest.mark.parametrize("args", [["run"], ["train", "1"], ["init"], ["draws", "1", "out"], ["fit", "1"], ["eval"], ["sample"]], ids=lambda a: a[0])
def test_program_refuses_an_unknown_products_value(prog, tmp_path, args):
    r = subprocess.run([prog] + args, cwd=str(tmp_path), env=dict(os.environ, BLA_UNET_PRODUCTS="bogus"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode != 0 and "BLA_UNET_PRODUCTS" in r.stdout + r.stderr, (r.returncode, r.stdout, r.stderr)
    assert not os.listdir(tmp_path)      # (init wrote nothing)


def test_create_mixed_refuses_an_unknown_products_value(pkg):
    class Cfg(C.Structure):
        _fields_ = [("image_h", C.c_int), ("image_w", C.c_int), ("in_channels", C.c_int), ("dims", C.c_int * 4), ("time_dim", C.c_int), ("kernel", C.c_int),
                    ("group_size", C.c_int), ("key_dim", C.c_int)]
    c = Cfg(16, 16, 3, (C.c_int * 4)(32, 64, 64, 48), 24, 3, 32, 8)
    h = C.c_void_p(0x1234)
    for products in (7, -1, 2):
        assert pkg.lib().bla_unet_create_mixed(C.byref(h), C.byref(c), 3, products) == 1      # BLA_ERR_INVALID
        assert h.value == 0x1234 and b"products" in pkg.lib().bla_last_error()
    assert pkg.UNET_PRODUCTS_F32 == 0 and pkg.UNET_PRODUCTS_BF16 == 1
