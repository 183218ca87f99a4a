"""Every step path of the device-resident MNIST-NN trainer (csrc/bla_mnist.hip) against a float64 restatement of one step, at layer sizes and
batches that leave the reference architecture: odd everything (scalar-load kernels, operands off 16-byte boundaries inside the bucket, pair
members launched alone), 16 < n3 <= 32 (fused softmax tail on the 32x32 tile), n3 > 32 (separate softmax / gradient pass), n0 > 1280 (first
forward product on a tiled kernel with the whole epilogue), B > 1280 (weight gradients on tiled kernels, bias sums as deferred row-sum passes),
and the fallbacks of fused_step / graph_step where the update cannot be folded into the products.

Reference: step64() below, plain numpy float64.  test_restatement_matches_the_oracle (no GPU) holds it against oracle.mnist_step, which
tests/test_oracle_golden.py pins bit for bit to the reference's own code.

Tolerances are the ones tests/test_mnist_gpu.py applies, at these shapes:
    activations, dZ, gradients   |got - ref| <= 1e-5 * (|ref| + mean|ref|)   elementwise
    new parameters               |got - ref| <= 1e-5 * |ref| + 1e-7          elementwise
    fused update vs train_step   ||p - q|| <= 1e-6 ||q|| + 1e-9 and ||(p - p0) - (q - p0)|| <= 1e-5 ||q - p0|| + 1e-9   (test_graph_replay_matches_eager)
    trajectories                 ||got - ref|| <= 1e-5 ||ref|| + 1e-7        (test_ten_steps_track_the_oracle)
A ReLU gate whose pre-activation lies within rounding of zero may open on one side only; instead of tolerating that, the inputs are chosen so
that the float64 Z1 and Z2 keep every element farther than 4e-5 * (|z| + mean|z|) from zero -- four times the bound the device's Z then has to
meet -- and that is asserted on the reference before any device work.  The Z check runs first: once it holds, the device's gates are the
reference's.  Each step test prints its worst error / bound ratio."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

from inputs import uniform, randint

RTOL = 1e-5
F32, F64 = np.float32, np.float64
LR = float(F32(-0.02))
INVALID, UNDEFINED = 1, 5
ACTS = ["z1", "a1", "z2", "a2", "z3", "a3", "dz3", "dz2", "dz1"]
GN = ["dw1", "db1", "dw2", "db2", "dw3", "db3"]
PN = ["w1", "b1", "w2", "b2", "w3", "b3"]

# name: (n0, n1, n2, n3), batch, base seed (parameter tensor i from seed + i, pixels seed + 10, labels seed + 11)
CASES = {
    "A": ((50, 37, 21, 7), 13, 9000),         # everything odd: scalar loads, W2 / W3 off 16-byte boundaries, pairs unshared, fused update on that path
    "B": ((50, 12, 9, 5), 13, 9000),          # as A with every width <= B: the as-written column sum is defined
    "C": ((100, 64, 48, 24), 96, 9000),       # 16 < n3 <= 32: fused softmax tail on the 32x32 tile
    "D": ((120, 80, 64, 40), 64, 9000),       # n3 > 32: separate softmax / gradient pass, no fused update, no device-side metrics
    "E": ((1296, 64, 32, 10), 64, 9000),      # n0 > 1280: layer 1 forward on a tiled kernel (bias, ReLU, pre_act, alpha = 1/255), no fused update
    "F": ((64, 32, 16, 10), 1296, 9100),      # B > 1280: dW on tiled kernels with deferred row sums, no fused update
}
FUSED_UPDATE = {"A": True, "B": True, "C": True, "D": False, "E": False, "F": False}   # can_fuse_update with true row sums
TRAJECTORY_SEEDS = {"A": (9200, 9201, 9202), "F": (9301, 9318, 9332)}                 # pixels from s, labels from s + 50, one pair per step; searched on the CPU for clear gates


def make_params(sizes, seed):
    """W_l uniform in +-sqrt(3 / fan_in) (W1 twice that: its input is pixels / 255), b_l in +-0.1; float32."""
    out = []
    for l in range(3):
        lim = float(np.sqrt(3.0 / sizes[l])) * (2 if l == 0 else 1)
        out.append(uniform(seed + 2 * l, (sizes[l + 1], sizes[l]), -lim, lim, F32))
        out.append(uniform(seed + 2 * l + 1, (sizes[l + 1], 1), -0.1, 0.1, F32))
    return out


def make_batch(sizes, B, s_pix, s_lab):
    x_raw = randint(s_pix, (sizes[0], B), 256).astype(F32)
    lab = randint(s_lab, (B,), sizes[3])
    y = np.zeros((sizes[3], B), F32); y[lab, np.arange(B)] = 1
    return x_raw, y


def step64(params, x_raw, y, lr=LR, col_sum=None):
    """One step in float64.  col_sum: the bias-gradient reduction (default: true row sums).  Returns (acts dict, grads list, new params)."""
    w1, b1, w2, b2, w3, b3 = (np.asarray(p, F64) for p in params)
    n0 = w1.shape[1]
    x = np.asarray(x_raw, F64) * F64(F32(1) / F32(255))
    z1 = w1 @ x + b1; a1 = np.maximum(z1, 0)
    z2 = w2 @ a1 + b2; a2 = np.maximum(z2, 0)
    z3 = w3 @ a2 + b3
    e = np.exp(z3 - z3.max(0, keepdims=True)); a3 = e / e.sum(0, keepdims=True)
    dz3 = (a3 - np.asarray(y, F64)) / n0
    dz2 = (w3.T @ dz3) * (z2 > 0)
    dz1 = (w2.T @ dz2) * (z1 > 0)
    cs = col_sum or (lambda m: m.sum(1, keepdims=True))
    grads = [dz1 @ x.T, cs(dz1), dz2 @ a1.T, cs(dz2), dz3 @ a2.T, cs(dz3)]
    new = [np.asarray(p, F64) + F64(F32(lr)) * g for p, g in zip(params, grads)]
    return dict(zip(ACTS, [z1, a1, z2, a2, z3, a3, dz3, dz2, dz1])), grads, new


def gates_clear(acts):
    """Every element of the float64 Z1, Z2 farther from zero than four times the bound the device's Z has to meet."""
    return all((np.abs(acts[n]) > 4 * RTOL * (np.abs(acts[n]) + np.abs(acts[n]).mean())).all() for n in ("z1", "z2"))


@functools.lru_cache(maxsize=None)
def case_data(name):
    """Inputs and the float64 step (true row sums) of one case, computed once and shared read-only."""
    sizes, B, seed = CASES[name]
    params = make_params(sizes, seed)
    x_raw, y = make_batch(sizes, B, seed + 10, seed + 11)
    acts, grads, new = step64(params, x_raw, y)
    for v in [*params, x_raw, y, *acts.values(), *grads, *new]:
        v.setflags(write=False)
    return {"sizes": sizes, "B": B, "params": params, "x_raw": x_raw, "y": y, "acts": acts, "grads": grads, "new": new}


# ---- no GPU: the restatement against the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_restatement_matches_the_oracle(ora, name):
    """step64 against oracle.mnist_step in float64, both column-sum forms where the as-written one is defined: every activation, gradient and new
    parameter within 1e-12 of the tensor's largest magnitude (the two differ by summation order only)."""
    d = case_data(name)
    n0, n1, n2, n3 = d["sizes"]
    p64 = [p.astype(F64) for p in d["params"]]
    for intended in (True, False):
        res = ora.mnist_step(p64, d["x_raw"].astype(F64), d["y"].astype(F64), colsum_intended=intended)
        if not intended and max(n1, n2, n3) > d["B"]:
            assert res is None and ora.col_sum_as_written(np.zeros((max(n1, n2, n3), d["B"]))) is None
            continue
        acts, grads, new = step64(d["params"], d["x_raw"], d["y"], col_sum=None if intended else ora.col_sum_as_written)
        o_new, o_acts, o_grads = res
        pairs = [(n, acts[n], o_acts[n]) for n in ACTS[:6]] + list(zip(GN, grads, o_grads)) + list(zip(PN, new, o_new))
        for n, mine, theirs in pairs:
            assert mine.shape == theirs.shape, (name, n)
            assert np.abs(mine - theirs).max() <= 1e-12 * np.abs(theirs).max(), (name, intended, n, np.abs(mine - theirs).max() / np.abs(theirs).max())


@pytest.mark.parametrize("name", list(CASES))
def test_reference_gates_are_clear_of_zero(name):
    assert gates_clear(case_data(name)["acts"])


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(pkg):
    pkg.init(0)
    pkg.lib().bla_gemm_set_config(-1, 0)
    return pkg


def last_name(dev):
    return dev.lib().bla_gemm_last_kernel().decode()


def is_tiled(name):
    return re.match(r"gemm_f32_(t|glds)\d+x\d+x\d+[a-z0-9]*_", name) is not None and "wsk" not in name


def trainer(dev, d, mode=1, x_raw=None, y=None):
    nn = dev.mnist_nn.MnistNN(d["B"], d["sizes"], mode)
    nn.set_params(d["params"])
    nn.load_batch(d["x_raw"] if x_raw is None else x_raw, d["y"] if y is None else y)
    return nn


def read_device(dev, ptr, shape, dtype=F32):
    out = np.empty(shape, dtype)
    dev.sync()
    dev.native.check(dev.lib().bla_memcpy_d2h(out.ctypes.data, ptr, out.nbytes, None))
    dev.sync()
    return out


def forward_only(dev, nn):
    dev.native.check(dev.lib().bla_mnist_nn_forward(nn.h, None, None, None))


def ratio(got, ref, atol=None):
    """max |got - ref| / bound; bound = 1e-5 (|ref| + mean|ref|), or 1e-5 |ref| + atol for parameters.  NaN (an unwritten or poisoned element) fails."""
    ref = np.asarray(ref, F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    bound = RTOL * (np.abs(ref) + np.abs(ref).mean()) if atol is None else RTOL * np.abs(ref) + atol
    r = np.abs(got.astype(F64) - ref) / bound
    return float("nan") if np.isnan(r).any() else float(r.max())


def same_params(p, q):
    return all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(p, q))


def fused_bounds(p, q, p0):
    """p: parameters after the fused-update step, q: after train_step, p0: before (test_graph_replay_matches_eager's two normwise bounds)."""
    for a, b, s in zip(p, q, p0):
        assert np.linalg.norm(a - b) <= 1e-6 * np.linalg.norm(b) + 1e-9
        assert np.linalg.norm((a - s) - (b - s)) <= 1e-5 * np.linalg.norm(b - s) + 1e-9


def check_step(dev, name, mode, ref):
    """train_step from fresh parameters against (acts, grads, new) of the float64 step; then the other step forms from the same start."""
    d = case_data(name)
    acts, grads, new = ref
    assert gates_clear(acts)
    a = trainer(dev, d, mode)
    a.train_step()
    worst = {}
    for n in ACTS:                                  # z1 first: its check is what makes the gates the reference's
        worst[n] = ratio(a.activation(n), acts[n])
        assert worst[n] <= 1, (name, n, worst[n])
    for n, got, want in zip(GN, a.grads(), grads):
        worst[n] = ratio(got, want)
        assert worst[n] <= 1, (name, n, worst[n])
    pa = a.get_params()
    for n, got, want in zip(PN, pa, new):
        worst["new_" + n] = ratio(got, want, atol=1e-7)
        assert worst["new_" + n] <= 1, (name, n, worst["new_" + n])
    top = max(worst, key=worst.get)
    print(f"\ncase {name} mode {mode}: worst error / bound = {worst[top]:.3f} ({top}); " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))

    b, c, e = trainer(dev, d, mode), trainer(dev, d, mode), trainer(dev, d, mode)
    b.graph_step(with_update=False); b.apply()
    c.graph_step()
    e.fused_step()
    pb, pc, pe = b.get_params(), c.get_params(), e.get_params()
    assert same_params(pb, pa), "graph replay of forward/backward + apply differs from train_step"
    assert same_params(pc, pe), "graph_step and fused_step differ"
    if FUSED_UPDATE[name] and mode == 1:
        fused_bounds(pc, pa, d["params"])
        for n, got, want in zip(PN, pc, new):
            r = ratio(got, want, atol=1e-7)
            assert r <= 1, (name, "fused", n, r)
    else:
        assert same_params(pc, pa), "the fallback of fused_step / graph_step differs from train_step"
    return a


def expect_last(dev, name, prefix, part=None):
    got = last_name(dev)
    assert got.startswith(prefix) and (part is None or part in got), f"case {name}: expected {prefix}*{part or ''}, ran {got}"


@gpu
def test_case_a_everything_odd(dev):
    d = case_data("A")
    nn = trainer(dev, d)
    forward_only(dev, nn); expect_last(dev, "A", "gemm_f32_wsk32x32_nn_ss_")            # output product: scalar loads on both operands, 32x32 tile
    nn.forward_backward(); expect_last(dev, "A", "gemm_f32_wsk32x32_nt_ss_")            # dW1 alone: the {dW2 | dW1} pair is not shared
    offs = np.cumsum([0] + [r * c for r, c in dev.mnist_nn.bucket_shapes(d["sizes"])])
    assert offs[2] % 4 != 0 and offs[4] % 4 != 0                                        # W2 and W3 start off 16-byte boundaries inside the bucket
    check_step(dev, "A", 1, (d["acts"], d["grads"], d["new"]))


@gpu
def test_case_a_as_written_is_refused(dev):
    d = case_data("A")
    for step in ("train_step", "fused_step"):
        nn = trainer(dev, d, mode=0)
        with pytest.raises(dev.BlaError) as e:
            getattr(nn, step)()
        assert e.value.status == UNDEFINED
        assert same_params(nn.get_params(), d["params"])


@gpu
@pytest.mark.parametrize("mode", [1, 0])
def test_case_b_both_column_sums(dev, ora, mode):
    d = case_data("B")
    nn = trainer(dev, d, mode)
    forward_only(dev, nn); expect_last(dev, "B", "gemm_f32_wsk32x32_nn_ss_")
    ref = (d["acts"], d["grads"], d["new"]) if mode == 1 else step64(d["params"], d["x_raw"], d["y"], col_sum=ora.col_sum_as_written)
    if mode == 0:      # the two forms must differ here, or the as-written run would prove nothing
        assert max(np.abs(g - h).max() / np.abs(h).max() for g, h in zip(ref[1][1::2], d["grads"][1::2])) > 0.1
    check_step(dev, "B", mode, ref)


@gpu
def test_case_c_softmax_tail_on_the_32x32_tile(dev):
    d = case_data("C")
    nn = trainer(dev, d)
    forward_only(dev, nn); expect_last(dev, "C", "gemm_f32_wsk32x32_nn_vv_")            # 16 < n3: the fused tail cannot take the 16x16 tile
    nn.forward_backward(); expect_last(dev, "C", "gemm_f32_wsk_pair_nt+nt_")
    check_step(dev, "C", 1, (d["acts"], d["grads"], d["new"]))


@gpu
def test_case_d_unfused_softmax(dev):
    d = case_data("D")
    nn = trainer(dev, d)
    assert dev.lib().bla_mnist_nn_metrics_enable(nn.h, 1) == INVALID                    # no fused tail, hence no device-side bookkeeping
    forward_only(dev, nn); expect_last(dev, "D", "gemm_f32_wsk16x16_nn_vv_")            # the plain output product (40 x 64 x 64) ...
    nn.forward_backward(); expect_last(dev, "D", "gemm_f32_wsk_pair_nt+nt_")
    check_step(dev, "D", 1, (d["acts"], d["grads"], d["new"]))                          # ... with A3 = softmax(Z3) and dZ3 from the separate pass


@gpu
def test_case_e_first_product_on_a_tiled_kernel(dev):
    d = case_data("E")
    n0, n1 = d["sizes"][:2]; B = d["B"]
    nn = trainer(dev, d)
    forward_only(dev, nn); expect_last(dev, "E", "gemm_f32_wsk16x16_nn_vv_")
    z1, a1 = nn.activation("z1"), nn.activation("a1")
    # bla_gemm_last_kernel names the last product only, so layer 1 is issued once more exactly as forward_pass issues it -- the trainer's own
    # operands, pitches and epilogue -- and must name a tiled kernel and reproduce the trainer's Z1 / A1 bit for bit
    L, nat = dev.lib(), dev.native
    zp, ap, rows = C.c_void_p(), C.c_void_p(), C.c_int()
    nat.check(L.bla_mnist_nn_activation(nn.h, 0, C.byref(zp), C.byref(rows)))
    nat.check(L.bla_mnist_nn_activation(nn.h, 1, C.byref(ap), C.byref(rows)))
    ep = nat.Epilogue()
    ep.alpha = float(F32(1) / F32(255)); ep.bias_row = nn.params_ptr + 4 * n1 * n0; ep.pre_act = zp.value; ep.ld_pre = B; ep.act = nat.ACT_RELU
    dev.sync()
    nat.check(L.bla_memset(zp.value, 0xFF, z1.nbytes, None)); nat.check(L.bla_memset(ap.value, 0xFF, a1.nbytes, None))
    nat.check(L.bla_gemm_f32(None, 0, 0, n1, B, n0, nn.params_ptr, n0, L.bla_mnist_nn_input(nn.h), B, ap.value, B, C.byref(ep)))
    assert is_tiled(last_name(dev)), last_name(dev)
    assert np.array_equal(nn.activation("z1"), z1) and np.array_equal(nn.activation("a1"), a1)
    nn.forward_backward(); expect_last(dev, "E", "gemm_f32_wsk_pair_nt+nt_")
    check_step(dev, "E", 1, (d["acts"], d["grads"], d["new"]))


@gpu
def test_case_f_weight_gradients_on_tiled_kernels(dev):
    d = case_data("F")
    nn = trainer(dev, d)
    forward_only(dev, nn); expect_last(dev, "F", "gemm_f32_wsk16x16_nn_vv_")            # 10 x 1296 x 16 with the fused tail
    nn.forward_backward()
    assert is_tiled(last_name(dev)) and "_nt_" in last_name(dev), last_name(dev)        # dW1 (k = B > 1280) left the wave-split-K kernel, db1 deferred
    check_step(dev, "F", 1, (d["acts"], d["grads"], d["new"]))


@gpu
def test_graph_is_captured_again_when_its_arguments_change(dev):
    """graph_step bakes lr, the column-sum form and with_update into the captured graph: a change of any of them must capture again.  The eager twin
    issues the same launches directly (fused_step where the graph holds the fused update, train_step where it holds forward/backward + axpy), so the
    parameters are bit-identical after every step; a third trainer on train_step alone bounds the fused rounding.  Case C: every width <= B, so the
    as-written column sum is defined too."""
    d = case_data("C")
    lr_a, lr_b = LR, float(F32(-0.05))
    g, twin, plain = trainer(dev, d), trainer(dev, d), trainer(dev, d)

    def compare(fused):
        pg, pt, pp = g.get_params(), twin.get_params(), plain.get_params()
        assert same_params(pg, pt)
        if fused: fused_bounds(pg, pp, d["params"])
        else: assert same_params(pg, pp)

    g.graph_step(lr=lr_a); twin.fused_step(lr=lr_a); plain.train_step(lr=lr_a); compare(True)
    g.graph_step(lr=lr_b); twin.fused_step(lr=lr_b); plain.train_step(lr=lr_b); compare(True)          # a stale graph would move by lr_a
    g.graph_step(lr=lr_b, with_update=False); g.apply(lr_b); twin.train_step(lr=lr_b); plain.train_step(lr=lr_b); compare(True)
    # from a common state: the column-sum form changes (as written: no fused update, separate column sums), then back
    for nn in (g, twin, plain):
        nn.set_params(d["params"]); nn.colsum_mode = 0
    g.graph_step(lr=lr_b); twin.train_step(lr=lr_b); plain.fused_step(lr=lr_b); compare(False)
    for nn in (g, twin, plain):
        nn.colsum_mode = 1
    before = g.get_params()
    g.graph_step(lr=lr_b); twin.fused_step(lr=lr_b)
    assert same_params(g.get_params(), twin.get_params())
    assert min(np.abs(a - b).max() for a, b in zip(g.get_params(), before)) > 0                          # every tensor moved


@gpu
@pytest.mark.parametrize("name", ["A", "F"])
def test_three_steps_track_the_float64_trajectory(dev, name):
    """Three consecutive fused_step calls with new pixels and labels each (parameters feed back) against the float64 trajectory, normwise 1e-5."""
    d = case_data(name)
    p64 = [p.astype(F64) for p in d["params"]]
    nn = trainer(dev, d)
    for s in TRAJECTORY_SEEDS[name]:
        x_raw, y = make_batch(d["sizes"], d["B"], s, s + 50)
        acts, _, p64 = step64(p64, x_raw, y)
        assert gates_clear(acts), (name, s)
        nn.load_batch(x_raw, y); nn.fused_step()
    worst = 0.0
    for got, ref in zip(nn.get_params(), p64):
        worst = max(worst, np.linalg.norm(got - ref) / (RTOL * np.linalg.norm(ref) + 1e-7))
        assert np.linalg.norm(got - ref) <= RTOL * np.linalg.norm(ref) + 1e-7
    print(f"\ncase {name}, three steps: worst normwise error / bound = {worst:.3f}")


def metrics_read(dev, nn, reset=0):
    loss, count = C.c_double(), C.c_longlong()
    dev.native.check(dev.lib().bla_mnist_nn_metrics_read(nn.h, C.byref(loss), C.byref(count), reset))
    return loss.value, count.value


@gpu
@pytest.mark.parametrize("name", ["A", "C"])
def test_metrics_from_the_output_layer(dev, ora, name):
    """Loss and accuracy accumulated by the output layer's launch against oracle.mnist_metrics of the float64 A3: the count exactly (asserted
    first on the reference alone: every column's winning probability leads the runner-up by more than 1e-4, fp32 cannot reorder them), the loss
    within 1e-5 relative."""
    d = case_data(name)
    acts, B = d["acts"], d["B"]
    top = np.sort(acts["a3"], axis=0)
    assert ((top[-1] - top[-2]) > 1e-4).all()                                                           # holds for the cases' own seeds (margin 1.1e-3)
    loss, count = ora.mnist_metrics(acts["a3"], d["y"])
    assert 0 < count < B and loss > 0
    L, nat = dev.lib(), dev.native
    nn = trainer(dev, d)
    out_l, out_c = C.c_double(), C.c_longlong()
    assert L.bla_mnist_nn_metrics_read(nn.h, C.byref(out_l), C.byref(out_c), 0) == INVALID            # before enable
    nat.check(L.bla_mnist_nn_metrics_enable(nn.h, 1))
    assert metrics_read(dev, nn) == (0.0, 0)
    forward_only(dev, nn)
    expect_last(dev, name, "gemm_f32_wsk32x32_")
    got_l, got_c = metrics_read(dev, nn)
    assert got_c == count and abs(got_l - loss) <= 1e-5 * loss, (got_l, loss, got_c, count)
    forward_only(dev, nn)
    got_l, got_c = metrics_read(dev, nn, reset=1)
    assert got_c == 2 * count and abs(got_l - 2 * loss) <= 1e-5 * 2 * loss
    assert metrics_read(dev, nn) == (0.0, 0)                                                            # reset cleared both
    nn.train_step()                                                                                     # same parameters, same batch: the same terms
    got_l, got_c = metrics_read(dev, nn)
    assert got_c == count and abs(got_l - loss) <= 1e-5 * loss
    nat.check(L.bla_mnist_nn_metrics_enable(nn.h, 0))
    assert L.bla_mnist_nn_metrics_read(nn.h, C.byref(out_l), C.byref(out_c), 0) == INVALID


@gpu
@pytest.mark.parametrize("name", ["A", "C"])
def test_gather_batch_is_bit_exact(dev, name):
    d = case_data(name)
    (n0, _, _, n3), B, N = d["sizes"], d["B"], 101
    X = randint(9400, (n0, N), 256).astype(F32)                       # feature-major dataset
    labels = randint(9401, (N,), n3).astype(F32)
    idx = randint(9402, (B,), N).astype(np.int32)
    idx[0], idx[1], idx[2], idx[B - 1] = N - 1, 0, N - 1, idx[3]      # both ends, and repeats
    want_x = np.ascontiguousarray(X[:, idx])
    want_y = np.zeros((n3, B), F32); want_y[labels[idx].astype(int), np.arange(B)] = 1
    L, nat = dev.lib(), dev.native
    dX, dl, di = dev.to_device(X), dev.to_device(labels), dev.to_device(idx, np.int32)
    nn = trainer(dev, d, x_raw=np.full((n0, B), 777, F32), y=np.full((n3, B), 5, F32))       # resident buffers start as garbage
    for args in [(None, dl.ptr, N, di.ptr), (dX.ptr, None, N, di.ptr), (dX.ptr, dl.ptr, N, None), (dX.ptr, dl.ptr, 0, di.ptr), (dX.ptr, dl.ptr, -3, di.ptr)]:
        assert L.bla_mnist_nn_gather_batch(nn.h, None, *args) == INVALID
    assert L.bla_mnist_nn_gather_batch(None, None, dX.ptr, dl.ptr, N, di.ptr) == INVALID
    nat.check(L.bla_mnist_nn_gather_batch(nn.h, None, dX.ptr, dl.ptr, N, di.ptr))
    assert np.array_equal(read_device(dev, L.bla_mnist_nn_input(nn.h), (n0, B)), want_x)
    assert np.array_equal(read_device(dev, L.bla_mnist_nn_labels(nn.h), (n3, B)), want_y)
    nn.train_step()
    twin = trainer(dev, d, x_raw=want_x, y=want_y)
    twin.train_step()
    assert same_params(nn.get_params(), twin.get_params()) and same_params(nn.grads(), twin.grads())
    assert not same_params(nn.get_params(), d["params"])


@gpu
def test_argument_checks(dev):
    L = dev.lib()
    h = C.c_void_p()
    for sizes, batch in [((12, 8, 6, 4), 0), ((12, 8, 6, 4), -1), ((0, 8, 6, 4), 16), ((12, 0, 6, 4), 16), ((12, 8, 0, 4), 16), ((12, 8, 6, 0), 16)]:
        assert L.bla_mnist_nn_create(C.byref(h), (C.c_int * 4)(*sizes), batch) == INVALID and not h.value
    nn = dev.mnist_nn.MnistNN(16, (12, 8, 6, 4))
    p, rows = C.c_void_p(), C.c_int()
    for which in (-1, 9):
        assert L.bla_mnist_nn_activation(nn.h, which, C.byref(p), C.byref(rows)) == INVALID
    assert L.bla_mnist_nn_activation(nn.h, 8, C.byref(p), C.byref(rows)) == 0 and rows.value == 8 and p.value
    other_p, other_g = dev.zeros((nn.count,)), dev.zeros((nn.count,))
    nn.load_batch(np.zeros((12, 16), F32), np.zeros((4, 16), F32))
    nn.graph_step()
    dev.sync()
    assert L.bla_mnist_nn_use_buckets(nn.h, other_p.ptr, other_g.ptr) == INVALID                         # the captured graph holds the old buckets
    assert nn.params_ptr != other_p.ptr
