"""Direct pin: oracle (fp64) == the reference itself bit for bit on fresh random shapes.  The reference's results for exactly these
inputs are recorded in tests/golden/oracle_vs_ref.npz (oracle/gen_golden.py, from oracle/_ref/libref.so = the reference's
lib/*.c compiled by oracle/Makefile), so the pin holds on every machine; where that reference build exists, every recorded value
is also recomputed through it and must still be what it computes."""
import ctypes as C

import numpy as np
import pytest

import ref
from conftest import golden
from inputs import uniform

FIX = golden("oracle_vs_ref")


def the_reference(name, live):
    """The reference's result for case `name`: the recorded one, checked against the reference itself where its build exists."""
    want = FIX[name]
    if ref.available():
        assert np.array_equal(live(), want, equal_nan=True), f"{name}: tests/golden/oracle_vs_ref.npz differs from the reference build"
    return want


@pytest.mark.parametrize("seed", range(12))
def test_matmul_random(ora, seed):
    rng = np.random.default_rng(seed)
    m, k, n = [int(v) for v in rng.integers(1, 90, 3)]
    a = uniform(seed * 3 + 1, (m, k), -3, 3); b = uniform(seed * 3 + 2, (k, n), -3, 3)
    assert np.array_equal(ora.matmul(a, b), the_reference(f"matmul_s{seed}", lambda: ref.matmul(a, b)))
    assert np.array_equal(ora.matmul(a, b), the_reference(f"matmul_inplace_s{seed}", lambda: ref.matmul_inplace(a, b)))


@pytest.mark.parametrize("shape", [(1, 1), (5, 9), (9, 5), (31, 64), (64, 64)])
def test_elementwise_and_reductions(ora, shape):
    a = uniform(11, shape, -2, 2); b = uniform(12, shape, -2, 2)
    t = f"ew_{shape[0]}x{shape[1]}_"
    assert np.array_equal(ora.scale(a, 1 / 3), the_reference(t + "scale", lambda: ref.inplace1("matrix_scale", a, C.c_double(1 / 3))))
    assert np.array_equal(ora.add(a, b), the_reference(t + "add", lambda: ref.inplace2("matrix_add", a, b)))
    assert np.array_equal(ora.hadamard(a, b), the_reference(t + "hadamard", lambda: ref.inplace2("matrix_multiply_elementwise", a, b)))
    assert np.array_equal(ora.transpose(a), the_reference(t + "transpose", lambda: ref.inplace1("matrix_transpose", a)))
    assert np.array_equal(ora.row_sum(a), the_reference(t + "row_sum", lambda: ref.take(ref.lib().matrix_row_sum(ref.mat(a)))))
    if shape[0] <= shape[1]:
        assert np.array_equal(ora.col_sum_as_written(a), the_reference(t + "col_sum", lambda: ref.take(ref.lib().matrix_col_sum(ref.mat(a)))))
    assert ora.frobenius(a) == the_reference(t + "frobenius", lambda: np.array(ref.lib().frobenius_norm(ref.mat(a))))
    assert ora.max_value(a) == the_reference(t + "max", lambda: np.array(ref.lib().max_value(ref.mat(a))))
    assert np.array_equal(ora.zscore(a), the_reference(t + "zscore", lambda: ref.inplace1("matrix_z_score_normalize", a)), equal_nan=True)  # 1x1 is 0/0 in both
    assert np.array_equal(ora.relu(a), the_reference(t + "relu", lambda: ref.data_fn("relu", a, a.size)))
    assert np.array_equal(ora.softmax_cols(a), the_reference(t + "softmax_cols", lambda: ref.data_fn("softmax", a, *shape)))
    assert np.array_equal(ora.softmax_rows(a), the_reference(t + "softmax_rows", lambda: ref.data_fn("softmax_row_wise", a, *shape)))


@pytest.mark.parametrize("cfg", [(4, 4, 1, 1, 3, 1), (9, 6, 2, 3, 3, 2), (10, 10, 3, 2, 1, 2), (5, 5, 2, 2, 3, 3)])
def test_im2col_geometry(ora, cfg):
    h, w, cin, cout, k, s = cfg
    x = uniform(21, (cin, h, w))
    ho, wo = ora.out_hw(h, w, s)

    def live():
        im = np.zeros((ho * wo, k * k * cin)); imm = ref.mat(im)
        ref.lib()._im2col(ref.mats(x), C.byref(imm), k, cin, s)
        return im
    assert np.array_equal(ora.im2col(x, k, s), the_reference("im2col_" + "_".join(map(str, cfg)), live))
