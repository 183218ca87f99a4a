"""Every group-norm kernel path of csrc/bla_group_norm.hip, held element by element to a derived rounding bound against a float64 reference.

The family is eight kernels behind launch_group_norm<RELU> and launch_group_norm_ddx: one workgroup per group or slices of 2,048 elements, 16-byte or
scalar loads -- chosen by the size of a full group and by alignment (`path_of` below restates the rule, and a host test asserts that the case table
reaches all four paths).  The batched entries add fold_groups (same file).  Every output is a view inside a larger allocation pre-filled with
0xFF bytes whose guard floats must come back untouched; an element a kernel does not write stays NaN and fails every bound.

Bounds, u = 2^-24 (m, v: the mean and variance the device returned; v is what `stdevs` holds and what the output is divided by -- the reference's quirk):
  mean      within 1 fp32 ulp of the float64 mean (one rounding of an fp64 sum)
  variance  |v - v*| <= 4u v*,  v* = mean((x - m)^2) in float64
  output    |out - y*| <= 4u |y*|,  y* = (x - m) / v in float64 (an fp32 subtraction, then an IEEE fp32 division); with ReLU against max(y*, 0)
  dropped   exactly where(drop, 0, relu_out)
  gradient  sv = gate <= 0 ? 0 : source, nv = (data - m) / v, A = mean(sv), B = mean(nv sv), Bbar = mean|nv sv|, r* = (sv - A - nv B) / v + addend:
            |dest - r*| <= 10u (|sv| + |A| + |nv| Bbar) / |v| + u |addend|
            (nv 2u, fgws 3u Bbar, two subtractions, the product, the division and the final add one u each, the rest slack for ordering)

The host tests (no gpu marker) run a numpy float32 restatement of the kernels' formulas through the same bound functions -- inside every bound as
written, outside under each mutation (a slice left out of the sums, the tail of a group not written, the gate ignored, the addend dropped) -- so the
bounds' sharpness is pinned on a machine without a GPU."""
import functools

import numpy as np
import pytest

from inputs import uniform

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
GUARD = 64            # guard elements on either side of every view (256 bytes of floats: a view keeps the 16-byte alignment of its allocation)
ONE_WG_MAX = 16384    # kGnThreads * kGnRegs / 2 = kGnThreads * kGnVec * 4
SLICE = 2048          # kGnSlice


def path_of(channels, group_size, hw, aligned=True):
    """The dispatch rule both launchers take from gn_route (csrc/bla_group_norm.hip), each with its own alignment predicate: one workgroup per group up to
    16,384 elements in a full group, slices beyond; 16-byte kernels when hw is a multiple of 4 and every tensor pointer is 16-byte aligned."""
    n_max = min(channels, group_size) * hw
    vec = hw % 4 == 0 and aligned
    return ("one-wg" if n_max <= ONE_WG_MAX else "sliced") + (" 16-byte" if vec else " scalar")


# (channels, group_size, hw, shift): shift = floats by which every pointer is moved off its 16-byte alignment
DIRECT = [
    (3, 32, 64, 0),          # 192 per group: a short single group
    (2, 1, 4, 0),            # one live thread
    (32, 32, 260, 0),        # 8,320: third float4 slot barely used
    (40, 16, 1020, 0),       # 16,320 / 8,160: fourth slot partly masked, ragged last group
    (64, 32, 512, 0),        # 16,384: the threshold itself, every slot full
    (4, 2, 1, 0),            # hw = 1
    (32, 32, 33, 0),         # 1,056: second register slot barely used
    (32, 32, 511, 0),        # 16,352: all 16 slots, the last partly
    (64, 32, 512, 1),        # alignment alone forces the scalar one-workgroup kernels
    (32, 32, 516, 0),        # 16,512: first size over the threshold, last slice 128 elements
    (3, 1, 16388, 0),        # last slice is one float4
    (48, 32, 516, 0),        # ragged last group leaves launched slices empty (lo >= n)
    (40, 32, 1024, 0),       # 32,768 / 8,192
    (3, 1, 16385, 0),        # last slice is one element
    (32, 32, 513, 0),        # odd hw
    (3, 32, 16386, 0),       # 49,158: 25 slices
    (64, 32, 1024, 1),       # alignment alone forces the scalar sliced kernels
]
PATHS = ["one-wg 16-byte"] * 5 + ["one-wg scalar"] * 4 + ["sliced 16-byte"] * 4 + ["sliced scalar"] * 4
SHIFTED = [(40, 32, 1024, 0), (64, 32, 512, 0)]     # forward only, data in [1000, 1001): the sliced and the one-workgroup 16-byte kernels
BATCHED = [
    (5, 64, 32, 64),         # folds into 10 groups
    (5, 3, 32, 64),          # folds with the group shortened to 3
    (3, 40, 16, 64),         # ragged: image by image
    (1, 40, 16, 64),         # batch 1
    (64, 128, 32, 64),       # 256 groups in one launch
    (2, 32, 32, 529),        # scalar sliced under the fold
]
RESNET = [
    (2, 32, 16, 16, 32),     # one-wg 16-byte
    (2, 32, 15, 15, 32),     # one-wg scalar, 8 slots
    (2, 32, 24, 24, 32),     # sliced 16-byte
    (2, 32, 23, 23, 32),     # sliced scalar
    (1, 32, 24, 24, 32),     # the single-image block
]


def case_id(cfg):
    return "x".join(str(v) for v in cfg)


# ---- the float64 reference and the bounds --------------------------------------------------------------------------------------------------------
def groups_of(channels, group_size, hw):
    """[lo, hi) of every group in the flat [channels * hw] tensor; the last group may be short"""
    return [(g * group_size * hw, min(channels, (g + 1) * group_size) * hw) for g in range((channels + group_size - 1) // group_size)]


def ref_stats(x, channels, group_size, hw):
    """float64 mean and variance (about that mean) per group"""
    x = x.astype(F64).ravel()
    mean = np.array([x[lo:hi].mean() for lo, hi in groups_of(channels, group_size, hw)])
    var = np.array([((x[lo:hi] - m) ** 2).mean() for (lo, hi), m in zip(groups_of(channels, group_size, hw), mean)])
    return mean, var


def ref_forward(x, m, v, channels, group_size, hw):
    """y* = (x - m) / v in float64: `stdevs` holds the variance and the output is divided by it"""
    x = x.astype(F64).ravel(); y = np.empty_like(x)
    for g, (lo, hi) in enumerate(groups_of(channels, group_size, hw)):
        with np.errstate(divide="ignore", invalid="ignore"):      # (a mutation below may return a zero variance)
            y[lo:hi] = (x[lo:hi] - F64(m[g])) / F64(v[g])
    return y


def ref_gradient(source, data, m, v, channels, group_size, hw, gate=None, addend=None):
    """(r*, bound): an exact function of the fp32 inputs, and the rounding bound of the module docstring"""
    s = source.astype(F64).ravel(); d = data.astype(F64).ravel()
    sv = s if gate is None else np.where(gate.astype(F64).ravel() <= 0, 0.0, s)
    ad = np.zeros_like(s) if addend is None else addend.astype(F64).ravel()
    r = np.empty_like(s); bound = np.empty_like(s)
    for g, (lo, hi) in enumerate(groups_of(channels, group_size, hw)):
        mg, vg = F64(m[g]), F64(v[g])
        nv = (d[lo:hi] - mg) / vg
        A = sv[lo:hi].mean(); B = (nv * sv[lo:hi]).mean(); Bbar = np.abs(nv * sv[lo:hi]).mean()
        r[lo:hi] = (sv[lo:hi] - A - nv * B) / vg + ad[lo:hi]
        bound[lo:hi] = 10 * U * (np.abs(sv[lo:hi]) + abs(A) + np.abs(nv) * Bbar) / abs(vg) + U * np.abs(ad[lo:hi])
    return r, bound


def worst(err, bound):
    """the largest err / bound: <= 1 means every element is inside its bound; inf for a NaN or for an error where the bound is zero"""
    err = np.atleast_1d(np.asarray(err, F64)); bound = np.atleast_1d(np.asarray(bound, F64))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isfinite(err) & np.isfinite(bound), r, np.inf)
    return float(r.max())


def forward_fractions(x, m, v, out, channels, group_size, hw, relu):
    """worst fraction of the mean, variance and output bounds that the returned (m, v, out) use"""
    x64 = x.astype(F64).ravel()
    mean64, _ = ref_stats(x, channels, group_size, hw)
    m64, v64 = np.asarray(m, F64).ravel(), np.asarray(v, F64).ravel()
    vstar = np.array([((x64[lo:hi] - m64[g]) ** 2).mean() for g, (lo, hi) in enumerate(groups_of(channels, group_size, hw))])
    y = ref_forward(x, m64, v64, channels, group_size, hw)
    want = np.maximum(y, 0) if relu else y
    with np.errstate(invalid="ignore"):
        err = np.abs(out.astype(F64).ravel() - want)
    return dict(mean=worst(np.abs(m64 - mean64), np.spacing(np.abs(mean64).astype(F32)).astype(F64)),
                variance=worst(np.abs(v64 - vstar), 4 * U * vstar),
                output=worst(err, 4 * U * np.abs(y)))


def gradient_fraction(dest, source, data, m, v, channels, group_size, hw, gate=None, addend=None):
    r, bound = ref_gradient(source, data, m, v, channels, group_size, hw, gate, addend)
    return worst(np.abs(dest.astype(F64).ravel() - r), bound)


# ---- inputs: generated once per shape and shared ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs_for(channels, group_size, hw, seed, lo=-1.0, hi=3.0):
    """data in [-1, 3) (or the shifted range), source in [-0.5, 1.5) -- a non-zero mean, so the sums matter --, gate and addend in [-1, 1);
    m, v: the float64 statistics rounded to fp32, the gradient's inputs"""
    n = channels * hw
    I = dict(data=uniform(seed, (n,), lo, hi, F32), source=uniform(seed + 1, (n,), -0.5, 1.5, F32), gate=uniform(seed + 2, (n,), -1, 1, F32),
             addend=uniform(seed + 3, (n,), -1, 1, F32))
    mean, var = ref_stats(I["data"], channels, group_size, hw)
    assert (var > 0).all()      # no constant group: the reference divides by a zero variance there, which is not under test
    I["m"], I["v"] = mean.astype(F32), var.astype(F32)
    for a in I.values():
        a.setflags(write=False)
    return I


def direct_inputs(i):
    c, gs, hw, _ = DIRECT[i]
    return inputs_for(c, gs, hw, 5000 + 10 * i)


def gate_addend(I, with_gate, with_addend):
    return (I["gate"] if with_gate else None), (I["addend"] if with_addend else None)


# ---- numpy float32 restatement of the kernels' formulas ----------------------------------------------------------------------------------------------------
def chunk_of(sliced):
    return SLICE if sliced else 1024      # a slice of the sliced kernels; one register slot of the one-workgroup kernels


def kept(n, sliced, skip_last_chunk):
    """which elements of a group enter the sums: all of them, or (the mutation) all but the group's last chunk"""
    keep = np.ones(n, bool)
    if skip_last_chunk:
        keep[(n - 1) // chunk_of(sliced) * chunk_of(sliced):] = False
    return keep


def restate_forward(x, channels, group_size, hw, sliced, relu, skip_last_chunk=False, unwritten=0):
    """group_norm_kernel / group_norm_vec_kernel (variance in a second pass about the float mean) and, sliced, group_norm_stats_kernel +
    group_norm_apply_kernel (sum x and sum x^2 in fp64, variance (sum x^2 - 2 m sum x + n m^2) / n).  Every fp32 operation rounds once (no FMA)."""
    x = x.ravel(); out = np.full(x.shape, np.nan, F32); ms, vs = [], []
    for lo, hi in groups_of(channels, group_size, hw):
        xs = x[lo:hi]; n = hi - lo; keep = kept(n, sliced, skip_last_chunk)
        a = xs.astype(F64)[keep].sum()
        mean = F32(a / n)
        if sliced:
            b = (xs.astype(F64)[keep] ** 2).sum(); m = F64(mean)
            var = F32((b - 2.0 * m * a + n * m * m) / n)
        else:
            var = F32(((xs - mean).astype(F64)[keep] ** 2).sum() / n)
        with np.errstate(divide="ignore", invalid="ignore"):
            y = (xs - mean) / var
        assert y.dtype == F32
        if relu:
            y = np.where(y < 0, F32(0), y)
        out[lo:hi - unwritten] = y[:n - unwritten]
        ms.append(mean); vs.append(var)
    return np.array(ms, F32), np.array(vs, F32), out


def restate_gradient(source, data, m, v, channels, group_size, hw, sliced, gate=None, addend=None, skip_last_chunk=False, unwritten=0):
    """group_norm_ddx_kernel / _vec_kernel and group_norm_ddx_stats_kernel + _apply_kernel: the same arithmetic on either path"""
    source, data = source.ravel(), data.ravel(); out = np.full(source.shape, np.nan, F32)
    for g, (lo, hi) in enumerate(groups_of(channels, group_size, hw)):
        n = hi - lo; keep = kept(n, sliced, skip_last_chunk)
        sv = source[lo:hi] if gate is None else np.where(gate.ravel()[lo:hi] <= 0, F32(0), source[lo:hi])
        nv = (data[lo:hi] - m[g]) / v[g]
        fgs = F32(sv.astype(F64)[keep].sum() / n)
        fgws = F32((nv.astype(F64) * sv.astype(F64))[keep].sum() / n)
        d = (sv - fgs - nv * fgws) / v[g]
        if addend is not None:
            d = d + addend.ravel()[lo:hi]
        assert d.dtype == F32
        out[lo:hi - unwritten] = d[:n - unwritten]
    return out


def host_cases():
    """every shape of the three tables as (channels, group_size, hw, seed, lo, hi, sliced): a batch is the same groups image after image"""
    out = [(c, gs, hw, 5000 + 10 * i, -1.0, 3.0) for i, (c, gs, hw, _) in enumerate(DIRECT)]
    out += [(c, gs, hw, 5400 + 10 * i, 1000.0, 1001.0) for i, (c, gs, hw, _) in enumerate(SHIFTED)]
    out += [(c, gs, hw, 5600 + 10 * i, -1.0, 3.0) for i, (_, c, gs, hw) in enumerate(BATCHED)]
    out += [(c, gs, h * w, 5800 + 10 * i, -1.0, 3.0) for i, (_, c, h, w, gs) in enumerate(RESNET)]
    return [cfg + (min(cfg[0], cfg[1]) * cfg[2] > ONE_WG_MAX,) for cfg in out]


def test_case_table_reaches_every_path():
    """The table's own claims: each row takes the path it is listed under, and the rows reach all four paths -- of launch_group_norm<RELU> and of
    launch_group_norm_ddx alike, since both take the same decision from the same three numbers and the alignment."""
    got = [path_of(c, gs, hw, shift == 0) for c, gs, hw, shift in DIRECT]
    assert got == PATHS
    assert set(got) == {"one-wg 16-byte", "one-wg scalar", "sliced 16-byte", "sliced scalar"}
    assert [path_of(c, gs, hw) for c, gs, hw, _ in SHIFTED] == ["sliced 16-byte", "one-wg 16-byte"]
    assert [path_of(c, gs, h * w) for _, c, h, w, gs in RESNET] == ["one-wg 16-byte", "one-wg scalar", "sliced 16-byte", "sliced scalar", "sliced 16-byte"]
    assert path_of(64, 32, 529) == "sliced scalar"      # (2, 32, 32, 529) folded
    # the slice edges the table names
    assert 16388 % SLICE == 4 and 16385 % SLICE == 1 and 16512 % SLICE == 128 and (49158 + SLICE - 1) // SLICE == 25


def test_reference_against_the_oracle(ora):
    """the numpy reference of this file against the oracle's restatement of lib/norm.c in float64, on a ragged case"""
    c, gs, hw = 40, 16, 1020
    I = inputs_for(c, gs, hw, 5030)
    x = I["data"].astype(F64).reshape(c, 1, hw); up = I["source"].astype(F64).reshape(c, 1, hw)
    out, sd, mu = ora.group_norm(x, gs)
    mean, var = ref_stats(I["data"], c, gs, hw)
    assert np.allclose(mu, mean, rtol=1e-12, atol=0) and np.allclose(sd, var, rtol=1e-12, atol=0)
    assert np.allclose(out.ravel(), ref_forward(I["data"], mean, var, c, gs, hw), rtol=1e-11, atol=1e-13)
    r, _ = ref_gradient(I["source"], I["data"], mu, sd, c, gs, hw)
    want = ora.group_norm_ddx(up, x, mu, sd, gs).ravel()
    assert np.abs(r - want).max() <= 1e-11 * np.abs(want).max()


@pytest.mark.parametrize("cfg", host_cases(), ids=case_id)
def test_restatement_stays_inside_every_bound(cfg):
    c, gs, hw, seed, lo, hi, sliced = cfg
    I = inputs_for(c, gs, hw, seed, lo, hi)
    for relu in (False, True):
        m, v, out = restate_forward(I["data"], c, gs, hw, sliced, relu)
        f = forward_fractions(I["data"], m, v, out, c, gs, hw, relu)
        assert max(f.values()) <= 1, (cfg, relu, f)
    for with_gate in (False, True):
        for with_addend in (False, True):
            gate, addend = gate_addend(I, with_gate, with_addend)
            dest = restate_gradient(I["source"], I["data"], I["m"], I["v"], c, gs, hw, sliced, gate, addend)
            f = gradient_fraction(dest, I["source"], I["data"], I["m"], I["v"], c, gs, hw, gate, addend)
            assert f <= 1, (cfg, with_gate, with_addend, f)


@pytest.mark.parametrize("cfg", host_cases(), ids=case_id)
def test_mutations_leave_the_bounds(cfg):
    """What a subtly wrong kernel would return is outside the bounds on every shape: a slice (or register slot) left out of the statistics, the last
    float4 / last element of each group not written, the gate ignored, the addend dropped."""
    c, gs, hw, seed, lo, hi, sliced = cfg
    I = inputs_for(c, gs, hw, seed, lo, hi)
    x, s, m, v = I["data"], I["source"], I["m"], I["v"]
    tail = 4 if hw % 4 == 0 else 1
    for relu in (False, True):
        f = forward_fractions(x, *restate_forward(x, c, gs, hw, sliced, relu, skip_last_chunk=True), c, gs, hw, relu)
        assert f["mean"] > 1 and f["variance"] > 1, (cfg, relu, f)      # (the output bound is relative to the returned m, v: the statistics' own bounds catch this)
        f = forward_fractions(x, *restate_forward(x, c, gs, hw, sliced, relu, unwritten=tail), c, gs, hw, relu)
        assert f["mean"] <= 1 and f["variance"] <= 1 and f["output"] > 1, (cfg, relu, f)
    for with_gate in (False, True):
        for with_addend in (False, True):
            gate, addend = gate_addend(I, with_gate, with_addend)
            frac = lambda dest: gradient_fraction(dest, s, x, m, v, c, gs, hw, gate, addend)
            assert frac(restate_gradient(s, x, m, v, c, gs, hw, sliced, gate, addend, skip_last_chunk=True)) > 1, (cfg, with_gate, with_addend)
            assert frac(restate_gradient(s, x, m, v, c, gs, hw, sliced, gate, addend, unwritten=tail)) > 1, (cfg, with_gate, with_addend)
            if with_gate:
                assert frac(restate_gradient(s, x, m, v, c, gs, hw, sliced, None, addend)) > 1, (cfg, with_addend)
            if with_addend:
                assert frac(restate_gradient(s, x, m, v, c, gs, hw, sliced, gate, None)) > 1, (cfg, with_gate)


# ---- on the device -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev(pkg):
    pkg.init(0)
    return pkg


class View:
    """A tensor inside a larger allocation pre-filled with 0xFF bytes: GUARD elements before and after it (and `shift` more in front, which moves the
    pointer off its alignment).  numpy() returns the tensor after checking that every guard byte is still 0xFF."""

    def __init__(self, dev, shape, init=None, shift=0, dtype=F32):
        self.shape = tuple(int(s) for s in np.atleast_1d(shape)); self.n = int(np.prod(self.shape)); self.dtype = np.dtype(dtype)
        self.lead = GUARD + shift
        total = self.lead + self.n + GUARD
        if init is None:
            self.base = dev.empty((total,), dtype).fill_bytes(0xFF)
        else:
            host = np.full(total * self.dtype.itemsize, 0xFF, np.uint8).view(self.dtype)
            host[self.lead:self.lead + self.n] = np.asarray(init, self.dtype).ravel()
            self.base = dev.to_device(host, dtype)
        self.ptr = self.base.ptr + self.lead * self.dtype.itemsize

    def numpy(self):
        a = self.base.numpy()
        raw = a.view(np.uint8); isz = self.dtype.itemsize
        assert (raw[:self.lead * isz] == 0xFF).all() and (raw[(self.lead + self.n) * isz:] == 0xFF).all(), "a guard element was written"
        return a[self.lead:self.lead + self.n].reshape(self.shape).copy()


def call(dev, name, *args):
    raw = [a.ptr if isinstance(a, (View, dev.DeviceArray)) else a for a in args]
    dev.native.check(getattr(dev.lib(), name)(*raw))


FRACTIONS = {}      # (path, quantity) -> worst fraction of its bound seen in this run


def record(path, quantity, value, tag):
    """print each figure before it is asserted; keep the worst per path"""
    FRACTIONS[(path, quantity)] = max(FRACTIONS.get((path, quantity), 0.0), value)
    print(f"group-norm bound fraction | {path} | {quantity} | {value:.3f} | worst so far {FRACTIONS[(path, quantity)]:.3f} | {tag}")
    assert value <= 1, (path, quantity, value, tag)


def run_forward(dev, entry, x, c, gs, hw, shift, batch=None):
    ng = (c + gs - 1) // gs * (batch or 1); n = c * hw * (batch or 1)
    dx = View(dev, (n,), x, shift); out, sd, mu = View(dev, (n,), None, shift), View(dev, (ng,), None, shift), View(dev, (ng,), None, shift)
    call(dev, entry, None, *([batch] if batch else []), dx, out, sd, mu, c, gs, hw)
    return mu.numpy(), sd.numpy(), out.numpy()


def run_gradient(dev, entry, I, c, gs, hw, shift, gate=None, addend=None, batch=None):
    n = c * hw * (batch or 1)
    ds, dd, dm, dv = View(dev, (n,), I["source"], shift), View(dev, (n,), I["data"], shift), View(dev, I["m"].shape, I["m"], shift), View(dev, I["v"].shape, I["v"], shift)
    dg = None if gate is None else View(dev, (n,), gate, shift); da = None if addend is None else View(dev, (n,), addend, shift)
    dest = View(dev, (n,), None, shift)
    if entry == "bla_group_norm_ddx_f32":
        call(dev, entry, None, ds, dest, dd, dm, dv, c, gs, hw)
    else:
        call(dev, entry, None, batch or 1, ds, dest, dd, dm, dv, c, gs, hw, dg, da)
    return dest.numpy()


def twice(path, run):
    """the sliced kernels add their partial sums in slice order: two runs return the same bits"""
    got = run()
    if path.startswith("sliced"):
        again = run()
        for a, b in zip(got if isinstance(got, tuple) else (got,), again if isinstance(again, tuple) else (again,)):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (path, "not bit-reproducible")
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(DIRECT)), ids=lambda i: case_id(DIRECT[i]))
def test_direct_forward(dev, i):
    c, gs, hw, shift = DIRECT[i]; path = PATHS[i]; I = direct_inputs(i)
    for entry, relu in (("bla_group_norm_f32", False), ("bla_group_norm_relu_f32", True)):
        m, v, out = twice(path, lambda: run_forward(dev, entry, I["data"], c, gs, hw, shift))
        for q, f in forward_fractions(I["data"], m, v, out, c, gs, hw, relu).items():
            record(path, q, f, (DIRECT[i], entry))


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(DIRECT)), ids=lambda i: case_id(DIRECT[i]))
def test_direct_gradient(dev, i):
    c, gs, hw, shift = DIRECT[i]; path = PATHS[i]; I = direct_inputs(i)
    dest = twice(path, lambda: run_gradient(dev, "bla_group_norm_ddx_f32", I, c, gs, hw, shift))
    record(path, "gradient", gradient_fraction(dest, I["source"], I["data"], I["m"], I["v"], c, gs, hw), (DIRECT[i], "plain"))
    for with_gate in (False, True):
        for with_addend in (False, True):
            gate, addend = gate_addend(I, with_gate, with_addend)
            dest = twice(path, lambda: run_gradient(dev, "bla_group_norm_ddx_gated_batched_f32", I, c, gs, hw, shift, gate, addend))
            record(path, "gradient", gradient_fraction(dest, I["source"], I["data"], I["m"], I["v"], c, gs, hw, gate, addend),
                   (DIRECT[i], "gate" if with_gate else "-", "addend" if with_addend else "-"))


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(SHIFTED)), ids=lambda i: case_id(SHIFTED[i]))
def test_forward_of_data_far_from_zero(dev, i):
    """data in [1000, 1001): the variance is 1e-7 of the mean square, so a variance formed carelessly from sum x^2 would be lost"""
    c, gs, hw, shift = SHIFTED[i]; path = path_of(c, gs, hw)
    x = inputs_for(c, gs, hw, 5400 + 10 * i, 1000.0, 1001.0)["data"]
    for entry, relu in (("bla_group_norm_f32", False), ("bla_group_norm_relu_f32", True)):
        m, v, out = run_forward(dev, entry, x, c, gs, hw, shift)
        for q, f in forward_fractions(x, m, v, out, c, gs, hw, relu).items():
            record(path + ", data in [1000, 1001)", q, f, (SHIFTED[i], entry))


@functools.lru_cache(maxsize=None)
def batched_inputs(i):
    """B different images; m, v laid out [B][groups], per image"""
    batch, c, gs, hw = BATCHED[i]
    per = [inputs_for(c, gs, hw, 5600 + 10 * i + 1000 * (b + 1)) for b in range(batch)]
    I = {k: np.concatenate([p[k] for p in per]) for k in per[0]}
    for a in I.values():
        a.setflags(write=False)
    return I


def per_image(I, b, c, hw, ng):
    return {k: (a[b * ng:(b + 1) * ng] if k in ("m", "v") else a[b * c * hw:(b + 1) * c * hw]) for k, a in I.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(BATCHED)), ids=lambda i: case_id(BATCHED[i]))
def test_batched_entries(dev, i):
    """bla_group_norm_relu_batched_f32 and bla_group_norm_ddx_gated_batched_f32 against the per-image reference: fold_groups (csrc/bla_group_norm.hip) folds
    the batch into the channel count, shortens the group to the image, or goes image by image -- the groups of one image never reach into the next."""
    batch, c, gs, hw = BATCHED[i]; I = batched_inputs(i)
    ng = (c + gs - 1) // gs; n = c * hw
    path = "batched, " + path_of(c, gs, hw)
    m, v, out = run_forward(dev, "bla_group_norm_relu_batched_f32", I["data"], c, gs, hw, 0, batch)
    dests = {(wg, wa): run_gradient(dev, "bla_group_norm_ddx_gated_batched_f32", I, c, gs, hw, 0, *gate_addend(I, wg, wa), batch=batch) for wg, wa in ((False, False), (True, True))}
    worst_f = {}
    for b in range(batch):
        J = per_image(I, b, c, hw, ng)
        f = forward_fractions(J["data"], m[b * ng:(b + 1) * ng], v[b * ng:(b + 1) * ng], out[b * n:(b + 1) * n], c, gs, hw, True)
        for (wg, wa), dest in dests.items():
            gate, addend = gate_addend(J, wg, wa)
            f["gradient"] = max(f.get("gradient", 0.0), gradient_fraction(dest[b * n:(b + 1) * n], J["source"], J["data"], J["m"], J["v"], c, gs, hw, gate, addend))
        worst_f = {q: max(worst_f.get(q, 0.0), f[q]) for q in f}
    for q, f in worst_f.items():
        record(path, q, f, BATCHED[i])


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", RESNET, ids=case_id)
def test_dropout_and_gated_forms_inside_a_resnet_block(dev, cfg):
    """group_norm_relu_dropout and the gated gradient with their real operands are internal; a ResNet block (Cin == Cout, so nothing is overwritten
    later in the pass) leaves all their inputs and outputs in caller-owned buffers, and each is checked there against the bounds:
    relu1 from x; (relu2, dp) from the device's own c1 and the drop mask; g_out_b from (g_out_a, c1, gate = dp); del_x from (g_in, x, gate = relu1,
    addend = del_out)."""
    import ctypes as C
    N = dev.native; L = dev.lib()
    batch, c, h, w, gs = cfg; hw = h * w; tdim = 16; ng = (c + gs - 1) // gs
    assert c % gs == 0      # the batch folds: batch * c channels in the same groups, statistics [B][groups]
    seed = 5800 + 10 * RESNET.index(cfg)
    u = lambda k, shape, lo, hi: uniform(seed + k, shape, lo, hi, F32)
    x, del_out = u(0, (batch, c, hw), -1, 3), u(7, (batch, c, hw), -1, 1)
    drop = (uniform(seed + 8, (batch, c, hw), 0, 1, F32) < 0.1).astype(np.uint8)
    P = dict(k1=u(2, (c, c, 3, 3), -0.2, 0.2), k2=u(3, (c, c, 3, 3), -0.1, 0.1), tw=u(4, (tdim, c), -0.1, 0.1), tb=u(5, (c,), -0.1, 0.1))
    D = {k: View(dev, a.shape, a) for k, a in dict(P, x=x, del_out=del_out, temb=u(1, (batch, tdim), 0, 1)).items()}
    D["drop"] = View(dev, drop.shape, drop, dtype=np.uint8)
    W = {k: View(dev, (batch, ng)) for k in ("mu1", "sd1", "mu2", "sd2")}
    W.update({k: View(dev, (batch, c, hw)) for k in ("relu1", "c1", "relu2", "dp", "c2", "res", "result", "g_out_a", "g_out_b", "g_in", "del_x")})
    W.update(tdense=View(dev, (batch, c)), dtb=View(dev, (batch, c)), flip=View(dev, (c * c * 9,)))
    G = {k: View(dev, a.shape) for k, a in P.items()}
    params = N.ResnetParams(D["k1"].ptr, D["k2"].ptr, D["tw"].ptr, D["tb"].ptr, None)
    ws = N.ResnetWs(*[W[k].ptr for k in ("mu1", "sd1", "relu1", "c1", "tdense", "mu2", "sd2", "relu2", "dp", "c2", "res")])
    grads = N.ResnetGrads(G["k1"].ptr, G["k2"].ptr, G["tw"].ptr, G["tb"].ptr, None)
    scratch = N.ResnetScratch(W["g_out_a"].ptr, W["g_out_b"].ptr, W["g_in"].ptr, W["flip"].ptr)
    N.check(L.bla_resnet_forward_batched_f32(None, batch, D["x"].ptr, D["temb"].ptr, C.byref(params), D["drop"].ptr, C.byref(ws), W["result"].ptr, h, w, c, c, 3, tdim, gs))
    N.check(L.bla_resnet_backward_batched_f32(None, batch, D["del_out"].ptr, D["x"].ptr, D["temb"].ptr, C.byref(params), C.byref(ws), C.byref(grads), C.byref(scratch),
                                              W["dtb"].ptr, W["del_x"].ptr, h, w, c, c, 3, tdim, gs))
    R = {k: W[k].numpy().ravel() for k in ("mu1", "sd1", "mu2", "sd2", "relu1", "c1", "relu2", "dp", "g_out_a", "g_out_b", "g_in", "del_x")}
    assert np.array_equal(D["x"].numpy(), x) and np.array_equal(D["del_out"].numpy(), del_out) and np.array_equal(D["drop"].numpy(), drop)
    ch = batch * c
    path = ("resnet block" if batch > 1 else "single-image resnet block") + ", " + path_of(ch, gs, hw)
    for q, f in forward_fractions(x, R["mu1"], R["sd1"], R["relu1"], ch, gs, hw, True).items():
        record(path, q, f, (cfg, "relu1"))
    for q, f in forward_fractions(R["c1"], R["mu2"], R["sd2"], R["relu2"], ch, gs, hw, True).items():
        record(path, q, f, (cfg, "relu2"))
    assert np.array_equal(R["dp"].view(np.uint32), np.where(drop.ravel() != 0, F32(0), R["relu2"]).view(np.uint32)), (cfg, "dp")
    assert 0.05 < drop.mean() < 0.15 and (R["dp"] > 0).any()
    record(path, "gradient", gradient_fraction(R["g_out_b"], R["g_out_a"], R["c1"], R["mu2"], R["sd2"], ch, gs, hw, gate=R["dp"]), (cfg, "g_out_b"))
    record(path, "gradient", gradient_fraction(R["del_x"], R["g_in"], x, R["mu1"], R["sd1"], ch, gs, hw, gate=R["relu1"], addend=del_out), (cfg, "del_x"))
