"""Host-side I/O units of the drop-in layer (csv, mnist_csv2, cifar10, bmp): same bytes / same values / same rand()
consumption as the reference's units, plus fixture-free known answers (data/a.csv values).  Each case is one
procedure run on a library of these units; what the reference's own units produced in it is recorded in tests/golden/host_io.npz
(oracle/gen_golden.py), and where the reference's sources exist the case also runs on them, compiled into a scratch .so."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, golden

LIB = os.path.join(ROOT, "big-linear-algebra_amd", "lib")
REF = "/root/reference"
libc = C.CDLL(None)


def reference_io_lib(tmp):
    """The reference's csv / mnist_csv2 / cifar10 / bmp units compiled as they are into a scratch .so (where its sources exist)."""
    so = str(tmp / "librefio.so")
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-w", "-fPIC", "-shared", "-o", so] +
                          [os.path.join(REF, "lib", f) for f in ("csv.c", "mnist_csv2.c", "cifar10.c", "bmp.c")] + ["-lm"])
    L = C.CDLL(so)
    L.read_csv_contents.restype = C.POINTER(C.c_float)
    return L


def check_case(name, mine, theirs_fn):
    """`mine` (a dict of arrays from one case on our units) against the reference's recorded result of the same case, and against
    the reference's units themselves where their sources exist (theirs_fn builds them and runs the case)."""
    rec = golden("host_io")
    want = {k[len(name) + 1:]: rec[k] for k in rec.z.files if k.startswith(name + ":")}
    assert sorted(mine) == sorted(want), (name, sorted(mine), sorted(want))
    for k in want:
        assert np.array_equal(mine[k], want[k]), f"{name}:{k} differs from the reference's recorded result"
    if os.path.isdir(REF):
        theirs = theirs_fn()
        for k in want:
            assert np.array_equal(theirs[k], want[k]), f"{name}:{k}: tests/golden/host_io.npz differs from the reference's units"


@pytest.fixture(scope="module")
def ours(pkg):
    pkg.build_native()
    L = C.CDLL(os.path.join(LIB, "libbla_host.so"))
    L.read_csv_contents.restype = C.POINTER(C.c_float)
    return L


def test_csv_roundtrip_and_known_answer(ours, tmp_path):
    p = str(tmp_path / "a.csv")
    open(p, "w").write("1,2.3,3,\n4,509,6,\n7,8,9.0,")          # data/a.csv layout: every value comma-terminated
    v = np.ctypeslib.as_array(ours.read_csv_contents(p.encode()), shape=(9,)).copy()
    assert np.allclose(v, [1, 2.3, 3, 4, 509, 6, 7, 8, 9])
    d = np.array([1, 2.3, 4.567, 0, 0, 0], np.float32)
    q = str(tmp_path / "b.csv")
    ours.write_csv_contents(q.encode(), d.ctypes.data_as(C.POINTER(C.c_float)), 3, 2)      # main.c:49-50
    assert open(q).read() == "1.000000,2.300000,4.567000,\n0.000000,0.000000,0.000000,\n"   # data/b.csv
    f = libc.fopen; f.restype = C.c_void_p
    fh = f(q.encode(), b"r")
    ours.count_num_lines.argtypes = [C.c_void_p]
    assert ours.count_num_lines(fh) == 2


def csv_case(L, tmp):
    rng = np.random.default_rng(0)
    d = (rng.normal(size=37 * 5) * 100).astype(np.float32)
    a = str(tmp / "csv_case.csv")
    L.write_csv_contents(a.encode(), d.ctypes.data_as(C.POINTER(C.c_float)), 5, 37)
    return {"bytes": np.frombuffer(open(a, "rb").read(), np.uint8),
            "read": np.ctypeslib.as_array(L.read_csv_contents(a.encode()), shape=(185,)).copy()}


def test_csv_matches_reference(ours, tmp_path):
    check_case("csv", csv_case(ours, tmp_path), lambda: csv_case(reference_io_lib(tmp_path), tmp_path))


class MnistCSV(C.Structure):
    _fields_ = [("file", C.c_void_p), ("X", C.POINTER(C.c_float)), ("y", C.POINTER(C.c_float)), ("num_examples", C.c_int),
                ("num_sampled", C.c_int), ("sampled", C.c_char_p)]


class MnistExample(C.Structure):
    _fields_ = [("X", C.POINTER(C.c_float)), ("y", C.c_float), ("num_examples", C.c_int)]


def mnist_case(L, tmp):
    rng = np.random.default_rng(1)
    n = 23
    rows = np.concatenate([rng.integers(0, 10, (n, 1)), rng.integers(0, 256, (n, 784))], 1)
    p = str(tmp / "mnist.csv")
    open(p, "w").write("".join(",".join(str(v) for v in r) + ",\n" for r in rows))
    fopen = libc.fopen; fopen.restype = C.c_void_p
    L.get_random_data_take.restype = MnistExample; L.get_random_data_take.argtypes = [C.POINTER(MnistCSV)]
    L.get_random_data_replace.restype = MnistExample; L.get_random_data_replace.argtypes = [C.POINTER(MnistCSV)]
    m = MnistCSV(fopen(p.encode(), b"r"), None, None, 0, 0, None)
    L.mnist_csv_init(C.byref(m))
    X = np.ctypeslib.as_array(m.X, shape=(784, n)).copy(); y = np.ctypeslib.as_array(m.y, shape=(n,)).copy()
    libc.srand(42)                                     # model/mnist_nn.c:513
    base = C.cast(m.X, C.c_void_p).value
    picks = []
    for _ in range(2 * n + 3):                         # runs past exhaustion: the sampler restarts (lib/mnist_csv2.c:43-46)
        ex = L.get_random_data_take(C.byref(m)); picks.append(((C.cast(ex.X, C.c_void_p).value - base) // 4, ex.y))
    for _ in range(5):
        ex = L.get_random_data_replace(C.byref(m)); picks.append(((C.cast(ex.X, C.c_void_p).value - base) // 4, ex.y))
    return {"X": X, "y": y, "picks": np.array(picks, np.float64), "rows": rows}


def test_mnist_store_and_samplers_match_reference(ours, tmp_path):
    mine = mnist_case(ours, tmp_path)
    assert np.array_equal(mine["X"], mine["rows"][:, 1:].T.astype(np.float32))     # feature-major store
    check_case("mnist", mine, lambda: mnist_case(reference_io_lib(tmp_path), tmp_path))
    # NB the reference's "without replacement" walk stops AT the n-th unsampled slot's successor without checking that
    # slot (lib/mnist_csv2.c:53-58), so repeats are possible; reproduced as is (the picks above are identical).


class BMPData(C.Structure):
    _fields_ = [("width", C.c_uint), ("height", C.c_uint), ("red", C.POINTER(C.c_uint8)), ("green", C.POINTER(C.c_uint8)),
                ("blue", C.POINTER(C.c_uint8))]


def bmp_cifar_case(L, tmp):
    rng = np.random.default_rng(2)
    batch = str(tmp / "data_batch_1.bin")
    rng.integers(0, 256, 3073 * 10000, dtype=np.uint8).tofile(batch)       # a full-size batch file (30,730,000 bytes)
    fd = os.open(batch, os.O_RDONLY)
    libc.srand(7)
    arr = np.zeros(3072, np.uint8)
    for _ in range(3):
        L.fill_random_data(fd, arr.ctypes.data_as(C.POINTER(C.c_uint8)))
    os.close(fd)
    out = {"image": arr.copy()}
    for w, h in [(32, 32), (5, 3)]:
        planes = [rng.integers(0, 256, w * h, dtype=np.uint8) for _ in range(3)]
        d = BMPData(w, h, *[p.ctypes.data_as(C.POINTER(C.c_uint8)) for p in planes])
        f = str(tmp / f"img_{w}.bmp"); L.write_bmp_data(f.encode(), C.byref(d))
        b = np.frombuffer(open(f, "rb").read(), np.uint8).copy()
        # byte 47 (info header [33]) is never written by the reference (lib/bmp.c:70-72 assigns [32] twice): stack garbage there
        b[47] = 0
        out[f"bmp_{w}x{h}"] = b
    return out


def test_bmp_and_cifar_match_reference(ours, tmp_path):
    mine = bmp_cifar_case(ours, tmp_path)
    for w, h in [(32, 32), (5, 3)]:
        f = mine[f"bmp_{w}x{h}"].tobytes()
        assert f[:2] == b"BM" and len(f) == 54 + ((24 * w + 31) // 32) * 4 * h
    check_case("bmp_cifar", mine, lambda: bmp_cifar_case(reference_io_lib(tmp_path), tmp_path))


def _legacy_reader(path_c, tmp):
    """lib/mnist_csv.c is a per-program unit (it clashes with mnist_csv2.c by the reference's design): build it alone."""
    so = str(tmp / (os.path.basename(os.path.dirname(os.path.dirname(path_c))) + "_legacy.so"))
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-w", "-fPIC", "-shared", "-o", so, path_c])
    L = C.CDLL(so)
    return L


class LegacyCSV(C.Structure):
    _fields_ = [("file", C.c_void_p), ("buffer", C.POINTER(C.c_float)), ("num_lines", C.c_int)]


def _legacy_rows(L, path, rows, tmp, tag):
    """get_next_data x rows (+ one call past the end), visualize_digit_data of the last row; returns (values, return codes, stdout)."""
    fopen = libc.fopen; fopen.restype = C.c_void_p
    libc.fclose.argtypes = [C.c_void_p]; libc.fflush.argtypes = [C.c_void_p]; libc.fgetc.argtypes = [C.c_void_p]
    buf = np.zeros(785, np.float32)
    csv = LegacyCSV(fopen(path.encode(), b"r"), buf.ctypes.data_as(C.POINTER(C.c_float)), rows)
    L.get_next_data.argtypes = [C.POINTER(LegacyCSV)]; L.visualize_digit_data.argtypes = [C.POINTER(LegacyCSV)]
    out_path = str(tmp / f"{tag}.txt")
    libc.fflush(None)
    saved = os.dup(1); fd = os.open(out_path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC); os.dup2(fd, 1)
    vals, rcs = [], []
    try:
        for _ in range(rows):
            rcs.append(L.get_next_data(C.byref(csv))); vals.append(buf.copy())
        buf[1:] /= 255.0                                  # callers normalise before drawing (model/mnist_hinge.c)
        L.visualize_digit_data(C.byref(csv))
        libc.fgetc(csv.file)                              # the reference tests feof(), which needs a read past the end first
        rcs.append(L.get_next_data(C.byref(csv)))
        libc.fflush(None)
    finally:
        os.dup2(saved, 1); os.close(saved); os.close(fd)
    libc.fclose(csv.file)
    return np.array(vals), rcs, open(out_path, "rb").read()


def legacy_case(L, tmp):
    rng = np.random.default_rng(3)
    rows = 4
    path = str(tmp / "mnist.csv")
    with open(path, "w") as f:
        for r in range(rows):
            f.write(",".join(str(int(v)) for v in [rng.integers(10)] + list(rng.integers(0, 256, 784))) + ("\n" if r % 2 else ",\n"))
    vals, rcs, out = _legacy_rows(L, path, rows, tmp, "legacy")
    return {"values": vals, "rcs": np.array(rcs, np.int64), "stdout": np.frombuffer(out, np.uint8)}


def test_legacy_streaming_reader_matches_reference(tmp_path):
    """lib/mnist_csv.c (get_next_data, visualize_digit_data): same values, same return codes, same stdout as the reference's unit
    on a synthetic MNIST-shaped file (label + 784 pixels per row, comma-terminated values, newline-terminated rows)."""
    mine = legacy_case(_legacy_reader(os.path.join(LIB, "mnist_csv.c"), tmp_path), tmp_path)
    out = mine["stdout"].tobytes()
    assert list(mine["rcs"]) == [0] * 4 + [1] and b"CSV file is empty" in out and out.count(b"\n") >= 31
    check_case("legacy", mine, lambda: legacy_case(_legacy_reader(os.path.join(REF, "lib", "mnist_csv.c"), tmp_path), tmp_path))
