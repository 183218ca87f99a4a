"""bla_conv_bf16_prepare_kernels_table (include/bla.h): every bf16 kernel matrix of a pass in one launch.  One chunk body stands behind this
kernel and bla_conv_bf16_prepare_kernels', so every destination must equal that entry's on the same job bit for bit -- the forward and the flipped
data-gradient form, inner extents that are no multiple of 8 (padding columns +0), k = 1, jobs far smaller than the one that sizes the grid (whole
workgroups past a job's extent), rows that straddle workgroups.  Every destination sits between 0xFFFF guards."""
import ctypes as C

import numpy as np
import pytest

from inputs import uniform

pytestmark = pytest.mark.gpu

#        f    c  k  dgrad
JOBS = [(3, 5, 3, 0), (5, 3, 3, 1), (16, 8, 1, 0), (40, 24, 3, 0), (40, 24, 3, 1), (130, 72, 3, 1)]      # the last one sizes the grid
GUARD = 64      # uint16 elements on either side: 128 bytes, so the matrix stays 16-byte aligned
BLA_ERR_INVALID = 1


def elements(pkg, job):
    f, c, k, dg = job
    return pkg.conv_bf16_prep_chunks(f, c, k, dg) * 8


def guarded(pkg, job):
    return pkg.DeviceArray((elements(pkg, job) + 2 * GUARD,), np.uint16).fill_bytes(0xFF)


def kernels(pkg, job, seed):
    f, c, k, _ = job
    return pkg.to_device(uniform(seed, (f, c, k, k), -2, 2, np.float32))


def single(pkg, job, kern):
    """bla_conv_bf16_prepare_kernels on the same job, between the same guards"""
    f, c, k, dg = job
    d = guarded(pkg, job)
    pkg.conv_bf16_prepare_kernels(kern, d.ptr + 2 * GUARD, f, c, k, bool(dg))
    pkg.sync()
    return d.numpy()


def check_guards(a, what):
    assert (a[:GUARD] == 0xFFFF).all() and (a[-GUARD:] == 0xFFFF).all(), what


@pytest.mark.parametrize("jobs", [JOBS, JOBS[3:4], JOBS[1:2]], ids=["mixed", "one_forward", "one_data_gradient"])
def test_table_launch_writes_what_the_single_launches_write(pkg, jobs):
    pkg.init(0)
    kerns = [kernels(pkg, j, 8800 + i) for i, j in enumerate(jobs)]
    dsts = [guarded(pkg, j) for j in jobs]
    table = pkg.conv_bf16_prepare_kernels_table([(kn, d.ptr + 2 * GUARD, f, c, k, dg) for kn, d, (f, c, k, dg) in zip(kerns, dsts, jobs)])
    pkg.sync()
    assert table.nbytes == 32 * len(jobs)      # sizeof(bla_conv_bf16_prep_job)
    for job, kn, d in zip(jobs, kerns, dsts):
        got, want = d.numpy(), single(pkg, job, kn)
        check_guards(got, job); check_guards(want, job)
        body = want[GUARD:-GUARD]
        assert (body != 0xFFFF).all() and np.count_nonzero(body) > body.size // 4, job      # every element written (no bf16 of a value in [-2, 2] is 0xFFFF)
        assert np.array_equal(got, want), (job, int(np.count_nonzero(got != want)))


def test_no_jobs_and_the_refusals_leave_the_outputs_alone(pkg):
    pkg.init(0)
    L = pkg.lib()
    job = JOBS[3]
    kern, d = kernels(pkg, job, 8900), guarded(pkg, job)
    arr = (pkg.native.ConvBf16PrepJob * 1)(pkg.native.ConvBf16PrepJob(kern.ptr, d.ptr + 2 * GUARD, job[0], job[1], job[2], job[3]))
    table = pkg.DeviceArray((C.sizeof(arr),), np.uint8)
    pkg.native.check(L.bla_memcpy_h2d(table.ptr, C.addressof(arr), C.sizeof(arr), None)); pkg.sync()
    chunks = pkg.conv_bf16_prep_chunks(*job)
    assert L.bla_conv_bf16_prepare_kernels_table(None, table.ptr, 0, chunks) == 0           # n_jobs == 0: nothing, BLA_OK
    assert L.bla_conv_bf16_prepare_kernels_table(None, None, 0, 0) == 0
    assert pkg.conv_bf16_prepare_kernels_table([]) is not None
    assert L.bla_conv_bf16_prepare_kernels_table(None, None, 1, chunks) == BLA_ERR_INVALID      # NULL table
    assert L.bla_conv_bf16_prepare_kernels_table(None, table.ptr, -1, chunks) == BLA_ERR_INVALID
    assert L.bla_conv_bf16_prepare_kernels_table(None, table.ptr, 1, 0) == BLA_ERR_INVALID      # max_chunks == 0
    pkg.sync()
    assert (d.numpy() == 0xFFFF).all()
    pkg.native.check(L.bla_conv_bf16_prepare_kernels_table(None, table.ptr, 1, chunks)); pkg.sync()   # the same table is sound
    assert np.array_equal(d.numpy(), single(pkg, job, kern))
