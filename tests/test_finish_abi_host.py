"""nabwa_refine_gapped_core / nabwa_cal_md / nabwa_finish_counts without a GPU: the symbols, the argument checks that need no device,
NABWA_ENODEV where there is none (no CPU fallback), and the tools' refusal of a NABWA_FINISH they do not know."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import nabwa_testlib as T

nabwa = importlib.import_module("network-aware-bwa_amd")
PKG = os.path.join(T.ROOT, "network-aware-bwa_amd")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(nabwa.LIB_PATH):
        nabwa.build()
    return nabwa.lib()


def _args(n=2, length=20):
    off = np.arange(n + 1, dtype=np.int64) * length
    qry = np.zeros(n * length, np.uint8)
    ext = np.ones(n, np.int32)
    pos = np.full(n, 1000, np.uint32)
    ncig = np.zeros(n, np.int32)
    cig = np.zeros((n, 8), np.uint16)
    return off, qry, ext, pos, ncig, cig


def test_library_exports_the_three_symbols(L):
    for name in ("nabwa_refine_gapped_core", "nabwa_cal_md", "nabwa_finish_counts"):
        assert hasattr(L, name), name
    assert len(nabwa.finish_counts()) == 4


def test_header_declares_them():
    h = open(os.path.join(T.ROOT, "include", "nabwa.h")).read()
    for name in ("int nabwa_refine_gapped_core(", "int nabwa_cal_md(", "void nabwa_finish_counts(uint64_t out[4]);"):
        assert name in h


def test_null_and_out_of_range_arguments_are_einval(L):
    fake = C.create_string_buffer(4096)            # stands in for an index: the checks below come before anything reads it
    ix = C.cast(fake, C.c_void_p)
    off, qry, ext, pos, ncig, cig = _args()
    P = T.ptr
    rg = L.nabwa_refine_gapped_core
    assert rg(None, 0, 1, 2, P(off), P(qry), P(ext), P(pos), P(ncig), P(cig), 8) == nabwa.EINVAL
    assert rg(ix, 0, 1, 2, None, P(qry), P(ext), P(pos), P(ncig), P(cig), 8) == nabwa.EINVAL
    assert rg(ix, 0, 1, 2, P(off), None, P(ext), P(pos), P(ncig), P(cig), 8) == nabwa.EINVAL
    assert rg(ix, 0, 1, 2, P(off), P(qry), None, P(pos), P(ncig), P(cig), 8) == nabwa.EINVAL
    assert rg(ix, 0, 1, 2, P(off), P(qry), P(ext), None, P(ncig), P(cig), 8) == nabwa.EINVAL
    assert rg(ix, 0, 1, 2, P(off), P(qry), P(ext), P(pos), None, P(cig), 8) == nabwa.EINVAL
    assert rg(ix, 0, 1, 2, P(off), P(qry), P(ext), P(pos), P(ncig), None, 8) == nabwa.EINVAL
    assert rg(ix, 2, 1, 2, P(off), P(qry), P(ext), P(pos), P(ncig), P(cig), 8) == nabwa.EINVAL          # which_ref
    assert rg(ix, 0, 1, -1, P(off), P(qry), P(ext), P(pos), P(ncig), P(cig), 8) == nabwa.EINVAL         # n
    assert rg(ix, 0, 1, 2, P(off), P(qry), P(ext), P(pos), P(ncig), P(cig), 0) == nabwa.EINVAL          # max_cigar
    empty = np.array([0, 0, 20], np.int64)                                                             # a query of length 0
    assert rg(ix, 0, 1, 2, P(empty), P(qry), P(ext), P(pos), P(ncig), P(cig), 8) == nabwa.EINVAL
    long_off = np.array([0, 0x4000], np.int64)                                                         # ... of 0x4000
    long_q = np.zeros(0x4000, np.uint8)
    assert rg(ix, 0, 1, 1, P(long_off), P(long_q), P(ext), P(pos), P(ncig), P(cig), 8) == nabwa.EINVAL
    bad_q = qry.copy()
    bad_q[3] = 5
    assert rg(ix, 0, 1, 2, P(off), P(bad_q), P(ext), P(pos), P(ncig), P(cig), 8) == nabwa.EINVAL
    md = L.nabwa_cal_md
    nm = np.zeros(2, np.int32)
    mo = np.zeros(3, np.int64)
    buf = np.zeros(256, np.uint8)
    assert md(None, 0, 2, P(off), P(qry), P(pos), P(ncig), P(cig), 8, P(nm), P(mo), P(buf), 256) == nabwa.EINVAL
    assert md(ix, 0, 2, P(off), P(qry), P(pos), P(ncig), P(cig), 8, P(nm), None, P(buf), 256) == nabwa.EINVAL
    assert md(ix, 0, 2, P(off), P(qry), P(pos), None, P(cig), 8, P(nm), P(mo), P(buf), 256) == nabwa.EINVAL
    assert md(ix, 0, 2, P(off), P(qry), P(pos), P(ncig), P(cig), 8, P(nm), P(mo), None, 256) == nabwa.EINVAL
    assert md(ix, 3, 2, P(off), P(qry), P(pos), P(ncig), P(cig), 8, P(nm), P(mo), P(buf), 256) == nabwa.EINVAL
    assert md(ix, 0, 2, P(empty), P(qry), P(pos), P(ncig), P(cig), 8, P(nm), P(mo), P(buf), 256) == nabwa.EINVAL
    nine = np.array([9, 0], np.int32)                                                                  # n_cigar above max_cigar
    assert md(ix, 0, 2, P(off), P(qry), P(pos), P(nine), P(cig), 8, P(nm), P(mo), P(buf), 256) == nabwa.EINVAL
    one = np.array([1, 0], np.int32)                                                                   # a CIGAR that does not consume its query
    short = cig.copy()
    short[0, 0] = 19
    assert md(ix, 0, 2, P(off), P(qry), P(pos), P(one), P(short), 8, P(nm), P(mo), P(buf), 256) == nabwa.EINVAL
    assert b"CIGAR" in L.nabwa_last_error()


def test_no_cpu_fallback_without_gpu(L):
    if L.nabwa_device_count() > 0:
        pytest.skip("a GPU is present")
    fake = C.create_string_buffer(4096)
    ix = C.cast(fake, C.c_void_p)
    off, qry, ext, pos, ncig, cig = _args()
    P = T.ptr
    assert L.nabwa_refine_gapped_core(ix, 0, 1, 2, P(off), P(qry), P(ext), P(pos), P(ncig), P(cig), 8) == nabwa.ENODEV
    nm = np.zeros(2, np.int32)
    mo = np.zeros(3, np.int64)
    buf = np.zeros(256, np.uint8)
    assert L.nabwa_cal_md(ix, 0, 2, P(off), P(qry), P(pos), P(ncig), P(cig), 8, P(nm), P(mo), P(buf), 256) == nabwa.ENODEV
    assert nabwa.finish_counts() == [0, 0, 0, 0]


@pytest.mark.parametrize("tool,args", [
    ("nabwa_bam2bam", ["-g", "no_such_prefix", "no_such.bam"]),
    ("nabwa_samse", ["no_such_prefix", "no_such.sai", "no_such.fq"]),
    ("nabwa_sampe", ["no_such_prefix", "no_such_1.sai", "no_such_2.sai", "no_such_1.fq", "no_such_2.fq"]),
])
def test_tools_refuse_an_unknown_nabwa_finish(L, tool, args):
    exe = os.path.join(PKG, tool)
    if not os.path.exists(exe):
        nabwa.build()
    env = dict(os.environ, NABWA_FINISH="cpu")
    r = subprocess.run([exe] + args, capture_output=True, text=True, env=env)
    assert r.returncode == 1 and "NABWA_FINISH=cpu: host or gpu" in r.stderr, r.stderr
    # a value it knows gets past that check: the missing input is what it reports
    r = subprocess.run([exe] + args, capture_output=True, text=True, env=dict(os.environ, NABWA_FINISH="gpu"))
    assert "NABWA_FINISH" not in r.stderr
