"""The CPU oracle's aln_global_core (orc_global, oracle/nabwa_oracle.c) against the reference's own (ref_global), on fresh tasks
of every kind dpgen makes, under every global parameter block -- the asymmetric matrices included.  orc_global is the answer key
of test_gpu_se.py::test_global_align_random_vs_oracle, so it must itself be the reference's."""
import ctypes as C

import numpy as np
import pytest

import dpgen
import nabwa_testlib as T

REF = dpgen.load_ref()
pytestmark = pytest.mark.skipif(REF is None, reason="compiled reference (oracle/_ref/libbwaref.so) not built")


@pytest.fixture(scope="module")
def olib():
    return T.load_oracle()


@pytest.mark.parametrize("block", dpgen.GLOBAL_BLOCKS, ids=dpgen.block_id)
def test_orc_global_matches_ref_global(olib, block):
    go, ge, gend, mname, band = block
    mat = dpgen.matrix(REF, mname)
    rng = np.random.default_rng(1000 + dpgen.GLOBAL_BLOCKS.index(block))
    tasks = dpgen.global_tasks(rng, 450, band) + dpgen.edge_tasks(rng)
    want = REF.global_many(tasks, go, ge, gend, mat, band)
    for (kind, r, q), (ws, wc) in zip(tasks, want):
        r, q = np.ascontiguousarray(r), np.ascontiguousarray(q)
        cig = np.zeros(len(r) + len(q) + 2, np.uint32)
        ncig = C.c_int(0)
        sc = olib.orc_global(T.ptr(r), len(r), T.ptr(q), len(q), go, ge, gend, T.ptr(mat), 5, band, T.ptr(cig), C.byref(ncig))
        assert (sc, list(cig[:ncig.value])) == (ws, list(wc)), (kind, len(r), len(q))
