"""The decode kernel of the colour-space chains at its own seam: nabwa_cs2nt against the reference's cs2nt_DP + cs2nt_nt_qual
(cs2nt.c:36-109), every output byte equal --
 * on the committed cases with the reference's answers (tests/golden/make_golden_cs.py): the "delicate example" of cs2nt.c:8-21 at
   q(O) = 25 and 26, sizes from 1 to the cap, nt_ref with 4s at the start, inside and throughout, N colours (quality 63), qualities on
   both sides of COLOR_MM = 19 and NUCL_MM = 25, all-equal penalties (ties: the first minimum wins);
 * on a few thousand fresh cases against oracle/_ref/libbwaref.so, when it travelled."""
import importlib
import os

import numpy as np
import pytest

import csgen
import nabwa_testlib as T

pytestmark = pytest.mark.gpu
nabwa = importlib.import_module("network-aware-bwa_amd")
REF = csgen.load_ref_lib()
need_ref = pytest.mark.skipif(REF is None, reason="compiled reference (oracle/_ref/libbwaref.so) did not travel")


def assert_same(off, got, want):
    assert got.shape == want.shape
    if (got != want).any():
        bad = [i for i in range(len(off) - 1) if (got[off[i] - i:off[i + 1] - i - 1] != want[off[i] - i:off[i + 1] - i - 1]).any()]
        i = bad[0]
        pytest.fail("%d of %d cases differ; case %d (size %d): got %s want %s" % (
            len(bad), len(off) - 1, i, off[i + 1] - off[i], got[off[i] - i:off[i + 1] - i - 1][:40], want[off[i] - i:off[i + 1] - i - 1][:40]))


def test_committed_cases_equal_the_reference():
    v = np.load(os.path.join(T.GOLDEN, "vectors_cs2nt.npz"))
    off, ref, cs, want = v["off"], v["nt_ref"], v["cs_read"], v["out"]
    sizes = np.diff(off)
    assert sizes.min() == 1 and sizes.max() == nabwa.CS2NT_MAX == csgen.CS2NT_MAX
    assert (cs & 63 == 63).any() and (ref == 4).any()
    # the delicate example, cases 0 and 1: q(O) = 25 keeps the reference's base (two colour changes), 26 takes the base change
    assert [int(x) >> 6 for x in want[0:4]] != [int(x) >> 6 for x in want[4:8]]
    assert_same(off, nabwa.cs2nt(off, ref, cs), want)


def test_size_one_and_bad_sizes():
    off = np.array([0, 1, 2], np.int64)
    out = nabwa.cs2nt(off, np.array([0, 1, 4, 4], np.uint8), np.array([1 << 6 | 30, 63], np.uint8))
    assert out.size == 0
    with pytest.raises(nabwa.NabwaError):
        nabwa.cs2nt(np.array([0, 0], np.int64), np.array([0], np.uint8), np.zeros(0, np.uint8))
    big = nabwa.CS2NT_MAX + 1
    with pytest.raises(nabwa.NabwaError):
        nabwa.cs2nt(np.array([0, big], np.int64), np.zeros(big + 1, np.uint8), np.zeros(big, np.uint8))


@need_ref
def test_fresh_cases_equal_the_compiled_reference():
    rng = np.random.default_rng(99)
    off, ref, cs = csgen.cases(rng, 4000)
    assert_same(off, nabwa.cs2nt(off, ref, cs), csgen.reference_decode(REF, off, ref, cs))
    # every size from 1 to 130, and the cap, in one batch of mixed lengths
    sizes = list(range(1, 131)) + [nabwa.CS2NT_MAX] * 3
    off, ref, cs = csgen.cases(rng, 10 * len(sizes), sizes=sizes)
    assert_same(off, nabwa.cs2nt(off, ref, cs), csgen.reference_decode(REF, off, ref, cs))


@need_ref
def test_delicate_example_threshold():
    for q_o in (24, 25, 26, 27):
        off, ref, cs = csgen.pack([csgen.delicate(q_o)])
        got = nabwa.cs2nt(off, ref, cs)
        assert_same(off, got, csgen.reference_decode(REF, off, ref, cs))
        assert "".join("ACGT"[int(x) >> 6] for x in got) == ("TTAA" if q_o <= 25 else "TTGA"), q_o
