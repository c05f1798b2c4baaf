"""nabwa_bam_sort* on the GPU (csrc/bam_sort.hip) and its Python face (bam_sort, BamSort): the records of tests/bam_sort_cases.py against the
NumPy oracle -- np.argsort(keys, kind="stable") over the records of the unsorted bytes, compared record for record as bytes -- with the
offsets and the keys of the output, the handle against the one-shot call, and the two errors the tests of the host checks leave: ECAP
without a write, EDATA naming the lowest record whose block_size is off.  (A device that is not there: tests/test_bam_sort_emu.py, through
the tool, in a process of its own.)"""
import ctypes as C
import importlib
import struct

import numpy as np
import pytest

import bam_sort_cases as S
import bamlib as B
import nabwa_testlib as T

nabwa = importlib.import_module("network-aware-bwa_amd")
pytestmark = pytest.mark.gpu


def check(recs, what, sorter=None, walk=False):
    data, off = S.join(recs)
    want, want_off, want_keys = S.oracle(data, off)
    f = sorter.sort if sorter is not None else nabwa.bam_sort
    got, got_off, got_keys = f(data.tobytes(), None if walk else off)
    S.assert_same_records(got, got_off, want, want_off, what)
    assert got_keys.tolist() == want_keys.tolist(), what
    assert all(got_keys[j] <= got_keys[j + 1] for j in range(0, len(got_keys) - 1, max(1, len(got_keys) // 1000))), what
    return got


@pytest.mark.parametrize("n", S.N_RECS)
def test_record_counts(n):
    check(S.mixed(n, seed=n + 1), "n_rec %d" % n)


def test_a_leading_record_shifts_the_rest_through_every_source_alignment():
    with nabwa.BamSort() as s:
        for lead in range(36, 52):
            check(S.with_lead(S.mixed(300, seed=lead), lead), "lead %d" % lead, sorter=s)


@pytest.mark.parametrize("k", range(len(S.named_cases())))
def test_named_cases(k):
    name, recs = S.named_cases()[k]
    check(recs, name)
    check(recs, name + ", offsets walked from the block_size words", walk=True)


def test_offsets_that_do_not_start_at_zero():
    recs = S.mixed(100, seed=31)
    data, off = S.join(recs)
    want, want_off, _ = S.oracle(data[off[7]:], off[7:] - off[7])
    got, got_off, _ = nabwa.bam_sort(data.tobytes(), off[7:])
    S.assert_same_records(got, got_off, want, want_off)


def test_a_handle_used_for_large_small_large_gives_the_one_shot_bytes():
    large, small, large2 = S.mixed(20000, seed=41), S.mixed(3, seed=42), S.mixed(25000, seed=43)
    with nabwa.BamSort() as s:
        for recs in (large, small, large2, small):
            data, off = S.join(recs)
            assert check(recs, "handle", sorter=s) == nabwa.bam_sort(data.tobytes(), off)[0]
        assert len(s.times()) == 6 and all(t >= 0 for t in s.times())


def test_cap_one_byte_short_is_ecap_and_writes_nothing():
    data, off = S.join(S.mixed(500, seed=51))
    total = len(data)
    with pytest.raises(nabwa.NabwaError) as e:
        nabwa.bam_sort(data.tobytes(), off, cap=total - 1)
    assert e.value.code == nabwa.ECAP and e.value.needed == total
    guard = 64
    buf = np.full(total + 2 * guard, 0xa5, np.uint8)
    out_off, keys = np.zeros(len(off), np.int64), np.zeros(len(off) - 1, np.uint64)
    L = nabwa.lib()
    rc = L.nabwa_bam_sort(0, len(off) - 1, T.ptr(data), T.ptr(off), buf.ctypes.data + guard, total - 1, T.ptr(out_off), T.ptr(keys))
    assert rc == nabwa.ECAP and str(total).encode() in L.nabwa_last_error()
    assert (buf == 0xa5).all()
    # with exactly the total the records fill the buffer and the guard bytes on both sides stay
    rc = L.nabwa_bam_sort(0, len(off) - 1, T.ptr(data), T.ptr(off), buf.ctypes.data + guard, total, T.ptr(out_off), T.ptr(keys))
    assert rc == nabwa.OK
    assert (buf[:guard] == 0xa5).all() and (buf[guard + total:] == 0xa5).all()
    assert buf[guard:guard + total].tobytes() == S.oracle(data, off)[0]


def test_a_block_size_off_by_one_is_edata_naming_the_lowest_record():
    recs = S.mixed(1000, seed=61)
    data, off = S.join(recs)
    data = data.copy()
    for k, delta, lowest in ((700, 1, 700), (123, -1, 123), (999, 1, 123)):
        data[off[k]:off[k] + 4] = np.frombuffer(struct.pack("<I", len(recs[k]) - 4 + delta), np.uint8)
        with pytest.raises(nabwa.NabwaError) as e:
            nabwa.bam_sort(data.tobytes(), off)
        assert e.value.code == nabwa.EDATA and "record %d:" % lowest in str(e.value), str(e.value)


def test_a_block_size_off_by_one_in_the_middle_record_of_three():
    """the whole message, and the handle as it was: the sound records sorted as by a fresh handle"""
    recs = S.mixed(3, seed=62)
    bad, text = B.head_damaged(recs[1], "block_size", 1)
    data, off = S.join(recs)
    with nabwa.BamSort() as s:
        with pytest.raises(nabwa.NabwaError) as e:
            s.sort(S.join([recs[0], bad, recs[2]])[0].tobytes(), off)
        assert e.value.code == nabwa.EDATA and str(e.value) == "libnabwa error %d: %s" % (nabwa.EDATA, text)
        got = s.sort(data.tobytes(), off)
    with nabwa.BamSort() as fresh:
        want = fresh.sort(data.tobytes(), off)
    assert len(got) == len(want) and all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(got, want))
