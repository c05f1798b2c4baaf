"""nabwa_bai_* on the GPU (csrc/nabwa_bai.hip, bai_kernels.hip) and its Python face (nabwa.Bai, nabwa.bai) against the Python oracle of
tests/bai_cases.py, byte for byte: the case lists tests/test_bai_emu.py runs through the bodies on the CPU, here through the kernels; calls
split in any way, with gaps; finish twice; clear; the size-only finish and a buffer too small; damaged and misplaced records; block tables
that are refused; and a file larger than a workgroup's share, read back through its index."""
import ctypes as C
import importlib

import numpy as np
import pytest

import bai_cases as M
import bamlib as B
import nabwa_testlib as T

nabwa = importlib.import_module("network-aware-bwa_amd")
pytestmark = pytest.mark.gpu


def gpu(n_ref, calls, u, c, walk=False):
    with nabwa.Bai(n_ref) as b:
        for recs, so in calls:
            data, off = B.pack(recs)
            b.add(data.tobytes() if walk else data, None if walk else off, so)
        return b.finish(u, c)


@pytest.fixture(scope="module")
def mix():
    """about 5 000 seeded sorted records, the table of blocks of 230 bytes behind a header, and what the oracle says"""
    recs = M.random_records(5000, 21)
    u, c = M.table(M.HEADER + sum(len(r) for r in recs), 230)
    return recs, u, c, M.oracle([(recs, M.HEADER)], 4, u, c)


def test_case_list_against_the_oracle():
    cases = M.all_cases()
    for name, n_ref, calls, u, c in cases:
        M.assert_same(gpu(n_ref, calls, u, c), M.oracle(calls, n_ref, u, c), name)
    name, n_ref, calls, u, c = cases[0]
    M.assert_same(gpu(n_ref, calls, u, c, walk=True), M.oracle(calls, n_ref, u, c), name + ", offsets walked from the block_size words")


def test_one_shot(mix):
    recs, u, c, want = mix
    data, off = B.pack(recs)
    M.assert_same(nabwa.bai(data, u, c, 4, M.HEADER, off), want, "nabwa.bai")
    M.assert_same(nabwa.bai(data.tobytes(), u, c, 4, stream_off=M.HEADER), want, "nabwa.bai, offsets walked")
    assert want[1][M.NO_COOR] > 100 and want[1][M.CHUNKS] > want[1][M.BINS] > 50 and want[1][M.WINDOWS] > 40


def test_many_calls_and_gaps(mix):
    recs, u, c, want = mix
    calls, at = [], M.HEADER
    for a in range(0, len(recs), 211):
        calls.append((recs[a:a + 211], at))
        at += sum(len(r) for r in recs[a:a + 211])
    assert len(calls) > 20
    M.assert_same(gpu(4, calls, u, c), want, "%d calls" % len(calls))
    gaps = [(r, so + 1000 * k) for k, (r, so) in enumerate(calls)]
    u2, c2 = M.table(M.stream_len(gaps), 230)
    want2 = M.oracle(gaps, 4, u2, c2)
    assert want2[0] != want[0]
    M.assert_same(gpu(4, gaps, u2, c2), want2, "calls with gaps")


def test_finish_twice_clear_size_and_cap(mix):
    recs, u, c, want = mix
    n0 = sum(len(r) for r in recs[:3000])
    u0, c0 = M.table(M.HEADER + n0, 230)
    L = nabwa.lib()
    with nabwa.Bai(4) as b:
        M.assert_same(b.finish(u, c), M.oracle([], 4, u, c), "nothing added")
        b.add(b"")
        b.add(np.zeros(0, np.uint8), np.zeros(1, np.int64), 5)
        M.assert_same(b.finish(u, c), M.oracle([], 4, u, c), "empty calls")
        b.add(*B.pack(recs[:3000]), M.HEADER)
        M.assert_same(b.finish(u0, c0), M.oracle([(recs[:3000], M.HEADER)], 4, u0, c0), "first finish")
        b.add(*B.pack(recs[3000:]), M.HEADER + n0)
        M.assert_same(b.finish(u, c), want, "second finish")
        M.assert_same(b.finish(u, c), want, "and again")
        ms = b.times()
        assert len(ms) == 7 and all(x >= 0 for x in ms) and ms[1] > 0 and ms[2] > 0
        # the size alone, and a buffer a byte too small
        assert b.size(u, c) == len(want[0])
        n, out, stats = C.c_int64(), np.zeros(len(want[0]), np.uint8), np.zeros(M.N_STATS, np.uint64)
        assert L.nabwa_bai_finish(b._h, u.size - 1, T.ptr(u), T.ptr(c), T.ptr(out), out.size - 1, C.byref(n), T.ptr(stats)) == nabwa.ECAP
        assert n.value == len(want[0]) and not out.any()
        assert L.nabwa_bai_finish(b._h, u.size - 1, T.ptr(u), T.ptr(c), T.ptr(out), out.size, None, None) == nabwa.OK and out.tobytes() == want[0]
        b.clear()
        M.assert_same(b.finish(u, c), M.oracle([], 4, u, c), "after clear")
        b.add(*B.pack(recs[:50]), 7)                               # the order and the offsets start afresh
        M.assert_same(b.finish(u, c), M.oracle([(recs[:50], 7)], 4, u, c), "an add after clear")


def test_damaged_records_are_named_and_add_nothing():
    good = M.good_records(400)
    n200 = sum(len(r) for r in good[:200])
    u, c = M.table(M.HEADER + sum(len(r) for r in good) + 4000, 97)
    want = M.oracle([(good[:200], M.HEADER)], 3, u, c)
    for name, r in M.damaged_cases():
        with nabwa.Bai(3) as b:
            b.add(*B.pack(good[:200]), M.HEADER)
            with pytest.raises(nabwa.NabwaError) as ex:
                b.add(*B.pack(good[200:230] + [r] + good[230:300] + [r]), M.HEADER + n200)
            assert ex.value.code == nabwa.EDATA and "record 30:" in str(ex.value), name
            M.assert_same(b.finish(u, c), want, name + ": the first call's records as if the second had never been made")
    with nabwa.Bai(3) as b:
        b.add(*B.pack(good[:200]), M.HEADER)
        with pytest.raises(nabwa.NabwaError):
            b.add(*B.pack([M.damaged_cases()[0][1]]), M.HEADER + n200)
        b.add(*B.pack(good[200:]), M.HEADER + n200)
        M.assert_same(b.finish(u, c), M.oracle([(good[:200], M.HEADER), (good[200:], M.HEADER + n200)], 3, u, c), "a good call after the failed one")


def test_records_out_of_order_are_damaged():
    good = [M.rec(0, 10 * k, "8M", name=b"s%d" % k) for k in range(40)] + [M.rec(1, 10 * k, "8M", name=b"t%d" % k) for k in range(20)]
    far = 10 ** 6

    def refused(b, recs, so, at):
        with pytest.raises(nabwa.NabwaError) as ex:
            b.add(*B.pack(recs), so)
        assert ex.value.code == nabwa.EDATA and "record %d:" % at in str(ex.value) and "order" in str(ex.value), str(ex.value)
    with nabwa.Bai(3) as b:
        b.add(*B.pack(good[:30]))
        refused(b, [good[29], good[28]], far, 1)                   # within a call (equal keys are in order)
        refused(b, [good[28]], far, 0)                             # across calls: the handle keeps the last key
        b.add(*B.pack([good[29], good[29], good[30]]), far)
        b.add(*B.pack([M.unmapped(), M.unmapped(-1, 5)]), 2 * far)
        refused(b, [M.unmapped(-1, 4)], 3 * far, 0)                # records without a reference are held to their order too
        refused(b, [good[59]], 3 * far, 0)                         # and nothing with a reference comes behind them
        kept = [(good[:30], 0), ([good[29], good[29], good[30]], far), ([M.unmapped(), M.unmapped(-1, 5)], 2 * far)]
        u, c = M.table(3 * far, 65536)
        M.assert_same(b.finish(u, c), M.oracle(kept, 3, u, c), "what the sound calls added")


def test_stream_offsets_and_block_tables_that_are_refused(mix):
    recs = mix[0][:100]
    data, off = B.pack(recs)
    total = M.HEADER + int(off[-1])
    u, c = M.table(total, 230)
    L = nabwa.lib()

    def finish(b, u, c):
        u, c = np.asarray(u, np.int64), np.asarray(c, np.int64)
        return L.nabwa_bai_finish(b._h, u.size - 1, T.ptr(u), T.ptr(c), None, 0, None, None)
    with nabwa.Bai(4) as b:
        b.add(data, off, M.HEADER)
        with pytest.raises(nabwa.NabwaError) as ex:
            b.add(data[:0], off[:1], total - 1)                    # even an empty call may not lie before the end
        assert ex.value.code == nabwa.EINVAL and "stream_off" in str(ex.value)
        assert finish(b, u, c) == nabwa.OK
        assert finish(b, u[:-1], c[:-1]) == nabwa.EINVAL and b"block table ends" in L.nabwa_last_error()      # a record ends behind the table
        assert finish(b, u + M.HEADER + 1, c) == nabwa.EINVAL and b"block table" in L.nabwa_last_error()       # a record starts before it
        bad = u.copy(); bad[3] = bad[2] - 1
        assert finish(b, bad, c) == nabwa.EINVAL and b"blk_uoff falls at block 2" in L.nabwa_last_error()
        bad = c.copy(); bad[3] = bad[2]
        assert finish(b, u, bad) == nabwa.EINVAL and b"blk_coff does not rise at block 2" in L.nabwa_last_error()
        assert finish(b, [0, 65537, total + 65537], [0, 10, 20]) == nabwa.EINVAL and b"65536" in L.nabwa_last_error()
        assert finish(b, u, c + ((1 << 48) - int(c[-1]))) == nabwa.EINVAL and b"48 bits" in L.nabwa_last_error()
        assert finish(b, u, c + ((1 << 48) - int(c[-1]) - 1)) == nabwa.OK
        M.assert_same(b.finish(u, c), M.oracle([(recs, M.HEADER)], 4, u, c), "after the refusals")
    h = C.c_void_p()
    assert L.nabwa_bai_create(1 << 20, 4, C.byref(h)) == nabwa.ENODEV and not h.value


def test_a_larger_file_read_back_through_its_index():
    """40 000 records (more than the persistent grid's first trip) in real BGZF blocks; the index equals the oracle's, the block table is that
    of the file, and regions read through the index give what a scan gives"""
    recs = M.random_records(40000, 33, span=3000000)
    header = b"BAM\1" + bytes(997)
    stream = header + b"".join(recs)
    data = M.bgzf_pack(stream, [0xff00], level=1)
    u, c = nabwa.bgzf_block_table(data)
    wu, wc = M.block_table(data)
    assert np.array_equal(u, wu) and np.array_equal(c, wc) and len(u) > 50
    got = nabwa.bai(b"".join(recs), u, c, 4, len(header))
    M.assert_same(got, M.oracle([(recs, len(header))], 4, u, c), "40 000 records")
    parsed = M.parse_bai(got[0])
    ext = [M.extent(r) for r in recs]
    for t, beg, end in ((0, 1500000, 1502000), (1, 0, 40000), (3, 2999000, 1 << 29), (2, 0, 1 << 29)):
        f = M.Bgzf(data)
        assert M.query(parsed, f, t, beg, end) == [r for r, e in zip(recs, ext) if e[0] == t and e[1] < end and e[2] > beg]      # M.scan, the extents taken once
        assert len(f.touched) < len(u) // 2


@pytest.mark.parametrize("kind", B.HEAD_DAMAGE)
def test_damage_in_the_head_of_the_middle_record_of_three(kind):
    """the two kinds of damage that all record-stream modules look for: the whole message, and the handle as it was"""
    good = [M.rec(0, 100, "25M"), M.rec(0, 200, "20M5S", name=b"s"), M.rec(1, 300, "25M", 16, name=b"t")]
    bad, text = B.head_damaged(good[1], kind, 1)
    u, c = M.table(M.HEADER + sum(len(r) for r in good) + 100, 97)
    with nabwa.Bai(3) as b:
        with pytest.raises(nabwa.NabwaError) as ex:
            b.add(*B.pack([good[0], bad, good[2]]), M.HEADER)
        assert ex.value.code == nabwa.EDATA and str(ex.value) == "libnabwa error %d: %s" % (nabwa.EDATA, text)
        b.add(*B.pack(good), M.HEADER)
        M.assert_same(b.finish(u, c), gpu(3, [(good, M.HEADER)], u, c), kind + ": as a fresh handle")
