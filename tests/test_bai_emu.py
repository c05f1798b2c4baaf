"""The bodies of the BAM index (csrc/bai_body.hpp) on the CPU (tests/emu/bai_emu.cpp) against the Python oracle of tests/bai_cases.py, byte
for byte, on the case lists tests/test_gpu_bai.py runs on the device: every record alignment, CIGARs around the lane group, every
operation, placed and unplaced unmapped records, coordinates on either side of every bin boundary, windows, empty references, empty
inputs, the chunk rule, and block tables of every kind.  The same cases run once more in a stand-alone program built with
-fsanitize=address,undefined, every buffer exactly as long as its records."""
import subprocess

import numpy as np
import pytest

import bai_cases as M


@pytest.fixture(scope="module")
def emu():
    return M.load_emu()


@pytest.fixture(scope="module")
def cases():
    return [(name, n_ref, calls, u, c, M.oracle(calls, n_ref, u, c)) for name, n_ref, calls, u, c in M.all_cases()]


def run(emu, n_ref, calls, u, c, n_blocks=3):
    e = M.Emu(emu, n_ref, n_blocks)
    for recs, so in calls:
        assert e.add(recs, so) == -1
    got = e.finish(u, c)
    e.close()
    return got


def test_case_list_covers_what_it_says(cases):
    by = {name: (n_ref, calls, u, c, want) for name, n_ref, calls, u, c, want in cases}
    recs = by["alignments, blocks of 230"][1][0][0]
    off = np.concatenate([[0], np.cumsum([len(r) for r in recs])])
    assert [int(off[2 * a + 1]) % 16 for a in range(16)] == list(range(16))
    recs = by["CIGAR lengths, blocks of 230"][1][0][0]
    assert [int.from_bytes(r[16:18], "little") for r in recs] == [0, 1, 15, 16, 17, 33, 200, 33]
    bins = M.parse_bai(by["bin boundaries, blocks of 230"][4][0])[0][0][0]
    assert {0, 1, 9, 73, 585, 4681, 4682, 4681 + (1 << 15) - 1} <= set(bins)           # what crosses 2^26, 2^23, 2^20, 2^17 and 2^14; either side of 2^14; the last bin
    lin = M.parse_bai(by["windows, blocks of 230"][4][0])[0][0][1]
    assert len(lin) == 15 and lin[0] == lin[1] == lin[2] and lin[3] == lin[12] != lin[2] and lin[13] == lin[14] != lin[12]      # three windows of one read; a gap filled from behind; the long read's last window
    refs = M.parse_bai(by["empty references, blocks of 230"][4][0])[0]
    assert [bool(b) for b, _ in refs] == [False, True, False, True, False, False] and [len(l) for _, l in refs] == [0, 1, 0, 5, 0, 0]
    # the chunk rule: a1 and a2 .. a4 are one chunk where they share blocks, and several where they do not
    assert len(M.parse_bai(by["chunks, blocks of 65536"][4][0])[0][0][0][4681]) == 1
    assert len(M.parse_bai(by["chunks, blocks of 37"][4][0])[0][0][0][4681]) == 3                       # a1 | a2 a3 | a4
    assert int(by["chunks, offsets near 2^48"][3][-1]) >> 40 == 0xff
    assert by["nothing, blocks of 230"][4][0] == b"BAI\1" + bytes([3, 0, 0, 0]) + bytes(24 + 8)
    assert by["nothing, no references, blocks of 230"][4][0] == b"BAI\1" + bytes(4 + 8)
    st = by["unmapped, placed and not, blocks of 230"][4][1]
    assert (int(st[M.RECORDS]), int(st[M.PLACED]), int(st[M.NO_COOR])) == (10, 7, 3)
    u = by["chunks, an empty block"][2]
    assert u[1] == u[2]


def test_bodies_against_the_oracle(emu, cases):
    for name, n_ref, calls, u, c, want in cases:
        for n_blocks in (1, 3, 64):
            M.assert_same(run(emu, n_ref, calls, u, c, n_blocks), want, "%s, %d workgroups" % (name, n_blocks))


def test_the_split_into_calls_and_gaps_do_not_matter(emu):
    recs = M.random_records(700, 5)
    total = M.HEADER + sum(len(r) for r in recs)
    u, c = M.table(total, 230)
    want = M.oracle([(recs, M.HEADER)], 4, u, c)
    assert want[1][M.NO_COOR] > 10 and want[1][M.CHUNKS] > want[1][M.BINS] > 30 and want[1][M.WINDOWS] > 30
    M.assert_same(run(emu, 4, [(recs, M.HEADER)], u, c), want, "one call")
    calls, at = [], M.HEADER
    for a in range(0, len(recs), 37):
        calls.append((recs[a:a + 37], at))
        at += sum(len(r) for r in recs[a:a + 37])
    assert len(calls) > 10
    M.assert_same(M.oracle(calls, 4, u, c), want, "the oracle, many calls")
    M.assert_same(run(emu, 4, calls, u, c, 2), want, "many calls")
    # gaps between the calls: other offsets, so another file, but the oracle's for those offsets
    gaps = [(r, so + 1000 * k) for k, (r, so) in enumerate(calls)]
    u2, c2 = M.table(M.stream_len(gaps), 230)
    want2 = M.oracle(gaps, 4, u2, c2)
    assert want2[0] != want[0] and len(want2[0]) >= len(want[0])
    M.assert_same(run(emu, 4, gaps, u2, c2, 5), want2, "many calls with gaps")


def test_finish_twice_and_clear(emu):
    recs = M.random_records(300, 6)
    n0 = sum(len(r) for r in recs[:140])
    u, c = M.table(M.HEADER + sum(len(r) for r in recs), 150)
    u0, c0 = M.table(M.HEADER + n0, 150)
    e = M.Emu(emu, 4)
    M.assert_same(e.finish(u, c), M.oracle([], 4, u, c), "nothing added")
    assert e.add([]) == -1
    assert e.add(recs[:140], M.HEADER) == -1
    M.assert_same(e.finish(u0, c0), M.oracle([(recs[:140], M.HEADER)], 4, u0, c0), "first finish")
    assert e.add(recs[140:], M.HEADER + n0) == -1
    M.assert_same(e.finish(u, c), M.oracle([(recs, M.HEADER)], 4, u, c), "second finish")
    M.assert_same(e.finish(u, c), M.oracle([(recs, M.HEADER)], 4, u, c), "and again")
    e.clear()
    assert e.add(recs[:50], 7) == -1                           # the order starts afresh
    M.assert_same(e.finish(u, c), M.oracle([(recs[:50], 7)], 4, u, c), "after clear")
    e.close()


def test_damaged_records_are_named_and_add_nothing(emu):
    good = M.good_records(60)
    n20 = sum(len(r) for r in good[:20])
    for name, r in M.damaged_cases():
        for recs, at in (([r], 0), ([good[20], r, good[41]], 1), (good[20:37] + [r] + good[37:50] + [r] + good[50:], 17)):
            with pytest.raises(M.Damaged) as ex:
                M.oracle([(recs, 0)], 3, [0, 1 << 16], [0, 100])
            assert ex.value.index == at, name
            tail = sum(len(x) for x in recs)
            u, c = M.table(M.HEADER + n20 + tail + sum(len(x) for x in good[20:]), 97)
            e = M.Emu(emu, 3)
            assert e.add(good[:20], M.HEADER) == -1
            assert e.add(recs, M.HEADER + n20) == at, name
            M.assert_same(e.finish(u, c), M.oracle([(good[:20], M.HEADER)], 3, u, c), name + ": the failed call added something")
            assert e.add(good[20:], M.HEADER + n20) == -1          # a following good call still adds, at the offset the failed one had
            M.assert_same(e.finish(u, c), M.oracle([(good[:20], M.HEADER), (good[20:], M.HEADER + n20)], 3, u, c), name)
            e.close()


def test_records_out_of_order_are_damaged(emu):
    good = [M.rec(0, 10 * k, "8M", name=b"s%d" % k) for k in range(40)] + [M.rec(1, 10 * k, "8M", name=b"t%d" % k) for k in range(20)]
    e = M.Emu(emu, 3)
    assert e.add(good[:30]) == -1
    assert e.add([good[29], good[28]], 10 ** 6) == 1               # within a call (equal keys are in order)
    assert e.add([good[28]], 10 ** 6) == 0                         # across calls: the handle keeps the last key
    assert e.add([good[29], good[29], good[30]], 10 ** 6) == -1
    assert e.add([M.unmapped(), M.unmapped(-1, 5)], 2 * 10 ** 6) == -1
    assert e.add([M.unmapped(-1, 4)], 3 * 10 ** 6) == 0            # records without a reference are held to their order too
    assert e.add([good[59]], 3 * 10 ** 6) == 0                     # and nothing with a reference comes behind them
    for bad in ([good[3], good[2]], [good[2], good[2], good[1]]):
        with pytest.raises(M.Damaged) as ex:
            M.oracle([(bad, 0)], 3, [0, 1 << 16], [0, 100])
        assert ex.value.index == len(bad) - 1
    with pytest.raises(M.Damaged) as ex:
        M.oracle([(good[:30], 0), ([good[28]], 10 ** 6)], 3, [0, 1 << 16, 1 << 17], [0, 100, 200])
    assert ex.value.index == 0
    e.close()


def test_cases_under_the_sanitizers(tmp_path, cases):
    exe = M.build_main()
    items = [(n_ref, [(recs, so, -1) for recs, so in calls], u, c, want[0], want[1]) for _, n_ref, calls, u, c, want in cases]
    good = M.good_records(40)
    n9 = sum(len(r) for r in good[:9])
    u, c = M.table(M.HEADER + sum(len(r) for r in good), 97)
    want = M.oracle([(good[:9], M.HEADER), (good[9:], M.HEADER + n9)], 3, u, c)
    low = M.rec(0, 0, "5M", name=b"low")
    assert M.sort_key(low) < M.sort_key(good[8])                   # out of order behind the first call
    for _, r in M.damaged_cases():
        items.append((3, [(good[:9], M.HEADER, -1), ([r], M.HEADER + n9, 0), (good[9:12] + [r] + good[12:20], M.HEADER + n9, 3), ([low] + good[9:], M.HEADER + n9, 0), (good[9:], M.HEADER + n9, -1)], u, c, want[0], want[1]))
    path = str(tmp_path / "cases.bin")
    M.write_case_file(path, items)
    r = subprocess.run([exe, path], capture_output=True, timeout=300)
    err = r.stderr.decode()
    assert "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
    assert r.returncode == 0, err[-2000:]
    assert r.stdout.decode().strip() == "ok %d" % (16 * sum(len(x[1]) + 1 for x in items))
