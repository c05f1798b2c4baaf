"""The bodies of duplicate marking (csrc/markdup_body.hpp) on the CPU (tests/emu/markdup_emu.cpp) against the Python oracle of
tests/markdup_cases.py, on the case lists tests/test_gpu_markdup.py runs on the device: every record alignment, read lengths around the
lanes' pieces, CIGARs longer than the lane group, clips of every kind on both strands, coordinates at the ends of their range, qualities on
either side of min_qual, read names that differ in one byte, every kind of damage.  The same cases run once more in a stand-alone program
built with -fsanitize=address,undefined, every buffer exactly as long as its records."""
import subprocess

import numpy as np
import pytest

import markdup_cases as M


@pytest.fixture(scope="module")
def emu():
    return M.load_emu()


@pytest.fixture(scope="module")
def cases():
    return [(name, opt, calls, M.oracle(calls, opt)) for name, opt, calls in M.shape_cases() + M.group_cases()]


def run(emu, opt, calls, n_blocks=3, reverse=False):
    e = M.Emu(emu, opt, n_blocks, reverse)
    for c in calls:
        assert e.add(c) == -1
    got = e.resolve()
    e.close()
    return got


def test_case_list_covers_what_it_says(cases):
    by = {name: (opt, calls, want) for name, opt, calls, want in cases}
    _, (recs,), _ = by["alignments"]
    off = np.concatenate([[0], np.cumsum([len(r) for r in recs])])
    assert [int(off[2 * a + 1]) % 16 for a in range(16)] == list(range(16))
    st = by["read names"][2][1]
    assert int(st[M.PAIRS]) == 2 * 5 and int(st[M.ORPHANS]) == 2 * 2 * 7                  # of the twelve couples of names five are equal
    st = by["coordinates"][2][1]
    assert int(st[M.FRAGMENTS]) == 9 and int(st[M.DUP_RECORDS]) == 2                     # neg, neg2 and zero's twin; big and big2
    assert [int(x) for x in by["qualities"][2][0]] == [1, 1, 1, 0, 1]                    # 14 and 0xff count nothing: qff16 and q16 both score 16, the earlier one wins
    assert [int(x) for x in by["qualities, min_qual 0"][2][0]] == [1, 1, 1, 1, 0]        # 16 + 7 * 14 is the most
    assert [int(x) for x in by["qualities, min_qual 17"][2][0]] == [0, 1, 1, 1, 1]       # nothing counts: the first wins
    d5, d_both = by["read lengths under ENDS_5P"][2], by["read lengths under ENDS_BOTH, and no shadows"][2]
    assert int(d5[0][:5].sum()) == 5 and int(d_both[0][:5].sum()) == 2                   # under a pair's shadow all five go; by both ends only the twins
    assert int(by["pairs"][2][1][M.DUP_PAIRS]) == 4                                      # two of a, b and e; one of g and h; one of i and j
    assert [int(x) for x in by["a fragment at a pair's end"][2][0]] == [1, 1, 0, 0, 0, 1]
    assert [int(x) for x in by["half pairs"][2][0]] == [1, 1, 0, 0, 1, 1, 0, 0, 1, 0, 0]
    assert int(by["mates in two calls are orphans"][2][1][M.ORPHANS]) == 2


def test_bodies_against_the_oracle(emu, cases):
    for name, opt, calls, want in cases:
        for n_blocks, reverse in ((1, False), (3, True), (64, False)):
            M.assert_same(run(emu, opt, calls, n_blocks, reverse), want, "%s, %d workgroups" % (name, n_blocks))


def test_the_split_into_calls_does_not_matter(emu):
    recs = M.random_records(600, 5)
    for opt in (M.opt_of(), M.opt_of(single_ends=M.ENDS_BOTH, min_qual=20)):
        want = M.oracle([recs], opt)
        assert want[1][M.DUP_PAIRS] > 5 and want[1][M.DUP_FRAGMENTS] > 20 and want[1][M.UNMAPPED] > 10 and 0 < want[0].sum() < len(recs)
        M.assert_same(run(emu, opt, [recs]), want, "one call")
        cuts = [i for i in range(1, len(recs)) if not (recs[i - 1][18] & 0x40 and recs[i][18] & 0x80)][::37]      # never between two mates
        calls = [recs[a:b] for a, b in zip([0] + cuts, cuts + [len(recs)])]
        assert len(calls) > 10
        M.assert_same(M.oracle(calls, opt), want, "the oracle, many calls")
        M.assert_same(run(emu, opt, calls, 2, True), want, "many calls")


def test_resolve_twice_and_clear(emu):
    recs, opt = M.random_records(300, 6), M.opt_of()
    e = M.Emu(emu, opt)
    M.assert_same(e.resolve(), M.oracle([], opt), "nothing added")
    assert e.add([]) == -1
    assert e.add(recs[:140]) == -1
    M.assert_same(e.resolve(), M.oracle([recs[:140]], opt), "first resolve")
    assert e.add(recs[140:]) == -1
    M.assert_same(e.resolve(), M.oracle([recs[:140], recs[140:]], opt), "second resolve")
    M.assert_same(e.resolve(), M.oracle([recs[:140], recs[140:]], opt), "and again")
    e.clear()
    assert e.add(recs[:50]) == -1
    M.assert_same(e.resolve(), M.oracle([recs[:50]], opt), "after clear")
    e.close()


def test_coordinates_at_the_ends_of_their_range(emu):
    opt = M.opt_of(single_ends=M.ENDS_BOTH)
    for inside, outside in M.edge_coordinate_records():
        assert M.parse(inside, opt) is not None and M.parse(outside, opt) is None
        e = M.Emu(emu, opt)
        assert e.add([inside, inside]) == -1 and e.add([inside, outside]) == 1
        assert [int(x) for x in e.resolve()[0]] == [0, 1]
        e.close()


def test_damaged_records_are_named_and_add_nothing(emu):
    good, opt = M.random_records(60, 7), M.opt_of()
    for name, r in M.damaged_cases():
        for recs, at in (([r], 0), ([good[0], r, good[1]], 1), (good[:17] + [r] + good[17:30] + [r] + good[30:], 17)):
            with pytest.raises(M.Damaged) as ex:
                M.oracle([recs], opt)
            assert ex.value.index == at, name
            e = M.Emu(emu, opt)
            assert e.add(good[:20]) == -1
            assert e.add(recs) == at, name
            M.assert_same(e.resolve(), M.oracle([good[:20]], opt), name + ": the failed call added something")
            assert e.add(good[20:]) == -1                                   # a following good call still adds
            M.assert_same(e.resolve(), M.oracle([good[:20], good[20:]], opt), name)
            e.close()


def test_cases_under_the_sanitizers(tmp_path, cases):
    exe = M.build_main()
    items = [(opt, [(c, -1) for c in calls], want[0], want[1]) for _, opt, calls, want in cases if sum(len(c) for c in calls) < 100]
    good, opt = M.random_records(40, 8), M.opt_of()
    want = M.oracle([good[:9], good[9:]], opt)
    for _, r in M.damaged_cases():
        items.append((opt, [(good[:9], -1), ([r], 0), (good[9:12] + [r] + good[12:20], 3), (good[9:], -1)], want[0], want[1]))
    for inside, outside in M.edge_coordinate_records():
        items.append((opt, [([inside], -1)], np.zeros(1, np.uint8), M.oracle([[inside]], opt)[1]))
    path = str(tmp_path / "cases.bin")
    M.write_case_file(path, items)
    r = subprocess.run([exe, path], capture_output=True, timeout=300)
    err = r.stderr.decode()
    assert "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
    assert r.returncode == 0, err[-2000:]
    assert r.stdout.decode().strip() == "ok %d" % (16 * sum(len(x[1]) + 1 for x in items))
