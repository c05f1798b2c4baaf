"""The bodies of the damage profile (csrc/damage_body.hpp) on the CPU (tests/emu/damage_emu.cpp) against the Python oracle of
tests/damage_cases.py, on the case list tests/test_gpu_damage.py runs on the device: read lengths around the lanes' pieces, n_pos below and
above half a read, every record alignment and both nibble phases, CIGAR shapes up to 300 operations, reference windows at the reference's
ends and over its holes, read codes without a base, every skip class, every kind of damage, the golden SAM files.  A second build with
DMG_FLUSH_BYTES of a few hundred bytes takes the flush paths that otherwise only gigabytes of records take."""
import numpy as np
import pytest

import damage_cases as D
import nabwa_testlib as T


@pytest.fixture(scope="module")
def ref():
    return D.toy_ref()


@pytest.fixture(scope="module")
def emu():
    return D.load_emu()


@pytest.fixture(scope="module")
def emu_small():
    return D.load_emu(flush_bytes=300)


@pytest.fixture(scope="module")
def cases(ref):
    return [(name, opt, recs, D.oracle(ref, opt, recs)) for name, opt, recs in D.cases(ref)]


def test_case_list_covers_what_it_says(ref, cases):
    by = {name: (opt, recs, want) for name, opt, recs, want in cases}
    _, recs, want = by["alignments and nibble phases"]
    _, off = D.join(recs)
    assert [int(off[3 * a + 1]) % 16 for a in range(16)] == list(range(16)) and [int(off[3 * a + 2]) % 16 for a in range(16)] == [(a + 10) % 16 for a in range(16)]
    for n_pos in D.N_POSS:
        want = by["lengths, n_pos %d" % n_pos][2]
        assert [int(want.len_hist[L]) for L in D.LENGTHS] == [2] * len(D.LENGTHS)
        assert int(want.stats[D.COLS]) == 2 * sum(D.LENGTHS) and int(want.sub5.sum()) == int(want.sub3.sum()) == 2 * sum(D.LENGTHS)
        assert int(want.sub5[n_pos].sum()) == 2 * sum(max(L - n_pos, 0) for L in D.LENGTHS)
    st = by["holes"][2].stats
    assert st[D.COLS_SK_REF] > 200 and st[D.COLS] > 500
    st = by["reference windows"][2].stats
    assert st[D.COLS_SK_REF] == 2 * 20 + (7 + 5) + 8 + 8             # the columns at and past l_pac: 20 of 30M twice, 7 and 5 of 2S10M1D5M three bases before the end, two reads wholly outside
    st = by["read codes"][2].stats
    assert st[D.COLS_SK_READ] == 2 * 3 + 9 + 3 + 12 and st[D.COLS_SK_REF] == 3 - 2      # (of the hole's three columns two carry no base in the read: the read comes first)
    st = by["skip classes"][2].stats
    assert [int(x) for x in st[:6]] == [15, 2, 6, 4, 1, 2]
    st = by["skip classes, required flags"][2].stats
    assert int(st[D.SEEN]) == 18 and int(st[D.SK_FLAGS]) == 16 and int(st[D.COUNTED]) == 2      # only flags 0x11 and 0x51 hold both required bits
    want = by["CIGAR shapes"][2]
    assert int(want.stats[D.COUNTED]) == 17 and int(want.len_hist[4]) == 1


def test_bodies_against_the_oracle(ref, emu, emu_small, cases):
    for name, opt, recs, want in cases:
        for n_blocks in (1, 3, 64):
            D.assert_same(D.emu_tables(emu, ref, opt, recs, n_blocks), want, "%s, %d workgroups" % (name, n_blocks))
        D.assert_same(D.emu_tables(emu_small, ref, opt, recs, 2), want, name + ", flushes every 300 bytes")


def test_one_record_at_a_time_and_in_any_order(ref, emu, cases):
    for name, opt, recs, want in cases:
        w = np.zeros(want.words().size, np.uint64)
        for r in recs[::-1]:
            assert D.emu_add(emu, ref, opt, [r], w, 1) == -1
        D.assert_same(D.Tables.from_words(opt["n_pos"], w), want, name)


def test_two_calls_sum_to_one_call_over_the_concatenation(ref, emu):
    recs, opt = D.good_records(ref, 90), D.opt_of(n_pos=7)
    w = np.zeros(D.Tables(7).words().size, np.uint64)
    assert D.emu_add(emu, ref, opt, recs[:31], w) == -1 and D.emu_add(emu, ref, opt, recs[31:], w) == -1
    D.assert_same(D.Tables.from_words(7, w), D.oracle(ref, opt, recs), "two calls")
    D.assert_same(D.emu_tables(emu, ref, opt, recs), D.oracle(ref, opt, recs), "one call")


def test_damaged_records_are_named_and_count_nothing(ref, emu, emu_small):
    good, opt = D.good_records(ref, 40), D.opt_of()
    before = D.oracle(ref, opt, good[:20])
    for name, rec in D.damaged_cases(ref):
        for lib in (emu, emu_small):
            for recs, at in (([rec], 0), ([good[0], rec, good[1]], 1), (good[:17] + [rec] + good[17:30] + [rec] + good[30:], 17)):
                with pytest.raises(D.Damaged) as e:
                    D.oracle(ref, opt, recs)
                assert e.value.index == at, name
                w = before.words().copy()
                assert D.emu_add(lib, ref, opt, recs, w) == at, name
                assert np.array_equal(w, before.words()), name + ": the totals changed"
                assert D.emu_add(lib, ref, opt, good[20:], w) == -1                  # a following good call still adds
                D.assert_same(D.Tables.from_words(opt["n_pos"], w), D.oracle(ref, opt, good), name)


@pytest.mark.parametrize("sam", D.GOLDEN_SAMS)
def test_golden_sam_files(ref, emu, sam):
    recs, lines = D.sam_records("%s/%s.sam" % (T.GOLDEN, sam), ref)
    for opt in (D.opt_of(), D.opt_of(n_pos=3, min_mapq=25)):
        want = D.oracle(ref, opt, recs)
        assert int(want.stats[D.SEEN]) == len(lines) and want.stats[D.COUNTED] > 100
        D.assert_same(D.emu_tables(emu, ref, opt, recs, 5), want, sam)
