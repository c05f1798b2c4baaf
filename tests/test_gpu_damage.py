"""nabwa_damage_* on the GPU (csrc/nabwa_damage.hip, damage_kernels.hip) and its Python face (nabwa.Damage) against the Python oracle of
tests/damage_cases.py: the case list tests/test_damage_emu.py runs through the bodies on the CPU, here through the kernel on the toy index;
damaged records; the argument checks that need a live handle; exact counts under contention, the same tables run after run, accumulation
and clear; the reference copy shared with the finishing chains' device path; a reference whose length is no multiple of 4; the nucleotide
reference of a colour index (which_ref 1)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import bamlib as B
import damage_cases as D
import nabwa_testlib as T

nabwa = importlib.import_module("network-aware-bwa_amd")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    return D.toy_ref()


@pytest.fixture(scope="module")
def ix():
    x = nabwa.Index.load(T.TOY, 0, True, with_ref=True)
    yield x
    x.close()


def tables_of(d):
    t = D.Tables(d.n_pos)
    for a, b in zip(t.parts(), d.fetch()):
        assert a.shape == b.shape and b.dtype == np.uint64
        a[:] = b
    return t


def gpu_tables(ix, opt, recs, which_ref=0, walk=False):
    with nabwa.Damage(ix, which_ref=which_ref, **opt) as d:
        data, off = D.join(recs)
        d.add(data.tobytes(), None if walk else off)
        return tables_of(d)


def test_case_list_against_the_oracle(ix, ref):
    for name, opt, recs in D.cases(ref):
        D.assert_same(gpu_tables(ix, opt, recs), D.oracle(ref, opt, recs), name)
    name, opt, recs = D.cases(ref)[0]
    D.assert_same(gpu_tables(ix, opt, recs, walk=True), D.oracle(ref, opt, recs), name + ", offsets walked from the block_size words")


@pytest.mark.parametrize("sam", D.GOLDEN_SAMS)
def test_golden_sam_files(ix, ref, sam):
    recs, _ = D.sam_records("%s/%s.sam" % (T.GOLDEN, sam), ref)
    want = D.oracle(ref, D.opt_of(), recs)
    assert want.stats[D.COUNTED] > 100
    D.assert_same(gpu_tables(ix, D.opt_of(), recs), want, sam)


def test_damaged_records_are_named_and_count_nothing(ix, ref):
    good, opt = D.good_records(ref, 40), D.opt_of()
    with nabwa.Damage(ix) as d:
        d.add(b"".join(good[:20]))
        before = tables_of(d)
        D.assert_same(before, D.oracle(ref, opt, good[:20]), "before")
        for name, rec in D.damaged_cases(ref):
            for recs, at in (([rec], 0), ([good[0], rec, good[1]], 1), (good[:17] + [rec] + good[17:30] + [rec] + good[30:], 17)):
                data, off = D.join(recs)
                with pytest.raises(nabwa.NabwaError) as e:
                    d.add(data.tobytes(), off)
                assert e.value.code == nabwa.EDATA and "record %d:" % at in str(e.value), (name, str(e.value))
                D.assert_same(tables_of(d), before, name + ": the totals changed")
        d.add(b"".join(good[20:]))                        # a following good call still adds
        D.assert_same(tables_of(d), D.oracle(ref, opt, good), "after")


def test_argument_checks_on_a_live_handle(ix, ref):
    L = nabwa.lib()
    data, off = D.join(D.good_records(ref, 5))
    with nabwa.Damage(ix) as d:
        h = d._h
        assert L.nabwa_damage_add(h, -1, T.ptr(data), T.ptr(off)) == nabwa.EINVAL
        assert L.nabwa_damage_add(h, 1 << 31, T.ptr(data), T.ptr(off)) == nabwa.EINVAL
        assert L.nabwa_damage_add(h, 5, None, T.ptr(off)) == nabwa.EINVAL
        assert L.nabwa_damage_add(h, 5, T.ptr(data), None) == nabwa.EINVAL
        flat = off.copy(); flat[3] = flat[2]
        assert L.nabwa_damage_add(h, 5, T.ptr(data), T.ptr(flat)) == nabwa.EINVAL and b"record 2" in L.nabwa_last_error()
        back = off.copy(); back[3] = back[2] - 1
        assert L.nabwa_damage_add(h, 5, T.ptr(data), T.ptr(back)) == nabwa.EINVAL
        short = np.array([0, 40, 75, 120], np.int64)
        assert L.nabwa_damage_add(h, 3, T.ptr(data), T.ptr(short)) == nabwa.EINVAL and b"record 1 has 35 bytes" in L.nabwa_last_error()
        assert L.nabwa_damage_add(h, 0, None, T.ptr(np.zeros(1, np.int64))) == nabwa.OK
        assert not any(x.any() for x in d.fetch())                           # none of these counted
        assert L.nabwa_damage_fetch(h, None, None, None, None) == nabwa.OK   # any output may be left out
        st = np.zeros(len(nabwa.damage_stat_names), np.uint64)
        d.add(data.tobytes(), off)
        assert L.nabwa_damage_fetch(h, None, None, None, T.ptr(st)) == nabwa.OK and int(st[D.SEEN]) == 5
        ms = d.times()
        assert len(ms) == 3 and all(x >= 0 for x in ms) and ms[1] > 0
    for bad in (dict(n_pos=0), dict(n_pos=257), dict(which_ref=2), dict(which_ref=1)):      # (the toy index has no nucleotide reference)
        with pytest.raises(nabwa.NabwaError) as e:
            nabwa.Damage(ix, **bad)
        assert e.value.code == nabwa.EINVAL
    bare = nabwa.Index.load(T.TOY, 0, True, with_ref=False)
    with pytest.raises(nabwa.NabwaError) as e:
        nabwa.Damage(bare)
    assert e.value.code == nabwa.EINVAL and "no reference attached" in str(e.value)
    bare.close()


def test_offsets_that_do_not_start_at_zero(ix, ref):
    recs = D.good_records(ref, 30, seed=5)
    data, off = D.join(recs)
    with nabwa.Damage(ix, n_pos=4) as d:
        d.add(data, off[10:])                              # records 10..29, where they lie in `data`
        D.assert_same(tables_of(d), D.oracle(ref, D.opt_of(n_pos=4), recs[10:]), "from record 10 on")


def test_exact_counts_under_contention_and_the_same_tables_twice(ix, ref):
    rng = np.random.default_rng(3)
    rec = D.aligned(ref, rng, 0, 1234, "3S60M2I30M", 16, mut=0.3, name_len=7)
    one = D.oracle(ref, D.opt_of(), [rec])
    with nabwa.Damage(ix) as d:
        d.add(rec * 4096)
        got = tables_of(d)
        for a, b in zip(got.parts(), one.parts()):
            assert np.array_equal(a, b * np.uint64(4096))
        d.clear()
        d.add(rec * 4096)
        D.assert_same(tables_of(d), got, "the same input again")
    mixed = D.good_records(ref, 3000, seed=9)
    want = D.oracle(ref, D.opt_of(), mixed)
    first = gpu_tables(ix, D.opt_of(), mixed)
    D.assert_same(first, want, "3000 records")
    D.assert_same(gpu_tables(ix, D.opt_of(), mixed), first, "3000 records again")


def test_three_calls_add_up_and_clear_empties(ix, ref):
    recs, opt = D.good_records(ref, 200, seed=11), D.opt_of(n_pos=256, min_mapq=10)
    with nabwa.Damage(ix, **opt) as d:
        for part in (recs[:1], recs[1:120], recs[120:]):
            d.add(b"".join(part))
        D.assert_same(tables_of(d), D.oracle(ref, opt, recs), "three calls")
        d.clear()
        assert not any(x.any() for x in d.fetch())
        d.add(b"".join(recs[:50]))
        D.assert_same(tables_of(d), D.oracle(ref, opt, recs[:50]), "after clear")


def test_the_reference_copy_is_the_finishing_chains(ref):
    """nabwa_cal_md puts the reference into HBM for the finishing chains' device path (NABWA_FINISH=gpu); a handle made afterwards adds no
    byte of reference, and one made first leaves nothing for nabwa_cal_md to add"""
    recs = D.good_records(ref, 60, seed=13)
    want = D.oracle(ref, D.opt_of(), recs)
    ref_bytes = ref.l_pac // 4 + 1 + 16 * len(ref.holes)
    for damage_first in (False, True):
        x = nabwa.Index.load(T.TOY, 0, True, with_ref=True)
        b0, d0 = nabwa.finish_counts()[3], x.device_bytes()

        def md():
            qry = ref.codes[1000:1030].astype(np.uint8)
            x.cal_md(qry, np.array([0, 30], np.int64), np.array([1000], np.uint32), [np.zeros(0, np.uint16)])      # (what it answers: tests/test_gpu_finish.py)
        if not damage_first:
            md()
            assert nabwa.finish_counts()[3] - b0 == ref_bytes == x.device_bytes() - d0
        D.assert_same(gpu_tables(x, D.opt_of(), recs), want, "damage_first %s" % damage_first)
        assert nabwa.finish_counts()[3] - b0 == ref_bytes == x.device_bytes() - d0
        md()
        D.assert_same(gpu_tables(x, D.opt_of(), recs), want, "second pass")
        assert nabwa.finish_counts()[3] - b0 == ref_bytes == x.device_bytes() - d0
        x.close()


def test_a_reference_whose_length_is_no_multiple_of_four():
    rng = np.random.default_rng(21)
    for l_pac in (4099, 4098, 4097):
        pac = rng.integers(0, 256, (l_pac + 3) // 4, dtype=np.uint8)
        x = nabwa.Index.load(T.TOY, 0, True, with_ref=True)
        names, offs, lens = x.set_reference(l_pac, 11, pac, n_contigs=3)
        ref = D.Ref(pac.tobytes(), l_pac, list(zip(names, [int(o) for o in offs], [int(n) for n in lens])), [])
        last = int(lens[2])
        recs = [D.aligned(ref, rng, 2, last - L, "%dM" % L, f) for L in (1, 2, 3, 4, 5, 8, 9, 40) for f in (0, 16)]
        recs += [D.aligned(ref, rng, 2, last - 5, "12M", 0), D.aligned(ref, rng, 2, last, "3M", 16), D.aligned(ref, rng, 0, int(lens[0]) - 7, "20M", 0), D.aligned(ref, rng, 0, 0, "64M1D3M", 16)]
        want = D.oracle(ref, D.opt_of(n_pos=2), recs)
        assert int(want.stats[D.COLS_SK_REF]) == 7 + 3
        D.assert_same(gpu_tables(x, D.opt_of(n_pos=2), recs), want, "l_pac %d" % l_pac)
        x.close()


def test_the_nucleotide_reference_of_a_colour_index(ref, tmp_path):
    """which_ref 1: the bases of <prefix>.nt.pac under the index's annotations.  The packing step of `nabwa_index -c` (host work) writes the
    toy genome's nucleotide files, which hold the bases of toy.pac; attached to the toy index they make it stand in for a colour index"""
    prefix = str(tmp_path / "toycs")
    assert nabwa.index_fa2pac(T.TOY + ".fa", prefix, colour=True) == ref.l_pac
    x = nabwa.Index.load(T.TOY, 0, True, with_ref=True)
    x.attach_nt_reference(prefix)
    name, opt, recs = [c for c in D.cases(ref) if c[0] == "holes"][0]
    want = D.oracle(ref, opt, recs)
    D.assert_same(gpu_tables(x, opt, recs, which_ref=1), want, "which_ref 1")
    D.assert_same(gpu_tables(x, opt, recs, which_ref=0), want, "which_ref 0 beside it")
    x.close()


@pytest.mark.parametrize("kind", B.HEAD_DAMAGE)
def test_damage_in_the_head_of_the_middle_record_of_three(ix, ref, kind):
    """the two kinds of damage that all record-stream modules look for: the whole message, and the handle as it was"""
    good = D.good_records(ref, 3)
    bad, text = B.head_damaged(good[1], kind, 1)
    with nabwa.Damage(ix) as d:
        data, off = D.join([good[0], bad, good[2]])
        with pytest.raises(nabwa.NabwaError) as ex:
            d.add(data.tobytes(), off)
        assert ex.value.code == nabwa.EDATA and str(ex.value) == "libnabwa error %d: %s" % (nabwa.EDATA, text)
        data, off = D.join(good)
        d.add(data.tobytes(), off)
        D.assert_same(tables_of(d), gpu_tables(ix, D.opt_of(), good), kind + ": as a fresh handle")
