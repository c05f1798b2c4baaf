"""nabwa_markdup_* on the GPU (csrc/nabwa_markdup.hip, markdup_kernels.hip) and its Python face (nabwa.MarkDup, nabwa.markdup) against the
Python oracle of tests/markdup_cases.py: the case lists tests/test_markdup_emu.py runs through the bodies on the CPU, here through the
kernels; groups larger than a wavefront and a workgroup; calls split in any way; a seeded mix resolved twice; damaged records; the argument
checks that need a live handle; and the permutation of nabwa_bam_sort_ex."""
import ctypes as C
import importlib
import struct

import numpy as np
import pytest

import bam_sort_cases as S
import bamlib as B
import markdup_cases as M
import nabwa_testlib as T

nabwa = importlib.import_module("network-aware-bwa_amd")
pytestmark = pytest.mark.gpu
ENDS = {M.ENDS_5P: "5p", M.ENDS_BOTH: "both"}


def handle(opt):
    return nabwa.MarkDup(0, opt["min_qual"], ENDS[opt["single_ends"]], opt["exclude_flags"])


def gpu(opt, calls, walk=False):
    with handle(opt) as m:
        for c in calls:
            data, off = B.pack(c)
            m.add(data.tobytes() if walk else data, None if walk else off)
        return m.resolve()


@pytest.fixture(scope="module")
def mix():
    """about 2 000 records drawn from a handful of sites, and what the oracle says of the first 1 500 and of all"""
    recs = M.random_records(2000, 21)
    cut = 1500 + bool(recs[1499][18] & 0x40 and recs[1500][18] & 0x80)
    return recs, cut, M.oracle([recs[:cut]], M.opt_of()), M.oracle([recs[:cut], recs[cut:]], M.opt_of())


def test_shapes_of_a_record_against_the_oracle():
    for name, opt, calls in M.shape_cases():
        M.assert_same(gpu(opt, calls), M.oracle(calls, opt), name)
    name, opt, calls = M.shape_cases()[0]
    M.assert_same(gpu(opt, calls, walk=True), M.oracle(calls, opt), name + ", offsets walked from the block_size words")


def test_groups_pairs_and_classes_against_the_oracle():
    """groups of 1, 2, 3, 65 and 257 in one, two and three calls; strands; clips; ENDS_BOTH; pairs; shadows; half pairs; orphans; classes"""
    for name, opt, calls in M.group_cases():
        M.assert_same(gpu(opt, calls), M.oracle(calls, opt), name)


def test_a_seeded_mix_resolved_twice(mix):
    recs, cut, want_first, want_all = mix
    assert want_all[1][M.DUP_PAIRS] > 50 and want_all[1][M.DUP_FRAGMENTS] > 500 and want_all[1][M.UNMAPPED] > 50 and want_all[1][M.ORPHANS] > 20
    assert max(np.bincount(want_all[0])) < len(recs)
    with handle(M.opt_of()) as m:
        m.add(*B.pack(recs[:cut]))
        M.assert_same(m.resolve(), want_first, "the first resolve")
        m.add(*B.pack(recs[cut:]))
        M.assert_same(m.resolve(), want_all, "the second resolve")
        M.assert_same(m.resolve(), want_all, "and again")
        ms = m.times()
        assert len(ms) == 5 and all(x >= 0 for x in ms) and ms[1] > 0 and ms[2] > 0
    both = M.opt_of(single_ends=M.ENDS_BOTH)
    M.assert_same(gpu(both, [recs]), M.oracle([recs], both), "both ends")


def test_many_calls_give_what_one_call_gives(mix):
    recs, _, _, want = mix
    cuts = [i for i in range(1, len(recs)) if not (recs[i - 1][18] & 0x40 and recs[i][18] & 0x80)][::53]
    calls = [recs[a:b] for a, b in zip([0] + cuts, cuts + [len(recs)])]
    assert len(calls) > 20
    M.assert_same(gpu(M.opt_of(), calls), want, "%d calls" % len(calls))


def test_nothing_added_and_clear(mix):
    recs = mix[0]
    with handle(M.opt_of()) as m:
        dup, stats = m.resolve()
        assert dup.size == 0 and not stats.any()
        m.add(b"")
        m.add(np.zeros(0, np.uint8), np.zeros(1, np.int64))
        dup, stats = m.resolve()
        assert dup.size == 0 and not stats.any()
        m.add(*B.pack(recs[:300]))
        assert m.resolve()[1][M.SEEN] == 300
        m.clear()
        dup, stats = m.resolve()
        assert dup.size == 0 and not stats.any()
        m.add(*B.pack(recs[300:500]))
        M.assert_same(m.resolve(), M.oracle([recs[300:500]], M.opt_of()), "after clear")


def test_a_damaged_record_in_the_second_call(mix):
    recs, opt = mix[0][:400], M.opt_of()
    want = M.oracle([recs[:200]], opt)
    for name, r in M.damaged_cases():
        with handle(opt) as m:
            m.add(*B.pack(recs[:200]))
            with pytest.raises(nabwa.NabwaError) as ex:
                m.add(*B.pack(recs[200:230] + [r] + recs[230:300] + [r]))
            assert ex.value.code == nabwa.EDATA and "record 30:" in str(ex.value), name
            M.assert_same(m.resolve(), want, name + ": the first call's records as if the second had never been made")
    with handle(opt) as m:
        m.add(*B.pack(recs[:200]))
        with pytest.raises(nabwa.NabwaError):
            m.add(*B.pack([M.damaged_cases()[0][1]]))
        m.add(*B.pack(recs[200:]))
        M.assert_same(m.resolve(), M.oracle([recs[:200], recs[200:]], opt), "a good call after the failed one")


def test_argument_checks_on_a_live_handle(mix):
    L = nabwa.lib()
    data, off = B.pack(mix[0][:10])
    with handle(M.opt_of()) as m:
        h = m._h
        assert L.nabwa_markdup_add(h, -1, T.ptr(data), T.ptr(off)) == nabwa.EINVAL
        assert L.nabwa_markdup_add(h, 1 << 31, T.ptr(data), T.ptr(off)) == nabwa.EINVAL
        assert L.nabwa_markdup_add(h, 10, None, T.ptr(off)) == nabwa.EINVAL
        assert L.nabwa_markdup_add(h, 10, T.ptr(data), None) == nabwa.EINVAL
        bad = off.copy(); bad[4] = bad[3]
        assert L.nabwa_markdup_add(h, 10, T.ptr(data), T.ptr(bad)) == nabwa.EINVAL and b"record 3" in L.nabwa_last_error()
        bad = off.copy(); bad[4] = bad[3] + 35
        assert L.nabwa_markdup_add(h, 10, T.ptr(data), T.ptr(bad)) == nabwa.EINVAL and b"at least 36" in L.nabwa_last_error()
        bad = off.copy(); bad[0] = -1
        assert L.nabwa_markdup_add(h, 10, T.ptr(data), T.ptr(bad)) == nabwa.EINVAL
        assert L.nabwa_markdup_add(h, 10, T.ptr(data), T.ptr(off)) == nabwa.OK
        dup, stats = np.zeros(10, np.uint8), np.zeros(M.N_STATS, np.uint64)
        assert L.nabwa_markdup_resolve(h, T.ptr(dup), 9, T.ptr(stats)) == nabwa.ECAP and b"10" in L.nabwa_last_error()
        assert L.nabwa_markdup_resolve(h, None, 10, T.ptr(stats)) == nabwa.EINVAL
        assert L.nabwa_markdup_resolve(h, T.ptr(dup), -1, T.ptr(stats)) == nabwa.EINVAL
        assert L.nabwa_markdup_resolve(h, T.ptr(dup), 10, None) == nabwa.OK
    o = nabwa.MarkDupOpt()
    L.nabwa_markdup_default_opt(C.byref(o))
    hh = C.c_void_p()
    assert L.nabwa_markdup_create(1 << 20, C.byref(o), C.byref(hh)) == nabwa.ENODEV and not hh.value


def test_markdup_sets_the_flag_on_the_duplicates(mix):
    recs, _, _, want = mix
    data, off = B.pack(recs)
    out, dup, stats = nabwa.markdup(data.tobytes())
    M.assert_same((dup, stats), want, "nabwa.markdup")
    assert len(out) == data.size
    for i, r in enumerate(recs):
        got = out[off[i]:off[i + 1]]
        flag = struct.unpack_from("<H", r, 18)[0]
        assert got == r[:18] + struct.pack("<H", flag | (0x400 if dup[i] else 0)) + r[20:], i
    out2, dup2, _ = nabwa.markdup(data.tobytes(), single_ends="both", min_qual=0)
    M.assert_same((dup2, _), M.oracle([recs], M.opt_of(single_ends=M.ENDS_BOTH, min_qual=0)), "nabwa.markdup with options")


def test_bam_sort_gives_the_permutation(mix):
    """perm is the stable argsort of the keys, records[perm] are the output records, and the first three results are those of the call without it"""
    data, off = B.pack(mix[0])
    out, out_off, keys = nabwa.bam_sort(data, off)
    out_p, out_off_p, keys_p, perm = nabwa.bam_sort(data, off, perm=True)
    assert out_p == out and np.array_equal(out_off_p, out_off) and np.array_equal(keys_p, keys)
    assert perm.dtype == np.uint32 and np.array_equal(perm, np.argsort(S.keys_of(data, off), kind="stable"))
    for j in (0, 1, len(perm) // 2, len(perm) - 1):
        i = int(perm[j])
        assert out[out_off[j]:out_off[j + 1]] == data[off[i]:off[i + 1]].tobytes()
    with nabwa.BamSort(0) as s:
        a = s.sort(data, off)
        b = s.run(data, off, perm=True)
        assert len(a) == 3 and a[0] == out and b[0] == out and np.array_equal(b[3], perm)
    assert len(nabwa.bam_sort(b"", perm=True)[3]) == 0


@pytest.mark.parametrize("kind", B.HEAD_DAMAGE)
def test_damage_in_the_head_of_the_middle_record_of_three(kind):
    """the two kinds of damage that all record-stream modules look for: the whole message, and the handle as it was"""
    good, opt = [M.rec(0, 900, "25M"), M.rec(0, 900, "20M5S", name=b"s"), M.rec(0, 900, "25M", 16, name=b"t")], M.opt_of()
    bad, text = B.head_damaged(good[1], kind, 1)
    with handle(opt) as m:
        with pytest.raises(nabwa.NabwaError) as ex:
            m.add(*B.pack([good[0], bad, good[2]]))
        assert ex.value.code == nabwa.EDATA and str(ex.value) == "libnabwa error %d: %s" % (nabwa.EDATA, text)
        m.add(*B.pack(good))
        M.assert_same(m.resolve(), gpu(opt, [good]), kind + ": as a fresh handle")
