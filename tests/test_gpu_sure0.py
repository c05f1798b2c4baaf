"""Kernel S's shortcut for reads one of whose strands occurs exactly (NABWA_SURE0) must change speed only.  A small
genome of its own with planted copies; every read of every batch is compared with the CPU oracle, which searches each read on its
own: the hit count, every row (info, k, l, score) and max_entries, for NABWA_SURE0 = 0, 1 and 2.  NABWA_SURE0_STATS counts what
the shortcut did, so each case also asserts that it ran where it should (reads, children resolved as dead, children stored landed),
that it stayed off where its preconditions do not hold, and that its safety net never fired."""
import ctypes as C
import importlib

import numpy as np
import pytest

import nabwa_testlib as T
from test_gpu_batch_mix import COMP, Oracle, check, collect, encode, gap_opt, mutate

pytestmark = pytest.mark.gpu
nabwa = importlib.import_module("network-aware-bwa_amd")
synth = importlib.import_module("network-aware-bwa_amd.synth")

N = 400_009                      # interval-table depth KT = floor(log4 N) + 1 = 10; a random 10-mer occurs with p = 1 - exp(-N / 4^10) = 0.32:
KT = 10                          # of the 1-mismatch children of a descent some die at their tail jump and some survive it
LEVELS = (0, 1, 2)


def rc(s):
    return s.translate(COMP)[::-1]


def sub(s, p, j=1):
    return s[:p] + "ACGT"[("ACGT".index(s[p]) + j) % 4] + s[p + 1:]


def make_world(rng):
    """-> (genome text, [(kind, read)]).  Planted pieces go to slots of 400 bases, one piece per slot, so that no piece overlaps another."""
    g = list("".join("ACGT"[x] for x in rng.integers(0, 4, N)))
    slots = [int(x) * 400 + 50 for x in rng.permutation(N // 400 - 1)]
    pool = []

    def plant(s):
        p = slots.pop()
        g[p:p + len(s)] = s
        return p

    def fresh(L=100):
        return "".join("ACGT"[x] for x in rng.integers(0, 4, L))

    def either(s):
        return s if rng.random() < 0.5 else rc(s)
    # one 1-mismatch copy elsewhere: a survivor of the descent becomes a hit, and gap_shadow runs; the substituted position near
    # either end (inside and outside the first KT symbols of either strand's descent) and in the middle
    for p in (1, 3, 6, 8, 9, 10, 11, 40, 60, 88, 89, 90, 91, 93, 96, 98):
        s = fresh()
        plant(s)
        plant(sub(s, p, 1 + p % 3))
        pool.append(("mm1", either(s)))
    # two such copies, substituted at different positions, or at the same one with different symbols
    for p, q in ((2, 97), (95, 97), (2, 5), (5, 5), (96, 96), (50, 94), (7, 93), (93, 93)):
        s = fresh()
        plant(s)
        plant(sub(s, p, 1))
        plant(sub(s, q, 2))
        pool.append(("mm2", either(s)))
    # the win_hi = ldp - 1 case: a child stored landed, pruned at its pop (bwtgap.c:156) by a bound that gap_shadow raised after the
    # child was created.  gap_shadow raises the bound at a position only where the hit's interval holds EVERY occurrence of the
    # read's symbols up to there, so a second real copy is never pruned by the first one's hit, and on the strand of the exact
    # occurrence no bound is ever raised (the exact copy is counted too).  What is pruned is a child that is not a copy: here the
    # read's other strand has ONE 1-mismatch copy, substituted at p with symbol j, and the two other symbols at p occur with enough
    # of the read around them (a decoy of 28 bases) to survive the descent to table depth -- they are popped after the copy's hit
    # where the copy's child was pushed after them.  NOTE what these reads do and do not show: such a child dies in its exact tail
    # if it is not pruned at its pop, without a hit or a push, so rows, n_aln and max_entries are the same whichever bound the pop
    # reads.  The pop-time bound of a landed entry follows the reference for fidelity and has no observable effect; these reads
    # check that landed entries next to a raised bound leave the answer alone, not that the GPU pop read that bound
    for p in (4, 6, 8, 92, 94, 96):
        for j in (1, 2, 3):
            s = fresh()
            t = rc(s)
            plant(s)
            plant(sub(t, p, j))
            for j2 in (1, 2, 3):
                if j2 != j:
                    plant(sub(t, p, j2)[max(0, p - 14):p + 14])
            pool.append(("prune", either(s)))
    # both strands occur: a reverse-complement palindrome, and a read whose reverse complement is planted too
    for _ in range(4):
        h = fresh(50)
        s = h + rc(h)
        plant(s)
        pool.append(("both", s))
        s = fresh()
        plant(s)
        plant(rc(s))
        plant(sub(s, 94, 1))
        pool.append(("both", either(s)))
    # repeats: more than max_top2 = 30 exact copies (the search ends at the first sub-optimal hit), and more than 16 hit rows (kernel D)
    s = fresh()
    for _ in range(40):
        plant(s)
    for p in (4, 93):
        plant(sub(s, p, 1))
    pool += [("top2", s), ("top2", rc(s))]
    s = fresh()
    plant(s)
    for p in range(3, 98, 5):
        plant(sub(s, p, 1 + p % 3))
    pool += [("cap16", s), ("cap16", rc(s))]
    G = "".join(g)

    def cut(L):
        p = int(rng.integers(0, N - L))
        return either(G[p:p + L])
    pool += [("exact", cut(100)) for _ in range(24)]
    for L in (KT - 1, KT, KT + 1, KT + 2, 32, 33, 89, 90, 91):
        pool += [("len%d" % L, cut(L)) for _ in range(4)]
    pool += [("err", mutate(rng, cut(100), 0.02, 0.3)[:100].ljust(100, "A")) for _ in range(16)]
    pool += [("junk", fresh()) for _ in range(8)]
    pool += [("nrich", mutate(rng, cut(100), 0.0, 0.0, 0.08)) for _ in range(8)]
    for p in (0, 50, 99):                    # never exact: an N restarts both strands' width passes
        s = cut(100)
        pool.append(("oneN", s[:p] + "N" + s[p + 1:]))
    return G, pool


class World:
    pass


@pytest.fixture(scope="module")
def world():
    olib = T.load_oracle()
    rng = np.random.default_rng(20261018)
    G, pool = make_world(rng)
    w = World()
    w.kinds, w.reads = [k for k, _ in pool], [s for _, s in pool]
    codes = np.frombuffer(G.encode().translate(bytes.maketrans(b"ACGT", bytes(range(4)))), np.uint8)
    w.d_text = synth.DevArray.from_host(codes)
    w.parts = [synth.build_index(w.d_text, N, rev, 32, True) for rev in (0, 1)]
    w.ix = nabwa.Index.from_arrays((w.parts[0][0].ptr, w.parts[0][1]), (w.parts[1][0].ptr, w.parts[1][1]),
                                   (w.parts[0][2].ptr, w.parts[0][3]), (w.parts[1][2].ptr, w.parts[1][3]), device_ptrs=True)
    w.h = [w.parts[q][0].to_host(np.uint32, w.parts[q][1]) for q in (0, 1)]
    w.oh = olib.orc_index_wrap(T.ptr(w.h[0]), len(w.h[0]), T.ptr(w.h[1]), len(w.h[1]))
    w.orc = Oracle(olib, w.oh, w.reads)
    w.olib = olib
    yield w
    w.ix.close()
    olib.orc_index_free(w.oh)
    for p in w.parts:
        p[0].free()
        p[2].free()
    w.d_text.free()


def of(w, *kinds):
    return [i for i, k in enumerate(w.kinds) if k in kinds]


def block(name):
    o = T.default_opt()
    o.max_entries = 20000
    if name == "N":                          # aln -N
        o.mode |= 0x10
    elif name == "O2M3":                     # aln -O 2 -M 3: a gap open is no dearer than a mismatch
        o.s_gapo, o.s_mm = 2, 3
    elif name in ("n0", "n1"):               # aln -n 0 / -n 1
        o.fnr, o.max_diff = 0.0, int(name[1])
    elif name.startswith("me"):              # max_entries: the bwtgap.c:140 cut-off
        o.max_entries = int(name[2:])
    else:
        assert name == "default"
    return o


def run_levels(w, monkeypatch, name, ids, what):
    """the batch under NABWA_SURE0 = 0, 1, 2, each against the oracle -> the counters per level"""
    o = block(name)
    monkeypatch.setenv("NABWA_SURE0_STATS", "1")
    stats = {}
    for lv in LEVELS:
        monkeypatch.setenv("NABWA_SURE0", str(lv))
        b = nabwa.Batch(w.ix, gap_opt(o), *encode([w.reads[i] for i in ids]))
        try:
            b.run()
            n2 = b.sync()
            got, maxe = collect(b)
            stats[lv] = b.sure0_stats()
            cfg = b.config()
        finally:
            b.close()
        print("%s, NABWA_SURE0=%d: %d reads (class 0: %d), %d to kernel D, counters %s" % (what, lv, len(ids), cfg["cls"][0], n2, stats[lv]))
        check(w.orc, name, o, False, ids, got, maxe, "%s, NABWA_SURE0=%d" % (what, lv))
    assert stats[0] == [0, 0, 0, 0], stats
    assert stats[1][3] == 0 and stats[2][3] == 0, "the safety net handed reads to kernel D: %s" % stats
    assert stats[1][2] == 0, stats           # setting 1 stores nothing landed
    return stats, cfg


def assert_ran(stats, landed=True):
    assert stats[1][0] > 0 and stats[1][0] == stats[2][0], stats
    assert stats[1][1] > 0 and stats[2][1] == stats[1][1], stats      # the same children die under either setting
    if landed:
        assert stats[2][2] > 0, stats


def assert_off(stats):
    assert stats[1] == [0, 0, 0, 0] and stats[2] == [0, 0, 0, 0], stats


def test_world_holds_what_the_cases_need(world):
    """the oracle's own answers: the planted copies are found, and the reference really prunes in the prune3 reads"""
    o = block("default")
    ids = list(range(len(world.reads)))
    want = dict(zip(ids, world.orc.want("default", o, False, ids)))

    def rows(i):
        return np.frombuffer(want[i][0], T.ALN_DT)
    for i in of(world, "exact", "mm1", "mm2", "prune", "both", "top2", "cap16"):
        r = rows(i)
        assert len(r) and int(r[0]["score"]) == 0, (world.kinds[i], i)
    assert all(len(rows(i)) == 2 and int(rows(i)[1]["score"]) == o.s_mm for i in of(world, "mm1"))
    assert all(len(rows(i)) == 3 for i in of(world, "mm2"))
    assert all(len(rows(i)) >= 2 for i in of(world, "both"))
    assert all(len(rows(i)) == 2 and int(rows(i)[1]["score"]) == o.s_mm for i in of(world, "prune"))
    # the reference prunes in the prune reads: on the strand of the copy the width pass restarts once, at the substituted position q;
    # the symbols below q occur once (width 1 = the copy's interval), so the copy's hit sets the bound at q - 1 to 1 (gap_shadow),
    # and a child created at q that is popped afterwards, with m == 0, fails bwtgap.c:156.  q above len - KT: created in key form
    world.olib.orc_cal_width.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    ow, ob, n_key = np.zeros(101, np.uint32), np.zeros(101, np.int32), 0
    for i in of(world, "prune"):
        seq, rseq, off = encode([world.reads[i]])
        qs = []
        for x, arr in ((0, seq), (1, rseq)):
            world.olib.orc_cal_width(C.c_void_p(world.oh + x * T.OracleIndex.BWT_SIZE), 100, T.ptr(np.ascontiguousarray(arr)), T.ptr(ow), T.ptr(ob))
            if ob[99] == 1:
                q = int(np.argmax(ob[:100] == 1))
                qs.append(q)
                if q > 16:
                    assert ow[q - 1] == 1, (i, x, q, ow[:q])
                    n_key += q > 100 - KT
            else:
                assert ob[99] == 0, (i, x)
        assert len(qs) == 1, (i, qs)
    assert n_key >= 6, n_key
    assert all(len(rows(i)) > 16 for i in of(world, "cap16"))
    assert all(int((rows(i)["l"].astype(np.int64) - rows(i)["k"] + 1)[0]) == 40 and len(rows(i)) == 1 for i in of(world, "top2"))     # (ended at the first sub-optimal hit)
    assert all(len(rows(i)) == 0 or int(rows(i)[0]["score"]) > 0 for i in of(world, "junk", "nrich", "oneN"))


@pytest.mark.parametrize("kind", ["exact", "mm1", "mm2", "prune", "both", "top2", "cap16"])
def test_each_kind_of_exact_read(world, monkeypatch, kind):
    """100 bp reads that occur exactly, a batch per kind (equal lengths: lockstep waves)"""
    ids = of(world, kind)
    stats, cfg = run_levels(world, monkeypatch, "default", ids, kind)
    assert cfg["w_sync"] == 1 and cfg["cls"][0] == len(ids), cfg
    assert stats[1][0] == len(ids), stats
    assert_ran(stats)


def test_lengths(world, monkeypatch):
    """KT - 1 .. KT + 2 (no key up to KT: nothing to resolve), seed_len and seed_len + 1, 89 / 90 / 91, in one batch of mixed
    lengths; then each length alone"""
    kinds = ["len%d" % L for L in (KT - 1, KT, KT + 1, KT + 2, 32, 33, 89, 90, 91)]
    stats, cfg = run_levels(world, monkeypatch, "default", of(world, *kinds), "lengths")
    assert cfg["w_sync"] == 0
    assert_ran(stats)
    for k in kinds:
        stats, cfg = run_levels(world, monkeypatch, "default", of(world, k), k)
        assert cfg["w_sync"] == 1
        # the table depth KT is the index's own choice (from the genome's size): the lengths straddle it only if reads up to KT, which
        # have no key, resolve nothing, and reads from KT + 1 on do, dead children and landed ones
        if int(k[3:]) <= KT:
            assert stats[1][0] > 0 and stats[1][1:] == [0, 0, 0] and stats[2][1:] == [0, 0, 0], (k, stats)
        else:
            assert stats[1][0] > 0 and stats[1][1] > 0 and stats[2][1] == stats[1][1] and stats[2][2] > 0, (k, stats)


def test_mixed_batches(world, monkeypatch):
    """class-0 reads among 2 %-error reads, junk and N-rich reads: every 100 bp read in one batch (lockstep), and the whole pool
    (mixed lengths: none)"""
    ids = [i for i in range(len(world.reads)) if len(world.reads[i]) == 100]
    rng = np.random.default_rng(5)
    ids = [int(i) for i in rng.permutation(ids)]
    stats, cfg = run_levels(world, monkeypatch, "default", ids, "all 100 bp reads")
    assert cfg["w_sync"] == 1 and 0 < cfg["cls"][0] < len(ids), cfg
    assert stats[1][0] == cfg["cls"][0], (stats, cfg)             # exactly kernel W's class 0 takes the shortcut
    assert_ran(stats)
    ids = [int(i) for i in rng.permutation(len(world.reads))]
    stats, cfg = run_levels(world, monkeypatch, "default", ids, "whole pool")
    assert cfg["w_sync"] == 0
    assert stats[1][0] == cfg["cls"][0], (stats, cfg)
    assert_ran(stats)


def test_n_rich_reads_never_take_it(world, monkeypatch):
    ids = of(world, "nrich", "oneN", "junk")
    stats, cfg = run_levels(world, monkeypatch, "default", ids, "N-rich and junk")
    assert cfg["cls"][0] == 0, cfg
    assert_off(stats)


@pytest.mark.parametrize("name", ["N", "O2M3", "n0"])
def test_option_blocks_where_it_stays_off(world, monkeypatch, name):
    ids = of(world, "exact")[:8] + of(world, "mm1")[:4] + of(world, "prune")[:4] + of(world, "err")[:4]
    stats, cfg = run_levels(world, monkeypatch, name, ids, "block " + name)
    assert cfg["cls"][0] >= 16, cfg
    assert_off(stats)


def test_smallest_max_diff(world, monkeypatch):
    """aln -n 1: on, with max_diff 1 from the start"""
    ids = of(world, "exact", "mm1", "mm2", "prune", "both") + of(world, "err")[:8]
    stats, cfg = run_levels(world, monkeypatch, "n1", ids, "block n1")
    assert_ran(stats)


@pytest.mark.parametrize("me,on", [(40, False), (200, False), (450, True), (20000, True)])
def test_entry_cut_off(world, monkeypatch, me, on):
    """max_entries 40 and 200: the search stops at the cut-off (bwtgap.c:140), and the guard keeps the flag off from the start
    (2 + 4 * 100 entries are more); 450: on at the start and dropped on the way down; 20000: never in reach"""
    ids = of(world, "exact", "mm1", "mm2", "prune", "both", "top2")
    stats, cfg = run_levels(world, monkeypatch, "me%d" % me, ids, "max_entries %d" % me)
    if not on:
        assert_off(stats)
    else:
        assert stats[1][0] == len(ids) and stats[1][1] > 0, stats
        if me == 20000:
            assert_ran(stats)
    if me <= 200:                            # the cut-off really fired: the reference counted more entries than it allows
        want = world.orc.want("me%d" % me, block("me%d" % me), False, ids)
        assert max(m for _, m in want) > me, sorted(m for _, m in want)
