"""Kernel S's leap (NABWA_SURE0=3): a text-form entry that is the read's own prefix on a strand kernel W proved to occur
is replaced by its hit, and the entries the levels in between would have pushed are counted in closed form.  It must change speed
only.  The small genome of test_gpu_sure0 (KT = 10); every read of every batch is compared with the CPU oracle under NABWA_SURE0 = 2
and 3: the hit count, every row and max_entries -- max_entries is where a wrong closed-form count shows.  The counters of
nabwa_batch_sure0_stats_ex say that the leap ran where it should and nowhere else, that no proven entry had to fall back to the
walk, and that the safety net never fired."""
import importlib

import numpy as np
import pytest

import nabwa_testlib as T
from test_gpu_batch_mix import check, collect, encode, gap_opt
from test_gpu_sure0 import KT, N, make_world, of, rc, world  # noqa: F401  (world: the module-scoped fixture, built once for this file too)

pytestmark = pytest.mark.gpu
nabwa = importlib.import_module("network-aware-bwa_amd")

EXACT_KINDS = ("exact", "mm1", "mm2", "prune", "both", "cap16")     # 100 bp, class 0, one row before the read ends
LENS = (KT - 1, KT, KT + 1, KT + 2, 32, 33, 89, 90, 91)


def lblock(name):
    """option blocks of this file (names of its own: the oracle cache is keyed by name)"""
    o = T.default_opt()
    o.max_entries = 20000
    kind, _, v = name[3:].partition("=")
    assert name.startswith("lp_")
    if kind == "ies":
        o.indel_end_skip = int(v)
    elif kind == "seed":
        o.seed_len = int(v)
    elif kind == "msd":
        o.max_seed_diff = int(v)
    elif kind == "gapo":
        o.max_gapo = int(v)
    elif kind == "gape":
        o.max_gape = int(v)
    elif kind == "loggap":
        o.mode |= 0x04
    elif kind == "n":                         # aln -n 0 / 1 / 2
        o.fnr, o.max_diff = 0.0, int(v)
    elif kind == "me":                        # the bwtgap.c:140 cut-off
        o.max_entries = int(v)
    elif kind == "N":                         # aln -N
        o.mode |= 0x10
    elif kind == "O2M3":                      # a gap open no dearer than a mismatch
        o.s_gapo, o.s_mm = 2, 3
    else:
        assert kind == "default", name
    return o


@pytest.fixture(scope="module")
def edges(world):
    """the first and the last 100 bases of the genome, as given and reverse-complemented, added to this module's pool: one index's
    start is the other's end (text position 0, and the k >= levels-left guard)"""
    G, _ = make_world(np.random.default_rng(20261018))
    assert len(G) == N
    first = len(world.reads)
    for s in (G[:100], rc(G[:100]), G[-100:], rc(G[-100:])):
        world.reads.append(s)
        world.kinds.append("edge")
    return list(range(first, first + 4))


def run23(w, monkeypatch, name, ids, what, per_read=False):
    """the batch under NABWA_SURE0 = 2 and 3, each against the oracle -> ({setting: the eight counters}, config)"""
    o = lblock(name)
    monkeypatch.setenv("NABWA_SURE0_STATS", "1")
    stats = {}
    for lv in (2, 3):
        monkeypatch.setenv("NABWA_SURE0", str(lv))
        b = nabwa.Batch(w.ix, gap_opt(o), *encode([w.reads[i] for i in ids]), per_read=per_read)
        try:
            b.run()
            n2 = b.sync()
            got, maxe = collect(b)
            stats[lv] = b.sure0_stats_ex()
            assert stats[lv][:4] == b.sure0_stats()
            cfg = b.config()
        finally:
            b.close()
        print("%s, NABWA_SURE0=%d: %d reads (class 0: %d), %d to kernel D, counters %s" % (what, lv, len(ids), cfg["cls"][0], n2, stats[lv]))
        check(w.orc, name, o, per_read, ids, got, maxe, "%s, NABWA_SURE0=%d" % (what, lv))
    for lv in (2, 3):
        assert stats[lv][3] == 0, "the safety net handed reads to kernel D: %s" % stats
        assert stats[lv][6] == 0 and stats[lv][7] == 0, "a proven entry fell back to the walk: %s" % stats
    assert stats[2][4:] == [0, 0, 0, 0], stats                     # setting 2 never leaps
    assert stats[3][:4] == stats[2][:4], stats                     # the leap leaves the key-form shortcut alone
    assert (stats[3][4] > 0) == (stats[3][5] > 0), stats
    return stats, cfg


@pytest.mark.parametrize("kind", EXACT_KINDS + ("top2",))
def test_each_kind_of_exact_read(world, monkeypatch, kind):
    ids = of(world, kind)
    stats, cfg = run23(world, monkeypatch, "lp_default", ids, kind)
    assert cfg["w_sync"] == 1 and cfg["cls"][0] == len(ids), cfg
    if kind == "top2":                        # 40 copies: the interval is never one row, so never text form
        assert stats[3][4] == 0, stats
    elif kind == "both":                      # each strand occurs and is alone in the genome: one leap per strand
        assert stats[3][4] == 2 * len(ids), stats
    else:
        assert stats[3][4] >= len(ids), stats
    # text form is entered below table depth, by the child of a one-row expansion: at most len - KT - 1 levels are left
    assert stats[3][5] <= stats[3][4] * (100 - KT - 1), stats


def test_lengths(world, monkeypatch):
    """KT - 1 .. KT + 2 (no text-form stretch, or 1 - 2 levels), either side of seed_len, 89 - 91: mixed in one batch (lanes are
    refilled one by one), then each length alone (lockstep waves)"""
    kinds = ["len%d" % L for L in LENS]
    stats, cfg = run23(world, monkeypatch, "lp_default", of(world, *kinds), "lengths")
    assert cfg["w_sync"] == 0
    assert stats[3][4] > 0, stats
    for L in LENS:
        ids = of(world, "len%d" % L)
        stats, cfg = run23(world, monkeypatch, "lp_default", ids, "len%d" % L)
        assert cfg["w_sync"] == 1
        if L <= KT + 1:                       # key form down to the read's end, or the one text-form child is the hit itself
            assert stats[3][4] == 0, (L, stats)
        else:
            assert stats[3][5] <= stats[3][4] * (L - KT - 1), (L, stats)
        if L >= 32:                           # a 32-mer of this genome is alone: one row long before the read ends
            assert stats[3][4] >= len(ids), (L, stats)


ON_BLOCKS = ["lp_ies=0", "lp_ies=1", "lp_ies=5", "lp_ies=60", "lp_seed=20", "lp_seed=32", "lp_seed=200", "lp_msd=0", "lp_msd=1", "lp_msd=2",
             "lp_gapo=0", "lp_gapo=1", "lp_gape=0", "lp_loggap", "lp_n=1", "lp_n=2", "lp_me=450", "lp_me=20000"]


@pytest.mark.parametrize("name", ON_BLOCKS + ["lp_N", "lp_O2M3", "lp_n=0"])
def test_option_blocks(world, monkeypatch, name):
    """every option the closed-form count of gap children reads, at values on either side of where it changes the count"""
    ids = of(world, "exact")[:8] + of(world, "mm1")[:4] + of(world, "both")[:4] + of(world, "prune")[:2] + of(world, "err")[:4]
    ids += of(world, "len%d" % (KT + 2), "len32", "len33", "len89", "len91")
    stats, cfg = run23(world, monkeypatch, name, ids, "block " + name)
    assert cfg["cls"][0] >= 18, cfg
    if name not in ON_BLOCKS:                 # the shortcut's own preconditions fail: no flag, no leap
        assert stats[3] == [0] * 8, stats
    elif name == "lp_me=450":                 # the flag is on at the start and dropped on the way down (2 + 4 * len entries in reach of the cut-off): no leap after that
        assert stats[3][0] > 0, stats
    else:
        assert stats[3][4] >= 18, stats


def test_text_edges(world, edges, monkeypatch):
    stats, cfg = run23(world, monkeypatch, "lp_default", edges, "text edges")
    assert cfg["cls"][0] == 4, cfg
    assert stats[3][4] >= 4, stats


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_batch_sizes(world, monkeypatch, n):
    """whole waves, one read more and one fewer, all class 0; then with 2 %-error reads shuffled in (chunks of the work order
    straddle the class boundary)"""
    c0 = of(world, *EXACT_KINDS)
    ids = (c0 * (n // len(c0) + 1))[:n]
    stats, cfg = run23(world, monkeypatch, "lp_default", ids, "%d class-0 reads" % n)
    assert cfg["cls"][0] == n, cfg
    assert stats[3][4] >= n, stats
    rng = np.random.default_rng(n)
    mixed = [int(i) for i in rng.permutation(ids + of(world, "err"))]
    stats, cfg = run23(world, monkeypatch, "lp_default", mixed, "%d class-0 reads among 2 %%-error reads" % n)
    assert n <= cfg["cls"][0] < len(mixed), cfg
    assert stats[3][4] >= n, stats


@pytest.mark.parametrize("per_read", [False, True])
def test_whole_pool(world, edges, monkeypatch, per_read):
    """every read of the pool, mixed lengths and classes, with max_diff by the batch's longest read and by each read's own length"""
    ids = [int(i) for i in np.random.default_rng(7).permutation(len(world.reads))]
    stats, cfg = run23(world, monkeypatch, "lp_default", ids, "whole pool, per_read=%s" % per_read, per_read)
    assert cfg["w_sync"] == 0 and stats[3][0] == cfg["cls"][0], (stats, cfg)
    assert stats[3][4] >= len(of(world, *EXACT_KINDS)), stats
