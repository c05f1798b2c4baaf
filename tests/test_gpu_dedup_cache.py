"""NABWA_DEDUP_CACHE=<MiB>: the index remembers the reads its batches searched, and a later batch takes a read it finds there without searching
it.  What the caller sees must be byte for byte what it sees with the variable unset.  Every case runs the same calls unset and set and compares
fetch_flat() (counts, rows, max_entries) and checksum(); where the oracle is at hand the rows are the oracle's too; and every case asserts,
through dedup_stats_ex(), exactly how many reads were searched and how many were served -- a case cannot pass with the cache silently off."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import dedup_cases as D
import nabwa_testlib as T
import test_gpu_batch_mix as M

pytestmark = pytest.mark.gpu
nabwa = importlib.import_module("network-aware-bwa_amd")
ENV = ("NABWA_DEDUP", "NABWA_DEDUP_HASH_BITS", "NABWA_DEDUP_CACHE", "NABWA_DEDUP_CACHE_ROWS")
ROW_CAP = 1024            # NABWA_DEDUP_CACHE_ROWS' default: reads with more rows are not entered


# ---------------------------------------------------------------------------------------------------------------- running a batch
def unset(mp):
    for v in ENV:
        mp.delenv(v, raising=False)


def switch_on(mp, mib=64, bits=None, rows=None):
    mp.setenv("NABWA_DEDUP", "1")
    mp.setenv("NABWA_DEDUP_CACHE", str(mib))
    if bits is not None:
        mp.setenv("NABWA_DEDUP_HASH_BITS", str(bits))
    if rows is not None:
        mp.setenv("NABWA_DEDUP_CACHE_ROWS", str(rows))


def run_batch(ix, o, seq, rseq, off, per_read=False):
    b = nabwa.Batch(ix, M.gap_opt(o), seq, rseq, off, per_read=per_read)
    try:
        b.run()
        n2 = b.sync()
        n_aln, rows, maxe = b.fetch_flat()
        cks = b.checksum()
        assert cks == M.host_checksum(n_aln, rows)
        return dict(n_aln=n_aln.copy(), rows=rows.tobytes(), maxe=maxe.copy(), cks=cks, n2=n2, cfg=b.config(), st=b.dedup_stats_ex())
    finally:
        b.close()


def plain(mp, ix, o, seq, rseq, off, per_read=False):
    unset(mp)
    r = run_batch(ix, o, seq, rseq, off, per_read)
    n = len(off) - 1
    assert r["st"] == [n, n, 0, 0, 0, 0, 0, 0]
    return r


def cached(mp, ix, o, seq, rseq, off, per_read=False, **kw):
    switch_on(mp, **kw)
    r = run_batch(ix, o, seq, rseq, off, per_read)
    unset(mp)
    assert r["st"][0] == len(off) - 1 and r["st"][3] == 1
    return r


def same(a, b, what=""):
    assert np.array_equal(a["n_aln"], b["n_aln"]), what
    assert np.array_equal(a["maxe"], b["maxe"]), what
    assert a["rows"] == b["rows"], what
    assert a["cks"] == b["cks"], what
    for f in ("n", "min_len", "max_len", "deep_only"):
        assert a["cfg"][f] == b["cfg"][f], (what, f)


def searched_served(r):
    return r["st"][1], r["st"][4]


def per_read_rows(res):
    bnd = np.concatenate([[0], np.cumsum(res["n_aln"])]) * 16
    return [res["rows"][bnd[i]:bnd[i + 1]] for i in range(len(res["n_aln"]))]


def rows_by_key(res, seq, rseq, off):
    """distinct read -> its row count, from a run with everything unset"""
    return {k: int(res["n_aln"][i]) for i, k in enumerate(D.keys_of(seq, rseq, off))}


# ---------------------------------------------------------------------------------------------------------------- fixtures
class World:
    pass


@pytest.fixture(scope="module")
def toy():
    w = World()
    w.olib = T.load_oracle()
    w.oix = T.OracleIndex(w.olib)
    w.kinds, w.reads = D.mixed_pool()
    w.orc = M.Oracle(w.olib, w.oix.h, w.reads)
    w.ix = nabwa.Index.load(T.TOY, 0, True, True)
    w.of = lambda *kinds: [i for i, k in enumerate(w.kinds) if k in kinds]
    yield w
    w.ix.close()


@pytest.fixture
def fresh_ix():
    """an index of its own: the cache's size is fixed by the first batch that asks for one"""
    ix = nabwa.Index.load(T.TOY, 0, True, True)
    yield ix
    ix.close()


@pytest.fixture
def cold(toy, monkeypatch):
    """the module's index with an empty cache, and the environment without the switches"""
    unset(monkeypatch)
    toy.ix.dedup_cache_clear()
    return toy


def enc(toy, ids):
    return M.encode([toy.reads[i] for i in ids])


def random_reads(n, L, seed):
    """n different reads of L random bases, as text"""
    rng = np.random.default_rng(seed)
    out = set()
    while len(out) < n:
        out.add("".join("ACGT"[x] for x in rng.integers(0, 4, L)))
    return sorted(out)


# ---------------------------------------------------------------------------------------------------------------- 1. replay
@pytest.mark.parametrize("per_read", [False, True])
@pytest.mark.parametrize("name", ["default", "adna", "n3"])
def test_replay_serves_every_read_and_a_cleared_cache_none(cold, monkeypatch, name, per_read):
    """the mixed batch of tests/test_gpu_dedup.py twice on one index: the second run searches nothing; after dedup_cache_clear everything again"""
    toy, o = cold, M.opt_block(name)
    ids = D.mixed_batch(len(toy.reads))
    seq, rseq, off = enc(toy, ids)
    n_d = len(toy.reads)
    off_ = plain(monkeypatch, toy.ix, o, seq, rseq, off, per_read)
    assert max(rows_by_key(off_, seq, rseq, off).values()) <= ROW_CAP          # every read of the pool can be entered
    first = cached(monkeypatch, toy.ix, o, seq, rseq, off, per_read)
    same(off_, first, "first run")
    assert first["st"] == [len(ids), n_d, 0, 1, 0, n_d, 0, 0]
    second = cached(monkeypatch, toy.ix, o, seq, rseq, off, per_read)
    same(off_, second, "replay")
    assert second["st"] == [len(ids), 0, 0, 1, n_d, 0, 0, 0]
    assert second["n2"] == 0 and second["cfg"]["cls"] == [-1, -1, -1]          # nothing ran: the diagnostics speak of the reads searched
    M.check(toy.orc, name, o, per_read, ids, per_read_rows(second), second["maxe"], "replay, %s" % name)
    cs = toy.ix.dedup_cache_stats()
    assert cs[2] == n_d and 0 < cs[1] <= cs[0] <= 64 << 20 and cs[3] >= 1024
    toy.ix.dedup_cache_clear()
    assert toy.ix.dedup_cache_stats()[1:3] == [0, 0]
    third = cached(monkeypatch, toy.ix, o, seq, rseq, off, per_read)
    same(off_, third, "after clear")
    assert third["st"] == [len(ids), n_d, 0, 1, 0, n_d, 0, 0]


# ---------------------------------------------------------------------------------------------------------------- 2. smallest shapes
def test_smallest_shapes(cold, monkeypatch):
    toy, o = cold, M.opt_block("default")
    known = toy.of("err100")[:10]
    new = toy.of("exact100")[:3]
    a = known[0]
    # one read, then the same read
    r = cached(monkeypatch, toy.ix, o, *enc(toy, [a]))
    assert r["st"] == [1, 1, 0, 1, 0, 1, 0, 0]
    r = cached(monkeypatch, toy.ix, o, *enc(toy, [a]))
    assert r["st"] == [1, 0, 0, 1, 1, 0, 0, 0]
    same(plain(monkeypatch, toy.ix, o, *enc(toy, [a])), r, "one read, served")
    # no read, with a warm cache
    empty = (np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(1, np.int64))
    r = cached(monkeypatch, toy.ix, o, *empty)
    assert r["st"] == [0, 0, 0, 1, 0, 0, 0, 0]
    same(plain(monkeypatch, toy.ix, o, *empty), r, "n = 0")
    # two equal reads: merged in the batch, then served
    r = cached(monkeypatch, toy.ix, o, *enc(toy, [a, a]))
    assert r["st"] == [2, 0, 0, 1, 1, 0, 0, 0] and r["n_aln"][0] == r["n_aln"][1]
    same(plain(monkeypatch, toy.ix, o, *enc(toy, [a, a])), r, "two equal reads")
    # exactly one new read, first, in the middle and last
    r = cached(monkeypatch, toy.ix, o, *enc(toy, known))
    assert searched_served(r) == (len(known) - 1, 1)
    for x, ids in zip(new, ([new[0]] + known, known[:5] + [new[1]] + known[5:], known + [new[2]])):
        r = cached(monkeypatch, toy.ix, o, *enc(toy, ids))
        assert r["st"] == [len(ids), 1, 0, 1, len(known), 1, 0, 0], ids.index(x)
        same(plain(monkeypatch, toy.ix, o, *enc(toy, ids)), r, "one new read at %d" % ids.index(x))
        M.check(toy.orc, "default", o, False, ids, per_read_rows(r), r["maxe"], "one new read")


# ---------------------------------------------------------------------------------------------------------------- 3. half known, half new
@pytest.mark.parametrize("name", ["default", "adna"])
def test_half_known_half_new_in_shuffled_order(cold, monkeypatch, name):
    toy, o = cold, M.opt_block(name)
    rng = np.random.default_rng(31)
    pool = [int(i) for i in rng.permutation(len(toy.reads))]
    A, B = pool[: len(pool) // 2], pool[len(pool) // 2:]
    r = cached(monkeypatch, toy.ix, o, *enc(toy, A))
    assert r["st"][1] == r["st"][5] == len(A)
    ids = [int(i) for i in rng.permutation(A + B + A[:50] + B[:50])]
    seq, rseq, off = enc(toy, ids)
    r = cached(monkeypatch, toy.ix, o, seq, rseq, off)
    assert r["st"] == [len(ids), len(B), 0, 1, len(A), len(B), 0, 0]
    same(plain(monkeypatch, toy.ix, o, seq, rseq, off), r, "half and half")
    M.check(toy.orc, name, o, False, ids, per_read_rows(r), r["maxe"], "half and half, %s" % name)


# ---------------------------------------------------------------------------------------------------------------- 4. near misses
def test_near_misses_are_not_served(cold, monkeypatch):
    """the cache holds, for each length around the chunk boundaries, one read at an odd byte offset.  Then the near_duplicates() batch: the same
    seq under another rseq, the one-base extension (the cached read is its prefix), the reads with only the first and only the last byte changed
    are searched; the read itself and its copy are served"""
    toy, o = cold, M.opt_block("default")
    seq, rseq, off = D.near_duplicates()
    assert {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 257} <= set(D.NEAR_LENS)
    base = [7 * g + 1 for g in range(len(D.NEAR_LENS))]
    bs = np.concatenate([seq[off[i]:off[i + 1]] for i in base]); br = np.concatenate([rseq[off[i]:off[i + 1]] for i in base])
    boff = np.concatenate([[0], np.cumsum([off[i + 1] - off[i] for i in base])]).astype(np.int64)
    warm = cached(monkeypatch, toy.ix, o, bs, br, boff)
    assert warm["st"] == [len(base), len(base), 0, 1, 0, len(base), 0, 0]
    keys, held = set(D.keys_of(seq, rseq, off)), set(D.keys_of(bs, br, boff))
    assert held <= keys and len(held) == len(base)
    r = cached(monkeypatch, toy.ix, o, seq, rseq, off)
    assert r["st"] == [len(off) - 1, len(keys) - len(held), 0, 1, len(held), len(keys) - len(held), 0, 0]
    same(plain(monkeypatch, toy.ix, o, seq, rseq, off), r, "near misses")


# ---------------------------------------------------------------------------------------------------------------- 5. effective options
def test_another_option_block_flushes_or_bypasses(cold, monkeypatch):
    toy = cold
    oa, ob = M.opt_block("default"), M.opt_block("n3")
    ids = toy.of("err100", "adna")[:60]
    seq, rseq, off = enc(toy, ids)
    pa, pb = plain(monkeypatch, toy.ix, oa, seq, rseq, off), plain(monkeypatch, toy.ix, ob, seq, rseq, off)
    f0, b0 = toy.ix.dedup_cache_stats()[6:8]
    # A, B, A with no batch alive in between: each change of block empties the cache
    for k, (o, want) in enumerate(((oa, pa), (ob, pb), (oa, pa))):
        r = cached(monkeypatch, toy.ix, o, seq, rseq, off)
        same(want, r, "flush %d" % k)
        assert r["st"] == [len(ids), len(ids), 0, 1, 0, len(ids), 0, 0]
        assert toy.ix.dedup_cache_stats()[6:8] == [f0 + k, b0] and toy.ix.dedup_cache_stats()[2] == len(ids)
    # a batch of A alive, holding served reads: B goes without the cache, and the cache cannot be cleared
    switch_on(monkeypatch)
    held = nabwa.Batch(toy.ix, M.gap_opt(oa), seq, rseq, off)
    try:
        assert held.dedup_stats_ex()[4] == len(ids)
        r = cached(monkeypatch, toy.ix, ob, seq, rseq, off)
        same(pb, r, "bypass")
        assert r["st"] == [len(ids), len(ids), 0, 1, 0, 0, 0, 1]
        assert toy.ix.dedup_cache_stats()[6:8] == [f0 + 2, b0 + 1] and toy.ix.dedup_cache_stats()[2] == len(ids)
        with pytest.raises(nabwa.NabwaError) as e:
            toy.ix.dedup_cache_clear()
        assert e.value.code == nabwa.EINVAL
        held.run()
        held.sync()
        got, maxe = M.collect(held)
        M.check(toy.orc, "default", oa, False, ids, got, maxe, "the held batch")
    finally:
        held.close()
    toy.ix.dedup_cache_clear()


def test_per_read_0_a_longer_read_changes_the_others_options(cold, monkeypatch):
    """per_read = 0: max_gapo of every read is cut to max_diff of the batch's longest read.  With -o 100 that is what it is: a batch of short reads,
    then the same reads and one of 300 bp -- their entries no longer apply and they are searched again"""
    toy, o = cold, M.opt_block("default")
    o.max_gapo = 100
    short = toy.of("adna")[:40]
    long_ = toy.of("long300")[0]
    max_short = max(len(toy.reads[i]) for i in short)
    assert M.md_of(o, max_short) != M.md_of(o, 300) and len(toy.reads[long_]) == 300
    r = cached(monkeypatch, toy.ix, o, *enc(toy, short))
    assert r["st"] == [len(short), len(short), 0, 1, 0, len(short), 0, 0]
    ids = short + [long_]
    seq, rseq, off = enc(toy, ids)
    want = plain(monkeypatch, toy.ix, o, seq, rseq, off)
    r = cached(monkeypatch, toy.ix, o, seq, rseq, off)
    same(want, r, "with the longer read")
    assert r["st"] == [len(ids), len(ids), 0, 1, 0, len(ids), 0, 0]
    r = cached(monkeypatch, toy.ix, o, seq, rseq, off)
    same(want, r, "with the longer read, again")
    assert r["st"] == [len(ids), 0, 0, 1, len(ids), 0, 0, 0]
    r = cached(monkeypatch, toy.ix, o, *enc(toy, short))                        # and the first batch's entries still answer for the first batch
    assert r["st"] == [len(short), 0, 0, 1, len(short), 0, 0, 0]
    same(plain(monkeypatch, toy.ix, o, *enc(toy, short)), r, "the short reads alone")


# ---------------------------------------------------------------------------------------------------------------- 6. a full cache
def test_full_cache_stops_inserting_and_goes_on_serving(fresh_ix, monkeypatch):
    ix, o = fresh_ix, M.opt_block("default")
    probe = M.encode(random_reads(8, 100, 1))
    r = cached(monkeypatch, ix, o, *probe, mib=1)
    cs = ix.dedup_cache_stats()
    assert r["st"][5] == 8 and cs[2] == 8 and cs[0] <= 1 << 20
    per_entry = cs[1] // cs[2]
    assert per_entry >= 32 + 2 * 112
    n = cs[0] // per_entry + 300                                               # more reads than the whole reservation could hold
    assert n < 6000
    reads = random_reads(n, 100, 2)
    seq, rseq, off = M.encode(reads)
    want = plain(monkeypatch, ix, o, seq, rseq, off)
    first = cached(monkeypatch, ix, o, seq, rseq, off, mib=1)
    same(want, first, "filling")
    g, s, _, _, served, ins, not_ins, byp = first["st"]
    assert (g, s, served, byp) == (n, n, 0, 0) and ins + not_ins == n and 0 < ins < n
    cs = ix.dedup_cache_stats()
    assert cs[2] == 8 + ins and cs[1] <= cs[0] <= 1 << 20
    second = cached(monkeypatch, ix, o, seq, rseq, off, mib=1)
    same(want, second, "full")
    assert second["st"] == [n, n - ins, 0, 1, ins, 0, n - ins, 0]
    assert ix.dedup_cache_stats()[1:3] == cs[1:3]


# ---------------------------------------------------------------------------------------------------------------- 7. collisions
@pytest.mark.parametrize("bits", [0, 1, 4])
def test_narrow_probe_keys_fill_their_chains_and_the_rest_is_searched(cold, monkeypatch, bits):
    """NABWA_DEDUP_HASH_BITS narrows the key the table is probed by: 2^bits chains of at most 16 entries.  (It also narrows the in-batch stage's key,
    which then merges fewer reads: equal reads may reach the cache, and are served by one entry.)"""
    toy, o = cold, M.opt_block("default")
    ids = D.mixed_batch(len(toy.reads))
    seq, rseq, off = enc(toy, ids)
    want = plain(monkeypatch, toy.ix, o, seq, rseq, off)
    first = cached(monkeypatch, toy.ix, o, seq, rseq, off, bits=bits)
    same(want, first, "%d bits" % bits)
    n1, ins = first["st"][1], first["st"][5]
    assert first["st"][4] == 0 and ins + first["st"][6] == n1 and n1 >= len(toy.reads) > 16
    assert ins <= 16 << bits and toy.ix.dedup_cache_stats()[2] == ins
    if bits == 0:
        assert ins == 16                                                       # one chain, filled to the probe bound
    second = cached(monkeypatch, toy.ix, o, seq, rseq, off, bits=bits)
    same(want, second, "%d bits, again" % bits)
    s2, served = searched_served(second)
    assert s2 + served == n1 and ins <= served <= n1 and second["st"][5] == 0  # every entry answers at least for its own read; nothing more fits
    if bits == 0:
        assert served < n1
    M.check(toy.orc, "default", o, False, ids, per_read_rows(second), second["maxe"], "%d hash bits" % bits)


# ---------------------------------------------------------------------------------------------------------------- 8. wide hit lists, the row cap
def test_rows_from_the_wide_lists_and_reads_over_the_row_cap(cold, monkeypatch):
    """NABWA_ALNCAP1=1: every read of two or more rows ends in the wide lists.  With a cap of 2 rows the reads of 2 rows are entered from there
    and served with both; the reads of more are searched again"""
    toy, o = cold, M.opt_block("default")
    monkeypatch.setenv("NABWA_ALNCAP1", "1")
    gold = [s for _, s, _ in T.read_fastq(os.path.join(T.GOLDEN, "reads_se.fq"))]
    reads = [toy.reads[i] for i in toy.of("polyT", "tandem")] + gold
    orc = M.Oracle(toy.olib, toy.oix.h, reads)
    ids = list(range(len(reads))) + list(range(len(reads)))[::-1]
    seq, rseq, off = M.encode([reads[i] for i in ids])
    want = plain(monkeypatch, toy.ix, o, seq, rseq, off)
    by_key = rows_by_key(want, seq, rseq, off)
    over = sum(v > 2 for v in by_key.values()); wide = sum(v == 2 for v in by_key.values())
    assert over >= 2 and wide >= 10, (over, wide)                              # (the golden reads have two different reads of three rows)
    first = cached(monkeypatch, toy.ix, o, seq, rseq, off, rows=2)
    same(want, first, "wide lists")
    assert first["st"] == [len(ids), len(by_key), 0, 1, 0, len(by_key) - over, over, 0]
    second = cached(monkeypatch, toy.ix, o, seq, rseq, off, rows=2)
    same(want, second, "wide lists, served")
    assert second["st"] == [len(ids), over, 0, 1, len(by_key) - over, 0, over, 0]
    M.check(orc, "default", o, False, ids, per_read_rows(second), second["maxe"], "wide lists, served")


# ---------------------------------------------------------------------------------------------------------------- 9. NABWA_ECAP
def test_fetch_with_too_few_rows_and_served_reads(cold, monkeypatch):
    toy, o = cold, M.opt_block("default")
    ids = D.mixed_batch(len(toy.reads))[:300]
    seq, rseq, off = enc(toy, ids)
    want = plain(monkeypatch, toy.ix, o, seq, rseq, off)
    total = int(want["n_aln"].sum())
    assert total > 1
    half = sorted(set(ids))[::2]
    cached(monkeypatch, toy.ix, o, *enc(toy, half))
    switch_on(monkeypatch)
    b = nabwa.Batch(toy.ix, M.gap_opt(o), seq, rseq, off)
    try:
        b.run()
        b.sync()
        assert b.dedup_stats_ex()[1:2] + b.dedup_stats_ex()[4:5] == [len(set(ids)) - len(half), len(half)]
        n_aln = np.full(len(ids), -1, np.int32); maxe = np.zeros(len(ids), np.int32)
        buf = np.zeros(total, nabwa.ALN_DT)
        rows = C.c_int64(-1)
        rc = nabwa.lib().nabwa_batch_fetch(b._h, T.ptr(n_aln), T.ptr(buf), total - 1, C.byref(rows), T.ptr(maxe))
        assert rc == nabwa.ECAP and rows.value == total and np.array_equal(n_aln, want["n_aln"]) and np.array_equal(maxe, want["maxe"])
        rc = nabwa.lib().nabwa_batch_fetch(b._h, T.ptr(n_aln), T.ptr(buf), total, C.byref(rows), T.ptr(maxe))
        assert rc == 0 and rows.value == total and buf.tobytes() == want["rows"]
    finally:
        b.close()


# ---------------------------------------------------------------------------------------------------------------- 10. live batches
@pytest.mark.parametrize("order", ["a first", "b first"])
def test_two_live_batches(cold, monkeypatch, order):
    """a batch whose reads are all served and one whose reads are all new, both alive on one index: run A, run B, sync B, sync A; created and
    destroyed in both orders; while either lives the cache cannot be cleared"""
    toy, o = cold, M.opt_block("default")
    known = toy.of("err100", "adna")
    new = toy.of("exact100", "long300")
    cached(monkeypatch, toy.ix, o, *enc(toy, known))
    A = [known[i % len(known)] for i in range(500)]
    switch_on(monkeypatch)
    mk = {"a": lambda: nabwa.Batch(toy.ix, M.gap_opt(o), *enc(toy, A)), "b": lambda: nabwa.Batch(toy.ix, M.gap_opt(o), *enc(toy, new))}
    bs = {}
    for k in (("a", "b") if order == "a first" else ("b", "a")):
        bs[k] = mk[k]()
    try:
        assert bs["a"].dedup_stats_ex() == [len(A), 0, 0, 1, len(set(A)), 0, 0, 0]
        with pytest.raises(nabwa.NabwaError) as e:
            toy.ix.dedup_cache_clear()
        assert e.value.code == nabwa.EINVAL
        bs["a"].run()
        bs["b"].run()
        assert bs["b"].sync() >= 0
        gb, mb = M.collect(bs["b"])
        assert bs["a"].sync() == 0
        ga, ma = M.collect(bs["a"])
        assert bs["b"].dedup_stats_ex() == [len(new), len(new), 0, 1, 0, len(new), 0, 0]
    finally:
        for k in (("a", "b") if order == "a first" else ("b", "a")):
            bs[k].close()
    M.check(toy.orc, "default", o, False, A, ga, ma, "live batch A")
    M.check(toy.orc, "default", o, False, new, gb, mb, "live batch B")
    toy.ix.dedup_cache_clear()                                                 # nothing holds it now


# ---------------------------------------------------------------------------------------------------------------- 11. one-call entries
def test_one_call_entries(cold, monkeypatch):
    toy, o = cold, M.opt_block("default")
    ids = D.mixed_batch(len(toy.reads), seed=11)[:400]
    seq, rseq, off = enc(toy, ids)
    n = len(ids)

    def records():
        arr = (nabwa.BwaSeq * n)()
        keep = []
        for i in range(n):
            s = np.ascontiguousarray(seq[off[i]:off[i + 1]]); r = np.ascontiguousarray(rseq[off[i]:off[i + 1]])
            if len(s) == 0:
                s = np.zeros(1, np.uint8); r = np.zeros(1, np.uint8)
            keep += [s, r]
            L = int(off[i + 1] - off[i])
            arr[i].seq = s.ctypes.data; arr[i].rseq = r.ctypes.data
            arr[i].bits0 = L; arr[i].lenbits = L; arr[i].clip_len = L
        toy.ix.bwa_cal_sa_reg_gap(arr, n, M.gap_opt(o))
        return [(C.string_at(arr[i].aln, 16 * arr[i].n_aln) if arr[i].n_aln else b"", arr[i].max_entries) for i in range(n)]

    def both():
        n_aln, rows, maxe = toy.ix.cal_sa_reg_gap_flat(M.gap_opt(o), seq, rseq, off, cap_rows=1 << 18)      # (room for every row: one batch per call)
        return n_aln.tobytes(), rows.tobytes(), maxe.tobytes(), records()

    unset(monkeypatch)
    want = both()
    switch_on(monkeypatch)
    s0 = toy.ix.dedup_cache_stats()
    assert both() == want                                                      # the first call fills the cache, the second (the records) is served
    s1 = toy.ix.dedup_cache_stats()
    assert s1[4] - s0[4] == 2 * len(set(ids)) and s1[5] - s0[5] == len(set(ids)) and s1[2] == len(set(ids))
    assert both() == want
    s2 = toy.ix.dedup_cache_stats()
    assert s2[5] - s1[5] == 2 * len(set(ids)) and s2[2] == s1[2]
    unset(monkeypatch)


# ---------------------------------------------------------------------------------------------------------------- 12. width records
def test_width_records_of_a_served_read_are_refused(cold, monkeypatch):
    toy, o = cold, M.opt_block("default")
    known, new = toy.of("err100")[:6], toy.of("exact100")[0]
    cached(monkeypatch, toy.ix, o, *enc(toy, known))
    ids = known + [new]
    seq, rseq, off = enc(toy, ids)
    W = int(np.diff(off).max()) + 1
    w = np.zeros((len(ids), 2, W), np.uint32); bid = np.zeros((len(ids), 2, W), np.uint8); sbid = np.zeros((len(ids), 2, o.seed_len + 1), np.uint8)
    L = nabwa.lib()
    L.nabwa_batch_width_records.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    switch_on(monkeypatch)
    b = nabwa.Batch(toy.ix, M.gap_opt(o), seq, rseq, off)
    try:
        assert b.dedup_stats_ex()[:5] == [len(ids), 1, 0, 1, len(known)]
        assert L.nabwa_batch_width_records(b._h, 0, len(ids), T.ptr(w), T.ptr(bid), T.ptr(sbid)) == nabwa.EINVAL
        assert "served" in str(L.nabwa_last_error())
        assert L.nabwa_batch_width_records(b._h, len(known) - 1, 1, T.ptr(w), T.ptr(bid), T.ptr(sbid)) == nabwa.EINVAL
        assert L.nabwa_batch_width_records(b._h, len(known), 1, T.ptr(w), T.ptr(bid), T.ptr(sbid)) == 0       # the read searched has its records
        assert w[0].any()
    finally:
        b.close()


# ---------------------------------------------------------------------------------------------------------------- 13. refusals
def test_values_the_library_refuses(cold, fresh_ix, monkeypatch):
    toy, o = cold, M.opt_block("default")
    args = (M.gap_opt(o),) + enc(toy, toy.of("err100")[:4])
    for bad in ("x", "-1", "", "1.5", "64MiB"):
        switch_on(monkeypatch, mib=bad)
        with pytest.raises(nabwa.NabwaError) as e:
            nabwa.Batch(toy.ix, *args)
        assert e.value.code == nabwa.EINVAL and "NABWA_DEDUP_CACHE" in str(e.value), bad
    for dedup in (None, "0"):                                                  # a positive value without NABWA_DEDUP=1
        unset(monkeypatch)
        monkeypatch.setenv("NABWA_DEDUP_CACHE", "64")
        if dedup:
            monkeypatch.setenv("NABWA_DEDUP", dedup)
        with pytest.raises(nabwa.NabwaError) as e:
            nabwa.Batch(toy.ix, *args)
        assert e.value.code == nabwa.EINVAL and "NABWA_DEDUP=1" in str(e.value)
    unset(monkeypatch)
    monkeypatch.setenv("NABWA_DEDUP_CACHE", "0")                               # 0 is off, with or without NABWA_DEDUP
    b = nabwa.Batch(toy.ix, *args)
    assert b.dedup_stats_ex() == [4, 4, 0, 0, 0, 0, 0, 0]
    b.close()
    # more than the device has free, on an index that has no cache yet: refused, and no cache is made
    before = fresh_ix.device_bytes()
    switch_on(monkeypatch, mib=1 << 30)
    with pytest.raises(nabwa.NabwaError) as e:
        nabwa.Batch(fresh_ix, *args)
    assert e.value.code == nabwa.EINVAL and "free" in str(e.value)
    assert fresh_ix.dedup_cache_stats() == [0] * 8 and fresh_ix.device_bytes() == before
    switch_on(monkeypatch, mib=2)
    b = nabwa.Batch(fresh_ix, *args)
    b.close()
    cs = fresh_ix.dedup_cache_stats()
    assert 0 < cs[0] <= 2 << 20 and fresh_ix.device_bytes() == before + cs[0]  # counted with the index
    unset(monkeypatch)
