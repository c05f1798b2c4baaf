"""A read's hits must not depend on the batch it is searched in.  The library decides several things per batch -- kernel S or
kernel D for the whole batch (deep_only), the S -> D hand-over budgets, lockstep waves for equal-length batches, the work order
by kernel W's classes, kernel D's wave-wide chains and whether it keeps the read in LDS, the alignment kernels' forms -- and
every such decision may change speed only, never a row.  Here one seeded pool of labelled reads (exact, 2 % substitutions and
indels, ancient-DNA-like, seed_len and seed_len + 1, 89 / 90 / 91 bp, junk, N-rich, empty, poly-T, tandem repeats, repeat-family
reads, 250 - 1600 bp) is searched in many compositions, and every read of every batch is compared with the CPU oracle, which
searches each read on its own (per_read=0: with the option block the reference derives from the batch's longest read).  Every
composition case also asserts, through nabwa_batch_config, that the switch it is about really flipped.  The option blocks
carry max_entries 20000, which bounds the oracle's long searches (the GPU applies the same cut-off)."""
import ctypes as C
import importlib
import os
import zlib

import numpy as np
import pytest

import nabwa_testlib as T

pytestmark = pytest.mark.gpu
nabwa = importlib.import_module("network-aware-bwa_amd")
synth = importlib.import_module("network-aware-bwa_amd.synth")

NTH = max(1, min(16, os.cpu_count() or 1))
COMP = str.maketrans("ACGTN", "TGCAN")


def opt_block(name):
    o = T.default_opt()
    o.max_entries = 20000
    if name == "adna":                       # aln -n 0.01 -o 2 -l 1024
        o.fnr, o.max_gapo, o.seed_len = 0.01, 2, 1024
    elif name == "n3":                       # aln -n 3
        o.fnr, o.max_diff = 0.0, 3
    else:
        assert name == "default"
    return o


def md_of(o, L):
    return nabwa.cal_maxdiff(L, 0.02, o.fnr) if o.fnr > 0 else o.max_diff


def deep_len():
    """the shortest read that alone sends a batch under the default options to kernel D (max_diff > 14)"""
    return next(L for L in range(500, 4000) if nabwa.cal_maxdiff(L, 0.02, 0.04) > 14)


# ---------------------------------------------------------------------------------------------------------------- the pool
def genome_text(prefix):
    seqs, cur = [], []
    for line in open(prefix + ".fa"):
        if line.startswith(">"):
            if cur:
                seqs.append("".join(cur))
            cur = []
        else:
            cur.append(line.strip())
    seqs.append("".join(cur))
    return "".join(seqs)


def mutate(rng, s, sub, indel=0.0, n_rate=0.0):
    s = list(s)
    for j in range(len(s)):
        if rng.random() < sub:
            s[j] = "ACGT"[("ACGT".index(s[j]) + 1 + int(rng.integers(0, 3))) % 4] if s[j] in "ACGT" else "A"
        if n_rate and rng.random() < n_rate:
            s[j] = "N"
    if indel and rng.random() < indel and len(s) > 30:
        q = int(rng.integers(10, len(s) - 10))
        if rng.random() < 0.5:
            del s[q]
        else:
            s.insert(q, "ACGT"[int(rng.integers(0, 4))])
    return "".join(s)


def build_pool(G, rng, long_lens=(250, 300, 600)):
    """[(kind, read)]: reads cut from text G (either strand), mutated as their kind says"""
    pool = []

    def cut(L, extra=2):
        p = int(rng.integers(0, len(G) - L - extra))
        s = G[p:p + L + extra]
        return s if rng.random() < 0.5 else s.translate(COMP)[::-1]

    def add(kind, n, make):
        for _ in range(n):
            pool.append((kind, make()))
    add("exact100", 60, lambda: cut(100)[:100])
    add("err100", 60, lambda: mutate(rng, cut(100), 0.02, 0.3)[:100])
    add("err150", 40, lambda: mutate(rng, cut(150), 0.02, 0.3)[:150])

    def adna():
        L = int(rng.integers(25, 71))
        s = list(mutate(rng, cut(L)[:L], 0.005))
        for j in range(min(4, L)):                            # deamination: C -> T at the 5' end, G -> A at the 3' end
            if s[j] == "C" and rng.random() < 0.5:
                s[j] = "T"
            if s[L - 1 - j] == "G" and rng.random() < 0.5:
                s[L - 1 - j] = "A"
        return "".join(s)
    add("adna", 80, adna)
    add("seed32", 20, lambda: mutate(rng, cut(32)[:32], 0.01))
    add("seed33", 20, lambda: mutate(rng, cut(33)[:33], 0.01))
    for L in (89, 90, 91):
        add("len%d" % L, 20, lambda L=L: mutate(rng, cut(L)[:L], 0.01))
    add("random", 30, lambda: "".join("ACGT"[x] for x in rng.integers(0, 4, 100)))
    add("nrich", 15, lambda: mutate(rng, cut(100)[:100], 0.0, 0.0, 0.08))
    add("allN", 4, lambda: "N" * int(rng.integers(20, 120)))
    add("empty", 4, lambda: "")
    add("polyT", 5, lambda: mutate(rng, "T" * 100, 0.01))
    for unit in ("CA", "AGG", "ATTC", "GGGAT"):
        add("tandem", 2, lambda u=unit: mutate(rng, (u * 60)[:100], 0.01))
    for L in long_lens:
        add("long%d" % L, 6, lambda L=L: mutate(rng, cut(L)[:L], 0.005))
    return pool


def encode(reads):
    seq, rseq, off, _ = T.encode_reads([(str(i), s, "I" * len(s)) for i, s in enumerate(reads)])
    return seq, rseq, off


# ---------------------------------------------------------------------------------------------------------------- oracle
class Oracle:
    """the oracle's rows per read, cached: under per_read=1 a read's answer is its own; under per_read=0 it depends on the batch
    only through max_diff of the batch's longest read, which an all-N read of that length (no hit, no search) reproduces"""

    def __init__(self, olib, oh, reads):
        self.olib, self.oh, self.reads, self.cache = olib, oh, reads, {}

    def want(self, name, o, per_read, ids):
        lens = [len(self.reads[i]) for i in ids]
        max_len = max(lens) if lens else 0
        key = (name, bytes(o), 1 if per_read else 0, -1 if per_read else md_of(o, max_len))
        memo = self.cache.setdefault(key, {})
        todo = sorted(set(i for i in ids if i not in memo))
        if todo:
            rs = [self.reads[i] for i in todo]
            if not per_read and max(len(r) for r in rs) < max_len:
                rs.append("N" * max_len)
            seq, rseq, off = encode(rs)
            rows, maxe = T.oracle_cal_sa_reg_gap(self.olib, self.oh, o, seq, rseq, off, per_read=int(bool(per_read)), n_threads=NTH)
            for j, i in enumerate(todo):
                memo[i] = (rows[j].tobytes(), int(maxe[j]))
        return [memo[i] for i in ids]


def mix64(x):
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xff51afd7ed558ccd)
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xc4ceb9fe1a85ec53)
    return x ^ (x >> np.uint64(33))


def host_checksum(n_aln, rows):
    """what checksum_kernel (batch_kernels.hip) computes over fetched rows: sum over reads of a mix of (read, count, rows)"""
    with np.errstate(over="ignore"):
        n_aln = n_aln.astype(np.uint64)
        i = np.arange(len(n_aln), dtype=np.uint64)
        s = mix64((i << np.uint64(20)) ^ n_aln ^ np.uint64(0x9e3779b97f4a7c15)).sum(dtype=np.uint64)
        if len(rows):
            rid = np.repeat(i, n_aln.astype(np.int64))
            start = np.concatenate([[0], np.cumsum(n_aln.astype(np.int64))[:-1]])
            j = np.arange(len(rows), dtype=np.int64) - np.repeat(start, n_aln.astype(np.int64))
            w = rows.view(np.uint32).reshape(-1, 4).astype(np.uint64)
            h = ((rid << np.uint64(32)) | j.astype(np.uint64)) ^ mix64((w[:, 0] << np.uint64(32)) | w[:, 1]) \
                ^ (mix64((w[:, 2] << np.uint64(32)) | w[:, 3]) * np.uint64(3))
            s = s + mix64(h).sum(dtype=np.uint64)
    return int(s), int(n_aln.sum())


def gap_opt(o):
    g = nabwa.GapOpt()
    C.memmove(C.byref(g), C.byref(o), 64)
    return g


def search(ix, o, reads, ids, per_read=False):
    """one batch of the pool's reads ids, in that order -> (rows per read, max_entries, n2, config, kernel D ms)"""
    b = nabwa.Batch(ix, gap_opt(o), *encode([reads[i] for i in ids]), per_read=per_read)
    try:
        b.run()
        n2 = b.sync()
        out = collect(b)
        return out + (n2, b.config(), b.last_deep_ms())
    finally:
        b.close()


def collect(b):
    n_aln, rows, maxe = b.fetch_flat()
    assert b.checksum() == host_checksum(n_aln, rows)          # the device's own reading of its rows agrees with what was fetched
    bnd = np.concatenate([[0], np.cumsum(n_aln)])
    return [rows[bnd[i]:bnd[i + 1]].tobytes() for i in range(len(n_aln))], maxe


def check(orc, name, o, per_read, ids, got, maxe, what=""):
    want = orc.want(name, o, per_read, ids)
    bad = [(t, ids[t]) for t in range(len(ids)) if got[t] != want[t][0] or int(maxe[t]) != want[t][1]]
    assert not bad, "%s: %d of %d reads differ from the oracle, first at batch position %d (pool read %d, %d bp)" % (
        what, len(bad), len(ids), bad[0][0], bad[0][1], len(orc.reads[bad[0][1]]))


# ---------------------------------------------------------------------------------------------------------------- fixtures
class World:
    """an index, its oracle, and the pool of reads cut from its text"""

    def __init__(self, ix, orc, kinds, reads, parts=None, d_text=None, oh=None):
        self.ix, self.orc, self.kinds, self.reads = ix, orc, kinds, reads
        self.parts, self.d_text, self.oh = parts, d_text, oh

    def of(self, *kinds):
        return [i for i, k in enumerate(self.kinds) if k in kinds]

    def close(self):
        self.ix.close()
        if self.oh is not None:
            self.orc.olib.orc_index_free(self.oh)
        for p in self.parts or ():
            p[0].free()
            p[2].free()
        if self.d_text is not None:
            self.d_text.free()


@pytest.fixture(scope="module")
def olib():
    return T.load_oracle()


@pytest.fixture(scope="module")
def toy(olib):
    oix = T.OracleIndex(olib)
    rng = np.random.default_rng(20261015)
    G = genome_text(T.TOY)
    pool = build_pool(G, rng, (250, 300, 600, deep_len(), 1600))
    kinds = [k for k, _ in pool]
    kinds = ["long1150" if k == "long%d" % deep_len() else k for k in kinds]
    reads = [s for _, s in pool]
    w = World(nabwa.Index.load(T.TOY, 0, True, True), Oracle(olib, oix.h, reads), kinds, reads)
    yield w
    w.ix.close()


@pytest.fixture(scope="module")
def rep(olib):
    """a 3 Mbp genome of repeat families (bench.py --repeats), index built on the GPU; its reads of several hit rows are the
    'repeat' kind"""
    n = 3_000_017
    d_text = synth.synth_text_repeats(n, 11)
    parts = [synth.build_index(d_text, n, rev, 32, True) for rev in (0, 1)]
    ix = nabwa.Index.from_arrays((parts[0][0].ptr, parts[0][1]), (parts[1][0].ptr, parts[1][1]),
                                 (parts[0][2].ptr, parts[0][3]), (parts[1][2].ptr, parts[1][3]), device_ptrs=True)
    h0 = parts[0][0].to_host(np.uint32, parts[0][1])
    h1 = parts[1][0].to_host(np.uint32, parts[1][1])
    oh = olib.orc_index_wrap(T.ptr(h0), len(h0), T.ptr(h1), len(h1))
    text = d_text.to_host(np.uint8, n)
    G = "".join("ACGT"[x] for x in text[:n])
    rng = np.random.default_rng(31)
    pool = build_pool(G, rng, (250, 600))
    reads = [s for _, s in pool]
    kinds = [k for k, _ in pool]
    orc = Oracle(olib, oh, reads)
    # the repeat kind: of 20000 reads cut anywhere, the 120 whose hits cover the most occurrences
    cand = [mutate(rng, G[p:p + 100], 0.005) for p in rng.integers(0, n - 200, 20000)]
    seq, rseq, off = encode(cand)
    rows, _ = T.oracle_cal_sa_reg_gap(olib, oh, opt_block("default"), seq, rseq, off, n_threads=NTH)
    assert sum(len(r) > 0 for r in rows) > 0.9 * len(cand), "reads cut from the genome must be found in its index"
    occ = np.array([int((r["l"].astype(np.int64) - r["k"] + 1).sum()) for r in rows])
    top = np.argsort(-occ, kind="stable")[:120]
    reads += [cand[i] for i in top]
    kinds += ["repeat"] * len(top)
    w = World(ix, orc, kinds, reads, parts, d_text, oh)
    w.h = (h0, h1)
    yield w
    w.close()


# ---------------------------------------------------------------------------------------------------------------- composition
@pytest.mark.parametrize("name", ["default", "adna", "n3"])
def test_each_kind_alone_and_single_read_batches(toy, name):
    """every kind in a batch of its own, then 100 reads each alone (a batch of one read is a uniform batch: lockstep on)"""
    o = opt_block(name)
    for kind in sorted(set(toy.kinds)):
        ids = toy.of(kind)
        got, maxe, n2, cfg, _ = search(toy.ix, o, toy.reads, ids)
        check(toy.orc, name, o, False, ids, got, maxe, "%s alone" % kind)
    rng = np.random.default_rng(3)
    for i in rng.choice(len(toy.reads), 100, replace=False):
        got, maxe, n2, cfg, _ = search(toy.ix, o, toy.reads, [int(i)])
        assert cfg["w_sync"] == 1 and cfg["n"] == 1
        check(toy.orc, name, o, False, [int(i)], got, maxe, "read %d alone" % i)


@pytest.mark.parametrize("per_read", [False, True])
def test_uniform_length_batch_against_the_same_reads_ragged(toy, per_read):
    """the 100 bp reads of every kind alone: lockstep waves (w_sync); the same reads with one 99 bp read among them: none"""
    o = opt_block("default")
    ids = [i for i in range(len(toy.reads)) if len(toy.reads[i]) == 100]
    assert len(set(toy.kinds[i] for i in ids)) >= 5
    got, maxe, _, cfg, _ = search(toy.ix, o, toy.reads, ids, per_read)
    assert cfg["w_sync"] == 1 and cfg["min_len"] == cfg["max_len"] == 100
    check(toy.orc, "default", o, per_read, ids, got, maxe, "uniform")
    short = next(i for i in toy.of("err100") if len(toy.reads[i]) == 100)
    toy.reads.append(toy.reads[short][:99])
    toy.kinds.append("cut99")
    ids2 = ids[: len(ids) // 2] + [len(toy.reads) - 1] + ids[len(ids) // 2:]
    got, maxe, _, cfg, _ = search(toy.ix, o, toy.reads, ids2, per_read)
    assert cfg["w_sync"] == 0
    check(toy.orc, "default", o, per_read, ids2, got, maxe, "ragged")


@pytest.mark.parametrize("name,per_read", [("default", False), ("default", True), ("adna", False), ("adna", True), ("n3", False)])
@pytest.mark.parametrize("world", ["toy", "rep"])
def test_whole_pool_in_three_orders(request, world, name, per_read):
    """the whole pool shuffled, sorted by length ascending and descending, with and without the reads long enough to send the
    batch to kernel D; on the toy genome and on the repeat-family genome"""
    w = request.getfixturevalue(world)
    o = opt_block(name)
    rng = np.random.default_rng(zlib.crc32(("%s %s %d" % (world, name, per_read)).encode()))
    everything = list(range(len(w.reads)))
    short = [i for i in everything if len(w.reads[i]) < 1000]
    for label, ids in (("all", everything), ("no long reads", short))[: 1 if len(short) == len(everything) else 2]:
        sh = list(rng.permutation(ids))
        for order, seq_ids in (("shuffled", sh), ("ascending", sorted(ids, key=lambda i: len(w.reads[i]))),
                               ("descending", sorted(ids, key=lambda i: -len(w.reads[i])))):
            got, maxe, n2, cfg, _ = search(w.ix, o, w.reads, [int(i) for i in seq_ids], per_read)
            check(w.orc, name, o, per_read, [int(i) for i in seq_ids], got, maxe, "%s, %s, %s" % (world, label, order))


def test_junk_majority_takes_the_hard_budget(toy):
    """reads without an exact occurrence (kernel W's classes 1 and 2+) in the majority: kernel S runs with the hard budget (200
    trips instead of 2000); in the minority: not -- the same genome reads either way"""
    o = opt_block("default")
    exact = toy.of("exact100")
    junk = toy.of("random", "nrich", "err100")
    few = exact[:50] + junk[:20]
    many = exact[:20] + junk[:50]
    for ids, hard in ((few, 0), (many, 1)):
        got, maxe, _, cfg, _ = search(toy.ix, o, toy.reads, ids)
        assert cfg["trip_budget"] == 2000 and cfg["trip_budget_hard"] == 200
        assert cfg["hard_budget"] == hard, cfg
        assert (2 * cfg["n_sync"] > len(ids)) == bool(hard)
        assert sum(cfg["cls"]) == len(ids) and cfg["cls"][0] == len(ids) - cfg["n_sync"]
        check(toy.orc, "default", o, False, ids, got, maxe, "junk %s" % ("majority" if hard else "minority"))


def test_89_bp_reads_with_and_without_one_90_bp_read(toy, monkeypatch):
    """kernel D's wave-wide one-row chains run for batches whose longest read has 90 bases or more: 89 bp reads alone without
    them, with one 90 bp read added with them (every search handed to D after one trip)"""
    monkeypatch.setenv("NABWA_TRIP_BUDGET", "1")
    o = opt_block("default")
    ids = toy.of("len89")
    for extra, coop in (([], 0), (toy.of("len90")[:1], 4)):
        b_ids = ids[:10] + extra + ids[10:]
        got, maxe, n2, cfg, ms = search(toy.ix, o, toy.reads, b_ids)
        assert n2 > 0 and ms > 0 and cfg["max_len"] == (90 if extra else 89)
        assert cfg["coop_lanes"] == coop, cfg
        check(toy.orc, "default", o, False, b_ids, got, maxe, "89 bp + %d" % len(extra))


@pytest.mark.parametrize("name,extra_len", [("default", 33), ("adna", 1025)])
def test_short_reads_with_and_without_one_read_longer_than_the_seed(toy, name, extra_len):
    """reads no longer than seed_len hand over to kernel D after 300 trips, a batch with one read longer than the seed after 2000
    (hard budget 200): 25 - 32 bp aDNA reads, then the same with one seed_len + 1 read"""
    o = opt_block(name)
    ids = [i for i in toy.of("adna", "seed32") if len(toy.reads[i]) <= 32]
    assert len(ids) >= 20
    src = next(i for i in toy.of("seed33", "long1150", "long1600") if len(toy.reads[i]) >= extra_len)
    toy.reads.append(toy.reads[src][:extra_len])
    toy.kinds.append("cut%d" % extra_len)
    assert len(toy.reads[-1]) == extra_len == o.seed_len + 1
    for b_ids, budget in ((ids, (300, 300)), (ids[:7] + [len(toy.reads) - 1] + ids[7:], (2000, 200))):
        got, maxe, n2, cfg, _ = search(toy.ix, o, toy.reads, b_ids)
        assert (cfg["trip_budget"], cfg["trip_budget_hard"]) == budget, cfg
        check(toy.orc, name, o, False, b_ids, got, maxe, "budget %d" % budget[0])


@pytest.mark.parametrize("per_read", [False, True])
def test_100_bp_reads_with_and_without_one_read_that_needs_kernel_d(toy, per_read):
    """one read long enough for max_diff > 14 sends the whole batch to kernel D (deep_only), read from LDS there; one 1600 bp
    read on top makes kernel D read the reads from HBM"""
    o = opt_block("default")
    ids = toy.of("exact100", "err100")[:100]
    L1, L2 = toy.of("long1150")[0], toy.of("long1600")[0]
    got, maxe, n2, cfg, ms = search(toy.ix, o, toy.reads, ids, per_read)
    assert cfg["deep_only"] == 0 and n2 < len(ids)
    check(toy.orc, "default", o, per_read, ids, got, maxe, "100 bp")
    b_ids = ids[:50] + [L1] + ids[50:]
    got, maxe, n2, cfg, ms = search(toy.ix, o, toy.reads, b_ids, per_read)
    assert cfg["deep_only"] == 1 and n2 == len(b_ids) and ms > 0
    assert cfg["lds_rd"] > 0, cfg                            # the reads in kernel D's LDS
    check(toy.orc, "default", o, per_read, b_ids, got, maxe, "100 bp + %d bp" % len(toy.reads[L1]))
    b_ids = ids[:50] + [L1] + ids[50:] + [L2]
    got, maxe, n2, cfg, ms = search(toy.ix, o, toy.reads, b_ids, per_read)
    assert cfg["deep_only"] == 1 and n2 == len(b_ids) and ms > 0
    assert cfg["lds_rd"] == 0, cfg                           # fm_deep_kernel<*, false, *>: the reads from HBM
    check(toy.orc, "default", o, per_read, b_ids, got, maxe, "100 bp + %d bp + 1600 bp" % len(toy.reads[L1]))


# ---------------------------------------------------------------------------------------------------------------- kernel S at its field limits
def planted(G, rng, n_sub=0, n_indel=0, del_len=0, L=100, seed_len=32):
    """a read of G with n_sub substitutions, n_indel one-base indels and one deletion of del_len bases, all after the seed"""
    p = int(rng.integers(0, len(G) - 3 * L))
    s = list(G[p:p + 2 * L])
    if del_len:
        q = int(rng.integers(seed_len + 8, L - 20))
        del s[q:q + del_len]
    for q in sorted(rng.choice(np.arange(seed_len + 4, L - 6), n_indel, replace=False), reverse=True):
        if q % 2:
            del s[q]
        else:
            s.insert(q, "ACGT"[(("ACGT".index(s[q]) + 1) % 4)])
    s = s[:L]
    for q in rng.choice(np.arange(seed_len + 2, L), n_sub, replace=False):
        s[q] = "ACGT"[("ACGT".index(s[q]) + 1 + int(rng.integers(0, 3))) % 4]
    s = "".join(s)
    return s if rng.random() < 0.5 else s.translate(COMP)[::-1]


def field_block(name):
    """(option block, its neighbour one step over, field index of the hit rows to fill, reads)"""
    o = opt_block("default")
    o.fnr = 0.0
    if name == "n_mm":                  # aln -n 14: a child holds up to 15 mismatches in its 4 bits
        o.max_diff = 14
        nb = opt_block("default"); C.memmove(C.byref(nb), C.byref(o), 64); nb.max_diff = 15
        return o, nb, 0, [dict(n_sub=k) for k in (6, 8, 10, 12, 13, 14) for _ in range(4)]
    if name == "n_gapo":                # aln -n 14 -o 14 -O 2 -E 1 -e 0: gap opens climb in their 4 bits
        o.max_diff, o.max_gapo, o.s_gapo, o.s_gape, o.max_gape = 14, 14, 2, 1, 0
        o.mode &= ~1
        nb = opt_block("default"); C.memmove(C.byref(nb), C.byref(o), 64); nb.max_diff = 15
        return o, nb, 1, [dict(n_indel=k) for k in (2, 4, 6, 8, 10) for _ in range(4)]
    if name == "n_gape":                # aln -n 4 -o 2 -O 1 -E 1 -e 31: gap extensions up to 31 in their 5 bits
        o.max_diff, o.max_gapo, o.s_gapo, o.s_gape, o.max_gape = 4, 2, 1, 1, 31
        o.mode &= ~1
        nb = opt_block("default"); C.memmove(C.byref(nb), C.byref(o), 64); nb.max_gape = 32
        return o, nb, 2, [dict(del_len=k) for k in (8, 16, 24, 28, 32) for _ in range(4)]
    assert name == "ns64"                # aln -n 14 -O 15: the first pass's score levels come to exactly 64
    o.max_diff, o.s_gapo = 14, 15
    nb = opt_block("default"); C.memmove(C.byref(nb), C.byref(o), 64); nb.s_gapo = 16
    return o, nb, 0, [dict(n_sub=k) for k in (8, 12, 14) for _ in range(4)] + [dict(n_sub=k, n_indel=1) for k in (4, 8) for _ in range(4)]


@pytest.mark.parametrize("name", ["n_mm", "n_gapo", "n_gape", "ns64"])
def test_kernel_s_at_its_field_limits(toy, olib, monkeypatch, name):
    """option blocks that keep the batch in kernel S with a packed field of its entries as full as the 64-level cap allows, reads
    planted to fill it, every search finished by S itself (no hand-over budget, an arena no search outgrows); then the block one
    step over, which must go to kernel D whole"""
    monkeypatch.setenv("NABWA_TRIP_BUDGET", "0")
    monkeypatch.setenv("NABWA_CAP1", "65534")
    o, nb, field, plan = field_block(name)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    G = genome_text(T.TOY)
    reads = []
    for kw in plan:                     # kept where kernel S's arena (bump-allocated: every push that reaches memory) holds the search
        r = planted(G, rng, **kw)
        cnt = T.Counters()
        T.oracle_cal_sa_reg_gap(olib, toy.orc.oh, o, *encode([r]), counters=cnt)
        if cnt.n_push < 60000:
            reads.append(r)
    assert len(reads) >= len(plan) // 2
    orc = Oracle(olib, toy.orc.oh, reads)
    ids = list(range(len(reads)))
    got, maxe, n2, cfg, _ = search(toy.ix, o, reads, ids)
    assert cfg["deep_only"] == 0 and cfg["ns1"] <= 64 and n2 == 0, cfg
    if name == "ns64":
        assert cfg["ns1"] == 64
    check(orc, name, o, False, ids, got, maxe, "block %s in kernel S" % name)
    top = max((int(r["info"]) >> (8 * field) & 255) for g in got for r in np.frombuffer(g, T.ALN_DT)) if any(got) else 0
    need = {"n_mm": 14, "n_gapo": 6, "n_gape": 16, "ns64": 12}[name]
    assert top >= need, "the planted reads reach %d in field %d, not %d" % (top, field, need)
    got, maxe, n2, cfg, _ = search(toy.ix, nb, reads, ids)
    assert cfg["deep_only"] == 1 and n2 == len(ids), cfg
    check(orc, name + "+1", nb, False, ids, got, maxe, "block %s one step over, in kernel D" % name)


# ---------------------------------------------------------------------------------------------------------------- pooled buffers
def test_pooled_buffers_and_interleaved_batches(toy):
    """a deep long-read batch closed, then a short batch that takes its pooled buffers; then two live batches of different shape
    run A, run B, sync B, sync A -- the streamed paths of the bench"""
    o = opt_block("default")
    longb = toy.of("long600", "long1150", "long1600") + toy.of("err100")[:40]
    shortb = [i for i in toy.of("adna", "seed32") if len(toy.reads[i]) <= 32]
    got, maxe, n2, cfg, _ = search(toy.ix, o, toy.reads, longb)
    assert cfg["deep_only"] == 1 and cfg["lds_rd"] == 0
    check(toy.orc, "default", o, False, longb, got, maxe, "long batch")
    got, maxe, n2, cfg, _ = search(toy.ix, o, toy.reads, shortb)
    check(toy.orc, "default", o, False, shortb, got, maxe, "short batch after it")
    A = [i for i in range(len(toy.reads)) if len(toy.reads[i]) < 1000]
    B = longb + shortb
    ba = nabwa.Batch(toy.ix, gap_opt(o), *encode([toy.reads[i] for i in A]))
    bb = nabwa.Batch(toy.ix, gap_opt(o), *encode([toy.reads[i] for i in B]))
    try:
        ba.run()
        bb.run()
        bb.sync()
        ga, ma = collect(bb)
        ba.sync()
        gb, mb = collect(ba)
        assert bb.config()["deep_only"] == 1 and ba.config()["deep_only"] == 0
    finally:
        ba.close()
        bb.close()
    check(toy.orc, "default", o, False, B, ga, ma, "live batch B")
    check(toy.orc, "default", o, False, A, gb, mb, "live batch A")


# ---------------------------------------------------------------------------------------------------------------- finishing chain
def ref_chain(ref, rix, o, seq, rseq, off, hits, seed):
    P = C.c_void_p
    ref.ref_se_chain_mt.argtypes = [P, P, C.c_int, C.c_int, P, P, P, P, P, C.c_int, P, P, P, C.c_int, P]
    n = len(off) - 1
    na = np.array([len(h) for h in hits], np.int32)
    rows = np.ascontiguousarray(np.concatenate([np.asarray(h, nabwa.ALN_DT) for h in hits] + [np.zeros(0, nabwa.ALN_DT)]))
    f = np.zeros((n, 16), np.int64); cg = np.zeros((n, 64), np.uint16); md = np.zeros((n, 512), np.uint8)
    secs = (C.c_double * 2)()
    copt = T.GapOpt(); C.memmove(C.byref(copt), C.byref(o), 64)
    ref.ref_seed48(seed)
    ref.ref_se_chain_mt(rix, C.byref(copt), 3, n, T.ptr(off), T.ptr(seq), T.ptr(rseq), T.ptr(na), T.ptr(rows), 4, T.ptr(f),
                        T.ptr(cg), T.ptr(md), 512, secs)
    return f, cg, md


def test_finishing_chain_on_the_mixed_pool(toy):
    """the single-end chain (se_finish) from the GPU rows of the whole pool against the compiled reference's chain on the same
    batch in the same order with the same seed, field by field; in two orders.  The reference draws its random hit choice from
    drand48 in batch order, so across the two orders only the reads with one best hit must agree"""
    ref = T.load_ref()
    if ref is None:
        pytest.skip("oracle/_ref is absent: the compiled reference chain is not at hand")
    o = opt_block("default")
    rix = C.c_void_p(ref.ref_index_load(T.TOY.encode(), 1))
    rng = np.random.default_rng(17)
    ids_all = [i for i in range(len(toy.reads)) if len(toy.reads[i]) > 0]
    per_order = {}
    forms0 = nabwa.dp_form_counts()
    for order, ids in (("shuffled", [int(i) for i in rng.permutation(ids_all)]), ("ascending", sorted(ids_all, key=lambda i: len(toy.reads[i])))):
        got, maxe, n2, cfg, _ = search(toy.ix, o, toy.reads, ids)
        check(toy.orc, "default", o, False, ids, got, maxe, "chain batch, " + order)
        hits = [np.frombuffer(g, nabwa.ALN_DT) for g in got]
        seq, rseq, off = encode([toy.reads[i] for i in ids])
        full = np.diff(off).astype(np.int32)
        recs, _ = toy.ix.se_finish(gap_opt(o), seq, rseq, off, full, hits, 3, nabwa.srand48_state(5))
        f, cg, md = ref_chain(ref, rix, o, seq, rseq, off, hits, 5)
        n_map = 0
        for t, i in enumerate(ids):
            s, w = recs[t], f[t]
            assert s.type == w[0], (order, i)
            if s.type == 0:
                continue
            n_map += 1
            assert [s.strand, s.n_mm, s.n_gapo, s.n_gape, s.score, s.sa, s.c1, s.c2, s.pos, s.mapQ] == [int(x) for x in w[1:11]], (order, i)
            assert s.n_cigar == w[12] and list(s.cigar[:s.n_cigar]) == list(cg[t, :s.n_cigar]) and s.nm == w[13], (order, i)
            assert s.md == bytes(md[t]).split(b"\0", 1)[0], (order, i)
        assert n_map > len(ids) // 2
        per_order[order] = {i: recs[t] for t, i in enumerate(ids)}
    n_same = 0
    for i in ids_all:
        a, b = per_order["shuffled"][i], per_order["ascending"][i]
        if a.type == 1 and a.c1 == 1:                       # BWA_TYPE_UNIQUE: no random choice
            n_same += 1
            assert (b.type, b.strand, b.pos, b.mapQ, b.n_cigar, list(b.cigar[:b.n_cigar]), b.md) == \
                (a.type, a.strand, a.pos, a.mapQ, a.n_cigar, list(a.cigar[:a.n_cigar]), a.md), i
    assert n_same > 100
    assert any(per_order["shuffled"][i].type for i in toy.of("long1600")), "the long reads were not placed"
    forms = [b - a for a, b in zip(forms0, nabwa.dp_form_counts())]
    assert sum(forms[:3]) > 0


# ---------------------------------------------------------------------------------------------------------------- alignment kernels
def test_alignment_kernels_form_follows_the_largest_task():
    """the global and the local alignment kernels pick their form from the batch's largest task: small tasks alone (one wavefront
    per task; rows in LDS) and the same tasks with one large task among them (lanes; rows in HBM) give the same answers"""
    rng = np.random.default_rng(23)
    mat = np.where(np.eye(5, dtype=bool), 11, -19).astype(np.int32)
    mat[4, :] = mat[:, 4] = -13
    mat = mat.reshape(-1)
    refs, qrys = [], []
    for _ in range(200):
        q = rng.integers(0, 4, int(rng.integers(30, 160))).astype(np.uint8)
        r = np.concatenate([rng.integers(0, 4, int(rng.integers(0, 20))), q, rng.integers(0, 4, int(rng.integers(0, 20)))]).astype(np.uint8)
        r[rng.integers(0, len(r), 3)] = rng.integers(0, 4, 3)
        refs.append(r); qrys.append(q)

    def flat(xs):
        return np.concatenate(xs), np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int64)
    big_q = rng.integers(0, 4, 3000).astype(np.uint8)
    big_r = np.concatenate([big_q[:1500], rng.integers(0, 4, 5), big_q[1500:]]).astype(np.uint8)
    big_w = np.concatenate([rng.integers(0, 4, 4500), big_q, rng.integers(0, 4, 1000)]).astype(np.uint8)   # a window beyond LDS
    for kind in ("global", "local"):
        outs = []
        for big in (False, True):
            R = refs[:100] + ([big_r if kind == "global" else big_w] if big else []) + refs[100:]
            Q = qrys[:100] + ([big_q] if big else []) + qrys[100:]
            (r, ro), (q, qo) = flat(R), flat(Q)
            c0 = nabwa.dp_form_counts()
            if kind == "global":
                score, cigs = nabwa.global_align(r, ro, q, qo, 26, 9, 5, mat, 50, max_cigar=512)
                res = [(int(score[t]), list(cigs[t])) for t in range(len(R))]
            else:
                score, coords, subo, cigs = nabwa.local_align(r, ro, q, qo, 26, 9, mat, 50, 1, max_cigar=512)
                res = [(int(score[t]), tuple(coords[t]), int(subo[t]), list(cigs[t])) for t in range(len(R))]
            d = [b - a for a, b in zip(c0, nabwa.dp_form_counts())]
            if kind == "global":
                assert (d[0] > 0 and d[1] + d[2] == 0) if not big else (d[0] == 0 and d[1] + d[2] > 0), d
            else:
                assert (d[3] > 0 and d[4] == 0) if not big else (d[3] == 0 and d[4] > 0), d
            if big:
                del res[100]
            outs.append(res)
        assert outs[0] == outs[1], kind
