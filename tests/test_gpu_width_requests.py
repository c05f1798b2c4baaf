"""Kernel W's table trips that take two levels from every 32 bytes (NABWA_W_QUADS), on the toy index: the primary keys of the
interval table, and the width records of reads chosen to reach the primary-row correction and to leave text mode at every place
of a window -- against the oracle's bwt_cal_width."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import nabwa_testlib as T
import width_cases as W

pytestmark = pytest.mark.gpu
nabwa = importlib.import_module("network-aware-bwa_amd")

EQUAL_LENGTHS = (8, 33, 40, 100)


def to_gap_opt(o):
    g = nabwa.GapOpt()
    C.memmove(C.byref(g), C.byref(o), 64)
    return g


@pytest.fixture(scope="module")
def olib():
    return T.load_oracle()


@pytest.fixture(scope="module")
def oix(olib):
    return T.OracleIndex(olib)


@pytest.fixture(scope="module")
def index_of():
    """the toy index with an interval table of depth kt (None: the depth the library picks), loaded once"""
    cache = {}

    def get(kt):
        if kt not in cache:
            old = os.environ.pop("NABWA_KMER_T", None)
            if kt is not None:
                os.environ["NABWA_KMER_T"] = str(kt)
            try:
                cache[kt] = nabwa.Index.load(T.TOY, 0, True)
            finally:
                os.environ.pop("NABWA_KMER_T", None)
                if old is not None:
                    os.environ["NABWA_KMER_T"] = old
        return cache[kt]
    yield get
    for ix in cache.values():
        ix.close()


# ------------------------------------------------------------------ the primary keys

@pytest.mark.parametrize("t", range(1, 8))
def test_primary_keys_and_the_width_identity_on_the_device_table(index_of, oix, t):
    a, b = index_of(t), index_of(t + 1)
    for which in (0, 1):
        primary, _, _ = W.bwt_header(oix.bwt(which))
        assert int(a.export(which, 4, 0, 1)[0]) == t and int(b.export(which, 4, 0, 1)[0]) == t + 1
        par = a.export(which, 3, 0, 4 ** t).astype(np.int64)
        kids = b.export(which, 3, 0, 4 ** (t + 1)).astype(np.int64)
        pk_a, pk_b = a.export(which, 5, 0, 17), b.export(which, 5, 0, 17)
        holds = (par[:, 0] <= par[:, 1]) & (par[:, 0] <= primary) & (primary <= par[:, 1])
        assert int(holds.sum()) == 1
        assert int(pk_a[t]) == int(np.flatnonzero(holds)[0]), "the key reported for level %d does not hold the primary row" % t
        assert np.array_equal(pk_b[1:t + 1], pk_a[1:t + 1])      # the levels the two tables share
        kk, kl = kids[int(pk_b[t + 1])]
        assert kk <= primary <= kl
        assert (pk_a[t + 1:] == 0xffffffff).all() and (pk_b[t + 2:] == 0xffffffff).all()      # no such level
        child_sum = W.widths(kids).reshape(-1, 4).sum(axis=1)
        assert np.array_equal(W.widths(par), child_sum + holds)


# ------------------------------------------------------------------ table trips against the oracle

@pytest.fixture(scope="module")
def trip_reads():
    rng = np.random.default_rng(1405)
    contigs = W.toy_contigs()
    text = "".join(contigs)
    ends = []
    for src in contigs + [text]:
        for L in list(range(1, 41)) + [64, 100]:
            for s in (src[:L], src[-L:]):
                ends += W.four_ways(s)
    reads = list(ends)
    reads += [W.with_n(s, int(rng.integers(0, len(s)))) for s in ends]
    for i in range(200):
        L = (3, 4, 5, 8, 20, 33, 100)[i % 7]
        if i % 2:
            reads.append("".join("ACGT"[x] for x in rng.integers(0, 4, L)))
        else:
            p = int(rng.integers(0, len(text) - L))
            s = list(text[p:p + L])
            for j in range(L):
                if rng.random() < 0.03:
                    s[j] = "ACGTN"[int(rng.integers(0, 5))]
            reads.append("".join(s))
    reads += W.primary_tail_reads(rng, text)
    return reads


def test_the_trip_reads_put_the_primary_row_inside_intervals_of_every_level(trip_reads, olib, oix):
    """by the oracle alone: on either index and at every level 1..8 at least one interval of the batch, at a position >= 1 that is
    not a pass's last, holds the primary row -- without that a wrong correction would go unseen"""
    seq, rseq, off = W.as_batch(trip_reads)
    seen = np.zeros((2, 9), np.int64)
    for i in range(len(trip_reads)):
        for x, arr in ((0, seq), (1, rseq)):
            for _, level in W.primary_hits(olib, oix.bwt(x), arr[off[i]:off[i + 1]]):
                seen[x, level] += 1
    print("intervals that hold the primary row, by index and level 1..8:", seen[:, 1:].tolist())
    assert (seen[:, 1:] >= 1).all(), seen[:, 1:].tolist()


@pytest.mark.parametrize("quads", ["1", "0"])
@pytest.mark.parametrize("kt", [None, 2, 3, 5, 6, 7])
def test_table_trips_match_bwt_cal_width(monkeypatch, index_of, olib, oix, trip_reads, kt, quads):
    monkeypatch.setenv("NABWA_W_QUADS", quads)
    ix = index_of(kt)
    opt = T.default_opt()
    batches = [trip_reads] + [[s for s in trip_reads if len(s) == L] for L in EQUAL_LENGTHS]
    for sync in ("0", "1"):
        monkeypatch.setenv("NABWA_W_SYNC", sync)
        for reads in batches:
            seq, rseq, off = W.as_batch(reads)
            T.check_width_records(nabwa, ix, to_gap_opt(opt), opt, olib, oix.bwt, seq, rseq, off)


# ------------------------------------------------------------------ text mode, left at every place of a window

def one_row_from(olib, bwt_ptr, s):
    """(restarts, first position at which the pass over the codes s has narrowed to one row) by the oracle"""
    olib.orc_cal_width.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    ow = np.zeros(len(s) + 1, np.uint32); ob = np.zeros(len(s) + 1, np.int32)
    s = np.ascontiguousarray(s)
    olib.orc_cal_width(bwt_ptr, len(s), T.ptr(s), T.ptr(ow), T.ptr(ob))
    one = np.flatnonzero(ow[:len(s)] == 1)
    return int(ob[len(s) - 1]), (int(one[0]) if len(one) else len(s))


def broken_runs(olib, oix, read, seed_len):
    """the read with one substitution, and with one N, at each of the 32 positions after the point where the pass of the strand
    that occurs -- the full pass, and the seed pass -- has become one row: text mode ends at every place inside a window"""
    seq, rseq, _ = W.as_batch([read])
    L, out = len(read), []
    for x, arr in ((0, seq), (1, rseq)):
        restarts, i0 = one_row_from(olib, oix.bwt(x), arr)
        if restarts:
            continue
        starts = [(0, i0)]      # (consumption index of the pass's first symbol, its one-row point)
        if L > seed_len:
            starts.append((L - seed_len, one_row_from(olib, oix.bwt(x), arr[L - seed_len:])[1]))
        for base, one in starts:
            for j in range(1, 33):
                i = base + one + j      # consumption index in the whole read: read position L - 1 - i
                if i >= L:
                    break
                p = L - 1 - i
                out.append(read[:p] + "ACGT"[("ACGT".index(read[p]) + 1 + j % 3) % 4] + read[p + 1:])
                out.append(W.with_n(read, p))
    return out


@pytest.mark.parametrize("seed_len", [20, 32, 35])
def test_text_mode_left_at_any_alignment_matches_bwt_cal_width(monkeypatch, index_of, olib, oix, seed_len):
    rng = np.random.default_rng(77 + seed_len)
    text = "".join(W.toy_contigs())
    N = len(text)
    reads = []
    for L in list(range(17, 49)) + [100, 101]:      # exact occurrences, shorter and longer than the seed
        for r in range(3):
            p = int(rng.integers(41, N - L - 41))
            reads.append(text[p:p + L] if r < 2 else W.revcomp(text[p:p + L]))
    for L, rc in ((100, False), (100, True), (48, False)):
        for _ in range(200):      # (the toy genome has repeats: a read whose pass becomes one row within 16 symbols)
            p = int(rng.integers(41, N - L - 41))
            s = W.revcomp(text[p:p + L]) if rc else text[p:p + L]
            seq, rseq, _ = W.as_batch([s])
            restarts, one = one_row_from(olib, oix.bwt(int(rc)), rseq if rc else seq)
            if "N" not in s and restarts == 0 and one <= 16:
                break
        got = broken_runs(olib, oix, s, seed_len)
        assert len(got) >= 64, "no base read that occurs once"
        reads += got
    # occurrences that start within the first 40 bases of the indexed text: the walk to the left meets text position 0, and the
    # bulk trip's 16 bases to the left are not there.  (Strand 1 walks the reversed text: the genome's last bases, read reversed.)
    for s0 in (0, 1, 5, 15, 16, 17, 31, 32, 33, 39):
        for L in (33, 48, 100):
            reads.append(text[s0:s0 + L])
            reads.append(W.revcomp(text[N - s0 - L:N - s0]))
    for L in (33, 48, 100):
        reads.append("ACGTACGT" + text[:L - 8])
        reads.append(W.revcomp(text[N - (L - 8):] + "ACGTACGT"))
    opt = T.default_opt()
    opt.seed_len = seed_len
    seq, rseq, off = W.as_batch(reads)
    for quads in ("1", "0"):
        monkeypatch.setenv("NABWA_W_QUADS", quads)
        T.check_width_records(nabwa, index_of(None), to_gap_opt(opt), opt, olib, oix.bwt, seq, rseq, off)


# ------------------------------------------------------------------ reads handed on

def test_handed_on_reads_rebuild_their_widths(monkeypatch, index_of, olib, oix):
    """NABWA_TRIP_BUDGET=50 hands many searches on to kernel D: kernel W runs again over their records (rebuild_widths), without
    lockstep; rows and max_entries are the oracle's"""
    monkeypatch.setenv("NABWA_TRIP_BUDGET", "50")
    opt, _ = T.read_sai(os.path.join(T.GOLDEN, "se_default.sai"))
    reads = T.read_fastq(os.path.join(T.GOLDEN, "reads_se.fq"))[:300]
    seq, rseq, off, _ = T.encode_reads(reads, opt.trim_qual)
    b = nabwa.Batch(index_of(None), to_gap_opt(opt), seq, rseq, off, False)
    try:
        b.run()
        n_deep = b.sync()
        got, maxe = b.fetch()
    finally:
        b.close()
    assert n_deep > 0, "no search was handed on"
    want, wmaxe = T.oracle_cal_sa_reg_gap(olib, oix.h, opt, seq, rseq, off)
    bad = [reads[i][0] for i in range(len(reads)) if got[i].tobytes() != want[i].tobytes()]
    assert not bad, bad[:5]
    assert np.array_equal(np.asarray(maxe)[:len(wmaxe)], wmaxe)
