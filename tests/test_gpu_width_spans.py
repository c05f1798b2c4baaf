"""Kernel W's trips that finish several positions at once and append their outputs as values -- text runs of up to 16 positions at
any alignment in both passes (NABWA_W_RUNS), table trips of up to 8 levels that may end a pass (NABWA_W_TRIP8) -- on the toy index:
the width records against the oracle's bwt_cal_width, every case with each knob on and off and with NABWA_W_SYNC 0 and 1."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import nabwa_testlib as T
import width_cases as W

pytestmark = pytest.mark.gpu
nabwa = importlib.import_module("network-aware-bwa_amd")

KNOBS = ("NABWA_W_RUNS", "NABWA_W_TRIP8")
# both on (the default), both off (the trips before them), each alone
SETTINGS = [(1, 1), (0, 0), (1, 0), (0, 1)]
SETTING_IDS = ["both", "none", "runs", "trip8"]


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


def set_knobs(monkeypatch, setting):
    for name, v in zip(KNOBS, setting):
        monkeypatch.setenv(name, str(v))


def check(monkeypatch, ix, opt, olib, oix, reads, equal_lengths=()):
    """the records of the whole batch without lockstep, and of its equal-length sub-batches with NABWA_W_SYNC 0 and 1"""
    monkeypatch.setenv("NABWA_W_SYNC", "1")
    seq, rseq, off = W.as_batch(reads)
    T.check_width_records(nabwa, ix, to_gap_opt(opt), opt, olib, oix.bwt, seq, rseq, off)
    for L in equal_lengths:
        sub = [s for s in reads if len(s) == L]
        assert sub, L
        seq, rseq, off = W.as_batch(sub)
        for sync in ("0", "1"):
            monkeypatch.setenv("NABWA_W_SYNC", sync)
            T.check_width_records(nabwa, ix, to_gap_opt(opt), opt, olib, oix.bwt, seq, rseq, off)


def cal_width(olib, bwt_ptr, s):
    """(widths, bids) of the oracle's bwt_cal_width over the codes s, positions 0 .. len(s)"""
    olib.orc_cal_width.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    ow = np.zeros(len(s) + 1, np.uint32); ob = np.zeros(len(s) + 1, np.int32)
    s = np.ascontiguousarray(s)
    olib.orc_cal_width(bwt_ptr, len(s), T.ptr(s), T.ptr(ow), T.ptr(ob))
    return ow, ob


# ------------------------------------------------------------------ table trips

@pytest.fixture(scope="module")
def trip_reads():
    """reads whose first restart falls on each of the first 24 positions of a pass (every place of an 8-level trip, three trips
    deep), on either strand and in the seed pass too; reads that put the primary row into an interval of every level; and the
    restart followed by a second pattern, so that trips begin at every position"""
    rng = np.random.default_rng(2015)
    text = "".join(W.toy_contigs())
    N = len(text)
    reads = []
    for L in (33, 40, 100):
        for j in range(24):
            for rc in (False, True):
                p = int(rng.integers(41, N - L - 41))
                s = text[p:p + L]
                # strand 0 consumes the read from its end: a foreign base j places before the end breaks the pattern there at the latest
                for at in (L - 1 - j, max(0, L - 33 - j)):
                    t = s[:at] + "ACGT"[("ACGT".index(s[at]) + 1 + j % 3) % 4] + s[at + 1:]
                    reads.append(W.revcomp(t) if rc else t)
    for i in range(120):
        L = (33, 40, 100)[i % 3]
        reads.append("".join("ACGT"[x] for x in rng.integers(0, 4, L)))
    reads += W.primary_tail_reads(rng, text)
    return reads


def test_the_trip_reads_restart_at_every_place_and_hold_the_primary_row_at_every_level(trip_reads, olib, oix):
    """by the oracle alone: on either index, in reads without an N, a restart falls at every level 7..14 of its pattern (level =
    symbols since the last restart) -- a trip begins at level 1 or 9 of a pattern, so with tables of depth 8..14 these are all 8
    places of a trip (the toy text of 103 kb has every pattern of 6 symbols: no restart below level 7) -- and at every level 1..8
    an interval of the batch holds the primary row at an inner position.  Without these a wrong clamp or correction would go unseen"""
    seq, rseq, off = W.as_batch(trip_reads)
    died = np.zeros((2, 17), np.int64); seen = np.zeros((2, 9), np.int64)
    for i in range(len(trip_reads)):
        for x, arr in ((0, seq), (1, rseq)):
            s = arr[off[i]:off[i + 1]]
            if (s > 3).any():
                continue
            _, ob = cal_width(olib, oix.bwt(x), s)
            at = np.flatnonzero(np.diff(ob[:len(s)]) > 0) + 1      # positions whose symbol restarted the pass
            if ob[0] > 0:
                at = np.concatenate([[0], at])
            start = 0
            for p in at:
                died[x, min(int(p) - start + 1, 16)] += 1
                start = int(p) + 1
            for _, level in W.primary_hits(olib, oix.bwt(x), s):
                seen[x, level] += 1
    print("restarts by level 1..16+:", died[:, 1:].tolist())
    print("intervals that hold the primary row, by index and level 1..8:", seen[:, 1:].tolist())
    assert (died[:, 7:15] >= 1).all(), died[:, 1:].tolist()
    assert (seen[:, 1:] >= 1).all(), seen[:, 1:].tolist()


@pytest.mark.parametrize("setting", SETTINGS, ids=SETTING_IDS)
@pytest.mark.parametrize("kt", [8, 9, 12, 14, 16])
def test_table_trips_match_bwt_cal_width(monkeypatch, index_of, olib, oix, trip_reads, kt, setting):
    """(a table of depth 16 is 46 GB per index whatever the text: in its place the depth the library picks for the toy index)"""
    set_knobs(monkeypatch, setting)
    for quads in ("1", "0"):
        monkeypatch.setenv("NABWA_W_QUADS", quads)
        check(monkeypatch, index_of(None if kt == 16 else kt), T.default_opt(), olib, oix, trip_reads, (33, 40, 100))


# ------------------------------------------------------------------ pass ends

@pytest.fixture(scope="module")
def end_reads():
    """every read length 1..48, 64 and 100 -- as an occurrence on either strand and as random bases -- and the same with an N at
    the first and at the last consumed position of either strand's pass"""
    rng = np.random.default_rng(404)
    text = "".join(W.toy_contigs())
    N = len(text)
    reads = []
    for L in list(range(1, 49)) + [64, 100]:
        for r in range(4):
            p = int(rng.integers(41, N - L - 41))
            s = text[p:p + L]
            s = (s, W.revcomp(s), s[::-1], "".join("ACGT"[x] for x in rng.integers(0, 4, L)))[r]
            reads.append(s)
            if r < 2:
                reads.append(W.with_n(s, 0))
                reads.append(W.with_n(s, L - 1))
    return reads


@pytest.mark.parametrize("setting", SETTINGS, ids=SETTING_IDS)
@pytest.mark.parametrize("seed_len", [20, 32, 35])
def test_pass_ends_match_bwt_cal_width(monkeypatch, index_of, olib, oix, end_reads, seed_len, setting):
    """a pass ends inside a table trip, inside a text run and in a single step: len == seed_len and len == seed_len + 1 are among
    the lengths"""
    set_knobs(monkeypatch, setting)
    opt = T.default_opt()
    opt.seed_len = seed_len
    check(monkeypatch, index_of(None), opt, olib, oix, end_reads, (seed_len, seed_len + 1, 48, 100))
    check(monkeypatch, index_of(9), opt, olib, oix, end_reads, (seed_len + 1,))


# ------------------------------------------------------------------ text runs

def one_row_from(olib, bwt_ptr, s):
    """(restarts, first position at which the pass over the codes s has narrowed to one row) by the oracle"""
    ow, ob = cal_width(olib, bwt_ptr, s)
    one = np.flatnonzero(ow[:len(s)] == 1)
    return int(ob[len(s) - 1]), (int(one[0]) if len(one) else len(s))


def broken_runs(olib, oix, read, seed_len):
    """the read with one substitution, and with one N, at each of the 32 positions after the point where the pass of the strand
    that occurs -- the full pass, and the seed pass -- has become one row: a run ends at every place inside a window"""
    seq, rseq, _ = W.as_batch([read])
    L, out = len(read), []
    for x, arr in ((0, seq), (1, rseq)):
        restarts, i0 = one_row_from(olib, oix.bwt(x), arr)
        if restarts:
            continue
        starts = [(0, i0)]
        if L > seed_len:
            starts.append((L - seed_len, one_row_from(olib, oix.bwt(x), arr[L - seed_len:])[1]))
        for base, one in starts:
            for j in range(1, 33):
                i = base + one + j
                if i >= L:
                    break
                p = L - 1 - i
                out.append(read[:p] + "ACGT"[("ACGT".index(read[p]) + 1 + j % 3) % 4] + read[p + 1:])
                out.append(W.with_n(read, p))
    return out


@pytest.fixture(scope="module")
def run_reads(olib, oix):
    def make(seed_len):
        rng = np.random.default_rng(91 + seed_len)
        text = "".join(W.toy_contigs())
        N = len(text)
        reads = []
        for L in list(range(17, 49)) + [100, 101]:      # exact occurrences: their runs end exactly at n, in both passes
            for r in range(3):
                p = int(rng.integers(41, N - L - 41))
                reads.append(text[p:p + L] if r < 2 else W.revcomp(text[p:p + L]))
        for L, rc in ((100, False), (100, True), (48, False)):
            for _ in range(200):
                p = int(rng.integers(41, N - L - 41))
                s = W.revcomp(text[p:p + L]) if rc else text[p:p + L]
                seq, rseq, _ = W.as_batch([s])
                restarts, one = one_row_from(olib, oix.bwt(int(rc)), rseq if rc else seq)
                if "N" not in s and restarts == 0 and one <= 16:
                    break
            got = broken_runs(olib, oix, s, seed_len)
            assert len(got) >= 64, "no base read that occurs once"
            reads += got
        # occurrences that begin within the first 40 bases of either text: the run is clamped by the text that is left
        for s0 in (0, 1, 5, 15, 16, 17, 31, 32, 33, 39):
            for L in (33, 48, 100):
                reads.append(text[s0:s0 + L])
                reads.append(W.revcomp(text[N - s0 - L:N - s0]))
        for L in (33, 48, 100):
            reads.append("ACGTACGT" + text[:L - 8])
            reads.append(W.revcomp(text[N - (L - 8):] + "ACGTACGT"))
        return reads
    cache = {}
    return lambda seed_len: cache.setdefault(seed_len, make(seed_len))


def one_stretches(ow, n):
    """the stretches [a, b] of positions < n whose width is 1, by the oracle's widths"""
    out, a = [], None
    for p in range(n + 1):
        if p < n and ow[p] == 1:
            a = p if a is None else a
        elif a is not None:
            out.append((a, p - 1)); a = None
    return out


@pytest.mark.parametrize("seed_len", [20, 32, 35])
def test_the_run_reads_hold_the_runs_the_cases_need(olib, oix, run_reads, seed_len):
    """by the oracle alone, over the reads as generated.  A pass is one row from the first position a of a stretch of width 1, in text
    mode from a + 1, and its first run can begin at a + 2.  In the full passes and in the seed passes there is: a run of 16 that
    begins off a 16-byte boundary of the bound bytes (so it crosses that one and those of the width chunks in one trip); a stretch
    that ends at every place 1..30 after its run can begin (the substitutions and Ns of broken_runs, inside every window); a run that ends exactly at
    the end of the pass.  In the full passes: a stretch that ends at the pass's end in a read that is the text from position s0 < 16
    on (the text to the left is shorter than a window), and a restart where the text has run out."""
    reads = run_reads(seed_len)
    text = "".join(W.toy_contigs())
    seq, rseq, off = W.as_batch(reads)
    cross = [0, 0]; at_end = [0, 0]; ends = [set(), set()]; short_text = 0; text_out = 0
    for i, r in enumerate(reads):
        for x, arr in ((0, seq), (1, rseq)):
            s = arr[off[i]:off[i + 1]]
            passes = [s] + ([s[len(s) - seed_len:]] if len(s) > seed_len else [])
            for ph, t in enumerate(passes):
                ow, ob = cal_width(olib, oix.bwt(x), t)
                for a, b in one_stretches(ow, len(t)):
                    if b - (a + 2) + 1 >= 16 and (a + 2) & 15:
                        cross[ph] += 1
                    if b >= a + 2:
                        ends[ph].add(b - (a + 2) + 1 if b < len(t) - 1 else 0)
                        if b == len(t) - 1 and (s <= 3).all():
                            at_end[ph] += 1
                            if ph == 0 and x == 0 and any(r == text[s0:s0 + len(r)] for s0 in range(16)):
                                short_text += 1
                    if ph == 0 and x == 0 and r.startswith("ACGTACGT") and r[8:] == text[:len(r) - 8] and b == len(r) - 9 and ob[b + 1] == ob[b] + 1:
                        text_out += 1
    print("runs off a boundary:", cross, "runs to the pass's end:", at_end, "clamped by the text:", short_text, "text run out:", text_out)
    assert cross[0] >= 1 and (cross[1] >= 1 or seed_len < 32) and min(at_end) >= 1 and short_text >= 1 and text_out >= 1      # (a seed pass of 20 has no room for a run of 16)
    for ph in (0, 1):
        want = set(range(1, 31 if ph == 0 else seed_len - 16))      # (broken_runs: the break j places after the one-row point ends a run of j - 2)
        assert want <= ends[ph], (ph, sorted(want - ends[ph]))


@pytest.mark.parametrize("setting", SETTINGS, ids=SETTING_IDS)
@pytest.mark.parametrize("seed_len", [20, 32, 35])
def test_text_runs_match_bwt_cal_width(monkeypatch, index_of, olib, oix, run_reads, seed_len, setting):
    set_knobs(monkeypatch, setting)
    opt = T.default_opt()
    opt.seed_len = seed_len
    check(monkeypatch, index_of(None), opt, olib, oix, run_reads(seed_len), (48, 100))


# ------------------------------------------------------------------ statistics

@pytest.mark.parametrize("sync", ["1", "0"])
@pytest.mark.parametrize("setting", SETTINGS, ids=SETTING_IDS)
def test_trip_statistics_add_up(monkeypatch, index_of, trip_reads, end_reads, setting, sync):
    """NABWA_W_STATS=1, the statistics instantiation: every position of every pass is counted on exactly one path, a wave-trip has at
    most 64 lane-trips, no trip takes more positions than its kind can; with the knobs off a text trip is the bulk trip -- 16
    positions, never in a seed pass -- and a table trip has at most 4 levels"""
    set_knobs(monkeypatch, setting)
    monkeypatch.setenv("NABWA_W_STATS", "1")
    monkeypatch.setenv("NABWA_W_SYNC", sync)
    opt = T.default_opt()
    L = nabwa.lib()
    L.nabwa_batch_width_records.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.nabwa_batch_w_stats.argtypes = [C.c_void_p, C.c_void_p]
    batches = [trip_reads + end_reads, [s for s in trip_reads if len(s) == 100]]
    for reads in batches:
        seq, rseq, off = W.as_batch(reads)
        lens = np.diff(off)
        b = nabwa.Batch(index_of(None), to_gap_opt(opt), seq, rseq, off, False)
        try:
            n, Wd, SW = len(reads), int(lens.max()) + 1, opt.seed_len + 1
            w = np.zeros((n, 2, Wd), np.uint32); bid = np.zeros((n, 2, Wd), np.uint8); sbid = np.zeros((n, 2, SW), np.uint8)
            assert L.nabwa_batch_width_records(b._h, 0, n, T.ptr(w), T.ptr(bid), T.ptr(sbid)) == 0, L.nabwa_last_error()
            t = np.zeros(6, np.uint64)
            assert L.nabwa_batch_w_stats(b._h, T.ptr(t)) == 0
        finally:
            b.close()
        t = [int(v) for v in t]
        wave, longest = t[0], t[1]
        text_trips, text_pos = t[2] >> 32, t[2] & 0xffffffff
        table_trips, table_pos = t[3] >> 32, t[3] & 0xffffffff
        seed_text_trips, rank_steps, other_steps = t[4] >> 32, t[4] & 0xffffffff, t[5]
        print(setting, sync, "wave-trips", wave, "longest item", longest, "text", text_trips, text_pos, "(seed passes:", seed_text_trips,
              ") table", table_trips, table_pos, "rank steps", rank_steps, "other steps", other_steps)
        want = 2 * int(sum(int(l) + (opt.seed_len if l > opt.seed_len else 0) for l in lens))
        assert text_pos + table_pos + rank_steps + other_steps == want
        lane_trips = text_trips + table_trips + rank_steps + other_steps
        assert 0 < lane_trips <= 64 * wave
        assert 1 <= longest <= wave
        runs, trip8 = setting
        assert text_trips > 0 and table_trips > 0
        if runs:
            assert text_trips <= text_pos <= 16 * text_trips and seed_text_trips > 0
        else:
            assert text_pos == 16 * text_trips and seed_text_trips == 0
        assert table_trips <= table_pos <= (8 if trip8 else 4) * table_trips
