"""NABWA_DEDUP=1: a search batch finds its equal reads on the device and searches each distinct read once.  What the caller sees must be byte
for byte what it sees with the switch off.  Every case here runs the same batch with the variable unset and with 1 and compares fetch_flat()
(counts, rows, max_entries), checksum() and the width records; and every case asserts, through dedup_stats(), that the stage ran and searched
exactly the distinct reads a Python set of (length, seq bytes, rseq bytes) counts -- a case cannot pass with the stage silently off."""
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


# ---------------------------------------------------------------------------------------------------------------- running a batch
def width_records(b, seq, off, seed_len):
    """kernel W's records of all reads, with everything beyond a read's own len + 1 (seed_len + 1) columns zeroed: those are not written"""
    n = len(off) - 1
    lens = np.diff(off).astype(np.int64)
    max_len = int(lens.max()) if n else 0
    Wd, SW = max_len + 1, seed_len + 1
    w = np.zeros((max(n, 1), 2, Wd), np.uint32); bid = np.zeros((max(n, 1), 2, Wd), np.uint8); sbid = np.zeros((max(n, 1), 2, SW), np.uint8)
    L = nabwa.lib()
    L.nabwa_batch_width_records.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert L.nabwa_batch_width_records(b._h, 0, n, T.ptr(w), T.ptr(bid), T.ptr(sbid)) == 0, L.nabwa_last_error()
    if n == 0:
        return b"", b"", b""
    keep = (np.arange(Wd)[None, None, :] <= lens[:, None, None]) & (lens > 0)[:, None, None]      # (kernel W leaves an empty read's record alone)
    w, bid = np.where(keep, w[:n], 0), np.where(keep, bid[:n], 0)
    sbid = np.where((lens > seed_len)[:, None, None], sbid[:n], 0) if max_len > seed_len else np.zeros(0, np.uint8)
    return w.tobytes(), bid.tobytes(), sbid.tobytes()


def run_batch(ix, o, seq, rseq, off, per_read=False, widths=True):
    b = nabwa.Batch(ix, M.gap_opt(o), seq, rseq, off, per_read=per_read)
    try:
        b.run()
        n2 = b.sync()
        n_aln, rows, maxe = b.fetch_flat()
        cks = b.checksum()
        assert cks == M.host_checksum(n_aln, rows)
        return dict(n_aln=n_aln.copy(), rows=rows.tobytes(), maxe=maxe.copy(), cks=cks, n2=n2, cfg=b.config(), stats=b.dedup_stats(),
                    width=width_records(b, seq, off, o.seed_len) if widths else None)
    finally:
        b.close()


def same_results(a, b, what=""):
    assert np.array_equal(a["n_aln"], b["n_aln"]), what
    assert np.array_equal(a["maxe"], b["maxe"]), what
    assert a["rows"] == b["rows"], what
    assert a["cks"] == b["cks"], what
    assert a["width"] == b["width"], what
    for f in ("n", "min_len", "max_len", "deep_only", "w_sync"):
        assert a["cfg"][f] == b["cfg"][f], (what, f)


def off_and_on(mp, ix, o, seq, rseq, off, per_read=False, bits=None, what="", widths=True):
    """the batch with NABWA_DEDUP unset and with 1 -> the results with 1, after the comparison and the assertions every case makes"""
    n = len(off) - 1
    mp.delenv("NABWA_DEDUP", raising=False)
    mp.delenv("NABWA_DEDUP_HASH_BITS", raising=False)
    plain = run_batch(ix, o, seq, rseq, off, per_read, widths)
    assert plain["stats"] == [n, n, 0, 0], what
    mp.setenv("NABWA_DEDUP", "1")
    if bits is not None:
        mp.setenv("NABWA_DEDUP_HASH_BITS", str(bits))
    on = run_batch(ix, o, seq, rseq, off, per_read, widths)
    mp.delenv("NABWA_DEDUP")
    mp.delenv("NABWA_DEDUP_HASH_BITS", raising=False)
    same_results(plain, on, what)
    st = on["stats"]
    assert st[0] == n and st[3] == 1, (what, st)
    if bits is None:
        assert st[1] == D.n_distinct(seq, rseq, off), (what, st)
        assert st[2] == 0, (what, st)                  # no two distinct reads of these fixed inputs share a 64-bit hash (tests/test_dedup_emu.py)
    return on


def per_read_rows(res):
    bnd = np.concatenate([[0], np.cumsum(res["n_aln"])]) * 16
    return [res["rows"][bnd[i]:bnd[i + 1]] for i in range(len(res["n_aln"]))]


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


def enc(toy, ids):
    return M.encode([toy.reads[i] for i in ids])


# ---------------------------------------------------------------------------------------------------------------- 1. the mixed pool
@pytest.mark.parametrize("per_read", [False, True])
@pytest.mark.parametrize("name", ["default", "adna", "n3"])
def test_mixed_pool_with_every_read_one_to_five_times(toy, monkeypatch, name, per_read):
    """exact, 2 % errors, ancient-DNA-like, all-N, empty, poly-T, tandem repeats and 250 - 600 bp reads, each 1..5 times, shuffled: more than
    half of the batch is duplicates.  Under the ancient-DNA options the searches go through kernel D.  Every read's rows are the oracle's."""
    o = M.opt_block(name)
    ids = D.mixed_batch(len(toy.reads))
    assert len(ids) >= 2 * len(toy.reads) and len(set(ids)) == len(toy.reads)
    on = off_and_on(monkeypatch, toy.ix, o, *enc(toy, ids), per_read=per_read, what=name)
    assert on["stats"][1] == len(toy.reads)
    if name == "adna":
        assert on["n2"] > 0                                    # kernel D had work, and no more of it than there are distinct reads
    assert on["n2"] <= len(toy.reads)
    M.check(toy.orc, name, o, per_read, ids, per_read_rows(on), on["maxe"], "mixed pool, %s" % name)


# ---------------------------------------------------------------------------------------------------------------- 2. shapes
def test_batches_of_no_read_one_read_and_two_equal_reads(toy, monkeypatch):
    o = M.opt_block("default")
    a = toy.of("err100")[0]
    empty = (np.zeros(0, np.uint8), np.zeros(0, np.uint8), np.zeros(1, np.int64))
    on = off_and_on(monkeypatch, toy.ix, o, *empty, what="n = 0")
    assert on["stats"] == [0, 0, 0, 1]
    on = off_and_on(monkeypatch, toy.ix, o, *enc(toy, [a]), what="n = 1")
    assert on["stats"] == [1, 1, 0, 1]
    on = off_and_on(monkeypatch, toy.ix, o, *enc(toy, [a, a]), what="n = 2")
    assert on["stats"] == [2, 1, 0, 1] and on["n_aln"][0] == on["n_aln"][1]


@pytest.mark.parametrize("times", [63, 64, 65, 257, 4097])
def test_one_read_many_times(toy, monkeypatch, times):
    """one read filling part of a wave, a wave, a wave and one, several blocks: one search"""
    o = M.opt_block("default")
    a = toy.of("err100", "polyT")[times % 7]
    on = off_and_on(monkeypatch, toy.ix, o, *enc(toy, [a] * times), what="x %d" % times)
    assert on["stats"] == [times, 1, 0, 1]
    M.check(toy.orc, "default", o, False, [a] * times, per_read_rows(on), on["maxe"], "one read %d times" % times)


def test_no_duplicates_and_first_read_duplicated_by_the_last(toy, monkeypatch):
    o = M.opt_block("default")
    ids = [i for i in range(len(toy.reads))]
    on = off_and_on(monkeypatch, toy.ix, o, *enc(toy, ids), what="all distinct")
    assert on["stats"] == [len(ids), len(ids), 0, 1]           # nothing to merge: the batch of the switch off
    ids = ids + [ids[0]]
    on = off_and_on(monkeypatch, toy.ix, o, *enc(toy, ids), what="first = last")
    assert on["stats"] == [len(ids), len(ids) - 1, 0, 1]
    M.check(toy.orc, "default", o, False, ids, per_read_rows(on), on["maxe"], "first = last")


def test_longest_read_as_a_duplicate_and_as_the_only_read_of_its_length(toy, monkeypatch):
    """per_read = 0: the longest read's max_diff sizes the whole batch's option block, whether it is searched as itself or as a copy"""
    o = M.opt_block("default")
    long_ = toy.of("long600")[0]
    short = toy.of("err100")[:6] + toy.of("adna")[:6]
    assert len(toy.reads[long_]) == 600 and all(len(toy.reads[i]) < 600 for i in short)
    for what, ids in (("longest twice", short[:4] + [long_] + short[4:] + [long_]),
                      ("longest once, the others twice", short + [long_] + short)):
        on = off_and_on(monkeypatch, toy.ix, o, *enc(toy, ids), per_read=False, what=what)
        assert on["stats"][1] == len(short) + 1 and on["cfg"]["max_len"] == 600
        M.check(toy.orc, "default", o, False, ids, per_read_rows(on), on["maxe"], what)


# ---------------------------------------------------------------------------------------------------------------- 3. near-duplicates
def test_near_duplicates_stay_apart(toy, monkeypatch):
    """the same seq under another rseq, a read and its one-base extension, reads that differ in the first byte only and in the last byte only,
    at lengths around every chunk boundary and at odd byte offsets: each is searched itself; only the exact copies merge"""
    seq, rseq, off = D.near_duplicates()
    n = len(off) - 1
    assert n == 7 * len(D.NEAR_LENS)
    want = D.n_distinct(seq, rseq, off)
    assert n - 2 * len(D.NEAR_LENS) <= want <= n - len(D.NEAR_LENS)      # the copies go; the junk reads in front of the groups may coincide
    on = off_and_on(monkeypatch, toy.ix, M.opt_block("default"), seq, rseq, off, what="near-duplicates")
    assert on["stats"] == [n, want, 0, 1]


# ---------------------------------------------------------------------------------------------------------------- 5. the collision path
@pytest.mark.parametrize("bits", [0, 1, 4])
def test_reads_that_share_a_hash_and_differ_are_searched_themselves(toy, monkeypatch, bits):
    """NABWA_DEDUP_HASH_BITS keeps the low 0, 1, 4 bits of the hash: distinct reads share runs, the byte comparison keeps them apart"""
    o = M.opt_block("default")
    ids = D.mixed_batch(len(toy.reads))
    seq, rseq, off = enc(toy, ids)
    on = off_and_on(monkeypatch, toy.ix, o, seq, rseq, off, bits=bits, what="%d hash bits" % bits)
    st = on["stats"]
    keys = D.keys_of(seq, rseq, off)
    assert D.n_distinct(seq, rseq, off) <= st[1] <= len(ids) and st[2] > 0
    if bits == 0:                                              # one run: its first read is read 0, and only read 0's copies merge
        assert st[1] == 1 + sum(k != keys[0] for k in keys) and st[2] == st[1] - 1
    M.check(toy.orc, "default", o, False, ids, per_read_rows(on), on["maxe"], "%d hash bits" % bits)


# ---------------------------------------------------------------------------------------------------------------- 6. wide hit lists
def test_duplicates_whose_rows_lie_in_the_wide_hit_lists(toy, monkeypatch):
    """NABWA_ALNCAP1=1: every read of two or more rows ends in the wide lists (kernel D).  The golden single-end reads, of which some
    thirty have several rows, each twice, with duplicated poly-T and tandem reads among them"""
    monkeypatch.setenv("NABWA_ALNCAP1", "1")
    o = M.opt_block("default")
    gold = [s for _, s, _ in T.read_fastq(os.path.join(T.GOLDEN, "reads_se.fq"))]
    reads = [toy.reads[i] for i in toy.of("polyT", "tandem")] + gold
    orc = M.Oracle(toy.olib, toy.oix.h, reads)
    ids = list(range(len(reads))) + list(range(len(reads)))[::-1]
    on = off_and_on(monkeypatch, toy.ix, o, *M.encode([reads[i] for i in ids]), what="wide lists")
    n_wide = int((on["n_aln"][: len(reads)] >= 2).sum())
    assert n_wide >= 10 and on["n2"] >= n_wide                 # reads of several rows, each in the batch twice, went through kernel D once
    M.check(orc, "default", o, False, ids, per_read_rows(on), on["maxe"], "wide lists")


# ---------------------------------------------------------------------------------------------------------------- 7. capacity, bad values
def test_fetch_with_too_few_rows_and_values_the_library_refuses(toy, monkeypatch):
    o = M.opt_block("default")
    ids = D.mixed_batch(len(toy.reads))[:300]
    seq, rseq, off = enc(toy, ids)
    on = off_and_on(monkeypatch, toy.ix, o, seq, rseq, off, what="capacity")
    total = int(on["n_aln"].sum())
    assert total > 1
    monkeypatch.setenv("NABWA_DEDUP", "1")
    b = nabwa.Batch(toy.ix, M.gap_opt(o), seq, rseq, off)
    try:
        b.run()
        b.sync()
        n_aln = np.full(len(ids), -1, np.int32); maxe = np.zeros(len(ids), np.int32)
        buf = np.zeros(total, nabwa.ALN_DT)
        rows = C.c_int64(-1)
        rc = nabwa.lib().nabwa_batch_fetch(b._h, T.ptr(n_aln), T.ptr(buf), total - 1, C.byref(rows), T.ptr(maxe))
        assert rc == nabwa.ECAP and rows.value == total and np.array_equal(n_aln, on["n_aln"]) and np.array_equal(maxe, on["maxe"])
        assert b.dedup_stats()[1] < len(ids)
    finally:
        b.close()
    for bad in ("2", "gpu", "", "01"):
        monkeypatch.setenv("NABWA_DEDUP", bad)
        with pytest.raises(nabwa.NabwaError) as e:
            nabwa.Batch(toy.ix, M.gap_opt(o), seq, rseq, off)
        assert e.value.code == nabwa.EINVAL and "NABWA_DEDUP" in str(e.value)
    monkeypatch.setenv("NABWA_DEDUP", "1")
    for bad in ("65", "-1", "x"):
        monkeypatch.setenv("NABWA_DEDUP_HASH_BITS", bad)
        with pytest.raises(nabwa.NabwaError) as e:
            nabwa.Batch(toy.ix, M.gap_opt(o), seq, rseq, off)
        assert e.value.code == nabwa.EINVAL


# ---------------------------------------------------------------------------------------------------------------- 8. live batches
def test_two_live_batches_and_pooled_buffers(toy, monkeypatch):
    """a batch with duplicates and one without, both live: run A, run B, sync B, sync A.  Then a deduplicated batch closed and a plain one
    after it, which takes its pooled buffers"""
    o = M.opt_block("default")
    A = D.mixed_batch(len(toy.reads), seed=9)[:500]
    Bd = toy.of("adna", "err100", "long300")
    monkeypatch.setenv("NABWA_DEDUP", "1")
    ba = nabwa.Batch(toy.ix, M.gap_opt(o), *enc(toy, A))
    bb = nabwa.Batch(toy.ix, M.gap_opt(o), *enc(toy, Bd))
    try:
        ba.run()
        bb.run()
        bb.sync()
        gb, mb = M.collect(bb)
        ba.sync()
        ga, ma = M.collect(ba)
        assert ba.dedup_stats() == [len(A), len(set(A)), 0, 1] and bb.dedup_stats() == [len(Bd), len(Bd), 0, 1]
    finally:
        ba.close()
        bb.close()
    M.check(toy.orc, "default", o, False, A, ga, ma, "live batch A")
    M.check(toy.orc, "default", o, False, Bd, gb, mb, "live batch B")
    monkeypatch.delenv("NABWA_DEDUP")
    plain = run_batch(toy.ix, o, *enc(toy, A))
    assert plain["stats"] == [len(A), len(A), 0, 0]
    M.check(toy.orc, "default", o, False, A, per_read_rows(plain), plain["maxe"], "plain batch after a deduplicated one")


# ---------------------------------------------------------------------------------------------------------------- 9. one-call entries
def test_one_call_entries_under_the_switch(toy, monkeypatch):
    """nabwa_cal_sa_reg_gap, and nabwa_bwa_cal_sa_reg_gap on bwa_seq_t records, build their batch themselves: the variable reaches them"""
    o = M.opt_block("default")
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
        return [(C.string_at(arr[i].aln, 16 * arr[i].n_aln) if arr[i].n_aln else b"", arr[i].max_entries) for i in range(n)], keep

    got = {}
    for sw in (None, "1"):
        if sw:
            monkeypatch.setenv("NABWA_DEDUP", sw)
        else:
            monkeypatch.delenv("NABWA_DEDUP", raising=False)
        n_aln, rows, maxe = toy.ix.cal_sa_reg_gap_flat(M.gap_opt(o), seq, rseq, off)
        got[sw] = (n_aln.tobytes(), rows.tobytes(), maxe.tobytes(), records()[0])
    assert got[None] == got["1"]
    want = toy.orc.want("default", o, False, ids)
    assert np.frombuffer(got["1"][0], np.int32).tolist() == [len(w[0]) // 16 for w in want]
    assert got["1"][1] == b"".join(w[0] for w in want)
