"""tests/indexref.py, the NumPy reference the GPU tests of the index geometry rest on, pinned on the CPU:
 * its word streams equal the committed toy index (tests/golden/toy.bwt/.rbwt/.sa/.rsa) byte for byte;
 * where the compiled reference travelled (oracle/_ref/bwa_ref) they equal `bwa_ref index -a is` at every text length of the list,
   and the .pac packing equals the reference's;
 * the oracle's orc_occ4 / orc_occ / orc_sa on indexes loaded from these streams equal the reference tables on every row, at every
   length, and orc_sa under other sampling intervals;
 * where the compiled reference travelled, orc_cal_sa_reg_gap equals `bwa_ref aln` on the edge reads of every text and option set."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import indexref as R
import nabwa_testlib as T

REFBIN = os.path.join(T.ROOT, "oracle", "_ref", "bwa_ref")
need_ref = pytest.mark.skipif(not os.path.exists(REFBIN), reason="the compiled reference (oracle/_ref/bwa_ref) did not travel")


def words(path):
    return np.fromfile(path, np.uint32)


def option_block(changes):
    o = T.default_opt()
    for k, v in changes.items():
        setattr(o, k, v)
    return o


@pytest.fixture(scope="module")
def olib():
    return T.load_oracle()


def test_construction_equals_the_toy_index():
    raw = np.fromfile(T.TOY + ".pac", np.uint8)
    n = (len(raw) - 2) * 4 + int(raw[-1])
    text = ((raw[:-1, None] >> np.array([6, 4, 2, 0], np.uint8)) & 3).reshape(-1)[:n].astype(np.uint8)
    assert R.pac_bytes(text) == raw.tobytes()
    ix = R.RefIndex(text)
    for ext, w in zip(("bwt", "rbwt", "sa", "rsa"), ix.streams(32)):
        assert w.tobytes() == open("%s.%s" % (T.TOY, ext), "rb").read(), ext
    assert sorted(ix.d[0].sa.tolist()) == list(range(n + 1))


def test_the_texts_have_the_properties_they_are_named_for():
    for n in R.SPECIAL_LENGTHS:
        assert R.RefDir(R.homopolymer(n)).primary == n and R.RefDir(R.a_then_c(n)).primary == 1
        t = R.tandem(n)
        assert (t[8:] == t[:-8]).all() and not any((t[p:] == t[:-p]).all() for p in range(1, 8))
    for (mod, res), seed in R.PRIMARY_SEEDS.items():
        assert R.RefDir(R.random_text(1000, seed)).primary % mod == res, (mod, res)
    assert [R.table_depth(n) for n in (1, 3, 4, 15, 16, 63, 64, 1000, 1024, 103000)] == [1, 1, 2, 2, 3, 3, 4, 5, 6, 9]


def test_tables_agree_with_a_direct_count():
    """occ and the intervals restated naively on a small text: counts of the last column, rows by string comparison"""
    text = R.random_text(65)
    d = R.RefDir(text)
    s = "".join("ACGT"[c] for c in text)
    suf = sorted(range(66), key=lambda i: s[i:])      # Python compares a shorter string as smaller: '$' first
    assert suf == d.sa.tolist()
    col = [s[i - 1] if i else "$" for i in suf]
    for k in range(-1, 66):
        assert d.occ[k + 1].tolist() == [col[:k + 1].count(c) for c in "ACGT"]
    for t in (1, 2, 3):
        kk, ll = d.kmer(t)
        for key in range(4 ** t):
            p = "".join("ACGT"[key >> (2 * j) & 3] for j in range(t))
            rows = [r for r in range(66) if s[suf[r]:].startswith(p)]
            if rows:
                assert (int(kk[key]), int(ll[key])) == (rows[0], rows[-1]) and rows == list(range(rows[0], rows[-1] + 1))
            else:
                assert kk[key] > ll[key]


@need_ref
@pytest.mark.parametrize("n", R.LENGTHS)
def test_construction_equals_the_compiled_reference(tmp_path, n):
    text = R.random_text(n)
    fa = str(tmp_path / "t.fa")
    open(fa, "w").write(R.fasta(text))
    pre = str(tmp_path / "ref")
    r = subprocess.run([REFBIN, "index", "-a", "is", "-p", pre, fa], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    for ext, w in zip(("bwt", "rbwt", "sa", "rsa"), R.RefIndex(text).streams(32)):
        assert w.tobytes() == open("%s.%s" % (pre, ext), "rb").read(), (n, ext)
    assert R.pac_bytes(text) == open(pre + ".pac", "rb").read()
    assert R.pac_bytes(text[::-1]) == open(pre + ".rpac", "rb").read()


def check_oracle_rows(olib, tmp_path, text, intv):
    ix = R.RefIndex(text)
    pre = str(tmp_path / ("o%d_%d" % (len(text), intv)))
    ix.write(pre, intv)
    h = olib.orc_index_load(pre.encode(), 1, 0)
    cnt = np.zeros(4, np.uint32)
    n = ix.n
    try:
        for t in (0, 1):
            d = ix.d[t]
            b = C.c_void_p(h + t * T.OracleIndex.BWT_SIZE)
            for k in list(range(n + 1)) + [0xffffffff]:
                olib.orc_occ4(b, k, T.ptr(cnt))
                want = d.occ[0 if k == 0xffffffff else k + 1]
                assert cnt.tolist() == want.tolist(), (n, t, k)
                assert [olib.orc_occ(b, k, c) for c in range(4)] == want.tolist(), (n, t, k)
            got = [olib.orc_sa(b, k) for k in range(n + 1)]
            assert got == [0xffffffff] + d.sa[1:].tolist(), (n, t, intv)
    finally:
        olib.orc_index_free(C.c_void_p(h))


@pytest.mark.parametrize("n", R.LENGTHS)
def test_oracle_rank_and_sa_on_every_row(olib, tmp_path, n):
    check_oracle_rows(olib, tmp_path, R.random_text(n), 32)


@pytest.mark.parametrize("n", R.SPECIAL_LENGTHS)
def test_oracle_rank_and_sa_on_the_special_texts(olib, tmp_path, n):
    for text in (R.homopolymer(n), R.a_then_c(n), R.tandem(n)):
        check_oracle_rows(olib, tmp_path, text, 32)
    for intv in (1, 33, n, n + 1):
        check_oracle_rows(olib, tmp_path, R.random_text(n), intv)


@need_ref
@pytest.mark.parametrize("name", [x[0] for x in R.search_texts()])
def test_oracle_search_equals_the_compiled_reference_on_the_edge_reads(olib, tmp_path, name):
    text, short = next((t, s) for nm, t, s in R.search_texts() if nm == name)
    reads = R.edge_reads(text, short=short)
    assert len(reads) >= (60 if short else 400)
    pre = str(tmp_path / "ix")
    ix = R.RefIndex(text)
    ix.write(pre)
    fq = str(tmp_path / "reads.fq")
    open(fq, "w").write(R.fastq(reads))
    seq, rseq, off = R.encode(reads)
    h = olib.orc_index_load(pre.encode(), 1, 0)
    try:
        for oname, args, changes in R.OPTION_SETS:
            sai = str(tmp_path / (oname + ".sai"))
            with open(sai, "wb") as f:
                r = subprocess.run([REFBIN, "aln"] + args + [pre, fq], stdout=f, stderr=subprocess.PIPE, timeout=300)
            assert r.returncode == 0, r.stderr.decode(errors="replace")
            opt, gold = T.read_sai(sai)
            assert bytes(opt) == bytes(option_block(changes)), oname          # the option block the GPU tests use is `bwa aln`'s
            assert len(gold) == len(reads)
            want, _ = T.oracle_cal_sa_reg_gap(olib, h, opt, seq, rseq, off)
            bad = [i for i in range(len(reads)) if want[i].tobytes() != gold[i].tobytes()]
            assert not bad, "%s, %s: the oracle differs from the reference for %d reads, e.g. %d" % (name, oname, len(bad), bad[0])
            if not short:
                assert sum(len(g) > 0 for g in gold) > len(reads) // 2
    finally:
        olib.orc_index_free(C.c_void_p(h))
