"""Index build, load and search at the text lengths the code has branches for, on the GPU, against tests/indexref.py (a NumPy
construction pinned by tests/test_indexref_host.py) and the CPU oracle.

Texts: seeded random ones of 1..1000 bases around every block size (16 bases a word, 29-base sort keys, 32-base words of the
builder's text, 128-row checkpoint blocks, 192-row buckets, 3 buckets); A^n (primary = n), A^(n-1)C (primary = 1) and a tandem of
an 8-base unit at 192, 193, 384, 385; random texts of 1 000 bases whose primary sits on a bucket or block edge.
  builder  FASTA -> index_fa2pac -> index_build: .bwt .rbwt .sa .rsa byte-equal to the reference streams, with sa_intv 32 for every
           text and 1, 2, 31, 33, 64, 192, n, n + 1 at four lengths; .pac / .rpac equal a NumPy packing
  loader   Index.from_arrays on the reference streams: occ4 on every row and 0xffffffff, sa_lookup on every row with the full SA
           and by the LF walk (NABWA_TEXT_MODE=0), the exported full SA, inverse SA and text, the interval table's depth and every
           entry of its last level, both directions
  search   reads cut at the first and last bases of the text, hanging off either end, longer than the text: cal_sa_reg_gap =
           the oracle's rows byte for byte under three option sets and seven index / kernel configurations; kernel W's records =
           the oracle's bwt_cal_width"""
import ctypes as C
import importlib

import numpy as np
import pytest

import indexref as R
import nabwa_testlib as T

pytestmark = pytest.mark.gpu
nabwa = importlib.import_module("network-aware-bwa_amd")


def geometry_texts():
    out = [("random%d" % n, lambda n=n: R.random_text(n)) for n in R.LENGTHS]
    for n in R.SPECIAL_LENGTHS:
        out += [("A%d" % n, lambda n=n: R.homopolymer(n)), ("A%dC" % (n - 1), lambda n=n: R.a_then_c(n)), ("tandem%d" % n, lambda n=n: R.tandem(n))]
    out += [("primary%%%d=%d" % k, lambda s=s: R.random_text(1000, s)) for k, s in R.PRIMARY_SEEDS.items()]
    return dict(out)


TEXTS = geometry_texts()
SEARCH = {name: (text, short) for name, text, short in R.search_texts()}
_REF = {}


def ref_of(name):
    """the reference index of a text, made once"""
    if name not in _REF:
        _REF[name] = R.RefIndex(TEXTS[name]() if name in TEXTS else SEARCH[name][0])
        _REF[name].text.setflags(write=False)
    return _REF[name]


def read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def olib():
    return T.load_oracle()


def test_primary_sits_where_the_texts_are_named_for():
    for (mod, res) in R.PRIMARY_SEEDS:
        assert ref_of("primary%%%d=%d" % (mod, res)).d[0].primary % mod == res
    for n in R.SPECIAL_LENGTHS:
        assert ref_of("A%d" % n).d[0].primary == n and ref_of("A%dC" % (n - 1)).d[0].primary == 1


# ------------------------------------------------------------------ builder

def make_pac(tmp_path, ix):
    fa = str(tmp_path / "t.fa")
    with open(fa, "w") as f:
        f.write(R.fasta(ix.text))
    prefix = str(tmp_path / "t")
    assert nabwa.index_fa2pac(fa, prefix) == ix.n
    assert read(prefix + ".pac") == R.pac_bytes(ix.text)
    assert read(prefix + ".rpac") == R.pac_bytes(ix.text[::-1])
    return prefix


def assert_built(prefix, ix, intv):
    for ext, w in zip(("bwt", "rbwt", "sa", "rsa"), ix.streams(intv)):
        got = read("%s.%s" % (prefix, ext))
        assert got == w.tobytes(), "n = %d, sa_intv = %d: .%s differs (%d vs %d bytes; first word %s)" % (
            ix.n, intv, ext, len(got), w.nbytes, next((i for i, (a, b) in enumerate(zip(np.frombuffer(got[:len(got) // 4 * 4], np.uint32), w)) if a != b), None))


@pytest.mark.parametrize("name", list(TEXTS))
def test_builder_writes_the_reference_streams(tmp_path, name):
    ix = ref_of(name)
    prefix = make_pac(tmp_path, ix)
    nabwa.index_build(prefix, device=0, sa_intv=32)
    assert_built(prefix, ix, 32)


@pytest.mark.parametrize("n", R.INTV_LENGTHS)
def test_builder_under_other_sampling_intervals(tmp_path, n):
    ix = ref_of("random%d" % n)
    prefix = make_pac(tmp_path, ix)
    for intv in R.special_intvs(n):
        nabwa.index_build(prefix, device=0, sa_intv=intv)
        assert_built(prefix, ix, intv)


# ------------------------------------------------------------------ loader

def check_sa_lookup(gix, ix, what):
    rows = np.arange(1, ix.n + 1, dtype=np.uint32)
    for t in (0, 1):
        got = gix.sa_lookup(np.full(len(rows), t, np.uint8), rows).astype(np.int64)
        assert np.array_equal(got, ix.d[t].sa[1:]), (what, t, np.nonzero(got != ix.d[t].sa[1:])[0][:5].tolist())


def check_loaded(gix, ix, what):
    n = ix.n
    T_ = R.table_depth(n)
    rows = np.concatenate([np.arange(0, n + 1, dtype=np.uint32), np.array([0xffffffff], np.uint32)])
    for t in (0, 1):
        d = ix.d[t]
        assert gix.seq_len(t) == n
        want = np.concatenate([d.occ[1:], d.occ[:1]])                                      # rows 0..n, then row -1
        got = gix.occ4(t, rows).astype(np.int64)
        assert np.array_equal(got, want), (what, t, rows[np.nonzero((got != want).any(1))[0][:5]].tolist())
        sa_full = gix.export(t, 0, 0, n + 1).astype(np.int64)
        assert sa_full[0] == 0xffffffff and np.array_equal(sa_full[1:], d.sa[1:]), (what, t)      # (row 0, the empty suffix: bwt->sa[0] = -1, bwt.c:69)
        assert np.array_equal(gix.export(t, 1, 0, n + 1).astype(np.int64), d.isa), (what, t)
        assert np.array_equal(gix.export(t, 2, 0, n).astype(np.uint8), d.text), (what, t)
        assert int(gix.export(t, 4, 0, 1)[0]) == T_, (what, t)
        tab = gix.export(t, 3, 0, 4 ** T_).astype(np.int64)
        k, l = d.kmer(T_)
        empty = k > l
        assert np.array_equal(tab[:, 0] > tab[:, 1], empty), (what, t)
        assert np.array_equal(tab[~empty, 0], k[~empty]) and np.array_equal(tab[~empty, 1], l[~empty]), (what, t)
    check_sa_lookup(gix, ix, what)


@pytest.mark.parametrize("name", list(TEXTS))
def test_loader_rank_sa_and_tables_on_every_row(monkeypatch, name):
    ix = ref_of(name)
    monkeypatch.delenv("NABWA_TEXT_MODE", raising=False)
    monkeypatch.delenv("NABWA_KMER_T", raising=False)
    gix = nabwa.Index.from_arrays(*ix.streams(32))
    try:
        check_loaded(gix, ix, name)
    finally:
        gix.close()
    monkeypatch.setenv("NABWA_TEXT_MODE", "0")                                             # the samples only: sa_lookup walks LF
    gix = nabwa.Index.from_arrays(*ix.streams(32))
    try:
        with pytest.raises(nabwa.NabwaError):
            gix.export(0, 0, 0, 1)
        check_sa_lookup(gix, ix, name + ", LF walk")
    finally:
        gix.close()


@pytest.mark.parametrize("name", ["random1", "random5", "random192", "random193", "random385", "random1000", "A385", "A191C", "tandem384", "primary%192=0"])
def test_loader_under_other_sampling_intervals(monkeypatch, name):
    ix = ref_of(name)
    for intv in (1, 33, ix.n + 1):
        for mode in (None, "0"):
            if mode is None:
                monkeypatch.delenv("NABWA_TEXT_MODE", raising=False)
            else:
                monkeypatch.setenv("NABWA_TEXT_MODE", mode)
            gix = nabwa.Index.from_arrays(*ix.streams(intv))
            try:
                if mode is None:
                    check_loaded(gix, ix, "%s, sa_intv %d" % (name, intv))
                else:
                    check_sa_lookup(gix, ix, "%s, sa_intv %d, LF walk" % (name, intv))
            finally:
                gix.close()


# ------------------------------------------------------------------ search at the text's edges

CONFIGS = [
    {},
    {"NABWA_TEXT_MODE": "0"},
    {"NABWA_KMER_T": "0"},
    {"NABWA_TEXT_MODE": "0", "NABWA_KMER_T": "0"},
    {"NABWA_TEXT_KERNELS": "1"},
    {"NABWA_TEXT_KERNELS": "2"},
    {"NABWA_CAP1": "48"},                                                                 # every search through kernel D
]
CONFIG_VARS = ("NABWA_TEXT_MODE", "NABWA_KMER_T", "NABWA_TEXT_KERNELS", "NABWA_CAP1")
_SEARCH = {}


def option_block(changes):
    o = T.default_opt()
    for k, v in changes.items():
        setattr(o, k, v)
    return o


def as_gap(opt):
    g = nabwa.GapOpt()
    C.memmove(C.byref(g), C.byref(opt), 64)
    return g


def search_case(olib, name):
    """the reads of a text and the oracle's answers under the three option sets, made once"""
    if name not in _SEARCH:
        text, short = SEARCH[name]
        ix = ref_of(name)
        reads = R.edge_reads(text, short=short)
        seq, rseq, off = R.encode(reads)
        w0, w1 = ix.d[0].bwt, ix.d[1].bwt
        ox = olib.orc_index_wrap(T.ptr(w0), len(w0), T.ptr(w1), len(w1))                   # (kept with the case: the oracle reads the arrays in place)
        want = {}
        for oname, _, changes in R.OPTION_SETS:
            opt = option_block(changes)
            want[oname] = (opt,) + T.oracle_cal_sa_reg_gap(olib, ox, opt, seq, rseq, off)
        _SEARCH[name] = (ix, reads, seq, rseq, off, ox, want)
    return _SEARCH[name]


def test_edge_reads_find_what_they_should(olib):
    """the reads are what they are meant to be: on every long text most are found and some are not (the default options allow no
    difference in a read hanging off the text by two bases plus a substitution); on the short ones some are longer than the text"""
    for name, (text, short) in SEARCH.items():
        ix, reads, seq, rseq, off, ox, want = search_case(olib, name)
        rows = want["default"][1]
        if name.startswith("random"):                                                      # (every read of a repeat's text is found somewhere)
            assert sum(len(r) == 0 for r in rows) > 0, name
        if short:
            assert any(len(r) > ix.n for r in reads), name
        else:
            assert sum(len(r) > 0 for r in rows) > len(reads) // 2, name


@pytest.mark.parametrize("env", CONFIGS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()) or "default")
@pytest.mark.parametrize("name", list(SEARCH))
def test_search_at_the_edges_of_the_text(monkeypatch, olib, name, env):
    ix, reads, seq, rseq, off, ox, want = search_case(olib, name)
    for v in CONFIG_VARS:
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("NABWA_DEEP_GB", "1")                # kernel D's page pool belongs to the index, and each case loads its own: 1 GiB, not the default 32
    gix = nabwa.Index.from_arrays(*ix.streams(32))
    try:
        for oname, (opt, rows, maxe) in want.items():
            b = nabwa.Batch(gix, as_gap(opt), seq, rseq, off, False)
            try:
                b.run()
                n_deep = b.sync()
                got, gmax = b.fetch()
            finally:
                b.close()
            bad = [i for i in range(len(reads)) if got[i].tobytes() != rows[i].tobytes()]
            assert not bad, "%s (%d bases), %s: %d of %d reads differ from the oracle, e.g. read %d %s: %s vs %s" % (
                name, ix.n, oname, len(bad), len(reads), bad[0], "".join("ACGT"[c] for c in reads[bad[0]]), got[bad[0]][:3], rows[bad[0]][:3])
            if not env or "NABWA_CAP1" in env:
                assert np.array_equal(gmax, maxe), (name, oname)
            if "NABWA_CAP1" in env and not SEARCH[name][1]:         # (on the short texts most searches end within 48 entries)
                assert n_deep > 0, "no search reached kernel D"
    finally:
        gix.close()


@pytest.mark.parametrize("name", list(SEARCH))
def test_width_records_at_the_edges_of_the_text(monkeypatch, olib, name):
    ix, reads, seq, rseq, off, ox, want = search_case(olib, name)
    for v in CONFIG_VARS:
        monkeypatch.delenv(v, raising=False)
    gix = nabwa.Index.from_arrays(*ix.streams(32))
    try:
        for oname, (opt, _, _) in want.items():
            T.check_width_records(nabwa, gix, as_gap(opt), opt, olib, lambda x: C.c_void_p(ox + x * T.OracleIndex.BWT_SIZE), seq, rseq, off)
    finally:
        gix.close()
