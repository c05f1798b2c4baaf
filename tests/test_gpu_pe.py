"""Paired-end chain on the GPU box: nabwa_pe_posn + nabwa_pe_finish (posn_pair / finish_pair, reference
bam2bam.c:683-811) against
  * vectors_pe_chain.npz -- the state of every end after the REFERENCE's own functions ran the same chain
    (tests/golden/make_golden.py: make_pe_chain; three insert-size estimates), bit-exact, and
  * pe_default.sam       -- what the reference's `sampe` command printed for the same pairs (flags, mate
    fields, template length, tags)."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import nabwa_testlib as T

nabwa = importlib.import_module("network-aware-bwa_amd")
pytestmark = pytest.mark.gpu

F = {k: i for i, k in enumerate(("type", "strand", "n_mm", "n_gapo", "n_gape", "score", "sa", "c1", "c2", "pos", "mapQ", "seQ",
                                 "extra_flag", "n_cigar", "nm", "n_multi", "len"))}


# accepted rescues (BWA_TYPE_MATESW records) each set must at least hold under a usable estimate; the short set has 26, every one
# soft-clipped where it overlaps its anchor, 10 left of a reverse-strand anchor and 16 right of a forward-strand one (make_golden.py
# check_short_set prints and asserts this)
MIN_MATESW = {"": 10, "150": 10, "short": 26}


@pytest.fixture(scope="module", params=["", "150", "short"], ids=["100bp", "150bp_config3", "short_inserts"])
def pe(request):
    """three fixture sets: the 100 bp toy pairs; 2 x 150 bp pairs with BASELINE config 3's error load (inserts ~ N(400, 40),
    up to 5 substitutions per read, gapped reads, diverged / far / cross-contig / duplicated / rescue pairs; make_golden.py
    pe_chain150); and 666 pairs of 25 - 151 bp fragments read with 76 bases (make_golden.py pe_chainshort): 318 pairs with both
    ends at one position, mates of unequal length, rescued mates that overlap their anchor, fragments at the first and last
    bases of every contig, rescue windows cut by either end of the text; estimates with low = 76 (sampe) and low = 1 (histogram)"""
    tag = request.param
    ix = nabwa.Index.load(T.TOY)
    ix.attach_reference(T.TOY)
    fq = [T.read_fastq(os.path.join(T.GOLDEN, "reads_pe%s_%d.fq" % (tag, e))) for e in (1, 2)]
    sai = [T.read_sai(os.path.join(T.GOLDEN, "pe%s_%d.sai" % (tag, e))) for e in (1, 2)]
    n = len(fq[0])
    inter = [fq[e][i] for i in range(n) for e in range(2)]               # interleaved ends: 2*pair + end
    hits = [sai[e][1][i] for i in range(n) for e in range(2)]
    seq, rseq, off, full = T.encode_reads(inter)
    v = np.load(os.path.join(T.GOLDEN, "vectors_pe%s_chain.npz" % tag))
    yield dict(tag=tag, ix=ix, opt=sai[1][0], seq=seq, rseq=rseq, off=off, full=full, hits=hits, v=v, n=n, names=[r[0] for r in fq[0]])
    ix.close()


def rec_fields(r):
    s = r.se
    return [s.type, s.strand, s.n_mm, s.n_gapo, s.n_gape, s.score, s.sa, s.c1, s.c2, s.pos, s.mapQ, s.seQ]


def test_pe_search_matches_reference_sai(pe):
    """the FM search of both ends, interleaved in one batch, gives the rows `bwa aln` wrote"""
    got, _ = pe["ix"].cal_sa_reg_gap(pe["opt"], pe["seq"], pe["rseq"], pe["off"])
    for i, (g, w) in enumerate(zip(got, pe["hits"])):
        assert len(g) == len(w) and (np.asarray(g) == np.asarray(w, nabwa.ALN_DT)).all(), i


def test_pe_posn_matches_reference(pe):
    recs, st = pe["ix"].pe_posn(pe["opt"], pe["off"], pe["full"], pe["hits"], nabwa.srand48_state(11))
    want = pe["v"]["posn_f"]
    for r in range(2 * pe["n"]):
        w = want[r]
        if w[F["type"]] == 0:
            assert recs[r].se.type == 0
            continue
        assert rec_fields(recs[r]) == [int(x) for x in w[:12]], r
        assert recs[r].extra_flag == w[F["extra_flag"]]


def finish(pe, mode):
    ix = pe["ix"]
    recs, _ = ix.pe_posn(pe["opt"], pe["off"], pe["full"], pe["hits"], nabwa.srand48_state(11))
    iv = pe["v"]["ii_" + mode]
    ii = nabwa.IsizeInfo(iv[0], iv[1], iv[2], int(iv[3]), int(iv[4]), int(iv[5]))
    if mode == "hist":                       # bam2bam's own route: bin the positioned pairs, infer from the histogram
        h = np.zeros(100000, np.uint16)
        for i in range(pe["n"]):
            a, b = recs[2 * i].se, recs[2 * i + 1].se
            if a.type and b.type:
                d = nabwa.lib().nabwa_isize_bin(2, a.mapQ, b.mapQ, a.pos, a.len, b.pos, b.len)
                if d >= 0:
                    h[d] += 1
        rc, ii2 = nabwa.isize_infer(h, 1e-5, toy_ann()[0])
        assert rc == 0
        assert (ii2.avg, ii2.std, ii2.ap_prior, ii2.low, ii2.high, ii2.high_bayesian) == tuple(iv), "insert-size estimate"
        ii = ii2
    tot, mp = ix.pe_finish(pe["opt"], nabwa.pe_opt_default(), ii, pe["seq"], pe["rseq"], pe["off"], pe["hits"], recs)
    return recs, tot, mp


def toy_ann():
    """(l_pac, contig names, contig offsets) from the .ann file (format: reference bntseq.c:63-75)"""
    lines = open(T.TOY + ".ann").read().split("\n")
    names = [l.split()[1] for l in lines[1::2] if l]
    offs = [int(l.split()[0]) for l in lines[2::2] if l]
    return int(lines[0].split()[0]), names, offs


@pytest.mark.parametrize("mode", ["sampe", "hist", "null"])
def test_pe_finish_matches_reference_chain(pe, mode):
    recs, tot, mp = finish(pe, mode)
    v = pe["v"]
    f, cg, mu, md = v["f_" + mode], v["cig_" + mode], v["multi_" + mode], v["md_" + mode]
    n_sw = 0
    for r in range(2 * pe["n"]):
        w, g = f[r], recs[r]
        s = g.se
        assert s.type == w[F["type"]], r
        if s.type == 0:
            continue
        # after bwa_update_bam1 a bridging end has mapQ 0; the chain golden is taken before that step
        bridging = bool(s.flag & 4)
        got = rec_fields(g)
        want = [int(x) for x in w[:12]]
        if bridging:
            got[10] = want[10]
        assert got == want, (r, got, want)
        assert (g.extra_flag & 0xff) == (w[F["extra_flag"]] & 0xff), r
        assert s.n_cigar == w[F["n_cigar"]] and list(s.cigar[:s.n_cigar]) == list(cg[r][:s.n_cigar]), r
        assert s.nm == w[F["nm"]] and s.md.decode() == str(md[r]), r
        assert s.len == w[F["len"]]
        assert s.n_multi == w[F["n_multi"]], r
        for k in range(s.n_multi):
            m = mu[r][21 * k: 21 * k + 21]
            q = s.multi[k]
            assert [q.pos, q.gap, q.mm, q.strand, q.n_cigar] == [int(x) for x in m[:5]], (r, k)
            assert list(q.cigar[:q.n_cigar]) == [int(x) for x in m[5:5 + q.n_cigar]], (r, k)
        n_sw += s.type == 3
    assert n_sw == int((f[:, 0] == 3).sum())
    assert mp[0] == n_sw and mp[1] == 0                     # singletons are never rescued
    if mode != "null":
        assert n_sw >= MIN_MATESW[pe["tag"]]                # the fixture does exercise the accepted-rescue branch


def test_pe_records_match_reference_sampe_output(pe):
    """flags, mate fields, template length and tags against the SAM the reference's `sampe` printed"""
    recs, _, _ = finish(pe, "sampe")
    sam = T.parse_sam(os.path.join(T.GOLDEN, "pe%s_default.sam" % pe["tag"]))
    _, names, offs = toy_ann()
    assert len(sam) == 2 * pe["n"]
    for r, w in enumerate(sam):
        g = recs[r]
        s = g.se
        assert w["name"] == pe["names"][r // 2]
        assert s.flag == w["flag"], (r, s.flag, w["flag"])
        if s.type == 0 and recs[r ^ 1].se.type == 0:
            assert w["rname"] == "*" and w["pos"] == 0 and w["rnext"] == "*"
            continue
        assert names[s.seqid] == w["rname"] and s.rpos == w["pos"], r
        assert (w["rnext"] == "=" and g.m_seqid == s.seqid) or names[g.m_seqid] == w["rnext"], r
        assert g.m_rpos == w["pnext"] and g.isize == w["tlen"], (r, g.m_rpos, w["pnext"], g.isize, w["tlen"])
        if s.type == 0:
            assert w["cigar"] == "*"
            continue
        assert s.mapQ == w["mapq"], r
        cig = T.cigar16_str(s.cigar[:s.n_cigar]) if s.n_cigar else "%dM" % s.len
        assert cig == w["cigar"], r
        t = w["tags"]
        assert t["XT"] == s.xt.decode() and t["NM"] == s.nm and t["SM"] == s.seQ and t["AM"] == g.am, r
        assert t.get("XN", 0) == s.nn
        assert (t["XM"], t["XO"], t["XG"]) == (s.n_mm, s.n_gapo, s.n_gapo + s.n_gape), r
        assert t["MD"] == s.md.decode(), r
        if s.type != 3:
            assert t["X0"] == s.c1
            if s.c1 <= pe["opt"].max_top2:
                assert t["X1"] == s.c2
        else:
            assert "X0" not in t
        xa = ""
        for k in range(s.n_multi):
            q = s.multi[k]
            sid = max(i for i, o in enumerate(offs) if q.pos >= o)
            c = T.cigar16_str(q.cigar[:q.n_cigar]) if q.n_cigar else "%dM" % s.len
            xa += "%s,%s%d,%s,%d;" % (names[sid], "-" if q.strand else "+", q.pos - offs[sid] + 1, c, q.gap + q.mm)
        assert t.get("XA", "") == xa, r


def test_pe_finish_rejects_colour_space(pe):
    recs, _ = pe["ix"].pe_posn(pe["opt"], pe["off"], pe["full"], pe["hits"], nabwa.srand48_state(11))
    po = nabwa.pe_opt_default()
    po.type = 2
    with pytest.raises(nabwa.NabwaError):
        pe["ix"].pe_finish(pe["opt"], po, nabwa.IsizeInfo(), pe["seq"], pe["rseq"], pe["off"], pe["hits"], recs)
