"""Colour space through `nabwa_samse` / `nabwa_sampe`: every stdout byte but the @PG line must be the reference's, and for sampe the
`[infer_isize]` lines of stderr too --
 * against the SAM goldens the reference wrote for the committed colour reads and .sai files (tests/golden/make_golden_cs.py): samse,
   samse -n 5, sampe -s;
 * against the compiled reference (oracle/_ref/bwa_ref, when it travelled) run on the spot on .sai files from `nabwa_aln -c`: more than
   one 0x40000 chunk, samse -n 0 / -n 10, sampe -s / -A / -s -a 250, reads over the ambiguity holes and across the contig borders, N
   colours, several lengths, `aln -c -q 20`, gzip input, a read at pos 0.
The colour index of the toy genome is built here with `nabwa_index -c`.  What keeps the comparisons from passing on nothing is asserted
on the reference's output."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import csgen
import nabwa_testlib as T
from test_gpu_sai2sam import ALN, CHUNK, INDEX, REFBIN, SAMPE, SAMSE, assert_same_sam, isize_lines, need_ref, run

pytestmark = pytest.mark.gpu
G = lambda x: os.path.join(T.GOLDEN, x)


@pytest.fixture(scope="module")
def cs_prefix(tmp_path_factory):
    d = tmp_path_factory.mktemp("csindex")
    prefix = str(d / "toycs")
    run([INDEX, "-c", "-p", prefix, T.TOY + ".fa"], timeout=600)
    for ext in (".nt.ann", ".nt.amb", ".nt.pac", ".bwt", ".sa"):
        assert os.path.exists(prefix + ext)
    return prefix


def aln(prefix, fq, sai, args=()):
    with open(sai, "wb") as f:
        r = subprocess.run([ALN, "-c"] + list(args) + [prefix, fq], stdout=f, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]


def records(sam):
    return [l.split("\t") for l in sam.decode(errors="replace").splitlines() if not l.startswith("@")]


def compare_se(prefix, sai, fq, args=()):
    got = run([SAMSE] + list(args) + [prefix, sai, fq])
    want = run([REFBIN, "samse"] + list(args) + [prefix, sai, fq], timeout=1800)
    assert_same_sam(got.stdout, want.stdout)
    return got, want


def compare_pe(prefix, sai, fq, args):
    got = run([SAMPE] + list(args) + [prefix, sai[0], sai[1], fq[0], fq[1]])
    want = run([REFBIN, "sampe"] + list(args) + [prefix, sai[0], sai[1], fq[0], fq[1]], timeout=1800)
    assert_same_sam(got.stdout, want.stdout)
    assert isize_lines(got.stderr) == isize_lines(want.stderr)
    return got, want


# ------------------------------------------------------------------------------------------------- committed goldens

@pytest.mark.parametrize("args,name", [([], "cs_se.sam"), (["-n", "5"], "cs_se_n5.sam")])
def test_samse_equals_the_reference_goldens(cs_prefix, args, name):
    r = run([SAMSE] + args + [cs_prefix, G("cs_se.sai"), G("reads_cs_se.fq.gz")], timeout=300)
    want = gzip.open(G(name + ".gz"), "rb").read()
    assert_same_sam(r.stdout, want)
    rec = records(want)
    assert rec[0][0] == "cs_pos0" and rec[0][3] == "1" and not int(rec[0][1]) & 4           # a read at pos 0: nt_ref[0] = 4
    assert any("I" in f[5] for f in rec) and any("D" in f[5] for f in rec) and any(t.startswith("XA:Z:") for f in rec for t in f[11:])
    end = [f for f in rec if f[0] == "cs_end"][0]                                          # a read that ends on the genome's last base
    assert not int(end[1]) & 4 and end[2] == "chr3" and end[5] == "49M"
    if args:                                                                                # reads with 5 or 6 hits are listed under -n 5 only
        n_xa = lambda sam: sum(1 for f in records(sam) for t in f[11:] if t.startswith("XA:Z:"))
        plain = gzip.open(G("cs_se.sam.gz"), "rb").read()
        assert want != plain and n_xa(want) >= n_xa(plain) + 20
    assert b"colour space: decoding" in r.stderr


def test_sampe_s_equals_the_reference_golden(cs_prefix):
    r = run([SAMPE, "-s", cs_prefix, G("cs_pe_1.sai"), G("cs_pe_2.sai"), G("reads_cs_pe_1.fq.gz"), G("reads_cs_pe_2.fq.gz")], timeout=300)
    want = gzip.open(G("cs_pe_s.sam.gz"), "rb").read()
    assert_same_sam(r.stdout, want)
    assert isize_lines(r.stderr) == open(G("cs_pe_s.err")).read().splitlines()
    rec = records(want)
    assert 2 * sum(1 for f in rec if int(f[1]) & 2) >= len(rec)


def test_refusals_with_a_colour_index(cs_prefix, tmp_path):
    """sampe without -s / -A, and reads without qualities (the reference reads p->qual[...] of a null pointer, cs2nt.c:129)"""
    r = run([SAMPE, "-f", tmp_path / "a.sam_", cs_prefix, G("cs_pe_1.sai"), G("cs_pe_2.sai"), G("reads_cs_pe_1.fq.gz"), G("reads_cs_pe_2.fq.gz")], ok=False)
    assert r.returncode == 1 and b"-s" in r.stderr and not (tmp_path / "a.sam").exists() and not (tmp_path / "a.sam_").exists()
    fa = tmp_path / "r.fa"
    with gzip.open(G("reads_cs_se.fq.gz"), "rt") as f, open(fa, "w") as o:
        lines = f.read().splitlines()
        for i in range(0, len(lines), 4):
            o.write(">%s\n%s\n" % (lines[i][1:], lines[i + 1]))
    r = run([SAMSE, "-f", tmp_path / "b.sam_", cs_prefix, G("cs_se.sai"), fa], ok=False)
    assert r.returncode == 1 and b"cs2nt.c:129" in r.stderr and not (tmp_path / "b.sam").exists()


# ------------------------------------------------------------------------------------------------- two chunks, on the spot

@pytest.fixture(scope="module")
def two_chunks(tmp_path_factory, cs_prefix):
    """0x40000 + 3000 pairs of 50 colours: 1 % SNPs, 1 % colour errors, 8 % of the reads with a 1-base indel, an N colour in 5 %"""
    d = tmp_path_factory.mktemp("cs2")
    rng = np.random.default_rng(17)
    g = csgen.genome()
    r1, r2 = [], []
    for i in range(CHUNK + 3000):
        if i % 80 == 40:                                              # short reads: some have the 5 to 11 hits that only -n 10 lists
            a, b = csgen.pair_from(rng, g, L=12)
        else:
            a, b = csgen.pair_from(rng, g, n_rate=0.05)
        r1.append(("p%06d/1" % i, a)); r2.append(("p%06d/2" % i, b))
    fq = [str(d / "r1.fq"), str(d / "r2.fq")]
    csgen.write_fq(fq[0], r1, rng)
    csgen.write_fq(fq[1], r2, rng)
    sai = [str(d / "r1.sai"), str(d / "r2.sai")]
    for e in range(2):
        aln(cs_prefix, fq[e], sai[e])
    return d, fq, sai, [s for _, s in r1]


@need_ref
def test_samse_two_chunks(two_chunks, cs_prefix):
    d, fq, sai, reads = two_chunks
    got, want = compare_se(cs_prefix, sai[0], fq[0])
    rec = records(want.stdout)
    assert len(rec) == CHUNK + 3000
    mapped = [not int(f[1]) & 4 for f in rec]
    assert sum(mapped) >= 0.8 * len(rec)
    n_i, n_d = sum(1 for f in rec if "I" in f[5]), sum(1 for f in rec if "D" in f[5])
    assert n_i >= 100 and n_d >= 100 and n_i + n_d >= 100
    assert any(t.startswith("XA:Z:") for f in rec for t in f[11:])
    assert any(t.startswith("CM:i:") and t != "CM:i:0" for f in rec for t in f[11:])
    assert any(m and "N" in s for m, s in zip(mapped, reads))                  # a mapped record whose read held an N colour
    assert all(len(f[9]) == len(f[10]) for f in rec)
    n_xa = lambda sam: sum(1 for f in records(sam) for t in f[11:] if t.startswith("XA:Z:"))
    for n in ("0", "10"):
        _, w = compare_se(cs_prefix, sai[0], fq[0], ["-n", n])
        assert w.stdout != want.stdout                                         # the switch shows in the reference's output
        assert n_xa(w.stdout) == 0 if n == "0" else n_xa(w.stdout) > n_xa(want.stdout)


@need_ref
def test_sampe_two_chunks(two_chunks, cs_prefix):
    d, fq, sai, _ = two_chunks
    got, want = compare_pe(cs_prefix, sai, fq, ["-s"])
    rec = records(want.stdout)
    assert len(rec) == 2 * (CHUNK + 3000)
    assert sum(1 for f in rec if not int(f[1]) & 4) >= 0.8 * len(rec)
    assert 2 * sum(1 for f in rec if int(f[1]) & 2) >= len(rec)
    assert sum(1 for f in rec if "I" in f[5]) >= 100 and sum(1 for f in rec if "D" in f[5]) >= 100
    assert len(isize_lines(want.stderr)) == 10


@need_ref
@pytest.mark.parametrize("args", [["-A"], ["-s", "-a", "250"]])
def test_sampe_switches(two_chunks, cs_prefix, args, tmp_path):
    d, fq, sai, _ = two_chunks                                        # the first 40000 pairs keep the runs short
    small = [str(tmp_path / "s1.fq"), str(tmp_path / "s2.fq")]
    for e in range(2):
        with open(fq[e]) as f, open(small[e], "w") as o:
            for k, line in enumerate(f):
                if k >= 4 * 40000:
                    break
                o.write(line)
    ssai = [str(tmp_path / "s1.sai"), str(tmp_path / "s2.sai")]
    for e in range(2):
        aln(cs_prefix, small[e], ssai[e])
    _, want = compare_pe(cs_prefix, ssai, small, args)
    rec = records(want.stdout)
    assert sum(1 for f in rec if not int(f[1]) & 4) >= 0.8 * len(rec)
    if args == ["-s", "-a", "250"]:
        assert 2 * sum(1 for f in rec if int(f[1]) & 2) >= len(rec)


# ------------------------------------------------------------------------------------------------- awkward reads

def awkward(rng, n=4000):
    """reads over the ambiguity holes of the toy genome (45000+200, 52000+3, 90000+1), across its contig borders (60000, 100000), with N
    colours, of several lengths, junk, and one at pos 0"""
    g = csgen.genome()
    out = [("w_pos0", csgen.read_at_pos0(g, 50))]
    spots = [(44900, 45300), (51900, 52100), (59900, 60100), (99900, 100100), (89900, 90100)]
    for i in range(n - 1):
        k = i % 8
        if k < 5:
            s = csgen.read_from(rng, g, 50, lo=spots[k][0], hi=spots[k][1])
        elif k == 5:
            s = csgen.read_from(rng, g, int(rng.integers(30, 100)), n_rate=0.5)
        elif k == 6:
            s = csgen.junk(rng, 50) if i % 16 == 6 else ("N" * 50 if i % 32 == 14 else csgen.read_from(rng, g, 50, n_rate=1.0))
        else:
            s = csgen.read_from(rng, g, 75)
        out.append(("w%05d" % i, s))
    return out


@need_ref
@pytest.mark.parametrize("case", ["plain", "q20", "gzip"])
def test_awkward_reads_equal_the_compiled_reference(cs_prefix, case, tmp_path):
    rng = np.random.default_rng(29)
    recs = awkward(rng)
    fq = str(tmp_path / ("a.fq.gz" if case == "gzip" else "a.fq"))
    csgen.write_fq(fq, recs, rng)
    sai = str(tmp_path / "a.sai")
    aln(cs_prefix, fq, sai, ["-q", "20"] if case == "q20" else [])
    _, want = compare_se(cs_prefix, sai, fq)
    rec = records(want.stdout)
    assert len(rec) == len(recs)
    assert rec[0][0] == "w_pos0" and rec[0][3] == "1" and not int(rec[0][1]) & 4
    assert any(t.startswith("XN:i:") for f in rec for t in f[11:])                          # holes
    assert any(int(f[1]) & 4 and f[2] != "*" for f in rec)                                  # across a contig border
    assert any(not int(f[1]) & 4 and "N" in s for f, (_, s) in zip(rec, recs))
    if case == "q20":
        # trimmed reads: XC on the unmapped ones only (a decoded read's full_len is its own length), and no soft clip for the trimmed tail
        assert any(t.startswith("XC:i:") for f in rec if int(f[1]) & 4 for t in f[11:])
        assert any(len(f[9]) < len(s) - 1 for f, (_, s) in zip(rec, recs) if not int(f[1]) & 4)
    if case == "plain":
        compare_se(cs_prefix, sai, fq, ["-n", "10"])
