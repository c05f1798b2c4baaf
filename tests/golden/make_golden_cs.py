#!/usr/bin/env python3
"""Colour-space goldens, written by the compiled reference (oracle/_ref/bwa_ref and libbwaref.so, `make -C oracle ref`):

  vectors_cs2nt.npz    cases for the decode kernel with cs2nt_DP + cs2nt_nt_qual's answers (reference cs2nt.c:36-109)
  vectors_pe_solid.npz pairing() with pe_opt_t.type = BWA_PET_SOLID (reference bwape.c:234-247), made as vectors_pe.npz's pairing cases are
  reads_cs_se.fq.gz, cs_se.sai, cs_se.sam.gz, cs_se_n5.sam.gz            colour reads, `aln -c`, `samse`, `samse -n 5`
  reads_cs_pe_[12].fq.gz, cs_pe_[12].sai, cs_pe_s.sam.gz, cs_pe_s.err    colour pairs (R3 first), `aln -c`, `sampe -s` and its [infer_isize] lines

The colour index of toy.fa is built in a scratch directory with the reference's `index -c` (nabwa_index -c writes the same bytes) and
is not committed.  Run from anywhere: python tests/golden/make_golden_cs.py"""
import ctypes as C
import gzip
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import csgen  # noqa: E402
import nabwa_testlib as T  # noqa: E402

REFBIN = os.path.join(ROOT, "oracle", "_ref", "bwa_ref")
REFLIB = os.path.join(ROOT, "oracle", "_ref", "libbwaref.so")


def gen_cs2nt(lib):
    rng = np.random.default_rng(20260116)
    items = []
    for q_o in (25, 26):                                               # the delicate example on both sides of NUCL_MM
        items.append(csgen.delicate(q_o))
    for q_b in (18, 19, 20):                                           # ... and with q(B) around COLOR_MM
        items.append(csgen.delicate(26, q_b=q_b))
    off, ref, cs = csgen.pack(items)
    o2, r2, c2 = csgen.cases(rng, 600)
    o3, r3, c3 = csgen.cases(rng, 20, sizes=[csgen.CS2NT_MAX, csgen.CS2NT_MAX - 1, 1, 2])
    off = np.concatenate([off, o2[1:] + off[-1]])
    off = np.concatenate([off, o3[1:] + off[-1]])
    ref = np.concatenate([ref, r2, r3]); cs = np.concatenate([cs, c2, c3])
    out = csgen.reference_decode(lib, off, ref, cs)
    np.savez_compressed(os.path.join(HERE, "vectors_cs2nt.npz"), off=off, nt_ref=ref, cs_read=cs, out=out)
    print("vectors_cs2nt.npz: %d cases, %d colours" % (len(off) - 1, int(off[-1])))


def gen_pairing(lib):
    """as make_golden.py's pairing cases, with pet_type = 2; both strands of both ends so that every branch of the sweep is met"""
    rng = np.random.default_rng(77)
    lib.ref_pairing.restype = C.c_int
    pin, pout, cnts, alns, aoff, hits, hoff, misc = [], [], [], [], [0], [], [0], []
    for t in range(400):
        na = [int(rng.integers(1, 5)), int(rng.integers(1, 5))]
        base = int(rng.integers(2000, 90000))
        rows = [[], []]
        hp, hr, he = [], [], []
        for e in range(2):
            for r in range(na[e]):
                a = int(rng.integers(0, 2)); nmm = int(rng.integers(0, 4)); go = int(rng.integers(0, 2)); ge = int(rng.integers(0, 3)) if go else 0
                score = 3 * nmm + 11 * go + 4 * ge
                k = int(rng.integers(1, 100000)); w = int(rng.choice([1, 1, 1, 2, 3]))
                rows[e].append([nmm | go << 8 | ge << 16 | a << 24, k, k + w - 1, score])
                for _ in range(w):
                    far = rng.random() < 0.3
                    pos = int(rng.integers(0, 100000)) if far else base + int(rng.integers(-700, 700))
                    hp.append(max(pos, 0)); hr.append(r); he.append(e)
        ii = np.array([0, 0, 1e-5, 0, 0, 0], np.float64)
        if t % 3:
            avg = float(rng.integers(200, 500)); sd = float(rng.integers(10, 60))
            ii = np.array([avg, sd, 1e-5, max(1, avg - 4 * sd), avg + 4 * sd, avg + float(rng.integers(3, 7)) * sd], np.float64)
        p_in = np.zeros(22, np.int64)
        for e in range(2):
            idx = [i for i, x in enumerate(he) if x == e]
            idx = idx[int(rng.integers(0, len(idx)))]
            r = rows[e][hr[idx]]
            ln = int(rng.choice([50, 50, 35, 75]))
            p_in[11 * e: 11 * e + 11] = [hp[idx] if rng.random() < 0.8 else hp[idx] + 3, r[0] >> 24 & 1, int(rng.choice([0, 0, 10, 23, 25, 37])),
                                          int(rng.choice([0, 23, 37])), ln, ln, r[0] & 0xff, r[0] >> 8 & 0xff, r[0] >> 16 & 0xff, r[3], 1 | (64 if e == 0 else 128)]
        a0 = np.array(rows[0], np.uint32).reshape(-1); a1 = np.array(rows[1], np.uint32).reshape(-1)
        hp_ = np.array(hp, np.uint32); hr_ = np.array(hr, np.int32); he_ = np.array(he, np.int32)
        p_out = np.zeros(22, np.int64)
        nn = np.array(na, np.int32)
        max_isize = int(rng.choice([500, 1000]))
        v = lambda x: x.ctypes.data_as(C.c_void_p)
        cnt = lib.ref_pairing(v(nn), v(a0), v(a1), len(hp), v(hp_), v(hr_), v(he_), v(p_in), max_isize, 2, 3, v(ii), v(p_out))
        pin.append(p_in); pout.append(p_out); cnts.append(cnt)
        alns.append(np.concatenate([a0, a1])); aoff.append(aoff[-1] + len(a0) + len(a1))
        hits.append(np.stack([hp_.astype(np.int64), hr_, he_], 1).reshape(-1)); hoff.append(hoff[-1] + 3 * len(hp))
        misc.append(np.concatenate([[na[0], na[1], max_isize], ii]))
    np.savez_compressed(os.path.join(HERE, "vectors_pe_solid.npz"), pr_in=np.array(pin), pr_out=np.array(pout), pr_cnt=np.array(cnts, np.int32),
                        pr_aln=np.concatenate(alns), pr_aln_off=np.array(aoff, np.int64), pr_hit=np.concatenate(hits),
                        pr_hit_off=np.array(hoff, np.int64), pr_misc=np.array(misc, np.float64))
    moved = sum(1 for a, b in zip(pin, pout) if (a != b).any())
    print("vectors_pe_solid.npz: 400 cases, %d change a record" % moved)


def ref(args, stdout=None):
    r = subprocess.run([REFBIN] + args, stdout=stdout if stdout else subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (args, r.returncode, r.stderr.decode()[-2000:])
    return r


def put_gz(name, data):
    """text goldens are kept gzipped (no timestamp inside, so a rerun writes the same bytes)"""
    with open(os.path.join(HERE, name + ".gz"), "wb") as f:
        with gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0) as z:
            z.write(data)


def multi_hit_reads(prefix, g, d, lo, hi, want):
    """short reads (12 and 13 colours) whose hits -- best and sub-optimal together -- number lo..hi: what `samse -n` lists or leaves out.
    The toy genome's 50-colour reads have 1, 2, 3 or 60 and more hits, so only short ones fall between the defaults and -n 5 / -n 10."""
    cand = [("m%05d_%d" % (p, L), csgen.colours(g[p:p + L + 1])) for L in (12, 13) for p in range(0, len(g) - L - 2, 7) if "N" not in g[p:p + L + 1]]
    fq, sai = os.path.join(d, "cand.fq"), os.path.join(d, "cand.sai")
    csgen.write_fq(fq, cand, np.random.default_rng(1))
    with open(sai, "wb") as f:
        ref(["aln", "-c", prefix, fq], stdout=f)
    _, hits = T.read_sai(sai)
    tot = [int(sum(int(x["l"]) - int(x["k"]) + 1 for x in h)) for h in hits]
    return [c for c, t in zip(cand, tot) if lo <= t <= hi][:want]


def gen_sam():
    rng = np.random.default_rng(4242)
    g = csgen.genome()
    with tempfile.TemporaryDirectory() as d:
        prefix = os.path.join(d, "toycs")
        ref(["index", "-c", "-p", prefix, os.path.join(HERE, "toy.fa")])
        out = lambda x: os.path.join(HERE, x)
        tmp = lambda x: os.path.join(d, x)
        # single-end: clean reads, reads over the holes and the contig borders, N colours, other lengths, junk, a read at pos 0
        recs = [("cs_pos0", csgen.read_at_pos0(g, 50))]
        for i in range(1199):
            k = i % 12
            if k == 0:
                s = csgen.read_from(rng, g, 50, lo=44900, hi=45300)
            elif k == 1:
                s = csgen.read_from(rng, g, 50, lo=59900, hi=60100)
            elif k == 2:
                s = csgen.read_from(rng, g, 50, n_rate=1.0)
            elif k == 3:
                s = csgen.read_from(rng, g, int(rng.integers(30, 76)))
            elif k == 4 and i % 24 == 4:
                s = csgen.junk(rng, 50)
            else:
                s = csgen.read_from(rng, g, 50)
            recs.append(("cs%04d" % i, s))
        recs.append(("cs_end", csgen.colours(g[-51:])))                  # ends on the last base of the genome
        recs += multi_hit_reads(prefix, g, d, 5, 6, 30) + multi_hit_reads(prefix, g, d, 7, 8, 8)
        csgen.write_fq(tmp("reads_cs_se.fq"), recs, rng)
        with open(out("cs_se.sai"), "wb") as f:
            ref(["aln", "-c", prefix, tmp("reads_cs_se.fq")], stdout=f)
        sams = {"cs_se.sam": ref(["samse", prefix, out("cs_se.sai"), tmp("reads_cs_se.fq")]).stdout,
                "cs_se_n5.sam": ref(["samse", "-n", "5", prefix, out("cs_se.sai"), tmp("reads_cs_se.fq")]).stdout}
        # pairs, R3 first
        r1, r2 = [], []
        for i in range(800):
            if i % 20 == 7:
                a, b = csgen.pair_from(rng, g)
                b = csgen.junk(rng, 50)
            elif i % 20 == 13:
                a, b = csgen.pair_from(rng, g, mu=2000, sd=300)
            else:
                a, b = csgen.pair_from(rng, g, n_rate=0.05)
            r1.append(("cp%04d/1" % i, a)); r2.append(("cp%04d/2" % i, b))
        csgen.write_fq(tmp("reads_cs_pe_1.fq"), r1, rng)
        csgen.write_fq(tmp("reads_cs_pe_2.fq"), r2, rng)
        for e in "12":
            with open(out("cs_pe_%s.sai" % e), "wb") as f:
                ref(["aln", "-c", prefix, tmp("reads_cs_pe_%s.fq" % e)], stdout=f)
        r = ref(["sampe", "-s", prefix, out("cs_pe_1.sai"), out("cs_pe_2.sai"), tmp("reads_cs_pe_1.fq"), tmp("reads_cs_pe_2.fq")])
        sams["cs_pe_s.sam"] = r.stdout
        with open(out("cs_pe_s.err"), "w") as f:
            f.write("".join(l + "\n" for l in r.stderr.decode().splitlines() if l.startswith("[infer_isize]")))
        for name in ("reads_cs_se.fq", "reads_cs_pe_1.fq", "reads_cs_pe_2.fq"):
            put_gz(name, open(tmp(name), "rb").read())
    for name, sam in sams.items():
        put_gz(name, sam)
        L = [l.split("\t") for l in sam.decode().splitlines() if not l.startswith("@")]
        print("%s: %d records, %d mapped, %d with I, %d with D, %d with XA, %d proper" % (
            name, len(L), sum(1 for f in L if not int(f[1]) & 4), sum(1 for f in L if "I" in f[5]), sum(1 for f in L if "D" in f[5]),
            sum(1 for f in L if any(t.startswith("XA:Z:") for t in f[11:])), sum(1 for f in L if int(f[1]) & 2)))


if __name__ == "__main__":
    if not (os.path.exists(REFBIN) and os.path.exists(REFLIB)):
        sys.exit("the compiled reference is missing: make -C oracle ref")
    lib = C.CDLL(REFLIB)
    gen_cs2nt(lib)
    gen_pairing(lib)
    gen_sam()
