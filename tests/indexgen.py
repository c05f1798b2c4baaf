"""Seeded inputs for the `bwa index` tests (test_index_pac.py, test_gpu_index_build.py): FASTA / FASTQ files that carry every
quirk of the reference's packing (bntseq.c:166-256 over kseq.h), and genomes whose suffix sorting needs many doubling rounds."""
import gzip
import os
import random

import numpy as np

IUPAC = "RYSWKMBDHVNU"        # every code nst_nt4_table maps to 4; '-' maps to 5
QUIRK_CASES = ["mix_t0", "mix_t1", "mix_t2", "mix_t3", "crlf", "no_final_newline", "gzip", "fastq", "single"]


def _acgt(rng, n, lower=False):
    s = "".join(rng.choice("ACGT") for _ in range(n))
    return s.lower() if lower else s


def _write(path, records, width=60, crlf=False, final_newline=True, fastq=False, gz=False):
    """records: (header line without '>', sequence).  Lines of `width` characters (0: one line)."""
    eol = "\r\n" if crlf else "\n"
    out = []
    for head, seq in records:
        out.append(("@" if fastq else ">") + head + eol)
        if fastq:
            out.append(seq + eol + "+" + eol + "I" * len(seq) + eol)
        else:
            w = width or max(len(seq), 1)
            for i in range(0, len(seq), w):
                out.append(seq[i:i + w] + eol)
    txt = "".join(out)
    if not final_newline:
        txt = txt.rstrip("\r\n")
    data = txt.encode()
    if gz:
        data = gzip.compress(data, mtime=0)
    with open(path, "wb") as f:
        f.write(data)
    return path


def _quirk_records(seed, tail):
    """Several contigs with: N runs at contig starts and ends and on both sides of a contig border, NNnn and NR
    adjacency, lower case, every IUPAC code and '-', a zero-length record, comments with tabs, records without a
    comment before any comment and after one.  `tail` bases end the last contig (to set l_pac % 4)."""
    rng = random.Random(seed)
    return [
        ("chr1", "NNNN" + _acgt(rng, 257) + "NNN"),                                    # no comment yet: "(null)"
        ("chr2 first comment", "NN" + _acgt(rng, 130) + "NNnn" + _acgt(rng, 17) + "NR" + _acgt(rng, 40) + IUPAC + IUPAC.lower() + "-" + _acgt(rng, 9) + "nnn"),
        ("chr3", "NNN" + _acgt(rng, 211, lower=True) + "acgtNNNNNNNNNN"),           # stale comment; a hole on each side of the border
        ("chr3b\twith a tab after the name", "NNNNN" + _acgt(rng, 77) + "--" + _acgt(rng, 5)),
        ("empty zero\tlength\trecord", ""),                                          # a zero-length record (not the first)
        ("chr4", "YYYYRRRR" + _acgt(rng, 64) + "n" + "N" + "n"),                     # stale comment again
        ("chr5 \tleading space and tab", _acgt(rng, 333) + _acgt(rng, 7, lower=True) + _acgt(rng, tail)),
    ]


def quirk_cases(root):
    """name -> FASTA/FASTQ path, written under root."""
    os.makedirs(root, exist_ok=True)
    cases = {}
    for tail in range(4):           # l_pac % 4 = 0, 1, 2, 3 across these four
        cases["mix_t%d" % tail] = _write(os.path.join(root, "mix_t%d.fa" % tail), _quirk_records(100 + tail, tail))
    recs = _quirk_records(7, 2)
    cases["crlf"] = _write(os.path.join(root, "crlf.fa"), recs, width=50, crlf=True)
    cases["no_final_newline"] = _write(os.path.join(root, "nonl.fa"), recs, width=0, final_newline=False)
    cases["gzip"] = _write(os.path.join(root, "mix.fa.gz"), recs, width=70, gz=True)
    cases["fastq"] = _write(os.path.join(root, "mix.fq"), [(h, s) for h, s in recs if s], fastq=True)
    rng = random.Random(11)
    cases["single"] = _write(os.path.join(root, "single.fa"), [("only one contig with a comment", _acgt(rng, 1001))])
    return cases


def _fasta_np(path, contigs, width=60):
    """contigs: (name, uint8 codes 0..3 or ord('N')) -> plain FASTA"""
    lut = np.frombuffer(b"ACGT", np.uint8)
    with open(path, "wb") as f:
        for name, codes in contigs:
            f.write((">%s\n" % name).encode())
            txt = np.where(codes < 4, lut[np.minimum(codes, 3)], codes).astype(np.uint8)
            n = len(txt)
            full = n // width * width
            if full:
                f.write(np.concatenate([txt[:full].reshape(-1, width), np.full((full // width, 1), 10, np.uint8)], axis=1).tobytes())
            if n > full:
                f.write(txt[full:].tobytes() + b"\n")
    return path


def homopolymer(root, n=100_000):
    return _fasta_np(os.path.join(root, "homopolymer.fa"), [("polyA", np.zeros(n, np.uint8))])


def tandem(root, unit=171, copies=2000, seed=5):
    rng = np.random.default_rng(seed)
    u = rng.integers(0, 4, unit, dtype=np.uint8)
    flank = rng.integers(0, 4, 1000, dtype=np.uint8)
    return _fasta_np(os.path.join(root, "tandem.fa"), [("alpha_satellite", np.concatenate([flank, np.tile(u, copies), flank[::-1]]))])


def segdup(root, seg=50_000, seed=6):
    """exact 50 kb segmental duplicates: one segment four times, on two contigs, one copy reverse-complemented"""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 4, seg, dtype=np.uint8)
    r = lambda k: rng.integers(0, 4, k, dtype=np.uint8)
    c1 = np.concatenate([r(3000), s, r(20_000), s, r(777)])
    c2 = np.concatenate([r(5000), s, s, r(1234), (3 - s)[::-1], r(99)])
    return _fasta_np(os.path.join(root, "segdup.fa"), [("dupA", c1), ("dupB", c2)])


def repeat_genome(root, n=10_000_000, n_contigs=12, seed=9, name="repeats10m.fa"):
    """~n bases with repeat families (a 6 kb LINE-like element truncated and diverged, a 300 bp Alu-like element at 1-15 %
    divergence, short tandem repeats, exact recent duplicates), cut into contigs with N runs."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 4, n, dtype=np.uint8)

    def plant(cons, n_copies, div_lo, div_hi, trunc):
        for _ in range(n_copies):
            c = cons[rng.integers(0, len(cons) - 50):] if trunc else cons
            d = rng.uniform(div_lo, div_hi)
            c = c.copy()
            m = rng.random(len(c)) < d
            c[m] = (c[m] + rng.integers(1, 4, int(m.sum()), dtype=np.uint8)) & 3
            if rng.random() < 0.5:
                c = (3 - c)[::-1]
            at = int(rng.integers(0, n - len(c)))
            t[at:at + len(c)] = c

    plant(rng.integers(0, 4, 6000, dtype=np.uint8), max(1, n // 50_000), 0.0, 0.2, True)
    plant(rng.integers(0, 4, 300, dtype=np.uint8), max(1, n // 3_000), 0.0, 0.15, False)
    for _ in range(n // 15_000):        # short tandem repeats
        u = rng.integers(0, 4, int(rng.integers(1, 7)), dtype=np.uint8)
        k = int(rng.integers(30, 301))
        at = int(rng.integers(0, n - k))
        t[at:at + k] = np.resize(u, k)
    for _ in range(20):                  # exact recent duplicates, 1-20 kb
        k = int(rng.integers(1000, 20_000))
        a, b = (int(x) for x in rng.integers(0, n - k, 2))
        t[b:b + k] = t[a:a + k]
    cuts = np.sort(rng.choice(np.arange(1, n), n_contigs - 1, replace=False))
    contigs = []
    for i, piece in enumerate(np.split(t, cuts)):
        piece = piece.copy()
        if len(piece) > 500:             # N runs inside, and at the start of every other contig
            for _ in range(3):
                k = int(rng.integers(1, 200))
                at = int(rng.integers(0, len(piece) - k))
                piece[at:at + k] = ord("N")
            if i % 2:
                piece[:50] = ord("N")
        contigs.append(("chr%d repeat model" % (i + 1), piece))
    return _fasta_np(os.path.join(root, name), contigs)
