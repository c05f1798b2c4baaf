"""Colour-space (SOLiD) test inputs: colour reads from a genome, and cases for the decode kernel (cs2nt_DP + cs2nt_nt_qual,
reference cs2nt.c:36-109) with the compiled reference's answers (oracle/_ref/libbwaref.so).  Test infrastructure only.

A read of L colours comes from L + 1 bases of a fragment, colour = XOR of the adjacent 2-bit base codes (A0 C1 G2 T3), written
double-encoded as ACGT, N where a base is N.  A SNP is two adjacent colour changes, a colour error is one.  Of a pair, R3 is the upstream
read and goes first, F3 second, both on the fragment's strand (reference bwape.c:234-247)."""
import ctypes as C
import gzip
import os

import numpy as np

import nabwa_testlib as T

CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
COMP = str.maketrans("ACGTNacgtn", "TGCANtgcan")
CS2NT_MAX = 1024


def rc(s):
    return s.translate(COMP)[::-1]


def colours(bases):
    """L + 1 bases -> L colour letters"""
    out = []
    for a, b in zip(bases[:-1], bases[1:]):
        out.append("ACGT"[CODE[a] ^ CODE[b]] if a in CODE and b in CODE else "N")
    return "".join(out)


def damage(rng, bases, snp=0.01, indel=0.08):
    """SNPs, and a 1-base insertion or deletion in some reads, on the bases a read is made from; returns one base more or less then"""
    s = list(bases)
    for j in np.nonzero(rng.random(len(s)) < snp)[0]:
        s[j] = "ACGT"[(CODE.get(s[j], 0) + 1 + int(rng.integers(3))) & 3]
    if rng.random() < indel and len(s) > 30:
        j = int(rng.integers(12, len(s) - 12))
        if rng.random() < 0.5:
            del s[j]
        else:
            s.insert(j, "ACGT"[int(rng.integers(4))])
    return "".join(s)


def colour_errors(rng, cs, err=0.01, n_rate=0.0):
    s = list(cs)
    for j in np.nonzero(rng.random(len(s)) < err)[0]:
        if s[j] in CODE:
            s[j] = "ACGT"[(CODE[s[j]] + 1 + int(rng.integers(3))) & 3]
    if n_rate and rng.random() < n_rate:
        s[int(rng.integers(len(s)))] = "N"
    return "".join(s)


def read_from(rng, genome, L, lo=0, hi=None, n_rate=0.0, indel=0.08, pos=None):
    """one colour read of L colours from either strand of genome[lo:hi]"""
    hi = len(genome) if hi is None else hi
    p = int(rng.integers(lo, max(lo + 1, hi - L - 2))) if pos is None else pos
    b = genome[p:p + L + 2]                                            # one spare base for a deletion
    if pos is None and rng.random() < 0.5:
        b = rc(b)
    b = damage(rng, b, indel=indel)
    return colour_errors(rng, colours(b[:L + 1]), n_rate=n_rate)


def read_at_pos0(genome, L):
    """the read that maps at position 0 of the colour text, whose first colour is the first base against an A (reference
    bwtmisc.c:210-254): bwa_cs2nt_core then has no base before the hit, nt_ref[0] = 4 (cs2nt.c:137)"""
    return genome[0] + colours(genome[:L])


def pair_from(rng, genome, L=50, mu=300, sd=25, lo=0, hi=None, n_rate=0.0):
    """(R3, F3): both on the fragment's strand, R3 upstream"""
    hi = len(genome) if hi is None else hi
    isize = max(L + 3, int(rng.normal(mu, sd)))
    p = int(rng.integers(lo, max(lo + 1, hi - isize)))
    frag = genome[p:p + isize]
    if rng.random() < 0.5:
        frag = rc(frag)
    a = damage(rng, frag[:L + 2])
    b = damage(rng, frag[-(L + 2):])
    return (colour_errors(rng, colours(a[:L + 1]), n_rate=n_rate), colour_errors(rng, colours(b[-(L + 1):]), n_rate=n_rate))


def junk(rng, L):
    return "".join("ACGT"[int(x)] for x in rng.integers(0, 4, L))


def quals(rng, n, base=33):
    q = rng.integers(2, 41, n)
    k = int(rng.integers(0, n // 2 + 1))
    if k:
        q[n - k:] = rng.integers(2, 12, k)                             # a low-quality tail for -q
    return "".join(chr(base + int(x)) for x in q)


def write_fq(path, recs, rng):
    op = gzip.open if str(path).endswith(".gz") else open
    with op(path, "wt") as f:
        for n, s in recs:
            f.write("@%s\n%s\n+\n%s\n" % (n, s, quals(rng, len(s))))


def genome():
    return "".join(s for _, s in T.read_fasta(T.TOY + ".fa"))


# ------------------------------------------------------------------------------------------------- decode-kernel cases

def _case(rng, size, kind):
    """(nt_ref of size + 1 codes, cs_read of size bytes) of one family of cases"""
    truth = rng.integers(0, 4, size + 1)
    ref = truth.copy()
    col = truth[:-1] ^ truth[1:]
    q = rng.integers(0, 61, size)
    if kind == "clean":
        pass
    elif kind == "snp":                                                 # the read differs from the reference in single bases
        for j in np.nonzero(rng.random(size + 1) < 0.08)[0]:
            ref[j] = (ref[j] + 1 + rng.integers(3)) & 3
    elif kind == "colour_err":
        for j in np.nonzero(rng.random(size) < 0.1)[0]:
            col[j] = (col[j] + 1 + rng.integers(3)) & 3
    elif kind == "q_edges":                                             # qualities on both sides of COLOR_MM = 19 and NUCL_MM = 25
        q = rng.choice([17, 18, 19, 20, 24, 25, 26, 27], size)
        for j in np.nonzero(rng.random(size) < 0.2)[0]:
            col[j] = (col[j] + 1 + rng.integers(3)) & 3
        for j in np.nonzero(rng.random(size + 1) < 0.1)[0]:
            ref[j] = (ref[j] + 1 + rng.integers(3)) & 3
    elif kind == "n_colours":                                           # quality 63: an N colour
        q[rng.random(size) < 0.15] = 63
    elif kind == "ref4_start":
        ref[0] = 4
    elif kind == "ref4_inside":
        ref[rng.random(size + 1) < 0.2] = 4
    elif kind == "ref4_all":
        ref[:] = 4
    elif kind == "ties":                                                # every penalty alike, colours at random: many equal paths
        q[:] = 25
        col = rng.integers(0, 4, size)
    elif kind == "random":
        ref = rng.integers(0, 5, size + 1)
        col = rng.integers(0, 4, size)
        q = rng.choice(np.concatenate([np.arange(61), [63, 63, 63]]), size)
    else:
        raise ValueError(kind)
    return ref.astype(np.uint8), (col << 6 | q).astype(np.uint8)


KINDS = ("clean", "snp", "colour_err", "q_edges", "n_colours", "ref4_start", "ref4_inside", "ref4_all", "ties", "random")


def delicate(q_o, q_b=20, q_rest=30):
    """the "delicate example" of cs2nt.c:8-21: ref_nt = ATTAAC (colours R B R B G = 3 0 3 0 1 -- in code letters T A T A C), read colours
    R B B O G = 3 0 0 2 1 with quality q(O) = q_o: one colour change and one base change, or two colour changes"""
    ref = np.array([CODE[c] for c in "ATTAAC"], np.uint8)
    col = np.array([3, 0, 0, 2, 1])
    q = np.array([q_rest, q_rest, q_b, q_o, q_rest])
    return ref, (col << 6 | q).astype(np.uint8)


def cases(rng, n, sizes=None):
    """n cases over all kinds -> (off, nt_ref, cs_read) as nabwa_cs2nt takes them"""
    refs, css, off = [], [], [0]
    for i in range(n):
        if sizes is not None:
            size = int(sizes[i % len(sizes)])
        else:
            size = int(rng.choice([1, 2, 3, int(rng.integers(4, 36)), int(rng.integers(36, 76)), int(rng.integers(76, 300))]))
        r, c = _case(rng, size, KINDS[i % len(KINDS)])
        refs.append(r); css.append(c); off.append(off[-1] + size)
    return np.array(off, np.int64), np.concatenate(refs), np.concatenate(css)


def pack(items):
    """[(nt_ref, cs_read)] -> (off, nt_ref, cs_read)"""
    off = np.cumsum([0] + [len(c) for _, c in items]).astype(np.int64)
    return off, np.concatenate([r for r, _ in items]), np.concatenate([c for _, c in items])


def reference_decode(lib, off, nt_ref, cs_read):
    """cs2nt_DP + cs2nt_nt_qual of the compiled reference for every case -> the array nabwa_cs2nt returns"""
    lib.cs2nt_DP.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.cs2nt_DP.restype = None
    lib.cs2nt_nt_qual.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.cs2nt_nt_qual.restype = C.c_void_p
    n = len(off) - 1
    out = np.zeros(max(int(off[-1]) - n, 0), np.uint8)
    for i in range(n):
        size = int(off[i + 1] - off[i])
        ref = np.ascontiguousarray(nt_ref[off[i] + i:off[i + 1] + i + 1])
        cs = np.ascontiguousarray(cs_read[off[i]:off[i + 1]])
        nt_read = np.zeros(size + 8, np.uint8)
        bt = np.zeros(4 * size + 16, np.uint8)
        tarr = np.zeros(2 * size + 16, np.uint8)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        lib.cs2nt_DP(size, p(ref), p(cs), p(nt_read), p(bt))
        lib.cs2nt_nt_qual(size, p(nt_read), p(cs), p(tarr))
        out[off[i] - i:off[i + 1] - i - 1] = tarr[size + 1:2 * size]     # t2array + 1, size - 1 bytes
    return out


def load_ref_lib():
    return C.CDLL(T.REF_SO) if os.path.exists(T.REF_SO) else None
