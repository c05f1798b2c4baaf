"""Helpers of the kernel-W table tests (test_width_sum_identity.py, test_gpu_width_requests.py): the interval table of an
oracle index stepped with the oracle's own occ, bwt_cal_width with its intervals kept, and the reads of the toy genome that
put the primary row inside an interval.  Test infrastructure only."""
import ctypes as C

import numpy as np

import nabwa_testlib as T

COMP = str.maketrans("ACGTN", "TGCAN")


def bwt_header(bwt_ptr):
    """(primary, L2[0..4], seq_len) of an orc_bwt_t (oracle/nabwa_oracle.h: seven leading u32)"""
    w = (C.c_uint32 * 7).from_address(bwt_ptr.value)
    return int(w[0]), [int(w[1 + c]) for c in range(5)], int(w[6])


def step4(olib, bwt_ptr, L2, k, l):
    """the four children {k', l'} of the interval {k, l} by one backward step (bwt.c:237-252); an empty child is {1, 0}"""
    ck, cl = (C.c_uint32 * 4)(), (C.c_uint32 * 4)()
    olib.orc_2occ4(bwt_ptr, (k - 1) & 0xffffffff, l, ck, cl)
    out = []
    for c in range(4):
        nk, nl = L2[c] + ck[c] + 1, L2[c] + cl[c]
        out.append((nk, nl) if nk <= nl else (1, 0))
    return out


def oracle_levels(olib, bwt_ptr, depth):
    """levels 0..depth of the interval table: level t is an int64 array [4^t][2], key = the consumed symbols as base-4 digits,
    first consumed most significant (the child c of key K is 4 K + c); an empty entry is {1, 0} and so are its children"""
    _, L2, seq_len = bwt_header(bwt_ptr)
    lv = [np.array([[0, seq_len]], np.int64)]
    for t in range(1, depth + 1):
        par = lv[-1]
        cur = np.empty((4 * len(par), 2), np.int64)
        for key in range(len(par)):
            k, l = int(par[key, 0]), int(par[key, 1])
            cur[4 * key:4 * key + 4] = step4(olib, bwt_ptr, L2, k, l) if k <= l else [(1, 0)] * 4
        lv.append(cur)
    return lv


def widths(level):
    """interval widths of a level (an empty entry {1, 0}: 0)"""
    return level[:, 1] - level[:, 0] + 1


def primary_hits(olib, bwt_ptr, s, max_level=8):
    """bwt_cal_width (bwtaln.c:52-76) over the symbol codes s with the intervals kept: the (position, level) pairs -- level =
    symbols consumed since the last restart -- at which the interval holds the primary row; positions >= 1 that are not the
    last of the pass (the last one is never part of a table trip), levels 1..max_level"""
    primary, L2, seq_len = bwt_header(bwt_ptr)
    ck, cl = (C.c_uint32 * 4)(), (C.c_uint32 * 4)()
    k, l, level, out = 0, seq_len, 0, []
    for i, c in enumerate(s):
        c = int(c)
        if c < 4:
            olib.orc_2occ4(bwt_ptr, (k - 1) & 0xffffffff, l, ck, cl)
            k, l = L2[c] + ck[c] + 1, L2[c] + cl[c]
            level += 1
        if k > l or c > 3:
            k, l, level = 0, seq_len, 0
        elif 1 <= i < len(s) - 1 and level <= max_level and k <= primary <= l:
            out.append((i, level))
    return out


def toy_contigs():
    return [s.upper() for _, s in T.read_fasta(T.TOY + ".fa")]


def revcomp(s):
    return s.translate(COMP)[::-1]


def four_ways(s):
    """a read as it is, reversed, complemented and reverse-complemented"""
    return [s, s[::-1], s.translate(COMP), revcomp(s)]


def with_n(s, at):
    return s[:at] + "N" + s[at + 1:]


def as_batch(seqs):
    """(seq, rseq, off) of nabwa_testlib.encode_reads for plain base strings"""
    seq, rseq, off, _ = T.encode_reads([("r%d" % i, s, "I" * len(s)) for i, s in enumerate(seqs)])
    return seq, rseq, off


def primary_tail_reads(rng, text, max_level=9):
    """Reads in whose width passes an interval of level t = 1..max_level holds the primary row at an inner position, on either index.
    The pass of strand 0 consumes the read from its end against the index of the text, so after t symbols the pattern is the read's
    last t bases: a read that ends with the text's first t bases has the text's own prefix -- the primary key -- at level t.  Strand 1
    consumes the complement against the index of the reversed text: the read ends with the complement of the text's last t bases,
    last base first.  With 'N' + three more bases behind it the pass restarts first, so level 1 comes at a position >= 1; the bases
    in front of the tail come from the genome, so the walk goes on through the levels above t."""
    out = []
    tails = lambda t: (text[:t], text[::-1][:t].translate(COMP))
    for t in range(1, max_level + 1):
        for tail in tails(t):
            for L in (12, 33, 40, 100):
                p = int(rng.integers(0, len(text) - L))
                body = text[p:p + L - t] + tail
                out.append(body)
                out.append(body[4:] + "N" + text[p + 7:p + 10])
    return out
