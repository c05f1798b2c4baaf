"""What the tests of duplicate marking (nabwa_markdup_*, nabwa.MarkDup, `nabwa_bam2bam --sort --mark-duplicates`) share: aligned BAM
records made in Python, the Python oracle of the semantics in include/nabwa.h -- a dict of groups, no sorting -- the case lists, and the CPU
builds of csrc/markdup_body.hpp under tests/emu/, so that tests/test_markdup_emu.py runs the inputs of tests/test_gpu_markdup.py through the
bodies without a GPU."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

import bamlib as B
import nabwa_testlib as T
from damage_cases import Damaged, many_ops, parse_cigar, record, split_records       # noqa: F401  (the record builder and its kin)

EMU_DIR = os.path.join(T.ROOT, "tests", "emu")
CSRC = os.path.join(T.ROOT, "network-aware-bwa_amd", "csrc")
STAT_NAMES = ("seen", "skipped_flags", "already", "unmapped", "fragments", "pairs", "orphans", "dup_fragments", "dup_pairs", "dup_records")
N_STATS = len(STAT_NAMES)
SEEN, SK_FLAGS, ALREADY, UNMAPPED, FRAGMENTS, PAIRS, ORPHANS, DUP_FRAGMENTS, DUP_PAIRS, DUP_RECORDS = range(N_STATS)
ENDS_5P, ENDS_BOTH = 0, 1
DEFAULT_OPT = dict(min_qual=15, single_ends=ENDS_5P, exclude_flags=0xB00)
COORD_LO, COORD_HI = -(1 << 30), (1 << 31) + (1 << 30)
SCORE_CAP = 0xfffffffe


def opt_of(**kw):
    return dict(DEFAULT_OPT, **kw)


# ---------------------------------------------------------------------------------------------------------------- records
def rec(ref_id, pos, cigar, flag=0, qual=None, name=b"r", seq=None, **kw):
    """an aligned record whose sequence is as long as its CIGAR says (all A) unless seq is given; qual: a number for every base, or bytes"""
    ops = parse_cigar(cigar)
    L = sum(n for n, op in ops if op in "MIS=X")
    seq = "A" * L if seq is None else seq
    if qual is None:
        qual = 30
    if isinstance(qual, int):
        qual = bytes([qual] * len(seq))
    return record(ref_id, pos, 37, flag, ops, seq, qual, name=name, **kw)


def unmapped(flag=4, name=b"u", L=8, ref_id=-1, pos=-1):
    return record(ref_id, pos, 0, flag, "*", "C" * L, bytes([30] * L), name=name)


def pair(name, a, b, flag_a=0, flag_b=0):
    """two mates next to each other: a and b are (ref_id, pos, cigar, reverse, qual), or None for an unmapped mate"""
    out = []
    for k, (x, extra) in enumerate(((a, flag_a), (b, flag_b))):
        flag = 0x1 | (0x40 if k == 0 else 0x80) | extra
        if x is None:
            out.append(unmapped(flag | 4, name))
        else:
            ref_id, pos, cigar, rev, qual = x
            out.append(rec(ref_id, pos, cigar, flag | (0x10 if rev else 0), qual, name))
    return out


# ---------------------------------------------------------------------------------------------------------------- the oracle
def parse(r, opt):
    """a record's bytes -> what the semantics look at, or None for a damaged one"""
    size = len(r)
    bs, ref_id, pos, l_name, _mapq, _bin, n_cig, flag, L = struct.unpack_from("<IiiBBHHHI", r, 0)
    if bs + 4 != size or 36 + l_name + 4 * n_cig + (L + 1) // 2 + L > size:
        return None
    x = dict(flag=flag, name=bytes(r[36:36 + l_name]), cls="mapped")
    if flag & opt["exclude_flags"]:
        x["cls"] = "skipped"
    elif flag & 0x400:
        x["cls"] = "already"
    elif (flag & 4) or ref_id < 0 or pos < 0 or n_cig == 0:
        x["cls"] = "unmapped"
    if x["cls"] != "mapped":
        return x
    cig = [(w >> 4, w & 15) for w in struct.unpack_from("<%dI" % n_cig, r, 36 + l_name)]
    if L > 0 and sum(n for n, op in cig if op in (0, 1, 4, 7, 8)) != L:
        return None
    is_ref = [op in (0, 2, 3, 7, 8) for _, op in cig]
    first = is_ref.index(True) if any(is_ref) else len(cig)
    last = len(cig) - 1 - is_ref[::-1].index(True) if any(is_ref) else len(cig)
    lead = sum(n for n, op in cig[:first] if op in (4, 5))
    trail = sum(n for n, op in cig[last + 1:] if op in (4, 5))
    left, right = pos - lead, pos + sum(n for (n, _), f in zip(cig, is_ref) if f) - 1 + trail
    if left < COORD_LO or right >= COORD_HI:
        return None
    rev = bool(flag & 0x10)
    q = r[36 + l_name + 4 * n_cig + (L + 1) // 2:][:L]
    x.update(end=(ref_id, rev, right if rev else left), c3=left if rev else right, score=min(sum(v for v in q if v != 0xff and v >= opt["min_qual"]), SCORE_CAP))
    return x


def oracle(calls, opt):
    """calls: lists of records (bytes), added in turn -> (dup, stats).  Raises Damaged(lowest index) for the first call that holds a damaged
    record; leave such a call out to see what the handle holds after it"""
    stats = np.zeros(N_STATS, np.uint64)
    groups, follow, n = {}, {}, 0       # key -> [(score, ordinal, the ordinals it marks or None for a shadow)]; unmapped mate -> its mate
    for recs in calls:
        xs = []
        for i, r in enumerate(recs):
            x = parse(bytes(r), opt)
            if x is None:
                raise Damaged(i)
            xs.append(x)
        mate = {}
        for i in range(len(xs) - 1):
            a, b = xs[i], xs[i + 1]
            if (a["flag"] & 0xC1) == 0x41 and (b["flag"] & 0xC1) == 0x81 and a["name"] == b["name"] and a["cls"] in ("mapped", "unmapped") and b["cls"] in ("mapped", "unmapped"):
                mate[i], mate[i + 1] = i + 1, i
        for i, x in enumerate(xs):
            o = n + i
            stats[SEEN] += 1
            j = mate.get(i)
            if x["cls"] == "skipped":
                stats[SK_FLAGS] += 1
            elif x["cls"] == "already":
                stats[ALREADY] += 1
            elif x["cls"] == "unmapped":
                stats[UNMAPPED] += 1
                if j is not None and xs[j]["cls"] == "mapped":
                    follow[o] = n + j
            elif j is not None and xs[j]["cls"] == "mapped":
                if j > i:
                    stats[PAIRS] += 1
                    ends = tuple(sorted((x["end"], xs[j]["end"])))
                    groups.setdefault(("pair", ends), []).append((min(x["score"] + xs[j]["score"], SCORE_CAP), o, (o, o + 1)))
                if opt["single_ends"] == ENDS_5P:
                    groups.setdefault(("fragment", x["end"]), []).append((None, o, None))
            else:
                stats[FRAGMENTS] += 1
                if (x["flag"] & 1) and j is None:
                    stats[ORPHANS] += 1
                key = ("fragment", x["end"]) if opt["single_ends"] == ENDS_5P else ("fragment", x["end"], x["c3"])
                groups.setdefault(key, []).append((x["score"], o, (o,)))
        n += len(xs)
    dup = np.zeros(n, np.uint8)
    for key, members in groups.items():
        real = [m for m in members if m[2] is not None]
        if not real:
            continue
        winner = None
        if len(real) == len(members):                      # no shadow outranks them: the highest score, then the lowest ordinal
            best = max(m[0] for m in real)
            winner = min(m[1] for m in real if m[0] == best)
        for score, o, marks in real:
            if o != winner:
                dup[list(marks)] = 1
                stats[DUP_PAIRS if key[0] == "pair" else DUP_FRAGMENTS] += 1
    for o, m in follow.items():
        dup[o] = dup[m]
    stats[DUP_RECORDS] = int(dup.sum())
    return dup, stats


# ---------------------------------------------------------------------------------------------------------------- the case lists
def name_of(k, n=6):
    return b"q%0*d" % (n - 1, k)


def shape_cases():
    """(name, options, calls): the shapes of a record at which the bodies can go wrong.  Every read has a twin that starts or ends where it
    does, so a wrong end shows as a wrong mark"""
    out = []
    # every byte alignment: records 2 a + 1 start at residue a mod 16 once the name of the one in front has been made as long as that takes
    recs = []
    for a in range(16):
        cur = sum(len(r) for r in recs)
        probe = rec(0, 100 + a // 2, "20M", name=b"n")
        recs.append(rec(0, 100 + a // 2, "20M", qual=20 + a, name=b"n" * (1 + (a - cur - len(probe)) % 16)))
        recs.append(rec(1, 700 + a // 3, "5S17M", flag=16 * (a & 1), qual=40 - a, name=b"m" * (1 + a % 5)))
    out.append(("alignments", opt_of(), [recs]))
    # l_seq around the lanes' pieces of 8 quality bytes; l_seq 0 (no bases stored: score 0, the CIGAR is not held to it)
    recs = []
    for L in (1, 2, 15, 16, 17, 33, 129, 300):
        for k in range(3):
            recs.append(rec(0, 50, "%dM" % L, qual=bytes([(10 + 7 * i + k) % 60 for i in range(L)]), name=name_of(L)))
    recs += [record(0, 50, 37, 0, "10M", "", b"", name=b"empty"), record(0, 50, 37, 0, "33M", "", b"", name=b"empty2")]
    out.append(("read lengths", opt_of(), [recs]))
    out.append(("read lengths, both ends", opt_of(single_ends=ENDS_BOTH), [recs]))
    # CIGARs of 1, 15, 16, 17 and 40 operations, the same two ends reached by another CIGAR
    recs = []
    for n_ops in (1, 15, 16, 17, 40):
        ops = many_ops(n_ops)
        if ops[-1][1] == "S":
            ops[-1] = (1, "M")
        span = sum(n for n, op in ops if op in "MDN=X")
        for f in (0, 16):
            recs += [rec(2, 1000, ops, f, 25, name_of(n_ops)), rec(2, 1000, "%dM" % span, f, 20, b"plain"), rec(2, 1001, [(1, "S"), (span - 1, "M")], f, 21, b"lead"),
                     rec(2, 1000, [(span - 1, "M"), (1, "S")], f, 22, b"trail")]
    out.append(("CIGAR lengths", opt_of(), [recs]))
    out.append(("CIGAR lengths, both ends", opt_of(single_ends=ENDS_BOTH), [recs]))
    # clips on either side and both strands; I, D, N, =, X, P inside
    recs = []
    for f in (0, 16):
        for c in ("30M", "4S26M", "4H26M", "2H2S26M", "26M4S", "26M4H", "26M2S2H", "3S24M3S", "1H2S24M2S1H", "10M2I18M", "10M3D17M", "10M50N20M", "10=1X19=", "12M2P18M",
                  "3S5M1I4=2D3X50N10M2P4M3S"):
            ops = parse_cigar(c)
            lead = 0
            for n, op in ops:
                if op not in "SH":
                    break
                lead += n
            recs.append(rec(1, 500 + lead, ops, f, 30 - len(c), c.encode()))
    recs.append(record(1, 500, 37, 0, "4M", "ACGT", raw_ops=[5 << 4 | 9, 7 << 4 | 15], name=b"raw"))      # unassigned operation codes consume nothing, clip nothing
    recs += [rec(1, 500, "5H", 0, name=b"only_h"), rec(1, 500, "6S", 16, name=b"only_s"), rec(1, 495, "5S6I", 0, name=b"no_ref")]
    out.append(("clips and operations", opt_of(), [recs]))
    out.append(("clips and operations, both ends", opt_of(single_ends=ENDS_BOTH), [recs]))
    # pos 0 with a leading clip: a negative coordinate; the largest refID; coordinates just inside the range
    big = 2 ** 31 - 1
    recs = [rec(0, 0, "5S20M", 0, 20, b"neg"), rec(0, 2, "7S20M", 0, 30, b"neg2"), rec(0, 0, "20M", 0, 40, b"zero"), rec(big, 7, "9M", 0, 20, b"big"), rec(big, 7, "9M", 16, 20, b"bigr"),
            rec(big, 9, "2S7M", 0, 25, b"big2"), rec(big - 1, 7, "9M", 0, 20, b"big3"),
            edge_coordinate_records()[0][0], edge_coordinate_records()[1][0]]
    out.append(("coordinates", opt_of(), [recs]))
    out.append(("coordinates, both ends", opt_of(single_ends=ENDS_BOTH), [recs]))
    # qualities on either side of min_qual, and 0xff
    recs = [rec(0, 10, "8M", 0, bytes([14] * 8), b"q14"), rec(0, 10, "8M", 0, bytes([14] * 7 + [15]), b"q15"), rec(0, 10, "8M", 0, bytes([0xff] * 8), b"qff"),
            rec(0, 10, "8M", 0, bytes([0xff] * 7 + [16]), b"qff16"), rec(0, 10, "8M", 0, bytes([16] + [14] * 7), b"q16")]
    out.append(("qualities", opt_of(), [recs]))
    out.append(("qualities, min_qual 0", opt_of(min_qual=0), [recs]))
    out.append(("qualities, min_qual 17", opt_of(min_qual=17), [recs]))
    # names: equal, of equal length with another last byte, another first byte, of unequal length, 1 and 254 bytes long
    recs = []
    long_a, long_b = b"x" * 254, b"x" * 253 + b"y"
    for k, (na, nb) in enumerate(((b"same", b"same"), (b"lasta", b"lastb"), (b"afirst", b"bfirst"), (b"short", b"shorter"), (b"longer", b"long"), (b"a", b"a"), (long_a, long_a),
                                  (long_a, long_b), (b"12345678", b"12345678"), (b"12345678", b"12345679"), (b"123456789", b"123456780"), (b"1234567", b"1234567"))):
        for copy in range(2):
            recs += [rec(0, 2000 + 10 * k, "12M", 0x41, 20 + copy, na), rec(0, 2100 + 10 * k, "12M", 0x91, 20, nb)]
    out.append(("read names", opt_of(), [recs]))
    return out


def edge_coordinate_records():
    """(just inside, just outside) at either end of the legal range of a coordinate"""
    big = 2 ** 31 - 1
    h = (1 << 28) - 1
    low_in = rec(0, 0, [(h, "H")] * 4 + [(4, "H"), (10, "M")], 0, 20, b"lowest")                    # left = -(2^30)
    low_out = rec(0, 0, [(h, "H")] * 4 + [(5, "H"), (10, "M")], 0, 20, b"too_low")                  # left = -(2^30) - 1
    high_in = rec(0, big, [(1, "M")] + [(h, "N")] * 4 + [(4, "D")], 16, 20, b"highest")    # right = 2^31 + 2^30 - 1
    high_out = rec(0, big, [(1, "M")] + [(h, "N")] * 4 + [(5, "D")], 16, 20, b"too_high")  # right = 2^31 + 2^30
    return (low_in, low_out), (high_in, high_out)


def damaged_cases():
    """(name, a damaged record): each kind of damage of include/nabwa.h, the shapes nabwa_damage_add refuses and the coordinates"""
    good = rec(0, 900, "25M")
    (_, low_out), (_, high_out) = edge_coordinate_records()
    return [("block_size one too large", struct.pack("<I", len(good) - 4 + 1) + good[4:]), ("block_size one too small", struct.pack("<I", len(good) - 4 - 1) + good[4:]),
            ("l_seq beyond the record", record(0, 900, 37, 0, "25M", "A" * 25, l_seq=26)), ("n_cigar_op beyond the record", record(0, 900, 37, 0, "25M", "A" * 25, n_cigar=15)),
            ("fields beyond a skipped record", record(-1, -1, 0, 0x104, "*", "ACGT", l_seq=4000)), ("fields beyond an unmapped record", record(-1, -1, 0, 4, "*", "ACGT", l_seq=4000)),
            ("l_seq of 2^31 and more", record(0, 900, 37, 0, "25M", "A" * 25, l_seq=-5)),
            ("CIGAR consumes one base fewer", record(0, 900, 37, 0, "24M", "A" * 25)), ("CIGAR consumes one base more", record(0, 900, 37, 16, "20M6I", "A" * 25)),
            ("CIGAR of D and H only", record(0, 900, 37, 0, "25D3H", "A" * 25)), ("a coordinate below the range", low_out), ("a coordinate above the range", high_out)]


def group_cases():
    """(name, options, calls): groups, pairs, shadows, classes -- what tests/test_gpu_markdup.py runs on the device"""
    out = []
    for n in (1, 2, 3, 65, 257):
        for what, scores in (("distinct scores", [(7 * i + 3) % n for i in range(n)]), ("equal scores", [30] * n), ("the best one last", [20] * (n - 1) + [41])):
            # a score of 400 + s from twenty bases: all of quality 20 + s // 20, the first s % 20 of them one more
            recs = [rec(0, 300, "20M", 0, bytes([20 + s // 20 + (j < s % 20) for j in range(20)]), name_of(i)) for i, s in enumerate(scores)]
            out.append(("%d equal fragments, %s" % (n, what), opt_of(), [recs]))
            if n >= 3:
                out.append(("%d equal fragments, %s, two calls" % (n, what), opt_of(), [recs[:n // 2], recs[n // 2:]]))
                out.append(("%d equal fragments, %s, three calls" % (n, what), opt_of(), [recs[:1], recs[1:n - 1], recs[n - 1:]]))
    strands = [rec(0, 500, "20M", 0, 20, b"fwd"), rec(0, 500, "20M", 16, 20, b"rev"), rec(0, 480, "40M", 16, 30, b"rev_same_end"), rec(0, 490, "30M", 16, 25, b"rev_same_end2"),
               rec(0, 500, "25M", 16, 30, b"rev_other_end"), rec(1, 500, "20M", 0, 20, b"other_contig")]
    out.append(("strands and unclipped ends", opt_of(), [strands]))
    clipped = [rec(0, 700, "30M", 0, 20, b"plain"), rec(0, 705, "5S25M", 0, 21, b"soft"), rec(0, 705, "5H25M", 0, 22, b"hard"), rec(0, 705, "2H3S25M", 0, 23, b"both"),
               rec(0, 700, "30M", 16, 20, b"rplain"), rec(0, 700, "25M5S", 16, 21, b"rsoft"), rec(0, 700, "22M8H", 16, 19, b"rhard")]
    out.append(("clipped and unclipped versions of one alignment", opt_of(), [clipped]))
    lengths = [rec(0, 900, "30M", 0, 20, b"l30"), rec(0, 900, "30M", 0, 21, b"l30b"), rec(0, 900, "25M", 0, 30, b"l25"), rec(0, 900, "20M5S", 0, 22, b"l25b"), rec(0, 900, "40M", 0, 10, b"l40")]
    mixed = lengths + pair(b"p1", (0, 900, "20M", False, 20), (0, 1000, "20M", True, 20)) + pair(b"p2", (0, 900, "20M", False, 25), (0, 1000, "20M", True, 20))
    out.append(("read lengths under ENDS_5P", opt_of(), [mixed]))
    out.append(("read lengths under ENDS_BOTH, and no shadows", opt_of(single_ends=ENDS_BOTH), [mixed]))
    pairs = (pair(b"a", (0, 100, "20M", False, 20), (0, 300, "20M", True, 20)) + pair(b"b", (0, 100, "20M", False, 22), (0, 300, "20M", True, 20))
             + pair(b"c", (0, 100, "20M", False, 30), (0, 305, "20M", True, 30)) + pair(b"d", (0, 101, "20M", False, 30), (0, 300, "20M", True, 30))
             + pair(b"e", (0, 300, "20M", True, 21), (0, 100, "20M", False, 20))                    # the mates in the other order of their ends: one group with a and b
             + pair(b"f", (0, 100, "20M", True, 30), (0, 300, "20M", True, 30))                     # another strand at one end
             + pair(b"g", (1, 100, "20M", False, 20), (0, 300, "20M", True, 20)) + pair(b"h", (0, 300, "20M", True, 20), (1, 100, "20M", False, 25))      # mates on different contigs
             + pair(b"i", (2, 100, "20M", False, 20), (2, 100, "20M", False, 20)) + pair(b"j", (2, 100, "20M", False, 20), (2, 100, "20M", False, 21)))    # both ends the same
    out.append(("pairs", opt_of(), [pairs]))
    out.append(("pairs, both ends", opt_of(single_ends=ENDS_BOTH), [pairs]))
    out.append(("pairs, two calls", opt_of(), [pairs[:6], pairs[6:]]))
    shadow = ([rec(0, 100, "20M", 0, 60, b"frag_at_first_end"), rec(0, 281, "39M", 16, 60, b"frag_at_second_end")] + pair(b"p", (0, 100, "20M", False, 16), (0, 300, "20M", True, 16))
              + [rec(0, 100, "20M", 16, 60, b"other_strand"), rec(0, 100, "22M", 0, 61, b"frag_again")])
    out.append(("a fragment at a pair's end", opt_of(), [shadow]))
    out.append(("a fragment at a pair's end, the pair in a later call", opt_of(), [shadow[:2], shadow[2:]]))
    half = (pair(b"h1", (0, 400, "20M", False, 20), None) + pair(b"h2", (0, 400, "20M", False, 25), None) + pair(b"h3", None, (0, 400, "20M", False, 22))
            + pair(b"h4", None, None) + [rec(0, 400, "20M", 0, 18, b"single")] + pair(b"h5", (0, 381, "20M", True, 20), None))
    out.append(("half pairs", opt_of(), [half]))
    out.append(("half pairs, both ends", opt_of(single_ends=ENDS_BOTH), [half]))
    first = pair(b"o1", (0, 600, "20M", False, 20), (0, 700, "20M", True, 20))
    orphans = ([first[1]] + pair(b"o2", (0, 600, "20M", False, 25), (0, 700, "20M", True, 20)) + [rec(0, 600, "20M", 0x41, 30, b"o3"), rec(0, 700, "20M", 0x91, 30, b"other_name")]
               + [rec(0, 600, "20M", 0xC1, 35, b"o4"), rec(0, 700, "20M", 0xD1, 35, b"o4")] + [rec(0, 600, "20M", 0x1, 36, b"o5"), rec(0, 700, "20M", 0x11, 36, b"o5")] + [first[0]])
    out.append(("orphans, one at either end of a call", opt_of(), [orphans]))
    out.append(("mates in two calls are orphans", opt_of(), [first[:1], first[1:]]))
    skipped_mate = (pair(b"s1", (0, 800, "20M", False, 20), (0, 900, "20M", True, 20), flag_b=0x100) + pair(b"s2", (0, 800, "20M", False, 20), (0, 900, "20M", True, 20), flag_a=0x800)
                    + pair(b"s3", (0, 800, "20M", False, 25), (0, 900, "20M", True, 20), flag_b=0x400) + pair(b"s4", (0, 800, "20M", False, 19), (0, 900, "20M", True, 20)))
    out.append(("a pair whose mate is skipped or already marked", opt_of(), [skipped_mate]))
    classes = [rec(0, 50, "20M", 0, 20, b"c0"), rec(0, 50, "20M", 0x400, 60, b"already"), rec(0, 50, "20M", 0x100, 60, b"secondary"), rec(0, 50, "20M", 0x200, 60, b"qcfail"),
               rec(0, 50, "20M", 0x800, 60, b"suppl"), rec(0, 50, "20M", 0xC00, 60, b"suppl_already"), unmapped(4, b"u1"), unmapped(0, b"u2", ref_id=0, pos=50), unmapped(0, b"u3", ref_id=-1, pos=50),
               unmapped(0, b"u4", ref_id=0, pos=-1), rec(0, 50, "20M", 4, 60, b"flag4"), rec(0, 50, "20M", 0, 21, b"c1"), rec(0, 50, "20M", 0, 19, b"c2")]
    out.append(("classes in the middle of a group", opt_of(), [classes]))
    out.append(("classes, nothing excluded", opt_of(exclude_flags=0), [classes]))
    out.append(("classes, duplicates excluded", opt_of(exclude_flags=0x400), [classes]))
    return out


def random_records(n, seed, sites=7):
    """a seeded mix drawn from a handful of sites, so that groups are large: single reads, pairs, half pairs, orphans, every class"""
    rng = np.random.default_rng(seed)
    out, k = [], 0
    while len(out) < n:
        k += 1
        nm = b"r%d" % k
        def place():
            ref_id, site, rev = int(rng.integers(0, 2)), int(rng.integers(0, sites)), bool(rng.integers(0, 2))
            L, clip = int(rng.integers(20, 40)), int(rng.integers(0, 3))
            cig = [(clip, "S")] * bool(clip) + [(L, "M")]
            pos = 1000 * site + clip if not rev else 1000 * site + 500 - L
            return ref_id, pos, cig, rev, bytes(int(q) for q in rng.integers(10, 42, L + clip))
        kind = int(rng.integers(0, 10))
        if kind < 5:
            p = place()
            flag = (0x400 if rng.random() < 0.05 else 0) | (0x100 if rng.random() < 0.05 else 0)
            out.append(rec(p[0], p[1], p[2], flag | (16 if p[3] else 0), p[4], nm))
        elif kind < 8:
            out += pair(nm, place(), place())
        elif kind == 8:
            out += pair(nm, place(), None) if rng.random() < 0.5 else pair(nm, None, place())
        else:
            out += [unmapped(4, nm)] if rng.random() < 0.5 else pair(nm, place(), place())[:1]
    return out


# ---------------------------------------------------------------------------------------------------------------- the CPU builds
def _build(out, srcs, deps, flags):
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(s) for s in srcs + deps):
        return out
    subprocess.run(["g++", "-std=c++17", "-I" + EMU_DIR, "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"] + flags + srcs + ["-o", out, "-lpthread"], check=True)
    return out


BODY = [os.path.join(CSRC, "markdup_body.hpp"), os.path.join(CSRC, "rec_body.hpp"), os.path.join(T.ROOT, "include", "nabwa.h")]


def load_emu():
    """the bodies as a library"""
    lib = C.CDLL(_build(os.path.join(EMU_DIR, "libmarkdup_emu.so"), [os.path.join(EMU_DIR, "markdup_emu.cpp")], BODY, ["-O2", "-fPIC", "-shared"]))
    P = C.c_void_p
    lib.emu_markdup_create.restype = P
    lib.emu_markdup_create.argtypes = [C.c_int, C.c_int, C.c_uint32]
    lib.emu_markdup_destroy.argtypes = [P]
    lib.emu_markdup_destroy.restype = None
    lib.emu_markdup_clear.argtypes = [P]
    lib.emu_markdup_clear.restype = None
    lib.emu_markdup_add.restype = C.c_int64
    lib.emu_markdup_add.argtypes = [P, C.c_int64, P, P, C.c_int, C.c_int]
    lib.emu_markdup_resolve.restype = C.c_int64
    lib.emu_markdup_resolve.argtypes = [P, P, P]
    return lib


def build_main():
    """the stand-alone program, under AddressSanitizer and UndefinedBehaviorSanitizer"""
    return _build(os.path.join(EMU_DIR, "markdup_main_asan"), [os.path.join(EMU_DIR, "markdup_main.cpp"), os.path.join(EMU_DIR, "markdup_emu.cpp")], BODY,
                  ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])


class Emu:
    """a handle of the emulation, used as nabwa.MarkDup is"""

    def __init__(self, lib, opt, n_blocks=3, reverse=False):
        self.lib, self.n_blocks, self.reverse = lib, n_blocks, reverse
        self.h = lib.emu_markdup_create(opt["min_qual"], opt["single_ends"], opt["exclude_flags"])
        self.n = 0

    def add(self, recs):
        """-> -1, or the lowest damaged record (and nothing added)"""
        data, off = B.pack(recs)
        data = data if len(data) else np.zeros(1, np.uint8)
        bad = int(self.lib.emu_markdup_add(self.h, len(recs), T.ptr(data), T.ptr(off), self.n_blocks, int(self.reverse)))
        assert bad >= -1, "the emulation's own check %d" % bad
        if bad < 0:
            self.n += len(recs)
        return bad

    def resolve(self):
        dup, stats = np.zeros(max(self.n, 1), np.uint8), np.zeros(N_STATS, np.uint64)
        assert self.lib.emu_markdup_resolve(self.h, T.ptr(dup), T.ptr(stats)) == self.n
        return dup[:self.n], stats

    def clear(self):
        self.lib.emu_markdup_clear(self.h)
        self.n = 0

    def close(self):
        self.lib.emu_markdup_destroy(self.h)


def assert_same(got, want, what=""):
    (dup, stats), (wdup, wstats) = got, want
    assert dup.shape == wdup.shape and dup.dtype == wdup.dtype == np.uint8, what
    if not np.array_equal(dup, wdup):
        at = int(np.argwhere(dup != wdup)[0][0])
        raise AssertionError("%s: dup[%d] is %d, not %d (%d of %d differ)" % (what, at, dup[at], wdup[at], int((dup != wdup).sum()), dup.size))
    for k, (a, b) in enumerate(zip(stats, wstats)):
        assert int(a) == int(b), "%s: stats[%s] is %d, not %d" % (what, STAT_NAMES[k], int(a), int(b))


def write_case_file(path, items):
    """the cases as data for tests/emu/markdup_main.cpp.  items: (options, [(records, expected damaged index or -1)], expected dup, expected stats)"""
    with open(path, "wb") as f:
        f.write(struct.pack("<qq", len(items), N_STATS))
        for opt, calls, dup, stats in items:
            f.write(struct.pack("<qqqqq", opt["min_qual"], opt["single_ends"], opt["exclude_flags"], len(calls), len(dup)))
            for recs, bad in calls:
                data, off = B.pack(recs)
                f.write(struct.pack("<qqq", len(recs), len(data), bad))
                f.write(off.astype("<i8").tobytes())
                f.write(data.tobytes())
            f.write(np.asarray(dup, np.uint8).tobytes())
            f.write(np.asarray(stats, "<u8").tobytes())


def set_flags(raw, dup):
    """the record stream `raw` with 0x400 set on the records dup names"""
    a = np.frombuffer(bytes(raw), np.uint8).copy()
    off, q = [], 0
    while q < a.size:
        off.append(q)
        q += 4 + struct.unpack_from("<I", raw, q)[0]
    a[np.array(off, np.int64)[np.asarray(dup) != 0] + 19] |= 0x04
    return a.tobytes()
