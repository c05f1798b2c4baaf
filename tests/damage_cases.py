"""What the tests of the damage profile (nabwa_damage_*, nabwa.Damage, `nabwa_bam2bam --damage`) share: aligned BAM records made in Python, SAM
lines as records, the Python oracle of the semantics in include/nabwa.h, the case lists, and the CPU builds of csrc/damage_body.hpp under
tests/emu/, so that tests/test_damage_emu.py runs the inputs of tests/test_gpu_damage.py through the bodies without a GPU."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np

import nabwa_testlib as T

EMU_DIR = os.path.join(T.ROOT, "tests", "emu")
CSRC = os.path.join(T.ROOT, "network-aware-bwa_amd", "csrc")
LEN_BINS = 1024
STAT_NAMES = ("seen", "counted", "skipped_flags", "skipped_place", "skipped_mapq", "skipped_empty", "columns_counted", "columns_skipped_read",
              "columns_skipped_ref")
N_STATS = len(STAT_NAMES)
SEEN, COUNTED, SK_FLAGS, SK_PLACE, SK_MAPQ, SK_EMPTY, COLS, COLS_SK_READ, COLS_SK_REF = range(N_STATS)
OPS = "MIDNSHP=X"
NIBBLES = "=ACMGRSVTWYHKDBN"
DEFAULT_OPT = dict(n_pos=25, min_mapq=0, exclude_flags=0xF04, require_flags=0)
LENGTHS = (1, 2, 3, 15, 16, 17, 63, 64, 65, 300)
N_POSS = (1, 2, 25, 256)
GOLDEN_SAMS = ("se_default", "se_adna", "se_q20", "pe_default", "pe150_default", "peshort_default")


def opt_of(**kw):
    return dict(DEFAULT_OPT, **kw)


# ---------------------------------------------------------------------------------------------------------------- the reference
class Ref:
    """a 2-bit reference: pac bytes (l_pac / 4 + 1 of them are ever read), contigs (name, offset, length), holes (offset, length)"""

    def __init__(self, pac, l_pac, contigs, holes):
        self.l_pac, self.contigs, self.holes = int(l_pac), list(contigs), list(holes)
        self.pac = np.zeros(self.l_pac // 4 + 1, np.uint8)
        src = np.frombuffer(bytes(pac), np.uint8)[:self.pac.size]
        self.pac[:src.size] = src
        k = np.arange(self.l_pac)
        self.codes = (self.pac[k >> 2] >> ((~k & 3) << 1)) & 3            # fin_pac_at
        self.hole = np.zeros(self.l_pac, bool)
        for o, n in self.holes:
            self.hole[o:o + n] = True
        self.offsets = np.array([c[1] for c in self.contigs], np.int64)
        self.ids = {c[0]: i for i, c in enumerate(self.contigs)}


def toy_ref():
    ann = open(T.TOY + ".ann").read().split("\n")
    l_pac, n_seqs = int(ann[0].split()[0]), int(ann[0].split()[1])
    contigs = []
    for i in range(n_seqs):
        o, n = ann[2 + 2 * i].split()[:2]
        contigs.append((ann[1 + 2 * i].split()[1], int(o), int(n)))
    amb = open(T.TOY + ".amb").read().split("\n")
    holes = [(int(x.split()[0]), int(x.split()[1])) for x in amb[1:1 + int(amb[0].split()[2])]]
    return Ref(open(T.TOY + ".pac", "rb").read(), l_pac, contigs, holes)


# ---------------------------------------------------------------------------------------------------------------- records
def parse_cigar(c):
    if isinstance(c, str):
        return [] if c == "*" else [(int(n), op) for n, op in re.findall(r"(\d+)([MIDNSHP=X])", c)]
    return list(c)


def record(ref_id, pos, mapq, flag, cigar, seq, qual=None, name=b"r", block_size=None, l_seq=None, n_cigar=None, raw_ops=None):
    """an aligned BAM record: u32 block_size + block.  cigar: "10M2I5M" or [(len, op)]; seq: letters of NIBBLES; the name's length is free,
    so that every field behind it lands at any alignment.  block_size / l_seq / n_cigar: what the fields say where that is not the truth;
    raw_ops: extra CIGAR words as they stand (operation codes without a letter)"""
    ops = parse_cigar(cigar)
    words = [n << 4 | OPS.index(op) for n, op in ops] + list(raw_ops or [])
    L = len(seq)
    packed = bytearray((L + 1) // 2)
    for i, ch in enumerate(seq):
        packed[i >> 1] |= NIBBLES.index(ch) << (0 if i & 1 else 4)
    qual = bytes([30] * L) if qual is None else bytes(qual)
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(name) + 1, mapq, 4680, len(words) if n_cigar is None else n_cigar, flag, L if l_seq is None else l_seq, -1, -1, 0)
    body += bytes(name) + b"\0" + struct.pack("<%dI" % len(words), *words) + bytes(packed) + qual
    return struct.pack("<I", len(body) if block_size is None else block_size) + body


def join(recs):
    """records -> (bytes as a uint8 array, offsets)"""
    off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)
    return np.frombuffer(b"".join(recs), np.uint8), off


def sam_records(path, ref):
    """the alignment lines of a SAM file as BAM records (tags dropped) -> (records, the parsed lines)"""
    out, lines = [], T.parse_sam(path)
    for i, r in enumerate(lines):
        qual = b"\xff" * len(r["seq"]) if r["qual"] == "*" else bytes(ord(c) - 33 for c in r["qual"])
        out.append(record(ref.ids.get(r["rname"], -1), r["pos"] - 1, r["mapq"], r["flag"], r["cigar"], "" if r["seq"] == "*" else r["seq"], qual,
                          name=r["name"].encode()[:1 + i % 40]))
    return out, lines


# ---------------------------------------------------------------------------------------------------------------- the oracle
class Damaged(Exception):
    def __init__(self, index):
        super().__init__("record %d is damaged" % index)
        self.index = index


class Tables:
    def __init__(self, n_pos):
        self.n_pos = n_pos
        self.sub5 = np.zeros((n_pos + 1, 4, 4), np.uint64)
        self.sub3 = np.zeros((n_pos + 1, 4, 4), np.uint64)
        self.len_hist = np.zeros(LEN_BINS, np.uint64)
        self.stats = np.zeros(N_STATS, np.uint64)

    def parts(self):
        return self.sub5, self.sub3, self.len_hist, self.stats

    def __iadd__(self, o):
        for a, b in zip(self.parts(), o.parts()):
            a += b
        return self

    def words(self):
        """as the library lays a table out: sub5, sub3, the length bins, the stats"""
        return np.concatenate([x.reshape(-1) for x in self.parts()])

    @classmethod
    def from_words(cls, n_pos, w):
        t, n = cls(n_pos), (n_pos + 1) * 16
        t.sub5[:] = w[:n].reshape(-1, 4, 4)
        t.sub3[:] = w[n:2 * n].reshape(-1, 4, 4)
        t.len_hist[:] = w[2 * n:2 * n + LEN_BINS]
        t.stats[:] = w[2 * n + LEN_BINS:2 * n + LEN_BINS + N_STATS]
        return t


def assert_same(got, want, what=""):
    for name, a, b in zip(("sub5", "sub3", "len_hist", "stats"), got.parts(), want.parts()):
        assert a.shape == b.shape and a.dtype == b.dtype == np.uint64, (what, name)
        if not np.array_equal(a, b):
            at = np.argwhere(a != b)[0]
            raise AssertionError("%s: %s differs at %s: %d, not %d%s" % (what, name, tuple(at), a[tuple(at)], b[tuple(at)],
                                                                       " (%s)" % STAT_NAMES[at[0]] if name == "stats" else ""))


CODE_OF = {1: 0, 2: 1, 4: 2, 8: 3}


def oracle_record(ref, opt, rec, t):
    """one record (its bytes, block_size word included) into the tables t; False for a damaged one.  Plain Python, column by column."""
    size = len(rec)
    bs, ref_id, pos, l_name, mapq, _bin, n_cig, flag, L = struct.unpack_from("<IiiBBHHHI", rec, 0)
    if bs + 4 != size:
        return False
    if 36 + l_name + 4 * n_cig + (L + 1) // 2 + L > size:
        return False
    n_pos = opt["n_pos"]
    if (flag & opt["exclude_flags"]) or (flag & opt["require_flags"]) != opt["require_flags"]:
        cls = SK_FLAGS
    elif ref_id < 0 or ref_id >= len(ref.contigs) or pos < 0:
        cls = SK_PLACE
    elif mapq < opt["min_mapq"]:
        cls = SK_MAPQ
    elif L == 0 or n_cig == 0:
        cls = SK_EMPTY
    else:
        cls = COUNTED
    if cls != COUNTED:
        t.stats[SEEN] += 1
        t.stats[cls] += 1
        return True
    cig = struct.unpack_from("<%dI" % n_cig, rec, 36 + l_name)
    seq = rec[36 + l_name + 4 * n_cig:]
    if sum(w >> 4 for w in cig if (w & 15) in (0, 1, 4, 7, 8)) != L:
        return False
    qi, k, rev = 0, int(ref.offsets[ref_id]) + pos, bool(flag & 0x10)
    for w in cig:
        op, n = w & 15, w >> 4
        if op in (0, 7, 8):
            for j in range(n):
                q4 = (seq[(qi + j) >> 1] >> (0 if (qi + j) & 1 else 4)) & 15
                if q4 not in CODE_OF:
                    t.stats[COLS_SK_READ] += 1
                    continue
                if k + j >= ref.l_pac or ref.hole[k + j]:
                    t.stats[COLS_SK_REF] += 1
                    continue
                r, q, d5, d3 = int(ref.codes[k + j]), CODE_OF[q4], qi + j, L - 1 - (qi + j)
                if rev:
                    r, q, d5, d3 = 3 - r, 3 - q, d3, d5
                t.sub5[min(d5, n_pos), r, q] += 1
                t.sub3[min(d3, n_pos), r, q] += 1
                t.stats[COLS] += 1
        if op in (0, 1, 4, 7, 8):
            qi += n
        if op in (0, 2, 3, 7, 8):
            k += n
    t.stats[SEEN] += 1
    t.stats[COUNTED] += 1
    t.len_hist[min(L, LEN_BINS - 1)] += 1
    return True


def oracle(ref, opt, recs):
    """the tables of a call over `recs` (a list of records as bytes); raises Damaged(lowest index) and counts nothing"""
    t = Tables(opt["n_pos"])
    for i, r in enumerate(recs):
        if not oracle_record(ref, opt, bytes(r), t):
            raise Damaged(i)
    return t


# ---------------------------------------------------------------------------------------------------------------- the case lists
def aligned(ref, rng, ref_id, pos, cigar, flag=0, mapq=37, mut=0.15, name_len=1, letters=None):
    """a record whose M / = / X columns carry the reference's bases, each replaced by another base with probability `mut`; inserted and
    clipped bases, and columns without a reference base, are random.  letters: {read index: letter} afterwards"""
    ops = parse_cigar(cigar)
    seq, k = [], int(ref.offsets[ref_id]) + pos
    for n, op in ops:
        if op in "M=X":
            for j in range(n):
                c = int(ref.codes[k + j]) if 0 <= k + j < ref.l_pac else int(rng.integers(0, 4))
                if rng.random() < mut:
                    c = (c + 1 + int(rng.integers(0, 3))) & 3
                seq.append("ACGT"[c])
        elif op in "IS":
            seq += ["ACGT"[int(x)] for x in rng.integers(0, 4, n)]
        if op in "MDN=X":
            k += n
    for i, ch in (letters or {}).items():
        seq[i] = ch
    return record(ref_id, pos, mapq, flag, ops, "".join(seq), name=b"n" * name_len)


def many_ops(n_ops, L_hint=2):
    """a CIGAR of exactly n_ops operations: M runs with I and D in turn between them"""
    ops = []
    for i in range(n_ops):
        ops.append((L_hint + i % 3, "M") if i % 2 == 0 else (1, "ID"[(i // 2) % 2]))
    if ops[-1][1] != "M":
        ops[-1] = (1, "S")
    return ops


def cases(ref):
    """(name, options, records): the smallest shapes at which the kernel can go wrong, all on the toy reference"""
    rng = np.random.default_rng(14)
    out = []
    # lengths x n_pos: reads shorter than 2 n_pos land in both tables with the same column; both strands; the start walks through every pac phase
    for n_pos in N_POSS:
        recs = []
        for i, L in enumerate(LENGTHS):
            for flag in (0, 16):
                recs.append(aligned(ref, rng, i % 3, 1000 + 7 * i + (flag >> 4), "%dM" % L, flag, name_len=1 + (3 * i + (flag >> 4)) % 16))
        out.append(("lengths, n_pos %d" % n_pos, opt_of(n_pos=n_pos), recs))
    # every start alignment mod 16 (a lead record of each size class in front), and both nibble phases (an odd and an even soft clip)
    recs = []
    for a in range(16):                 # records 3 a + 1 and 3 a + 2 start at residues a and a + 10 mod 16: the name of the one in front is as long as that takes
        cur = sum(len(r) for r in recs)
        recs.append(aligned(ref, rng, 1, 500 + a, "37M", name_len=1 + (a - cur - len(aligned(ref, rng, 1, 500 + a, "37M"))) % 16))
        recs.append(aligned(ref, rng, 0, 300 + a, "21M", name_len=1))
        recs.append(aligned(ref, rng, 0, 400 + a, "%dS30M2S" % (1 + a % 4), 16 * (a & 1), name_len=3))
    out.append(("alignments and nibble phases", opt_of(), recs))
    # CIGAR shapes
    shapes = ["40M", "5S20M3S", "1S1M", "10M2I3D10M", "10M3D2I10M", "10M50N10M", "3H10M2P10M4H", "10=1X10=", "7S9=2X1I4=3D6X5S", "100M1D100M1I99M"]
    recs = [aligned(ref, rng, i % 3, 2000 + 13 * i, c, 16 * (i & 1), name_len=1 + i) for i, c in enumerate(shapes)]
    for i, n_ops in enumerate((1, 16, 17, 64, 65, 300)):
        recs.append(aligned(ref, rng, 0, 7000 + 100 * i, many_ops(n_ops), 16 * (i & 1), name_len=5 + i))
    recs.append(record(0, 100, 37, 0, "4M", "ACGT", raw_ops=[5 << 4 | 9, 7 << 4 | 15]))      # unassigned operation codes consume nothing
    out.append(("CIGAR shapes", opt_of(), recs))
    # reference windows: each phase of a .pac byte, base 0, ending on l_pac - 1, running past l_pac, across a contig boundary
    last = len(ref.contigs) - 1
    end = ref.contigs[last][2]
    recs = [aligned(ref, rng, 0, p, "%dM" % L, f, name_len=1 + p) for p in range(4) for L in (1, 5, 33) for f in (0, 16)]
    recs += [aligned(ref, rng, last, end - L, "%dM" % L, f) for L in (1, 2, 3, 4, 5, 9, 64) for f in (0, 16)]
    recs += [aligned(ref, rng, last, end - 10, "30M", f) for f in (0, 16)] + [aligned(ref, rng, last, end - 3, "2S10M1D5M", 0), aligned(ref, rng, last, end, "8M", 0),
                                                                               aligned(ref, rng, last, end + 50, "8M", 16)]
    recs += [aligned(ref, rng, 0, ref.contigs[0][2] - 10, "30M", f) for f in (0, 16)]
    out.append(("reference windows", opt_of(), recs))
    # holes of length 1 and longer at the first, a middle and the last column; a read inside a long hole; a read over two holes
    recs = []
    for o, n in ref.holes:
        cid = max(i for i, c in enumerate(ref.contigs) if c[1] <= o)
        at = o - ref.contigs[cid][1]
        for f in (0, 16):
            recs += [aligned(ref, rng, cid, at, "21M", f), aligned(ref, rng, cid, at - 10, "21M", f), aligned(ref, rng, cid, at + n - 21, "21M", f),
                     aligned(ref, rng, cid, at - 20, "21M", f), aligned(ref, rng, cid, at + n - 1, "1M", f), aligned(ref, rng, cid, at + n, "9M", f),
                     aligned(ref, rng, cid, at - 9, "9M", f), aligned(ref, rng, cid, at - 5, "5M3I4M2D6M", f)]
    recs.append(aligned(ref, rng, 0, 45050, "60M", 0))
    recs.append(aligned(ref, rng, 0, 45150, "50M6800N10M", 0))
    out.append(("holes", opt_of(), recs))
    # read codes other than A, C, G, T: first, middle, last column, a whole piece of eight, next to a hole
    recs = [aligned(ref, rng, 0, 3000, "30M", f, letters={0: "N", 13: "R", 29: "="}) for f in (0, 16)]
    recs.append(aligned(ref, rng, 1, 3100, "3S30M", 0, letters={i: "N" for i in range(3, 12)}))
    recs.append(aligned(ref, rng, 0, 51995, "12M", 16, letters={5: "N", 6: "M", 4: "B"}))
    recs.append(record(2, 5, 20, 0, "16M", NIBBLES))
    out.append(("read codes", opt_of(), recs))
    # one record of every skip class, the first class that fits
    good = aligned(ref, rng, 1, 100, "25M")
    skips = [record(-1, -1, 0, 4, "*", "ACGTACGT"), aligned(ref, rng, 0, 10, "25M", 0x100), aligned(ref, rng, 0, 10, "25M", 0x200), aligned(ref, rng, 0, 10, "25M", 0x400),
             aligned(ref, rng, 0, 10, "25M", 0x810), record(-1, 50, 37, 0, "8M", "ACGTACGT"), record(len(ref.contigs), 50, 37, 0, "8M", "ACGTACGT"),
             record(0, -1, 37, 0, "8M", "ACGTACGT"), record(2 ** 31 - 1, 0, 37, 16, "8M", "ACGTACGT"), aligned(ref, rng, 0, 10, "25M", 0, mapq=19), aligned(ref, rng, 0, 10, "25M", 0, mapq=20),
             record(0, 10, 37, 0, "*", "ACGTACGT"), record(0, 10, 37, 0, "5H", ""), record(-1, -1, 0, 0x904, "*", ""), good]
    out.append(("skip classes", opt_of(min_mapq=20), skips))
    out.append(("skip classes, required flags", opt_of(require_flags=0x11, exclude_flags=0x4), skips + [aligned(ref, rng, 0, 10, "25M", 0x11), aligned(ref, rng, 0, 10, "25M", 0x1),
                                                                                                       aligned(ref, rng, 0, 10, "25M", 0x51)]))
    return out


def damaged_cases(ref):
    """(name, a damaged record): each kind of damage of include/nabwa.h"""
    rng = np.random.default_rng(15)
    good = aligned(ref, rng, 0, 900, "25M")
    out = [("block_size one too large", struct.pack("<I", len(good) - 4 + 1) + good[4:]), ("block_size one too small", struct.pack("<I", len(good) - 4 - 1) + good[4:]),
           ("l_seq beyond the record", record(0, 900, 37, 0, "25M", "A" * 25, l_seq=26)), ("n_cigar_op beyond the record", record(0, 900, 37, 0, "25M", "A" * 25, n_cigar=15)),
           ("fields beyond a skipped record", record(-1, -1, 0, 4, "*", "ACGT", l_seq=4000)), ("l_seq of 2^31 and more", record(0, 900, 37, 0, "25M", "A" * 25, l_seq=-5)),
           ("CIGAR consumes one base fewer", record(0, 900, 37, 0, "24M", "A" * 25)), ("CIGAR consumes one base more", record(0, 900, 37, 16, "20M6I", "A" * 25)),
           ("CIGAR of D and H only", record(0, 900, 37, 0, "25D3H", "A" * 25))]
    return out


def good_records(ref, n=40, seed=16):
    rng = np.random.default_rng(seed)
    return [aligned(ref, rng, int(rng.integers(0, 2)), int(rng.integers(0, 30000)), "%dM" % int(rng.integers(1, 120)), 16 * int(rng.integers(0, 2)), name_len=1 + i % 16) for i in range(n)]


# ---------------------------------------------------------------------------------------------------------------- the CPU builds
def _build(out, srcs, deps, flags):
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(s) for s in srcs + deps):
        return out
    subprocess.run(["g++", "-std=c++17", "-I" + EMU_DIR, "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"] + flags + srcs + ["-o", out, "-lpthread"], check=True)
    return out


BODY = [os.path.join(CSRC, "damage_body.hpp"), os.path.join(CSRC, "rec_body.hpp"), os.path.join(CSRC, "finish_body.hpp"), os.path.join(CSRC, "wave_spmd.hpp"), os.path.join(EMU_DIR, "emu_hip.hpp"),
        os.path.join(T.ROOT, "include", "nabwa.h")]


def load_emu(flush_bytes=None):
    """the bodies as a library; flush_bytes: DMG_FLUSH_BYTES, so that a few hundred bytes of records take the paths that gigabytes take"""
    name, flags = "libdamage_emu.so", ["-O2", "-fPIC", "-shared"]
    if flush_bytes is not None:
        name, flags = "libdamage_emu_f%d.so" % flush_bytes, flags + ["-DDMG_FLUSH_BYTES=%dull" % flush_bytes]
    lib = C.CDLL(_build(os.path.join(EMU_DIR, name), [os.path.join(EMU_DIR, "damage_emu.cpp")], BODY, flags))
    P = C.c_void_p
    lib.emu_damage_run.restype = C.c_int64
    lib.emu_damage_run.argtypes = [C.c_int64, P, P, P, C.c_int64, C.c_int, P, P, C.c_int, P, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_int, P]
    return lib


def build_main():
    """the stand-alone program, under AddressSanitizer and UndefinedBehaviorSanitizer"""
    return _build(os.path.join(EMU_DIR, "damage_main_asan"), [os.path.join(EMU_DIR, "damage_main.cpp"), os.path.join(EMU_DIR, "damage_emu.cpp")], BODY,
                  ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])


def emu_add(emu, ref, opt, recs, words, n_blocks=3):
    """one call through the bodies on the CPU: `words` (a table as Tables.words()) += the call's table; -> -1, or the lowest damaged record and
    `words` as it was"""
    data, off = join(recs)
    data = np.ascontiguousarray(data) if len(data) else np.zeros(1, np.uint8)
    ho = np.array([h[0] for h in ref.holes], np.int64)
    hl = np.array([h[1] for h in ref.holes], np.int32)
    return emu.emu_damage_run(len(recs), T.ptr(data), T.ptr(off), T.ptr(ref.pac), ref.l_pac, len(ref.holes), T.ptr(ho), T.ptr(hl), len(ref.contigs), T.ptr(ref.offsets),
                              opt["n_pos"], opt["min_mapq"], opt["exclude_flags"], opt["require_flags"], n_blocks, T.ptr(words))


def emu_tables(emu, ref, opt, recs, n_blocks=3):
    w = np.zeros(Tables(opt["n_pos"]).words().size, np.uint64)
    bad = emu_add(emu, ref, opt, recs, w, n_blocks)
    if bad >= 0:
        assert not w.any(), "a failed call counted"
        raise Damaged(int(bad))
    return Tables.from_words(opt["n_pos"], w)


def write_case_file(path, ref, items):
    """the cases as data for tests/emu/damage_main.cpp.  items: (options, records, expected table words or None, expected damaged index or -1).
    Little-endian: a file header of l_pac, its pac bytes, holes and contigs; then per case its numbers, offsets, bytes and expected words"""
    with open(path, "wb") as f:
        f.write(struct.pack("<qqq", ref.l_pac, len(ref.holes), len(ref.contigs)))
        f.write(ref.pac.tobytes())
        for o, n in ref.holes:
            f.write(struct.pack("<qq", o, n))
        f.write(ref.offsets.astype("<i8").tobytes())
        f.write(struct.pack("<q", len(items)))
        for opt, recs, words, bad in items:
            data, off = join(recs)
            n_words = Tables(opt["n_pos"]).words().size
            f.write(struct.pack("<qqqqqqqq", len(recs), len(data), opt["n_pos"], opt["min_mapq"], opt["exclude_flags"], opt["require_flags"], bad, n_words))
            f.write(off.astype("<i8").tobytes())
            f.write(data.tobytes())
            f.write((np.zeros(n_words, np.uint64) if words is None else words).astype("<u8").tobytes())


# ---------------------------------------------------------------------------------------------------------------- the tool's file
def profile_text(t):
    """what `nabwa_bam2bam --damage FILE` writes for the tables t"""
    out = ["# nabwa damage profile v1"] + ["# %s %d" % (n, int(v)) for n, v in zip(STAT_NAMES, t.stats)]
    out.append("end\tpos\t" + "\t".join("%s>%s" % (r, q) for r in "ACGT" for q in "ACGT"))
    for end, sub in (("5p", t.sub5), ("3p", t.sub3)):
        for p in range(t.n_pos + 1):
            out.append("%s\t%s\t" % (end, p + 1 if p < t.n_pos else ">%d" % t.n_pos) + "\t".join(str(int(x)) for x in sub[p].reshape(-1)))
    out += ["len\t%d\t%d" % (L, int(c)) for L, c in enumerate(t.len_hist) if c]
    return "\n".join(out) + "\n"


def summary_line(t):
    """the line the tool says on stderr: the records counted, C>T at the first 5' base among the reference's C there, G>A at the first 3' base"""
    def freq(sub, r, q):
        tot = int(sub[0, r].sum())
        return "%.4f" % (int(sub[0, r, q]) / tot) if tot else "nan"
    return "[nabwa_bam2bam] damage profile of %d records: 5' C>T at position 1 %s, 3' G>A at position 1 %s" % (int(t.stats[COUNTED]), freq(t.sub5, 1, 3), freq(t.sub3, 2, 0))


def split_records(raw):
    """the records of an uncompressed BAM record stream"""
    out, q = [], 0
    while q < len(raw):
        n = 4 + struct.unpack_from("<I", raw, q)[0]
        out.append(raw[q:q + n])
        q += n
    assert q == len(raw)
    return out
