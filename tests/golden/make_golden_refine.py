"""Regenerates tests/golden/vectors_refine.npz: positioned hits on the toy index with what the compiled reference's bwa_refine_gapped
(ref_refine_one, oracle/ref_harness.c) makes of them -- position, CIGAR, NM, MD.  Inputs and recorded results only.

Needs oracle/_ref/libbwaref.so (build() makes it where the reference is at hand) and oracle/liboracle.so.  A read is cut from the packed
toy reference with substitutions, insertions and deletions planted, and n_gapo / n_gape set to match; the position is the one
bwa_cal_pac_pos would hand on (reverse strand: the hit's start; forward strand: its end minus the read length).  Every case is one where
the reference is defined: its window is not empty, and an ungapped hit ends inside the text.  The generator asserts both, and that the
aspects listed in COVER are all met."""
import ctypes as C
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nabwa_testlib as T  # noqa: E402

L_PAC = 103000
HOLES = [(45000, 200), (52000, 3), (90000, 1)]
LENS = [17, 63, 64, 65, 100, 150, 257]
MAXC = 32
MAQ = np.array([11, -19, -19, -19, -13, -19, 11, -19, -19, -13, -19, -19, 11, -19, -13, -19, -19, -19, 11, -13, -13, -13, -13, -13, -13], np.int32)


def pac_bases():
    pac = np.fromfile(T.TOY + ".pac", np.uint8)
    k = np.arange(L_PAC)
    return (pac[k >> 2] >> ((~k & 3) << 1) & 3).astype(np.uint8)


def extent(pos, length, ext):
    """the window of bwase.c:197-209 (is_end_correct = 1)"""
    ref_len = length + abs(ext)
    p = pos - (1 << 32) if pos > L_PAC and pos >= (1 << 31) else pos
    if ext > 0:
        lo, hi = max(p, 0), min(p + ref_len, L_PAC)
    else:
        x = p + length
        lo, hi = max(x - ref_len, 0), min(x, L_PAC)
    return lo, max(hi - lo, 0)


class Maker:
    def __init__(self):
        self.base = pac_bases()
        self.rng = np.random.default_rng(20240607)
        self.cases = []

    def query(self, p, length, edits):
        """the read in alignment orientation: reference bases from p on with edits = [(read position, kind, k)] applied left to right;
        kind 'X' substitutes one base, 'N' makes it an N, 'I' inserts k random bases in front of the position, 'D' skips k reference bases
        in front of it.  -> (codes, reference bases consumed)"""
        ed = {}
        for at, kind, k in edits:
            ed.setdefault(at, []).append((kind, k))
        q, g = [], p
        while len(q) < length:
            at = len(q)
            todo = ed.pop(at, [])
            ins = [k for kind, k in todo if kind == "I"]
            dele = [k for kind, k in todo if kind == "D"]
            for k in dele:
                g += k
            if ins:
                for _ in range(ins[0]):
                    if len(q) < length:
                        q.append(int(self.rng.integers(0, 4)))
                ed[len(q)] = [(kind, k) for kind, k in todo if kind in "XN"] + ed.get(len(q), [])
                continue
            b = int(self.base[g]) if 0 <= g < L_PAC else int(self.rng.integers(0, 4))
            if any(kind == "X" for kind, _ in todo):
                b = (b + 1 + int(self.rng.integers(0, 3))) & 3
            if any(kind == "N" for kind, _ in todo):
                b = 4
            q.append(b)
            g += 1
        return np.array(q, np.uint8), g - p

    def add(self, tag, p, length, strand, edits=(), pos=None):
        """a hit whose alignment starts at reference position p.  pos: the position handed to the refinement, worked out when None"""
        q, used = self.query(p, length, list(edits))
        n_ins = sum(k for _, kind, k in edits if kind == "I")
        n_del = sum(k for _, kind, k in edits if kind == "D")
        n_gapo = sum(1 for _, kind, _ in edits if kind in "ID")
        n_gape = n_ins + n_del - n_gapo
        if pos is None:
            pos = p if strand else p + used - length      # forward strand: the end is anchored (bwa_cal_pac_pos)
        pos &= 0xffffffff
        ext = (1 if strand else -1) * (n_gapo + n_gape)
        if n_gapo:
            lo, wn = extent(pos, length, ext)
            assert wn > 0, (tag, "empty window")
        else:
            assert pos + length <= L_PAC, (tag, "ungapped hit past the end of the text")
        if strand:      # the query is rseq = the reverse complement of the read
            rseq = q
            seq = np.where(q < 4, 3 - q, q).astype(np.uint8)
        else:           # the query is the read; seq holds it reversed
            seq = q[::-1].copy()
            rseq = np.where(seq < 4, 3 - seq, seq).astype(np.uint8)
        self.cases.append(dict(tag=tag, seq=seq, rseq=rseq, strand=strand, n_gapo=n_gapo, n_gape=n_gape, pos=pos, len=length))

    def build(self):
        r = self.rng
        # lengths x strands x pac phases: ungapped, insertions and deletions
        for length in LENS:
            for strand in (0, 1):
                for phase in range(4):
                    p = int(r.integers(2000, 40000)) // 4 * 4 + phase
                    mid = length // 2
                    self.add("ungapped", p, length, strand, [(int(r.integers(0, length)), "X", 1)])
                    self.add("ins1", p + 400, length, strand, [(mid, "I", 1), (int(r.integers(0, mid)), "X", 1)])
                    self.add("ins2", p + 800, length, strand, [(mid, "I", 2)])
                    self.add("del1", p + 1200, length, strand, [(mid, "D", 1)])
                    self.add("del3", p + 1600, length, strand, [(mid, "D", 3), (min(length - 1, mid + 3), "X", 1)])
        # mismatch positions and patterns (ungapped and behind an insertion), run lengths of one, two and three digits, an N in the read
        for strand in (0, 1):
            for length in (65, 150, 257):
                for at in sorted({0, length - 1, 63, 64}):
                    self.add("mm@%d" % at, 3001 + 7 * at, length, strand, [(at, "X", 1)])
                    self.add("mm@%d+ins" % at, 5003 + 7 * at, length, strand, [(at, "X", 1), (30, "I", 1)] if at != 30 else [(at, "X", 1)])
                self.add("adjacent", 7000, length, strand, [(20, "X", 1), (21, "X", 1)])
                self.add("adjacent64", 7100, length, strand, [(63, "X", 1), (64, "X", 1)])
                self.add("N", 7200, length, strand, [(10, "N", 1)])
                self.add("N+del", 7300, length, strand, [(10, "N", 1), (40, "D", 2)])
            self.add("digits", 8000, 257, strand, [(5, "X", 1), (50, "X", 1), (200, "X", 1)])        # 5, 44, 149, 56
            self.add("clean", 8300, 257, strand)
            self.add("clean+del", 8600, 257, strand, [(130, "D", 1)])
        # CIGAR end rules: indels at the very ends of the read
        for strand in (0, 1):
            for length in (64, 100):
                self.add("ins@0", 9000, length, strand, [(0, "I", 2)])
                self.add("ins@end", 9300, length, strand, [(length - 2, "I", 2)])
                self.add("ins@1", 9600, length, strand, [(1, "I", 1)])
                self.add("del@1", 9900, length, strand, [(1, "D", 2)])
                self.add("del@end", 10200, length, strand, [(length - 1, "D", 2)])
                self.add("ins+del", 10500, length, strand, [(20, "I", 2), (50, "D", 1)])           # net insertion
                self.add("del+ins", 10800, length, strand, [(20, "D", 3), (50, "I", 1)])           # net deletion
        # window clipped at 0 on the forward strand -- pos = -2 as 0xfffffffe included (bwase.c:197) --, at l_pac on the reverse strand
        self.add("clip0", 0, 64, 0, [(30, "I", 2)])
        assert self.cases[-1]["pos"] == 0xfffffffe
        self.add("clip0", 0, 100, 0, [(50, "I", 1)])
        self.add("clip0", 1, 65, 0, [(30, "I", 3)])
        self.add("clip0", 0, 63, 0, [(30, "D", 2)])
        self.add("clip0", 2, 100, 1, [(50, "I", 2)])
        self.add("clip0", 0, 100, 1, [(50, "D", 2)])
        for length, k in ((64, 1), (100, 2), (257, 3)):
            self.add("clipL", L_PAC - length - 1, length, 1, [(length // 2, "I", k)])
            self.add("clipL", L_PAC - length - k, length, 1, [(length // 2, "D", k)])
            self.add("clipL", L_PAC - length - k - 2, length, 0, [(length // 2, "D", k)])
            self.add("ungapped-end", L_PAC - length, length, 1, [(length - 1, "X", 1)])
            self.add("ungapped-end", L_PAC - length, length, 0, [(0, "X", 1)])
        # end of the text: a gapped hit on the forward strand whose anchored end lies past l_pac -- its M runs into l_pac
        for length, over in ((64, 3), (100, 5), (150, 1)):
            self.add("M-into-l_pac", L_PAC - length + over, length, 0, [(length // 2, "I", 1)], pos=L_PAC - length + over)
            self.add("M-into-l_pac", L_PAC - length + over, length, 0, [(length // 3, "D", 2)], pos=L_PAC - length + over)
        # holes: a hit that starts inside one, ends inside one, spans one, deletes hole bases
        for strand in (0, 1):
            self.add("hole-start", 45100, 100, strand, [(70, "X", 1)])
            self.add("hole-start", 45150, 100, strand, [(80, "I", 1)])
            self.add("hole-end", 44950, 100, strand, [(10, "X", 1)])
            self.add("hole-end", 44940, 100, strand, [(20, "D", 2)])
            self.add("hole-span", 51950, 100, strand)
            self.add("hole-span", 89990, 65, strand, [(40, "I", 1)])
            self.add("hole-span", 44900, 257, strand, [(20, "D", 1)])
            self.add("hole-del", 51950, 100, strand, [(50, "D", 3)])                              # ^NNN
            self.add("hole-del", 89950, 100, strand, [(50, "D", 1)])                              # ^N
            self.add("hole-del", 51960, 150, strand, [(40, "D", 5), (100, "X", 1)])


COVER = ["leading D", "trailing D", "leading I", "trailing I", "shift+", "shift-", "^N", "0A0C-like", "three digits"]


def main():
    ref = T.load_ref()
    assert ref is not None, "oracle/_ref/libbwaref.so is missing"
    olib = T.load_oracle()
    rix = C.c_void_p(ref.ref_index_load(T.TOY.encode(), 1))
    ref.ref_refine_one.restype = None
    ref.ref_refine_one.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_uint32] + [C.c_void_p] * 5 + [C.c_int]
    M = Maker()
    M.build()
    base = M.base
    n = len(M.cases)
    pos_out = np.zeros(n, np.uint32)
    n_cig = np.zeros(n, np.int32)
    cig = np.zeros((n, MAXC), np.uint16)
    nm = np.zeros(n, np.int32)
    mds = []
    seen = set()
    for i, c in enumerate(M.cases):
        po, nc, nmv = C.c_uint32(0), C.c_int(0), C.c_int(0)
        row = np.zeros(256, np.uint16)
        md = C.create_string_buffer(2048)
        ref.ref_refine_one(rix, c["len"], T.ptr(c["seq"]), T.ptr(c["rseq"]), 1, c["strand"], 0, c["n_gapo"], c["n_gape"], c["pos"],
                           C.byref(po), C.byref(nc), T.ptr(row), C.byref(nmv), md, 2048)
        assert nc.value <= MAXC
        pos_out[i], n_cig[i], nm[i] = po.value, nc.value, nmv.value
        cig[i, :nc.value] = row[:nc.value]
        mds.append(md.value)
        # which aspects this case covers: the raw path of the alignment, from the oracle's aln_global_core
        if c["n_gapo"]:
            ext = (1 if c["strand"] else -1) * (c["n_gapo"] + c["n_gape"])
            lo, wn = extent(c["pos"], c["len"], ext)
            q = c["rseq"] if c["strand"] else c["seq"][::-1].copy()
            w = base[lo:lo + wn].copy()
            c32 = np.zeros(512, np.uint32)
            ncc = C.c_int(0)
            olib.orc_global(T.ptr(w), wn, T.ptr(q), len(q), 26, 9, 5, T.ptr(MAQ), 5, 50, T.ptr(c32), C.byref(ncc))
            ops = [int(x) & 0xf for x in c32[:ncc.value]]
            seen.add({1: "leading I", 2: "leading D"}.get(ops[0]))
            seen.add({1: "trailing I", 2: "trailing D"}.get(ops[-1]))
            if ext < 0:
                d = sum((int(x) >> 4) * {1: 1, 2: -1}.get(int(x) & 0xf, 0) for x in c32[:ncc.value])
                seen.add("shift+" if d > 0 else "shift-" if d < 0 else None)
        s = md.value.decode()
        if "^N" in s:
            seen.add("^N")
        if re.search(r"[ACGTN]0[ACGTN]", s):
            seen.add("0A0C-like")
        if re.search(r"\d{3}", s):
            seen.add("three digits")
    missing = [a for a in COVER if a not in seen]
    assert not missing, missing
    seq = np.concatenate([c["seq"] for c in M.cases])
    rseq = np.concatenate([c["rseq"] for c in M.cases])
    off = np.concatenate([[0], np.cumsum([c["len"] for c in M.cases])]).astype(np.int64)
    md_off = np.concatenate([[0], np.cumsum([len(m) + 1 for m in mds])]).astype(np.int64)
    out = os.path.join(HERE, "vectors_refine.npz")
    np.savez_compressed(out, seq=seq, rseq=rseq, off=off,
                        strand=np.array([c["strand"] for c in M.cases], np.int32), n_gapo=np.array([c["n_gapo"] for c in M.cases], np.int32),
                        n_gape=np.array([c["n_gape"] for c in M.cases], np.int32), pos=np.array([c["pos"] for c in M.cases], np.uint32),
                        tag=np.array([c["tag"] for c in M.cases]), pos_out=pos_out, n_cigar=n_cig, cigar=cig, nm=nm,
                        md=np.frombuffer(b"".join(m + b"\0" for m in mds), np.uint8), md_off=md_off)
    print("%d cases (%d gapped), %d bytes" % (n, int((n_cig > 0).sum()), os.path.getsize(out)))


if __name__ == "__main__":
    main()
