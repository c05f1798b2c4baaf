"""Helpers for the tests of indexes at genome size and beyond: the synthetic text and its FM-indexes (built on the GPU by
network-aware-bwa_amd.synth) written out as the reference's files -- .bwt / .rbwt / .sa / .rsa (bwtio.c:161-204), .pac
(bntseq.c:240-250), .ann / .amb (bntseq.c:63-85).  Test infrastructure only."""
import ctypes as C
import importlib

import numpy as np

import nabwa_testlib as T

nabwa = importlib.import_module("network-aware-bwa_amd")


def pack_pac(d_text, n):
    """the .pac bytes of a device text of n base codes (0-3, one byte each): four bases per byte, first one in the top bits"""
    t = d_text.to_host(np.uint8)[:n]
    pad = (-n) % 4
    if pad:
        t = np.concatenate([t, np.zeros(pad, np.uint8)])
    t = t.reshape(-1, 4)
    return np.ascontiguousarray((t[:, 0] << 6) | (t[:, 1] << 4) | (t[:, 2] << 2) | t[:, 3]).astype(np.uint8)


def write_pac(prefix, pac, n):
    """bntseq.c:240-250: the packed bases, a zero byte when they end on a byte border, the count of bases in the last byte"""
    with open(prefix + ".pac", "wb") as f:
        f.write(pac.tobytes())
        if n % 4 == 0:
            f.write(b"\0")
        f.write(bytes([n % 4]))


def write_index_words(prefix, parts):
    """parts = [(bwt DevArray, n_words, sa DevArray, n_sa_words)] forward, reverse (synth.build_index); the device arrays are freed"""
    for t, (bw, nbw, sa, nsa) in enumerate(parts):
        bw.to_host(np.uint32, nbw).tofile(prefix + (".rbwt" if t else ".bwt"))        # primary, L2[1..4], then the Occ-interleaved BWT words (bwtio.c:184-204)
        sa.to_host(np.uint32, nsa).tofile(prefix + (".rsa" if t else ".sa"))          # primary, 4 skipped words, sa_intv, seq_len, then the samples (bwtio.c:161-182)
        bw.free(); sa.free()


def write_ann_amb(prefix, n, rng, n_ctg=240, n_holes=3000, cuts=None, holes=None):
    """.ann / .amb (bns_dump, bntseq.c:63-75) of n_ctg contigs of unequal lengths, each under 2^31 (bntann1_t.len is an int), and
    n_holes ambiguity holes that do not overlap -> (names, offsets, lengths, hole offsets, hole lengths, the contigs' cuts).
    cuts (the n_ctg - 1 contig starts after the first) and holes ((offset, length) pairs) may be given instead of drawn from rng."""
    if cuts is None:
        cuts = np.sort(rng.choice(np.arange(1000, n - 1000), n_ctg - 1, replace=False))
    cuts = np.asarray(cuts, np.int64)
    n_ctg = len(cuts) + 1
    offs = np.concatenate([[0], cuts]).astype(np.int64)
    lens = np.diff(np.concatenate([offs, [n]])).astype(np.int64)
    assert lens.max() < 2**31
    names = ["ctg%03d" % i for i in range(n_ctg)]
    if holes is None:
        hole_off = np.sort(rng.choice(np.arange(5000, n - 5000), n_holes, replace=False)).astype(np.int64)
        hole_len = rng.integers(1, 2000, n_holes).astype(np.int64)
    else:
        hole_off = np.array([o for o, _ in holes], np.int64)
        hole_len = np.array([l for _, l in holes], np.int64)
        n_holes = len(holes)
    hole_len = np.minimum(hole_len, np.diff(np.concatenate([hole_off, [n]])) - 1)    # holes do not overlap
    ctg_of_hole = np.searchsorted(offs, hole_off, side="right") - 1
    with open(prefix + ".ann", "w") as f:
        f.write("%d %d %u\n" % (n, n_ctg, 11))
        for i in range(n_ctg):
            f.write("%d %s a synthetic contig\n" % (i, names[i]) if i % 3 else "%d %s\n" % (i, names[i]))
            f.write("%d %d %d\n" % (offs[i], lens[i], int((ctg_of_hole == i).sum())))
    with open(prefix + ".amb", "w") as f:
        f.write("%d %d %d\n" % (n, n_ctg, n_holes))
        for o, l in zip(hole_off, hole_len):
            f.write("%d %d N\n" % (o, l))
    return names, offs, lens, hole_off, hole_len, cuts


def se_chain_vs_reference(ix, ref, rix, opt, s_seq, s_rseq, s_off, n_occ=3, seed=11):
    """the reads' hits through the finishing chain (ix.se_finish: positions, strand, mapQ, gapped refinement, MD/NM, contig and N count)
    and through the compiled reference's chain (ref_se_chain_mt, bwase.c) on the files of the same index, field by field.
    ix must have its reference attached; rix = ref_index_load(prefix, 1).  -> (mapped, over a hole, bridging two contigs, the records)"""
    n = len(s_off) - 1
    full = np.diff(s_off).astype(np.int32)
    hits, _ = ix.cal_sa_reg_gap(opt, s_seq, s_rseq, s_off, per_read=True)
    recs, _ = ix.se_finish(opt, s_seq, s_rseq, s_off, full, hits, n_occ, nabwa.srand48_state(seed))
    P = C.c_void_p
    ref.ref_se_chain_mt.argtypes = [P, P, C.c_int, C.c_int, P, P, P, P, P, C.c_int, P, P, P, C.c_int, P]
    ref.ref_pac2real.argtypes = [P, C.c_int64, C.c_int, P, P]
    copt = T.GapOpt(); C.memmove(C.byref(copt), C.byref(opt), 64)
    na = np.array([len(h) for h in hits], np.int32)
    rows = np.ascontiguousarray(np.concatenate([np.asarray(h, nabwa.ALN_DT) for h in hits] + [np.zeros(0, nabwa.ALN_DT)]))
    f = np.zeros((n, 16), np.int64); cg = np.zeros((n, 64), np.uint16); md = np.zeros((n, 256), np.uint8)
    secs = (C.c_double * 2)()
    ref.ref_seed48(seed)
    ref.ref_se_chain_mt(rix, C.byref(copt), n_occ, n, T.ptr(s_off), T.ptr(s_seq), T.ptr(s_rseq), T.ptr(na), T.ptr(rows), 4, T.ptr(f), T.ptr(cg), T.ptr(md), 256, secs)
    n_map = n_hole = n_bridge = 0
    for i in range(n):
        s, w = recs[i], f[i]
        assert s.type == w[0], i
        if s.type == 0:
            continue
        n_map += 1
        bridging = bool(s.flag & 4)
        n_bridge += bridging
        assert [s.strand, s.n_mm, s.n_gapo, s.n_gape, s.score, s.sa, s.c1, s.c2, s.pos] == [int(x) for x in w[1:10]], i
        assert bridging or s.mapQ == w[10], i
        assert s.n_cigar == w[12] and list(s.cigar[:s.n_cigar]) == list(cg[i, :s.n_cigar]) and s.nm == w[13], i
        assert s.md == bytes(md[i]).split(b"\0", 1)[0], i           # N's of the holes restored in MD (bwase.c:243-268)
        sid, o = C.c_int32(), C.c_int64()
        ln = int(full[i]) if s.n_cigar == 0 else sum((c & 0x3fff) for c in s.cigar[:s.n_cigar] if (c >> 14) in (0, 2))
        nn = ref.ref_pac2real(rix, int(s.pos), ln, C.byref(sid), C.byref(o))
        assert (s.seqid, s.rpos, s.nn) == (sid.value, int(s.pos) - o.value + 1, nn), (i, s.seqid, s.rpos, s.nn, sid.value, o.value, nn)
        n_hole += nn > 0
    return n_map, n_hole, n_bridge, recs
