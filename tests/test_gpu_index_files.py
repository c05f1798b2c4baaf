"""The index AT SIZE from files in the reference's on-disk layout: the synthetic GRCh38-sized
FM-indexes bench.py builds on the GPU are written out as <prefix>.bwt / .rbwt / .sa / .rsa / .pac / .ann / .amb (bwtio.c:161-204,
bntseq.c:63-117,240-250) -- 240 contigs of unequal lengths, 3000 ambiguity holes -- and loaded with nabwa_index_load(prefix, with_sa,
with_pac): the search of the headline reads gives the rows (checksum) the index made from the same arrays in memory gives, the
annotation comes back as written, and a sample of reads placed on contig borders and holes goes through the finishing chain against
the compiled reference loading the SAME files (bns_restore, bwt_restore_*).  Falls back to 256 Mbp where /tmp is short of room."""
import ctypes as C
import importlib
import os
import shutil

import numpy as np
import pytest

import bigindex as BI
import nabwa_testlib as T

nabwa = importlib.import_module("network-aware-bwa_amd")
synth = importlib.import_module("network-aware-bwa_amd.synth")
pytestmark = pytest.mark.gpu


def test_genome_sized_index_from_reference_format_files(tmp_path_factory):
    n = int(os.environ.get("NABWA_TEST_GENOME", 3_099_734_149))
    root = os.environ.get("NABWA_TEST_TMP", "/tmp")
    if shutil.disk_usage(root).free < 3 * n:                      # ~1.5 bytes per base on disk, with room to spare
        n = 256_000_000
    d = os.path.join(root, "nabwa_index_files_%d" % os.getpid())
    os.makedirs(d, exist_ok=True)
    prefix = os.path.join(d, "synth")
    try:
        run(n, prefix)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def run(n, prefix):
    n_reads = 2_000_000 if n > 1_000_000_000 else 300_000
    d_text = synth.synth_text(n, 20261004, n_dup=2000, dup_len=5000, device=0)
    parts = [synth.build_index(d_text, n, rev, 32, True, device=0) for rev in (0, 1)]
    seq, rseq, off = synth.synth_reads(d_text, n, n_reads, 100, 2000, 0, 2, device=0)
    opt = nabwa.gap_init_opt()
    # ---- the index from the arrays in memory: the rows to expect
    ix = nabwa.Index.from_arrays((parts[0][0].ptr, parts[0][1]), (parts[1][0].ptr, parts[1][1]), (parts[0][2].ptr, parts[0][3]), (parts[1][2].ptr, parts[1][3]),
                                 device=0, device_ptrs=True)
    b = nabwa.Batch(ix, opt, seq, rseq, off, per_read=True)
    b.run(); b.sync()
    want_sum = b.checksum()
    b.close(); ix.close()
    # ---- the same arrays as files of the reference's formats
    BI.write_index_words(prefix, parts)
    pac = BI.pack_pac(d_text, n)
    d_text.free()
    BI.write_pac(prefix, pac, n)
    rng = np.random.default_rng(8)
    n_ctg = 240
    names, offs, lens, hole_off, hole_len, cuts = BI.write_ann_amb(prefix, n, rng, n_ctg, 3000)
    # ---- loaded from the files
    ix = nabwa.Index.load(prefix, 0, True, True)
    L = nabwa.lib()
    assert ix.seq_len(0) == n and ix.seq_len(1) == n
    assert L.nabwa_index_n_contigs(ix._h) == n_ctg
    L.nabwa_index_contig.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p]
    L.nabwa_index_reference_info.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    for i in (0, 1, 119, n_ctg - 1):
        nm, o, l = C.create_string_buffer(64), C.c_int64(), C.c_int32()
        assert L.nabwa_index_contig(ix._h, i, nm, 64, C.byref(o), C.byref(l)) == 0
        assert (nm.value.decode(), o.value, l.value) == (names[i], int(offs[i]), int(lens[i]))
    lp, sd = C.c_int64(), C.c_uint32()
    assert L.nabwa_index_reference_info(ix._h, C.byref(lp), C.byref(sd)) == 0 and (lp.value, sd.value) == (n, 11)
    b = nabwa.Batch(ix, opt, seq, rseq, off, per_read=True)
    b.run(); b.sync()
    assert b.checksum() == want_sum                          # the same rows for every one of the reads
    hits_head = b.fetch_flat()
    b.close()
    # ---- a sample through the finishing chain against the reference loading the same files: reads cut where contigs meet and where holes lie
    ref = T.load_ref()
    if ref is None:
        ix.close()
        pytest.skip("oracle/_ref did not travel: rows and annotation checked, the chain against the reference not")
    text_at = lambda p, l: np.array([(pac[(p + j) >> 2] >> ((~(p + j) & 3) << 1)) & 3 for j in range(l)], np.uint8)
    starts = []
    for c in cuts[:60]:
        starts += [int(c) - 100, int(c) - 37, int(c)]          # inside a contig's end, across the border, at the next one's start
    for o, l in list(zip(hole_off, hole_len))[:120]:
        starts += [int(o) - 50, int(o) + int(l) - 30]           # into a hole, out of one
    starts += [int(x) for x in rng.integers(0, n - 100, 400)]
    reads = []
    for k, p in enumerate(starts):
        r = text_at(p, 100)
        if k % 4 == 1:
            r = r.copy(); r[int(rng.integers(10, 90))] ^= 1      # a substitution
        if k % 9 == 2:
            c0 = int(rng.integers(20, 80))
            r = np.concatenate([r[:c0], r[c0 + 1:], text_at(p + 100, 1)])      # a deleted base
        if k % 2:
            r = (3 - r)[::-1]                                    # the other strand
        reads.append(r)
    s_seq = np.concatenate([r[::-1] for r in reads]).astype(np.uint8)              # bwa_seq_t.seq: the read reversed; rseq: its complement
    s_rseq = (3 - s_seq).astype(np.uint8)
    s_off = np.arange(len(reads) + 1, dtype=np.int64) * 100
    ref.ref_index_load.restype = C.c_void_p
    ref.ref_index_load.argtypes = [C.c_char_p, C.c_int]
    rix = C.c_void_p(ref.ref_index_load(prefix.encode(), 1))
    n_map, n_hole, n_bridge, _ = BI.se_chain_vs_reference(ix, ref, rix, opt, s_seq, s_rseq, s_off)
    ref.ref_index_free(rix)
    assert n_map > 0.9 * len(reads) and n_hole >= 100 and n_bridge >= 20
    ix.close()
