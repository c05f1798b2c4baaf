"""The finishing chains split their records over host threads (NABWA_HOST_THREADS, at most 16 by default): the records they
write must not depend on how many threads there are.  One single-end and one paired-end batch, each above the size below which
the chains stay on one thread (4096 records / pairs), run once on one thread and once with the default, byte for byte."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import nabwa_testlib as T

pytestmark = pytest.mark.gpu
nabwa = importlib.import_module("network-aware-bwa_amd")

REPEAT = 10                                      # the fixture's reads repeated: 606 reads -> 6060, 436 pairs -> 4360


def both_ways(monkeypatch, run):
    monkeypatch.setenv("NABWA_HOST_THREADS", "1")
    one = run()
    monkeypatch.delenv("NABWA_HOST_THREADS")
    many = run()
    assert one == many


def test_se_finish_same_on_one_thread(monkeypatch):
    opt, _ = T.read_sai(os.path.join(T.GOLDEN, "se_default.sai"))
    reads = T.read_fastq(os.path.join(T.GOLDEN, "reads_se.fq")) * REPEAT
    assert len(reads) >= 4096
    seq, rseq, off, full = T.encode_reads(reads, opt.trim_qual)
    g = nabwa.GapOpt()
    C.memmove(C.byref(g), C.byref(opt), 64)
    ix = nabwa.Index.load(T.TOY, 0, True, True)
    hits, _ = ix.cal_sa_reg_gap(g, seq, rseq, off, per_read=False)

    def run():
        out, st = ix.se_finish(g, seq, rseq, off, full, hits, 3, nabwa.srand48_state(11))
        assert sum(out[i].n_cigar > 0 for i in range(len(reads))) > 0       # gap refinement ran
        return bytes(out), st
    both_ways(monkeypatch, run)
    ix.close()


def test_pe_finish_same_on_one_thread(monkeypatch):
    ix = nabwa.Index.load(T.TOY)
    ix.attach_reference(T.TOY)
    fq = [T.read_fastq(os.path.join(T.GOLDEN, "reads_pe_%d.fq" % e)) * REPEAT for e in (1, 2)]
    sai = [T.read_sai(os.path.join(T.GOLDEN, "pe_%d.sai" % e)) for e in (1, 2)]
    n = len(fq[0])
    assert n >= 4096
    inter = [fq[e][i] for i in range(n) for e in range(2)]
    hits = [sai[e][1][i % len(sai[e][1])] for i in range(n) for e in range(2)]
    seq, rseq, off, full = T.encode_reads(inter)
    opt = sai[1][0]
    iv = np.load(os.path.join(T.GOLDEN, "vectors_pe_chain.npz"))["ii_sampe"]
    ii = nabwa.IsizeInfo(iv[0], iv[1], iv[2], int(iv[3]), int(iv[4]), int(iv[5]))

    def run():
        recs, st = ix.pe_posn(opt, off, full, hits, nabwa.srand48_state(11))
        tot, mp = ix.pe_finish(opt, nabwa.pe_opt_default(), ii, seq, rseq, off, hits, recs)
        assert mp[0] > 0                                                      # mate rescue ran
        return bytes(recs), st, tot, mp
    both_ways(monkeypatch, run)
    ix.close()
