"""The statistics lines of the counting run (NABWA_TRIP_STATS): the counters kernels W and S write into the touch block
and the class counters of the partition, read back by slot (csrc/search_slots.hpp).  A slot mixed up on either side
prints a wrong number silently; the relations below hold for any correct map, whatever the tuning."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import nabwa_testlib as T

pytestmark = pytest.mark.gpu
nabwa = importlib.import_module("network-aware-bwa_amd")

N_READS = 96
LANE_KINDS = ["expand", "exact", "entry-load", "spec", "query", "two-bucket", "exited", "tail-jump", "text-expand", "text-tail"]
TRIPS_RE = re.compile(r"\[nabwa\] search kernel: wave-trips (\d+); lane-trips: " + " ".join(k + r" (\d+)" for k in LANE_KINDS)
                      + r"; longest read (\d+) trips, (\d+) reads over 2000 trips, (\d+) over 500\n")
CLASS_RE = re.compile(r"\[nabwa\] read classes by restarts 0 / 1 / 2\+: (\d+) / (\d+) / (\d+)\n")


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def make_reads():
    """reads kernel S finishes itself: windows of the genome that occur once, 40-60 bases, either strand -- half of them as they
    are, half with one base substituted"""
    genome = "".join(s for _, s in T.read_fasta(T.TOY + ".fa")).upper()
    both = genome + "N" + revcomp(genome)          # (an N stays an N: no window matches across it)
    rng = np.random.default_rng(20)
    reads = []
    while len(reads) < N_READS:
        L = int(rng.integers(40, 61))
        p = int(rng.integers(0, len(genome) - L))
        w = genome[p:p + L]
        if "N" in w or both.count(w) != 1:
            continue
        if len(reads) % 2:
            q = int(rng.integers(0, L))
            w = w[:q] + "ACGT"[("ACGT".index(w[q]) + 1 + int(rng.integers(0, 3))) % 4] + w[q + 1:]
        if rng.integers(0, 2):
            w = revcomp(w)
        reads.append(("t%d" % len(reads), w, "I" * L))
    return reads


@pytest.fixture(scope="module")
def gix():
    ix = nabwa.Index.load(T.TOY, 0, True)
    yield ix
    ix.close()


def counted(b, capfd, monkeypatch, mode):
    """one counting run -> (search touches, width touches, the trips line as a dict, the three class counts)"""
    monkeypatch.setenv("NABWA_TRIP_STATS", mode)
    capfd.readouterr()
    ts, tw = b.count_touches()
    err = capfd.readouterr().err
    m, c = TRIPS_RE.search(err), CLASS_RE.search(err)
    assert m and c, err
    v = [int(x) for x in m.groups()]
    trips = dict(zip(["wave-trips"] + LANE_KINDS + ["longest", "over2000", "over500"], v))
    return ts, tw, trips, [int(x) for x in c.groups()]


def test_trip_statistics_are_consistent(gix, capfd, monkeypatch):
    for k in ("NABWA_TIMING", "NABWA_DEEP_STATS", "NABWA_DEEP_HIST"):
        monkeypatch.delenv(k, raising=False)
    reads = make_reads()
    seq, rseq, off, _ = T.encode_reads(reads)
    opt = T.default_opt()
    g = nabwa.GapOpt()
    C.memmove(C.byref(g), C.byref(opt), 64)
    olib = T.load_oracle()
    ctr = T.Counters()
    T.oracle_cal_sa_reg_gap(olib, T.OracleIndex(olib).h, opt, seq, rseq, off, per_read=0, counters=ctr)
    b = nabwa.Batch(gix, g, seq, rseq, off, False)
    try:
        b.run()
        assert b.sync() == 0                     # kernel S finishes every read: kernel D is not launched
        has_tables = os.environ.get("NABWA_KMER_T", "") != "0"
        for mode in ("1", "jump"):
            ts, tw, t, cls = counted(b, capfd, monkeypatch, mode)
            assert sum(cls) == N_READS
            assert t["two-bucket"] <= t["query"]
            assert t["wave-trips"] >= 1
            for k in LANE_KINDS:
                assert t[k] <= 64 * t["wave-trips"], k
            assert t["over2000"] <= t["over500"] <= N_READS
            assert t["longest"] >= 1
            if mode == "1":
                # the interval tables and the text are off in this run; its touches are the reference's
                assert t["tail-jump"] == 0 and t["text-expand"] == 0 and t["text-tail"] == 0
                assert ts + tw == ctr.n_bucket and ts > 0 and tw > 0
            elif has_tables:
                assert t["tail-jump"] > 0
    finally:
        b.close()
