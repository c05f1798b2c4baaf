"""NABWA_DEDUP_CACHE through the command-line tools: nabwa_aln and nabwa_bam2bam cut their input into batches, every batch is made by
nabwa_batch_create, and the copies of a read that fall into later batches are served from the index's read cache.  The output must not change,
the summary line must show reads served, and a value the library would refuse ends the tools before the index is loaded."""
import gzip
import importlib
import os
import re
import subprocess

import pytest

import bamlib as B
import nabwa_testlib as T
from test_gpu_bam import pe_records
from test_gpu_bam2bam_cli import write_bam

pytestmark = pytest.mark.gpu
nabwa = importlib.import_module("network-aware-bwa_amd")
HERE = os.path.dirname(nabwa.LIB_PATH)
ALN, BAM2BAM = os.path.join(HERE, "nabwa_aln"), os.path.join(HERE, "nabwa_bam2bam")
SUMMARY = re.compile(r"\[nabwa_\w+\] dedup cache: (\d+) reads given, (\d+) searched, (\d+) served, (\d+) entries, (\d+) of (\d+) bytes")
SWITCHES = ("NABWA_DEDUP", "NABWA_DEDUP_HASH_BITS", "NABWA_DEDUP_CACHE", "NABWA_DEDUP_CACHE_ROWS", "NABWA_TIMING")


def env_with(**more):
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(more)
    return e


CHUNK = 0x40000      # nabwa_aln's batches are whole chunks of this many reads (the reference's, bwtaln.c:207), whatever smaller NABWA_ALN_BATCH asks for


def test_aln_writes_the_same_sai_and_serves_the_second_batch(tmp_path):
    """reads_se.fq given over and over until a second batch begins (NABWA_ALN_BATCH=64 means one chunk of 262144 reads): the first batch searches
    every distinct read once, the second is served whole, and the head of the .sai is the golden file"""
    reads = T.read_fastq(os.path.join(T.GOLDEN, "reads_se.fq"))
    times = CHUNK // len(reads) + 1
    assert 0 < times * len(reads) - CHUNK <= len(reads)
    fq = str(tmp_path / "many.fq")
    with open(fq, "w") as f:
        for rep in range(times):
            f.write("".join("@%d_%d\n%s\n+\n%s\n" % (i, rep, s, q) for i, (_, s, q) in enumerate(reads)))
    out = {}
    for sw in (False, True):
        e = env_with(NABWA_ALN_BATCH="64", **({"NABWA_DEDUP": "1", "NABWA_DEDUP_CACHE": "16"} if sw else {}))
        r = subprocess.run([ALN, T.TOY, fq], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=600)
        err = r.stderr.decode(errors="replace")
        assert r.returncode == 0, err[-2000:]
        out[sw] = r.stdout
        lines = SUMMARY.findall(err)
        assert len(lines) == (1 if sw else 0), err[-2000:]
        if sw:
            given, searched, served, entries, used, reserved = (int(x) for x in lines[0])
            distinct = len(set(s for _, s, _ in reads))
            in_second = len(set(s for _, s, _ in (reads * times)[CHUNK:]))
            assert (given, searched, served, entries) == (distinct + in_second, distinct, in_second, distinct)      # every distinct read is searched once in the whole run
            assert in_second > 100
            assert 0 < used <= reserved <= 16 << 20
    assert out[False] == out[True]
    gold = open(os.path.join(T.GOLDEN, "se_default.sai"), "rb").read()
    assert out[True][: len(gold)] == gold and len(out[True]) > len(gold)


def test_bam2bam_with_small_batches_writes_the_same_records(tmp_path):
    """single reads and pairs, every record twice under new names, in batches of 64 records"""
    pairs, n_pairs = pe_records()
    fq = [T.read_fastq(os.path.join(T.GOLDEN, "reads_pe_%d.fq" % e)) for e in (1, 2)]
    se = T.read_fastq(os.path.join(T.GOLDEN, "reads_se.fq"))[:150]
    recs = []
    for rep in range(2):
        for i in range(n_pairs):
            a, b = fq[0][i], fq[1][i]
            name = "%s_%d" % (a[0][:-2] if a[0].endswith("/1") else a[0], rep)
            recs += [B.make_record(name, a[1], a[2], 1 | 4 | 8 | 64), B.make_record(name, b[1], b[2], 1 | 4 | 8 | 128)]
        recs += [B.make_record("%s_%d" % (n, rep), s, q, 4) for n, s, q in se]
    inp = str(tmp_path / "in.bam")
    write_bam(inp, recs, True)
    out = {}
    for sw in (False, True):
        outp = str(tmp_path / ("out_%s.bam" % ("b" if sw else "a")))
        e = env_with(NABWA_BAM_BATCH="64", **({"NABWA_DEDUP": "1", "NABWA_DEDUP_CACHE": "16"} if sw else {}))
        r = subprocess.run([BAM2BAM, "-g", T.TOY, "-f", outp, inp], capture_output=True, text=True, env=e, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        out[sw] = gzip.decompress(open(outp, "rb").read())
        lines = SUMMARY.findall(r.stderr)
        assert len(lines) == (1 if sw else 0), r.stderr[-2000:]
        if sw:
            given, searched, served = (int(x) for x in lines[0][:3])
            assert given == searched + served and served >= len(recs) // 2 - 64 and searched <= len(recs) // 2 + 64
    # (the @PG line carries the command line, which names the output file: out_a.bam, out_b.bam)
    assert out[False].replace(b"out_a.bam", b"out_b.bam") == out[True] and len(out[True]) > 100 * len(recs)


@pytest.mark.parametrize("dedup,value", [("1", "x"), ("1", "-5"), ("1", ""), (None, "16"), ("0", "16")])
def test_a_value_the_library_would_refuse_ends_the_tools_before_the_index_is_loaded(tmp_path, dedup, value):
    """exit status 1 and a line that names the variable; the index prefix does not exist, and nothing is said about that"""
    fq = os.path.join(T.GOLDEN, "reads_se.fq")
    inp = str(tmp_path / "in.bam")
    write_bam(inp, [B.make_record("r", "ACGT" * 10, "I" * 40, 4)], True)
    e = env_with(NABWA_DEDUP_CACHE=value, **({"NABWA_DEDUP": dedup} if dedup is not None else {}))
    missing = str(tmp_path / "no_such_index")
    for cmd in ([ALN, missing, fq], [BAM2BAM, "-g", missing, "-f", str(tmp_path / "o.bam"), inp]):
        r = subprocess.run(cmd, capture_output=True, text=True, env=e, timeout=600)
        assert r.returncode == 1 and "NABWA_DEDUP_CACHE=" + value in r.stderr and "no_such" not in r.stderr, (cmd[0], r.returncode, r.stderr[-500:])
