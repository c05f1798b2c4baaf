"""NABWA_DEDUP=1 through the command-line tools: nabwa_aln and nabwa_bam2bam build their search batches with nabwa_batch_create, which reads the
variable; their output must not change, the stage must be seen to run, and a value the library would refuse ends them before the index is
loaded."""
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
LINE = re.compile(r"\[nabwa\] dedup: (\d+) reads given, (\d+) searched, (\d+) hash collisions, stage ([0-9.]+) ms")


def env_with(dedup, **more):
    e = {k: v for k, v in os.environ.items() if k not in ("NABWA_DEDUP", "NABWA_DEDUP_HASH_BITS", "NABWA_TIMING")}
    if dedup is not None:
        e["NABWA_DEDUP"] = dedup
    e.update(more)
    return e


@pytest.mark.parametrize("args", [[], ["-n", "0.01", "-o", "2", "-l", "1024"]], ids=["default", "adna"])
def test_aln_writes_the_same_sai_and_searches_fewer_reads(tmp_path, args):
    """reads_se.fq with every read three times under new names"""
    reads = T.read_fastq(os.path.join(T.GOLDEN, "reads_se.fq"))
    fq = str(tmp_path / "x3.fq")
    with open(fq, "w") as f:
        for rep in range(3):
            for n, s, q in reads:
                f.write("@%s_%d\n%s\n+\n%s\n" % (n, rep, s, q))
    out = {}
    for sw in (None, "1"):
        r = subprocess.run([ALN] + args + [T.TOY, fq], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env_with(sw, NABWA_TIMING="1"), timeout=600)
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
        out[sw] = r.stdout
        lines = LINE.findall(r.stderr.decode(errors="replace"))
        if sw is None:
            assert not lines
        else:
            assert lines and sum(int(x[0]) for x in lines) == 3 * len(reads)
            assert sum(int(x[1]) for x in lines) <= len(reads) and all(int(x[2]) == 0 for x in lines)
    assert len(out[None]) > 3 * len(reads) * 4 and out[None] == out["1"]


def test_bam2bam_writes_the_same_records(tmp_path):
    """the golden pairs, every pair three times under new names"""
    pairs, n_pairs = pe_records()
    fq = [T.read_fastq(os.path.join(T.GOLDEN, "reads_pe_%d.fq" % e)) for e in (1, 2)]
    recs = []
    for rep in range(3):
        for i in range(n_pairs):
            a, b = fq[0][i], fq[1][i]
            name = "%s_%d" % (a[0][:-2] if a[0].endswith("/1") else a[0], rep)
            recs += [B.make_record(name, a[1], a[2], 1 | 4 | 8 | 64), B.make_record(name, b[1], b[2], 1 | 4 | 8 | 128)]
    inp = str(tmp_path / "in.bam")
    write_bam(inp, recs, True)
    out = {}
    for sw in (None, "1"):
        outp = str(tmp_path / ("out_%s.bam" % ("b" if sw else "a")))
        r = subprocess.run([BAM2BAM, "-g", T.TOY, "-f", outp, inp], capture_output=True, text=True, env=env_with(sw, NABWA_TIMING="1"), timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        out[sw] = gzip.decompress(open(outp, "rb").read())
        lines = LINE.findall(r.stderr)
        assert bool(lines) == (sw == "1")
        if lines:
            assert sum(int(x[1]) for x in lines) < sum(int(x[0]) for x in lines)
    # (the @PG line carries the command line, which names the output file: out_a.bam, out_b.bam)
    assert out[None].replace(b"out_a.bam", b"out_b.bam") == out["1"] and len(out["1"]) > 100 * len(recs)


@pytest.mark.parametrize("var,value", [("NABWA_DEDUP", "2"), ("NABWA_DEDUP", "gpu"), ("NABWA_DEDUP_HASH_BITS", "65")])
def test_a_value_the_library_would_refuse_ends_the_tools_before_the_index_is_loaded(tmp_path, var, value):
    """exit status 1 and a line that names the variable; the index prefix does not exist, and nothing is said about that"""
    fq = os.path.join(T.GOLDEN, "reads_se.fq")
    inp = str(tmp_path / "in.bam")
    write_bam(inp, [B.make_record("r", "ACGT" * 10, "I" * 40, 4)], True)
    e = env_with("1")
    e[var] = value
    missing = str(tmp_path / "no_such_index")
    for cmd in ([ALN, missing, fq], [BAM2BAM, "-g", missing, "-f", str(tmp_path / "o.bam"), inp]):
        r = subprocess.run(cmd, capture_output=True, text=True, env=e, timeout=600)
        assert r.returncode == 1 and var + "=" + value in r.stderr and "no_such" not in r.stderr, (cmd[0], r.returncode, r.stderr[-500:])
