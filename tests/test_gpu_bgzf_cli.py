"""`nabwa_bam2bam` with NABWA_BGZF=gpu (csrc/bam2bam_main.cpp): the output's blocks come from the library's GPU compressor instead of
zlib on host threads.  The inflated file is the same byte for byte, the blocks are well-formed BGZF followed by the end-of-file block,
and the default writer is untouched: its compressed bytes repeat from run to run."""
import gzip
import importlib
import os
import subprocess

import pytest

import bamlib as B
import bgzf_cases as Z
import nabwa_testlib as T
from test_gpu_bam import pe_records
from test_gpu_bam2bam_cli import write_bam

nabwa = importlib.import_module("network-aware-bwa_amd")
pytestmark = pytest.mark.gpu
EXE = os.path.join(os.path.dirname(nabwa.LIB_PATH), "nabwa_bam2bam")


def tool(tmp_path, inp, name, args, env):
    """one run in a folder of its own, with the same relative names every time: the @PG line carries the command line"""
    d = tmp_path / name
    d.mkdir()
    r = subprocess.run([EXE, "-g", T.TOY, "-f", "out.bam"] + args + [os.path.relpath(inp, d)], capture_output=True, text=True, env=dict(os.environ, **env),
                       timeout=600, cwd=d)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(d / "out.bam", "rb").read(), r.stderr


def check_gpu_file(raw, inflated):
    assert raw[-28:] == Z.EOF_BLOCK
    Z.walk(raw[:-28], inflated)


@pytest.mark.parametrize("kind", ["single", "paired"])
def test_same_inflated_bytes_as_the_host_writer(tmp_path, kind):
    if kind == "single":
        recs = [B.make_record(n, s, q, 4) for n, s, q in T.read_fastq(os.path.join(T.GOLDEN, "reads_se.fq"))]
    else:
        recs, _ = pe_records()
    inp = str(tmp_path / "in.bam")
    write_bam(inp, recs, "blocks")
    env = {"NABWA_BAM_BATCH": "200", "NABWA_TIMING": "1"}
    host, err_h = tool(tmp_path, inp, "host", [], env)
    host2, _ = tool(tmp_path, inp, "host2", [], dict(env, NABWA_BGZF="host"))
    gpu, err_g = tool(tmp_path, inp, "gpu", [], dict(env, NABWA_BGZF="gpu"))
    assert host == host2                                     # the default path: the same compressed bytes, named or not
    want = gzip.decompress(host)
    assert len(want) > len(b"".join(recs)) and gzip.decompress(gpu) == want
    check_gpu_file(gpu, want)
    assert "BGZF on the GPU" in err_g and "zlib level 2 on host threads" in err_h


def test_partial_flushes_and_the_final_one(tmp_path):
    """more than 64 MB of records: the writer hands over whole blocks while the run goes on, keeps the rest, and the final flush
    brings the last, shorter block; --only-aligned, batches of 50 000 records"""
    reads = T.read_fastq(os.path.join(T.GOLDEN, "reads_se.fq"))
    recs = [B.make_record(n, s, q, 4) for n, s, q in reads] * 560
    inp = str(tmp_path / "in.bam")
    write_bam(inp, recs, "plain")
    env = {"NABWA_BAM_BATCH": "50000"}
    host, _ = tool(tmp_path, inp, "host", ["--only-aligned"], env)
    gpu, _ = tool(tmp_path, inp, "gpu", ["--only-aligned"], dict(env, NABWA_BGZF="gpu"))
    want = gzip.decompress(host)
    assert len(want) > (64 << 20) + 0xff00, "the input no longer fills one flush: %d bytes" % len(want)
    assert len(want) % 0xff00 != 0
    check_gpu_file(gpu, want)
    print("records %d bytes: host writer %d, gpu writer %d" % (len(want), len(host), len(gpu)))
