"""`nabwa_bam2bam` with NABWA_BGZF_IN=gpu (csrc/bam2bam_main.cpp): the input's BGZF blocks are inflated by the library's GPU decompressor
instead of zlib on host threads.  The output inflates to the same bytes, a damaged input ends the run as it does under `host`, and
the default reader is untouched: two default runs write the same bytes."""
import gzip
import importlib
import os
import subprocess

import pytest

import bamlib as B
import nabwa_testlib as T
from test_bgzf_in import bgzf
from test_gpu_bam import pe_records
from test_gpu_bam2bam_cli import write_bam

nabwa = importlib.import_module("network-aware-bwa_amd")
pytestmark = pytest.mark.gpu
EXE = os.path.join(os.path.dirname(nabwa.LIB_PATH), "nabwa_bam2bam")


def tool(tmp_path, inp, name, env, ok=True):
    """one run in a folder of its own, with the same relative names every time: the @PG line carries the command line"""
    d = tmp_path / name
    d.mkdir()
    r = subprocess.run([EXE, "-g", T.TOY, "-f", "out.bam", os.path.relpath(inp, d)], capture_output=True, text=True, env=dict(os.environ, **env), timeout=600, cwd=d)
    if not ok:
        return r
    assert r.returncode == 0, r.stderr[-2000:]
    return open(d / "out.bam", "rb").read(), r.stderr


def records(kind):
    if kind == "single":
        return [B.make_record(n, s, q, 4) for n, s, q in T.read_fastq(os.path.join(T.GOLDEN, "reads_se.fq"))]
    return pe_records()[0]


@pytest.mark.parametrize("kind", ["single", "paired"])
def test_same_output_as_the_host_reader(tmp_path, kind):
    inp = str(tmp_path / "in.bam")
    write_bam(inp, records(kind), "blocks")
    env = {"NABWA_BAM_BATCH": "200", "NABWA_TIMING": "1"}
    host, err_h = tool(tmp_path, inp, "host", env)
    host2, _ = tool(tmp_path, inp, "host2", dict(env, NABWA_BGZF_IN="host"))
    gpu, err_g = tool(tmp_path, inp, "gpu", dict(env, NABWA_BGZF_IN="gpu"))
    assert host == host2                                     # the default path: the same bytes from run to run, named or not
    assert len(gzip.decompress(host)) > 1000 and gzip.decompress(gpu) == gzip.decompress(host)
    assert "BGZF blocks on the GPU" in err_g and "BGZF blocks in parallel" in err_h


def test_small_blocks_many_members_in_one_fill(tmp_path):
    """the same file cut into blocks of 1000 bytes: more members than lanes of a wave in the reader's one fill"""
    plain = str(tmp_path / "plain.bam")
    write_bam(plain, records("single"), "plain")
    raw = open(plain, "rb").read()
    inp = str(tmp_path / "in.bam")
    open(inp, "wb").write(bgzf(raw, 1000))
    assert len(raw) > 64 * 1000
    env = {"NABWA_BAM_BATCH": "200"}
    host, _ = tool(tmp_path, inp, "host", env)
    gpu, _ = tool(tmp_path, inp, "gpu", dict(env, NABWA_BGZF_IN="gpu"))
    assert gzip.decompress(gpu) == gzip.decompress(host)


def test_gzip_and_plain_input_stay_on_the_host(tmp_path):
    recs = records("single")
    outs = []
    for form in ("blocks", "plain", False):
        d = tmp_path / str(form)                             # the same relative names in every run: the @PG line carries the command line
        d.mkdir()
        inp = str(d / "in.bam")
        write_bam(inp, recs, form)
        out, err = tool(d, inp, "run", {"NABWA_BAM_BATCH": "200", "NABWA_TIMING": "1", "NABWA_BGZF_IN": "gpu"})
        assert ("BGZF blocks on the GPU" in err) == (form == "blocks")
        outs.append(gzip.decompress(out))
    assert outs[0] == outs[1] == outs[2]


def test_an_unknown_reader_exits_1(tmp_path):
    inp = str(tmp_path / "in.bam")
    write_bam(inp, records("single")[:10], "blocks")
    r = tool(tmp_path, inp, "zlib", {"NABWA_BGZF_IN": "zlib"}, ok=False)
    assert r.returncode == 1 and "NABWA_BGZF_IN" in r.stderr


def test_a_damaged_file_ends_the_run_under_both(tmp_path):
    good = str(tmp_path / "good.bam")
    write_bam(good, records("single"), "blocks")
    data = open(good, "rb").read()
    inp = str(tmp_path / "in.bam")
    open(inp, "wb").write(data[:5000] + bytes([data[5000] ^ 0x41]) + data[5001:])
    runs = {v: tool(tmp_path, inp, v, {"NABWA_BGZF_IN": v}, ok=False) for v in ("host", "gpu")}
    for v, r in runs.items():
        assert r.returncode != 0 and "a BGZF block does not inflate to what its trailer says" in r.stderr, (v, r.stderr[-1000:])
    assert runs["host"].returncode == runs["gpu"].returncode
    assert "member 0 " in runs["gpu"].stderr
