"""`nabwa_bam2bam` with NABWA_BGZF=gpu-dynamic (csrc/bam2bam_main.cpp): the output's blocks come from the library's GPU compressor in
its dynamic mode.  The three writers' files inflate to the same bytes, every block of the new one passes zlib, it is smaller than the
fixed mode's file, and it ends with the end-of-file block."""
import gzip
import os

import pytest

import bamlib as B
import bgzf_cases as Z
import bgzf_dyn_cases as D
import nabwa_testlib as T
from test_gpu_bam import pe_records
from test_gpu_bam2bam_cli import write_bam
from test_gpu_bgzf_cli import check_gpu_file, tool

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", ["single", "paired"])
def test_three_writers_one_inflated_file(tmp_path, kind):
    if kind == "single":
        recs = [B.make_record(n, s, q, 4) for n, s, q in T.read_fastq(os.path.join(T.GOLDEN, "reads_se.fq"))]
    else:
        recs, _ = pe_records()
    inp = str(tmp_path / "in.bam")
    write_bam(inp, recs, "blocks")
    env = {"NABWA_BAM_BATCH": "200", "NABWA_TIMING": "1"}
    host, err_h = tool(tmp_path, inp, "host", [], dict(env, NABWA_BGZF="host"))
    gpu, err_g = tool(tmp_path, inp, "gpu", [], dict(env, NABWA_BGZF="gpu"))
    dyn, err_d = tool(tmp_path, inp, "dyn", [], dict(env, NABWA_BGZF="gpu-dynamic"))
    want = gzip.decompress(host)
    assert len(want) > len(b"".join(recs)) and gzip.decompress(gpu) == want and gzip.decompress(dyn) == want
    check_gpu_file(dyn, want)                                # ends with the end-of-file block; every block before it through zlib
    assert dyn[-28:] == Z.EOF_BLOCK
    assert len(dyn) < len(gpu)
    assert any(D.btype(b) == 2 for b in D.blocks(dyn[:-28]))
    assert "dynamic Huffman codes" in err_d and "dynamic" not in err_g and "zlib level 2 on host threads" in err_h
    print(kind, "records", len(want), "host", len(host), "gpu", len(gpu), "gpu-dynamic", len(dyn))
