"""`nabwa_bam2bam --sort` (csrc/bam2bam_main.cpp: sort_runs): the output is the stable coordinate sort of what the tool writes without
--sort -- np.argsort(keys, kind="stable") over the records of the unsorted file, compared record for record as bytes -- for one run and
for several (NABWA_SORT_RUN_MIB), with --temp-dir, --only-aligned and batches that do not line up with the runs, sorted on the GPU and
(NABWA_SORT=host) on host threads; @HD says SO:coordinate then and only then."""
import gzip
import importlib
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import bam_sort_cases as S
import bamlib as B
import nabwa_testlib as T
from test_gpu_bam import pe_records
from test_gpu_bam2bam_cli import EXE, read_bam, run, write_bam

nabwa = importlib.import_module("network-aware-bwa_amd")
pytestmark = pytest.mark.gpu
SORT_VARS = ("NABWA_SORT", "NABWA_SORT_RUN_MIB")


def tool(tmp_path, records, args, env=None, rc=0):
    """-> (header text, the inflated file up to the first record, the records' bytes, stderr); the file names are the same in every run,
    so runs with the same options write the same @PG line"""
    if not os.path.exists(EXE):
        nabwa.build()
    inp, outp = str(tmp_path / "in.bam"), str(tmp_path / "out.bam")
    if os.path.exists(outp):
        os.remove(outp)
    write_bam(inp, records, "blocks")
    e = {k: v for k, v in os.environ.items() if k not in SORT_VARS}
    e.update(env or {})
    r = subprocess.run([EXE, "-g", T.TOY, "-f", outp + "_"] + args + [inp], capture_output=True, text=True, env=e, timeout=600)
    assert r.returncode == rc, r.stderr[-2000:]
    if rc:
        assert not os.path.exists(outp)
        return None, None, None, r.stderr
    raw = gzip.decompress(open(outp, "rb").read())
    l_text = struct.unpack_from("<i", raw, 4)[0]
    p = 8 + l_text
    n_ref = struct.unpack_from("<i", raw, p)[0]; p += 4
    for _ in range(n_ref):
        p += 4 + struct.unpack_from("<i", raw, p)[0] + 4
    return raw[8:8 + l_text].decode(), raw[:p], raw[p:], r.stderr


def summary(err):
    m = re.search(r"^\[nabwa_bam2bam\] sorted (\d+) records in (\d+) run\(s\) on the (gpu|host)$", err, re.M)
    assert m, err[-1500:]
    assert err.rstrip("\n").split("\n")[-1] == m.group(0)              # the line the tool ends with
    return int(m.group(1)), int(m.group(2)), m.group(3)


def assert_sorted_of(body, unsorted, what=""):
    off = S.offsets_of(unsorted)
    want, want_off, want_keys = S.oracle(np.frombuffer(unsorted, np.uint8), off)
    S.assert_same_records(body, S.offsets_of(body), want, want_off, what)
    return want_keys


def drop_pg(head):
    """the inflated file up to the first record without its length word and without the @PG line this run added"""
    return re.sub(rb"@PG\tID:bwa-1[^\n]*\n", b"", head[8:], count=1)


def flags_of(body):
    off = S.offsets_of(body)
    return [struct.unpack_from("<H", body, int(o) + 18)[0] for o in off[:-1]]


def toy_records():
    reads = T.read_fastq(os.path.join(T.GOLDEN, "reads_se.fq"))
    singles = [B.make_record(n, s, q, 4) for n, s, q in reads]
    pairs, _ = pe_records()
    return singles[:200] + pairs + singles[200:260]


def big_records():
    """about 20 000 reads: more than 3 MiB of finished records, pairs in the middle"""
    reads = T.read_fastq(os.path.join(T.GOLDEN, "reads_se.fq"))
    pairs, _ = pe_records()
    recs = []
    for k in range(32):
        recs += [B.make_record("%s_%d" % (n, k), s, q, 4) for n, s, q in reads]
        if k == 10:
            recs += pairs
    return recs


def test_toy_index_pairs_singletons_unmapped_and_both_strands(tmp_path):
    recs = toy_records()
    text_u, head_u, unsorted, err_u = tool(tmp_path, recs, [], env={"NABWA_BAM_BATCH": "128", "NABWA_SORT": "fast"})      # without --sort the variable is not read
    assert text_u.split("\n")[0] == "@HD\tVN:1.4" and "SO:" not in text_u.split("\n")[0] and "sorted" not in err_u
    _, _, plain, _ = tool(tmp_path, recs, [], env={"NABWA_BAM_BATCH": "128"})
    assert plain == unsorted
    fl = flags_of(unsorted)
    assert any(f & 1 for f in fl) and any(not f & 1 for f in fl) and any(f & 4 for f in fl) and any(f & 16 for f in fl) and any(not f & 20 for f in fl)
    text, head, body, err = tool(tmp_path, recs, ["--sort"], env={"NABWA_BAM_BATCH": "128"})
    lines, lines_u = text.split("\n"), text_u.split("\n")
    assert lines[0] == "@HD\tVN:1.4\tSO:coordinate"
    assert lines[1] == lines_u[1].replace("out.bam_ ", "out.bam_ --sort ") and lines[1] != lines_u[1] and lines[2:] == lines_u[2:]
    keys = assert_sorted_of(body, unsorted)
    assert summary(err) == (len(keys), 1, "gpu")
    assert len({int(k) for k in keys}) > 50 and int(keys[-1]) >> 32 == 0xffffffff          # many places, and the unmapped at the end
    # the same through the helpers of tests/test_gpu_bam2bam_cli.py: the decoded records are in coordinate order, every read is there
    _, refs, out = run(tmp_path, recs, ["--sort"], env={"NABWA_BAM_BATCH": "128"}, bgzf="blocks")
    names = [r[0] for r in refs]
    place = [(names.index(o["rname"]) if o["rname"] != "*" else 1 << 31, o["pos"]) for o in out]
    assert place == sorted(place) and len(out) == len(recs)


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    """the big input, what the tool writes for it without --sort, and the one-run sorted file"""
    tmp = tmp_path_factory.mktemp("bam_sort_big")
    recs = big_records()
    _, _, unsorted, _ = tool(tmp, recs, [])
    assert len(unsorted) > (3 << 20) + (1 << 19)
    _, head, body, err = tool(tmp, recs, ["--sort"])
    assert summary(err)[1:] == (1, "gpu")
    assert_sorted_of(body, unsorted)
    return recs, unsorted, head, body


def test_several_runs_give_the_bytes_of_one_run(tmp_path, big):
    recs, unsorted, head1, body1 = big
    _, head, body, err = tool(tmp_path, recs, ["--sort"], env={"NABWA_SORT_RUN_MIB": "1", "NABWA_TIMING": "1"})
    n, runs, where = summary(err)
    assert runs >= 3 and where == "gpu" and n == len(S.offsets_of(unsorted)) - 1
    assert "timing: sort thread" in err
    assert body == body1


def test_several_runs_with_temp_dir(tmp_path, big):
    """--temp-dir: the batches wait in one file and the sorted runs in another; batches of single reads come back from the first as ready-made bytes"""
    recs = big[0]
    spill = tmp_path / "spill"
    spill.mkdir()
    env = {"NABWA_BAM_BATCH": "2000"}
    _, _, unsorted, _ = tool(tmp_path, recs, ["--temp-dir", str(spill)], env=env)
    _, _, body, err = tool(tmp_path, recs, ["--sort", "--temp-dir", str(spill)], env=dict(env, NABWA_SORT_RUN_MIB="1"))
    assert summary(err)[1] >= 3
    assert_sorted_of(body, unsorted)
    assert body == big[3]                                  # and the one-run file's bytes
    _, _, one, err = tool(tmp_path, recs, ["--sort", "--temp-dir", str(spill)], env=env)
    assert summary(err)[1] == 1 and one == body
    assert os.listdir(str(spill)) == []


def test_several_runs_with_only_aligned(tmp_path, big):
    recs = big[0]
    _, _, unsorted, _ = tool(tmp_path, recs, ["--only-aligned"])
    assert (3 << 20) < len(unsorted) < len(big[1])
    _, _, one, err1 = tool(tmp_path, recs, ["--sort", "--only-aligned"])
    _, _, body, err = tool(tmp_path, recs, ["--sort", "--only-aligned"], env={"NABWA_SORT_RUN_MIB": "1"})
    assert summary(err1)[1] == 1 and summary(err)[1] >= 3 and summary(err)[0] == len(S.offsets_of(unsorted)) - 1
    assert_sorted_of(body, unsorted)
    assert body == one
    assert not any(f & 4 for f in flags_of(body))


def test_runs_and_batches_that_do_not_line_up(tmp_path, big):
    recs, _, _, body1 = big
    _, _, unsorted, _ = tool(tmp_path, recs, [], env={"NABWA_BAM_BATCH": "777"})
    _, _, body, err = tool(tmp_path, recs, ["--sort"], env={"NABWA_BAM_BATCH": "777", "NABWA_SORT_RUN_MIB": "1"})
    assert summary(err)[1] >= 3
    assert_sorted_of(body, unsorted)
    assert body == body1


def test_host_sort_gives_the_same_bytes(tmp_path, big):
    recs, _, head1, body1 = big
    _, head, body, err = tool(tmp_path, recs, ["--sort"], env={"NABWA_SORT": "host"})
    assert summary(err)[1:] == (1, "host") and body == body1
    assert drop_pg(head) == drop_pg(head1)                 # (the @PG line names the files, which lie elsewhere)
    _, _, body, err = tool(tmp_path, recs, ["--sort"], env={"NABWA_SORT": "host", "NABWA_SORT_RUN_MIB": "1", "NABWA_BAM_BATCH": "1500"})
    assert summary(err)[1] >= 3 and summary(err)[2] == "host" and body == body1


def test_values_the_tool_refuses(tmp_path):
    recs = toy_records()[:20]
    for env, word in (({"NABWA_SORT": "fast"}, "NABWA_SORT=fast"), ({"NABWA_SORT_RUN_MIB": "0"}, "NABWA_SORT_RUN_MIB=0"), ({"NABWA_SORT_RUN_MIB": "12x"}, "NABWA_SORT_RUN_MIB=12x"),
                      ({"NABWA_SORT_RUN_MIB": "-3"}, "NABWA_SORT_RUN_MIB=-3"), ({"NABWA_SORT_RUN_MIB": ""}, "NABWA_SORT_RUN_MIB=")):
        _, _, _, err = tool(tmp_path, recs, ["--sort"], env=env, rc=1)
        assert word in err and "genome length" not in err, err            # said before the index is loaded


def test_a_file_without_records(tmp_path):
    text, head, body, err = tool(tmp_path, [], ["--sort"])
    assert body == b"" and text.split("\n")[0] == "@HD\tVN:1.4\tSO:coordinate"
    assert summary(err) == (0, 0, "gpu")


def test_gpu_bgzf_writer_takes_the_sorted_bytes(tmp_path, big):
    recs, _, head1, body1 = big
    _, head, body, err = tool(tmp_path, recs, ["--sort"], env={"NABWA_BGZF": "gpu", "NABWA_SORT_RUN_MIB": "2"})
    assert summary(err)[1] >= 2 and drop_pg(head) == drop_pg(head1) and body == body1
