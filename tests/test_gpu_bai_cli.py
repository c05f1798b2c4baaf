"""`nabwa_bam2bam --sort --index` (csrc/bam2bam_main.cpp: index_records, BgzfOut::note): out.bam.bai is byte for byte what the Python oracle of
tests/bai_cases.py makes of the records of the inflated out.bam and of the file's own BGZF blocks (nabwa.bgzf_block_table); regions read
through it give what a scan gives; the tool ends with the line that counts records, chunks and bins -- alone, behind the duplicate marker
(flagged and removed), with --damage, under either BGZF writer, and with several sorted runs.  The switch changes nothing else: the
inflated file is that of the run without it but for the switch itself in the @PG line's command (so the deflated bytes are not compared:
the header is eight bytes longer)."""
import importlib
import os
import struct

import pytest

import bai_cases as M
from test_gpu_bam_sort_cli import big_records, tool, toy_records

nabwa = importlib.import_module("network-aware-bwa_amd")
pytestmark = pytest.mark.gpu


def indexed(tmp_path, recs, args, env=None):
    """a run with --index behind the other switches -> (the file, the inflated header, the records' bytes, stderr, the .bai)"""
    bai = str(tmp_path / "out.bam.bai")
    if os.path.exists(bai):
        os.remove(bai)
    _, head, body, err = tool(tmp_path, recs, args + ["--index"], env=env)
    assert sorted(os.listdir(str(tmp_path))) == ["in.bam", "out.bam", "out.bam.bai"] or "--damage" in args
    return open(str(tmp_path / "out.bam"), "rb").read(), head, body, err, open(bai, "rb").read()


def check(tmp_path, recs, args, env=None, regions=lambda records: ()):
    """the index of a run against the oracle, its last line, region queries through it, and the run without the switch -> (stats, the
    parsed index, the records, stderr, the file)"""
    data, head, body, err, bai = indexed(tmp_path, recs, args, env)
    n_ref = struct.unpack_from("<i", head, 8 + struct.unpack_from("<i", head, 4)[0])[0]
    records = M.split_records(body)
    u, c = nabwa.bgzf_block_table(data)
    assert int(u[-1]) == len(head) + len(body) and int(c[-1]) == len(data) - 28
    want, stats = M.oracle([(records, len(head))], n_ref, u, c)
    assert bai == want, "another index\ngot\n%s\nexpected\n%s" % (M.describe(bai), M.describe(want))
    assert err.rstrip("\n").split("\n")[-1] == "[nabwa_bam2bam] indexed %d records, %d chunks in %d bins on the gpu" % (len(records), int(stats[M.CHUNKS]), int(stats[M.BINS]))
    parsed = M.parse_bai(bai)
    ext = [M.extent(r) for r in records]
    for t, beg, end in regions(records):
        f = M.Bgzf(data)
        assert M.query(parsed, f, t, beg, end) == [r for r, e in zip(records, ext) if e[0] == t and e[1] < end and e[2] > beg], (t, beg, end)
    # without the switch: the same inflated bytes but for " --index" in the @PG line's command and the header's length word
    os.remove(str(tmp_path / "out.bam.bai"))
    _, head0, body0, err0 = tool(tmp_path, recs, args, env=env)
    assert not os.path.exists(str(tmp_path / "out.bam.bai")) and "] indexed " not in err0
    assert body0 == body and head.count(b" --index") == 1
    assert head0[8:] == head[8:].replace(b" --index", b"") and struct.unpack_from("<i", head0, 4)[0] == struct.unpack_from("<i", head, 4)[0] - len(" --index")
    assert [l for l in err0.split("\n") if "timing" not in l and "renaming" not in l] == [l for l in err.split("\n") if "timing" not in l and "renaming" not in l][:-2] + [""]
    return stats, parsed, records, err, data


def toy_regions(records):
    """every reference whole, and narrow regions at and beside the placed records' ends"""
    ext = [M.extent(r) for r in records if M.extent(r)[0] >= 0]
    refs = sorted({e[0] for e in ext})
    out = [(t, 0, 1 << 29) for t in refs]
    for t, beg, end in ext[::max(1, len(ext) // 25)]:
        out += [(t, beg, beg + 1), (t, end - 1, end), (t, end, end + 1), (t, max(0, beg - 50), beg)]
    return out


def test_toy_records_indexed(tmp_path):
    recs = toy_records()
    env = {"NABWA_BAM_BATCH": "128"}
    stats, parsed, records, _, _ = check(tmp_path, recs, ["--sort"], env, toy_regions)
    assert int(stats[M.RECORDS]) == len(recs) and stats[M.NO_COOR] > 0 and stats[M.PLACED] > 100 and stats[M.BINS] >= 1
    assert len(toy_regions(records)) > 50


@pytest.mark.parametrize("env", [{"NABWA_BGZF": "host"}, {"NABWA_BGZF": "gpu"}, {"NABWA_SORT_RUN_MIB": "1"}, {"NABWA_SORT": "host", "NABWA_SORT_RUN_MIB": "1", "NABWA_BAM_BATCH": "1500"}],
                         ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_big_input_under_either_writer_and_in_several_runs(tmp_path, env):
    recs = big_records()
    stats, parsed, records, err, data = check(tmp_path, recs, ["--sort"], env, toy_regions)
    if "NABWA_SORT_RUN_MIB" in env:
        assert int(err.split("] sorted ")[1].split(" run(s)")[0].split(" in ")[1]) >= 3
    assert len(nabwa.bgzf_block_table(data)[0]) > 40 and stats[M.PLACED] > 10000                  # more than 3 MiB of records: many blocks


def test_behind_the_duplicate_marker(tmp_path):
    recs = toy_records()
    env = {"NABWA_BAM_BATCH": "100"}
    marked = check(tmp_path, recs, ["--sort", "--mark-duplicates"], env, toy_regions)[0]
    removed = check(tmp_path, recs, ["--sort", "--remove-duplicates"], env, toy_regions)[0]
    assert int(marked[M.RECORDS]) == len(recs) > int(removed[M.RECORDS]) > 0                     # the index sees the records that are written


@pytest.mark.parametrize("dups", [[], ["--mark-duplicates"]], ids=["alone", "behind the marker"])
def test_with_the_damage_profile(tmp_path, dups):
    prof = str(tmp_path / "damage.tsv")
    check(tmp_path, toy_records(), ["--sort"] + dups + ["--damage", prof], {"NABWA_BAM_BATCH": "100"})
    assert os.path.getsize(prof) > 0


def test_a_file_without_records(tmp_path):
    stats, parsed = check(tmp_path, [], ["--sort"])[:2]
    assert not stats[:M.BYTES].any() and all(not b and not l for b, l in parsed[0]) and parsed[1] == 0


def test_misuse_leaves_no_file(tmp_path):
    recs = toy_records()[:20]
    _, _, _, err = tool(tmp_path, recs, ["--index"], rc=1)
    assert "--index needs --sort" in err
    _, _, _, err = tool(tmp_path, recs, ["--sort", "--index"], env={"NABWA_DEVICES": str(1 << 20), "NABWA_SORT": "host"}, rc=2)
    assert "--index on the GPU" in err
    assert sorted(os.listdir(str(tmp_path))) == ["in.bam"]
