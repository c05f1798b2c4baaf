"""`nabwa_bam2bam --sort --mark-duplicates | --remove-duplicates` (csrc/bam2bam_main.cpp: mark_duplicates, sort_runs): the output is the stable
coordinate sort of what the tool writes without --sort, with flag 0x400 set on exactly the records the Python oracle of tests/markdup_cases.py
marks in that unsorted stream (or with exactly those records left out) -- for one run and several, batches of any size, --temp-dir and
NABWA_SORT=host; the summary line carries the oracle's counts; --damage behind the marker leaves the duplicates out."""
import os
import struct

import numpy as np
import pytest

import bam_sort_cases as S
import bamlib as B
import damage_cases as D
import markdup_cases as M
import nabwa_testlib as T
from test_gpu_bam_sort_cli import assert_sorted_of, big_records, tool, toy_records

pytestmark = pytest.mark.gpu
MARK, REMOVE = ["--sort", "--mark-duplicates"], ["--sort", "--remove-duplicates"]


def summary_line(stats, word="marked"):
    return "[nabwa_bam2bam] %s %d of %d records as duplicates (%d pairs, %d single reads) on the gpu" % (
        word, int(stats[M.DUP_RECORDS]), int(stats[M.SEEN]), int(stats[M.DUP_PAIRS]), int(stats[M.DUP_FRAGMENTS]))


def last_line(err):
    return err.rstrip("\n").split("\n")[-1]


def expected(unsorted, opt=None, remove=False):
    """what the tool must write for the unsorted stream it writes without --sort -> (the records' bytes, dup, stats)"""
    recs = M.split_records(unsorted)
    dup, stats = M.oracle([recs], M.opt_of() if opt is None else opt)
    stream = b"".join(r for r, d in zip(recs, dup) if not d) if remove else M.set_flags(unsorted, dup)
    want, _, _ = S.oracle(np.frombuffer(stream, np.uint8), S.offsets_of(stream))
    return bytes(want), dup, stats


def clear_dup_flag(body):
    a = np.frombuffer(body, np.uint8).copy()
    a[S.offsets_of(body)[:-1] + 19] &= 0xfb
    return a.tobytes()


@pytest.fixture(scope="module")
def big(tmp_path_factory):
    """the big input (32 renamed copies of the same reads: nearly everything is a duplicate and all scores tie), what the tool writes for it
    without --sort, and what it must write with the switch"""
    tmp = tmp_path_factory.mktemp("markdup_big")
    recs = big_records()
    _, _, unsorted, _ = tool(tmp, recs, [])
    want, dup, stats = expected(unsorted)
    assert stats[M.DUP_FRAGMENTS] > 10000 and stats[M.DUP_PAIRS] == 0 and stats[M.PAIRS] > 50 and stats[M.UNMAPPED] > 1000 and 0 < dup.sum() < len(dup) - 1000
    return recs, unsorted, want, stats


def test_toy_records_marked(tmp_path):
    recs = toy_records()
    env = {"NABWA_BAM_BATCH": "128"}
    _, _, unsorted, _ = tool(tmp_path, recs, [], env=env)
    _, head_s, sorted_body, err_s = tool(tmp_path, recs, ["--sort"], env=env)
    assert "duplicates" not in err_s
    text, head, body, err = tool(tmp_path, recs, MARK, env=dict(env, NABWA_TIMING="1"))
    want, dup, stats = expected(unsorted)
    assert text.split("\n")[0] == "@HD\tVN:1.4\tSO:coordinate"
    assert len(body) == len(sorted_body) and clear_dup_flag(body) == sorted_body and S.offsets_of(body).tolist() == S.offsets_of(sorted_body).tolist()      # the order of --sort; only bit 0x400 differs
    assert body == want
    assert last_line(err) == summary_line(stats) and "timing: duplicates thread" in err
    assert err.index("] sorted ") < err.index("] marked ")
    assert int(stats[M.SEEN]) == len(recs) and stats[M.PAIRS] > 50 and stats[M.FRAGMENTS] > 100


def test_big_input_in_one_run(tmp_path, big):
    recs, unsorted, want, stats = big
    _, _, body, err = tool(tmp_path, recs, MARK)
    assert body == want and last_line(err) == summary_line(stats)
    assert_sorted_of(clear_dup_flag(body), unsorted)


@pytest.mark.parametrize("env", [{"NABWA_SORT_RUN_MIB": "1"}, {"NABWA_BAM_BATCH": "64"}, {"NABWA_BAM_BATCH": "2000", "NABWA_SORT_RUN_MIB": "1"}, {"NABWA_SORT": "host"},
                                 {"NABWA_SORT": "host", "NABWA_SORT_RUN_MIB": "1", "NABWA_BAM_BATCH": "1500"}], ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_runs_batches_and_the_host_sort_give_the_same_marks(tmp_path, big, env):
    recs, unsorted, want, stats = big
    _, _, body, err = tool(tmp_path, recs, MARK, env=env)
    assert body == want and last_line(err) == summary_line(stats)
    if "NABWA_SORT_RUN_MIB" in env:
        assert int(err.split("] sorted ")[1].split(" run(s)")[0].split(" in ")[1]) >= 3


def test_with_temp_dir(tmp_path, big):
    recs, _, want, stats = big
    spill = tmp_path / "spill"
    spill.mkdir()
    _, _, body, err = tool(tmp_path, recs, MARK + ["--temp-dir", str(spill)], env={"NABWA_BAM_BATCH": "2000", "NABWA_SORT_RUN_MIB": "1"})
    assert body == want and last_line(err) == summary_line(stats) and os.listdir(str(spill)) == []


def test_remove_duplicates_gives_the_unmarked_records(tmp_path, big):
    recs, unsorted, want, stats = big
    want_removed, dup, _ = expected(unsorted, remove=True)
    for env in ({}, {"NABWA_SORT_RUN_MIB": "1"}):
        _, _, body, err = tool(tmp_path, recs, REMOVE, env=env)
        assert body == want_removed and last_line(err) == summary_line(stats, "removed")
    kept = [r for r in M.split_records(want) if not struct.unpack_from("<H", r, 18)[0] & 0x400]
    assert b"".join(kept) == want_removed and len(kept) == len(dup) - int(dup.sum())


def test_damage_behind_the_marker_leaves_the_duplicates_out(tmp_path):
    ref = D.toy_ref()
    recs = toy_records()[:200] + [B.make_record("copy_" + n, s, q, 4) for n, s, q in T.read_fastq(os.path.join(T.GOLDEN, "reads_se.fq"))[:80]] + toy_records()[200:]
    prof = str(tmp_path / "damage.tsv")
    env = {"NABWA_BAM_BATCH": "100"}
    _, _, plain, err_plain = tool(tmp_path, recs, ["--sort", "--damage", prof], env=env)
    text_plain = open(prof).read()
    os.remove(prof)
    _, _, body, err = tool(tmp_path, recs, MARK + ["--damage", prof], env=env)
    text = open(prof).read()
    assert clear_dup_flag(body) == plain and last_line(err).startswith("[nabwa_bam2bam] marked ")
    all_recs, marked = D.split_records(plain), D.split_records(body)
    t_all, t_marked = D.oracle(ref, D.opt_of(), all_recs), D.oracle(ref, D.opt_of(), marked)
    assert text_plain == D.profile_text(t_all) and text == D.profile_text(t_marked) and text != text_plain
    assert D.summary_line(t_marked) + "\n" in err and D.summary_line(t_all) + "\n" in err_plain
    # the difference is the duplicates' columns: what the records that got the flag count for on their own
    dups = [a for a, b in zip(all_recs, marked) if a != b]
    t_dups = D.oracle(ref, D.opt_of(), dups)
    assert len(dups) > 50 and t_dups.stats[D.COUNTED] > 50
    for name, a, b, c in zip(("sub5", "sub3", "len_hist"), t_all.parts(), t_marked.parts(), t_dups.parts()):
        assert np.array_equal(a - b, c), name
    assert int(t_marked.stats[D.SK_FLAGS]) == int(t_all.stats[D.SK_FLAGS]) + int(t_dups.stats[D.SEEN]) - int(t_dups.stats[D.SK_FLAGS])      # (a half pair's unmapped mate was skipped before)
    # with --remove-duplicates they are gone before the damage stage sees them
    os.remove(prof)
    _, _, removed, _ = tool(tmp_path, recs, REMOVE + ["--damage", prof], env=env)
    t_removed = D.oracle(ref, D.opt_of(), D.split_records(removed))
    assert open(prof).read() == D.profile_text(t_removed)
    D.assert_same(Dparts(t_removed), Dparts(t_marked), "removed against marked")


def Dparts(t):
    """the tables without the counters of the records that were skipped"""
    u = D.Tables(t.n_pos)
    u.sub5[:], u.sub3[:], u.len_hist[:] = t.sub5, t.sub3, t.len_hist
    u.stats[D.COUNTED], u.stats[D.COLS] = t.stats[D.COUNTED], t.stats[D.COLS]
    return u


def test_both_ends_from_the_environment(tmp_path):
    """reads and copies of them cut short at their 3' end: one 5' end, two lengths"""
    reads = T.read_fastq(os.path.join(T.GOLDEN, "reads_se.fq"))[:150]
    recs = [B.make_record(n, s, q, 4) for n, s, q in reads] + [B.make_record("cut_" + n, s[:-6], q[:-6], 4) for n, s, q in reads]
    _, _, unsorted, _ = tool(tmp_path, recs, [])
    want5, dup5, stats5 = expected(unsorted)
    want_both, dup_both, stats_both = expected(unsorted, M.opt_of(single_ends=M.ENDS_BOTH, min_qual=20))
    assert dup5.sum() > 50 and dup_both.sum() < dup5.sum() and want5 != want_both
    _, _, body, err = tool(tmp_path, recs, MARK, env={"NABWA_MARKDUP_ENDS": "5p"})
    assert body == want5 and last_line(err) == summary_line(stats5)
    _, _, body, err = tool(tmp_path, recs, MARK, env={"NABWA_MARKDUP_ENDS": "both", "NABWA_MARKDUP_QUAL": "20"})
    assert body == want_both and last_line(err) == summary_line(stats_both)


def test_a_file_without_records(tmp_path):
    for args, word in ((MARK, "marked"), (REMOVE, "removed")):
        text, _, body, err = tool(tmp_path, [], args)
        assert body == b"" and text.split("\n")[0] == "@HD\tVN:1.4\tSO:coordinate"
        assert last_line(err) == summary_line(np.zeros(M.N_STATS, np.uint64), word)
