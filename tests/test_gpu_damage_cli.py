"""`nabwa_bam2bam --damage FILE` (csrc/bam2bam_main.cpp: count_damage): the file is what the Python oracle of tests/damage_cases.py makes of the
records the tool itself writes, decoded from its output; the output BAM is the one of a run without the switch, byte for byte; with --sort
the tables are the same and the BAM is the sorted one; NABWA_DAMAGE_POS and NABWA_DAMAGE_MAPQ reach the tables; records that come back from
--temp-dir as ready-made bytes are counted like the rest."""
import os
import re

import pytest

import damage_cases as D
from test_gpu_bam_sort_cli import drop_pg, tool, toy_records

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    return D.toy_ref()


def with_damage(tmp_path, recs, args=(), env=None):
    """-> (the inflated file up to the first record, the records' bytes, the profile file's text, stderr)"""
    prof = str(tmp_path / "damage.tsv")
    if os.path.exists(prof):
        os.remove(prof)
    _, head, body, err = tool(tmp_path, recs, ["--damage", prof] + list(args), env=env)
    return head, body, open(prof).read(), err


def check(tmp_path, ref, recs, args=(), env=None, opt=None):
    opt = D.opt_of() if opt is None else opt
    _, head0, body0, err0 = tool(tmp_path, recs, list(args), env=env)
    assert "damage" not in err0
    head, body, text, err = with_damage(tmp_path, recs, args, env)
    assert body == body0 and drop_pg(head) == drop_pg(head0)          # (the @PG line carries the command line)
    want = D.oracle(ref, opt, D.split_records(body))
    assert text == D.profile_text(want)
    assert err.rstrip("\n").split("\n")[-1] == D.summary_line(want)
    return want, text, body


def test_single_reads(tmp_path, ref):
    recs = toy_records()[:200]
    want, text, _ = check(tmp_path, ref, recs, env={"NABWA_BAM_BATCH": "64"})
    assert int(want.stats[D.SEEN]) == 200 and want.stats[D.COUNTED] > 150 and want.stats[D.SK_FLAGS] > 0 and want.stats[D.COLS] > 5000
    assert text.startswith("# nabwa damage profile v1\n# seen 200\n") and len(re.findall(r"^5p\t", text, re.M)) == 26 == len(re.findall(r"^3p\t", text, re.M))
    assert "\n5p\t>25\t" in text and "\n3p\t1\t" in text and re.search(r"^len\t\d+\t\d+$", text, re.M)


def test_pairs_and_single_reads_with_and_without_sort(tmp_path, ref):
    recs = toy_records()
    want, text, body = check(tmp_path, ref, recs, env={"NABWA_BAM_BATCH": "128"})
    assert want.stats[D.COUNTED] > 250 and int(want.stats[D.SEEN]) == len(recs)
    _, text_s, body_s = check(tmp_path, ref, recs, args=["--sort"], env={"NABWA_BAM_BATCH": "128"})
    assert text_s == text and body_s != body and sorted(D.split_records(body_s)) == sorted(D.split_records(body))


def test_positions_and_mapping_quality_from_the_environment(tmp_path, ref):
    recs = toy_records()[:200]
    want, text, _ = check(tmp_path, ref, recs, env={"NABWA_DAMAGE_POS": "3", "NABWA_DAMAGE_MAPQ": "30"}, opt=D.opt_of(n_pos=3, min_mapq=30))
    assert want.stats[D.SK_MAPQ] > 0 and len(re.findall(r"^[53]p\t", text, re.M)) == 8 and "\n3p\t>3\t" in text


def test_records_that_come_back_from_the_temporary_file(tmp_path, ref):
    recs = toy_records()
    spill = tmp_path / "spill"
    spill.mkdir()
    want, text, _ = check(tmp_path, ref, recs, args=["--temp-dir", str(spill)], env={"NABWA_BAM_BATCH": "64"})
    _, _, plain, _ = with_damage(tmp_path, recs, env={"NABWA_BAM_BATCH": "64"})
    assert plain == text and os.listdir(str(spill)) == []


def test_a_file_without_records(tmp_path, ref):
    _, body, text, err = with_damage(tmp_path, [])
    empty = D.Tables(25)
    assert body == b"" and text == D.profile_text(empty) and err.rstrip("\n").split("\n")[-1] == D.summary_line(empty) and err.rstrip("\n").endswith("nan")
