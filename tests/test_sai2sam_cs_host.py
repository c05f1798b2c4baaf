"""Colour space in nabwa_samse / nabwa_sampe, the parts that need no GPU: what is refused before a GPU is looked for (exit 1, nothing
written), what a valid colour input does without a GPU (exit 2, nothing written), and pairing()'s BWA_PET_SOLID sweep (reference
bwape.c:234-247) against the reference's own answers (tests/golden/make_golden_cs.py)."""
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest

import nabwa_testlib as T

nabwa = importlib.import_module("network-aware-bwa_amd")
TOOLS = {"samse": nabwa.SAMSE_PATH, "sampe": nabwa.SAMPE_PATH}
G = lambda x: os.path.join(T.GOLDEN, x)


def run_tool(name, args):
    env = dict(os.environ, NABWA_DEVICE="99")                    # no such GPU: what exits 1 must do so before looking for one
    if not os.path.exists(TOOLS[name]):
        pytest.fail("%s was not built" % TOOLS[name])
    return subprocess.run([TOOLS[name]] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=60)


@pytest.fixture(scope="module")
def colour_prefix(tmp_path_factory):
    """the host half of `nabwa_index -c` on the toy genome (.pac, .ann, .amb, .nt.*) with stand-ins for the FM-index files, which are
    only looked at, not read, before the GPU is"""
    d = tmp_path_factory.mktemp("cshost")
    prefix = str(d / "toycs")
    nabwa.index_fa2pac(T.TOY + ".fa", prefix, colour=True)
    for ext in ("bwt", "rbwt", "sa", "rsa"):
        shutil.copy(T.TOY + "." + ext, prefix + "." + ext)
    return prefix


def nothing_written(tmp_path, stem):
    return not (tmp_path / (stem + "_")).exists() and not (tmp_path / stem).exists()


def test_colour_sai_without_nt_files_is_refused(tmp_path):
    r = run_tool("samse", ["-f", tmp_path / "a.sam_", T.TOY, G("cs_se.sai"), G("reads_cs_se.fq.gz")])
    assert r.returncode == 1 and r.stdout == b""
    assert b"colour-space" in r.stderr and b".nt." in r.stderr
    assert nothing_written(tmp_path, "a.sam")
    r = run_tool("sampe", ["-s", "-f", tmp_path / "b.sam_", T.TOY, G("cs_pe_1.sai"), G("cs_pe_2.sai"), G("reads_cs_pe_1.fq.gz"), G("reads_cs_pe_2.fq.gz")])
    assert r.returncode == 1 and r.stdout == b"" and b"colour-space" in r.stderr
    assert nothing_written(tmp_path, "b.sam")


def test_colour_sampe_needs_s_or_A(colour_prefix, tmp_path):
    """the reference's mate rescue dereferences a null pac in colour space (bwape.c:651,692-701): refused instead of crashing"""
    ops = [colour_prefix, G("cs_pe_1.sai"), G("cs_pe_2.sai"), G("reads_cs_pe_1.fq.gz"), G("reads_cs_pe_2.fq.gz")]
    r = run_tool("sampe", ["-f", tmp_path / "c.sam_"] + ops)
    assert r.returncode == 1 and r.stdout == b""
    assert b"-s" in r.stderr and b"-A" in r.stderr and b"colour-space" in r.stderr
    assert nothing_written(tmp_path, "c.sam")
    for sw in ("-s", "-A"):                                      # with the switch the run gets as far as the GPU
        r = run_tool("sampe", [sw, "-f", tmp_path / "d.sam_"] + ops)
        assert r.returncode == 2 and r.stdout == b"" and b"no usable GPU" in r.stderr, (sw, r.stderr)
        assert nothing_written(tmp_path, "d.sam")


def test_valid_colour_input_without_a_gpu_exits_2(colour_prefix, tmp_path):
    r = run_tool("samse", ["-f", tmp_path / "e.sam_", colour_prefix, G("cs_se.sai"), G("reads_cs_se.fq.gz")])
    assert r.returncode == 2 and r.stdout == b"" and b"no usable GPU" in r.stderr
    assert nothing_written(tmp_path, "e.sam")


def test_mixed_inputs_follow_the_second_sai(colour_prefix, tmp_path):
    """bwape.c:690-692: the second .sai's option block decides -- colour second: -s is asked for; nucleotide second: it is not"""
    r = run_tool("sampe", [colour_prefix, G("pe_1.sai"), G("cs_pe_2.sai"), G("reads_pe_1.fq"), G("reads_cs_pe_2.fq.gz")])
    assert r.returncode == 1 and b"colour-space" in r.stderr
    r = run_tool("sampe", [colour_prefix, G("cs_pe_1.sai"), G("pe_2.sai"), G("reads_cs_pe_1.fq.gz"), G("reads_pe_2.fq")])
    assert r.returncode == 2, r.stderr


def test_usage_names_the_colour_refusals():
    for name in TOOLS:
        r = run_tool(name, [])
        assert r.returncode == 1 and b"cs2nt.c:129" in r.stderr
    assert b"bwape.c:651" in run_tool("sampe", []).stderr


def test_solid_pairing_golden():
    v = np.load(G("vectors_pe_solid.npz"))
    n = len(v["pr_cnt"])
    differs_from_std = 0
    for t in range(n):
        na0, na1, max_isize = [int(x) for x in v["pr_misc"][t][:3]]
        iiv = v["pr_misc"][t][3:]
        ii = nabwa.IsizeInfo(iiv[0], iiv[1], iiv[2], int(iiv[3]), int(iiv[4]), int(iiv[5]))
        rows = v["pr_aln"][v["pr_aln_off"][t]:v["pr_aln_off"][t + 1]].astype(np.uint32)
        r0 = np.ascontiguousarray(rows[:4 * na0]).view(nabwa.ALN_DT)
        r1 = np.ascontiguousarray(rows[4 * na0:]).view(nabwa.ALN_DT)
        h = v["pr_hit"][v["pr_hit_off"][t]:v["pr_hit_off"][t + 1]].reshape(-1, 3)
        hits = (h[:, 0].astype(np.uint64) << np.uint64(32)) | (h[:, 1].astype(np.uint64) << np.uint64(1)) | h[:, 2].astype(np.uint64)
        res = {}
        for pe_type in (2, 1):
            ends = (nabwa.PeEnd * 2)()
            for e in range(2):
                ends[e] = nabwa.PeEnd(*[int(x) for x in v["pr_in"][t][11 * e:11 * e + 11]])
            cnt = nabwa.pairing_typed(ends, hits.copy(), r0, r1, max_isize, 3, ii, pe_type)
            res[pe_type] = (cnt, [[getattr(ends[e], f) for f, _ in nabwa.PeEnd._fields_] for e in range(2)])
        want = [[int(x) for x in v["pr_out"][t][11 * e:11 * e + 11]] for e in range(2)]
        assert res[2] == (int(v["pr_cnt"][t]), want), t
        differs_from_std += res[1] != res[2]
    assert differs_from_std >= 50                                # the cases tell the two sweeps apart
    with pytest.raises(nabwa.NabwaError):
        nabwa.pairing_typed((nabwa.PeEnd * 2)(), np.zeros(0, np.uint64), r0, r1, 500, 3, ii, 3)
