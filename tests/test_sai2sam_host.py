"""Host-only tests of `nabwa_samse` / `nabwa_sampe` pieces (no GPU needed):
 * nabwa_isize_infer_pairs -- `bwa sampe`'s per-chunk insert-size estimate (reference bwape.c:74-175) -- against the estimate the
   reference's own code computed on the same positioned pairs (ii_sampe of the committed PE chain vectors), and on its failure paths;
 * the command lines' argument errors, which must exit 1 before any GPU is touched."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import nabwa_testlib as T

nabwa = importlib.import_module("network-aware-bwa_amd")

# posn_f columns (make_golden.py snapshot of bwa_seq_t after the SE step of bwa_cal_pac_pos_pe)
TYPE, POS, MAPQ, LEN = 0, 9, 10, 16


def toy_l_pac():
    return int(open(T.TOY + ".ann").read().split()[0])


@pytest.mark.parametrize("tag", ["", "150", "short"])
def test_isize_infer_pairs_equals_the_reference_estimate(tag):
    v = np.load(os.path.join(T.GOLDEN, "vectors_pe%s_chain.npz" % tag))
    f = v["posn_f"]
    # what the reference reads: pos and len whatever the type, mapQ as the SE step left it (0 for unmapped ends)
    rc, ii, log = nabwa.isize_infer_pairs(f[:, POS], f[:, LEN], f[:, MAPQ], 1e-5, toy_l_pac())
    assert rc == 0
    want = v["ii_sampe"]
    assert (ii.avg, ii.std, ii.ap_prior, ii.low, ii.high, ii.high_bayesian) == tuple(want)
    lines = log.splitlines()
    assert len(lines) == 5 and all(l.startswith("[infer_isize] ") for l in lines)
    assert lines[1] == "[infer_isize] low and high boundaries: %d and %d for estimating avg and std" % (want[3], want[4])
    assert "inferred maximum insert size: %d (" % want[5] in lines[4]
    assert (f[:, TYPE] > 0).sum() > 0


def pairs(isizes, length=100, mapq=37):
    """positioned pairs with the given outer distances: end 0 at 1000 + 10 * i, end 1 downstream"""
    n = len(isizes)
    pos = np.zeros(2 * n, np.uint32)
    ln = np.full(2 * n, length, np.int32)
    mq = np.full(2 * n, mapq, np.int32)
    for i, d in enumerate(isizes):
        pos[2 * i] = 1000 + 10 * i
        pos[2 * i + 1] = pos[2 * i] + d - length
    return pos, ln, mq


def assert_failed(ii):
    assert ii.avg == -1.0 and ii.std == -1.0 and ii.low == 0 and ii.high == 0 and ii.high_bayesian == 0


def test_isize_infer_pairs_too_few_good_pairs():
    pos, ln, mq = pairs([300 + i % 7 for i in range(40)])
    mq[1:41:2] = 19                     # 20 of the 40 pairs lose their second end's mapQ >= 20: 20 good pairs left ...
    rc, ii, log = nabwa.isize_infer_pairs(pos, ln, mq, 1e-5, 10 ** 6)
    assert rc == 0
    mq[1:43:2] = 19                     # ... one fewer is not enough
    rc, ii, log = nabwa.isize_infer_pairs(pos, ln, mq, 1e-5, 10 ** 6)
    assert rc == nabwa.ISIZE_FEW
    assert_failed(ii)
    assert ii.ap_prior == 1e-5                                     # defined on this path too: the prior it was given
    assert log == "[infer_isize] fail to infer insert size: too few good pairs\n"


def test_isize_infer_pairs_weird_pairing():
    # one distance for every pair: the sum of squares starts from -1.0 (bwape.c:86), so std is the root of a negative number
    pos, ln, mq = pairs([300] * 40)
    rc, ii, log = nabwa.isize_infer_pairs(pos, ln, mq, 1e-5, 10 ** 6)
    assert rc == nabwa.ISIZE_WEIRD
    assert_failed(ii)
    assert log.splitlines() == ["[infer_isize] (25, 50, 75) percentile: (300, 300, 300)", "[infer_isize] fail to infer insert size: weird pairing"]


def test_isize_infer_pairs_ignores_distances_of_100000_and_more():
    pos, ln, mq = pairs([100000 + 7 * i for i in range(50)] + [99999] * 19)
    rc, ii, log = nabwa.isize_infer_pairs(pos, ln, mq, 1e-5, 10 ** 7)
    assert rc == nabwa.ISIZE_FEW
    assert_failed(ii)


def test_isize_infer_pairs_floors_low_at_the_longest_read():
    # quartiles 200 / 210 / 220: p25 - 2 (p75 - p25) = 160, but one read of the chunk is 180 bases long
    d = [200] * 30 + [210] * 30 + [220] * 30
    pos, ln, mq = pairs(d, length=50)
    rc, ii, _ = nabwa.isize_infer_pairs(pos, ln, mq, 1e-5, 10 ** 6)
    assert rc == 0 and ii.low == 160 and ii.high == 260
    ln[7] = 180                          # an end that takes no part in any distance still counts for the floor
    mq[6] = 0
    pos[6] = 10 ** 6
    rc, ii, _ = nabwa.isize_infer_pairs(pos, ln, mq, 1e-5, 10 ** 6)
    assert rc == 0 and ii.low == 180
    # the end with mapQ 0 dropped its pair from the distances
    assert ii.avg == pytest.approx(np.mean([x for i, x in enumerate(d) if i != 3 and 180 <= x <= 260]))


def test_isize_infer_pairs_reference_arithmetic():
    rng = np.random.default_rng(7)
    d = np.concatenate([rng.normal(350, 30, 400).astype(int), rng.integers(2000, 90000, 9)])
    pos, ln, mq = pairs(d)
    rc, ii, log = nabwa.isize_infer_pairs(pos, ln, mq, 1e-5, 3 * 10 ** 6)
    assert rc == 0
    s = np.sort(d.astype(np.uint64))
    tot = len(s)
    p25, p50, p75 = (int(s[int(tot * q + 0.5)]) for q in (0.25, 0.5, 0.75))
    low = max(int(p25 - 2.0 * (p75 - p25) + .499), 100)
    high = int(p75 + 2.0 * (p75 - p25) + .499)
    inl = s[(s >= low) & (s <= high)]
    avg = float(int(inl.sum())) / len(inl)
    ss = -1.0
    for x in inl:
        ss += (float(x) - avg) * (float(x) - avg)
    std = float(np.sqrt(ss / len(inl)))
    assert (ii.low, ii.high) == (low, high)
    assert ii.avg == avg and ii.std == std
    assert log.splitlines()[0] == "[infer_isize] (25, 50, 75) percentile: (%d, %d, %d)" % (p25, p50, p75)
    assert ii.high_bayesian >= int(avg) and ii.ap_prior >= 1e-5


TOOLS = {"samse": nabwa.SAMSE_PATH, "sampe": nabwa.SAMPE_PATH}


def run_tool(name, args):
    env = dict(os.environ, NABWA_DEVICE="99")                    # no such GPU: what exits 1 must do so before looking for one
    if not os.path.exists(TOOLS[name]):
        pytest.fail("%s was not built" % TOOLS[name])
    return subprocess.run([TOOLS[name]] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=60)


@pytest.mark.parametrize("name,args", [
    ("samse", []),
    ("samse", [T.TOY]),
    ("samse", [T.TOY, os.path.join(T.GOLDEN, "se_default.sai")]),
    ("sampe", [T.TOY, os.path.join(T.GOLDEN, "pe_1.sai"), os.path.join(T.GOLDEN, "pe_2.sai"), os.path.join(T.GOLDEN, "reads_pe_1.fq")]),
    ("samse", ["-r", "RG\\tID:x", T.TOY, os.path.join(T.GOLDEN, "se_default.sai"), os.path.join(T.GOLDEN, "reads_se.fq")]),
    ("samse", ["-r", "@RG\\tSM:y", T.TOY, os.path.join(T.GOLDEN, "se_default.sai"), os.path.join(T.GOLDEN, "reads_se.fq")]),
    ("sampe", ["-r", "@RG SM:y", T.TOY, "a", "b", "c", "d"]),
    ("samse", ["-n", "16", T.TOY, os.path.join(T.GOLDEN, "se_default.sai"), os.path.join(T.GOLDEN, "reads_se.fq")]),
    ("sampe", ["-N", "17", T.TOY] + [os.path.join(T.GOLDEN, x) for x in ("pe_1.sai", "pe_2.sai", "reads_pe_1.fq", "reads_pe_2.fq")]),
    ("samse", [T.TOY, os.path.join(T.GOLDEN, "no_such.sai"), os.path.join(T.GOLDEN, "reads_se.fq")]),
    ("samse", [T.TOY, os.path.join(T.GOLDEN, "se_default.sai"), os.path.join(T.GOLDEN, "no_such.fq")]),
    ("samse", [T.TOY + "_missing", os.path.join(T.GOLDEN, "se_default.sai"), os.path.join(T.GOLDEN, "reads_se.fq")]),
    ("samse", ["-x", T.TOY, os.path.join(T.GOLDEN, "se_default.sai"), os.path.join(T.GOLDEN, "reads_se.fq")]),
])
def test_argument_errors_exit_1_without_a_gpu(name, args, tmp_path):
    r = run_tool(name, args + [])
    assert r.returncode == 1, r.stderr
    assert r.stdout == b""


def test_no_gpu_exits_2_and_writes_nothing(tmp_path):
    out = tmp_path / "o.sam_"
    r = run_tool("samse", ["-f", str(out), T.TOY, os.path.join(T.GOLDEN, "se_default.sai"), os.path.join(T.GOLDEN, "reads_se.fq")])
    assert r.returncode == 2 and r.stdout == b""
    assert b"no usable GPU" in r.stderr
    assert not out.exists() and not (tmp_path / "o.sam").exists()


def test_colour_space_sai_is_refused(tmp_path):
    raw = bytearray(open(os.path.join(T.GOLDEN, "se_default.sai"), "rb").read())
    mode = int.from_bytes(raw[12:16], "little") & ~2           # gap_opt_t.mode without BWA_MODE_COMPREAD
    raw[12:16] = mode.to_bytes(4, "little")
    p = tmp_path / "cs.sai"
    p.write_bytes(bytes(raw))
    r = run_tool("samse", [T.TOY, str(p), os.path.join(T.GOLDEN, "reads_se.fq")])
    assert r.returncode == 1 and b"colour-space" in r.stderr
