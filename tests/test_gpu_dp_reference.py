"""The three alignment entry points against the reference's own stdaln cores, called on the spot on fresh tasks (dpgen.py):
 * nabwa_global_align against aln_global_core (ref_global): score and CIGAR;
 * nabwa_local_align against aln_local_core (ref_local): score, first and last cell of the path, sub-optimal score, CIGAR;
 * nabwa_extend_align against aln_extend_core (ref_extend): score and CIGAR.
Every field is compared bit for bit, under the reference's matrices and test-made asymmetric ones, in every form of the kernels;
each case also checks from nabwa.dp_form_counts() that the form it names is the one that ran:
  [0] global, wave per task   [1] global, lanes, rows in LDS   [2] global, lanes, rows in HBM
  [3] local, rows in LDS      [4] local, rows in HBM           [5] extension, rows in LDS   [6] extension, rows in HBM"""
import importlib

import numpy as np
import pytest

import dpgen
import nabwa_testlib as T

nabwa = importlib.import_module("network-aware-bwa_amd")
REF = dpgen.load_ref()
pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(REF is None, reason="compiled reference (oracle/_ref/libbwaref.so) not built")]

KNOBS = ("NABWA_DP_WAVE", "NABWA_DP_SMALL", "NABWA_DP_ROWS", "NABWA_DP_FORWARD")
GLOBAL_FORMS = {"natural": ({}, 0), "lds_lanes": ({"NABWA_DP_WAVE": "0"}, 1),
                "hbm_lanes": ({"NABWA_DP_WAVE": "0", "NABWA_DP_SMALL": "0"}, 2)}
LOCAL_FORMS = {"natural": ({}, 3), "rows_hbm": ({"NABWA_DP_ROWS": "hbm"}, 4), "forward_rows": ({"NABWA_DP_FORWARD": "rows"}, 3),
               "both": ({"NABWA_DP_ROWS": "hbm", "NABWA_DP_FORWARD": "rows"}, 4)}
EXTEND_FORMS = {"natural": ({}, 5), "rows_hbm": ({"NABWA_DP_ROWS": "hbm"}, 6)}
_cache = {}


def set_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def counted(fn):
    """-> fn(), launches by form during the call"""
    c0 = nabwa.dp_form_counts()
    out = fn()
    return out, [b - a for a, b in zip(c0, nabwa.dp_form_counts())]


def expect_forms(d, lo, hi, want):
    """the launches of slots lo..hi-1 during a call were exactly `want` ({slot: count})"""
    assert d[lo:hi] == [want.get(k, 0) for k in range(lo, hi)], (d, want)


def report(bad, what):
    assert not bad, "%s: %d tasks differ from the reference, first: %s" % (what, len(bad), bad[:4])


# ---------------------------------------------------------------------------------------------------------------- global
def gpu_global(tasks, go, ge, gend, mat, band, max_cigar=512):
    """nabwa_global_align as it stands: -> score, full n_cigar, the kept rows of the CIGAR"""
    ref, ro, qry, qo = dpgen.flat(tasks)
    n = len(tasks)
    score, ncig = np.zeros(n, np.int32), np.zeros(n, np.int32)
    cig = np.zeros((n, max_cigar), np.uint32)
    mat = np.ascontiguousarray(mat, np.int32)
    rc = nabwa.lib().nabwa_global_align(0, n, T.ptr(ro), T.ptr(ref), T.ptr(qo), T.ptr(qry), go, ge, gend, T.ptr(mat), band,
                                        T.ptr(score), T.ptr(ncig), T.ptr(cig), max_cigar)
    assert rc == 0, nabwa.lib().nabwa_last_error()
    return score, ncig, [cig[t, :min(int(ncig[t]), max_cigar)] for t in range(n)]


def check_global(tasks, want, got, what, max_cigar=512):
    score, ncig, cigs = got
    bad = []
    for t, ((kind, r, q), (ws, wc)) in enumerate(zip(tasks, want)):
        if (int(score[t]), int(ncig[t]), list(cigs[t])) != (ws, len(wc), list(wc[:max_cigar])):
            bad.append((t, kind, len(r), len(q), int(score[t]), ws))
    report(bad, what)


def global_case(key, make, block):
    """tasks and the reference's answers, made once per key"""
    key = ("global", key)
    if key not in _cache:
        go, ge, gend, mname, band = block
        tasks = make()
        _cache[key] = tasks, REF.global_many(tasks, go, ge, gend, dpgen.matrix(REF, mname), band)
    return _cache[key]


@pytest.mark.parametrize("form", list(GLOBAL_FORMS))
@pytest.mark.parametrize("block", dpgen.GLOBAL_BLOCKS, ids=dpgen.block_id)
def test_global_blocks(monkeypatch, block, form):
    """every parameter block -- symmetric and asymmetric matrices, gap_end 5 / -1 / 0, band 1, a band wider than both
    sequences -- on every kind of task and every pair of edge lengths, in each form of the kernel"""
    go, ge, gend, mname, band = block
    i = dpgen.GLOBAL_BLOCKS.index(block)
    tasks, want = global_case(("blk", i), lambda: dpgen.global_tasks(np.random.default_rng(2000 + i), 360, band)
                              + dpgen.edge_tasks(np.random.default_rng(3000 + i)), block)
    env, slot = GLOBAL_FORMS[form]
    set_env(monkeypatch, env)
    got, d = counted(lambda: gpu_global(tasks, go, ge, gend, dpgen.matrix(REF, mname), band))
    expect_forms(d, 0, 3, {slot: 1})
    check_global(tasks, want, got, (block, form))


def equal_length_tasks(rng, L, n=6):
    out = []
    for k in range(n):
        q = dpgen.rand_seq(rng, L)
        if k % 3 == 0:
            r = dpgen.mutate(rng, q, 0.05, n_indel=0)
        elif k % 3 == 1:
            r = dpgen.tandem(rng, 2 + k % 2, L // 2 + 2)[:L]
            q = r[2 + k % 2:].tolist() + r[:2 + k % 2].tolist()
            q = np.array(q, np.uint8)
        else:
            r = dpgen.with_n_runs(rng, dpgen.mutate(rng, q, 0.02, n_indel=0), runs=3)
        out.append(("eq%d" % L, r, q))
    return out


@pytest.mark.parametrize("L,slots", [(798, {0: 1}), (799, {2: 1})])
def test_global_wave_form_edge(monkeypatch, L, slots):
    """equal-length tasks at band 50: the wave form's LDS is 6 W 4 + H ((wb + 1) / 2 + 1) + (W + H) 2 + 16 with W = H = L + 1 and
    wb = 101 -- 63936 bytes at 798 bases, within the 64000 of nabwa_launch_dp_global, and 64016 at 799, when the lanes take over
    (and with W = 800 the lanes' 8 rows of 25 bytes per column pass 60000: rows in HBM)"""
    set_env(monkeypatch, {})
    block = (26, 9, 5, "maq", 50)
    assert dpgen.global_wave_lds([L], [L], 50) == {798: 63936, 799: 64016}[L]
    tasks, want = global_case(("wave", L), lambda: equal_length_tasks(np.random.default_rng(L), L), block)
    got, d = counted(lambda: gpu_global(tasks, 26, 9, 5, REF.maq, 50))
    expect_forms(d, 0, 3, slots)
    check_global(tasks, want, got, L)


@pytest.mark.parametrize("L,slots", [(299, {1: 1}), (300, {2: 1})])
def test_global_lanes_lds_edge(monkeypatch, L, slots):
    """wave form off: the lanes keep their rows in LDS while (max l1 + 1) 8 25 <= 60000, i.e. windows up to 299 bases"""
    set_env(monkeypatch, {"NABWA_DP_WAVE": "0"})
    assert (dpgen.global_lanes_lds([L]) <= 60000) == (L == 299)
    block = (5, 2, 2, "blast", 7)

    def make():
        rng = np.random.default_rng(10 + L)
        q = dpgen.rand_seq(rng, L - 5)
        return dpgen.global_tasks(rng, 60, 7) + [("window%d" % L, dpgen.mutate(rng, q, n_indel=0)[:L - 5].tolist() + [0] * 5, q)]
    tasks, want = global_case(("lanes", L), lambda: [(k, np.asarray(r, np.uint8), q) for k, r, q in make()], block)
    assert max(len(t[1]) for t in tasks) == L
    got, d = counted(lambda: gpu_global(tasks, 5, 2, 2, REF.blast, 7))
    expect_forms(d, 0, 3, slots)
    check_global(tasks, want, got, L)


@pytest.mark.parametrize("n,slots", [(4096, {1: 1}), (4097, {2: 1})])
def test_global_lanes_task_count_edge(monkeypatch, n, slots):
    """wave form off: the lanes keep their rows in LDS for launches of up to NABWA_DP_SMALL = 4096 tasks"""
    set_env(monkeypatch, {"NABWA_DP_WAVE": "0"})
    block = (26, 9, 5, "asym5", 10)
    tasks, want = global_case("count", lambda: dpgen.global_tasks(np.random.default_rng(41), 4097, 10, max_len=60), block)
    got, d = counted(lambda: gpu_global(tasks[:n], 26, 9, 5, dpgen.matrix(REF, "asym5"), 10))
    expect_forms(d, 0, 3, slots)
    check_global(tasks[:n], want[:n], got, n)


@pytest.mark.parametrize("n,slots", [(65536, {0: 1}), (65537, {0: 1, 2: 1})])
def test_global_chunk_edge(monkeypatch, n, slots):
    """a batch is launched 65536 tasks at a time (CHUNK in nabwa_global_align), each launch in the form of its own largest task:
    65536 small tasks are one wave-form launch; one task more -- a large one -- is a second launch, with its rows in HBM"""
    set_env(monkeypatch, {})
    block = (26, 9, 5, "maq", 50)

    def make():
        rng = np.random.default_rng(65536)
        q = dpgen.rand_seq(rng, 900)
        return dpgen.global_tasks(rng, 65536, 50, max_len=60) + [("large", dpgen.mutate(rng, q, 0.02, 3, 20), q)]
    tasks, want = global_case("chunk", make, block)
    got, d = counted(lambda: gpu_global(tasks[:n], 26, 9, 5, REF.maq, 50))
    expect_forms(d, 0, 3, slots)
    check_global(tasks[:n], want[:n], got, n)


@pytest.mark.parametrize("block", [dpgen.GLOBAL_BLOCKS[k] for k in (0, 4, 6, 7)], ids=dpgen.block_id)
def test_global_small_tasks_in_a_large_tasks_form(monkeypatch, block):
    """the edge lengths and short tasks in one launch with a task of 1000 x 1030 bases, whose size puts the launch in the
    lanes with rows in HBM"""
    set_env(monkeypatch, {})
    go, ge, gend, mname, band = block
    i = dpgen.GLOBAL_BLOCKS.index(block)

    def make():
        rng = np.random.default_rng(500 + i)
        q = dpgen.rand_seq(rng, 1000)
        small = dpgen.edge_tasks(rng) + dpgen.global_tasks(rng, 200, band)
        return small[:150] + [("large", dpgen.long_indel(rng, dpgen.mutate(rng, q), 30, 30), q)] + small[150:]
    tasks, want = global_case(("mixed", i), make, block)
    got, d = counted(lambda: gpu_global(tasks, go, ge, gend, dpgen.matrix(REF, mname), band))
    expect_forms(d, 0, 3, {2: 1})
    check_global(tasks, want, got, block)


@pytest.mark.parametrize("form", list(GLOBAL_FORMS))
@pytest.mark.parametrize("max_cigar", [1, 2, 3])
def test_global_max_cigar_truncation(monkeypatch, max_cigar, form):
    """rows of max_cigar operations: n_cigar is the reference's full count, the kept operations are its first ones"""
    block = (26, 9, 5, "maq", 50)

    def make():
        rng = np.random.default_rng(77)
        out = []
        for t in range(300):
            q = dpgen.rand_seq(rng, int(rng.integers(1, 200)))
            out.append(("indels", dpgen.mutate(rng, q, 0.05, n_indel=8, max_indel=4), q))
        return out
    tasks, want = global_case("trunc", make, block)
    assert sum(1 for _, wc in want if len(wc) > 3) > 150
    env, slot = GLOBAL_FORMS[form]
    set_env(monkeypatch, env)
    got, d = counted(lambda: gpu_global(tasks, 26, 9, 5, REF.maq, 50, max_cigar=max_cigar))
    expect_forms(d, 0, 3, {slot: 1})
    check_global(tasks, want, got, (max_cigar, form), max_cigar=max_cigar)


# ---------------------------------------------------------------------------------------------------------------- local
def check_local(tasks, want, want_end, got, what):
    """want: ref_local at this threshold; want_end: its end cells at thres 1 (the forward pass's, reported with or without a path)"""
    score, coords, subo, cigs = got
    bad = []
    for t, ((kind, r, q), (ws, wco, wsu, wc)) in enumerate(zip(tasks, want)):
        g = (int(score[t]), tuple(int(x) for x in coords[t]), int(subo[t]), list(cigs[t]))
        if wco is None:       # no path: the library's own values -- no CIGAR, subo 0, the end cell of the forward pass alone
            w = (ws, (0, 0) + want_end[t], 0, [])
        else:
            w = (ws, wco, 0 if wsu == dpgen.SUBO_UNSET else wsu, list(wc))
        if g != w:
            bad.append((t, kind, len(r), len(q), g[:3], w[:3]))
    report(bad, what)


def local_case(key, make, block, thres_kinds=("1",)):
    """tasks and the reference's answers for each threshold kind: "1", "mid" (inside the scores), "above" (above every score)"""
    key = ("local", key)
    if key not in _cache:
        go, ge, mname, band = block
        mat = dpgen.matrix(REF, mname)
        tasks = make()
        res = {"1": REF.local_many(tasks, go, ge, mat, band, 1)}
        pos = sorted(x[0] for x in res["1"] if x[0] > 0)
        thres = {"1": 1, "mid": pos[len(pos) // 2] if pos else 1, "above": (pos[-1] if pos else 0) + 1}
        for k in thres_kinds:
            if k != "1":
                res[k] = REF.local_many(tasks, go, ge, mat, band, thres[k])
        ends = [(x[1][2], x[1][3]) if x[1] is not None else (0, 0) for x in res["1"]]
        _cache[key] = tasks, res, thres, ends
    return _cache[key]


def gpu_local(tasks, go, ge, mat, band, thres):
    ref, ro, qry, qo = dpgen.flat(tasks)
    return nabwa.local_align(ref, ro, qry, qo, go, ge, mat, band, thres, max_cigar=4096)


@pytest.mark.parametrize("form", list(LOCAL_FORMS))
@pytest.mark.parametrize("block", dpgen.SW_BLOCKS, ids=dpgen.block_id)
def test_local_blocks(monkeypatch, block, form):
    """every kind of task -- ties (homopolymers, tandem repeats, a read twice in its window), long indels, N runs, all-N reads,
    reads longer than their window, edge lengths -- at three thresholds, in the four forms of the kernel"""
    go, ge, mname, band = block
    i = dpgen.SW_BLOCKS.index(block)
    tasks, res, thres, ends = local_case(("blk", i), lambda: dpgen.local_tasks(np.random.default_rng(4000 + i), 200, band)
                                         + dpgen.edge_tasks(np.random.default_rng(4100 + i))[::3], block, ("1", "mid", "above"))
    env, slot = LOCAL_FORMS[form]
    set_env(monkeypatch, env)
    for k in ("1", "mid", "above"):
        got, d = counted(lambda: gpu_local(tasks, go, ge, dpgen.matrix(REF, mname), band, thres[k]))
        expect_forms(d, 3, 5, {slot: 1})
        check_local(tasks, res[k], ends, got, (block, form, k, thres[k]))
    assert sum(1 for x in res["above"] if x[1] is None) == len(tasks)


@pytest.mark.parametrize("L,slot", [(7107, 3), (7108, 4)])
def test_local_window_edge(monkeypatch, L, slot):
    """a task's rows stay in LDS while W 9 + 16 <= 64000 with W = window + 2: windows of 7107 bases, not 7108"""
    assert ((L + 2) * 9 + 16 <= 64000) == (L == 7107)
    set_env(monkeypatch, {})
    block = (26, 9, "maq", 50)

    def make():
        rng = np.random.default_rng(L)
        q = dpgen.rand_seq(rng, 300)
        w = np.concatenate([dpgen.rand_seq(rng, 5000), dpgen.mutate(rng, q), dpgen.rand_seq(rng, L)])[:L]
        return [("window%d" % L, w, q)] + dpgen.local_tasks(rng, 30, 50)
    tasks, res, _, ends = local_case(("win", L), make, block)
    got, d = counted(lambda: gpu_local(tasks, 26, 9, REF.maq, 50, 1))
    expect_forms(d, 3, 5, {slot: 1})
    check_local(tasks, res["1"], ends, got, L)


@pytest.mark.parametrize("mname,L", [("maq", 2909), ("maq", 2910), ("hs", 320), ("hs", 321)])
@pytest.mark.parametrize("forward", ["natural", "rows"])
def test_local_forward_form_edge(monkeypatch, mname, L, forward):
    """the forward pass runs along the anti-diagonals while l2 max_score <= 32000 (no score can reach the 16-bit drop) and row by
    row beyond: 2909 / 2910 bases under aln_sm_maq (11), 320 / 321 under aln_sm_hs (100).  The choice is not counted; both sides
    are run as dispatched and with the row form forced"""
    mat = dpgen.matrix(REF, mname)
    assert (L * int(mat.max()) <= 32000) == (L in (2909, 320))
    set_env(monkeypatch, {"NABWA_DP_FORWARD": "rows"} if forward == "rows" else {})
    block = (26, 9, mname, 50) if mname == "maq" else (400, 30, mname, 20)

    def make():
        rng = np.random.default_rng(L)
        q, w = dpgen.long_copy(rng, L, sub_rate=0.003, n_indel=2)
        t = dpgen.tandem(rng, 2, L // 2 + 1)[:L]
        return [("copy", w, q), ("tandem", np.concatenate([dpgen.rand_seq(rng, 20), t, t[:50]]), t),
                ("twice", np.concatenate([q[:L // 3], q, q]), q)]
    tasks, res, _, ends = local_case(("fwd", mname, L), make, block)
    got, d = counted(lambda: gpu_local(tasks, block[0], block[1], mat, block[3], 1))
    expect_forms(d, 3, 5, {3: 1})
    check_local(tasks, res["1"], ends, got, (mname, L, forward))


@pytest.mark.parametrize("form", ["natural", "rows_hbm"])
@pytest.mark.parametrize("block", [dpgen.SW_BLOCKS[k] for k in (0, 2, 4)], ids=dpgen.block_id)
def test_local_drops_ties_and_long_indels(monkeypatch, block, form):
    """scores that pass 32000 once (one 16-bit drop) and 48000 (two drops), beside tie-rich and long-indel tasks"""
    go, ge, mname, band = block
    mat = dpgen.matrix(REF, mname)
    i = dpgen.SW_BLOCKS.index(block)
    per_base = float(np.mean(mat.reshape(5, 5).diagonal()[:4]))

    def make():
        rng = np.random.default_rng(6000 + i)
        out = []
        for target, tag in ((36000, "one_drop"), (52000, "two_drops")):
            q, w = dpgen.long_copy(rng, int(target / per_base * 1.04), sub_rate=0.002, n_indel=2)
            out.append((tag, w, q))
        ties = [t for t in dpgen.local_tasks(rng, 120, band) if t[0] in ("homopolymer", "tandem2", "tandem3", "twice", "longindel")]
        return out + ties
    tasks, res, _, ends = local_case(("drop", i), make, block)
    assert res["1"][0][0] > 32000 and res["1"][1][0] > 48000
    env, slot = LOCAL_FORMS[form]
    set_env(monkeypatch, env)
    got, d = counted(lambda: gpu_local(tasks, go, ge, mat, band, 1))
    expect_forms(d, 3, 5, {slot: 1})
    check_local(tasks, res["1"], ends, got, (block, form))


# ---------------------------------------------------------------------------------------------------------------- extension
def extend_case(key, make, block, band):
    key = ("extend", key)
    if key not in _cache:
        go, ge, mname, _ = block
        tasks, g0 = make()
        _cache[key] = tasks, g0, REF.extend_many(tasks, go, ge, dpgen.matrix(REF, mname), band, g0)
    return _cache[key]


def gpu_extend(tasks, go, ge, mat, band, g0):
    ref, ro, qry, qo = dpgen.flat(tasks)
    return nabwa.extend_align(ref, ro, qry, qo, go, ge, mat, band, np.asarray(g0, np.int32), max_cigar=4096)


def check_extend(tasks, g0, want, got, what):
    score, cigs = got
    bad = [(t, kind, len(r), len(q), g0[t], int(score[t]), ws)
           for t, ((kind, r, q), (ws, wc)) in enumerate(zip(tasks, want)) if (int(score[t]), list(cigs[t])) != (ws, list(wc))]
    report(bad, what)


def g0_mix(rng, n):
    """seeds from 1 to 600, 0 (the reference returns -1 there), and 31900 - 32000, where the first row already drops"""
    g = rng.integers(1, 601, n)
    u = rng.random(n)
    g[u < 0.1] = 0
    hi = u > 0.75
    g[hi] = rng.integers(31900, 32001, int(hi.sum()))
    return g.astype(np.int32)


@pytest.mark.parametrize("form", list(EXTEND_FORMS))
@pytest.mark.parametrize("band", [1, 12, 50, 1000])
@pytest.mark.parametrize("block", dpgen.SW_BLOCKS, ids=dpgen.block_id)
def test_extend_blocks(monkeypatch, block, band, form):
    """every kind of extension (stopping early among them), every seed range, bands of 1, 12, 50 and wider than both sequences"""
    go, ge, mname, _ = block
    i = dpgen.SW_BLOCKS.index(block)

    def make():
        rng = np.random.default_rng(7000 + 10 * i + band)
        tasks = dpgen.extend_tasks(rng, 200, min(band, 60)) + dpgen.edge_tasks(rng)[::4]
        return tasks, g0_mix(rng, len(tasks))
    tasks, g0, want = extend_case(("blk", i, band), make, block, band)
    env, slot = EXTEND_FORMS[form]
    set_env(monkeypatch, env)
    got, d = counted(lambda: gpu_extend(tasks, go, ge, dpgen.matrix(REF, mname), band, g0))
    expect_forms(d, 5, 7, {slot: 1})
    check_extend(tasks, g0, want, got, (block, band, form))


@pytest.mark.parametrize("L,slot", [(7107, 5), (7108, 6)])
def test_extend_window_edge(monkeypatch, L, slot):
    """the extension keeps its rows in LDS under the local rule: windows of 7107 bases, not 7108"""
    set_env(monkeypatch, {})
    block = (26, 9, "maq", 50)

    def make():
        rng = np.random.default_rng(L + 1)
        q = dpgen.rand_seq(rng, 400)
        tasks = [("window%d" % L, np.concatenate([dpgen.mutate(rng, q), dpgen.rand_seq(rng, L)])[:L], q)]
        tasks += dpgen.extend_tasks(rng, 30, 50)
        return tasks, g0_mix(rng, len(tasks))
    tasks, g0, want = extend_case(("win", L), make, block, 50)
    got, d = counted(lambda: gpu_extend(tasks, 26, 9, REF.maq, 50, g0))
    expect_forms(d, 5, 7, {slot: 1})
    check_extend(tasks, g0, want, got, L)


@pytest.mark.parametrize("form", list(EXTEND_FORMS))
@pytest.mark.parametrize("block", [dpgen.SW_BLOCKS[k] for k in (0, 2, 4)], ids=dpgen.block_id)
def test_extend_drops(monkeypatch, block, form):
    """extensions whose scores pass 32000 once and 48000 (two 16-bit drops), from small seeds and from seeds just under 32000"""
    go, ge, mname, band = block
    mat = dpgen.matrix(REF, mname)
    i = dpgen.SW_BLOCKS.index(block)
    per_base = float(np.mean(mat.reshape(5, 5).diagonal()[:4]))

    def make():
        rng = np.random.default_rng(8000 + i)
        tasks, g0 = [], []
        for target, tag in ((36000, "one_drop"), (52000, "two_drops")):
            for seed in (int(rng.integers(1, 600)), 31990):
                L = int(max(target - seed, 2000) / per_base * 1.04)
                q = dpgen.rand_seq(rng, L)
                tasks.append((tag, np.concatenate([dpgen.mutate(rng, q, 0.002, 2), dpgen.rand_seq(rng, 30)]), q))
                g0.append(seed)
        return tasks, np.array(g0, np.int32)
    tasks, g0, want = extend_case(("drop", i), make, block, band)
    # the seed counts towards the forward score (the 31990 ones drop in their first row), not towards the returned one: that is
    # the global score of the two prefixes (stdaln.c:985-1000)
    assert want[0][0] > 32000 and want[2][0] > 48000
    env, slot = EXTEND_FORMS[form]
    set_env(monkeypatch, env)
    got, d = counted(lambda: gpu_extend(tasks, go, ge, mat, band, g0))
    expect_forms(d, 5, 7, {slot: 1})
    check_extend(tasks, g0, want, got, (block, form))


# ---------------------------------------------------------------------------------------------------------------- arena reuse
def test_arena_reuse(monkeypatch):
    """each entry point: a batch, a larger and different one, the first again, the working memory given back, the first once
    more -- every run of the first batch identical, and equal to the reference"""
    set_env(monkeypatch, {})
    rng = np.random.default_rng(99)
    small_g, big_g = dpgen.global_tasks(rng, 100, 50), dpgen.global_tasks(rng, 3000, 50, max_len=200)
    q = dpgen.rand_seq(rng, 2000)
    big_g.append(("large", dpgen.mutate(rng, q), q))
    small_l, big_l = dpgen.local_tasks(rng, 60, 50), dpgen.local_tasks(rng, 400, 50, max_flank=2000)
    small_e, big_e = dpgen.extend_tasks(rng, 80, 50), dpgen.extend_tasks(rng, 600, 50, max_len=600)
    g0_s, g0_b = g0_mix(rng, len(small_e)), g0_mix(rng, len(big_e))
    mat = REF.maq
    runs = {
        "global": (lambda ts: gpu_global(ts, 26, 9, 5, mat, 50), small_g, big_g,
                   lambda g: check_global(small_g, REF.global_many(small_g, 26, 9, 5, mat, 50), g, "global")),
        "local": (lambda ts: gpu_local(ts, 26, 9, mat, 50, 1), small_l, big_l, None),
        "extend": (lambda ts: gpu_extend(ts, 26, 9, mat, 50, g0_s if ts is small_e else g0_b), small_e, big_e,
                   lambda g: check_extend(small_e, g0_s, REF.extend_many(small_e, 26, 9, mat, 50, g0_s), g, "extend")),
    }
    want_l = REF.local_many(small_l, 26, 9, mat, 50, 1)
    ends_l = [(x[1][2], x[1][3]) if x[1] is not None else (0, 0) for x in want_l]
    runs["local"] = runs["local"][:3] + (lambda g: check_local(small_l, want_l, ends_l, g, "local"),)

    def key(out):
        return [np.asarray(x).tobytes() if not isinstance(x, list) else [np.asarray(c).tobytes() for c in x] for x in out]
    for name, (run, small, big, check) in runs.items():
        first = run(small)
        check(first)
        run(big)
        again = run(small)
        nabwa.lib().nabwa_dp_scratch_release(0)
        fresh = run(small)
        assert key(first) == key(again) == key(fresh), name


@pytest.mark.parametrize("form", list(EXTEND_FORMS))
def test_extend_drop_cuts_a_long_insertion(monkeypatch, form):
    """under aln_sm_hs the score passes 32000 within a 340-base match, and the drop leaves some 16000 in the 16-bit cells: 700
    inserted read bases (400 + 700 x 30) after the match run them to 0 before the read's last 400 bases match again.  Without the
    drop the extension would cross the insertion (it does at 500 bases); the reference stops at the end of the first match"""
    set_env(monkeypatch, {})
    block = (400, 30, "hs", 720)

    def make():
        rng = np.random.default_rng(340)
        tasks = []
        for _ in range(4):
            p, x = dpgen.rand_seq(rng, 340), dpgen.rand_seq(rng, 400)
            tasks.append(("drop_cuts_gap", np.concatenate([p, x]), np.concatenate([p, dpgen.rand_seq(rng, 700), x])))
        return tasks, np.array([1, 300, 600, 31990], np.int32)
    tasks, g0, want = extend_case("cut", make, block, 720)
    assert all(len(w[1]) == 1 and w[0] > 32000 for w in want)       # one match run: the insertion was not crossed
    env, slot = EXTEND_FORMS[form]
    set_env(monkeypatch, env)
    got, d = counted(lambda: gpu_extend(tasks, 400, 30, REF.hs, 720, g0))
    expect_forms(d, 5, 7, {slot: 1})
    check_extend(tasks, g0, want, got, form)
