"""Alignment tasks for the DP kernel tests, and ctypes wrappers of the reference's own stdaln cores (oracle/ref_harness.c:
ref_global, ref_local, ref_extend, built into oracle/_ref/libbwaref.so).  Test infrastructure only.

A task is (kind, ref, qry): ref is stdaln's seq1 (the window), qry its seq2 (the read), both uint8 codes 0-4.  Every generator
is seeded and labels its tasks, so that a failure names the kind of input it came from."""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import nabwa_testlib as T

_P = C.c_void_p
_IP = C.POINTER(C.c_int)
SUBO_UNSET = -(1 << 30)          # stdaln leaves *_subo unwritten below the threshold (stdaln.c:633)
REF_THREADS = 16


# ---------------------------------------------------------------------------------------------------------------- the reference
class RefDP:
    """the reference's aln_global_core / aln_local_core / aln_extend_core, one task per call, many calls on a thread pool
    (ctypes drops the GIL; the cores allocate their own memory)"""

    def __init__(self, path=T.REF_SO):
        lib = C.CDLL(path)
        lib.ref_global.restype = C.c_int
        lib.ref_global.argtypes = [_P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, _P, _IP, _P, _IP]
        lib.ref_local.restype = C.c_int
        lib.ref_local.argtypes = [_P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _IP,
                                  _P, _IP, _IP]
        lib.ref_extend.restype = C.c_int
        lib.ref_extend.argtypes = [_P, C.c_int, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _IP,
                                   _P, _IP]
        self.lib = lib
        # the reference's own nucleotide matrices (stdaln.c), read from the compiled library
        self.maq, self.blast, self.hs = [np.array((C.c_int * 25).in_dll(lib, name), np.int32)
                                         for name in ("aln_sm_maq", "aln_sm_blast", "aln_sm_hs")]

    @staticmethod
    def _bufs(l1, l2):
        n = l1 + l2 + 2
        return np.zeros(n, np.uint32), np.zeros(3 * n, np.int32)

    def global_one(self, r, q, gap_open, gap_ext, gap_end, mat, band):
        """-> (score, cigar32)"""
        r, q, mat = _c(r), _c(q), np.ascontiguousarray(mat, np.int32)
        cig, path = self._bufs(len(r), len(q))
        ncig, plen = C.c_int(0), C.c_int(0)
        s = self.lib.ref_global(T.ptr(r), len(r), T.ptr(q), len(q), gap_open, gap_ext, gap_end, T.ptr(mat), 5, band,
                                T.ptr(cig), C.byref(ncig), T.ptr(path), C.byref(plen))
        return int(s), cig[:ncig.value].copy()

    def local_one(self, r, q, gap_open, gap_ext, mat, band, thres):
        """-> (score, coords (start_i, start_j, end_i, end_j) or None where no path was written, subo (SUBO_UNSET where not
        written), cigar32).  The path runs from the end cell back to the start cell (as make_golden.py run_local reads it)."""
        r, q, mat = _c(r), _c(q), np.ascontiguousarray(mat, np.int32)
        cig, path = self._bufs(len(r), len(q))
        ncig, plen, subo = C.c_int(0), C.c_int(0), C.c_int(SUBO_UNSET)
        s = self.lib.ref_local(T.ptr(r), len(r), T.ptr(q), len(q), gap_open, gap_ext, 5, T.ptr(mat), 5, band, thres,
                               T.ptr(cig), C.byref(ncig), T.ptr(path), C.byref(plen), C.byref(subo))
        n_p = plen.value
        coords = (int(path[3 * (n_p - 1)]), int(path[3 * (n_p - 1) + 1]), int(path[0]), int(path[1])) if n_p > 0 else None
        return int(s), coords, int(subo.value), cig[:ncig.value].copy()

    def extend_one(self, r, q, gap_open, gap_ext, mat, band, g0):
        """-> (score, cigar32)"""
        r, q, mat = _c(r), _c(q), np.ascontiguousarray(mat, np.int32)
        cig, path = self._bufs(len(r), len(q))
        ncig, plen = C.c_int(0), C.c_int(0)
        s = self.lib.ref_extend(T.ptr(r), len(r), T.ptr(q), len(q), gap_open, gap_ext, 5, T.ptr(mat), 5, band, int(g0),
                                T.ptr(cig), C.byref(ncig), T.ptr(path), C.byref(plen))
        return int(s), cig[:ncig.value].copy()

    @staticmethod
    def _map(fn, items):
        with ThreadPoolExecutor(max_workers=min(REF_THREADS, os.cpu_count() or 1)) as ex:
            return list(ex.map(fn, items))

    def global_many(self, tasks, gap_open, gap_ext, gap_end, mat, band):
        return self._map(lambda t: self.global_one(t[1], t[2], gap_open, gap_ext, gap_end, mat, band), tasks)

    def local_many(self, tasks, gap_open, gap_ext, mat, band, thres):
        return self._map(lambda t: self.local_one(t[1], t[2], gap_open, gap_ext, mat, band, thres), tasks)

    def extend_many(self, tasks, gap_open, gap_ext, mat, band, g0s):
        return self._map(lambda tg: self.extend_one(tg[0][1], tg[0][2], gap_open, gap_ext, mat, band, tg[1]),
                         list(zip(tasks, g0s)))


def load_ref():
    return RefDP() if os.path.exists(T.REF_SO) else None


def _c(a):
    return np.ascontiguousarray(a, np.uint8)


def flat(tasks):
    """-> ref, ref_off, qry, qry_off as the entry points take them"""
    refs, qrys = [t[1] for t in tasks], [t[2] for t in tasks]
    ro = np.concatenate([[0], np.cumsum([len(x) for x in refs])]).astype(np.int64)
    qo = np.concatenate([[0], np.cumsum([len(x) for x in qrys])]).astype(np.int64)
    cat = lambda xs: np.concatenate([np.asarray(x, np.uint8) for x in xs] + [np.zeros(1, np.uint8)])
    return cat(refs), ro, cat(qrys), qo


# ---------------------------------------------------------------------------------------------------------------- matrices
def asym_matrix(seed, top):
    """a seeded 5x5 matrix that is not symmetric: positive diagonal with maximum `top`, negative elsewhere, an N row and
    column that are not uniform"""
    rng = np.random.default_rng(seed)
    while True:
        m = -rng.integers(1, 3 * top + 2, (5, 5))
        d = rng.integers(1, top + 1, 4)
        d[rng.integers(0, 4)] = top
        m[np.arange(4), np.arange(4)] = d
        if (m != m.T).sum() >= 8 and len(set(m[4].tolist())) > 1 and len(set(m[:, 4].tolist())) > 1:
            return m.reshape(-1).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- sequences
def rand_seq(rng, n, n_rate=0.0):
    s = rng.integers(0, 4, n).astype(np.uint8)
    if n_rate and n:
        s[rng.random(n) < n_rate] = 4
    return s


def mutate(rng, s, sub_rate=0.03, n_indel=2, max_indel=3):
    """substitutions and short indels"""
    s = list(np.asarray(s, np.uint8))
    for p in np.nonzero(rng.random(len(s)) < sub_rate)[0]:
        s[p] = (s[p] + int(rng.integers(1, 4))) % 4
    for _ in range(int(rng.integers(0, n_indel + 1))):
        k = int(rng.integers(1, max_indel + 1))
        p = int(rng.integers(0, len(s) + 1))
        if rng.random() < 0.5:
            del s[p:p + k]
        else:
            s[p:p] = rng.integers(0, 4, k).tolist()
    return np.array(s, np.uint8)


def long_indel(rng, s, lo, hi):
    """one deletion or insertion of lo..hi bases in the middle half"""
    s = np.asarray(s, np.uint8)
    k = int(rng.integers(lo, hi + 1))
    p = int(rng.integers(len(s) // 4, max(len(s) // 4 + 1, 3 * len(s) // 4)))
    if rng.random() < 0.5 and len(s) > k:
        return np.concatenate([s[:p], s[p + k:]])
    return np.concatenate([s[:p], rand_seq(rng, k), s[p:]])


def tandem(rng, period, reps):
    unit = rand_seq(rng, period)
    while len(set(unit.tolist())) < 2:
        unit = rand_seq(rng, period)
    return np.tile(unit, reps)


def with_n_runs(rng, s, runs=2, max_run=6):
    s = np.array(s, np.uint8)
    for _ in range(runs):
        if len(s):
            p = int(rng.integers(0, len(s)))
            s[p:p + int(rng.integers(1, max_run + 1))] = 4
    return s


EDGE_LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257)


# ---------------------------------------------------------------------------------------------------------------- global tasks
def global_tasks(rng, n, band, max_len=200):
    """pairs for aln_global_core, neither side longer than max_len: near-copies, long indels (1-4x the band), unrelated
    pairs, homopolymers, tandem repeats shifted by one period, N runs, all-N reads, very unequal lengths"""
    kinds = ("near", "longindel", "unrelated", "homopolymer", "tandem2", "tandem3", "nrun", "alln", "unequal")
    out = []
    for t in range(n):
        kind = kinds[t % len(kinds)]
        if kind == "near":
            q = rand_seq(rng, int(rng.integers(1, max_len - 10)))
            r = mutate(rng, q)[:max_len]
        elif kind == "longindel":
            k_hi = min(4 * band, max_len // 2)
            k_lo = min(band, k_hi)
            q = rand_seq(rng, int(rng.integers(min(max(2 * k_lo, 8), max_len - k_hi), max_len - k_hi + 1)))
            r = long_indel(rng, q, k_lo, k_hi)
            if rng.random() < 0.5:
                r, q = q, r
        elif kind == "unrelated":
            r, q = rand_seq(rng, int(rng.integers(1, max_len + 1))), rand_seq(rng, int(rng.integers(1, max_len + 1)))
        elif kind == "homopolymer":
            b = int(rng.integers(0, 4))
            l2 = int(rng.integers(1, max_len - 8))
            q = np.full(l2, b, np.uint8)
            r = np.full(max(1, l2 + int(rng.integers(-8, 9))), b, np.uint8)
            if rng.random() < 0.5:
                r[int(rng.integers(0, len(r)))] = (b + 1) % 4
        elif kind in ("tandem2", "tandem3"):
            per = 2 if kind == "tandem2" else 3
            reps = int(rng.integers(3, (max_len - 10) // per))
            tail = rand_seq(rng, int(rng.integers(0, 8)))
            r = np.concatenate([tandem(rng, per, reps), tail])
            q = np.concatenate([r[:per * (reps - 1)], tail])           # one period fewer: where the gap goes is a tie
            if rng.random() < 0.5:
                q = np.concatenate([r[per:per * reps], tail])        # the read shifted by one period
        elif kind == "nrun":
            q = with_n_runs(rng, rand_seq(rng, int(rng.integers(4, max_len - 10))))
            r = with_n_runs(rng, mutate(rng, q))[:max_len]
        elif kind == "alln":
            q = np.full(int(rng.integers(1, max_len)), 4, np.uint8)
            r = rand_seq(rng, int(rng.integers(1, max_len)))
        else:
            r, q = rand_seq(rng, int(rng.integers(1, 6))), rand_seq(rng, int(rng.integers(max_len // 2, max_len)))
            if rng.random() < 0.5:
                r, q = q, r
        out.append((kind, r[:max_len], q[:max_len]))
    return out


def edge_tasks(rng, max_len=257):
    """every pair of the edge lengths (0, 1, and both sides of the 64 / 128 / 256 lane-strip edges), related where both
    have bases"""
    out = []
    for l1 in EDGE_LENGTHS:
        for l2 in EDGE_LENGTHS:
            if l1 > max_len or l2 > max_len:
                continue
            q = rand_seq(rng, l2)
            r = mutate(rng, np.resize(q, l1), n_indel=0) if l1 and l2 else rand_seq(rng, l1)
            out.append(("len%d_%d" % (l1, l2), r, q))
    return out


# ---------------------------------------------------------------------------------------------------------------- local tasks
def local_tasks(rng, n, band, max_read=250, max_flank=250):
    """(window, read) pairs for aln_local_core: near-copies inside a window, long indels (1-4x the band), unrelated pairs,
    homopolymers, tandem repeats, a read present twice in its window, N runs, all-N reads, a read longer than its window"""
    kinds = ("near", "longindel", "unrelated", "homopolymer", "tandem2", "tandem3", "twice", "nrun", "alln", "longread")
    out = []
    fl = lambda: rand_seq(rng, int(rng.integers(0, max_flank + 1)))
    for t in range(n):
        kind = kinds[t % len(kinds)]
        if kind == "near":
            q = rand_seq(rng, int(rng.integers(1, max_read + 1)))
            r = np.concatenate([fl(), mutate(rng, q), fl()])
        elif kind == "longindel":
            q = rand_seq(rng, int(rng.integers(max(2 * band, 20), max(2 * band, 20) + max_read)))
            r = np.concatenate([fl(), long_indel(rng, q, band, 4 * band), fl()])
        elif kind == "unrelated":
            r, q = rand_seq(rng, int(rng.integers(1, 500))), rand_seq(rng, int(rng.integers(1, max_read + 1)))
        elif kind == "homopolymer":
            b = int(rng.integers(0, 4))
            q = np.full(int(rng.integers(1, 80)), b, np.uint8)
            r = np.concatenate([fl(), np.full(len(q) + int(rng.integers(0, 40)), b, np.uint8), fl()])
        elif kind in ("tandem2", "tandem3"):
            per = 2 if kind == "tandem2" else 3
            reps = int(rng.integers(5, 60))
            tr = tandem(rng, per, reps + int(rng.integers(1, 10)))
            q = tr[per:per * reps]                                   # shifted by one period inside a longer repeat
            r = np.concatenate([fl(), tr, fl()])
        elif kind == "twice":
            q = rand_seq(rng, int(rng.integers(10, max_read + 1)))
            r = np.concatenate([fl(), q, rand_seq(rng, int(rng.integers(0, 50))), q, fl()])
        elif kind == "nrun":
            q = with_n_runs(rng, rand_seq(rng, int(rng.integers(10, max_read + 1))), runs=3)
            r = np.concatenate([fl(), with_n_runs(rng, mutate(rng, q)), fl()])
        elif kind == "alln":
            q = np.full(int(rng.integers(1, 100)), 4, np.uint8)
            r = np.concatenate([fl(), rand_seq(rng, 50), fl()])
        else:
            r = rand_seq(rng, int(rng.integers(5, 100)))
            q = np.concatenate([rand_seq(rng, int(rng.integers(0, 60))), mutate(rng, r), rand_seq(rng, int(rng.integers(1, 60)))])
        out.append((kind, r, q))
    return out


def long_copy(rng, l2, flank=50, sub_rate=0.01, n_indel=4):
    """a long read in a window of its near-copy: its best local / extension score grows with its length"""
    q = rand_seq(rng, l2)
    return q, np.concatenate([rand_seq(rng, flank), mutate(rng, q, sub_rate, n_indel), rand_seq(rng, flank)])


# ---------------------------------------------------------------------------------------------------------------- extension tasks
def extend_tasks(rng, n, band, max_len=300):
    """(window prefix, read prefix) pairs for aln_extend_core, both anchored at their first base: near-copies, extensions that
    stop (a matching prefix, then junk), long indels (1-4x the band), homopolymers, tandem repeats, N runs, unrelated pairs"""
    kinds = ("near", "stop", "longindel", "homopolymer", "tandem2", "tandem3", "nrun", "unrelated")
    out = []
    for t in range(n):
        kind = kinds[t % len(kinds)]
        if kind == "near":
            q = rand_seq(rng, int(rng.integers(1, max_len)))
            r = np.concatenate([mutate(rng, q), rand_seq(rng, int(rng.integers(0, 40)))])
        elif kind == "stop":
            m = int(rng.integers(1, 80))
            p = rand_seq(rng, m)
            q = np.concatenate([p, rand_seq(rng, int(rng.integers(0, 150)))])
            r = np.concatenate([mutate(rng, p, n_indel=0), rand_seq(rng, int(rng.integers(0, 150)))])
        elif kind == "longindel":
            q = rand_seq(rng, int(rng.integers(2 * band + 10, 2 * band + 10 + max_len // 2)))
            r = long_indel(rng, q, band, 4 * band)
        elif kind == "homopolymer":
            b = int(rng.integers(0, 4))
            q = np.full(int(rng.integers(1, 100)), b, np.uint8)
            r = np.full(len(q) + int(rng.integers(0, 20)), b, np.uint8)
        elif kind in ("tandem2", "tandem3"):
            per = 2 if kind == "tandem2" else 3
            reps = int(rng.integers(3, 60))
            r = tandem(rng, per, reps + 2)
            q = r[per:] if rng.random() < 0.5 else r[:per * reps]
        elif kind == "nrun":
            q = with_n_runs(rng, rand_seq(rng, int(rng.integers(10, max_len))))
            r = with_n_runs(rng, mutate(rng, q))
        else:
            r, q = rand_seq(rng, int(rng.integers(1, 200))), rand_seq(rng, int(rng.integers(1, 200)))
        out.append((kind, r, q))
    return out


# ---------------------------------------------------------------------------------------------------------------- forms
def global_wave_lds(l1s, l2s, band):
    """LDS bytes of the one-wavefront-per-task global form for a launch of these tasks (nabwa_launch_dp_global)"""
    W, H = max([1] + [a + 1 for a in l1s]), max([1] + [b + 1 for b in l2s])
    maxdiff = max([0] + [abs(a - b) for a, b in zip(l1s, l2s)])
    wb = min(W, 2 * band + maxdiff + 1)
    return 6 * W * 4 + H * ((wb + 1) // 2 + 1) + (W + H) * 2 + 16


def global_lanes_lds(l1s):
    return max([1] + [a + 1 for a in l1s]) * 8 * 25


# ---------------------------------------------------------------------------------------------------------------- parameter blocks
ASYM = {"asym5": (101, 5), "asym100": (202, 100)}       # test-made asymmetric matrices: (seed, maximum score)


def matrix(ref, name):
    if name in ASYM:
        return asym_matrix(*ASYM[name])
    return {"maq": ref.maq, "blast": ref.blast, "hs": ref.hs}[name]


# (gap_open, gap_ext, gap_end, matrix, band) of aln_global_core
GLOBAL_BLOCKS = [(26, 9, 5, "maq", 50), (26, 9, -1, "maq", 50), (37, 9, 0, "maq", 50), (5, 2, 2, "blast", 7),
                 (400, 30, 30, "hs", 20), (13, 4, 4, "asym5", 10), (260, 35, 35, "asym100", 30),
                 (26, 9, 5, "maq", 1), (5, 2, 2, "blast", 1000)]
# (gap_open, gap_ext, matrix, band) of aln_local_core / aln_extend_core
SW_BLOCKS = [(26, 9, "maq", 50), (5, 2, "blast", 7), (400, 30, "hs", 20), (13, 4, "asym5", 10), (260, 35, "asym100", 30)]


def block_id(b):
    return "_".join(str(x) for x in b)
