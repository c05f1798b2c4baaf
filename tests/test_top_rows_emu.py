"""The top of the 32-bit row range on the CPU: an index of A^n whose rows reach kernel D's key-form marker.

For the text A^n every row is known in closed form: row r is the suffix A^r$, SA[r] = n - r, primary = n, L2 = [0, n, n, n, n], and the
stored BWT (the primary row left out) is all A, so Occ(A, r) = min(r + 1, n).  Its `.bwt` words in the reference's layout (bwtio.c:184-204,
bwtmisc.c:120-140) are built here in numpy at three sizes:
  0xfffffefe  the largest text whose searches keep key form (nabwa_batch_deep.hip: seq_len < DEEP_KEYL - 1),
  0xffffff00  the first whose rows reach DEEP_KEYL (fm_deep.hpp): the root [0, n] and the T child's l are rows that look like the marker,
  0xffffffdf  the largest text the library loads (bwtio.c:175 wraps above it).
At each size the oracle's occ4 on the wrapped words must give the closed form, and kernel D's CPU emulation (tests/emu/) must give the
oracle's rows and max_entries on all-A reads, reads with a few substitutions or an indel, and random reads.  Each size runs in a child
process: a search that reads past its tables ends the child, not the suite, and its memory (about 5 GB) goes with it."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import nabwa_testlib as T

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [0xfffffefe, 0xffffff00, 0xffffffdf]


def poly_a_words(n):
    """<prefix>.bwt of A^n as u32 words: primary, L2[1..4], then per 128 rows 4 Occ words and 8 BWT words, and a last Occ"""
    n_occ = (n + 127) // 128 + 1
    size = (n + 15) // 16 + n_occ * 4
    w = np.zeros(5 + size, np.uint32)
    w[:5] = [n, n, n, n, n]
    body = w[5:]
    body[0:12 * (n_occ - 1):12] = (np.arange(n_occ - 1, dtype=np.uint64) * 128).astype(np.uint32)     # Occ(A) before each block
    body[4 * (n_occ - 1) + (n + 15) // 16] = n                                                      # the last checkpoint: all n
    return w


def poly_a_occ4(n, k):
    """closed form of bwt_occ4 on A^n (k = -1: nothing)"""
    k = np.asarray(k, np.int64)
    out = np.zeros((len(k), 4), np.int64)
    out[:, 0] = np.where(k < 0, 0, np.minimum(k + 1, n))
    return out


def deep_opt(name):
    opt, _ = T.read_sai(os.path.join(T.GOLDEN, "se_%s.sai" % name))
    return opt


def reads_for(seed):
    """~300 reads: all-A, 1-3 substitutions, an inserted non-A base or an N (a deleted base would change nothing on A^n), random"""
    rng = np.random.default_rng(seed)
    reads = []
    for L in (17, 32, 33, 50, 76, 100):
        reads.append(np.zeros(L, np.uint8))
    for _ in range(150):
        L = int(rng.choice([32, 36, 50, 64, 76, 100]))
        r = np.zeros(L, np.uint8)
        for p in rng.choice(L, int(rng.integers(1, 4)), replace=False):
            r[p] = rng.integers(1, 4)
        reads.append(r)
    for _ in range(80):
        L = int(rng.choice([36, 50, 76, 100]))
        p = int(rng.integers(1, L - 1))
        r = np.zeros(L, np.uint8)
        if rng.integers(0, 2):
            r = np.concatenate([r[:p], [rng.integers(1, 4)], r[p:-1]]).astype(np.uint8)       # an inserted non-A base
        else:
            r[p] = 4                                                                            # an N
        reads.append(r)
    for _ in range(60):
        L = int(rng.choice([20, 32, 50]))
        r = rng.integers(0, 4, L).astype(np.uint8)
        r[:int(rng.integers(0, L))] = 0                                                         # an all-A start and a random end
        reads.append(r)
    seq = np.concatenate([r[::-1] for r in reads]).astype(np.uint8)                             # bwa_seq_t.seq: the read reversed
    rseq = np.where(seq > 3, 4, 3 - seq).astype(np.uint8)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    return seq, rseq, off


def check_size(n, asan=False, tables=(0,)):
    """the whole check at one size (runs in a child process, see run_child)"""
    import emu_deep as E
    w = poly_a_words(n)
    o = T.load_oracle()
    ox = o.orc_index_wrap(T.ptr(w), len(w), T.ptr(w), len(w))
    try:
        rows = np.unique(np.concatenate([np.arange(n - 599, n + 1), np.arange(2**31 - 300, 2**31 + 300), [0, 1, 127, 128, n - 128]]))
        want = poly_a_occ4(n, rows)
        cnt = np.zeros(4, np.uint32)
        for which in (0, 1):
            for r, wv in zip(rows, want):
                o.orc_occ4(C.c_void_p(ox + which * T.OracleIndex.BWT_SIZE), int(r), T.ptr(cnt))
                assert cnt.tolist() == wv.tolist(), (hex(n), which, int(r), cnt.tolist())
        lib = E.load(asan=asan)
        words = [w, w, np.zeros(8, np.uint32), np.zeros(8, np.uint32)]      # (no .sa: text mode stays off)
        for name, seed in (("default", 1), ("adna", 2)):
            opt = deep_opt(name)
            seq, rseq, off = reads_for(seed)
            want, wmaxe = T.oracle_cal_sa_reg_gap(o, ox, opt, seq, rseq, off)
            assert sum(len(x) for x in want) > 100, "the reads should hit"
            if n >= 0xffffff00:
                assert any(int(x["l"]) >= 0xffffff00 for h in want for x in h), "no hit reaches the marker's rows"
            for table in tables:
                got, maxe, st, _ = E.run(lib, words, opt, seq, rseq, off, table=table)
                bad = [i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes() or st[i] != 0 or maxe[i] != wmaxe[i]]
                assert not bad, "%s, %s options, table %d: %d of %d reads differ, e.g. read %d: %s vs %s" % (
                    hex(n), name, table, len(bad), len(want), bad[0], got[bad[0]][:3], want[bad[0]][:3])
    finally:
        o.orc_index_free(C.c_void_p(ox))
    print("size ok")


def run_child(n, asan=False, tables=(0,)):
    env = dict(os.environ)
    if asan:
        import emu_deep as E
        E.build(asan=True)
        env.update(LD_PRELOAD=subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip(),
                   ASAN_OPTIONS="detect_leaks=0", PYTHONMALLOC="malloc")
    code = "import sys; sys.path.insert(0, %r); import test_top_rows_emu as M; M.check_size(%d, %r, %r)" % (HERE, n, asan, tuple(tables))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=1800)
    assert r.returncode == 0 and "size ok" in r.stdout, "%s: exit %d\n%s\n%s" % (hex(n), r.returncode, r.stdout[-2000:], r.stderr[-4000:])


def test_poly_a_words_small():
    """the word builder against the layout rules on sizes whose blocks end everywhere (the big sizes reuse it unchecked otherwise)"""
    for n in (1, 15, 16, 127, 128, 129, 300, 1000):
        w = poly_a_words(n)
        n_occ = (n + 127) // 128 + 1
        assert len(w) == 5 + (n + 15) // 16 + n_occ * 4
        body = w[5:]
        # walk the layout as bwt_bwtupdate_core writes it (bwtmisc.c:120-140): a checkpoint every 128 bases, a BWT word every 16
        k, c = 0, 0
        for i in range(n):
            if i % 128 == 0:
                assert body[k:k + 4].tolist() == [c, 0, 0, 0], (n, i)
                k += 4
            if i % 16 == 0:
                assert body[k] == 0
                k += 1
            c += 1
        assert body[k:k + 4].tolist() == [n, 0, 0, 0] and k + 4 == len(body), n


@pytest.mark.parametrize("n", SIZES, ids=[hex(n) for n in SIZES])
def test_top_rows(n):
    run_child(n, tables=(0, 6) if n < 0xffffff00 else (0,))


def test_top_rows_asan():
    """the first size whose rows reach the marker, under AddressSanitizer: a row taken for a key reads past the (absent) table"""
    run_child(0xffffff00, asan=True)
