"""What the tests of the duplicate-read stage (NABWA_DEDUP=1) share: the CPU build of csrc/dedup_body.hpp (tests/emu/dedup_emu.cpp), and the
fixed inputs of tests/test_gpu_dedup.py, so that tests/test_dedup_emu.py can hash the same reads without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np

import nabwa_testlib as T
import test_gpu_batch_mix as M

EMU_DIR = os.path.join(T.ROOT, "tests", "emu")
CSRC = os.path.join(T.ROOT, "network-aware-bwa_amd", "csrc")
SRCS = [os.path.join(EMU_DIR, "dedup_emu.cpp"), os.path.join(EMU_DIR, "emu_hip.hpp"), os.path.join(CSRC, "dedup_body.hpp")]
NEAR_LENS = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257)


def build_emu():
    out = os.path.join(EMU_DIR, "libdedup_emu.so")
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(s) for s in SRCS):
        return out
    subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + EMU_DIR, "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", SRCS[0], "-o", out],
                   check=True)
    return out


def load_emu():
    lib = C.CDLL(build_emu())
    P = C.c_void_p
    lib.emu_dedup_hash.restype = C.c_uint64
    lib.emu_dedup_hash.argtypes = [P, P, C.c_int64, C.c_int]
    lib.emu_dedup_hash_batch.restype = None
    lib.emu_dedup_hash_batch.argtypes = [C.c_int, P, P, P, P]
    lib.emu_dedup_equal.restype = C.c_int
    lib.emu_dedup_equal.argtypes = [P, P, P, C.c_int, C.c_int]
    return lib


def emu_hashes(emu, seq, rseq, off):
    seq, rseq, off = np.ascontiguousarray(seq, np.uint8), np.ascontiguousarray(rseq, np.uint8), np.ascontiguousarray(off, np.int64)
    out = np.zeros(len(off) - 1, np.uint64)
    if len(seq) == 0:
        seq = rseq = np.zeros(1, np.uint8)
    emu.emu_dedup_hash_batch(len(off) - 1, T.ptr(seq), T.ptr(rseq), T.ptr(off), T.ptr(out))
    return out


def keys_of(seq, rseq, off):
    """what makes two reads of a batch one read: length and the bytes of both strands"""
    return [(int(off[i + 1] - off[i]), seq[off[i]:off[i + 1]].tobytes(), rseq[off[i]:off[i + 1]].tobytes()) for i in range(len(off) - 1)]


def n_distinct(seq, rseq, off):
    return len(set(keys_of(seq, rseq, off)))


# ---------------------------------------------------------------------------------------------------------------- the mixed pool (case 1)
def mixed_pool():
    """(kinds, distinct reads as text): exact, 2 % errors, ancient-DNA-like at 25-70 bp, all-N, empty, poly-T, tandem repeats, 250-600 bp"""
    rng = np.random.default_rng(20261019)
    G = M.genome_text(T.TOY)
    pool = [(k, s) for k, s in M.build_pool(G, rng, (250, 300, 600))
            if k in ("exact100", "err100", "adna", "allN", "empty", "polyT", "tandem", "long250", "long300", "long600")]
    seen, kinds, reads = set(), [], []
    for k, s in pool:                      # the pool's own equal reads (its empty reads) once: the ids below are ids of distinct reads
        if s not in seen:
            seen.add(s)
            kinds.append(k)
            reads.append(s)
    return kinds, reads


def mixed_batch(n_reads, seed=5):
    """every distinct read 1..5 times, shuffled -> ids into the pool, one per read of the batch"""
    rng = np.random.default_rng(seed)
    ids = np.repeat(np.arange(n_reads), rng.integers(1, 6, n_reads))
    return [int(i) for i in rng.permutation(ids)]


# ---------------------------------------------------------------------------------------------------------------- near-duplicates (case 3)
def near_duplicates():
    """(seq, rseq, off, distinct reads): for every length of NEAR_LENS a read, the same seq under another rseq, its one-base extension, the read
    with only its first and with only its last byte changed -- and one exact copy of the read, so that the stage has something to merge.
    A read of an odd number of junk bases in front of each group puts the starts on odd byte offsets."""
    rng = np.random.default_rng(77)
    seqs, rseqs = [], []

    def add(s, r):
        seqs.append(np.asarray(s, np.uint8))
        rseqs.append(np.asarray(r, np.uint8))
    for L in NEAR_LENS:
        pad = 2 * int(rng.integers(0, 8)) + 1
        if sum(len(x) for x in seqs) % 2 == 1:
            pad += 1                                    # the group starts at an odd offset
        add(rng.integers(0, 4, pad), rng.integers(0, 4, pad))
        s = rng.integers(0, 4, L).astype(np.uint8)
        r = (3 - s)[::-1].copy()
        add(s, r)
        r2 = r.copy(); r2[L // 2] = (r2[L // 2] + 1) % 4
        add(s, r2)                                      # the same seq, another rseq
        e = np.concatenate([s, [0]]).astype(np.uint8)   # one base more; the new base is code 0, the pad value of the hash's last chunk
        add(e, np.concatenate([[3], r]).astype(np.uint8))
        f = s.copy(); f[0] = (f[0] + 1) % 4
        add(f, r)
        g = s.copy(); g[-1] = (g[-1] + 2) % 4
        add(g, r)
        add(s, r)                                       # the copy
    off = np.concatenate([[0], np.cumsum([len(x) for x in seqs])]).astype(np.int64)
    seq, rseq = np.concatenate(seqs).astype(np.uint8), np.concatenate(rseqs).astype(np.uint8)
    starts = [int(off[7 * g + 1]) for g in range(len(NEAR_LENS))]
    assert all(x % 2 == 1 for x in starts), starts
    return seq, rseq, off
