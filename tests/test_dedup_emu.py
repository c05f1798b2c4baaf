"""The bodies of the duplicate-read stage (csrc/dedup_body.hpp; NABWA_DEDUP=1) on the CPU (tests/emu/dedup_emu.cpp): the hash of a read over
its length and both strands, and the exact comparison that decides a merge.  The hash must not depend on where a read lies, must see every
byte of both strands and the length, and neither body may touch a byte beyond the reads' buffers."""
import os
import subprocess

import numpy as np
import pytest

import dedup_cases as D
import nabwa_testlib as T

LENS = list(range(1, 41)) + [63, 64, 65, 100, 257]


@pytest.fixture(scope="module")
def emu():
    return D.load_emu()


def batch_of(reads):
    """[(seq, rseq)] -> seq, rseq, off"""
    off = np.concatenate([[0], np.cumsum([len(s) for s, _ in reads])]).astype(np.int64)
    cat = lambda xs: np.concatenate(xs + [np.zeros(0, np.uint8)]).astype(np.uint8)
    return cat([s for s, _ in reads]), cat([r for _, r in reads]), off


def test_hash_does_not_depend_on_where_the_read_lies(emu):
    """equal reads hash equal at every byte offset of their start (0..15 within the buffer) and at every position in the batch"""
    rng = np.random.default_rng(1)
    for L in [0] + LENS:
        s, r = rng.integers(0, 5, L).astype(np.uint8), rng.integers(0, 5, L).astype(np.uint8)
        seen = set()
        for shift in range(16):
            junk = (rng.integers(0, 5, shift).astype(np.uint8), rng.integers(0, 5, shift).astype(np.uint8))
            other = (rng.integers(0, 5, 37).astype(np.uint8), rng.integers(0, 5, 37).astype(np.uint8))
            seq, rseq, off = batch_of([junk, (s, r), other, (s, r), other, other, (s, r)])
            h = D.emu_hashes(emu, seq, rseq, off)
            assert off[1] % 16 == shift
            seen |= {int(h[1]), int(h[3]), int(h[6])}
            assert emu.emu_dedup_equal(T.ptr(seq), T.ptr(rseq), T.ptr(off), 6, 1) == 1
        assert len(seen) == 1, L


def test_hash_and_equality_see_every_byte_of_both_strands_and_the_length(emu):
    """lengths 1..40, 63, 64, 65, 100, 257: a change of any single byte of seq, or of rseq alone, changes the hash, and so does a change of the
    length by one with the same prefix (the added byte is code 0 and code 4 in turn); the comparison tells each of them from the read"""
    rng = np.random.default_rng(2)
    n_checked = 0
    for L in LENS:
        s, r = rng.integers(0, 5, L).astype(np.uint8), rng.integers(0, 5, L).astype(np.uint8)
        reads = [(s, r)]
        for strand in (0, 1):
            for k in range(L):
                x = [s.copy(), r.copy()]
                x[strand][k] = (x[strand][k] + 1 + k % 4) % 5
                reads.append((x[0], x[1]))
        for extra in (0, 4):
            reads.append((np.append(s, extra).astype(np.uint8), np.append(r, extra).astype(np.uint8)))
        reads.append((s[:-1], r[:-1]))
        seq, rseq, off = batch_of(reads)
        h = D.emu_hashes(emu, seq, rseq, off)
        assert len(reads) == 2 * L + 4
        bad = [i for i in range(1, len(reads)) if h[i] == h[0]]
        assert not bad, (L, bad)
        for i in range(1, len(reads)):
            assert emu.emu_dedup_equal(T.ptr(seq), T.ptr(rseq), T.ptr(off), i, 0) == 0, (L, i)
        assert emu.emu_dedup_equal(T.ptr(seq), T.ptr(rseq), T.ptr(off), 0, 0) == 1
        n_checked += len(reads) - 1
    assert n_checked == sum(2 * L + 3 for L in LENS)


def test_equality_is_exact_on_random_pairs(emu):
    """pairs that differ in 0, 1 or 2 bytes anywhere: the body's answer is numpy's"""
    rng = np.random.default_rng(3)
    for L in [0] + LENS:
        reads = []
        for _ in range(12):
            s, r = rng.integers(0, 5, L).astype(np.uint8), rng.integers(0, 5, L).astype(np.uint8)
            s2, r2 = s.copy(), r.copy()
            for _ in range(int(rng.integers(0, 3))):
                if L:
                    (s2 if rng.random() < 0.5 else r2)[int(rng.integers(0, L))] = int(rng.integers(0, 5))
            reads += [(s, r), (s2, r2)]
        seq, rseq, off = batch_of(reads)
        for i in range(0, len(reads), 2):
            want = int(np.array_equal(reads[i][0], reads[i + 1][0]) and np.array_equal(reads[i][1], reads[i + 1][1]))
            assert emu.emu_dedup_equal(T.ptr(seq), T.ptr(rseq), T.ptr(off), i + 1, i) == want, (L, i)


def test_no_two_distinct_reads_of_the_gpu_tests_inputs_share_a_hash(emu):
    """tests/test_gpu_dedup.py asserts that no read meets a hash collision at 64 bits; the same reads, hashed here"""
    kinds, reads = D.mixed_pool()
    assert {"exact100", "err100", "adna", "allN", "empty", "polyT", "tandem", "long250", "long300", "long600"} <= set(kinds)
    seq, rseq, off = T.encode_reads([(str(i), s, "I" * len(s)) for i, s in enumerate(reads)])[:3]
    for seq, rseq, off in ((seq, rseq, off), D.near_duplicates()):
        h = D.emu_hashes(emu, seq, rseq, off)
        by_hash = {}
        for key, x in zip(D.keys_of(seq, rseq, off), h):
            by_hash.setdefault(int(x), set()).add(key)
        assert all(len(v) == 1 for v in by_hash.values())
        assert len(by_hash) == D.n_distinct(seq, rseq, off)


def test_stand_alone_emulation_under_the_sanitizers(tmp_path):
    """the same bodies as a program of their own with -fsanitize=address,undefined: every buffer is exactly off[n] bytes, the last read ends at
    the buffers' end and its length runs over 0..33"""
    exe = str(tmp_path / "dedup_emu_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I" + D.EMU_DIR,
                    "-Wno-unknown-pragmas", "-DDEDUP_EMU_MAIN", os.path.join(D.EMU_DIR, "dedup_emu.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "578 cases, 0 failed" in r.stdout, r.stdout + r.stderr
