"""The bodies of the cross-batch read cache (csrc/dedup_cache_body.hpp; NABWA_DEDUP_CACHE) on the CPU (tests/emu/dedup_cache_emu.cpp): the probe
order and its bound, how an entry lies in the arena, the exact comparison of a read with an entry, and a full table and a full arena.  Nothing
here needs a GPU, and nothing is preloaded into Python: the sanitizer run is a program of its own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dedup_cases as D
import nabwa_testlib as T

SRC = os.path.join(D.EMU_DIR, "dedup_cache_emu.cpp")
DEPS = [SRC, os.path.join(D.EMU_DIR, "emu_hip.hpp"), os.path.join(D.CSRC, "dedup_body.hpp"), os.path.join(D.CSRC, "dedup_cache_body.hpp")]
LENS = list(range(0, 41)) + [63, 64, 65, 257]
HDR, FULL64 = 32, (1 << 64) - 1
DC_BUMP, DC_USED, DC_ENTRIES, DC_FULL, DC_SKIPPED = range(5)


@pytest.fixture(scope="module")
def emu():
    out = os.path.join(D.EMU_DIR, "libdedup_cache_emu.so")
    if not (os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(s) for s in DEPS)):
        subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + D.EMU_DIR, "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", SRC, "-o", out], check=True)
    lib = C.CDLL(out)
    P = C.c_void_p
    lib.emu_dcache_entry_size.restype = C.c_uint32
    lib.emu_dcache_entry_size.argtypes = [C.c_int, C.c_int]
    lib.emu_dcache_slot_index.restype = C.c_uint64
    lib.emu_dcache_slot_index.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_int]
    lib.emu_dcache_hash.restype = C.c_uint64
    lib.emu_dcache_hash.argtypes = [P, P, C.c_int64, C.c_int]
    lib.emu_dcache_insert.restype = C.c_longlong
    lib.emu_dcache_insert.argtypes = [P, C.c_uint32, P, C.c_uint64, P, C.c_uint64, P, P, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P, C.c_int]
    lib.emu_dcache_lookup.restype = C.c_longlong
    lib.emu_dcache_lookup.argtypes = [P, C.c_uint32, P, C.c_uint64, P, P, C.c_int64, C.c_int, C.c_int, C.c_int, P]
    lib.emu_dcache_entry.argtypes = [P, C.c_longlong, P, P, P]
    return lib


class Cache:
    def __init__(self, emu, n_slots, arena_bytes, mask=FULL64):
        self.emu, self.n_slots, self.mask = emu, n_slots, mask
        self.slots = np.zeros(n_slots, np.uint64)
        self.arena = np.full(max(arena_bytes, 1), 0xAB, np.uint8)
        self.arena_bytes = arena_bytes
        self.ctr = np.zeros(8, np.uint64)

    def insert(self, s, r, md=3, mg=1, rows=None, maxe=7, row_cap=64, o=0, L=None):
        rows = np.zeros((0, 4), np.uint32) if rows is None else rows
        buf = np.ascontiguousarray(rows if len(rows) else np.zeros((1, 4), np.uint32), np.uint32)
        return self.emu.emu_dcache_insert(T.ptr(self.slots), self.n_slots, T.ptr(self.arena), self.arena_bytes, T.ptr(self.ctr), self.mask, T.ptr(s), T.ptr(r), o,
                                          len(s) - o if L is None else L, md, mg, len(rows), maxe, T.ptr(buf), row_cap)

    def lookup(self, s, r, md=3, mg=1, o=0, L=None):
        nc = C.c_int()
        w = self.emu.emu_dcache_lookup(T.ptr(self.slots), self.n_slots, T.ptr(self.arena), self.mask, T.ptr(s), T.ptr(r), o, len(s) - o if L is None else L, md, mg, C.byref(nc))
        return w, nc.value


def rand_read(rng, L):
    """(seq, rseq), never of size 0 as arrays: the bodies touch none of a length-0 read's bytes, numpy needs one to point at"""
    return rng.integers(0, 5, max(L, 1)).astype(np.uint8), rng.integers(0, 5, max(L, 1)).astype(np.uint8)


def test_probe_order_and_bound(emu):
    """probe p of a hash looks at slot (hash & mask) + p modulo the table, p < 16; with mask 0 every read starts at slot 0"""
    assert emu.emu_dcache_probes() == 16
    rng = np.random.default_rng(1)
    for n_slots in (1024, 16384):
        for h in [0, FULL64, n_slots - 3] + [int(x) for x in rng.integers(0, 1 << 63, 50)]:
            for mask in (FULL64, 0, 1, 15):
                assert [emu.emu_dcache_slot_index(h, mask, n_slots, p) for p in range(16)] == [((h & mask) + p) % n_slots for p in range(16)]


@pytest.mark.parametrize("L", LENS)
def test_entry_layout(emu, L):
    """header, both strands padded with zero bytes to whole 16-byte chunks, the rows; entries lie back to back on 16-byte boundaries"""
    rng = np.random.default_rng(100 + L)
    c = Cache(emu, 1024, 1 << 16)
    at = 0
    for k, n_rows in enumerate((0, 1, 5)):
        s, r = rand_read(rng, L)
        s[0] = k                                                       # three different reads, however short
        rows = rng.integers(0, 1 << 32, (n_rows, 4), dtype=np.uint64).astype(np.uint32)
        pl = (L + 15) // 16 * 16
        size = HDR + 2 * pl + 16 * n_rows
        assert emu.emu_dcache_entry_size(L, n_rows) == size
        w = c.insert(s, r, md=4, mg=2, rows=rows, maxe=1234 + n_rows, L=L)
        assert w == at and w % 16 == 0
        e = c.arena[w:w + size]
        h = emu.emu_dcache_hash(T.ptr(s), T.ptr(r), 0, L)
        assert int(e[0:8].view(np.uint64)[0]) == h and int(e[8:12].view(np.uint32)[0]) == L
        assert (int(e[12]), int(e[13]), int(e[14]), int(e[15])) == (4, 2, 0, 0)
        assert e[16:32].view(np.int32).tolist() == [n_rows, 1234 + n_rows, HDR + 2 * pl, size]
        assert e[HDR:HDR + L].tobytes() == s[:L].tobytes() and not e[HDR + L:HDR + pl].any()
        assert e[HDR + pl:HDR + pl + L].tobytes() == r[:L].tobytes() and not e[HDR + pl + L:HDR + 2 * pl].any()
        assert e[HDR + 2 * pl:].tobytes() == rows.tobytes()
        assert (c.arena[w + size:] == 0xAB).all()                      # nothing beyond the entry
        at += size
        n_aln, maxe = C.c_int32(), C.c_int32()
        got = np.zeros((max(n_rows, 1), 4), np.uint32)
        emu.emu_dcache_entry(T.ptr(c.arena), w, C.byref(n_aln), C.byref(maxe), T.ptr(got))
        assert (n_aln.value, maxe.value) == (n_rows, 1234 + n_rows) and got[:n_rows].tobytes() == rows.tobytes()
        assert c.lookup(s, r, md=4, mg=2, L=L)[0] == (w if L else 0)      # (empty reads are one read: the first entry answers)
    assert c.ctr[DC_USED] == at and c.ctr[DC_ENTRIES] == 3 and c.ctr[DC_BUMP] == at


def test_comparison_is_exact_at_every_byte_offset(emu):
    """a read is found wherever it lies (start 0..16 within the buffer); a change of any single byte of either strand, of the length by one, of
    max_diff or of max_gapo is not"""
    rng = np.random.default_rng(3)
    for L in [1, 2, 15, 16, 17, 31, 32, 33, 40, 63, 64, 65, 257]:
        s, r = rand_read(rng, L)
        c = Cache(emu, 1024, 1 << 14)
        w = c.insert(s, r)
        assert w == 0
        for shift in range(17):
            js, jr = rand_read(rng, shift)
            s2 = np.concatenate([js[:shift], s, [0]]).astype(np.uint8); r2 = np.concatenate([jr[:shift], r, [4]]).astype(np.uint8)
            assert c.lookup(s2, r2, o=shift, L=L) == (0, 1)
            assert c.lookup(s2, r2, o=shift, L=L + 1)[0] == -1 and c.lookup(s2, r2, o=shift, L=L - 1)[0] == -1
        assert c.lookup(s, r, md=2)[0] == -1 and c.lookup(s, r, mg=0)[0] == -1
        for strand in (0, 1):
            for k in range(L):
                x = [s.copy(), r.copy()]
                x[strand][k] = (x[strand][k] + 1 + k % 4) % 5
                assert c.lookup(x[0], x[1])[0] == -1, (L, strand, k)


def test_one_chain_fills_to_the_probe_bound_and_refuses_cleanly(emu):
    """mask 0: every read probes slots 0..15.  Sixteen reads enter, the seventeenth is refused and counted, nothing of it is written; all
    sixteen are still found, the last after sixteen comparisons' worth of probing"""
    rng = np.random.default_rng(4)
    c = Cache(emu, 1024, 1 << 16, mask=0)
    reads = [rand_read(rng, 50) for _ in range(20)]
    for i, (s, r) in enumerate(reads):
        w = c.insert(s, r)
        assert (w >= 0) == (i < 16), i
    assert c.ctr[DC_ENTRIES] == 16 and c.ctr[DC_FULL] == 4 and c.ctr[DC_USED] == c.ctr[DC_BUMP] == 16 * emu.emu_dcache_entry_size(50, 0)
    assert np.count_nonzero(c.slots) == 16 and c.slots[:16].all()
    for i, (s, r) in enumerate(reads):
        w, n_cand = c.lookup(s, r)
        assert (w >= 0) == (i < 16) and n_cand <= 16
    # with all 64 bits the same reads spread over the table
    c = Cache(emu, 1024, 1 << 16)
    assert all(c.insert(s, r) >= 0 for s, r in reads) and c.ctr[DC_FULL] == 0


def test_full_arena_refuses_cleanly_and_lookups_go_on(emu):
    """an arena of exactly three entries: the fourth read is refused, takes no slot and leaves the counters' used bytes alone"""
    rng = np.random.default_rng(5)
    size = emu.emu_dcache_entry_size(100, 2)
    c = Cache(emu, 1024, 3 * size)
    rows = rng.integers(0, 1 << 32, (2, 4), dtype=np.uint64).astype(np.uint32)
    reads = [rand_read(rng, 100) for _ in range(5)]
    got = [c.insert(s, r, rows=rows) for s, r in reads]
    assert got == [0, size, 2 * size, -1, -1]
    assert c.ctr[DC_USED] == 3 * size and c.ctr[DC_ENTRIES] == 3 and c.ctr[DC_FULL] == 2 and np.count_nonzero(c.slots) == 3
    assert [c.lookup(s, r)[0] for s, r in reads] == [0, size, 2 * size, -1, -1]
    # a read over the row cap is not entered and is counted apart
    c = Cache(emu, 1024, 1 << 16)
    s, r = reads[0]
    assert c.insert(s, r, rows=rows, row_cap=1) == -1 and c.ctr[DC_SKIPPED] == 1 and c.ctr[DC_FULL] == 0 and not c.slots.any()


def test_stand_alone_emulation_under_the_sanitizers(tmp_path):
    """lookup and insert as a program of their own with -fsanitize=address,undefined: table, arena and reads are heap blocks of exactly their
    bytes, and the last entry ends where the arena ends"""
    exe = str(tmp_path / "dedup_cache_emu_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I" + D.EMU_DIR,
                    "-Wno-unknown-pragmas", "-DDCACHE_EMU_MAIN", SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "306 cases, 0 failed" in r.stdout, r.stdout + r.stderr
