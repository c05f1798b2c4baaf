"""What the tests of the BAM coordinate sort (nabwa_bam_sort*, `nabwa_bam2bam --sort`) share: records made in Python, the NumPy oracle
(np.argsort(keys, kind="stable") over the records of the unsorted bytes), the CPU builds of csrc/bam_sort_body.hpp and
csrc/bam_sort_host.hpp under tests/emu/, and the fixed inputs of tests/test_gpu_bam_sort.py, so that tests/test_bam_sort_emu.py can run the
same inputs through the bodies without a GPU."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

import nabwa_testlib as T

EMU_DIR = os.path.join(T.ROOT, "tests", "emu")
CSRC = os.path.join(T.ROOT, "network-aware-bwa_amd", "csrc")
KEY_TIDS = (-1, 0, 1, 2 ** 31 - 1)
KEY_POSS = (-1, 0, 1, 2 ** 31 - 2)
COPY_SIZES = tuple(range(36, 53)) + (63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 70000)
N_RECS = (0, 1, 2, 63, 64, 65, 257, 70000)


def key_of(tid, pos):
    """NABWA_BAM_SORT_KEY, restated"""
    return ((tid & 0xffffffff) << 32) | ((pos + 1) & 0xffffffff)


def record(tid, pos, size, fill):
    """a record of `size` bytes (>= 36): block_size, refID, pos, then bytes that tell records apart"""
    assert size >= 36
    body = np.random.default_rng(fill).integers(0, 256, size - 12, dtype=np.uint8).tobytes()
    return struct.pack("<Iii", size - 4, tid, pos) + body


def join(recs):
    """records -> (bytes as a uint8 array, offsets)"""
    off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)
    return np.frombuffer(b"".join(recs), np.uint8), off


def keys_of(data, off):
    """the keys of the records of a stream, from its bytes"""
    n = len(off) - 1
    if n == 0:
        return np.zeros(0, np.uint64)
    idx = off[:-1, None] + np.arange(4, 12)[None, :]
    w = np.ascontiguousarray(data[idx]).view("<i4")                      # (n, 2): refID, pos
    return (w[:, 0].astype(np.int64).astype(np.uint64) & np.uint64(0xffffffff)) << np.uint64(32) | ((w[:, 1].astype(np.int64) + 1).astype(np.uint64) & np.uint64(0xffffffff))


def oracle(data, off):
    """-> (sorted bytes, their offsets, their keys): the stable sort of the records by key"""
    data, off = np.asarray(data, np.uint8), np.asarray(off, np.int64)
    keys = keys_of(data, off)
    order = np.argsort(keys, kind="stable")
    sizes = (off[1:] - off[:-1])[order]
    out_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    raw = data.tobytes()
    return b"".join(raw[off[i]:off[i + 1]] for i in order), out_off, keys[order]


def offsets_of(raw):
    """the offsets of the records of a record stream, from the block_size words"""
    off, q = [0], 0
    while q < len(raw):
        q += 4 + struct.unpack_from("<I", raw, q)[0]
        off.append(q)
    assert q == len(raw)
    return np.array(off, np.int64)


def assert_same_records(got, got_off, want, want_off, what=""):
    """record for record, as bytes"""
    assert list(got_off) == list(want_off), what
    if got != want:
        for j in range(len(want_off) - 1):
            assert got[want_off[j]:want_off[j + 1]] == want[want_off[j]:want_off[j + 1]], (what, "record", j)
    assert got == want, what


# ---------------------------------------------------------------------------------------------------------------- the fixed inputs
def mixed(n, seed=1, n_tid=5, n_pos=1000):
    """n records: sizes over every residue mod 16, keys with many ties, some unmapped (tid -1 with and without a pos) and some pos -1"""
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 256, 1 << 16, dtype=np.uint8).tobytes()        # the bodies are slices of one pool; 4 bytes of each say which record it is
    recs = []
    for i in range(n):
        size = 36 + int(rng.integers(0, 300)) if i % 16 else 36 + (i // 16) % 16 + 16 * int(rng.integers(0, 4))
        u = rng.random()
        tid = -1 if u < 0.1 else int(rng.integers(0, n_tid))
        pos = -1 if (u < 0.05 or 0.5 < u < 0.53) else int(rng.integers(0, n_pos))
        at = int(rng.integers(0, len(pool) - 400))
        recs.append(struct.pack("<IiiI", size - 4, tid, pos, i) + pool[at:at + size - 16])
    return recs


def with_lead(recs, lead):
    """a leading record of `lead` bytes (36..51) shifts everything behind it through another source alignment; its key sorts last"""
    return [record(-1, 2 ** 31 - 2, lead, 99)] + recs


def named_cases():
    """(name, records) of tests/test_gpu_bam_sort.py beyond the plain sizes"""
    out = []
    out.append(("all keys equal", [record(3, 77, 36 + (7 * i) % 100, i) for i in range(300)]))
    rng = np.random.default_rng(3)
    out.append(("1000 records on 3 keys", [record(int(k), 10 * int(k), 36 + int(s), i) for i, (k, s) in enumerate(zip(rng.integers(0, 3, 1000), rng.integers(0, 200, 1000)))]))
    out.append(("unmapped with and without a place, pos -1 on a real tid",
                [record(t, p, 40 + i % 33, i) for i, (t, p) in enumerate([(-1, -1), (0, 5), (-1, 100), (1, -1), (0, -1), (-1, -1), (1, 0), (-1, 100), (0, 5), (1, -1), (2 ** 31 - 1, 2 ** 31 - 2), (-1, 0)] * 9)]))
    short = mixed(200, seed=8)
    out.append(("one 70 000-byte record among short ones", short[:100] + [record(1, 500, 70000, 5)] + short[100:]))
    data, off = join(mixed(500, seed=9))
    s, so, _ = oracle(data, off)
    srt = [s[so[j]:so[j + 1]] for j in range(500)]
    out.append(("already sorted", srt))
    out.append(("reverse sorted", srt[::-1]))
    return out


# ---------------------------------------------------------------------------------------------------------------- the CPU builds
def _build(out, srcs, deps, flags):
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(s) for s in srcs + deps):
        return out
    subprocess.run(["g++", "-std=c++17", "-I" + EMU_DIR, "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas"] + flags + srcs + ["-o", out, "-lpthread"], check=True)
    return out


BODY = [os.path.join(CSRC, "bam_sort_body.hpp"), os.path.join(CSRC, "rec_body.hpp"), os.path.join(EMU_DIR, "emu_hip.hpp"), os.path.join(T.ROOT, "include", "nabwa.h")]


def load_emu():
    lib = C.CDLL(_build(os.path.join(EMU_DIR, "libbam_sort_emu.so"), [os.path.join(EMU_DIR, "bam_sort_emu.cpp")], BODY, ["-O2", "-fPIC", "-shared"]))
    P = C.c_void_p
    lib.emu_bsort_key.restype = C.c_uint64
    lib.emu_bsort_key.argtypes = [P]
    lib.emu_bsort_copy.restype = None
    lib.emu_bsort_copy.argtypes = [P, P, C.c_int64, C.c_int]
    lib.emu_bsort_run.restype = C.c_int64
    lib.emu_bsort_run.argtypes = [C.c_int64, P, P, P, P, P]
    return lib


def build_main():
    """the stand-alone program, under AddressSanitizer and UndefinedBehaviorSanitizer"""
    return _build(os.path.join(EMU_DIR, "bam_sort_main_asan"), [os.path.join(EMU_DIR, "bam_sort_main.cpp"), os.path.join(EMU_DIR, "bam_sort_emu.cpp")], BODY,
                  ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])


def build_host_main():
    """the host half of `nabwa_bam2bam --sort` (csrc/bam_sort_host.hpp) as a program"""
    return _build(os.path.join(EMU_DIR, "bam_sort_host_main"), [os.path.join(EMU_DIR, "bam_sort_host_main.cpp")], [os.path.join(CSRC, "bam_sort_host.hpp")], ["-O2"])


def build_header_main():
    return _build(os.path.join(EMU_DIR, "bam_header_main"), [os.path.join(EMU_DIR, "bam_header_main.cpp")], [os.path.join(CSRC, "bam_header.hpp")], ["-O1"])


def emu_run(emu, data, off):
    """the whole stage through the bodies on the CPU -> (bad, bytes, offsets, keys)"""
    data, off = np.ascontiguousarray(data, np.uint8), np.ascontiguousarray(off, np.int64)
    n = len(off) - 1
    out = np.zeros(max(len(data), 1), np.uint8)
    out_off, keys = np.zeros(n + 1, np.int64), np.zeros(max(n, 1), np.uint64)
    src = data if len(data) else np.zeros(1, np.uint8)
    bad = emu.emu_bsort_run(n, T.ptr(src), T.ptr(off), T.ptr(out), T.ptr(out_off), T.ptr(keys))
    return bad, out[:len(data)].tobytes(), out_off, keys[:n]
