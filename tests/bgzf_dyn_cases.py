"""What the tests of the BGZF compressor's dynamic mode share: the smallest inputs at which its new phases (histogram, length-limited
codes, coded lengths; csrc/bgzf_deflate_body.hpp) can go wrong, beside the cases of bgzf_cases.py, the histograms for the code builder
alone, the checks both the CPU and the GPU tests make, and the CPU build (tests/emu/bgzf_dyn_emu.cpp).  Test infrastructure only."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

import bgzf_cases as Z

SLICE = Z.SLICE


def fib(n):
    """F(1) .. F(n): 1, 1, 2, 3, ..."""
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def cases():
    """-> [(name, bytes)], built once per process"""
    global _CASES
    if _CASES is not None:
        return _CASES
    c = [("one_byte", b"Q")]                            # two literal/length codes of one bit, no distance used: both forced distance codes
    c.append(("one_distance", b"b" + b"a" * 300))       # every match has distance 1: distance symbol 0 and its forced neighbour
    c.append(("all_values_twice", bytes(range(256)) * 2))      # HLIT at its widest without symbol 285; long runs of equal lengths (16)
    f = fib(21)                                         # byte value i occurs F(i) times: 20 bits deep without the limit of 15
    a = np.repeat(np.arange(1, 22, dtype=np.uint8), f)
    assert a.size == 28656
    np.random.default_rng(1951).shuffle(a)
    c.append(("fibonacci", a.tobytes()))
    _CASES = c
    return c


_CASES = None


def all_cases():
    return Z.cases() + cases()


def histograms():
    """-> [(name, limit, [frequency])] for the code builder alone.  A frequency is a 32-bit word, so Fibonacci numbers past it are cut
    to the largest word (the builder's sums saturate)"""
    top = 0xffffffff
    h = [("fib286", 15, [min(x, top) for x in fib(286)]), ("fib30", 15, fib(30)), ("fib19", 7, fib(19))]
    for n, limit in ((286, 15), (30, 15), (19, 7)):
        h.append(("single%d" % n, limit, [0] * (n - 1) + [5]))
        h.append(("single_first%d" % n, limit, [7] + [0] * (n - 1)))
        h.append(("two%d" % n, limit, [0, 3] + [0] * (n - 3) + [1000]))
        h.append(("equal%d" % n, limit, [9] * n))
        h.append(("none%d" % n, limit, [0] * n))
    return h


def check_lengths(freq, limit, lens):
    """what every code the builder returns must be"""
    n = len(freq)
    assert len(lens) == n and max(lens) <= limit
    used = [s for s in range(n) if freq[s]]
    coded = [s for s in range(n) if lens[s]]
    assert sum(1 << (limit - lens[s]) for s in coded) == 1 << limit, "Kraft sum is not 1"
    assert len(coded) >= 2
    assert set(used) <= set(coded)
    if len(used) >= 2:
        assert coded == used, "a symbol that does not occur has a code"
    else:
        assert len(coded) == 2 and all(lens[s] == 1 for s in coded)
    for a in used:
        for b in used:
            if freq[a] > freq[b]:
                assert lens[a] <= lens[b], "symbol %d (%d times) has a longer code than %d (%d times)" % (a, freq[a], b, freq[b])


def blocks(out):
    """-> the blocks of a BGZF stream"""
    out, p, r = bytes(out), 0, []
    while p < len(out):
        size = struct.unpack_from("<H", out, p + 16)[0] + 1
        r.append(out[p:p + size])
        p += size
    return r


def btype(block):
    return (block[18] >> 1) & 3


def check_pair(name, data, dyn, fixed):
    """the dynamic mode's stream against the fixed mode's of the same tokens"""
    sd, sf = Z.walk(dyn, data), Z.walk(fixed, data)
    assert len(sd) == len(sf)
    for k, (a, b) in enumerate(zip(sd, sf)):
        assert a <= b, "%s block %d: dynamic mode %d bytes, fixed mode %d" % (name, k, a, b)
    if name in ("len1", "len2", "len3", "len4"):
        assert dyn == fixed                             # a dynamic header alone is more than 29 bits; these payloads are at most 6 bytes
    if name == "random":
        assert sd == [SLICE + 31]
    if name in ("text", "bam"):
        assert sum(sd) < sum(sf)
        assert any(btype(b) == 2 for b in blocks(dyn)), "%s: no block of BTYPE 10" % name


EMU_SRC = [os.path.join(Z.EMU_DIR, "bgzf_dyn_emu.cpp"), os.path.join(Z.CSRC, "bgzf_deflate_body.hpp")]


def _stale(out, srcs):
    return not os.path.exists(out) or any(os.path.getmtime(out) < os.path.getmtime(s) for s in srcs)


def build_emu():
    out = os.path.join(Z.EMU_DIR, "libbgzf_dyn_emu.so")
    if _stale(out, EMU_SRC):
        subprocess.run(["g++", "-std=c++17", "-fPIC", "-shared", "-I" + Z.CSRC, "-Wall", "-Wno-unused-function", "-O2", EMU_SRC[0], "-o", out], check=True)
    return out


def build_main_sanitized():
    """the stand-alone program under AddressSanitizer and UBSan"""
    out = os.path.join(Z.EMU_DIR, "bgzf_dyn_main_asan")
    main = os.path.join(Z.EMU_DIR, "bgzf_dyn_main.cpp")
    if _stale(out, EMU_SRC + [main]):
        subprocess.run(["g++", "-std=c++17", "-I" + Z.CSRC, "-Wall", "-Wno-unused-function", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", main, EMU_SRC[0], "-o", out], check=True)
    return out


def emu_compress(lib, data, order=0):
    """the dynamic mode's phases on the CPU; order: the lanes run 0 first-to-last, 1 last-to-first, 2 interleaved"""
    lib.emu_bgzf_dyn.restype = C.c_long
    lib.emu_bgzf_dyn.argtypes = [C.c_char_p, C.c_long, C.c_void_p, C.c_int]
    out = C.create_string_buffer(max((len(data) + SLICE - 1) // SLICE * 0x10000, 1))
    n = lib.emu_bgzf_dyn(bytes(data), len(data), out, order)
    assert n >= 0, "a block's size is not what its header phase said"
    return out.raw[:n]


def emu_code_lengths(lib, freq, limit):
    lib.emu_bgzf_code_lengths.restype = C.c_int
    lib.emu_bgzf_code_lengths.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    f = (C.c_uint32 * len(freq))(*freq)
    out = C.create_string_buffer(len(freq))
    assert lib.emu_bgzf_code_lengths(f, len(freq), limit, out) == 0
    return list(out.raw)
