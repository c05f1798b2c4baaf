"""What the BGZF compressor's tests share: the walk over a stream of BGZF blocks that checks each of them, the inputs (the smallest
at which each rule of the format can break), and the CPU build of the kernel body (tests/emu/bgzf_emu.cpp).  Test infrastructure only."""
import ctypes as C
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np

import bamlib as B
import nabwa_testlib as T

SLICE = 0xff00
HEADER = bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0])
EOF_BLOCK = HEADER + bytes([27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def walk(out, data):
    """every block of `out` against its slice of `data`; -> the blocks' sizes"""
    out, data = bytes(out), bytes(data)
    sizes, p, k = [], 0, 0
    while p < len(out):
        assert out[p:p + 16] == HEADER, "block %d: header" % k
        size = struct.unpack_from("<H", out, p + 16)[0] + 1
        assert p + size <= len(out), "block %d runs past the end" % k
        assert size <= 0x10000
        want = data[k * SLICE:(k + 1) * SLICE]
        assert len(want) > 0, "more blocks than slices"
        assert size <= len(want) + 31, "block %d is larger than its slice stored" % k
        assert struct.unpack_from("<I", out, p + size - 4)[0] == len(want), "block %d: ISIZE" % k
        assert zlib.decompress(out[p:p + size], 31) == want, "block %d inflates to other bytes" % k      # zlib checks CRC-32 and ISIZE
        sizes.append(size)
        p += size
        k += 1
    assert p == len(out) and k == (len(data) + SLICE - 1) // SLICE
    assert (gzip.decompress(out) if out else b"") == data
    return sizes


def text_like(n, seed):
    """words of a small vocabulary with numbers between them: literals and matches of many lengths and distances"""
    rng = np.random.default_rng(seed)
    vocab = [bytes(rng.integers(97, 123, rng.integers(2, 12)).astype(np.uint8)) for _ in range(300)]
    parts, size = [], 0
    while size < n:
        w = vocab[int(rng.integers(0, 300))] + (b" %d\t" % rng.integers(0, 100000) if rng.random() < 0.2 else b" ")
        parts.append(w)
        size += len(w)
    return b"".join(parts)[:n]


def golden_bam_bytes():
    """the records of the golden single-end reads as they stand in a BAM stream, repeated to a little more than two slices.  No BAM file
    is committed under tests/golden/, so the records are made from reads_se.fq (bamlib.make_record): records only, without the BAM
    header and the reference dictionary, which the tool's runs in tests/test_gpu_bgzf_cli.py send through the compressor."""
    reads = T.read_fastq(os.path.join(T.GOLDEN, "reads_se.fq"))
    raw = b"".join(B.make_record(n, s, q, 4) for n, s, q in reads)
    while len(raw) <= 2 * SLICE:
        raw += raw
    return raw[:2 * SLICE + 1234]


def cases():
    """-> [(name, bytes)], built once per process"""
    global _CASES
    if _CASES is not None:
        return _CASES
    rng = np.random.default_rng(20260)
    c = [("len%d" % n, bytes(range(65, 65 + n))) for n in (0, 1, 2, 3, 4)]
    c += [("run%d" % n, b"a" * n) for n in (257, 258, 259, 600)]
    c += [("text%s" % nm, text_like(n, 7)) for nm, n in (("-1", SLICE - 1), ("", SLICE), ("+1", SLICE + 1), ("x3+17", 3 * SLICE + 17))]
    c.append(("random", rng.integers(0, 256, SLICE).astype(np.uint8).tobytes()))
    c.append(("128values", rng.integers(0, 128, SLICE).astype(np.uint8).tobytes()))
    half = rng.integers(0, 256, 32768).astype(np.uint8).tobytes()
    c.append(("dist32768", (half + half)[:40000]))
    c.append(("dist32769", (half + b"\x00" + half)[:40000]))
    fresh = rng.permutation(np.arange(3, 256)).astype(np.uint8)
    c.append(("matches3", b"".join(b"\x00\x01\x02" + bytes([int(x)]) for x in fresh) * 3))
    c.append(("allff", b"\xff" * 70000))
    c.append(("bam", golden_bam_bytes()))
    _CASES = c
    return c


_CASES = None

EMU_DIR = os.path.join(T.ROOT, "tests", "emu")
CSRC = os.path.join(T.ROOT, "network-aware-bwa_amd", "csrc")


def build_emu(asan=False):
    out = os.path.join(EMU_DIR, "libbgzf_emu_asan.so" if asan else "libbgzf_emu.so")
    srcs = [os.path.join(EMU_DIR, "bgzf_emu.cpp"), os.path.join(CSRC, "bgzf_deflate_body.hpp")]
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(s) for s in srcs):
        return out
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] if asan else ["-O2"]
    subprocess.run(["g++", "-std=c++17", "-fPIC", "-shared", "-I" + CSRC, "-Wall", "-Wno-unused-function"] + flags + [srcs[0], "-o", out], check=True)
    return out


def emu_compress(lib, data, order=0):
    """the kernel body on the CPU; order: the lanes of the parse phase run 0 first-to-last, 1 last-to-first, 2 interleaved"""
    lib.emu_bgzf.restype = C.c_long
    lib.emu_bgzf.argtypes = [C.c_char_p, C.c_long, C.c_void_p, C.c_int]
    out = C.create_string_buffer(max((len(data) + SLICE - 1) // SLICE * 0x10000, 1))
    n = lib.emu_bgzf(bytes(data), len(data), out, order)
    return out.raw[:n]
