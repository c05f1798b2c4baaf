"""Shared helpers of the finishing-kernel tests (test_finish_emu.py, test_gpu_finish.py): the fixture tests/golden/vectors_refine.npz
(made by tests/golden/make_golden_refine.py from the compiled reference's bwa_refine_gapped) and the CPU emulation of the kernel bodies
(tests/emu/finish_emu.cpp).  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

import nabwa_testlib as T

EMU_DIR = os.path.join(T.ROOT, "tests", "emu")
CSRC = os.path.join(T.ROOT, "network-aware-bwa_amd", "csrc")
L_PAC = 103000
HOLES = (np.array([45000, 52000, 90000], np.int64), np.array([200, 3, 1], np.int32), b"NNN")
MAQ = np.array([11, -19, -19, -19, -13, -19, 11, -19, -19, -13, -19, -19, 11, -19, -13, -19, -19, -19, 11, -13, -13, -13, -13, -13, -13], np.int32)


class Case:
    """one positioned hit of the fixture and what the reference made of it"""

    def __init__(self, v, i):
        a, b = int(v["off"][i]), int(v["off"][i + 1])
        self.seq, self.rseq = v["seq"][a:b].copy(), v["rseq"][a:b].copy()
        self.len = b - a
        self.strand = int(v["strand"][i])
        self.gaps = int(v["n_gapo"][i]) + int(v["n_gape"][i])
        self.gapped = int(v["n_gapo"][i]) > 0
        self.ext = (1 if self.strand else -1) * self.gaps
        self.pos = int(v["pos"][i])
        self.tag = str(v["tag"][i])
        self.query = self.rseq if self.strand else self.seq[::-1].copy()      # alignment orientation
        self.pos_out = int(v["pos_out"][i])
        self.cigar = v["cigar"][i, :int(v["n_cigar"][i])].copy()
        self.nm = int(v["nm"][i])
        self.md = bytes(v["md"][int(v["md_off"][i]):int(v["md_off"][i + 1]) - 1]).decode()


_cases = None


def cases():
    global _cases
    if _cases is None:
        v = np.load(os.path.join(T.GOLDEN, "vectors_refine.npz"))
        _cases = [Case(v, i) for i in range(len(v["off"]) - 1)]
    return _cases


def build_emu():
    out = os.path.join(EMU_DIR, "libfinish_emu.so")
    srcs = [os.path.join(EMU_DIR, "finish_emu.cpp"), os.path.join(EMU_DIR, "emu_hip.hpp"), os.path.join(CSRC, "finish_body.hpp"), os.path.join(CSRC, "wave_spmd.hpp")]
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(s) for s in srcs):
        return out
    subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-I" + EMU_DIR, "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", srcs[0], "-o", out],
                   check=True)
    return out


def load_emu():
    lib = C.CDLL(build_emu())
    P = C.c_void_p
    lib.emu_fin_extent.restype = None
    lib.emu_fin_extent.argtypes = [C.c_int64, C.c_uint32, C.c_int, C.c_int, C.c_int, P, P, P]
    lib.emu_fin_window.restype = None
    lib.emu_fin_window.argtypes = [P, C.c_int64, C.c_int64, C.c_int, P, P, C.c_int, C.c_int, P, P]
    lib.emu_fin_cigar.restype = C.c_int
    lib.emu_fin_cigar.argtypes = [P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, P, P]
    lib.emu_fin_md.restype = C.c_int
    lib.emu_fin_md.argtypes = [P, C.c_int64, C.c_int, P, P, C.c_char_p, P, P, C.c_int, C.c_int, C.c_uint32, C.c_int, P, C.c_char_p, C.c_int, P]
    return lib


def toy_pac():
    return np.fromfile(T.TOY + ".pac", np.uint8)


def emu_refine(emu, olib, pac, seq, rseq, strand, ext, pos, gapped, max_cigar=64):
    """bwa_refine_gapped of one hit through the emulated bodies: window -> orc_global -> CIGAR rules -> MD.  -> (pos, cigar, nm, md)"""
    n = len(seq)
    cig = np.zeros(0, np.uint16)
    if gapped:
        ps, lo, wn = C.c_int64(0), C.c_int64(0), C.c_int(0)
        emu.emu_fin_extent(L_PAC, pos, n, ext, 1, C.byref(ps), C.byref(lo), C.byref(wn))
        assert wn.value > 0
        win = np.zeros(wn.value, np.uint8)
        qry = np.zeros(n, np.uint8)
        emu.emu_fin_window(T.ptr(pac), L_PAC, lo.value, wn.value, T.ptr(seq), T.ptr(rseq), n, 1 if strand else 0, T.ptr(win), T.ptr(qry))
        c32 = np.zeros(wn.value + n + 2, np.uint32)
        nc = C.c_int(0)
        olib.orc_global(T.ptr(win), wn.value, T.ptr(qry), n, 26, 9, 5, T.ptr(MAQ), 5, 50, T.ptr(c32), C.byref(nc))
        row = np.zeros(max_cigar, np.uint16)
        po = C.c_uint32(0)
        m = emu.emu_fin_cigar(T.ptr(c32), nc.value, max_cigar, ext, 1, ps.value, T.ptr(row), C.byref(po))
        assert m >= 1
        cig, pos = row[:m].copy(), po.value
    md = C.create_string_buffer(4096)
    nm = C.c_int32(0)
    r = emu.emu_fin_md(T.ptr(pac), L_PAC, 3, T.ptr(HOLES[0]), T.ptr(HOLES[1]), HOLES[2], T.ptr(seq), T.ptr(rseq), n, 1 if strand else 0, pos, len(cig),
                       T.ptr(cig) if len(cig) else None, md, 4096, C.byref(nm))
    assert r >= 0, r
    return pos, cig, nm.value, md.value.decode()
