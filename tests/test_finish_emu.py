"""The bodies of the finishing kernels (csrc/finish_body.hpp) on the CPU: the window, CIGAR and MD bodies run as loops over the lanes of
one wavefront (tests/emu/finish_emu.cpp) and must give what the reference's bwa_refine_gapped gave -- on every case of the fixture
tests/golden/vectors_refine.npz, and, where the compiled reference is at hand, on fresh seeded cases.  The alignment between window and
CIGAR comes from the oracle's orc_global."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import finish_cases as F
import nabwa_testlib as T


@pytest.fixture(scope="module")
def env():
    return F.load_emu(), T.load_oracle(), F.toy_pac()


def test_fixture_covers_what_it_promises():
    cs = F.cases()
    assert 200 <= len(cs) <= 600 and os.path.getsize(os.path.join(T.GOLDEN, "vectors_refine.npz")) < 200 * 1024
    assert {c.len for c in cs} >= {17, 63, 64, 65, 100, 150, 257}
    gapped = [c for c in cs if c.gapped]
    # every pac phase of the window's first base on both strands
    emu = F.load_emu()
    seen = set()
    for c in gapped:
        ps, lo, wn = C.c_int64(0), C.c_int64(0), C.c_int(0)
        emu.emu_fin_extent(F.L_PAC, c.pos, c.len, c.ext, 1, C.byref(ps), C.byref(lo), C.byref(wn))
        assert wn.value > 0
        seen.add((c.strand, lo.value & 3))
    assert seen == {(s, p) for s in (0, 1) for p in range(4)}
    assert any(c.pos == 0xfffffffe and c.strand == 0 for c in gapped)
    assert all(c.pos + c.len <= F.L_PAC for c in cs if not c.gapped)
    assert any("^N" in c.md for c in cs) and any(c.md.startswith("0") and len(c.md) > 1 for c in cs)
    assert any(c.cigar[0] >> 14 == 3 for c in gapped) and any(c.cigar[-1] >> 14 == 3 for c in gapped)      # an end I became S
    assert any(4 in c.query for c in cs)


def test_every_fixture_case_through_the_emulated_bodies(env):
    emu, olib, pac = env
    bad = []
    for i, c in enumerate(F.cases()):
        pos, cig, nm, md = F.emu_refine(emu, olib, pac, c.seq, c.rseq, c.strand, c.ext, c.pos, c.gapped)
        if not (pos == c.pos_out and cig.tolist() == c.cigar.tolist() and nm == c.nm and md == c.md):
            bad.append((i, c.tag, pos, c.pos_out, T.cigar16_str(cig), T.cigar16_str(c.cigar), nm, c.nm, md, c.md))
    assert not bad, bad[:5]


def test_window_body_matches_a_base_by_base_walk(env):
    """windows over 256 bases (more than one round of the lanes), every phase, both ends of the text"""
    emu, _, pac = env
    k = np.arange(F.L_PAC)
    base = (pac[k >> 2] >> ((~k & 3) << 1) & 3).astype(np.uint8)
    rng = np.random.default_rng(5)
    for lo, wn in [(0, 1), (1, 2), (2, 3), (3, 5), (0, 256), (1, 257), (5, 700), (F.L_PAC - 1, 1), (F.L_PAC - 263, 263), (F.L_PAC - 1030, 1030)]:
        n = 70
        seq = rng.integers(0, 5, n).astype(np.uint8)
        rseq = rng.integers(0, 5, n).astype(np.uint8)
        for copy in (0, 1):
            win = np.full(wn, 9, np.uint8)
            qry = np.full(n, 9, np.uint8)
            emu.emu_fin_window(T.ptr(pac), F.L_PAC, lo, wn, T.ptr(seq), T.ptr(rseq), n, copy, T.ptr(win), T.ptr(qry))
            assert win.tolist() == base[lo:lo + wn].tolist()
            assert qry.tolist() == (rseq if copy else seq[::-1]).tolist()


def test_cigar_body_flags_paths_that_do_not_fit(env):
    emu = env[0]
    c32 = np.array([5 << 4 | 0, 1 << 4 | 1, 5 << 4 | 0], np.uint32)
    row = np.zeros(8, np.uint16)
    po = C.c_uint32(0)
    assert emu.emu_fin_cigar(T.ptr(c32), 3, 8, 1, 1, 10, T.ptr(row), C.byref(po)) == 3 and po.value == 10
    assert emu.emu_fin_cigar(T.ptr(c32), 3, 2, 1, 1, 10, T.ptr(row), C.byref(po)) == -1
    assert emu.emu_fin_cigar(T.ptr(c32), 0, 8, 1, 1, 10, T.ptr(row), C.byref(po)) == -1


def test_fresh_cases_against_the_compiled_reference(env):
    """about 2000 seeded hits with random edits through the emulated bodies and through ref_refine_one"""
    ref = T.load_ref()
    if ref is None:
        pytest.skip("oracle/_ref/libbwaref.so is not built")
    emu, olib, pac = env
    rix = C.c_void_p(ref.ref_index_load(T.TOY.encode(), 1))
    ref.ref_refine_one.restype = None
    ref.ref_refine_one.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_uint32] + [C.c_void_p] * 5 + [C.c_int]
    k = np.arange(F.L_PAC)
    base = (pac[k >> 2] >> ((~k & 3) << 1) & 3).astype(np.uint8)
    rng = np.random.default_rng(77)
    n_run = 0
    for it in range(2000):
        n = int(rng.choice([17, 35, 63, 64, 65, 100, 129, 257]))
        strand = int(rng.integers(0, 2))
        near = int(rng.integers(0, 6))
        p = [int(rng.integers(0, F.L_PAC - n - 8)), int(rng.integers(44900, 45250)), int(rng.integers(51900, 52010)), int(rng.integers(89900, 90005)),
             int(rng.integers(0, 6)), F.L_PAC - n - 8 + int(rng.integers(0, 4))][near]
        gaps = int(rng.choice([0, 0, 1, 1, 2, 3]))
        kind = int(rng.integers(0, 2))                                     # 0: insertion, 1: deletion
        at = int(rng.integers(1, n - 1))
        q = []
        g = p
        while len(q) < n:
            if gaps and len(q) == at:
                if kind:
                    g += gaps
                else:
                    q.extend(int(x) for x in rng.integers(0, 4, min(gaps, n - len(q))))
                    at = -1
                    continue
            q.append(int(base[g]) if g < F.L_PAC else 0)
            g += 1
        q = np.array(q[:n], np.uint8)
        for _ in range(int(rng.integers(0, 4))):
            j = int(rng.integers(0, n))
            q[j] = (q[j] + 1 + int(rng.integers(0, 4))) % 5 if rng.integers(0, 8) else 4
        used = g - p
        pos = (p if strand else p + used - n) & 0xffffffff
        if not gaps and pos + n > F.L_PAC:
            continue
        if strand:
            rseq, seq = q, np.where(q < 4, 3 - q, q).astype(np.uint8)
        else:
            seq = q[::-1].copy()
            rseq = np.where(seq < 4, 3 - seq, seq).astype(np.uint8)
        ext = (1 if strand else -1) * gaps
        if gaps:
            ps, lo, wn = C.c_int64(0), C.c_int64(0), C.c_int(0)
            emu.emu_fin_extent(F.L_PAC, pos, n, ext, 1, C.byref(ps), C.byref(lo), C.byref(wn))
            if wn.value == 0:
                continue
        po, nc, nmv = C.c_uint32(0), C.c_int(0), C.c_int(0)
        row = np.zeros(512, np.uint16)
        md = C.create_string_buffer(4096)
        ref.ref_refine_one(rix, n, T.ptr(seq), T.ptr(rseq), 1, strand, 0, 1 if gaps else 0, max(gaps - 1, 0), pos,
                           C.byref(po), C.byref(nc), T.ptr(row), C.byref(nmv), md, 4096)
        got = F.emu_refine(emu, olib, pac, seq, rseq, strand, ext, pos, gaps > 0)
        assert (got[0], got[1].tolist(), got[2], got[3]) == (po.value, row[:nc.value].tolist(), nmv.value, md.value.decode()), (it, n, strand, p, gaps, kind)
        n_run += 1
    assert n_run > 1500


def test_stand_alone_emulation_under_the_sanitizers(tmp_path):
    """the same bodies as a program of their own with -fsanitize=address,undefined: every buffer has exactly the size the kernel may touch"""
    exe = str(tmp_path / "finish_emu_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I" + F.EMU_DIR,
                    "-DFINISH_EMU_MAIN", os.path.join(F.EMU_DIR, "finish_emu.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "0 failed" in r.stdout, r.stdout + r.stderr
