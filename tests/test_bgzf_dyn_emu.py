"""The BGZF compressor's dynamic mode (the phases of bgzf_deflate_dyn_kernel, csrc/bgzf_deflate_body.hpp) on the CPU: the phases
between the kernel's barriers run as loops over the lanes in three orders (tests/emu/bgzf_dyn_emu.cpp), every block goes through
zlib, and the blocks are held against the fixed mode's of the same tokens.  The code builder is checked on its own.  The same cases
run once more in a stand-alone program under AddressSanitizer and UBSan (tests/emu/bgzf_dyn_main.cpp)."""
import ctypes as C
import struct
import subprocess

import pytest

import bgzf_cases as Z
import bgzf_dyn_cases as D


@pytest.fixture(scope="module")
def emu():
    return C.CDLL(D.build_emu())


@pytest.fixture(scope="module")
def fixed_emu():
    return C.CDLL(Z.build_emu())


@pytest.mark.parametrize("name", [n for n, _ in D.all_cases()])
def test_blocks_inflate_and_are_no_larger_than_fixed(emu, fixed_emu, name):
    data = dict(D.all_cases())[name]
    for order in (0, 1, 2):
        D.check_pair(name, data, D.emu_compress(emu, data, order), Z.emu_compress(fixed_emu, data, order))


def test_the_fibonacci_case_leaves_as_a_dynamic_block(emu):
    """the limit of 15 bits is checked by zlib only if the block it acts on is sent.  (The other small cases reach the builder and the
    choice, and leave as the fixed mode's blocks: a fixed block of few tokens is shorter than any dynamic header.)"""
    data = dict(D.all_cases())["fibonacci"]
    for order in (0, 1, 2):
        assert [D.btype(b) for b in D.blocks(D.emu_compress(emu, data, order))] == [2]


@pytest.mark.parametrize("name", [h[0] for h in D.histograms()])
def test_code_builder(emu, name):
    _, limit, freq = [h for h in D.histograms() if h[0] == name][0]
    D.check_lengths(freq, limit, D.emu_code_lengths(emu, freq, limit))


def test_fibonacci_needs_the_limit(emu):
    """the case is of use only if the unlimited code is deeper than 15: a limit of 15 on 30 Fibonacci frequencies must give lengths
    other than the unlimited 1, 2, 3, ..., and the limit must be reached"""
    lens = D.emu_code_lengths(emu, D.fib(30), 15)
    assert max(lens) == 15 and sorted(lens, reverse=True)[:17].count(15) > 2


def test_stand_alone_under_sanitizers(tmp_path):
    exe = D.build_main_sanitized()
    cases, hists = D.all_cases(), D.histograms()
    for i, (_, data) in enumerate(cases):
        (tmp_path / ("case%d.in" % i)).write_bytes(data)
    for i, (_, limit, freq) in enumerate(hists):
        (tmp_path / ("hist%d.in" % i)).write_bytes(struct.pack("<II%dI" % len(freq), limit, len(freq), *freq))
    r = subprocess.run([exe, str(tmp_path), str(len(cases)), str(len(hists))], capture_output=True, text=True, timeout=600)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert r.returncode == 0 and "bgzf_dyn_main ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    fixed = C.CDLL(Z.build_emu())
    for i, (name, data) in enumerate(cases):
        for order in (0, 1, 2):
            D.check_pair(name, data, (tmp_path / ("case%d.%d.out" % (i, order))).read_bytes(), Z.emu_compress(fixed, data, order))
    for i, (_, limit, freq) in enumerate(hists):
        D.check_lengths(freq, limit, list((tmp_path / ("hist%d.out" % i)).read_bytes()))
