"""The BGZF compressor's kernel body (csrc/bgzf_deflate_body.hpp) on the CPU: the phases between the kernel's barriers run as loops over
the lanes (tests/emu/bgzf_emu.cpp), on the inputs of the GPU test and through the same walk over the blocks -- and once more under
AddressSanitizer, which is where an index past the LDS image or the block's slot shows without a GPU."""
import os
import subprocess
import sys

import pytest

import bgzf_cases as Z
import ctypes as C


@pytest.fixture(scope="module")
def emu():
    return C.CDLL(Z.build_emu())


@pytest.mark.parametrize("name", [n for n, _ in Z.cases()])
def test_blocks_inflate_to_their_slices(emu, name):
    data = dict(Z.cases())[name]
    outs = [Z.emu_compress(emu, data, order) for order in (0, 1, 2)]
    for out in outs:
        Z.walk(out, data)


def test_matches_are_found():
    """fixed Huffman literals alone take at least a byte per byte: text of a 300-word vocabulary must come out clearly smaller in any
    order of the lanes, and 600 equal bytes are five matches and one literal (tests/test_gpu_bgzf.py has the sum)"""
    emu = C.CDLL(Z.build_emu())
    text = dict(Z.cases())["text"]
    for order in (0, 1, 2):
        assert len(Z.emu_compress(emu, text, order)) < len(text) * 0.9
        assert len(Z.emu_compress(emu, b"a" * 600, order)) <= 18 + 8 + 14


def test_under_address_sanitizer():
    so = Z.build_emu(asan=True)
    asan = subprocess.run(["g++", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    code = ("import sys; sys.path.insert(0, %r); import ctypes as C, bgzf_cases as Z\n"
            "lib = C.CDLL(%r)\n"
            "for name, data in Z.cases():\n"
            "    for order in (0, 1, 2):\n"
            "        Z.walk(Z.emu_compress(lib, data, order), data)\n"
            "print('asan ok')\n" % (os.path.dirname(os.path.abspath(__file__)), so))
    env = dict(os.environ, LD_PRELOAD=":".join(x for x in (asan, os.environ.get("LD_PRELOAD", "")) if x), ASAN_OPTIONS="detect_leaks=0", PYTHONMALLOC="malloc")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "asan ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
