"""The bodies of the BAM coordinate sort as a stand-alone program (tests/emu/bam_sort_main.cpp) built with -fsanitize=address,undefined
and run as a child process: the keys and the record copies of tests/test_bam_sort_emu.py, every source in a heap buffer that ends with the
record's last byte and every destination between guard bytes.  Exit 0, the number of checks, and no report of a sanitizer."""
import subprocess

import pytest

import bam_sort_cases as S


@pytest.fixture(scope="module")
def exe():
    return S.build_main()


def test_keys_and_copies_under_the_sanitizers(exe):
    r = subprocess.run([exe] + [str(x) for x in S.COPY_SIZES], capture_output=True, timeout=300)
    err = r.stderr.decode()
    assert "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
    assert r.returncode == 0, err[-2000:]
    assert r.stdout.decode().strip() == "ok %d" % (16 * len(S.KEY_TIDS) * len(S.KEY_POSS) + 256 * len(S.COPY_SIZES))
