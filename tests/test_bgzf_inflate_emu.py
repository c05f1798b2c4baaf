"""The BGZF decompressor's kernel body (csrc/bgzf_inflate_body.hpp) on the CPU: the phases between the kernel's barriers run as loops
over the lanes (tests/emu/bgzf_inflate_emu.cpp) on every case of tests/bgzf_inflate_cases.py.  A valid member gives the bytes zlib gives;
a damaged one, which zlib refuses, gives its own status word and writes nothing outside its ISIZE bytes."""
import ctypes as C

import pytest

import bgzf_inflate_cases as I


@pytest.fixture(scope="module")
def emu():
    return C.CDLL(I.build_emu())


@pytest.mark.parametrize("name", [c[0] for c in I.valid_cases()])
def test_valid_members_inflate_to_zlibs_bytes(emu, name):
    _, members, raw = next(c for c in I.valid_cases() if c[0] == name)
    got = b""
    for m in members:
        want = I.zlib_verdict(m)
        assert want is not None, "zlib refuses a member of " + name
        st, out = I.emu_inflate(emu, m)
        assert st == I.OK and out == want
        got += out
    assert got == raw


@pytest.mark.parametrize("name", [c[0] for c in I.damaged_cases() if c[2] is not None])
def test_damaged_members_get_their_status(emu, name):
    _, m, status = next(c for c in I.damaged_cases() if c[0] == name)
    assert I.zlib_verdict(m) is None, "zlib accepts it: not a damaged member"
    st, _ = I.emu_inflate(emu, m)
    assert st == status


def test_the_statuses_of_the_damaged_list_are_distinct_per_rule():
    """one word per rule of the format: the list reaches thirteen of them"""
    seen = {st for _, _, st in I.damaged_cases() if st is not None}
    assert seen == {I.CRC, I.OUTPUT_LONG, I.OUTPUT_SHORT, I.BTYPE3, I.STORED_LEN, I.TRUNCATED, I.DIST_TOO_FAR, I.OVERSUBSCRIBED, I.INCOMPLETE,
                    I.REPEAT_FIRST, I.LENGTHS_OVERRUN, I.NO_EOB, I.BAD_SYMBOL}
