"""`nabwa.bgzf_decompress` (csrc/bgzf_inflate.hip, nabwa_bgzf.hip): BGZF members -> their bytes on the GPU.  The yardstick is zlib on the
CPU: every valid member of tests/bgzf_inflate_cases.py is first inflated by zlib, and the GPU's bytes must equal zlib's; every damaged one
is first refused by zlib, and the GPU call must raise EDATA naming that member -- between two valid members, with a valid call on the
same handle after it."""
import importlib
import os

import pytest

import bgzf_cases as Z
import bgzf_inflate_cases as I

nabwa = importlib.import_module("network-aware-bwa_amd")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    h = nabwa.Bgzf(0)
    yield h
    h.close()


@pytest.mark.parametrize("name", [c[0] for c in I.valid_cases()])
def test_valid_members_inflate_to_zlibs_bytes(handle, name):
    _, members, raw = next(c for c in I.valid_cases() if c[0] == name)
    assert b"".join(I.zlib_verdict(m) for m in members) == raw          # zlib on the CPU first: a None here is a broken case, not a kernel
    data = b"".join(members)
    assert nabwa.bgzf_inflated_size(data) == (len(raw), len(members))
    assert nabwa.bgzf_decompress(data) == raw
    assert handle.decompress(data) == raw


@pytest.mark.parametrize("name", [c[0] for c in I.damaged_cases()])
def test_damaged_members_are_edata_and_leave_the_handle_usable(handle, name):
    _, m, status = next(c for c in I.damaged_cases() if c[0] == name)
    if status is not None:
        assert I.zlib_verdict(m) is None, "zlib accepts it: not a damaged member"
    data, k = I.sandwich(m)
    for call in (nabwa.bgzf_decompress, handle.decompress):
        with pytest.raises(nabwa.NabwaError) as e:
            call(data, cap=1 << 20)
        assert e.value.code == nabwa.EDATA and "member %d " % k in str(e.value), str(e.value)
    _, members, raw = next(c for c in I.valid_cases() if c[0] == "three_deflate_blocks")
    assert handle.decompress(b"".join(members)) == raw


def test_capacity_one_byte_short(handle):
    _, members, raw = next(c for c in I.valid_cases() if c[0] == "text_level6")
    data = b"".join(members) + I.EOF_BLOCK
    assert handle.decompress(data, cap=len(raw)) == raw
    for call in (nabwa.bgzf_decompress, handle.decompress):
        with pytest.raises(nabwa.NabwaError) as e:
            call(data, cap=len(raw) - 1)
        assert e.value.code == nabwa.ECAP and e.value.needed == len(raw)


def test_compress_decompress_compress_on_one_handle(handle):
    c = dict(Z.cases())
    first = handle.compress(c["bam"])
    assert handle.decompress(first) == c["bam"]
    assert handle.compress(c["bam"]) == first
    assert handle.decompress(b"") == b""


def test_more_than_one_round(monkeypatch):
    """the handle's rounds hold 256 MB of inflated bytes; NABWA_BGZF_INFLATE_CAP, read when the handle is made, lowers that to 100 000
    bytes here, so the 320 members of one case go through in some forty rounds of whole members"""
    _, members, raw = next(c for c in I.valid_cases() if c[0] == "many_members")
    monkeypatch.setenv("NABWA_BGZF_INFLATE_CAP", "100000")
    with nabwa.Bgzf(0) as h:
        assert h.decompress(b"".join(members)) == raw
        bad, k = I.sandwich(next(c[1] for c in I.damaged_cases() if c[0] == "crc_one_bit"))
        with pytest.raises(nabwa.NabwaError) as e:
            h.decompress(b"".join(members) + bad, cap=len(raw) + (1 << 20))
        assert e.value.code == nabwa.EDATA and "member %d " % (len(members) + k) in str(e.value)


@pytest.mark.parametrize("name", [n for n, _ in Z.cases()])
def test_round_trip_through_the_compressor(handle, name):
    data = dict(Z.cases())[name]
    assert nabwa.bgzf_decompress(nabwa.bgzf_compress(data)) == data
