"""`nabwa.bgzf_compress` (csrc/bgzf_deflate.hip, nabwa_bgzf.hip): bytes -> BGZF blocks on the GPU.  Only the inflated bytes are contract,
so each block is checked by what it is (tests/bgzf_cases.py: header, BSIZE, tiling, ISIZE, zlib's own inflate with its CRC check)."""
import importlib

import pytest

import bgzf_cases as Z

nabwa = importlib.import_module("network-aware-bwa_amd")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    h = nabwa.Bgzf(0)
    yield h
    h.close()


@pytest.mark.parametrize("name", [n for n, _ in Z.cases()])
def test_blocks_inflate_to_their_slices(name):
    data = dict(Z.cases())[name]
    out = nabwa.bgzf_compress(data)
    sizes = Z.walk(out, data)
    print(name, len(data), "->", len(out), sizes[:4])


def test_stored_fallback_and_matches():
    """random bytes leave as one stored block (fixed Huffman would expand them: 8 or 9 bits a byte).  Matches are found and used:
    fixed Huffman literals alone take at least a byte per byte, so text of a 300-word vocabulary must come out clearly smaller, and
    600 equal bytes are three lanes' literals and matches at distance 1 (258 + 13, 258 + 14, 56 bytes: five matches and one literal,
    at most 18 bits each, with the header bits and the end code 14 bytes)"""
    c = dict(Z.cases())
    assert len(nabwa.bgzf_compress(c["random"])) == Z.SLICE + 31
    assert len(nabwa.bgzf_compress(c["text"])) < Z.SLICE * 0.9
    assert len(nabwa.bgzf_compress(c["run600"])) <= 18 + 8 + 14


def test_capacity_one_byte_short(handle):
    data = dict(Z.cases())["textx3+17"]
    out = handle.compress(data)
    assert handle.compress(data, cap=len(out)) == out
    with pytest.raises(nabwa.NabwaError) as e:
        handle.compress(data, cap=len(out) - 1)
    assert e.value.code == nabwa.ECAP and e.value.needed == len(out)
    with pytest.raises(nabwa.NabwaError) as e:
        nabwa.bgzf_compress(data, cap=len(out) - 1)
    assert e.value.code == nabwa.ECAP and e.value.needed == len(out)


def test_a_handle_starts_every_call_afresh(handle):
    """the tables, the bitmap and the block's slot are set up by every call: a second call gives the same bytes, whatever ran between"""
    c = dict(Z.cases())
    first = handle.compress(c["bam"])
    Z.walk(handle.compress(c["random"] + c["allff"]), c["random"] + c["allff"])
    Z.walk(handle.compress(c["run600"]), c["run600"])
    assert handle.compress(c["bam"]) == first
    assert handle.compress(b"") == b""


@pytest.mark.parametrize("name", ["text", "128values", "textx3+17", "matches3"])
def test_same_bytes_from_every_call(handle, name):
    """the lanes of the one wave that parses a slice share the hash table without locks; which of two lanes' entries a bucket keeps is
    the hardware's order of the wave's LDS writes, the same in every run of one binary on one device: three calls, one output"""
    data = dict(Z.cases())[name]
    first = handle.compress(data)
    assert handle.compress(data) == first and nabwa.bgzf_compress(data) == first


def test_more_than_one_chunk(handle):
    """at most 1040 slices go through per launch: one slice more takes two rounds of 521 and 520, and the blocks still tile"""
    data = (dict(Z.cases())["text"] * 1041)[:1040 * Z.SLICE + 99]
    out = handle.compress(data)
    assert len(Z.walk(out, data)) == 1041
