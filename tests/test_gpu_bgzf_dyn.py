"""`nabwa.bgzf_compress(data, codes="dynamic")` (bgzf_deflate_dyn_kernel in csrc/bgzf_deflate.hip): the compressor's dynamic Huffman
blocks on the GPU.  Every block goes through zlib (tests/bgzf_cases.py), is held against the fixed mode's block of the same slice from
the same handle, and is read back by the project's own device inflater."""
import importlib

import pytest

import bgzf_cases as Z
import bgzf_dyn_cases as D

nabwa = importlib.import_module("network-aware-bwa_amd")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    h = nabwa.Bgzf(0)
    yield h
    h.close()


@pytest.mark.parametrize("name", [n for n, _ in D.all_cases()])
def test_blocks_inflate_and_are_no_larger_than_fixed(handle, name):
    """len1..len4 equal the fixed mode's bytes, random is one stored block, text and bam are strictly smaller with a block of BTYPE 10
    (bgzf_dyn_cases.check_pair); textx3+17 is more than one slice per launch"""
    data = dict(D.all_cases())[name]
    dyn, fixed = handle.compress(data, codes="dynamic"), handle.compress(data, codes="fixed")
    assert fixed == handle.compress(data)
    D.check_pair(name, data, dyn, fixed)
    assert nabwa.bgzf_compress(data, codes="dynamic") == dyn
    print(name, len(data), "-> fixed", len(fixed), "dynamic", len(dyn), [D.btype(b) for b in D.blocks(dyn)][:4])


@pytest.mark.parametrize("name", ["text", "bam", "fibonacci"])
def test_same_bytes_from_every_call(handle, name):
    data = dict(D.all_cases())[name]
    first = handle.compress(data, codes="dynamic")
    assert any(D.btype(b) == 2 for b in D.blocks(first))
    assert handle.compress(data, codes="dynamic") == first and handle.compress(data, codes="dynamic") == first
    for _ in range(3):
        assert nabwa.bgzf_compress(data, codes="dynamic") == first


def test_a_handle_alternating_the_modes(handle):
    c = dict(D.all_cases())
    want = {(name, codes): handle.compress(c[name], codes=codes) for name in ("bam", "textx3+17") for codes in ("fixed", "dynamic")}
    assert want[("bam", "fixed")] != want[("bam", "dynamic")]
    for _ in range(2):
        for key in (("bam", "dynamic"), ("textx3+17", "fixed"), ("bam", "fixed"), ("textx3+17", "dynamic")):
            assert handle.compress(c[key[0]], codes=key[1]) == want[key]
    assert handle.compress(b"", codes="dynamic") == b""


@pytest.mark.parametrize("name", ["one_byte", "one_distance", "all_values_twice", "fibonacci", "text", "bam", "textx3+17", "random", "dist32768", "run600"])
def test_the_device_inflater_reads_it(handle, name):
    data = dict(D.all_cases())[name]
    out = handle.compress(data, codes="dynamic")
    assert handle.decompress(out) == data
    assert nabwa.bgzf_decompress(out) == data


def test_capacity_one_byte_short(handle):
    data = dict(D.all_cases())["textx3+17"]
    out = handle.compress(data, codes="dynamic")
    assert handle.compress(data, cap=len(out), codes="dynamic") == out
    with pytest.raises(nabwa.NabwaError) as e:
        handle.compress(data, cap=len(out) - 1, codes="dynamic")
    assert e.value.code == nabwa.ECAP and e.value.needed == len(out)
    with pytest.raises(nabwa.NabwaError) as e:
        nabwa.bgzf_compress(data, cap=len(out) - 1, codes="dynamic")
    assert e.value.code == nabwa.ECAP and e.value.needed == len(out)
