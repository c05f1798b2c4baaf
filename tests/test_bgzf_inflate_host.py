"""The BGZF decompressor where no GPU is needed: the walk over the members' headers (nabwa.bgzf_inflated_size), the refusal without a
device, the tool's NABWA_BGZF_IN switch, and the optional inflater of csrc/bgzf_in.hpp's BamIn with a zlib-backed stand-in for the
library (tests/emu/bgzf_in_inflater_main.cpp)."""
import gzip
import importlib
import os
import subprocess

import numpy as np
import pytest

import bgzf_inflate_cases as I
import nabwa_testlib as T
from test_bgzf_in import bgzf

nabwa = importlib.import_module("network-aware-bwa_amd")
EXE = os.path.join(os.path.dirname(nabwa.LIB_PATH), "nabwa_bam2bam")
NO_DEVICE = 9999      # a device number no machine has: the same refusal with and without a GPU


def test_inflated_size_of_valid_input():
    assert nabwa.bgzf_inflated_size(b"") == (0, 0)
    assert nabwa.bgzf_inflated_size(I.EOF_BLOCK) == (0, 1)
    for name, members, raw in I.valid_cases():
        assert nabwa.bgzf_inflated_size(b"".join(members)) == (len(raw), len(members)), name


def test_inflated_size_reads_headers_and_trailers_only():
    """a damaged payload is not its business; a trailer's ISIZE is"""
    for name, m, status in I.damaged_cases():
        if status is not None:
            assert nabwa.bgzf_inflated_size(m) == (I.split(m)[2], 1), name


def test_inflated_size_refuses_what_is_not_whole_members():
    good = I.valid_cases()[2][1][0]
    bad = {name: m for name, m, status in I.damaged_cases() if status is None}
    assert sorted(bad) == ["bsize_past_the_input", "trailing_half_header"]
    cases = dict(bad, not_gzip=b"BAM\1" + bytes(40), gzip_without_bc=gzip.compress(b"abc"), isize_above_64k=I.member(b"\3\0", b"", crc=0, isize=0x10001),
                 cut_in_the_trailer=good[:-3])
    for name, m in cases.items():
        for k, data in ((0, m), (1, good + m)):
            with pytest.raises(nabwa.NabwaError) as e:
                nabwa.bgzf_inflated_size(data)
            assert e.value.code == nabwa.EDATA == -7 and "member %d " % k in str(e.value), (name, str(e.value))


def test_no_device_is_an_error():
    with pytest.raises(nabwa.NabwaError) as e:
        nabwa.bgzf_decompress(I.EOF_BLOCK, device=NO_DEVICE)
    assert e.value.code == nabwa.ENODEV


def test_an_unknown_reader_is_refused_before_any_output(tmp_path):
    inp, outp = str(tmp_path / "in.bam"), str(tmp_path / "out.bam")
    open(inp, "wb").write(b"")
    for value in ("zlib", "", "GPU"):
        r = subprocess.run([EXE, "-g", T.TOY, "-f", outp, inp], capture_output=True, text=True, env=dict(os.environ, NABWA_BGZF_IN=value), timeout=120)
        assert r.returncode == 1 and "NABWA_BGZF_IN" in r.stderr, r.stderr[-500:]
        assert not os.path.exists(outp)


def test_gpu_reader_without_its_device_exits_2(tmp_path):
    inp, outp = str(tmp_path / "in.bam"), str(tmp_path / "out.bam")
    open(inp, "wb").write(b"")
    r = subprocess.run([EXE, "-g", T.TOY, "-f", outp, inp], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, NABWA_BGZF_IN="gpu", NABWA_DEVICE=str(NO_DEVICE), NABWA_DEVICES=str(NO_DEVICE)))
    assert r.returncode == 2 and "BGZF on the GPU" in r.stderr, r.stderr[-500:]
    assert not os.path.exists(outp)


# ---------------------------------------------------------------- BamIn's inflater
@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("bgzf_inflater")
    out = []
    for src in ("bgzf_in_main.cpp", "bgzf_in_inflater_main.cpp"):
        out.append(str(d / src[:-4]))
        subprocess.run(["g++", "-O1", "-std=c++17", "-o", out[-1], os.path.join(T.ROOT, "tests", "emu", src), "-lz", "-lpthread"], check=True)
    return out


def test_the_inflater_gives_the_thread_loops_bytes(exes, tmp_path):
    """the containers of tests/test_bgzf_in.py: BGZF goes through the callable, any other gzip stream and a plain file never reach it"""
    rng = np.random.default_rng(3)
    raw = b"BAM\1" + bytes(rng.integers(0, 7, 3_000_000, dtype=np.uint8)) + bytes(rng.integers(0, 256, 200_000, dtype=np.uint8))
    forms = {
        "bgzf": (bgzf(raw), "bgzf"),
        "bgzf_small_blocks": (bgzf(raw, 1000), "bgzf"),
        "bgzf_other_subfield": (bgzf(raw, 40000, extra_first=True), "bgzf"),
        "only_marker": (I.EOF_BLOCK, "bgzf"),
        "members": (b"".join(gzip.compress(raw[o:o + 300_000], 1) for o in range(0, len(raw), 300_000)), "stream"),
        "plain": (raw, "raw"),
    }
    for name, (data, kind) in forms.items():
        p = str(tmp_path / name)
        open(p, "wb").write(data)
        a = subprocess.run([exes[0], p], capture_output=True, timeout=120)
        b = subprocess.run([exes[1], p], capture_output=True, timeout=120)
        assert a.returncode == 0 and b.returncode == 0, (name, b.stderr[-500:])
        assert a.stdout == b.stdout == (raw if name != "only_marker" else b""), name
        got_kind, calls = b.stderr.decode().split()
        assert got_kind == kind and (int(calls) > 0) == (kind == "bgzf"), (name, b.stderr)


def test_a_false_return_ends_the_run(exes, tmp_path):
    p = str(tmp_path / "in")
    open(p, "wb").write(bgzf(b"abc" * 1000))
    r = subprocess.run([exes[1], p, "refuse"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and "BGZF block" in r.stderr and "the stand-in refuses block 0" in r.stderr, r.stderr
    assert r.stdout == ""


def test_damage_is_an_error_with_the_inflater_too(exes, tmp_path):
    raw = bytes(np.random.default_rng(4).integers(0, 5, 500_000, dtype=np.uint8))
    good = bgzf(raw)
    for name, data in {"cut_in_a_block": good[:len(good) // 2], "flipped_payload": good[:5000] + bytes([good[5000] ^ 0x41]) + good[5001:]}.items():
        p = str(tmp_path / name)
        open(p, "wb").write(data)
        r = subprocess.run([exes[1], p], capture_output=True, timeout=120)
        assert r.returncode == 3 and b"BGZF" in r.stderr, (name, r.stderr)
