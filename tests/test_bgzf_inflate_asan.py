"""The BGZF decompressor's kernel body as a stand-alone program (tests/emu/bgzf_inflate_main.cpp) built with
-fsanitize=address,undefined: every case file of tests/bgzf_inflate_cases.py, the damaged ones included, each payload and each output in
a buffer of exactly its size.  Exit 0 with zlib's bytes, or exit 3 with the member and its status (4: the header walk refuses the file);
the sanitizers report nothing."""
import subprocess

import pytest

import bgzf_inflate_cases as I


@pytest.fixture(scope="module")
def exe():
    return I.build_main()


def run(exe, tmp_path, data):
    p = str(tmp_path / "members.bgzf")
    open(p, "wb").write(data)
    r = subprocess.run([exe, p], capture_output=True, timeout=300)
    err = r.stderr.decode()
    assert "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
    return r.returncode, r.stdout, err


def test_valid_files(exe, tmp_path):
    for name, members, raw in I.valid_cases():
        rc, out, err = run(exe, tmp_path, b"".join(members))
        assert rc == 0 and out == raw, (name, rc, err[-500:])


def test_damaged_files(exe, tmp_path):
    for name, m, status in I.damaged_cases():
        data, k = I.sandwich(m)
        rc, out, err = run(exe, tmp_path, data)
        if status is None:
            assert rc == 4 and "member %d:" % k in err, (name, rc, err[-500:])
        else:
            assert rc == 3 and "member %d: status %d\n" % (k, status) in err, (name, rc, err[-500:])
        assert out == b""
