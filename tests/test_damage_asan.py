"""The bodies of the damage profile as a stand-alone program (tests/emu/damage_main.cpp) built with -fsanitize=address,undefined and run as a
child process on the cases of tests/test_damage_emu.py: every record in a heap buffer that ends with the record's last byte, the .pac in a
buffer of exactly l_pac / 4 + 1 bytes.  Exit 0, the number of checks, and no report of a sanitizer."""
import subprocess

import pytest

import damage_cases as D
import nabwa_testlib as T


@pytest.fixture(scope="module")
def exe():
    return D.build_main()


def test_cases_under_the_sanitizers(exe, tmp_path):
    ref = D.toy_ref()
    items = [(opt, recs, D.oracle(ref, opt, recs).words(), -1) for _, opt, recs in D.cases(ref)]
    good = D.good_records(ref, 20)
    for _, rec in D.damaged_cases(ref):
        items.append((D.opt_of(), [rec], None, 0))
        items.append((D.opt_of(), good[:9] + [rec] + good[9:], None, 9))
    recs, _ = D.sam_records("%s/se_adna.sam" % T.GOLDEN, ref)
    items.append((D.opt_of(), recs, D.oracle(ref, D.opt_of(), recs).words(), -1))
    path = str(tmp_path / "cases.bin")
    D.write_case_file(path, ref, items)
    r = subprocess.run([exe, path], capture_output=True, timeout=300)
    err = r.stderr.decode()
    assert "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
    assert r.returncode == 0, err[-2000:]
    assert r.stdout.decode().strip() == "ok %d" % sum(2 + len(x[1]) for x in items)
