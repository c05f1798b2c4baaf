"""What the four record-stream modules (nabwa_bam_sort_run_ex, nabwa_damage_add, nabwa_markdup_add, nabwa_bai_add) decide from n_rec, in and
in_off alone, in one list run against all four: the result and the whole text of nabwa_last_error().  The checks come before the handle is
looked at, so any address stands in for one and no device is needed.  The texts are those the modules had while each carried its own copy
of the checks (csrc/rec_stream.hpp: rec_check_offsets)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import bamlib as B
import markdup_cases as M
import nabwa_testlib as T

nabwa = importlib.import_module("network-aware-bwa_amd")

N = 5
DATA, OFF = B.pack(M.random_records(N, 1)[:N])


def _off(change):
    o = OFF.copy()
    change(o)
    return o


def _set(k, v):
    def change(o):
        o[k] = v(o)
    return change


# name, n_rec, whether `in` is given, the offsets (None: a null pointer), the result, the whole message (None: not looked at)
CASES = [
    ("n_rec -1", -1, True, OFF, "EINVAL", b"n_rec -1: 0 .. 2147483647 records"),
    ("n_rec 2^31", 1 << 31, True, OFF, "EINVAL", b"n_rec 2147483648: 0 .. 2147483647 records"),
    ("null in", N, False, OFF, "EINVAL", b"null argument"),
    ("null in_off", N, True, None, "EINVAL", b"null argument"),
    ("negative first offset", N, True, _off(_set(0, lambda o: -1)), "EINVAL", b"the first offset is negative"),
    ("equal offsets at record 2", N, True, _off(_set(3, lambda o: o[2])), "EINVAL", b"the offsets do not increase at record 2"),
    ("a record of 35 bytes", N, True, _off(_set(3, lambda o: o[2] + 35)), "EINVAL", b"record 2 has 35 bytes: a BAM record has at least 36"),
    ("no records and null in", 0, False, OFF, "OK", None),
]


def _call(module, handle, n_rec, data, off):
    L = nabwa.lib()
    if module == "sort":
        out = np.zeros(int(OFF[-1]), np.uint8)
        return L.nabwa_bam_sort_run_ex(handle, n_rec, data, off, T.ptr(out), len(out), None, None, None)
    if module == "bai":
        return L.nabwa_bai_add(handle, n_rec, data, off, 0)
    return getattr(L, "nabwa_%s_add" % module)(handle, n_rec, data, off)


@pytest.mark.parametrize("module", ["sort", "damage", "markdup", "bai"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_what_the_offsets_alone_say(module, case):
    _, n_rec, with_in, off, code, text = case
    # zero bytes, which no handle looks like.  The one read of it: nabwa_bai_add looks at its count of records added (0 here) before it
    # returns for n_rec == 0; nothing else is read and nothing is written
    some = C.create_string_buffer(4096)
    r = _call(module, some, n_rec, T.ptr(DATA) if with_in else None, None if off is None else T.ptr(off))
    assert r == getattr(nabwa, code)
    if text is not None:
        assert nabwa.lib().nabwa_last_error() == text
    assert some.raw == bytes(4096)
