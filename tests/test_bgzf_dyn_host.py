"""The host side of the BGZF compressor's dynamic mode where no GPU is needed: the refusal of an unknown `codes` value in C and in
Python, the refusal without a device, and the tool's NABWA_BGZF=gpu-dynamic."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

from test_bgzf_host import NO_DEVICE, run_tool

nabwa = importlib.import_module("network-aware-bwa_amd")


def call_ex(device, codes):
    L = nabwa.lib()
    data = np.arange(100, dtype=np.uint8)
    out = np.zeros(0x10000, np.uint8)
    n_out, n_blocks = C.c_int64(), C.c_int64()
    return L.nabwa_bgzf_compress_ex(device, codes, data.ctypes.data, 100, out.ctypes.data, out.size, C.byref(n_out), C.byref(n_blocks))


def test_the_two_values_of_codes():
    L = nabwa.lib()
    assert (nabwa.BGZF_CODES["fixed"], nabwa.BGZF_CODES["dynamic"]) == (0, 1)
    header = open(os.path.join(os.path.dirname(nabwa.LIB_PATH), "..", "include", "nabwa.h")).read()
    assert "#define NABWA_BGZF_CODES_FIXED    0\n" in header and "#define NABWA_BGZF_CODES_DYNAMIC  1\n" in header
    assert L.nabwa_bgzf_handle_compress_ex


@pytest.mark.parametrize("codes", [2, -1, 256, 1 << 30])
def test_an_unknown_codes_value_is_einval_in_c(codes):
    """on any device number, the one no machine has included: the value is refused before a device is looked for"""
    L = nabwa.lib()
    for device in (0, NO_DEVICE):
        assert call_ex(device, codes) == nabwa.EINVAL
        assert b"codes" in L.nabwa_last_error()


@pytest.mark.parametrize("codes", ["dynamics", "", "Dynamic", None, 1, b"dynamic"])
def test_an_unknown_codes_value_is_a_valueerror_in_python(codes):
    with pytest.raises(ValueError):
        nabwa.bgzf_compress(b"abc", device=NO_DEVICE, codes=codes)
    with pytest.raises(ValueError):
        nabwa.Bgzf.compress(object(), b"abc", codes=codes)      # refused before the handle is looked at


def test_dynamic_without_a_device_is_enodev():
    assert call_ex(NO_DEVICE, nabwa.BGZF_CODES["dynamic"]) == nabwa.ENODEV
    assert call_ex(NO_DEVICE, nabwa.BGZF_CODES["fixed"]) == nabwa.ENODEV
    with pytest.raises(nabwa.NabwaError) as e:
        nabwa.bgzf_compress(b"abc", device=NO_DEVICE, codes="dynamic")
    assert e.value.code == nabwa.ENODEV


def test_the_dynamic_writer_without_its_device_exits_2(tmp_path):
    r, outp = run_tool(tmp_path, "gpu-dynamic", str(NO_DEVICE))
    assert r.returncode == 2 and "BGZF on the GPU" in r.stderr, r.stderr[-500:]
    assert not os.path.exists(outp)


def test_a_value_one_letter_longer_exits_1(tmp_path):
    r, outp = run_tool(tmp_path, "gpu-dynamics")
    assert r.returncode == 1 and "host, gpu or gpu-dynamic" in r.stderr, r.stderr[-500:]
    assert not os.path.exists(outp)
