"""The BGZF compressor's host side where no GPU is needed: the bound, the refusal without a device, and the tool's NABWA_BGZF switch."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import nabwa_testlib as T

nabwa = importlib.import_module("network-aware-bwa_amd")
EXE = os.path.join(os.path.dirname(nabwa.LIB_PATH), "nabwa_bam2bam")


def test_bound_is_one_slot_per_slice():
    for n in (0, 1, 0xff00 - 1, 0xff00, 0xff00 + 1, 5 * 0xff00, 5 * 0xff00 + 1, (1 << 33) + 12345):
        assert nabwa.bgzf_bound(n) == (n + 0xff00 - 1) // 0xff00 * 0x10000
    assert nabwa.bgzf_bound(-1) == 0


NO_DEVICE = 9999      # a device number no machine has: the same refusal with and without a GPU


def test_no_device_is_an_error():
    L = nabwa.lib()
    data = np.arange(100, dtype=np.uint8)
    out = np.zeros(0x10000, np.uint8)
    n_out, n_blocks = C.c_int64(), C.c_int64()
    assert L.nabwa_bgzf_compress(NO_DEVICE, data.ctypes.data, 100, out.ctypes.data, out.size, C.byref(n_out), C.byref(n_blocks)) == nabwa.ENODEV
    assert L.nabwa_last_error()
    with pytest.raises(nabwa.NabwaError) as e:
        nabwa.bgzf_compress(b"abc", device=NO_DEVICE)
    assert e.value.code == nabwa.ENODEV
    h = C.c_void_p()
    assert L.nabwa_bgzf_create(NO_DEVICE, C.byref(h)) == nabwa.ENODEV and not h.value


def run_tool(tmp_path, value, device="0"):
    outp = str(tmp_path / "out.bam")
    inp = str(tmp_path / "in.bam")
    open(inp, "wb").write(b"")
    r = subprocess.run([EXE, "-g", T.TOY, "-f", outp, inp], capture_output=True, text=True, env=dict(os.environ, NABWA_BGZF=value, NABWA_DEVICE=device, NABWA_DEVICES=device), timeout=120)
    return r, outp


def test_an_unknown_writer_is_refused_before_any_output(tmp_path):
    for value in ("bogus", "", "GPU"):
        r, outp = run_tool(tmp_path, value)
        assert r.returncode == 1 and "NABWA_BGZF" in r.stderr, r.stderr[-500:]
        assert not os.path.exists(outp)


def test_gpu_writer_without_its_device_exits_2(tmp_path):
    r, outp = run_tool(tmp_path, "gpu", str(NO_DEVICE))
    assert r.returncode == 2 and "BGZF on the GPU" in r.stderr, r.stderr[-500:]
    assert not os.path.exists(outp)
