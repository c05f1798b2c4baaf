"""`nabwa_worker` without a GPU: its command line, the run-time binding of libzmq (a missing library, a library that lacks a call) and
the first step of the start-up exchange (reference bam2bam.c:2250-2265) against the stand-in libzmq of tests/zmq_double -- up to the point
where the program looks for its GPU.  Also what of a damaged positioned record can be refused without an index: the message-level
checks of the codec (the row checks of nabwa_bam_batch_restore need a batch, tests/test_gpu_worker_exe.py)."""
import ctypes as C
import importlib
import os
import struct
import subprocess

import pytest

import bamlib as B
import nabwa_testlib as T
import wirelib as W
import zmq_double as Z

nabwa = importlib.import_module("network-aware-bwa_amd")


def run(args, env):
    if not os.path.exists(nabwa.WORKER_PATH):
        pytest.fail("%s was not built" % nabwa.WORKER_PATH)
    e = dict(os.environ, NABWA_DEVICE="99")                    # no such GPU, wherever the test runs
    e.pop("NABWA_ZMQ_LIB", None)
    e.update(env)
    return subprocess.run([nabwa.WORKER_PATH] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=60)


@pytest.mark.parametrize("args", [[], ["-h", "somewhere"], ["-p", "5000", "operand"], ["-t", "2", "-T", "5"]])
def test_usage_on_stderr_and_exit_1_without_a_port_or_with_an_operand(args):
    r = run(args, {"NABWA_ZMQ_LIB": "/nonexistent/libzmq.so"})
    assert r.returncode == 1 and r.stdout == b""
    for word in (b"Usage:", b"--num-threads", b"--host", b"--port", b"--timeout"):
        assert word in r.stderr


def system_has_libzmq():
    for name in ("libzmq.so.5", "libzmq.so.3", "libzmq.so"):
        try:
            C.CDLL(name)
            return True
        except OSError:
            pass
    return False


def test_missing_library_exits_2_and_is_named(tmp_path):
    if system_has_libzmq():
        pytest.skip("this machine has a libzmq of its own: the program would load it")
    missing = str(tmp_path / "no_such_libzmq.so")
    r = run(["-p", "5000"], {"NABWA_ZMQ_LIB": missing})
    assert r.returncode == 2 and r.stdout == b""
    lines = r.stderr.decode().splitlines()
    assert len(lines) == 1                                       # one clear line
    assert missing in lines[0] and "libzmq.so.5" in lines[0] and "libzmq.so.3" in lines[0]


def test_library_without_a_needed_call_exits_2_and_the_call_is_named(tmp_path):
    stub = Z.build(tmp_path, "libstub.so", defines=["ZMQ_DOUBLE_NO_POLL"])
    r = run(["-p", "5000"], {"NABWA_ZMQ_LIB": stub, "ZMQ_DOUBLE_DIR": str(tmp_path)})
    assert r.returncode == 2 and r.stdout == b""
    lines = r.stderr.decode().splitlines()
    assert len(lines) == 1 and stub in lines[0] and "zmq_poll" in lines[0]
    assert not (tmp_path / "log.txt").exists()                   # nothing of the library was called


def toy_config():
    L = W.bind(nabwa.lib())
    opt, po = nabwa.gap_init_opt(), nabwa.pe_opt_default()
    n = L.nabwa_wire_config_encode(C.byref(opt), C.byref(po), T.TOY.encode(), None, 0)
    assert n == nabwa.ECAP or n > 0
    out = (C.c_uint8 * (112 + len(T.TOY.encode())))()
    assert L.nabwa_wire_config_encode(C.byref(opt), C.byref(po), T.TOY.encode(), out, len(out)) == len(out)
    return bytes(out)


@pytest.mark.parametrize("defines", [(), ("ZMQ_DOUBLE_OLD_NAMES",)])
def test_hello_goes_to_host_and_port_first_then_no_gpu_exits_2(tmp_path, defines):
    lib = Z.build(tmp_path, defines=defines)
    scen = Z.write_scenario(tmp_path, toy_config(), [], ["terminate"])
    r = Z.run_worker(lib, scen, ["-h", "master.example", "-p", "6100", "-t", "2"], env={"NABWA_DEVICE": "99"}, timeout=60)
    assert r.returncode == 2, r.stderr
    assert b"no usable GPU" in r.stderr and r.stdout == b""
    log = Z.Log(scen)
    assert log.connects() == [(log.sockets(Z.REQ)[0], "tcp://master.example:6100")]       # the first and, without a GPU, the only connection
    assert log.hellos() == [b"\0" + os.uname().nodename.encode()]
    assert log.sockets(Z.DEALER) == [] and log.sockets(Z.SUB) == []
    assert log.number("replies") == 0 and [l[0] for l in log.lines][0] == ("init" if defines else "ctx_new")


def test_configuration_reply_that_is_too_short_exits_1(tmp_path):
    lib = Z.build(tmp_path)
    scen = Z.write_scenario(tmp_path, toy_config()[:100], [], ["terminate"])
    r = Z.run_worker(lib, scen, ["-p", "6100"], env={"NABWA_DEVICE": "99"}, timeout=60)
    assert r.returncode == 1 and b"configuration" in r.stderr, r.stderr
    assert Z.Log(scen).connects()[0][1] == "tcp://localhost:6100"                          # -h defaults to localhost


def test_worker_wrapper_starts_the_tool(monkeypatch):
    monkeypatch.setenv("NABWA_ZMQ_LIB", "/nonexistent/libzmq.so")
    if system_has_libzmq():
        pytest.skip("this machine has a libzmq of its own: the program would load it")
    r = nabwa.worker("localhost", 5000, args=("-t", 2), device=99, timeout=60)
    assert r.returncode == 2 and b"/nonexistent/libzmq.so" in r.stderr


def test_libnabwa_has_no_dependency_on_zmq():
    r = subprocess.run(["readelf", "-d", nabwa.LIB_PATH], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        r = subprocess.run(["ldd", nabwa.LIB_PATH], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, check=True)
    assert "zmq" not in r.stdout
    r = subprocess.run(["readelf", "-d", nabwa.WORKER_PATH], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode == 0:
        assert "zmq" not in r.stdout


def test_damaged_positioned_message_is_refused_by_the_codec():
    """what can be checked without an index: counts that do not fit the message never reach a batch"""
    L = W.bind(nabwa.lib())
    bam = B.make_record("r", "ACGTACGTACGTAACCGGTT", "I" * 20, 4)
    aln = [struct.pack("<IIIi", 0, 100, 102, 3)]
    d = dict(bam=bam, strand=0, type=1, n_mm=0, n_gapo=0, n_gape=0, seQ=23, mapQ=25, len=20, clip_len=20, score=3, sa=101, c1=1, c2=0, pos=5000,
             multi=[], max_entries=10, aln=aln)
    good = W.message(1, 1, 2, [d])
    assert W.decode(L, good)[0] == 0
    at_n_aln = len(good) - 16 - 4                                  # i32 n_aln stands in front of the one row
    at_n_multi = at_n_aln - 4 - 4                                  # ... and i32 n_multi in front of max_entries
    assert struct.unpack_from("<i", good, at_n_aln)[0] == 1 and struct.unpack_from("<i", good, at_n_multi)[0] == 0
    for at, bad in ((at_n_aln, -1), (at_n_aln, 2), (at_n_aln, 0x7fffffff), (at_n_multi, -1), (at_n_multi, 1), (at_n_multi, 0x10000000)):
        m = bytearray(good)
        struct.pack_into("<i", m, at, bad)
        assert W.decode(L, bytes(m))[0] == nabwa.EINVAL, (at, bad)
    assert W.decode(L, good[:-1])[0] == nabwa.EINVAL and W.decode(L, good + b"\0")[0] == nabwa.EINVAL
