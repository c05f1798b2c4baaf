"""The stand-in libzmq of the nabwa_worker tests (zmq_double.cpp, next to this file): compile it, write the scenario directory it plays,
start the worker with it, read back what it wrote.  Test code only; nothing of the product refers to it."""
import importlib
import os
import struct
import subprocess

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "zmq_double.cpp")
SUB, REQ, DEALER = "SUB", "REQ", "DEALER"
SNDHWM, RCVHWM = 23, 24


def build(where, name="libzmq_double.so", defines=()):
    """-> the path of the shared library, compiled into `where` (a test's temporary directory).
    defines: ZMQ_DOUBLE_NO_POLL leaves zmq_poll out (a library that is not a usable libzmq), ZMQ_DOUBLE_OLD_NAMES exports zmq_init and
    zmq_term in place of zmq_ctx_new and zmq_ctx_term."""
    out = os.path.join(str(where), name)
    cmd = ["g++", "-shared", "-fPIC", "-O1", "-std=c++17"] + ["-D" + d for d in defines] + [SRC, "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    return out


def frame(messages):
    return b"".join(struct.pack("<I", len(m)) + m for m in messages)


def unframe(blob):
    out, p = [], 0
    while p < len(blob):
        n = struct.unpack_from("<I", blob, p)[0]
        out.append(blob[p + 4:p + 4 + n])
        p += 4 + n
    assert p == len(blob)
    return out


def write_scenario(where, config, messages, steps, isize=b"", files=None):
    """the directory ZMQ_DOUBLE_DIR names; steps: lines as zmq_double.cpp lists them; files: {name: bytes} for `broadcast NAME`"""
    d = os.path.join(str(where), "scenario")
    os.makedirs(d)
    for name, data in dict(files or {}, **{"config.bin": config, "isize.bin": isize, "messages.bin": frame(messages)}).items():
        with open(os.path.join(d, name), "wb") as f:
            f.write(bytes(data))
    with open(os.path.join(d, "steps.txt"), "w") as f:
        f.write("".join(s + "\n" for s in steps))
    return d


def run_worker(lib, scenario, args, env=None, timeout=120):
    """nabwa_worker as a child process with the double as its libzmq"""
    nabwa = importlib.import_module("network-aware-bwa_amd")
    e = dict(os.environ, NABWA_ZMQ_LIB=lib, ZMQ_DOUBLE_DIR=scenario)
    e.update(env or {})
    return subprocess.run([nabwa.WORKER_PATH] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=timeout)


def replies(scenario):
    with open(os.path.join(scenario, "replies.bin"), "rb") as f:
        return unframe(f.read())


class Log:
    """log.txt as a list of word lists, with the questions the tests ask"""

    def __init__(self, scenario):
        with open(os.path.join(scenario, "log.txt")) as f:
            self.lines = [l.split() for l in f.read().splitlines() if l]

    def sockets(self, kind):
        return [int(l[1]) for l in self.lines if l[0] == "socket" and l[2] == kind]

    def connects(self):
        """[(socket id, address)] in the order made"""
        return [(int(l[1]), l[2]) for l in self.lines if l[0] == "connect"]

    def hellos(self):
        return [bytes.fromhex(l[2]) if len(l) > 2 else b"" for l in self.lines if l[0] == "hello"]

    def options_before_connect(self, sock):
        """{option: value} set on a socket before its zmq_connect"""
        seen = {}
        for l in self.lines:
            if l[0] == "connect" and int(l[1]) == sock:
                return seen
            if l[0] == "setsockopt" and int(l[1]) == sock:
                seen[int(l[2])] = int(l[3])
        return None

    def number(self, what):
        v = [int(l[1]) for l in self.lines if l[0] == what]
        assert len(v) == 1, (what, self.lines[-8:])
        return v[0]
