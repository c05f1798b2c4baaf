"""`nabwa_worker`, the executable, against the stand-in libzmq of tests/zmq_double, which plays `bwa bam2bam -p` inside the worker's
process: the two-phase exchange of a mixed file with the insert-size broadcast in between, the master's resends, the records-in-flight
settings, and positioned records whose hit rows cannot come from the index.  What the worker sends must be, byte for byte, what the
library's own worker core (nabwa_worker_process, built as tests/test_gpu_worker.py builds it) answers in-process to the same messages in
the same order.  Each test starts the worker once, as a child process under its own timeout.  PARITY UNPINNED, as for the codec: no real
libzmq and no reference master has been run against the program."""
import ctypes as C
import importlib
import os
import re
import struct

import pytest

import bamlib as B
import nabwa_testlib as T
import wirelib as W
import zmq_double as Z
from test_gpu_bam import chk
from test_gpu_worker import bam_of, bind, direct, new_worker, pristine_messages, process

nabwa = importlib.import_module("network-aware-bwa_amd")
pytestmark = pytest.mark.gpu
P = C.c_void_p
PORT = 6100


@pytest.fixture(scope="module")
def world():
    """about 200 logical records of the committed toy reads: pairs of two read groups with a single read after every third"""
    L = bind()
    ix = nabwa.Index.load(T.TOY, 0, True, True)
    se = T.read_fastq(os.path.join(T.GOLDEN, "reads_se.fq"))
    pe = [T.read_fastq(os.path.join(T.GOLDEN, "reads_pe_%d.fq" % e)) for e in (1, 2)]
    logical = []
    for i in range(150):
        if i % 3 == 0:
            n, s, q = se[i // 3]
            logical.append((1, [B.make_record(n, s, q, 4)]))
        n, s1, q1 = pe[0][i]
        _, s2, q2 = pe[1][i]
        rg = B.tag_z("RG", "libA" if i % 2 else "libB")
        logical.append((2, [B.make_record(n, s1, q1, 1 | 64 | 4 | 8, rg), B.make_record(n, s2, q2, 1 | 128 | 4 | 8, rg)]))
    opt, po = nabwa.gap_init_opt(), nabwa.pe_opt_default()
    w = dict(L=L, ix=ix, logical=logical, opt=opt, po=po, se=se)
    n = 112 + len(T.TOY.encode())
    cfg = (C.c_uint8 * n)()
    assert L.nabwa_wire_config_encode(C.byref(opt), C.byref(po), T.TOY.encode(), cfg, n) == n
    w["config"] = bytes(cfg)
    _, blob = direct(w)                                         # the estimates of the whole file, as the master's output thread infers them
    w["blob"] = bytes(blob)
    yield w
    ix.close()


@pytest.fixture(scope="module")
def zlib(tmp_path_factory):
    return Z.build(tmp_path_factory.mktemp("zmq_double"))


def counts_of(L, wk):
    cnt = (C.c_uint64 * 4)()
    L.nabwa_worker_counts(wk, cnt)
    return list(cnt)


def counts_line(stderr):
    m = re.search(rb"records: (\d+) positioned, (\d+) finished, (\d+) bounced \(no estimates\), (\d+) passed through", stderr)
    assert m, stderr
    return [int(x) for x in m.groups()]


def test_two_phase_exchange_equals_the_in_process_core(world, zlib, tmp_path):
    L = world["L"]
    first = pristine_messages(world)
    assert 190 <= len(first) <= 210
    # a few records that arrive already finished, and an end marker, among them
    for at, (kind, rs) in ((5, world["logical"][5]), (77, world["logical"][77]), (140, world["logical"][140])):
        first.insert(at, W.message(5000 + at, kind, 3, [dict(bam=r) for r in rs]))
    first.append(W.message(9999, 0, 0, []))
    # in-process: everything pristine -> positioned, the estimates, the positioned answers again -> finished
    wk = new_worker(world)
    rc, one = process(L, wk, first)
    assert rc == 0, L.nabwa_last_error()
    blob = world["blob"]
    chk(L, L.nabwa_worker_set_isize(wk, blob, len(blob)))
    rc, two = process(L, wk, one)
    assert rc == 0, L.nabwa_last_error()
    want_counts = counts_of(L, wk)
    L.nabwa_worker_destroy(wk)
    phases = [bam_of(L, m)[0].phase for m in two]
    assert phases.count(3) == len(first) - 1 and want_counts[:3] == [len(first) - 4, len(first) - 4, 0]
    # the same through the sockets' stand-in
    steps = ["send %d" % len(first), "wait %d" % len(first), "broadcast estimates.bin", "echo", "wait %d" % len(first), "terminate"]
    scen = Z.write_scenario(tmp_path, world["config"], first, steps, files={"estimates.bin": b"\2" + blob})
    r = Z.run_worker(zlib, scen, ["-p", PORT], timeout=120)
    assert r.returncode == 0, r.stderr
    got = Z.replies(scen)
    assert len(got) == 2 * len(first)
    for i, (g, x) in enumerate(zip(got, one + two)):
        assert g == x, i
    assert counts_line(r.stderr) == want_counts
    log = Z.Log(scen)
    host = "tcp://localhost:%d"
    req, dealers, sub = log.sockets(Z.REQ), log.sockets(Z.DEALER), log.sockets(Z.SUB)
    assert len(req) == 1 and len(dealers) == 1 and len(sub) == 1
    assert log.connects() == [(req[0], host % PORT), (dealers[0], host % (PORT + 1)), (sub[0], host % (PORT + 2))]
    node = os.uname().nodename.encode()
    assert log.hellos() == [b"\0" + node, b"\1" + node]
    assert ["setsockopt", str(sub[0]), "6", "0"] in log.lines                      # ZMQ_SUBSCRIBE to everything
    assert log.number("replies") == 2 * len(first)


def test_resent_record_and_a_positioned_record_before_any_estimate(world, zlib, tmp_path):
    L = world["L"]
    first = pristine_messages(world)
    other = new_worker(world)
    rc, pos = process(L, other, [first[4]])
    assert rc == 0
    L.nabwa_worker_destroy(other)
    msgs = [first[1], first[2], first[1], pos[0]]                                # first[1] goes out twice, as the master's resend loop does it
    wk = new_worker(world)
    rc, want = process(L, wk, msgs)
    assert rc == 0, L.nabwa_last_error()
    want_counts = counts_of(L, wk)
    L.nabwa_worker_destroy(wk)
    assert want_counts == [3, 0, 1, 0] and want[3] == pos[0]
    assert bam_of(L, want[0])[0].recno == bam_of(L, want[2])[0].recno and bam_of(L, want[2])[0].phase == 2
    scen = Z.write_scenario(tmp_path, world["config"], msgs, ["send 4", "wait 4", "terminate"])          # no estimates in the second hello's reply
    r = Z.run_worker(zlib, scen, ["-p", PORT], timeout=120)
    assert r.returncode == 0, r.stderr
    assert Z.replies(scen) == want
    assert counts_line(r.stderr) == want_counts


def test_records_in_flight(world, zlib, tmp_path):
    L = world["L"]
    se = world["se"]
    msgs = [W.message(k, 1, 0, [dict(bam=B.make_record(se[k % len(se)][0], se[k % len(se)][1], se[k % len(se)][2], 4))]) for k in range(2000)]
    scen = Z.write_scenario(tmp_path, world["config"], msgs, ["send 2000", "wait 2000", "terminate"])
    r = Z.run_worker(zlib, scen, ["-p", PORT, "-t", 3], env={"NABWA_WORKER_INFLIGHT": "4096"}, timeout=120)
    assert r.returncode == 0, r.stderr
    log = Z.Log(scen)
    dealers = log.sockets(Z.DEALER)
    assert len(dealers) == 3                                                     # -t 3: three connections, three peers to the master
    for d in dealers:
        before = log.options_before_connect(d)
        assert before is not None and before.get(Z.RCVHWM) == 4096 and before.get(Z.SNDHWM) == 4096
        assert (d, "tcp://localhost:%d" % (PORT + 1)) in log.connects()
    assert log.number("max_outstanding") > 64                                    # more than the reference's per-peer 64 was on its way at once
    assert log.number("delivered") == 2000 and log.number("replies") == 2000 and log.number("max_queued") <= 4096
    got = Z.replies(scen)
    assert sorted(bam_of(L, m)[0].recno for m in got) == list(range(2000))
    assert all(bam_of(L, m)[0].phase == 2 for m in got[::97])
    assert counts_line(r.stderr) == [2000, 0, 0, 0]


def test_high_water_mark_bounds_what_the_double_queues(world, zlib, tmp_path):
    """the stand-in honours the receive high-water mark it was given: with 8 it never lets more than 8 records wait in the connection"""
    se = world["se"]
    msgs = [W.message(k, 1, 0, [dict(bam=B.make_record(*se[k], 4))]) for k in range(100)]
    scen = Z.write_scenario(tmp_path, world["config"], msgs, ["send 100", "wait 100", "terminate"])
    r = Z.run_worker(zlib, scen, ["-p", PORT], env={"NABWA_WORKER_INFLIGHT": "8"}, timeout=120)
    assert r.returncode == 0, r.stderr
    log = Z.Log(scen)
    assert log.number("replies") == 100 and 1 <= log.number("max_queued") <= 8


def damaged(L, msg, change):
    """msg, positioned, with the first hit row of its first read changed by change(k, l) -> (k, l); the read must have a row"""
    rc, rec, keep = W.decode(L, msg)
    assert rc == 0
    x = rec.read[0]
    assert x.n_aln > 0
    rows = bytearray(C.string_at(x.aln, 16 * x.n_aln))
    k, l = struct.unpack_from("<II", rows, 4)
    struct.pack_into("<II", rows, 4, *change(k, l))
    hold = (C.c_uint8 * len(rows)).from_buffer_copy(bytes(rows))
    rec.read[0].aln = C.addressof(hold)
    return W.encode(L, rec)


def restore(world, msg):
    """a fresh batch of the message's records, and its state handed to nabwa_bam_batch_restore -> (rc, last error)"""
    L = world["L"]
    rc, rec, keep = W.decode(L, msg)
    assert rc == 0
    _, recs = bam_of(L, msg)
    buf, off = B.pack(recs)
    h = P()
    chk(L, L.nabwa_bam_batch_create(world["ix"]._h, C.byref(world["opt"]), C.byref(world["po"]), len(recs), T.ptr(buf), T.ptr(off), C.byref(h)))
    state = (W.WireRead * len(recs))(*[rec.read[e] for e in range(rec.kind)])
    rc = L.nabwa_bam_batch_restore(h, state)
    err = L.nabwa_last_error()
    L.nabwa_bam_batch_destroy(h)
    return rc, err


def test_rows_outside_the_index_never_reach_the_gpu(world, zlib, tmp_path):
    L = world["L"]
    seq_len = world["ix"].seq_len(0)
    first = pristine_messages(world)
    wk = new_worker(world)
    rc, pos = process(L, wk, first[:40])
    assert rc == 0
    L.nabwa_worker_destroy(wk)
    mapped = [m for m in pos if bam_of(L, m)[0].kind == 1 and bam_of(L, m)[0].read[0].n_aln > 0]             # single reads with a hit
    assert len(mapped) >= 3
    assert restore(world, mapped[0])[0] == 0                                     # what the library made itself goes in
    beyond = damaged(L, mapped[0], lambda k, l: (k, seq_len + 1))                # l beyond the BWT's last row
    crossed = damaged(L, mapped[1], lambda k, l: (l + 1, l))                     # k > l
    for m in (beyond, crossed):
        rc, err = restore(world, m)
        assert rc == nabwa.EINVAL and err == b"record 0: hit row outside the index", err
    edge = damaged(L, mapped[0], lambda k, l: (seq_len, seq_len))                # the last row there is: inside
    assert restore(world, edge)[0] == 0
    # through the executable: estimates are there from the start, so the records go to pass 2 -- and stop at its door
    scen = Z.write_scenario(tmp_path, world["config"], [mapped[2], beyond, crossed], ["send 3", "wait 3", "terminate"], isize=world["blob"])
    r = Z.run_worker(zlib, scen, ["-p", PORT], timeout=120)
    assert r.returncode == 1, r.stderr                                           # an error exit, not a signal
    assert b"record 1: hit row outside the index" in r.stderr
    assert b"illegal memory access" not in r.stderr and b"HSA_STATUS" not in r.stderr
    assert Z.replies(scen) == []                                                 # the batch was refused as a whole
    assert counts_line(r.stderr) == [0, 0, 0, 0]
