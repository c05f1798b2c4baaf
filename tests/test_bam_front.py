"""The BAM front-end's host-only units (csrc/bam_rec.hpp, bam_front.cpp, host_pool.cpp, read_trim.hpp) on the CPU, through
tests/emu/bam_front_main.cpp: built plain and with AddressSanitizer + UndefinedBehaviorSanitizer (every case runs in both), and with
ThreadSanitizer for the threaded case where g++ can build that.  The records come from a socket as well as from files
(nabwa_worker_process), so malformed ones must be refused without a byte read or written outside them.

Three yardsticks: today's messages for what is refused; a Python model (bam_front_lib, on bamlib) for everything; and for the well-formed
cases the answers of the reference's own read_bam_pair / bam_get_rg / bam1_to_seq, recorded in tests/golden/vectors_bam_front.npz by
tests/golden/make_golden_bam.py (--skip-duplicates is bam2bam.c's unique(), which cannot be compiled: model only)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bam_front_lib as F
import bamlib as B

GOLDEN = os.path.join(F.ROOT, "tests", "golden", "vectors_bam_front.npz")
BAD_REC, BAD_TAGS = "malformed BAM record", "malformed tags in a BAM record"


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_front")
    out = {}
    for name, flags in (("plain", []), ("asan_ubsan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        out[name] = str(d / name)
        r = F.build(out[name], *flags)
        assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def exe(request, exes):
    return exes[request.param]


@pytest.fixture(scope="module")
def exe_tsan(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bam_front_tsan") / "tsan")
    r = F.build(out, "-fsanitize=thread")
    if r.returncode != 0:
        pytest.skip("g++ here does not build with -fsanitize=thread: " + r.stderr.strip()[-300:])
    r = subprocess.run([out, "reg2bin", "0", "1"], capture_output=True, text=True, timeout=10)
    if r.returncode != 0 and "FATAL: ThreadSanitizer" in r.stderr:
        pytest.skip("ThreadSanitizer does not start on this machine: " + r.stderr.strip()[-300:])
    return out


@pytest.fixture(scope="module")
def cases():
    return F.well_formed_cases()


def same_front(got, want, what):
    assert got["rc"] == want["rc"], (what, got, want.get("msg"))
    if want["rc"]:
        assert got["msg"] == want["msg"], what
        return
    for k in ("kind", "first", "rg", "skip", "rg_names", "full_len", "seq", "rseq"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert got["recs"] == want["recs"], what


# ------------------------------------------------------------------ parse / refuse

def patched(r, at, fmt, value):
    b = bytearray(r)
    struct.pack_into(fmt, b, at, value)
    return bytes(b)


def malformed():
    ok = F.record("read", "ACGTACGT", [30] * 8, F.SU)
    with_tags = lambda t: F.record("read", "ACGTACGT", [30] * 8, F.SU, t)
    yield "shorter than 36 bytes", [ok[:35]], None, F.EINVAL, BAD_REC
    yield "block_size larger than the offsets say", [patched(ok, 0, "<I", len(ok))], None, F.EINVAL, BAD_REC
    yield "block_size smaller than the offsets say", [patched(ok, 0, "<I", len(ok) - 8)], None, F.EINVAL, BAD_REC
    yield "l_qname 0", [patched(ok, 12, "<B", 0)], None, F.EINVAL, BAD_REC
    yield "name without NUL inside l_qname", [patched(ok, 36 + 4, "<B", ord("x"))], None, F.EINVAL, BAD_REC
    yield "l_qseq negative", [patched(ok, 20, "<i", -1)], None, F.EINVAL, BAD_REC
    yield "l_qseq beyond the record", [patched(ok, 20, "<i", 9)], None, F.EINVAL, BAD_REC
    yield "n_cigar beyond the record", [patched(ok, 16, "<H", 1)], None, F.EINVAL, BAD_REC
    yield "tags cut after 1 byte", [with_tags(b"Z")], None, F.EINVAL, BAD_TAGS
    yield "tags cut after 2 bytes", [with_tags(b"ZZ")], None, F.EINVAL, BAD_TAGS
    yield "tag without its value", [with_tags(b"ZZi\1\2")], None, F.EINVAL, BAD_TAGS
    yield "Z tag without terminator", [with_tags(b"ZZZabc")], None, F.EINVAL, BAD_TAGS
    yield "B tag cut before its count", [with_tags(b"ZZBi\1\0")], None, F.EINVAL, BAD_TAGS
    yield "B tag whose count overruns the record", [with_tags(b"ZZBi" + struct.pack("<I", 3) + bytes(8))], None, F.EINVAL, BAD_TAGS
    yield "B tag with a count of 2^32 - 1 doubles", [with_tags(b"ZZBd" + struct.pack("<I", 0xffffffff) + bytes(8))], None, F.EINVAL, BAD_TAGS
    yield "a good record, then a bad one", [ok, with_tags(b"ZZZabc"), ok], None, F.EINVAL, BAD_TAGS


@pytest.mark.parametrize("what, recs, off, rc, msg", list(malformed()), ids=[m[0] for m in malformed()])
def test_malformed_records_are_refused(exe, tmp_path, what, recs, off, rc, msg):
    got = F.front(exe, tmp_path, recs, 0, 20, off=off)
    assert (got["rc"], got.get("msg")) == (rc, msg)


def test_unknown_type_letters(exe, tmp_path):
    """erase_tags takes a type letter it does not know as a tag without a value, as erase_unwanted_tags does (bwaseqio.c:432-454); get_rg stops
    at one, where bam_get_rg leaves the program (bamlite.c:196): the read group behind it is not seen"""
    t = b"ZQ?" + F.tag("NM", "i", bytes(4)) + F.tag("RG", "Z", b"g\0")
    got = F.front(exe, tmp_path, [F.record("r", "ACGT", [30] * 4, F.SU, t)], 0, 0)
    assert got["rc"] == 0 and F.split(got["recs"][0])["tags"] == b"ZQ?" + F.tag("RG", "Z", b"g\0") and got["rg_names"] == [b""]


# ------------------------------------------------------------------ the well-formed cases: model and reference

COMBOS = [(b, d, t) for b in (0, 1) for d in (0, 1) for t in (0, 20)]


@pytest.mark.parametrize("name", list(F.well_formed_cases()))
def test_create_stage_against_the_model_and_the_reference(exe, tmp_path, cases, name):
    gold = np.load(GOLDEN)
    recs = cases[name]
    assert gold["in_" + name].tobytes() == b"".join(recs) and gold["off_" + name].tolist() == F.offsets_of(recs).tolist(), "the fixture is of other cases: rerun make_golden_bam.py"
    for broken, drop, trim in COMBOS:
        flags = broken * F.BROKEN | drop * F.DROP
        got = F.front(exe, tmp_path, recs, flags, trim)
        same_front(got, F.model_front(recs, flags, trim), (name, flags, trim))
        r, logical = F.parse_ref(gold["ref_%s_%d%d_%d" % (name, broken, drop, trim)].tobytes())
        if r < 0:                                        # the reference stops at what it does not take; here the batch is refused as a whole
            assert got["rc"] == F.EINVAL, (name, flags)
            continue
        mates = [m for _, ms in logical for m in ms]
        assert got["rc"] == 0 and got["kind"] == [k for k, _ in logical], (name, flags)
        assert got["recs"] == [m["rec"] for m in mates], (name, flags)
        assert [got["rg_names"][g] for g in got["rg"]] == [ms[0]["rg"] for _, ms in logical], (name, flags)
        assert got["full_len"] == [m["full_len"] for m in mates] and [len(s) for s in got["seq"]] == [len(m["seq"]) for m in mates], (name, flags, trim)
        assert got["seq"] == [m["seq"] for m in mates] and got["rseq"] == [m["rseq"] for m in mates], (name, flags, trim)


def test_what_the_cases_reach(cases):
    """the cases are what their names say (model): every branch of read_bam_pair_core, erased and kept tags, read groups in first-seen order"""
    m = lambda name, flags=0, trim=0: F.model_front(cases[name], flags, trim)
    assert m("mates_in_order_and_reversed")["kind"] == [2, 2, 1, 2]
    assert [F.split(r)["flag"] & (F.R1 | F.R2) for r in m("mates_in_order_and_reversed")["recs"][2:4]] == [F.R1, F.R2]       # swapped
    assert m("wrong_read_flags")["msg"].startswith("a pair whose") and m("wrong_read_flags", F.BROKEN)["kind"] == [2, 2, 2, 1]
    assert m("lone_mate_in_mid_batch")["msg"].startswith("lone mate") and m("lone_mate_in_mid_batch", F.BROKEN)["kind"] == [2, 2, 1]
    assert m("lone_mate_before_singleton", F.BROKEN)["kind"] == [1, 2]
    assert m("paired_read_last")["msg"].startswith("a paired read at the end") and m("paired_read_last", F.BROKEN)["kind"] == [1, 2]
    assert m("mapped_ends")["kind"] == [2, 2, 2, 2, 1, 1] and m("mapped_ends", F.DROP)["kind"] == [2, 1]
    assert m("duplicates_and_qc", F.NODUP)["skip"] == [1, 0, 1, 1, 0] and m("duplicates_and_qc")["skip"] == [0] * 5
    assert [F.split(r)["flag"] & F.QC for r in m("duplicates_and_qc")["recs"]] == [0, 0, F.QC, F.QC, F.QC, F.QC, 0, F.QC]
    kept = [[k + ":" + t for _, k, t, _ in F.walk(F.split(r)["tags"])] for r in m("erase_and_keep")["recs"]]
    assert kept[0] == [] and kept[1] == kept[2] == ["XB:i", "AS:C", "MC:Z", "YS:s", "RG:Z", "ZB:B", "ZH:H"] and kept[3] == []
    assert [m("read_groups")["rg_names"][g] for g in m("read_groups")["rg"]] == [b"lib one", b"lib one", b"", b"x", b"", b"lib one", b"lib one", b"", b"first"]
    assert m("two_groups_alternating")["rg_names"] == [b"B", b"A", b""] and m("two_groups_alternating")["rg"] == [0, 1, 0, 0, 0, 1, 2]
    lens = {F.split(r)["name"][:-1].decode(): len(s) for r, s in zip(m("trim", 0, 20)["recs"], m("trim", 0, 20)["seq"])}
    assert (lens["trim60_none_4"], lens["trim60_floor_4"], lens["trim60_between_4"], lens["trim60_q255_20"], lens["trim34_floor_4"]) == (60, 35, 58, 49, 34)
    assert lens["trim36_floor_20"] == 35 and lens["trim35_floor_4"] == 35


def test_skip_duplicates(exe, tmp_path, cases):
    """NABWA_BAM_SKIP_DUPLICATES: a logical record with a flagged duplicate is marked and its reads are encoded with length 0 (model only)"""
    for flags in (F.NODUP, F.NODUP | F.BROKEN | F.DROP):
        for name in ("duplicates_and_qc", "mapped_ends", "lone_mate_in_mid_batch"):
            got = F.front(exe, tmp_path, cases[name], flags, 20)
            same_front(got, F.model_front(cases[name], flags, 20), (name, flags))
    got = F.front(exe, tmp_path, cases["duplicates_and_qc"], F.NODUP, 0)
    assert got["skip"] == [1, 0, 1, 1, 0] and [len(s) for s in got["seq"]] == [0, 0, 36, 36, 0, 0, 0, 40] and got["full_len"] == [36] * 6 + [40, 40]


def test_singletons_fast_path_against_the_general_loop(exe, tmp_path, cases):
    """single-end records and no flag that leaves records out: no loop over the records.  NABWA_BAM_DROP_ALIGNED on unmapped records changes
    nothing and sends the same input through the loop"""
    for name in ("singletons_only", "encode", "trim", "read_groups"):
        fast, loop = F.front(exe, tmp_path, cases[name], 0, 20, raw=True), F.front(exe, tmp_path, cases[name], F.DROP, 20, raw=True)
        assert fast == loop and F.parse_front(fast)["kind"] == [1] * len(cases[name]), name
    assert F.front(exe, tmp_path, [], 0, 20) == F.front(exe, tmp_path, [], F.DROP, 20) == F.model_front([], 0, 20)


# ------------------------------------------------------------------ threads

@pytest.fixture(scope="module")
def many():
    """20 000 records (BAM_MIN_N is 8192): pairs of two read groups, singletons, reverse flags, erased tags, mapped records, duplicates"""
    rng = np.random.default_rng(5)
    recs, i = [], 0
    junk = F.tag("NM", "i", bytes(4)) + F.tag("ZZ", "Z", b"kept\0") + F.tag("MD", "Z", b"40\0")
    while len(recs) < 20000:
        L = int(rng.integers(30, 64))
        q = lambda: rng.integers(2, 41, L).tolist()
        s = lambda: rng.integers(0, 16, L).tolist()
        t = (F.tag("RG", "Z", b"ab"[i % 3 % 2:i % 3 % 2 + 1] + b"\0") if i % 3 else b"") + (junk if i % 4 == 0 else b"")
        fl = F.SU * (i % 17 != 0) | F.SR * (i % 5 == 0) | F.DP * (i % 23 == 0)
        if i % 2 and len(recs) + 2 <= 20000:
            pair = [F.record("p%d" % i, s(), q(), fl | F.PD | F.R1, t), F.record("p%d" % i, s(), q(), fl | F.PD | F.R2 | F.QC * (i % 7 == 0), t)]
            recs += pair[::-1] if i % 9 == 0 else pair
        else:
            recs.append(F.record("s%d" % i, s(), q(), fl, t))
        i += 1
    return recs


def threaded(binary, tmp_path, recs):
    for flags in (0, F.BROKEN | F.DROP | F.NODUP):
        one = F.front(binary, tmp_path, recs, flags, 20, env={"NABWA_HOST_THREADS": "1"}, raw=True)
        four = F.front(binary, tmp_path, recs, flags, 20, env={"NABWA_HOST_THREADS": "4"}, raw=True)
        assert struct.unpack_from("<i", one, 0)[0] == 0 and one == four, flags
    return one


def test_four_threads_give_what_one_gives(exe, tmp_path, many):
    got = F.parse_front(threaded(exe, tmp_path, many))
    same_front(got, F.model_front(many, F.BROKEN | F.DROP | F.NODUP, 20), "20 000 records")
    assert 1 in got["kind"] and 2 in got["kind"] and 1 in got["skip"] and len(got["recs"]) < len(many)


def test_four_threads_under_thread_sanitizer(exe_tsan, tmp_path, many):
    threaded(exe_tsan, tmp_path, many)


# ------------------------------------------------------------------ the trim function

def test_one_trim_function_for_three_quality_domains(exe, tmp_path, cases):
    """bwa_trimmed_len in the domain of each of its callers -- the BAM front-end (phred, 255 capped at 93; forward and reverse-flagged), the
    tools' readers (phred + 33 characters, capped at 126) and nabwa_encode_read (raw phred) -- against the loop each of them had before"""
    quals = [F.split(r)["qual"] for r in cases["trim"]]
    with open(str(tmp_path / "q"), "wb") as f:
        f.write(b"".join(bytes(q) for q in quals))
    F.offsets_of([bytes(q) for q in quals]).tofile(str(tmp_path / "o"))
    differs = False
    for tq in (0, 1, 20, 40):
        rows = [[int(x) for x in l.split()] for l in F.run(exe, ["trim", tmp_path / "q", tmp_path / "o", tq]).splitlines()]
        assert len(rows) == len(quals)
        for q, (fwd, fwd0, rev, rev0, chars, chars0, raw, raw0) in zip(quals, rows):
            assert (fwd, rev, chars, raw) == (fwd0, rev0, chars0, raw0), (tq, q)
            cap = [min(x, 93) for x in q]
            differs = differs or fwd != raw
            if tq:
                assert (fwd, rev, chars, raw) == (F.model_trim(cap, tq), F.model_trim(cap[::-1], tq), F.model_trim(cap, tq), F.model_trim(q, tq)), (tq, q)
    assert differs, "no input on which the cap at 93 matters"


# ------------------------------------------------------------------ record edits

EDIT_LENGTHS = [0, 1, 2, 3, 4, 5, 511, 512, 513]          # 513: the first odd length whose bytes outgrow revcom_rec's 256-byte stack buffer


def edit(exe, tmp, recs, script):
    tmp = str(tmp)
    with open(os.path.join(tmp, "e.bytes"), "wb") as f:
        f.write(b"".join(recs))
    F.offsets_of(recs).tofile(os.path.join(tmp, "e.off"))
    with open(os.path.join(tmp, "e.script"), "w") as f:
        f.write("".join(l + "\n" for l in script))
    F.run(exe, ["edit", os.path.join(tmp, "e.bytes"), os.path.join(tmp, "e.off"), os.path.join(tmp, "e.script"), os.path.join(tmp, "e.out")])
    return F.parse_records(open(os.path.join(tmp, "e.out"), "rb").read(), 0, len(recs))[0]


def test_revcom(exe, tmp_path):
    rng = np.random.default_rng(7)
    tags = F.tag("ZZ", "Z", b"behind\0")
    recs = [F.record("r%d" % L, rng.integers(0, 16, L).tolist(), rng.integers(0, 94, L).tolist(), F.SU | (F.SR if L % 2 else 0), tags, cigar=[L << 4] if L % 3 == 0 else [])
            for L in EDIT_LENGTHS]
    once = edit(exe, tmp_path, recs, ["revcom"] * len(recs))
    assert once == [F.join(F.model_revcom(F.split(r))) for r in recs]
    assert edit(exe, tmp_path, recs, ["revcom;revcom"] * len(recs)) == recs
    want = [dict(F.model_revcom(F.split(r))) for r in recs]
    for w in want:
        w["tags"] += F.tag("XT", "A", b"U") + F.tag("NM", "i", struct.pack("<i", -7)) + F.tag("MD", "Z", b"10A5\0")
    assert edit(exe, tmp_path, recs, ["revcom;pushc XT U;pushi NM -7;pushs MD 10A5"] * len(recs)) == [F.join(w) for w in want]


def test_set_cigar_and_push(exe, tmp_path):
    """0 -> 64 operations are 256 bytes: more than REC_ROOM, the record's bytes move from the arena to the heap; the tags stay behind the CIGAR"""
    tags = F.tag("RG", "Z", b"grp\0") + F.tag("ZZ", "i", struct.pack("<i", 77))
    words = lambda n: [(i + 1) << 4 | i % 3 for i in range(n)]
    steps = [(0, 1), (1, 0), (1, 3), (3, 1), (0, 64), (3, 3), (64, 0)]
    recs = [F.record("c%d_%d" % s, "ACGTNACGTA", list(range(10)), F.SU, tags, cigar=[7 << 4 | 4] * s[0]) for s in steps]
    script = ["cigar %d %s;pushi X0 %d;pushc XT R;pushs XA chr1,+5,10M,0" % (n, " ".join(map(str, words(n))), 1 << 30) for _, n in steps]
    want = []
    for r, (_, n) in zip(recs, steps):
        d = F.split(r)
        d["cigar"] = words(n)
        d["tags"] += F.tag("X0", "i", struct.pack("<i", 1 << 30)) + F.tag("XT", "A", b"R") + F.tag("XA", "Z", b"chr1,+5,10M,0\0")
        want.append(F.join(d))
    got = edit(exe, tmp_path, recs, script)
    assert got == want
    # what write_rec wrote reads back through bamlib
    dec = B.decode(np.frombuffer(b"".join(got), np.uint8), F.offsets_of(got), [])
    for x, (_, n) in zip(dec, steps):
        assert x["seq"] == "ACGTNACGTA" and x["tags"] == {"RG": "grp", "ZZ": 77, "X0": 1 << 30, "XT": "R", "XA": "chr1,+5,10M,0"}
        assert x["order"] == ["RG:Z", "ZZ:i", "X0:i", "XT:A", "XA:Z"] and x["cigar"] == ("".join("%d%s" % (w >> 4, B.CIG[w & 15]) for w in words(n)) or "*")


def test_reg2bin(exe):
    pairs = [(0, 1)]
    for bits in (14, 17, 20, 23, 26):
        e = 1 << bits
        pairs += [(e - 10, e), (e - 10, e + 1), (e, e + 10), (e - 1, e + 1), (3 * e - 5, 3 * e), (3 * e - 5, 3 * e + 1)]
    pairs += [(0, 1 << 29), ((1 << 29) - 1, 1 << 29)]
    out = F.run(exe, ["reg2bin"] + [x for p in pairs for x in p]).split()
    assert [int(x) for x in out] == [F.reg2bin(b, e) for b, e in pairs]
    assert F.reg2bin(0, 1 << 14) == 4681 and F.reg2bin(0, (1 << 14) + 1) == 585 and F.reg2bin(0, (1 << 26) + 1) == 0
