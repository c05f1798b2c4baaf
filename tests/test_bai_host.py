"""What the BAM index (nabwa_bai_*, `nabwa_bam2bam --sort --index`) can be held to without a device.  First the oracle of tests/bai_cases.py
itself, which every other test of the index compares with: against one index written out by hand, and by what an index is for -- on a
BGZF file of small blocks, the records fetched through the oracle's index for a region are those a scan of the whole file finds, and a
narrow region inflates only a few of the file's blocks.  Then the library's host-only parts: the block table of a BGZF file, the argument
checks that come before the device is touched, the names of the counters, and the tool's refusals before the index is loaded."""
import ctypes as C
import importlib
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import bai_cases as M
import bamlib as B
import nabwa_testlib as T

nabwa = importlib.import_module("network-aware-bwa_amd")


def test_the_oracle_against_an_index_written_by_hand():
    """Four records behind a header of 100 bytes, in blocks that start at 0, 200 and 274 of the stream and at 0, 1000 and 1500 of the file;
    the end-of-file block at 374 and 2000.
      r0  reference 0, 100 .. 150      bytes 100 .. 217   bin 4681 (one window), starts in block 0 at 100, ends in block 1 at 17
      r1  reference 0, 16380 .. 16390  bytes 217 .. 274   bin 585 (windows 0 and 1), starts in block 1 at 17, ends where block 2 starts
      r2  reference 1, placed at 5, flag 0x4: one base    bytes 274 .. 324   bin 4681, block 2 at 0 .. 50
      r3  no reference                 bytes 324 .. 374"""
    recs = [M.rec(0, 100, "50M"), M.rec(0, 16380, "10M"), M.unmapped(1, 5, 4), M.unmapped()]
    assert [len(r) for r in recs] == [117, 57, 50, 50]
    b1, b2 = 1000 << 16, 1500 << 16
    want = (b"BAI\1" + struct.pack("<i", 2)
            # reference 0: two bins and the pseudo-bin, in rising bin number
            + struct.pack("<i", 3)
            + struct.pack("<IiQQ", 585, 1, b1 | 17, b2 | 0)
            + struct.pack("<IiQQ", 4681, 1, 100, b1 | 17)
            + struct.pack("<IiQQQQ", 37450, 2, 100, b2 | 0, 2, 0)
            + struct.pack("<iQQ", 2, 100, b1 | 17)             # window 0 is touched by r0 and r1: the lower start
            # reference 1
            + struct.pack("<i", 2)
            + struct.pack("<IiQQ", 4681, 1, b2 | 0, b2 | 50)
            + struct.pack("<IiQQQQ", 37450, 2, b2 | 0, b2 | 50, 0, 1)
            + struct.pack("<iQ", 1, b2 | 0)
            + struct.pack("<Q", 1))
    got, stats = M.oracle([(recs, 100)], 2, [0, 200, 274, 374], [0, 1000, 1500, 2000])
    assert got == want, M.describe(got)
    assert [int(x) for x in stats] == [4, 3, 1, 3, 3, 3, len(want)]
    # the same in two calls; and with r1 in a block of its own its bin is no other, but r0 now ends where that block starts
    assert M.oracle([(recs[:1], 100), (recs[1:], 217)], 2, [0, 200, 274, 374], [0, 1000, 1500, 2000])[0] == want
    other, _ = M.oracle([(recs, 100)], 2, [0, 217, 274, 374], [0, 1000, 1500, 2000])
    assert other == want.replace(struct.pack("<Q", b1 | 17), struct.pack("<Q", b1 | 0)) and other != want
    # a third reference without records, and nothing at all
    assert M.oracle([(recs[:2], 100)], 3, [0, 200, 274], [0, 1000, 1500])[0][-24:] == struct.pack("<iiiiQ", 0, 0, 0, 0, 0)
    assert M.oracle([], 1, [0], [0])[0] == b"BAI\1" + struct.pack("<iiiQ", 1, 0, 0, 0)


def test_the_chunk_rule_of_the_oracle():
    """two records of one bin with a record of another bin between them: one chunk where the second starts in the block in which the first
    ends, two where a block boundary lies between"""
    recs = [M.rec(0, 100, "20M", name=b"a1"), M.rec(0, 150, "20M20000N5M", name=b"b"), M.rec(0, 200, "20M", name=b"a2")]
    n = [len(r) for r in recs]
    total = 50 + sum(n)
    one = M.parse_bai(M.oracle([(recs, 50)], 1, [0, total], [0, 400])[0])[0][0][0]
    assert one[4681] == [(50, 400 << 16)] and one[585] == [(50 + n[0], 50 + n[0] + n[1])]
    cut = 50 + n[0] + 5                                        # a block boundary inside b
    two = M.parse_bai(M.oracle([(recs, 50)], 1, [0, cut, total], [0, 300, 400])[0])[0][0][0]
    assert two[4681] == [(50, 50 + n[0]), (300 << 16 | n[1] - 5, 400 << 16)]
    # a record that ends exactly where a block ends: its end is the next block's start, so the record behind it joins its chunk
    edge = M.parse_bai(M.oracle([(recs[::2], 50)], 1, [0, 50 + n[0], 50 + n[0] + n[2]], [0, 300, 400])[0])[0][0][0]
    assert edge[4681] == [(50, 400 << 16)]


@pytest.fixture(scope="module")
def small_blocks():
    """400 seeded sorted records on 4 references (one of them empty) behind a header, as a BGZF file of blocks of 100 .. 300 bytes"""
    recs = M.random_records(400, 11)
    header = b"BAM\1" + bytes(173)
    stream = header + b"".join(recs)
    ends, sizes, q = [len(header)], [], 0
    for r in recs:
        ends.append(ends[-1] + len(r))
    while q < len(stream):                                     # blocks of 100 .. 300 bytes; every tenth ends where a record ends
        s = [100, 300, 177, 256, 131][len(sizes) % 5]
        if len(sizes) % 10 == 3:
            s = next((e - q for e in ends if 100 <= e - q <= 300), s)
        sizes.append(s)
        q += s
    data = M.bgzf_pack(stream, sizes)
    u, c = M.block_table(data)
    assert u[-1] == len(stream) and len(u) > 150
    bai, stats = M.oracle([(recs, len(header))], 4, u, c)
    return recs, data, bai, stats


def test_records_fetched_through_the_index_are_those_of_a_scan(small_blocks):
    recs, data, bai, stats = small_blocks
    parsed = M.parse_bai(bai)
    assert parsed[1] == int(stats[M.NO_COOR]) > 5 and int(stats[M.CHUNKS]) > int(stats[M.BINS]) > 20
    placed = [r for r in recs if M.extent(r)[0] >= 0]
    ends = [0]
    for r in recs:
        ends.append(ends[-1] + len(r))
    u, _ = M.block_table(data)
    on_edge = sum(1 for e in ends if 177 + e in set(u.tolist()))
    assert on_edge >= 10                                       # records that end where a block ends, and start where one starts
    assert any(np.searchsorted(u, 177 + b, "right") - np.searchsorted(u, 177 + a, "right") >= 2 for a, b in zip(ends, ends[1:]))      # and records over three blocks
    rng = np.random.default_rng(5)
    n_hits = 0
    regions = [(t, 0, 1 << 29) for t in range(4)] + [(0, 16383, 16384), (0, 16384, 16385), (0, 0, 1)]
    while len(regions) < 110:
        t, beg = int(rng.integers(0, 4)), int(rng.integers(0, 320000))
        regions.append((t, beg, beg + int(rng.choice([1, 50, 3000, 40000, 200000]))))
    for t, beg, end in regions:
        f = M.Bgzf(data)
        got, want = M.query(parsed, f, t, beg, end), M.scan(placed, t, beg, end)
        assert got == want, "reference %d, %d .. %d: %d records through the index, %d by the scan" % (t, beg, end, len(got), len(want))
        n_hits += len(want)
    assert n_hits > 500 and M.scan(placed, 2, 0, 1 << 29) == [] and len(M.scan(placed, 0, 0, 1 << 29)) > 150


def test_a_narrow_region_inflates_few_blocks(small_blocks):
    """an index that names the whole file for every region would pass the test above"""
    recs, data, bai, _ = small_blocks
    parsed = M.parse_bai(bai)
    n_blocks = len(M.block_table(data)[0]) - 1
    placed = [r for r in recs if M.extent(r)[0] >= 0]
    for t, beg in ((0, 150000), (0, 299000), (1, 10), (3, 100000)):
        f = M.Bgzf(data)
        got = M.query(parsed, f, t, beg, beg + 2000)
        assert got == M.scan(placed, t, beg, beg + 2000)
        assert len(f.touched) < n_blocks // 2, "%d of %d blocks for 2000 bases" % (len(f.touched), n_blocks)


def test_block_table_of_a_bgzf_file():
    stream = bytes(range(256)) * 40
    for sizes in ([100, 300, 177], [65280], [1]):
        data = M.bgzf_pack(stream[:5000 if sizes == [1] else None], sizes)
        u, c = nabwa.bgzf_block_table(data)
        wu, wc = M.block_table(data)
        assert u.dtype == c.dtype == np.int64 and np.array_equal(u, wu) and np.array_equal(c, wc)
        assert u[-1] == nabwa.bgzf_inflated_size(data)[0] and c[-1] == len(data) - 28 and len(u) == nabwa.bgzf_inflated_size(data)[1]
    u, c = nabwa.bgzf_block_table(M.bgzf_pack(b"", [100]))
    assert u.tolist() == [0] and c.tolist() == [0]
    data = M.bgzf_pack(stream, [3000])
    for bad in (b"", data[:-28], data[:-1], data + b"x", b"x" + data):
        with pytest.raises(nabwa.NabwaError) as ex:
            nabwa.bgzf_block_table(bad)
        assert ex.value.code == nabwa.EDATA
    L = nabwa.lib()
    a, n = np.frombuffer(data, np.uint8), C.c_int64()
    few = np.zeros(3, np.int64)
    assert L.nabwa_bgzf_block_table(T.ptr(a), a.size, T.ptr(few), None, 3, C.byref(n)) == nabwa.ECAP and n.value == len(nabwa.bgzf_block_table(data)[0]) - 1
    assert L.nabwa_bgzf_block_table(T.ptr(a), a.size, None, None, 0, None) == nabwa.EINVAL


def test_counter_names():
    assert nabwa.bai_stat_names == M.STAT_NAMES
    text = open(os.path.join(T.ROOT, "include", "nabwa.h")).read()
    body = re.search(r"enum \{ (NABWA_BAI_STAT_RECORDS = 0,.*?NABWA_BAI_N_STATS) \};", text, re.S).group(1)
    names = [x.strip().split(" ")[0] for x in body.split(",")]
    assert names == ["NABWA_BAI_STAT_" + n.upper() for n in M.STAT_NAMES] + ["NABWA_BAI_N_STATS"]


def test_argument_checks_come_before_the_device():
    L = nabwa.lib()
    h = C.c_void_p(0x1234)
    assert L.nabwa_bai_create(0, 3, None) == nabwa.EINVAL
    assert L.nabwa_bai_create(1 << 20, -1, C.byref(h)) == nabwa.EINVAL and not h.value and b"n_ref" in L.nabwa_last_error()
    data, off = B.pack(M.good_records(5))
    out = np.zeros(16, np.uint64)
    tab = np.array([0, 100, 200], np.int64)
    assert L.nabwa_bai_add(None, 5, T.ptr(data), T.ptr(off), 0) == nabwa.EINVAL
    assert L.nabwa_bai_finish(None, 2, T.ptr(tab), T.ptr(tab), None, 0, None, None) == nabwa.EINVAL
    assert L.nabwa_bai_clear(None) == nabwa.EINVAL
    assert L.nabwa_bai_times(None, T.ptr(out)) == nabwa.EINVAL
    L.nabwa_bai_destroy(None)
    # what nabwa_bai_add decides from its other arguments comes before the handle is looked at: `some` is never read
    some = C.create_string_buffer(4096)
    assert L.nabwa_bai_add(some, -1, T.ptr(data), T.ptr(off), 0) == nabwa.EINVAL and b"n_rec" in L.nabwa_last_error()
    assert L.nabwa_bai_add(some, 1 << 31, T.ptr(data), T.ptr(off), 0) == nabwa.EINVAL and b"n_rec" in L.nabwa_last_error()
    assert L.nabwa_bai_add(some, 5, None, T.ptr(off), 0) == nabwa.EINVAL
    assert L.nabwa_bai_add(some, 5, T.ptr(data), None, 0) == nabwa.EINVAL
    bad = off.copy(); bad[0] = -1
    assert L.nabwa_bai_add(some, 5, T.ptr(data), T.ptr(bad), 0) == nabwa.EINVAL and b"negative" in L.nabwa_last_error()
    bad = off.copy(); bad[3] = bad[2]
    assert L.nabwa_bai_add(some, 5, T.ptr(data), T.ptr(bad), 0) == nabwa.EINVAL and b"record 2" in L.nabwa_last_error()
    bad = off.copy(); bad[3] = bad[2] + 35
    assert L.nabwa_bai_add(some, 5, T.ptr(data), T.ptr(bad), 0) == nabwa.EINVAL and b"at least 36" in L.nabwa_last_error()
    assert L.nabwa_bai_add(some, 5, T.ptr(data), T.ptr(off), -1) == nabwa.EINVAL and b"stream_off" in L.nabwa_last_error()
    assert L.nabwa_bai_times(some, None) == nabwa.EINVAL
    for args in ((None, T.ptr(tab)), (T.ptr(tab), None)):
        assert L.nabwa_bai_finish(some, 2, args[0], args[1], None, 0, None, None) == nabwa.EINVAL
    assert L.nabwa_bai_finish(some, 2, T.ptr(tab), T.ptr(tab), None, -1, None, None) == nabwa.EINVAL
    assert L.nabwa_bai_finish(some, 2, T.ptr(tab), T.ptr(tab), None, 5, None, None) == nabwa.EINVAL
    assert L.nabwa_bai_finish(some, -1, T.ptr(tab), T.ptr(tab), None, 0, None, None) == nabwa.EINVAL and b"n_blk" in L.nabwa_last_error()
    for u, c, word in (([0, 100, 99], [0, 50, 60], b"blk_uoff falls at block 1"), ([0, 100, 200], [0, 50, 50], b"blk_coff does not rise at block 1"), ([0, 100, 200], [0, 50, 49], b"blk_coff"),
                       ([0, 65537, 65540], [0, 50, 60], b"block 0 holds 65537"), ([0, 100, 200], [0, 50, 1 << 48], b"48 bits"), ([-1, 100, 200], [0, 50, 60], b"below 0")):
        r = L.nabwa_bai_finish(some, 2, T.ptr(np.array(u, np.int64)), T.ptr(np.array(c, np.int64)), None, 0, None, None)
        assert r == nabwa.EINVAL and word in L.nabwa_last_error(), (u, c, L.nabwa_last_error())


def test_tool_says_no_before_the_index_is_loaded(tmp_path):
    exe = os.path.join(os.path.dirname(nabwa.LIB_PATH), "nabwa_bam2bam")
    if not os.path.exists(exe):
        nabwa.build()
    outp = str(tmp_path / "out.bam")
    base = {k: v for k, v in os.environ.items() if not k.startswith("NABWA_")}

    def tool(args, env):
        return subprocess.run([exe, "-g", T.TOY] + args + [str(tmp_path / "no_such.bam")], capture_output=True, text=True, env=dict(base, **env), timeout=120)
    r = tool(["-f", outp, "--index"], {})
    assert r.returncode == 1 and "--index needs --sort" in r.stderr and "genome length" not in r.stderr, r.stderr
    r = tool(["--sort", "--index"], {})
    assert r.returncode == 1 and "--index needs -f" in r.stderr and "genome length" not in r.stderr and r.stdout == "", r.stderr
    r = tool(["--index"], {})
    assert r.returncode == 1 and "--index needs" in r.stderr and r.stdout == ""
    for env in ({}, {"NABWA_SORT": "host"}):                  # no usable device: nothing is written, and no host path takes over
        r = tool(["-f", outp, "--sort", "--index"], dict(env, NABWA_DEVICES=str(1 << 20)))
        assert r.returncode == 2 and ("--index" if env else "--sort") + " on the GPU" in r.stderr and "genome length" not in r.stderr, r.stderr      # (the sort's own handle comes first)
    assert not os.path.exists(outp) and not os.path.exists(outp + ".bai") and os.listdir(str(tmp_path)) == []
    r = subprocess.run([exe], capture_output=True, text=True, env=base, timeout=120)
    assert r.returncode == 1 and "--index" in r.stderr and ".bai" in r.stderr and "no host" in r.stderr
