"""The bodies of the BAM coordinate sort (csrc/bam_sort_body.hpp) on the CPU (tests/emu/bam_sort_emu.cpp): the key of a record at every
byte alignment, the copy of one record by its group of 16 lanes for every pair of source and destination alignment, and the whole stage
against the NumPy oracle on the inputs of tests/test_gpu_bam_sort.py.  Also what needs no device of the library and the tool: the
argument checks of nabwa_bam_sort*, the NABWA_SORT=host sort and the merge of runs (csrc/bam_sort_host.hpp), and the header text."""
import ctypes as C
import importlib
import os
import struct
import subprocess

import numpy as np
import pytest

import bam_sort_cases as S
import nabwa_testlib as T

nabwa = importlib.import_module("network-aware-bwa_amd")


@pytest.fixture(scope="module")
def emu():
    return S.load_emu()


def at_alignment(n_bytes, residue, slack=64):
    """a uint8 array of n_bytes whose first byte lies at `residue` mod 16, with `slack` bytes of its buffer on either side -> (buffer, start)"""
    buf = np.zeros(n_bytes + 2 * slack + 16, np.uint8)
    start = slack + (residue - (buf.ctypes.data + slack)) % 16
    assert (buf.ctypes.data + start) % 16 == residue
    return buf, start


def test_keys_at_every_byte_offset(emu):
    assert nabwa.bam_sort_key(-1, -1) == 0xffffffff00000000 and nabwa.bam_sort_key(0, -1) == 0 and nabwa.bam_sort_key(0, 0) == 1
    for a in range(16):
        for tid in S.KEY_TIDS:
            for pos in S.KEY_POSS:
                buf, st = at_alignment(36, a)
                buf[st:st + 36] = np.frombuffer(S.record(tid, pos, 36, 1), np.uint8)
                got = emu.emu_bsort_key(buf.ctypes.data + st)
                assert got == nabwa.bam_sort_key(tid, pos) == S.key_of(tid, pos), (a, tid, pos)
    # the order the keys give: a real tid by pos with -1 first, unmapped without a place last
    ks = [nabwa.bam_sort_key(t, p) for t, p in [(0, -1), (0, 0), (0, 2 ** 31 - 2), (1, -1), (2 ** 31 - 1, 5), (-1, -1), (-1, 0)]]
    assert ks == sorted(ks) and len(set(ks)) == len(ks)


@pytest.mark.parametrize("size", S.COPY_SIZES)
def test_record_copy_at_every_pair_of_alignments(emu, size):
    rng = np.random.default_rng(size)
    payload = rng.integers(0, 256, size, dtype=np.uint8)
    for sa in range(16):
        src, ss = at_alignment(size, sa, slack=0)
        src[ss:ss + size] = payload
        for da in range(16):
            dst, ds = at_alignment(size, da)
            dst[:] = 0xa5
            emu.emu_bsort_copy(src.ctypes.data + ss, dst.ctypes.data + ds, size, (sa ^ da) & 1)
            assert dst[ds:ds + size].tobytes() == payload.tobytes(), (size, sa, da)
            assert (dst[:ds] == 0xa5).all() and (dst[ds + size:] == 0xa5).all(), ("guard bytes", size, sa, da)


def check_stage(emu, recs, what):
    data, off = S.join(recs)
    bad, got, got_off, got_keys = S.emu_run(emu, data, off)
    want, want_off, want_keys = S.oracle(data, off)
    assert bad == -1, what
    S.assert_same_records(got, got_off, want, want_off, what)
    assert got_keys.tolist() == want_keys.tolist(), what


def test_whole_stage_against_the_oracle(emu):
    for n in S.N_RECS:
        if n <= 257:
            check_stage(emu, S.mixed(n, seed=n + 1), "n_rec %d" % n)
    for lead in range(36, 52):
        check_stage(emu, S.with_lead(S.mixed(40, seed=lead), lead), "lead %d" % lead)
    for name, recs in S.named_cases():
        check_stage(emu, recs, name)


def test_stage_flags_the_lowest_bad_block_size(emu):
    recs = S.mixed(50, seed=4)
    data, off = S.join(recs)
    data = data.copy()
    for k in (31, 12):
        data[off[k]:off[k] + 4] = np.frombuffer(struct.pack("<I", len(recs[k]) - 4 + 1), np.uint8)
        assert S.emu_run(emu, data, off)[0] == k


# ---------------------------------------------------------------------------------------------------------------- the library without a device
def raw_sort(n, data, off, out, cap, device=0, out_off=None, keys=None):
    return nabwa.lib().nabwa_bam_sort(device, n, T.ptr(data) if data is not None else None, T.ptr(off) if off is not None else None,
                                      T.ptr(out) if out is not None else None, cap, T.ptr(out_off) if out_off is not None else None, T.ptr(keys) if keys is not None else None)


def test_argument_checks_come_before_the_device():
    """device 1 << 20 does not exist: an answer other than EINVAL / ECAP would mean the device was looked for first"""
    data, off = S.join(S.mixed(5, seed=2))
    out = np.zeros(len(data), np.uint8)
    nowhere = 1 << 20
    assert raw_sort(5, None, off, out, len(out), nowhere) == nabwa.EINVAL
    assert raw_sort(5, data, None, out, len(out), nowhere) == nabwa.EINVAL
    assert raw_sort(5, data, off, None, len(out), nowhere) == nabwa.EINVAL
    assert raw_sort(-1, data, off, out, len(out), nowhere) == nabwa.EINVAL
    assert raw_sort(1 << 31, data, off, out, len(out), nowhere) == nabwa.EINVAL
    flat = off.copy(); flat[3] = flat[2]
    assert raw_sort(5, data, flat, out, len(out), nowhere) == nabwa.EINVAL and b"record 2" in nabwa.lib().nabwa_last_error()
    back = off.copy(); back[3] = back[2] - 1
    assert raw_sort(5, data, back, out, len(out), nowhere) == nabwa.EINVAL
    short = np.array([0, 40, 75, 120], np.int64)
    assert raw_sort(3, data, short, out, len(out), nowhere) == nabwa.EINVAL and b"record 1 has 35 bytes" in nabwa.lib().nabwa_last_error()
    assert raw_sort(5, data, off, out, len(data) - 1, nowhere) == nabwa.ECAP and str(len(data)).encode() in nabwa.lib().nabwa_last_error()
    assert raw_sort(0, None, np.zeros(1, np.int64), None, 0, nowhere) == nabwa.OK                 # nothing to sort, nothing written, no device needed
    assert nabwa.lib().nabwa_bam_sort_run(None, 5, T.ptr(data), T.ptr(off), T.ptr(out), len(out), None, None) == nabwa.EINVAL
    assert nabwa.lib().nabwa_bam_sort_create(0, None) == nabwa.EINVAL
    with pytest.raises(nabwa.NabwaError) as e:
        nabwa.bam_sort(data.tobytes(), device=nowhere, cap=len(data) - 1)
    assert e.value.code == nabwa.ECAP and e.value.needed == len(data)


# ---------------------------------------------------------------------------------------------------------------- the tool's host half
def host_sort(exe, tmp_path, data, threads, run_bytes):
    p = str(tmp_path / "records.bin")
    open(p, "wb").write(bytes(data))
    r = subprocess.run([exe, p, str(threads), str(run_bytes)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    runs = int([l for l in r.stderr.decode().split("\n") if l.startswith("runs ")][0].split()[1])
    return r.stdout, runs


def runs_of(off, run_bytes):
    """a run is closed by the record that brings it to run_bytes (0: one run)"""
    runs, start = 0, 0
    for i in range(len(off) - 1):
        if run_bytes > 0 and off[i + 1] - off[start] >= run_bytes:
            runs, start = runs + 1, i + 1
    return runs + (1 if start < len(off) - 1 else 0)


def test_host_sort_and_merge_of_runs(tmp_path):
    """NABWA_SORT=host and the merge: any run size and any number of threads give the stable sort of the whole"""
    exe = S.build_host_main()
    cases = [("mixed 3000", S.mixed(3000, seed=21))] + S.named_cases()
    for name, recs in cases:
        data, off = S.join(recs)
        want, want_off, _ = S.oracle(data, off)
        for threads, run_bytes in ((1, 0), (5, 0), (16, 0), (3, 1 << 14), (4, 4000), (2, 1)):
            got, runs = host_sort(exe, tmp_path, data.tobytes(), threads, run_bytes)
            S.assert_same_records(got, S.offsets_of(got), want, want_off, (name, threads, run_bytes))
            assert runs == runs_of(off, run_bytes), (name, threads, run_bytes)


def test_header_says_coordinate_only_with_the_flag():
    exe = S.build_header_main()
    old = "@HD\tVN:1.0\tSO:unsorted\n@SQ\tSN:stale\tLN:5\n@RG\tID:lib1\tSM:x\n@PG\tID:first\tPN:demux\n@PG\tID:bwa\tPN:bwa\tPP:first\n@CO\tkept as it is\n"
    args = ["VER", "chrA:1000,chrB:25", "nabwa_bam2bam", "-g", "toy", "in.bam"]
    rest = "@PG\tID:bwa-1\tPP:bwa\tPN:bwa\tVN:VER\tCL:nabwa_bam2bam -g toy in.bam\n@SQ\tSN:chrA\tLN:1000\n@SQ\tSN:chrB\tLN:25\n" \
           "@RG\tID:lib1\tSM:x\n@PG\tID:first\tPN:demux\n@PG\tID:bwa\tPN:bwa\tPP:first\n@CO\tkept as it is\n"
    plain = subprocess.run([exe] + args, input=old, capture_output=True, text=True, check=True).stdout
    assert plain == "@HD\tVN:1.4\n" + rest                         # what tests/test_gpu_bam2bam_cli.py pins for the tool, byte for byte
    coord = subprocess.run([exe, "--coordinate"] + args, input=old, capture_output=True, text=True, check=True).stdout
    assert coord == "@HD\tVN:1.4\tSO:coordinate\n" + rest


def test_tool_says_no_before_anything_is_loaded_or_written(tmp_path):
    """values the tool refuses exit 1 before the index is loaded; --sort on a GPU that is not there exits 2 before anything is written;
    without --sort neither variable is read"""
    exe = os.path.join(os.path.dirname(nabwa.LIB_PATH), "nabwa_bam2bam")
    if not os.path.exists(exe):
        nabwa.build()
    outp = str(tmp_path / "out.bam")
    base = {k: v for k, v in os.environ.items() if not k.startswith("NABWA_")}

    def tool(args, env):
        return subprocess.run([exe, "-g", T.TOY, "-f", outp] + args + [str(tmp_path / "no_such.bam")], capture_output=True, text=True, env=dict(base, **env), timeout=120)
    for env, word in (({"NABWA_SORT": "fast"}, "NABWA_SORT=fast: gpu or host"), ({"NABWA_SORT_RUN_MIB": "0"}, "NABWA_SORT_RUN_MIB=0"), ({"NABWA_SORT_RUN_MIB": "1.5"}, "NABWA_SORT_RUN_MIB=1.5")):
        r = tool(["--sort"], env)
        assert r.returncode == 1 and word in r.stderr and "genome length" not in r.stderr, r.stderr
    r = tool(["--sort"], {"NABWA_DEVICES": str(1 << 20)})
    assert r.returncode == 2 and "--sort on the GPU" in r.stderr, r.stderr
    r = tool([], {"NABWA_SORT": "fast", "NABWA_SORT_RUN_MIB": "0", "NABWA_DEVICES": str(1 << 20)})
    assert "NABWA_SORT" not in r.stderr and "--sort" not in r.stderr and r.returncode != 0      # (it ends at the index: no such device)
    assert not os.path.exists(outp)
