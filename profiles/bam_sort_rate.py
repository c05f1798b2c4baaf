"""What `nabwa_bam2bam --sort` costs: the sort stage on its own, and file to file.

    python profiles/bam_sort_rate.py stage [--mib 1024] [--repeats 5] [--threads 16]
    python profiles/bam_sort_rate.py files [--parent-exe PATH/nabwa_bam2bam] [--rounds 4] [--se 8000000] [--pe 4000000] [--dir /tmp/bam_sort_rate]

stage: one run of --mib MiB of finished single-end 100 bp records, made from seed 20261020 -- every record 235 bytes (the 36 fixed bytes, a
9-character name, one CIGAR operation 100M, 50 + 100 bytes of bases and qualities, XT NM X0 X1 XM XO XG and MD:Z:100), 99 % of them placed
uniformly over the 24 primary contigs of GRCh38 by their lengths (a draw over the 3.09 G bases, cut at the contig starts), 1 % unmapped
(refID -1, pos -1), in the order of the draw, which is the order reads come in.  nabwa_bam_sort_run on one handle: one warm-up call, then
--repeats calls; per call the six device-event times of nabwa_bam_sort_times and the wall time of the call; the output of the last call is
compared with NumPy's stable sort.  Then the host path for the same run: csrc/bam_sort_host.hpp as tests/emu/bam_sort_host_main.cpp
builds it, --threads threads, one warm-up and --repeats timed sorts inside one process.

files: the 8 M single-end and 4 M paired reads of profiles/r03_cli_rate.txt (100 bp reads drawn from the toy genome under seed 7 with 1 %
substitutions, mates 300 +- 30 bp apart, a true BGZF file; profiles/probes/cli_rate.py made those) through four configurations -- the parent
commit's nabwa_bam2bam (--parent-exe), this tree's without --sort, with --sort under NABWA_SORT=gpu and under NABWA_SORT=host -- in turn,
--rounds rounds, each round starting with another configuration, wall time of each command.  The records of parent and this tree without
--sort must inflate to the same bytes (the headers' @PG lines name the program), and so must the records of the two sorted outputs.  Nothing here reads anything outside the repository."""
import argparse
import ctypes as C
import hashlib
import importlib
import os
import re
import struct
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRCH38 = [248956422, 242193529, 198295559, 190214555, 181538259, 170805979, 159345973, 145138636, 138394717, 133797422, 135086622, 133275309,
          114364328, 107043718, 101991189, 90338345, 83257441, 80373285, 58617616, 64444167, 46709983, 50818468, 156040895, 57227415]
REC = 235                 # bytes of a finished record of the stage run
HBM_PEAK = 8.0e12             # MI355X_MICROARCH.md: HBM3E peak BW, spec
HBM_COPY = 6.29e12            # ... and the float4 copy measured there


def f3(v, fmt="%.2f"):
    v = sorted(v)
    return " ".join(fmt % x for x in (v[0], v[len(v) // 2], v[-1]))


def finished_records(n, seed):
    """n finished single-end 100 bp records of REC bytes -> (n, REC) uint8"""
    rng = np.random.default_rng(seed)
    tags = b"XTAU" + b"NMC\0" + b"X0C\1" + b"X1C\0" + b"XMC\0" + b"XOC\0" + b"XGC\0" + b"MDZ100\0"
    size = 36 + 10 + 4 + 50 + 100 + len(tags)
    assert size == REC
    rec = np.zeros((n, size), np.uint8)
    starts = np.concatenate([[0], np.cumsum(GRCH38)])
    g = rng.integers(0, starts[-1] - 100 * len(GRCH38), n)
    tid = np.searchsorted(starts, g, side="right") - 1
    pos = np.minimum(g - starts[tid], np.array(GRCH38)[tid] - 100)
    unmapped = rng.random(n) < 0.01
    tid[unmapped] = -1
    pos[unmapped] = -1
    rec[:, 0:4] = np.frombuffer(struct.pack("<I", size - 4), np.uint8)
    rec[:, 4:8] = tid.astype("<i4").view(np.uint8).reshape(n, 4)
    rec[:, 8:12] = pos.astype("<i4").view(np.uint8).reshape(n, 4)
    rec[:, 12:36] = np.frombuffer(struct.pack("<IIiiii", (4680 << 16) | (37 << 8) | 10, 1, 100, -1, -1, 0), np.uint8)
    rec[unmapped, 18] = 4
    rec[~unmapped, 18] = (rng.integers(0, 2, int((~unmapped).sum())) * 16).astype(np.uint8)
    rec[:, 36] = ord("r")
    rec[:, 37:45] = np.frombuffer("".join(np.char.zfill(np.arange(n).astype("U8"), 8)).encode(), np.uint8).reshape(n, 8)
    rec[:, 46:50] = np.frombuffer(struct.pack("<I", 100 << 4), np.uint8)
    rec[:, 50:100] = rng.integers(0, 256, (n, 50), dtype=np.uint8) & 0x33 | 0x11      # (any bases)
    rec[:, 100:200] = rng.integers(2, 41, (n, 100), dtype=np.uint8)
    rec[:, 200:] = np.frombuffer(tags, np.uint8)
    return rec


def stage(args):
    sys.path.insert(0, ROOT)
    nabwa = importlib.import_module("network-aware-bwa_amd")
    n = (args.mib << 20) // REC
    rec = finished_records(n, 20261020)
    total = rec.size
    off = (np.arange(n + 1, dtype=np.int64) * REC)
    out = np.empty(total, np.uint8)
    out_off, keys = np.zeros(n + 1, np.int64), np.zeros(n, np.uint64)
    L = nabwa.lib()
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    print("one run: %d records of 235 bytes, %.1f MiB, seed 20261020" % (n, total / 2 ** 20), flush=True)
    names = ["upload", "key kernel", "radix sort", "sizes + scan", "gather kernel", "download"]
    ev, wall = [], []
    with nabwa.BamSort(0) as s:
        for rep in range(1 + args.repeats):
            t0 = time.time()
            rc = L.nabwa_bam_sort_run(s._h, n, P(rec), P(off), P(out), total, P(out_off), P(keys))
            dt = time.time() - t0
            assert rc == 0, L.nabwa_last_error()
            if rep:                                   # the first call allocates and warms
                ev.append(s.times())
                wall.append(1e3 * dt)
    k = (rec[:, 4:8].copy().view("<u4")[:, 0].astype(np.uint64) << np.uint64(32)) | ((rec[:, 8:12].copy().view("<i4")[:, 0].astype(np.int64) + 1).astype(np.uint64) & np.uint64(0xffffffff))
    order = np.argsort(k, kind="stable")
    ok = bool((keys == k[order]).all()) and bool((out.reshape(n, REC)[:, 36:46] == rec[order][:, 36:46]).all()) and bool((out_off == off).all())
    same = bool((out.reshape(n, REC) == rec[order]).all())
    print("output against np.argsort(keys, kind='stable'): %s" % ("equal, record for record" if ok and same else "DIFFERS"))
    print("\nGPU path, %d calls after one warm-up call, ms (min med max):" % args.repeats)
    for i, nm in enumerate(names):
        print("  %-14s %s" % (nm, f3([e[i] for e in ev], "%.3f")))
    print("  %-14s %s" % ("all six", f3([sum(e) for e in ev], "%.3f")))
    print("  %-14s %s" % ("wall, the call", f3(wall, "%.1f")))
    g = sorted(e[4] for e in ev)[len(ev) // 2]
    rate = 2 * total / (g * 1e-3)
    print("  gather kernel: 2 x %.1f MiB moved in %.3f ms (median) = %.2f TB/s = %.0f %% of the HBM peak of MI355X_MICROARCH.md (8.0 TB/s, spec; %.0f %% of the 6.29 TB/s its float4 copy reaches)"
          % (total / 2 ** 20, g, rate / 1e12, 100 * rate / HBM_PEAK, 100 * rate / HBM_COPY))
    up = sorted(e[0] for e in ev)[len(ev) // 2]
    dn = sorted(e[5] for e in ev)[len(ev) // 2]
    print("  upload %.1f GB/s, download %.1f GB/s (pageable host memory)" % (total / up / 1e6, total / dn / 1e6))
    # the host path
    tmp = tempfile.mkdtemp(prefix="bam_sort_rate_")
    exe = os.path.join(tmp, "bam_sort_host_main")
    subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "emu", "bam_sort_host_main.cpp"), "-o", exe, "-lpthread"], check=True)
    path = os.path.join(tmp, "records.bin")
    rec.tofile(path)
    r = subprocess.run([exe, path, str(args.threads), "0", str(1 + args.repeats)], capture_output=True, text=True)
    os.remove(path)
    assert r.returncode == 0, r.stderr[-2000:]
    ms = [float(x) for x in re.findall(r"sort_ms ([0-9.]+)", r.stderr)][1:]
    print("\nhost path (bam_sort_host, %d threads), %d sorts after one warm-up, ms (min med max): %s" % (args.threads, len(ms), f3(ms, "%.1f")))


# ---------------------------------------------------------------------------------------------------------------- file to file
def bgzf_block(chunk):
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    d = c.compress(chunk) + c.flush()
    return bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0]) + struct.pack("<H", len(d) + 25) + d + struct.pack("<II", zlib.crc32(chunk), len(chunk))


def write_input(path, n, paired):
    """the input of profiles/probes/cli_rate.py"""
    fa = "".join(l.strip() for l in open(os.path.join(ROOT, "tests", "golden", "toy.fa")) if not l.startswith(">"))
    g = np.frombuffer(fa.upper().encode(), np.uint8)
    code = np.full(256, 15, np.uint8); code[ord("A")] = 1; code[ord("C")] = 2; code[ord("G")] = 4; code[ord("T")] = 8
    g16 = code[g]
    rng = np.random.default_rng(7)
    L = 100
    start = rng.integers(0, len(g16) - L - 400, n)
    if paired:
        start[1::2] = start[0::2] + 300 + rng.integers(-30, 30, n // 2)
    reads = g16[start[:, None] + np.arange(L)[None, :]]
    if paired:
        comp = np.zeros(16, np.uint8); comp[[1, 2, 4, 8, 15]] = [8, 4, 2, 1, 15]
        reads[1::2] = comp[reads[1::2, ::-1]]
    sub = rng.random((n, L)) < 0.01
    reads[sub] = np.array([1, 2, 4, 8], np.uint8)[rng.integers(0, 4, int(sub.sum()))]
    rec_len = 36 + 10 + L // 2 + L
    rec = np.zeros((n, rec_len), np.uint8)
    rec[:, 0:4] = np.frombuffer(struct.pack("<I", rec_len - 4), np.uint8)
    rec[:, 4:36] = np.frombuffer(struct.pack("<iiIIiiii", -1, -1, (4680 << 16) | 10, 4 << 16, L, -1, -1, 0), np.uint8)
    rec[:, 36] = ord("r")
    ids = np.arange(n) // 2 * 2 if paired else np.arange(n)
    rec[:, 37:45] = np.frombuffer("".join(np.char.zfill(ids.astype("U8"), 8)).encode(), np.uint8).reshape(n, 8)
    if paired:
        rec[0::2, 18] = 1 | 4 | 8 | 64; rec[1::2, 18] = 1 | 4 | 8 | 128
    rec[:, 46:46 + L // 2] = (reads[:, 0::2] << 4) | reads[:, 1::2]
    rec[:, 46 + L // 2:] = 40
    text = b"@HD\tVN:1.0\n"
    raw = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", 0) + rec.tobytes()
    view = memoryview(raw)
    chunks = [view[o:o + 0xff00] for o in range(0, len(raw), 0xff00)]
    with ThreadPoolExecutor(16) as ex, open(path, "wb") as f:
        for b in ex.map(lambda c: bgzf_block(bytes(c)), chunks, chunksize=64):
            f.write(b)
        f.write(bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0, 27, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0]))


def header_bytes(raw):
    """the length of the BAM header at the start of raw, or None while raw is too short to say"""
    if len(raw) < 12:
        return None
    p = 8 + struct.unpack_from("<i", raw, 4)[0]
    if len(raw) < p + 4:
        return None
    n_ref = struct.unpack_from("<i", raw, p)[0]
    p += 4
    for _ in range(n_ref):
        if len(raw) < p + 4:
            return None
        p += 4 + struct.unpack_from("<i", raw, p)[0] + 4
    return p if len(raw) >= p else None


def records_digest(path):
    """SHA-256 of the inflated records of a BAM file: everything behind the header (whose @PG line names the program and the files)"""
    h = hashlib.sha256()
    d = zlib.decompressobj(31)
    head = b""
    with open(path, "rb") as f:
        while True:
            b = f.read(1 << 24)
            if not b:
                break
            while b:
                piece = d.decompress(b)
                if head is not None:
                    head += piece
                    n = header_bytes(head)
                    piece = b"" if n is None else head[n:]
                    head = head if n is None else None
                h.update(piece)
                b = d.unused_data
                if d.eof:
                    d = zlib.decompressobj(31)
    assert head is None, "no whole BAM header in %s" % path
    return h.hexdigest()


def files(args):
    os.makedirs(args.dir, exist_ok=True)
    this = os.path.join(ROOT, "network-aware-bwa_amd", "nabwa_bam2bam")
    confs = ([("parent", args.parent_exe, [], {})] if args.parent_exe else []) + [("this, no --sort", this, [], {}), ("this, --sort gpu", this, ["--sort"], {"NABWA_SORT": "gpu"}),
                                                                                   ("this, --sort host", this, ["--sort"], {"NABWA_SORT": "host"})]
    for shape, n, paired in (("single-end", args.se, False), ("paired", args.pe, True)):
        inp = os.path.join(args.dir, "in.bam")
        t0 = time.time()
        write_input(inp, n, paired)
        print("\n== %s: %d reads, input %.1f MB BGZF (made in %.0f s)" % (shape, n, os.path.getsize(inp) / 1e6, time.time() - t0), flush=True)
        wall, digest, busy = {}, {}, {}
        for rnd in range(args.rounds):
            for name, exe, extra, env in confs[rnd % len(confs):] + confs[:rnd % len(confs)]:      # every round starts with another configuration
                outp = os.path.join(args.dir, "out_%s.bam" % re.sub(r"\W+", "_", name))
                e = dict(os.environ, NABWA_TIMING="1", **env)
                for k in ("NABWA_SORT", "NABWA_SORT_RUN_MIB"):
                    if k not in env:
                        e.pop(k, None)
                t0 = time.time()
                r = subprocess.run([exe, "-g", os.path.join(ROOT, "tests", "golden", "toy"), "-f", os.path.join(args.dir, "out.bam")] + extra + [inp], capture_output=True, text=True, env=e)
                dt = time.time() - t0
                if r.returncode != 0:
                    sys.exit("%s, round %d: exit %d\n%s" % (name, rnd, r.returncode, r.stderr[-3000:]))
                os.replace(os.path.join(args.dir, "out.bam"), outp)
                wall.setdefault(name, []).append(dt)
                m = re.search(r"sort thread ([0-9.]+) s busy \((\d+) run", r.stderr)
                if m:
                    busy.setdefault(name, []).append(float(m.group(1)))
                print("#  round %d  %-18s %.2f s wall, output %.1f MB%s" % (rnd, name, dt, os.path.getsize(outp) / 1e6, ", sort thread %s s busy, %s run(s)" % m.groups() if m else ""), flush=True)
                if rnd == 0:
                    digest[name] = records_digest(outp)
        print("%-18s %-22s %-12s %s" % ("configuration", "wall s (min med max)", "M reads/s", "sort thread busy s (min med max)"))
        for name, _, _, _ in confs:
            w = sorted(wall[name])
            print("%-18s %-22s %-12.2f %s" % (name, f3(w), n / w[len(w) // 2] / 1e6, f3(busy[name], "%.3f") if name in busy else "-"))
        if args.parent_exe:
            print("records without --sort, parent and this tree: %s" % ("the same inflated bytes" if digest["parent"] == digest["this, no --sort"] else "DIFFER"))
        print("records with --sort under NABWA_SORT=gpu and host: %s" % ("the same inflated bytes" if digest["this, --sort gpu"] == digest["this, --sort host"] else "DIFFER"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["stage", "files"])
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--parent-exe", default=None)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--se", type=int, default=8_000_000)
    ap.add_argument("--pe", type=int, default=4_000_000)
    ap.add_argument("--dir", default=os.path.join(tempfile.gettempdir(), "bam_sort_rate"))
    args = ap.parse_args()
    (stage if args.what == "stage" else files)(args)


if __name__ == "__main__":
    main()
