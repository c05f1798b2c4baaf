"""What `nabwa_bam2bam --sort --mark-duplicates` costs: the stage on its own, and file to file.

    python profiles/markdup_rate.py stage [--mib 1024] [--repeats 5]
    python profiles/markdup_rate.py files --parent-exe PATH/nabwa_bam2bam [--rounds 3] [--se 8000000] [--pe 4000000] [--dir /tmp/markdup_rate]

stage: the run of profiles/bam_sort_rate.py -- --mib MiB of finished single-end 100 bp records of 235 bytes, seed 20261020, placed uniformly
over GRCh38 -- through one nabwa_markdup handle: one warm-up round (add, resolve, clear), then --repeats rounds; per round the five
device-event times of nabwa_markdup_times and the wall times of the two calls.  Then the same records with every position folded onto
100 000 sites, so that nearly every record is a duplicate.  The marks of the last round are compared with a NumPy restatement for these
records (single reads, one CIGAR operation: the end is pos or pos + 99 by strand, the score the sum of the qualities from 15 up).

files: the 8 M single-end and 4 M paired reads of profiles/bam_sort_rate.py through three configurations -- the parent commit's
nabwa_bam2bam --sort (--parent-exe), this tree's --sort, and this tree's --sort --mark-duplicates -- in turn, --rounds rounds, each round
starting with another configuration, wall time of each command.  The records of the two --sort outputs must inflate to the same bytes, and
those of the marked output may differ from them in bit 0x400 alone.  Nothing here reads anything outside the repository."""
import argparse
import ctypes as C
import importlib
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_sort_rate as R                                                # noqa: E402

ROOT = R.ROOT
REC = R.REC


def numpy_marks(rec):
    """dup[] of the stage's records: single reads, 100M, flags 0, 4 or 16"""
    n = rec.shape[0]
    flag = rec[:, 18].astype(np.int64)
    tid = rec[:, 4:8].copy().view("<i4")[:, 0].astype(np.int64)
    pos = rec[:, 8:12].copy().view("<i4")[:, 0].astype(np.int64)
    mapped = (flag & 4) == 0
    rev = (flag & 16) != 0
    q = rec[:, 100:200]
    score = np.where(q >= 15, q, 0).sum(axis=1).astype(np.int64)
    end = (tid << 34) | (rev.astype(np.int64) << 33) | (np.where(rev, pos + 99, pos) + (1 << 30))
    idx = np.flatnonzero(mapped)
    order = idx[np.lexsort((idx, -score[idx], end[idx]))]              # by end, then falling score, then rising ordinal
    head = np.ones(order.size, bool)
    head[1:] = end[order][1:] != end[order][:-1]
    dup = np.zeros(n, np.uint8)
    dup[order[~head]] = 1
    return dup


def stage_round(nabwa, rec, repeats, what):
    n, total = rec.shape[0], rec.size
    off = np.arange(n + 1, dtype=np.int64) * REC
    L = nabwa.lib()
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    dup, stats = np.zeros(n, np.uint8), np.zeros(len(nabwa.markdup_stat_names), np.uint64)
    ev, wall_add, wall_res = [], [], []
    with nabwa.MarkDup(0) as m:
        for rep in range(1 + repeats):
            t0 = time.time()
            rc = L.nabwa_markdup_add(m._h, n, P(rec), P(off))
            t1 = time.time()
            assert rc == 0, L.nabwa_last_error()
            rc = L.nabwa_markdup_resolve(m._h, P(dup), n, P(stats))
            t2 = time.time()
            assert rc == 0, L.nabwa_last_error()
            if rep:                                   # the first round allocates and warms
                ev.append(m.times())
                wall_add.append(1e3 * (t1 - t0))
                wall_res.append(1e3 * (t2 - t1))
            m.clear()
    want = numpy_marks(rec)
    print("\n%s: %d records of %d bytes, %.1f MiB; %d tuples, %d marked" % (what, n, REC, total / 2 ** 20, int(stats[4]) + int(stats[5]), int(stats[9])))
    print("marks against the NumPy restatement: %s" % ("equal, record for record" if np.array_equal(dup, want) else "DIFFER"))
    print("%d rounds after one warm-up round, ms (min med max):" % repeats)
    for i, nm in enumerate(("add: upload", "add: signature and tuple kernels", "resolve: radix sorts", "resolve: mark kernels", "resolve: download")):
        print("  %-34s %s" % (nm, R.f3([e[i] for e in ev], "%.3f")))
    print("  %-34s %s" % ("wall, nabwa_markdup_add", R.f3(wall_add, "%.1f")))
    print("  %-34s %s" % ("wall, nabwa_markdup_resolve", R.f3(wall_res, "%.1f")))
    k = sorted(e[1] for e in ev)[len(ev) // 2]
    s = sorted(e[2] + e[3] for e in ev)[len(ev) // 2]
    print("  signature kernels: %.1f MiB read in %.3f ms (median) = %.2f TB/s = %.0f %% of the HBM peak of MI355X_MICROARCH.md (8.0 TB/s, spec)" % (total / 2 ** 20, k, total / (k * 1e-3) / 1e12, 100 * total / (k * 1e-3) / R.HBM_PEAK))
    print("  resolve on the device: %.3f ms (median) = %.1f M tuples/s" % (s, (int(stats[4]) + int(stats[5])) / s / 1e3))


def stage(args):
    sys.path.insert(0, ROOT)
    nabwa = importlib.import_module("network-aware-bwa_amd")
    n = (args.mib << 20) // REC
    rec = R.finished_records(n, 20261020)
    stage_round(nabwa, rec, args.repeats, "positions over GRCh38")
    pos = rec[:, 8:12].copy().view("<i4")[:, 0]
    mapped = pos >= 0
    pos[mapped] %= 100000
    rec[:, 8:12] = pos.astype("<i4").view(np.uint8).reshape(n, 4)
    stage_round(nabwa, rec, args.repeats, "positions folded onto 100 000 sites per contig")


def only_0x400_differs(sorted_path, marked_path):
    """-> (whether the inflated files, headers aside, differ in nothing but bits of value 0x04, the number of bytes that carry one)"""
    import gzip
    a, b = gzip.decompress(open(sorted_path, "rb").read()), gzip.decompress(open(marked_path, "rb").read())
    a, b = np.frombuffer(a, np.uint8)[R.header_bytes(a):], np.frombuffer(b, np.uint8)[R.header_bytes(b):]
    if a.size != b.size:
        return False, 0
    x = a ^ b
    nz = np.flatnonzero(x)
    return bool((x[nz] == 4).all()), int(nz.size)


def files(args):
    os.makedirs(args.dir, exist_ok=True)
    this = os.path.join(ROOT, "network-aware-bwa_amd", "nabwa_bam2bam")
    confs = [("parent, --sort", args.parent_exe, ["--sort"]), ("this, --sort", this, ["--sort"]), ("this, --sort --mark-duplicates", this, ["--sort", "--mark-duplicates"])]
    for shape, n, paired in (("single-end", args.se, False), ("paired", args.pe, True)):
        inp = os.path.join(args.dir, "in.bam")
        t0 = time.time()
        R.write_input(inp, n, paired)
        print("\n== %s: %d reads, input %.1f MB BGZF (made in %.0f s)" % (shape, n, os.path.getsize(inp) / 1e6, time.time() - t0), flush=True)
        wall, busy, digest, last = {}, {}, {}, {}
        for rnd in range(args.rounds):
            for name, exe, extra in confs[rnd % len(confs):] + confs[:rnd % len(confs)]:      # every round starts with another configuration
                outp = os.path.join(args.dir, "out_%s.bam" % re.sub(r"\W+", "_", name))
                e = dict(os.environ, NABWA_TIMING="1")
                for k in ("NABWA_SORT", "NABWA_SORT_RUN_MIB", "NABWA_MARKDUP_ENDS", "NABWA_MARKDUP_QUAL"):
                    e.pop(k, None)
                t0 = time.time()
                r = subprocess.run([exe, "-g", os.path.join(ROOT, "tests", "golden", "toy"), "-f", os.path.join(args.dir, "out.bam")] + extra + [inp], capture_output=True, text=True, env=e)
                dt = time.time() - t0
                if r.returncode != 0:
                    sys.exit("%s, round %d: exit %d\n%s" % (name, rnd, r.returncode, r.stderr[-3000:]))
                os.replace(os.path.join(args.dir, "out.bam"), outp)
                wall.setdefault(name, []).append(dt)
                m = re.search(r"duplicates thread ([0-9.]+) s busy", r.stderr)
                s = re.search(r"sort thread ([0-9.]+) s busy", r.stderr)
                busy.setdefault(name, []).append((float(s.group(1)) if s else 0.0, float(m.group(1)) if m else 0.0))
                last[name] = r.stderr.rstrip("\n").split("\n")[-1]
                print("#  round %d  %-32s %.2f s wall, sort thread %s s busy%s" % (rnd, name, dt, s.group(1) if s else "-", ", duplicates thread %s s busy" % m.group(1) if m else ""), flush=True)
                if rnd == 0 and "mark" not in name:
                    digest[name] = R.records_digest(outp)
        print("%-32s %-22s %-12s %-34s %s" % ("configuration", "wall s (min med max)", "M reads/s", "sort thread busy s (min med max)", "duplicates thread busy s (min med max)"))
        for name, _, _ in confs:
            w = sorted(wall[name])
            print("%-32s %-22s %-12.2f %-34s %s" % (name, R.f3(w), n / w[len(w) // 2] / 1e6, R.f3([b[0] for b in busy[name]], "%.3f"), R.f3([b[1] for b in busy[name]], "%.3f") if "mark" in name else "-"))
        print("records of the two --sort outputs: %s" % ("the same inflated bytes" if digest["parent, --sort"] == digest["this, --sort"] else "DIFFER"))
        same, n_marked = only_0x400_differs(os.path.join(args.dir, "out_this_sort.bam"), os.path.join(args.dir, "out_this_sort_mark_duplicates.bam"))
        print("records of the marked output against those of --sort: %s" % ("the same bytes but for bit 0x400, which %d records carry" % n_marked if same else "DIFFER"))
        print(last["this, --sort --mark-duplicates"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["stage", "files"])
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-exe", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--se", type=int, default=8_000_000)
    ap.add_argument("--pe", type=int, default=4_000_000)
    ap.add_argument("--dir", default=os.path.join(tempfile.gettempdir(), "markdup_rate"))
    args = ap.parse_args()
    if args.what == "files" and not args.parent_exe:
        ap.error("files needs --parent-exe: the comparison is with the parent commit's --sort")
    (stage if args.what == "stage" else files)(args)


if __name__ == "__main__":
    main()
