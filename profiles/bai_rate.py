"""What `nabwa_bam2bam --sort --index` costs: the stage on its own, and file to file.

    python profiles/bai_rate.py stage [--mib 1024] [--repeats 5] [--threads 16]
    python profiles/bai_rate.py files --parent-exe PATH/nabwa_bam2bam [--rounds 3] [--se 8000000] [--pe 4000000] [--dir /tmp/bai_rate]

stage: the run of profiles/bam_sort_rate.py -- --mib MiB of finished single-end 100 bp records of 235 bytes, seed 20261020, placed uniformly
over GRCh38 -- put into coordinate order and handed to one nabwa_bai handle as one call, with a block table of blocks of 0xff00 bytes: one
warm-up round (add, finish, clear), then --repeats rounds; per round the seven device-event times of nabwa_bai_times and the wall times of
the two calls.  The file of the last round is compared with the one the CPU emulation of the bodies (tests/emu/bai_emu.cpp) writes.  Beside
it, in the same process on the same bytes: nabwa_markdup_add (its signature and tuple kernels), the gather kernel of nabwa_bam_sort_run,
and the emulation's add on --threads host threads (a slice and a handle each).

files: the 8 M single-end and 4 M paired reads of profiles/bam_sort_rate.py through three configurations -- the parent commit's
nabwa_bam2bam --sort (--parent-exe), this tree's --sort, and this tree's --sort --index -- in turn, --rounds rounds, each round starting
with another configuration, wall time of each command.  The records of the three outputs must inflate to the same bytes.  Nothing here
reads anything outside the repository."""
import argparse
import ctypes as C
import importlib
import os
import re
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_sort_rate as R                                                # noqa: E402

ROOT = R.ROOT
REC = R.REC
HEADER = 4096                 # the bytes taken to lie in front of the first record


def stage(args):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    nabwa = importlib.import_module("network-aware-bwa_amd")
    import bai_cases as M
    n = (args.mib << 20) // REC
    rec = R.finished_records(n, 20261020)
    k = (rec[:, 4:8].copy().view("<u4")[:, 0].astype(np.uint64) << np.uint64(32)) | ((rec[:, 8:12].copy().view("<i4")[:, 0].astype(np.int64) + 1).astype(np.uint64) & np.uint64(0xffffffff))
    unsorted = rec
    rec = np.ascontiguousarray(rec[np.argsort(k, kind="stable")])
    total, n_ref = rec.size, len(R.GRCH38)
    off = np.arange(n + 1, dtype=np.int64) * REC
    u = np.append(np.arange(0, HEADER + total, 0xff00, dtype=np.int64), HEADER + total)
    c = (u // 4) + 28 * np.arange(u.size, dtype=np.int64)
    L = nabwa.lib()
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    ev, wall_add, wall_fin = [], [], []
    n_out, stats = C.c_int64(), np.zeros(len(nabwa.bai_stat_names), np.uint64)
    with nabwa.Bai(n_ref) as b:
        out = None
        for rep in range(1 + args.repeats):
            t0 = time.time()
            rc = L.nabwa_bai_add(b._h, n, P(rec), P(off), HEADER)
            t1 = time.time()
            assert rc == 0, L.nabwa_last_error()
            if out is None:
                assert L.nabwa_bai_finish(b._h, u.size - 1, P(u), P(c), None, 0, C.byref(n_out), None) == 0, L.nabwa_last_error()
                out = np.zeros(n_out.value, np.uint8)
                t1 = time.time()
            t2 = time.time()
            rc = L.nabwa_bai_finish(b._h, u.size - 1, P(u), P(c), P(out), out.size, C.byref(n_out), P(stats))
            t3 = time.time()
            assert rc == 0, L.nabwa_last_error()
            if rep:                                   # the first round allocates and warms
                ev.append(b.times())
                wall_add.append(1e3 * (t1 - t0))
                wall_fin.append(1e3 * (t3 - t2))
            b.clear()
    print("one call: %d records of %d bytes in coordinate order, %.1f MiB, seed 20261020; %d references, %d blocks" % (n, REC, total / 2 ** 20, n_ref, u.size - 1))
    print("the index: %d bytes, %d bins, %d chunks, %d windows, %d records without a reference" % (int(stats[6]), int(stats[3]), int(stats[4]), int(stats[5]), int(stats[2])))
    emu = M.load_emu()
    h = emu.emu_bai_create(n_ref)
    t0 = time.time()
    assert emu.emu_bai_add(h, n, P(rec), P(off), HEADER, 64) == -1
    t_emu_one = time.time() - t0
    want, wstats = np.zeros(out.size, np.uint8), np.zeros(M.N_STATS, np.uint64)
    t0 = time.time()
    size = emu.emu_bai_finish(h, u.size - 1, P(u), P(c), P(want), want.size, P(wstats))
    t_emu_fin = time.time() - t0
    emu.emu_bai_destroy(h)
    print("file against the CPU emulation of the bodies: %s" % ("equal, byte for byte" if size == out.size and np.array_equal(out, want) and np.array_equal(stats, wstats) else "DIFFERS"))
    print("%d rounds after one warm-up round, ms (min med max):" % args.repeats)
    for i, nm in enumerate(("add: upload", "add: signature kernel", "finish: radix sort", "finish: offsets, chunks, layout", "finish: linear index", "finish: writer kernels", "finish: download")):
        print("  %-34s %s" % (nm, R.f3([e[i] for e in ev], "%.3f")))
    print("  %-34s %s" % ("wall, nabwa_bai_add", R.f3(wall_add, "%.1f")))
    print("  %-34s %s" % ("wall, nabwa_bai_finish", R.f3(wall_fin, "%.1f")))
    kk = sorted(e[1] for e in ev)[len(ev) // 2]
    print("  signature kernel: %.1f MiB read in %.3f ms (median) = %.2f TB/s = %.0f %% of the HBM peak of MI355X_MICROARCH.md (8.0 TB/s, spec)" % (total / 2 ** 20, kk, total / (kk * 1e-3) / 1e12, 100 * total / (kk * 1e-3) / R.HBM_PEAK))
    fin = sorted(sum(e[2:6]) for e in ev)[len(ev) // 2]
    print("  finish on the device without the download: %.3f ms (median) = %.1f M records/s" % (fin, n / fin / 1e3))
    # beside it, on the same bytes in the same process
    md = []
    with nabwa.MarkDup(0) as m:
        for rep in range(1 + args.repeats):
            assert L.nabwa_markdup_add(m._h, n, P(rec), P(off)) == 0, L.nabwa_last_error()
            if rep:
                md.append(m.times())
            m.clear()
    print("\nnabwa_markdup_add on the same bytes, ms (min med max): upload %s, signature and tuple kernels %s" % (R.f3([e[0] for e in md], "%.3f"), R.f3([e[1] for e in md], "%.3f")))
    so = []
    sorted_out, out_off, keys = np.empty(total, np.uint8), np.zeros(n + 1, np.int64), np.zeros(n, np.uint64)
    with nabwa.BamSort(0) as s:
        for rep in range(1 + args.repeats):
            assert L.nabwa_bam_sort_run(s._h, n, P(unsorted), P(off), P(sorted_out), total, P(out_off), P(keys)) == 0, L.nabwa_last_error()
            if rep:
                so.append(s.times())
    print("nabwa_bam_sort_run on the same records before they were sorted, ms (min med max): gather kernel %s (it moves the bytes twice)" % R.f3([e[4] for e in so], "%.3f"))
    # the body on host threads: a slice and a handle per thread
    nt = args.threads
    cuts = [n * t // nt for t in range(nt + 1)]
    hs = [emu.emu_bai_create(n_ref) for _ in range(nt)]
    bad = [0] * nt

    def work(t):
        a, z = cuts[t], cuts[t + 1]
        o = np.ascontiguousarray(off[a:z + 1])
        bad[t] = emu.emu_bai_add(hs[t], z - a, P(rec), P(o), HEADER + int(o[0]), 64)
    ths = [threading.Thread(target=work, args=(t,)) for t in range(nt)]
    t0 = time.time()
    for x in ths:
        x.start()
    for x in ths:
        x.join()
    t_emu = time.time() - t0
    for x in hs:
        emu.emu_bai_destroy(x)
    assert all(x == -1 for x in bad)
    print("the emulation body (g++ -O2): add of the same records %.1f ms on one thread, %.1f ms on %d threads; its finish %.1f ms on one thread" % (1e3 * t_emu_one, 1e3 * t_emu, nt, 1e3 * t_emu_fin))


def files(args):
    os.makedirs(args.dir, exist_ok=True)
    this = os.path.join(ROOT, "network-aware-bwa_amd", "nabwa_bam2bam")
    confs = [("parent, --sort", args.parent_exe, ["--sort"]), ("this, --sort", this, ["--sort"]), ("this, --sort --index", this, ["--sort", "--index"])]
    for shape, n, paired in (("single-end", args.se, False), ("paired", args.pe, True)):
        inp = os.path.join(args.dir, "in.bam")
        t0 = time.time()
        R.write_input(inp, n, paired)
        print("\n== %s: %d reads, input %.1f MB BGZF (made in %.0f s)" % (shape, n, os.path.getsize(inp) / 1e6, time.time() - t0), flush=True)
        wall, busy, digest, last, size = {}, {}, {}, {}, 0
        for rnd in range(args.rounds):
            for name, exe, extra in confs[rnd % len(confs):] + confs[:rnd % len(confs)]:      # every round starts with another configuration
                outp = os.path.join(args.dir, "out_%s.bam" % re.sub(r"\W+", "_", name))
                e = dict(os.environ, NABWA_TIMING="1")
                for k in ("NABWA_SORT", "NABWA_SORT_RUN_MIB", "NABWA_BGZF"):
                    e.pop(k, None)
                t0 = time.time()
                r = subprocess.run([exe, "-g", os.path.join(ROOT, "tests", "golden", "toy"), "-f", os.path.join(args.dir, "out.bam")] + extra + [inp], capture_output=True, text=True, env=e)
                dt = time.time() - t0
                if r.returncode != 0:
                    sys.exit("%s, round %d: exit %d\n%s" % (name, rnd, r.returncode, r.stderr[-3000:]))
                os.replace(os.path.join(args.dir, "out.bam"), outp)
                if "index" in name:
                    size = os.path.getsize(os.path.join(args.dir, "out.bam.bai"))
                    os.remove(os.path.join(args.dir, "out.bam.bai"))
                wall.setdefault(name, []).append(dt)
                m = re.search(r"index thread ([0-9.]+) s busy", r.stderr)
                f = re.search(r"index finished and written in ([0-9.]+) s", r.stderr)
                busy.setdefault(name, []).append((float(m.group(1)) if m else 0.0, float(f.group(1)) if f else 0.0))
                last[name] = r.stderr.rstrip("\n").split("\n")[-1]
                print("#  round %d  %-24s %.2f s wall%s" % (rnd, name, dt, ", index thread %s s busy, finish and write %s s" % (m.group(1), f.group(1)) if m and f else ""), flush=True)
                if rnd == 0:
                    digest[name] = R.records_digest(outp)
        print("%-24s %-22s %-12s %-36s %s" % ("configuration", "wall s (min med max)", "M reads/s", "index thread busy s (min med max)", "finish and write s (min med max)"))
        for name, _, _ in confs:
            w = sorted(wall[name])
            ix = "index" in name
            print("%-24s %-22s %-12.2f %-36s %s" % (name, R.f3(w), n / w[len(w) // 2] / 1e6, R.f3([b[0] for b in busy[name]], "%.3f") if ix else "-", R.f3([b[1] for b in busy[name]], "%.3f") if ix else "-"))
        print("records of the three outputs: %s" % ("the same inflated bytes" if digest["parent, --sort"] == digest["this, --sort"] == digest["this, --sort --index"] else "DIFFER"))
        print("%s; out.bam.bai has %d bytes" % (last["this, --sort --index"], size))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["stage", "files"])
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--parent-exe", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--se", type=int, default=8_000_000)
    ap.add_argument("--pe", type=int, default=4_000_000)
    ap.add_argument("--dir", default=os.path.join(tempfile.gettempdir(), "bai_rate"))
    args = ap.parse_args()
    if args.what == "files" and not args.parent_exe:
        ap.error("files needs --parent-exe: the comparison is with the parent commit's --sort")
    (stage if args.what == "stage" else files)(args)


if __name__ == "__main__":
    main()
