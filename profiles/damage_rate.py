"""What the damage profile costs: nabwa_damage_add on its own, and `nabwa_bam2bam --damage` file to file.

    python profiles/damage_rate.py stage [--mib 1024] [--repeats 5] [--threads 16] [--mbases 1024]
    python profiles/damage_rate.py files [--parent-exe PATH/nabwa_bam2bam] [--rounds 3] [--se 8000000] [--pe 4000000] [--dir /tmp/damage_rate]

stage: one call of --mib MiB of finished single-end 100 bp records of 235 bytes, the layout of profiles/bam_sort_rate.py's stage run (seed
20261020), against a reference of --mbases x 2^20 random bases in 16 contigs set on the toy index with nabwa_index_set_reference: 99 % of the
records placed uniformly, half of them on the reverse strand, 1 % unmapped; a read carries its reference window with 1 % substitutions and, on
its own strand, C>T at the 5' end and G>A at the 3' end with probability 0.3 x 0.7^distance.  One handle: one warm-up call, then --repeats
calls; per call the three device-event times of nabwa_damage_times and the wall time.  The kernel's bytes are the records once plus 25 bytes of
reference window per counted record.  The tables of the full call are held against what must be true of them (every record seen, 100 columns per
counted record, both tables sum to the columns) and, for the first 5000 records through a second handle, against the Python oracle of
tests/damage_cases.py.  Then the host comparison: csrc/damage_body.hpp as tests/emu/damage_emu.cpp builds it for the CPU (-O2), the same records
split evenly over --threads threads, their tables added.

files: the 8 M single-end and 4 M paired inputs of profiles/bam_sort_rate.py through the parent commit's nabwa_bam2bam (--parent-exe), this
tree's without --damage and with it, in turn, --rounds rounds, each round starting with another configuration; wall time of each command.  The
records of all three must inflate to the same bytes.  Nothing here reads anything outside the repository."""
import argparse
import ctypes as C
import importlib
import os
import re
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles"))
import bam_sort_rate as S          # noqa: E402  (the records' layout, the file-to-file inputs, the digest of a file's records)

REC, L = S.REC, 100
SORT_GATHER = 3.16e12              # profiles/bam_sort_rate.txt: the sort's gather kernel on a run of the same bytes


def damaged_records(n, seed, pac, l_pac, contig_off, contig_len):
    """n finished records of REC bytes on the reference -> (n, REC) uint8"""
    rng = np.random.default_rng(seed)
    rec = S.finished_records(n, seed)                                   # names, qualities, tags, the CIGAR 100M; places and bases are replaced
    tid = rng.integers(0, len(contig_off), n)
    pos = (rng.random(n) * (np.asarray(contig_len)[tid] - L)).astype(np.int64)
    unmapped = rng.random(n) < 0.01
    rev = rng.random(n) < 0.5
    g = np.asarray(contig_off)[tid] + pos
    step = 1 << 18
    nib = np.array([1, 2, 4, 8], np.uint8)
    decay = 0.3 * 0.7 ** np.arange(L)
    for a in range(0, n, step):
        b = min(a + step, n)
        k = g[a:b, None] + np.arange(L)[None, :]
        code = (pac[k >> 2] >> ((~k & 3) << 1).astype(np.uint8)) & 3     # the window, reference orientation (the stored orientation)
        sub = rng.random(code.shape) < 0.01
        code[sub] = (code[sub] + rng.integers(1, 4, int(sub.sum()))) & 3
        u = rng.random(code.shape)
        fw, rv = ~rev[a:b, None], rev[a:b, None]
        # forward reads: C>T near the first stored base, G>A near the last.  A reverse-strand read is stored as its reverse complement: its own
        # C>T at its 5' end shows as G>A near the last stored base, its own G>A at its 3' end as C>T near the first -- the same two lines
        ct5, ga3 = u < decay[None, :], u < decay[None, ::-1]
        code[fw & ct5 & (code == 1)] = 3
        code[fw & ga3 & (code == 2)] = 0
        code[rv & ga3 & (code == 2)] = 0
        code[rv & ct5 & (code == 1)] = 3
        rec[a:b, 50:100] = (nib[code[:, 0::2]] << 4) | nib[code[:, 1::2]]
    tid = np.where(unmapped, -1, tid)
    pos = np.where(unmapped, -1, pos)
    rec[:, 4:8] = tid.astype("<i4").view(np.uint8).reshape(n, 4)
    rec[:, 8:12] = pos.astype("<i4").view(np.uint8).reshape(n, 4)
    rec[:, 18] = np.where(unmapped, 4, rev * 16).astype(np.uint8)
    return rec


def stage(args):
    import damage_cases as D
    import nabwa_testlib as T
    nabwa = importlib.import_module("network-aware-bwa_amd")
    n = (args.mib << 20) // REC
    l_pac = args.mbases << 20
    rng = np.random.default_rng(20261020)
    pac = rng.integers(0, 256, l_pac // 4, dtype=np.uint8)
    ix = nabwa.Index.load(T.TOY, 0, True, with_ref=True)
    names, offs, lens = ix.set_reference(l_pac, 11, pac, n_contigs=16)
    t0 = time.time()
    rec = damaged_records(n, 20261020, pac, l_pac, offs, lens)
    total = rec.size
    off = np.arange(n + 1, dtype=np.int64) * REC
    print("one call: %d records of %d bytes, %.1f MiB, seed 20261020; reference of %d x 2^20 bases in 16 contigs (made in %.0f s)" % (n, REC, total / 2 ** 20, args.mbases, time.time() - t0), flush=True)
    Lb = nabwa.lib()
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    ev, wall = [], []
    with nabwa.Damage(ix) as d:
        for rep in range(1 + args.repeats):
            d.clear()
            t0 = time.time()
            rc = Lb.nabwa_damage_add(d._h, n, P(rec), P(off))
            dt = time.time() - t0
            assert rc == 0, Lb.nabwa_last_error()
            if rep:                                   # the first call allocates and warms
                ev.append(d.times())
                wall.append(1e3 * dt)
        sub5, sub3, len_hist, stats = d.fetch()
    counted = int(stats[D.COUNTED])
    ok = int(stats[D.SEEN]) == n and int(stats[D.SK_FLAGS]) == n - counted and int(stats[D.COLS]) == L * counted == int(sub5.sum()) == int(sub3.sum()) and int(len_hist[L]) == counted
    print("tables of the call: %s (%d of %d records counted, %d columns)" % ("consistent" if ok else "INCONSISTENT", counted, n, int(stats[D.COLS])))
    ref = D.Ref(pac.tobytes(), l_pac, list(zip(names, [int(o) for o in offs], [int(x) for x in lens])), [])
    few = [rec[i].tobytes() for i in range(5000)]
    with nabwa.Damage(ix) as d:
        d.add(b"".join(few))
        got = D.Tables(25)
        for a, b in zip(got.parts(), d.fetch()):
            a[:] = b
    want = D.oracle(ref, D.opt_of(), few)
    same = all(np.array_equal(a, b) for a, b in zip(got.parts(), want.parts()))
    print("first 5000 records against the Python oracle: %s" % ("equal" if same else "DIFFER"))
    ct = sub5[:, 1, 3] / np.maximum(sub5[:, 1, :].sum(axis=1), 1)
    ga = sub3[:, 2, 0] / np.maximum(sub3[:, 2, :].sum(axis=1), 1)
    print("5' C>T at positions 1, 2, 3, 10, >25: %s;  3' G>A: %s" % (" ".join("%.4f" % ct[p] for p in (0, 1, 2, 9, 25)), " ".join("%.4f" % ga[p] for p in (0, 1, 2, 9, 25))))
    print("\nGPU path, %d calls after one warm-up call, ms (min med max):" % args.repeats)
    for i, nm in enumerate(["upload", "kernel", "table add"]):
        print("  %-14s %s" % (nm, S.f3([e[i] for e in ev], "%.3f")))
    print("  %-14s %s" % ("all three", S.f3([sum(e) for e in ev], "%.3f")))
    print("  %-14s %s" % ("wall, the call", S.f3(wall, "%.1f")))
    k = sorted(e[1] for e in ev)[len(ev) // 2]
    moved = total + (L // 4) * counted
    rate = moved / (k * 1e-3)
    print("  kernel: %.1f MiB of records + %.1f MiB of reference windows in %.3f ms (median) = %.3f TB/s = %.1f %% of the HBM peak of MI355X_MICROARCH.md (8.0 TB/s, spec); "
          "the sort's gather kernel moves a run of these bytes at %.2f TB/s (profiles/bam_sort_rate.txt): this kernel runs at %.1f %% of that; %.1f G columns/s"
          % (total / 2 ** 20, (L // 4) * counted / 2 ** 20, k, rate / 1e12, 100 * rate / S.HBM_PEAK, SORT_GATHER / 1e12, 100 * rate / SORT_GATHER, L * counted / (k * 1e-3) / 1e9))
    up = sorted(e[0] for e in ev)[len(ev) // 2]
    print("  upload %.1f GB/s (pageable host memory)" % (total / up / 1e6))
    # the host comparison: the same body, compiled for the CPU, on --threads threads
    emu = D.load_emu()
    T_ = args.threads
    cut = [n * t // T_ for t in range(T_ + 1)]
    words = D.Tables(25).words().size
    co, ho, hl = np.ascontiguousarray(offs, np.int64), np.zeros(1, np.int64), np.zeros(1, np.int32)
    pac1 = np.concatenate([pac, np.zeros(1, np.uint8)])                 # l_pac / 4 + 1 bytes

    def part(t):
        w = np.zeros(words, np.uint64)
        o = np.ascontiguousarray(off[cut[t]:cut[t + 1] + 1])
        bad = emu.emu_damage_run(cut[t + 1] - cut[t], P(rec), P(o), P(pac1), l_pac, 0, P(ho), P(hl), 16, P(co), 25, 0, 0xF04, 0, 1, P(w))
        assert bad == -1
        return w
    ms = []
    for rep in range(1 + args.repeats):
        t0 = time.time()
        with ThreadPoolExecutor(T_) as ex:
            w = sum(ex.map(part, range(T_)))
        if rep:
            ms.append(1e3 * (time.time() - t0))
    host = D.Tables.from_words(25, w)
    print("\nhost comparison (damage_body.hpp compiled for the CPU, -O2, %d threads), %d passes after one warm-up, ms (min med max): %s; tables %s"
          % (T_, len(ms), S.f3(ms, "%.1f"), "equal to the device's" if all(np.array_equal(a, b) for a, b in zip(host.parts(), (sub5, sub3, len_hist, stats))) else "DIFFER"))
    ix.close()


def files(args):
    os.makedirs(args.dir, exist_ok=True)
    this = os.path.join(ROOT, "network-aware-bwa_amd", "nabwa_bam2bam")
    prof = os.path.join(args.dir, "damage.tsv")
    confs = ([("parent", args.parent_exe, [])] if args.parent_exe else []) + [("this, no --damage", this, []), ("this, --damage", this, ["--damage", prof])]
    for shape, n, paired in (("single-end", args.se, False), ("paired", args.pe, True)):
        inp = os.path.join(args.dir, "in.bam")
        t0 = time.time()
        S.write_input(inp, n, paired)
        print("\n== %s: %d reads, input %.1f MB BGZF (made in %.0f s)" % (shape, n, os.path.getsize(inp) / 1e6, time.time() - t0), flush=True)
        wall, digest, busy, line = {}, {}, {}, ""
        for rnd in range(args.rounds):
            for name, exe, extra in confs[rnd % len(confs):] + confs[:rnd % len(confs)]:      # every round starts with another configuration
                e = dict(os.environ, NABWA_TIMING="1")
                t0 = time.time()
                r = subprocess.run([exe, "-g", os.path.join(ROOT, "tests", "golden", "toy"), "-f", os.path.join(args.dir, "out.bam")] + extra + [inp], capture_output=True, text=True, env=e)
                dt = time.time() - t0
                if r.returncode != 0:
                    sys.exit("%s, round %d: exit %d\n%s" % (name, rnd, r.returncode, r.stderr[-3000:]))
                wall.setdefault(name, []).append(dt)
                m = re.search(r"damage thread ([0-9.]+) s busy", r.stderr)
                if m:
                    busy.setdefault(name, []).append(float(m.group(1)))
                    line = [x for x in r.stderr.split("\n") if "damage profile of" in x][0]
                print("#  round %d  %-18s %.2f s wall%s" % (rnd, name, dt, ", damage thread %s s busy" % m.group(1) if m else ""), flush=True)
                if rnd == 0:
                    digest[name] = S.records_digest(os.path.join(args.dir, "out.bam"))
        print("%-18s %-22s %-12s %s" % ("configuration", "wall s (min med max)", "M reads/s", "damage thread busy s (min med max)"))
        for name, _, _ in confs:
            w = sorted(wall[name])
            print("%-18s %-22s %-12.2f %s" % (name, S.f3(w), n / w[len(w) // 2] / 1e6, S.f3(busy[name], "%.3f") if name in busy else "-"))
        print("records of %s: %s" % (", ".join(digest), "the same inflated bytes" if len(set(digest.values())) == 1 else "DIFFER"))
        print(line)
        print("".join(open(prof).readlines()[:10]), end="")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["stage", "files"])
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--mbases", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--parent-exe", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--se", type=int, default=8_000_000)
    ap.add_argument("--pe", type=int, default=4_000_000)
    ap.add_argument("--dir", default=os.path.join(tempfile.gettempdir(), "damage_rate"))
    args = ap.parse_args()
    (stage if args.what == "stage" else files)(args)


if __name__ == "__main__":
    main()
