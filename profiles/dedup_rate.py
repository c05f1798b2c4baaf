"""What NABWA_DEDUP=1 costs where a batch has nothing to merge, and what it gains where it has: bench.py's two
single-end shapes -- 10 M x 100 bp under the default options, 6.25 M reads of 50-76 bp under the ancient-DNA options -- on the
GRCh38-sized synthetic index, as they are (k = 1) and with the first n / k distinct reads each present k = 2 and 5 times, shuffled.

    python profiles/dedup_rate.py [--parent-lib PATH/libnabwa.so] [--rounds 3] [--reads N] [--adna-reads N] [--genome-len N]

One child process per library and round, the libraries in turn within the one command; a child builds the index, then runs every set-up
of its library: for this tree each batch with the variable unset and with 1, for the parent commit's library (--parent-lib) the k = 1
batches.  Per set-up: wall time of nabwa_batch_create, wall time of each of three run + sync steps after one warm-up step, the row
checksum, and with 1 the stage's own HIP-event time from its NABWA_TIMING line.  The summary goes to stdout."""
import argparse
import importlib
import importlib.util
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"\[nabwa\] dedup: (\d+) reads given, (\d+) searched, (\d+) hash collisions, stage ([0-9.]+) ms")


def duplicated(seq, rseq, off, k, seed):
    """the first n / k reads, each k times, shuffled -> (seq, rseq, off) of n / k * k reads"""
    n = (len(off) - 1) // k
    ids = np.random.default_rng(seed).permutation(np.repeat(np.arange(n), k))
    lens = np.diff(off)[ids]
    new_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    out_s, out_r = np.empty(new_off[-1], np.uint8), np.empty(new_off[-1], np.uint8)
    for lo in range(0, len(ids), 1 << 20):
        hi = min(len(ids), lo + (1 << 20))
        src = np.repeat(off[ids[lo:hi]] - new_off[lo:hi], lens[lo:hi]) + np.arange(new_off[lo], new_off[hi])
        out_s[new_off[lo]:new_off[hi]] = seq[src]
        out_r[new_off[lo]:new_off[hi]] = rseq[src]
    return out_s, out_r, new_off


def child(args):
    sys.path.insert(0, ROOT)
    nabwa = importlib.import_module("network-aware-bwa_amd")
    synth = importlib.import_module("network-aware-bwa_amd.synth")
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    n = args.genome_len
    d_text = synth.synth_text(n, 20261004, n_dup=2000, dup_len=5000)
    parts = [synth.build_index(d_text, n, rev, 32, True) for rev in (0, 1)]
    ix = nabwa.Index.from_arrays((parts[0][0].ptr, parts[0][1]), (parts[1][0].ptr, parts[1][1]),
                                 (parts[0][2].ptr, parts[0][3]), (parts[1][2].ptr, parts[1][3]), device_ptrs=True)
    for p in parts:
        p[0].free()
        p[2].free()
    shapes = []
    opt = nabwa.gap_init_opt()
    shapes.append(("default 100 bp", opt, synth.synth_reads(d_text, n, args.reads, 100, 2000, 0, 2)))
    seq, rseq, off = synth.synth_reads(d_text, n, args.adna_reads, 76, 10000, 0, 2)
    opt = nabwa.gap_init_opt()
    opt.fnr, opt.max_diff, opt.max_gapo, opt.seed_len = 0.01, -1, 2, 16500
    shapes.append(("ancient-DNA 50-76 bp", opt, bench.adna_profile(seq, args.adna_reads, 76, 5)))
    d_text.free()
    ix.cal_sa_reg_gap_flat(shapes[0][1], shapes[0][2][0][:100000], shapes[0][2][1][:100000], shapes[0][2][2][:1001], per_read=True)      # code objects, pool
    for shape, opt, reads in shapes:
        for k in ((1,) if args.child == "parent" else (1, 2, 5)):
            seq, rseq, off = reads if k == 1 else duplicated(*reads, k, 7 + k)
            for sw in ((None,) if args.child == "parent" else (None, "1")):
                os.environ.pop("NABWA_DEDUP", None)
                if sw:
                    os.environ["NABWA_DEDUP"] = sw
                t0 = time.time()
                b = nabwa.Batch(ix, opt, seq, rseq, off, per_read=True)
                create_s = time.time() - t0
                b.run()
                b.sync()
                steps = []
                for _ in range(args.steps):
                    t0 = time.time()
                    b.run()
                    b.sync()
                    steps.append(1e3 * (time.time() - t0))
                cks, rows = b.checksum()
                st = b.dedup_stats() if hasattr(nabwa.lib(), "nabwa_batch_dedup_stats") else [len(off) - 1, len(off) - 1, 0, 0]
                b.close()
                print(json.dumps(dict(lib=args.child, shape=shape, k=k, dedup=sw or "unset", n=st[0], n_u=st[1], coll=st[2], create_s=create_s,
                                      step_ms=steps, checksum="%016x" % cks, rows=rows)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--adna-reads", type=int, default=6_250_000)
    ap.add_argument("--genome-len", type=int, default=3099734149)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    res = []
    for rnd in range(args.rounds):
        for which in (["parent"] if args.parent_lib else []) + ["this"]:
            env = dict(os.environ, NABWA_TIMING="1")
            env.pop("NABWA_DEDUP", None)
            if which == "parent":
                env["NABWA_LIB"] = args.parent_lib
            cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--steps", str(args.steps), "--reads", str(args.reads),
                   "--adna-reads", str(args.adna_reads), "--genome-len", str(args.genome_len)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True)
            if r.returncode != 0:
                sys.exit("round %d, %s: exit %d\n%s" % (rnd, which, r.returncode, r.stderr[-3000:]))
            got = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
            stage = [float(m[3]) for m in LINE.findall(r.stderr)]
            on = [g for g in got if g["dedup"] == "1"]
            assert len(stage) == len(on), (len(stage), len(on))
            for g, ms in zip(on, stage):
                g["stage_ms"] = ms
            for g in got:
                g["round"] = rnd
                print("# " + json.dumps(g), flush=True)
            res += got
    keys = []
    for g in res:
        key = (g["shape"], g["k"], g["lib"], g["dedup"])
        if key not in keys:
            keys.append(key)
    print("\n%-22s %2s %-7s %-6s %9s %9s  %-26s %-30s %-22s %s" % ("shape", "k", "library", "DEDUP", "reads", "searched", "create s (min med max)",
                                                                "step ms (min med max)", "stage ms (min med max)", "M reads/s  checksum"))
    for key in keys:
        gs = [g for g in res if (g["shape"], g["k"], g["lib"], g["dedup"]) == key]
        cr = sorted(g["create_s"] for g in gs)
        st = sorted(x for g in gs for x in g["step_ms"])
        sg = sorted(g["stage_ms"] for g in gs if "stage_ms" in g)
        cks = sorted(set(g["checksum"] for g in gs))
        f3 = lambda v, fmt: " ".join(fmt % x for x in (v[0], v[len(v) // 2], v[-1])) if v else "-"
        print("%-22s %2d %-7s %-6s %9d %9d  %-26s %-30s %-22s %8.2f  %s" % (key[0], key[1], key[2], key[3], gs[0]["n"], gs[0]["n_u"], f3(cr, "%.3f"), f3(st, "%.1f"),
                                                                        f3(sg, "%.2f"), gs[0]["n"] / st[len(st) // 2] / 1e3, ",".join(cks)))
    for shape, k in sorted(set((g["shape"], g["k"]) for g in res)):
        sums = set(g["checksum"] for g in res if (g["shape"], g["k"]) == (shape, k))
        print("checksums of %s, k = %d: %s" % (shape, k, "equal over libraries, switches and rounds" if len(sums) == 1 else "DIFFER: %s" % sorted(sums)))


if __name__ == "__main__":
    main()
