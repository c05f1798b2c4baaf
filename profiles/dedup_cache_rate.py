"""What NABWA_DEDUP_CACHE costs where no read of a batch was seen before, and what it gains where some were: a SEQUENCE
of batches of bench.py's two single-end shapes -- 100 bp reads under the default options, reads of 50-76 bp under the ancient-DNA options --
on the GRCh38-sized synthetic index, in which a stated share of each batch's reads (0 %, 25 %, 50 %) occurred in earlier batches of the
sequence and the rest are new.

    python profiles/dedup_cache_rate.py [--parent-lib PATH/libnabwa.so] [--rounds 3] [--batches 4] [--reads N] [--adna-reads N]
                                        [--cache-mib 16384] [--genome-len N] [--out profiles/dedup_cache_rate.txt]

One child process per library and round, the libraries in turn within the one command; a child builds the index, then runs every sequence:
this tree with NABWA_DEDUP=1 NABWA_DEDUP_CACHE=<MiB> (the cache cleared before each sequence), the parent commit's library (--parent-lib)
with NABWA_DEDUP=1 alone.  Per batch: wall time of nabwa_batch_create, wall time of its one run + sync step (a batch of a stream runs
once; the insert stage is part of that sync), the lookup and insert stages' own HIP-event times from their NABWA_TIMING lines, reads
searched and served, bytes per entry, the row checksum.  The summary goes to stdout and, with --out, to that file."""
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
LOOKUP = re.compile(r"\[nabwa\] dedup cache: (\d+) reads looked up, (\d+) to search, (\d+) served, stage ([0-9.]+) ms")
INSERT = re.compile(r"\[nabwa\] dedup cache: (\d+) reads searched, (\d+) entered, (\d+) not .*?stage ([0-9.]+) ms")
SHARES = (0, 25, 50)


def take(seq, rseq, off, ids):
    """reads ids of (seq, rseq, off), in that order -> (seq, rseq, off)"""
    lens = np.diff(off)[ids]
    new_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    out_s, out_r = np.empty(new_off[-1], np.uint8), np.empty(new_off[-1], np.uint8)
    for lo in range(0, len(ids), 1 << 20):
        hi = min(len(ids), lo + (1 << 20))
        src = np.repeat(off[ids[lo:hi]] - new_off[lo:hi], lens[lo:hi]) + np.arange(new_off[lo], new_off[hi])
        out_s[new_off[lo]:new_off[hi]] = seq[src]
        out_r[new_off[lo]:new_off[hi]] = rseq[src]
    return out_s, out_r, new_off


def sequence(n_pool, n_batch, n_batches, share, seed):
    """ids into a pool of n_pool different reads, per batch: share % of a batch's reads are drawn from the reads of the batches before it
    (none in the first batch), the others are the pool's next unused reads; shuffled"""
    rng = np.random.default_rng(seed)
    out, used = [], 0
    for j in range(n_batches):
        n_old = n_batch * share // 100 if j else 0
        old = rng.choice(used, n_old, replace=False) if n_old else np.zeros(0, np.int64)
        new = np.arange(used, used + n_batch - n_old)
        used += n_batch - n_old
        assert used <= n_pool
        out.append(rng.permutation(np.concatenate([old, new]).astype(np.int64)))
    return out


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
    shapes.append(("default 100 bp", opt, args.reads, synth.synth_reads(d_text, n, args.reads * args.batches, 100, 2000, 0, 2)))
    seq, rseq, off = synth.synth_reads(d_text, n, args.adna_reads * args.batches, 76, 10000, 0, 2)
    opt = nabwa.gap_init_opt()
    opt.fnr, opt.max_diff, opt.max_gapo, opt.seed_len = 0.01, -1, 2, 16500
    shapes.append(("ancient-DNA 50-76 bp", opt, args.adna_reads, bench.adna_profile(seq, args.adna_reads * args.batches, 76, 5)))
    d_text.free()
    os.environ.pop("NABWA_DEDUP_CACHE", None)
    os.environ["NABWA_DEDUP"] = "1"
    ix.cal_sa_reg_gap_flat(shapes[0][1], shapes[0][3][0][:100000], shapes[0][3][1][:100000], shapes[0][3][2][:1001], per_read=True)      # code objects, pool
    this = args.child == "this"
    if this:
        os.environ["NABWA_DEDUP_CACHE"] = str(args.cache_mib)
    for shape, opt, n_batch, reads in shapes:
        for share in SHARES:
            if this and hasattr(ix, "dedup_cache_clear"):
                ix.dedup_cache_clear()
            for j, ids in enumerate(sequence(len(reads[2]) - 1, n_batch, args.batches, share, 100 + share)):
                seq, rseq, off = take(*reads, ids)
                t0 = time.time()
                b = nabwa.Batch(ix, opt, seq, rseq, off, per_read=True)
                create_s = time.time() - t0
                t0 = time.time()
                b.run()
                b.sync()
                step_ms = 1e3 * (time.time() - t0)
                cks, rows = b.checksum()
                st = b.dedup_stats_ex() if this else b.dedup_stats() + [0, 0, 0, 0]
                cs = ix.dedup_cache_stats() if this else [0] * 8
                b.close()
                print(json.dumps(dict(lib=args.child, shape=shape, share=share, batch=j, n=st[0], searched=st[1], served=st[4], entered=st[5], not_entered=st[6],
                                      entries=cs[2], used=cs[1], create_s=create_s, step_ms=step_ms, checksum="%016x" % cks, rows=rows)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--reads", type=int, default=4 << 20)          # nabwa_aln's batch
    ap.add_argument("--adna-reads", type=int, default=1 << 20)     # nabwa_bam2bam's batch
    ap.add_argument("--cache-mib", type=int, default=16384)
    ap.add_argument("--genome-len", type=int, default=3099734149)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    res = []
    for rnd in range(args.rounds):
        for which in (["parent"] if args.parent_lib else []) + ["this"]:
            env = dict(os.environ, NABWA_TIMING="1")
            for v in ("NABWA_DEDUP", "NABWA_DEDUP_CACHE", "NABWA_DEDUP_HASH_BITS", "NABWA_LIB"):
                env.pop(v, None)
            if which == "parent":
                env["NABWA_LIB"] = args.parent_lib
            cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--batches", str(args.batches), "--reads", str(args.reads),
                   "--adna-reads", str(args.adna_reads), "--genome-len", str(args.genome_len), "--cache-mib", str(args.cache_mib)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True)
            if r.returncode != 0:
                sys.exit("round %d, %s: exit %d\n%s" % (rnd, which, r.returncode, r.stderr[-3000:]))
            got = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
            if which == "this":      # the stages' lines, in the order of the batches (the warm-up call has the switch off)
                look, ins = [float(m[3]) for m in LOOKUP.findall(r.stderr)], [float(m[3]) for m in INSERT.findall(r.stderr)]
                assert len(look) == len(got), (len(look), len(got))
                ins_of = iter(ins)
                for g, ms in zip(got, look):
                    g["lookup_ms"] = ms
                    g["insert_ms"] = next(ins_of) if g["searched"] else 0.0      # a batch with nothing searched has no insert stage
            for g in got:
                g["round"] = rnd
                print("# " + json.dumps(g), flush=True)
            res += got
    lines = []
    lines.append("%-22s %5s %5s %-7s %9s %9s %9s %7s  %-24s %-26s %-20s %-20s %s" % (
        "shape", "share", "batch", "library", "reads", "searched", "served", "B/entry", "create s (min med max)", "step ms (min med max)", "lookup ms (min med max)",
        "insert ms (min med max)", "checksum"))
    f3 = lambda v, fmt: " ".join(fmt % x for x in (v[0], v[len(v) // 2], v[-1])) if v else "-"
    keys = []
    for g in res:
        key = (g["shape"], g["share"], g["batch"], g["lib"])
        if key not in keys:
            keys.append(key)
    for key in sorted(keys, key=lambda k: (k[0], k[1], k[2], k[3] != "parent")):
        gs = [g for g in res if (g["shape"], g["share"], g["batch"], g["lib"]) == key]
        per = "%.0f" % (gs[0]["used"] / gs[0]["entries"]) if gs[0]["entries"] else "-"
        lines.append("%-22s %5d %5d %-7s %9d %9d %9d %7s  %-24s %-26s %-20s %-20s %s" % (
            key[0], key[1], key[2], key[3], gs[0]["n"], gs[0]["searched"], gs[0]["served"], per, f3(sorted(g["create_s"] for g in gs), "%.3f"),
            f3(sorted(g["step_ms"] for g in gs), "%.1f"), f3(sorted(g["lookup_ms"] for g in gs if "lookup_ms" in g), "%.2f"),
            f3(sorted(g["insert_ms"] for g in gs if "insert_ms" in g), "%.2f"), ",".join(sorted(set(g["checksum"] for g in gs)))))
    for shape in sorted(set(g["shape"] for g in res)):      # the parent's run-to-run spread: what a difference has to exceed to be one
        ps = [g for g in res if g["shape"] == shape and g["lib"] == "parent"]
        by = {}
        for g in ps:
            by.setdefault((g["share"], g["batch"]), []).append(g["step_ms"])
        spread = [100.0 * (max(v) - min(v)) / min(v) for v in by.values() if len(v) > 1]
        if spread:
            lines.append("parent's run-to-run spread of a step, %s: max - min over the rounds, %.1f %% at the median batch, %.1f %% at the worst" % (
                shape, sorted(spread)[len(spread) // 2], max(spread)))
    for shape, share, batch in sorted(set((g["shape"], g["share"], g["batch"]) for g in res)):
        sums = set(g["checksum"] for g in res if (g["shape"], g["share"], g["batch"]) == (shape, share, batch))
        if len(sums) != 1:
            lines.append("checksums of %s, share %d, batch %d DIFFER: %s" % (shape, share, batch, sorted(sums)))
    if all(len(set(g["checksum"] for g in res if (g["shape"], g["share"], g["batch"]) == k)) == 1 for k in set((g["shape"], g["share"], g["batch"]) for g in res)):
        lines.append("checksums: equal over libraries and rounds for every batch")
    print("\n" + "\n".join(lines))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
