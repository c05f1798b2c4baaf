"""nabwa_bam2bam file to file with the input inflated on the host and on the GPU (NABWA_BGZF_IN), beside another build's tool where one
is named: the runs are taken in alternation (other, host, gpu, other, ...), three each, on the input profiles/probes/cli_rate.py
left in <dir>/in.bam.  Prints each run's wall time and the reader's part of the timing line, then the medians and spreads.

    python profiles/probes/bgzf_inflate_rate.py <dir> <n_reads> [<other build's nabwa_bam2bam>]"""
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
d, n = sys.argv[1], int(sys.argv[2])
setups = [("host", os.path.join(ROOT, "network-aware-bwa_amd", "nabwa_bam2bam"), {"NABWA_BGZF_IN": "host"}),
          ("gpu", os.path.join(ROOT, "network-aware-bwa_amd", "nabwa_bam2bam"), {"NABWA_BGZF_IN": "gpu"})]
if len(sys.argv) > 3:
    setups.insert(0, ("other", sys.argv[3], {}))
inp, outp = os.path.join(d, "in.bam"), os.path.join(d, "out.bam")
wall = {k: [] for k, _, _ in setups}
for rep in range(3):
    for name, exe, env in setups:
        t0 = time.time()
        r = subprocess.run([exe, "-g", os.path.join(ROOT, "tests", "golden", "toy"), "-f", outp, inp], capture_output=True, text=True,
                           env=dict(os.environ, NABWA_TIMING="1", **env))
        dt = time.time() - t0
        if r.returncode:
            print(r.stderr[-2000:])
            sys.exit("%s: rc %d" % (name, r.returncode))
        wall[name].append(dt)
        line = [l for l in r.stderr.split("\n") if "timing: reader thread" in l][-1]
        m = re.search(r"reader thread ([0-9.]+) s busy \(([0-9.]+) s of it inflate, ([^)]*)\).*\(\+ ([0-9.]+) s waiting for input", line)
        print("%-5s run %d: %.2f s wall, %.2f M reads/s; reader %s s busy, %s s inflate (%s), main thread waited %s s for input"
              % (name, rep, dt, n / dt / 1e6, m.group(1), m.group(2), m.group(3), m.group(4)), flush=True)
for name, v in wall.items():
    print("%-5s wall: median %.2f s, min %.2f, max %.2f" % (name, statistics.median(v), min(v), max(v)))
