"""The reference's struct layouts as numbers, for the ABI tests (test_abi_headers.py, test_wire.py).

Where the reference's headers are at hand (the build container), the C compiler is asked for the sizes and member offsets of its
structs; tests/golden/make_ref_abi.py stores what it answered in tests/golden/ref_abi.json, together with the digest of the
INTEGRATION.md snippets it compiled against those headers.  Everywhere else the tests check include/nabwa.h against the stored
numbers, so they need nothing outside the repository.  Test infrastructure only; no reference source text is stored."""
import hashlib
import json
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("NABWA_REFERENCE", "/root/reference")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_abi.json")

# struct -> members whose offsets the ABI relies on (the same names on both sides unless mapped in NABWA_OF)
MEMBERS = {
    "gap_opt_t": ["s_mm", "s_gapo", "s_gape", "mode", "indel_end_skip", "max_del_occ", "max_entries", "fnr", "max_diff", "max_gapo",
                  "max_gape", "max_seed_diff", "seed_len", "n_threads", "max_top2", "trim_qual"],
    "bwt_aln1_t": ["k", "l", "score"],
    "bwa_seq_t": ["name", "seq", "rseq", "qual", "score", "clip_len", "n_aln", "aln", "n_multi", "multi", "sa", "pos", "n_cigar",
                  "cigar", "tid", "bc", "md", "max_entries"],
    "pe_opt_t": ["max_isize", "force_isize", "max_occ", "max_occ_se", "n_multi", "N_multi", "type", "is_sw", "is_preload", "ap_prior"],
    "isize_info_t": ["avg", "std", "ap_prior", "low", "high", "high_bayesian"],
    "bwt_multi1_t": ["cigar"],
}
NABWA_OF = {"gap_opt_t": "nabwa_gap_opt_t", "bwt_aln1_t": "nabwa_aln1_t", "bwa_seq_t": "nabwa_bwa_seq_t", "pe_opt_t": "nabwa_pe_opt_t",
            "isize_info_t": "nabwa_isize_t"}
NABWA_EXTRA = {"nabwa_bwa_seq_t": ["bits0", "bits1", "c1c2seq", "lenbits"]}

# the message's raw blocks (test_wire.py): sizes, and the words bam1_core_t / bwt_multi1_t leave in memory for known field values
RAW_BLOCKS = r'''
#include <stdio.h>
#include <string.h>
#include "bamlite.h"
#include "bwtaln.h"
int main(void) {
    bam1_core_t c; unsigned w[8]; bwt_multi1_t m; unsigned mw[4];
    memset(&c, 0, sizeof c); c.bin = 4681; c.qual = 37; c.l_qname = 9; c.flag = 0x63; c.n_cigar = 5; memcpy(w, &c, 32);
    memset(&m, 0, sizeof m); m.pos = 777; m.gap = 3; m.mm = 2; m.strand = 1; memcpy(mw, &m, 16);
    printf("%zu %zu %zu %zu %zu %u %u %u %u\n", sizeof(bam1_core_t), sizeof(bwt_multi1_t), sizeof(bwt_aln1_t), sizeof(gap_opt_t), sizeof(pe_opt_t), w[2], w[3], mw[0], mw[1]);
    return 0; }
'''


def have_reference():
    return os.path.isdir(REF)


def load():
    with open(GOLDEN) as f:
        return json.load(f)


def _run_probe(src, includes):
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "probe.c")
        with open(c, "w") as f:
            f.write(src)
        exe = os.path.join(td, "probe")
        subprocess.run(["gcc", "-std=gnu11", "-fgnu89-inline", "-w"] + ["-I" + i for i in includes] + ["-o", exe, c], check=True)
        return subprocess.run([exe], capture_output=True, text=True, check=True).stdout


def _layout_probe(headers, structs):
    """C source printing `name size` and `name.member offset` lines for structs = {type: [members]}"""
    lines = ["#include <stdio.h>", "#include <stddef.h>", "#include <stdint.h>", "#include <stdlib.h>"] + ['#include "%s"' % h for h in headers]
    lines.append("int main(void) {")
    for t, ms in structs.items():
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (t, t))
        for m in ms:
            lines.append('    printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (t, m, t, m))
    lines.append("    return 0; }")
    return "\n".join(lines) + "\n"


def _parse(out):
    return {k: int(v) for k, v in (line.split() for line in out.splitlines())}


def measure_reference_layouts():
    """{"gap_opt_t": 64, "gap_opt_t.s_mm": 0, ...} of the reference's headers (needs them)"""
    return _parse(_run_probe(_layout_probe(["bwtaln.h", "bwase.h", "bwape.h"], MEMBERS), [REF]))


def measure_nabwa_layouts():
    """the same numbers for include/nabwa.h's counterparts, under their own names"""
    structs = {}
    for t, ms in MEMBERS.items():
        if t in NABWA_OF and t != "isize_info_t":
            structs[NABWA_OF[t]] = list(ms)
    structs["nabwa_isize_t"] = list(MEMBERS["isize_info_t"])
    for t, ms in NABWA_EXTRA.items():
        structs[t] = structs[t] + ms
    return _parse(_run_probe(_layout_probe(["nabwa.h"], structs), [os.path.join(ROOT, "include")]))


def measure_raw_blocks():
    return [int(x) for x in _run_probe(RAW_BLOCKS, [REF]).split()]


def integration_snippets():
    """every ```c block of INTEGRATION.md, in order"""
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        return re.findall(r"```c\n(.*?)```", f.read(), re.S)


def snippets_digest(blocks):
    return hashlib.sha256("\n".join(blocks).encode()).hexdigest()
