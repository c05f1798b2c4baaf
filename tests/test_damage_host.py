"""What the damage profile (nabwa_damage_*, `nabwa_bam2bam --damage`) can be held to without a device.

The oracle of tests/damage_cases.py, which every other test of the profile compares against, is pinned to the reference program: for the golden
SAM files its tables from toy.pac, toy.ann and toy.amb equal tables derived without the reference genome, from the reference program's own MD:Z
and CIGAR alone (a column's reference base is the read's base unless MD names another; a letter that is no base is a hole).

The argument checks of the library that need no handle, and the tool's refusals before the index is loaded.  An index, and with it a handle,
exists only on a device (nabwa_index_load is NABWA_ENODEV without one), so the checks of nabwa_damage_add's arguments on a live handle are in
tests/test_gpu_damage.py."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import damage_cases as D
import nabwa_testlib as T

nabwa = importlib.import_module("network-aware-bwa_amd")


# ---------------------------------------------------------------------------------------------------------------- the oracle against MD:Z
def md_tables(lines, ref, opt):
    """the tables of SAM lines from flag, CIGAR, SEQ and MD:Z alone -> (tables, reverse-strand records counted, counted records with I, D or S)"""
    t, n_rev, n_gapped = D.Tables(opt["n_pos"]), 0, 0
    n_pos = opt["n_pos"]
    for r in lines:
        t.stats[D.SEEN] += 1
        flag, ops = r["flag"], D.parse_cigar(r["cigar"])
        if (flag & opt["exclude_flags"]) or (flag & opt["require_flags"]) != opt["require_flags"]:
            t.stats[D.SK_FLAGS] += 1
        elif r["rname"] not in ref.ids or r["pos"] < 1:
            t.stats[D.SK_PLACE] += 1
        elif r["mapq"] < opt["min_mapq"]:
            t.stats[D.SK_MAPQ] += 1
        elif r["seq"] == "*" or not ops:
            t.stats[D.SK_EMPTY] += 1
        else:
            seq, L, rev = r["seq"], len(r["seq"]), bool(flag & 16)
            named = []                                   # per M column: None where MD counts a match, else the reference's letter
            for num, dele, letter in re.findall(r"(\d+)|(\^[A-Za-z]+)|([A-Za-z])", r["tags"]["MD"]):
                if num:
                    named += [None] * int(num)
                elif letter:
                    named.append(letter.upper())
            qi = col = 0
            for n, op in ops:
                if op in "M=X":
                    for j in range(n):
                        read, refc = seq[qi + j].upper(), named[col + j]
                        refc = read if refc is None else refc
                        if read not in "ACGT":
                            t.stats[D.COLS_SK_READ] += 1
                            continue
                        if refc not in "ACGT":
                            t.stats[D.COLS_SK_REF] += 1
                            continue
                        rr, q, d5, d3 = "ACGT".index(refc), "ACGT".index(read), qi + j, L - 1 - (qi + j)
                        if rev:
                            rr, q, d5, d3 = 3 - rr, 3 - q, d3, d5
                        t.sub5[min(d5, n_pos), rr, q] += 1
                        t.sub3[min(d3, n_pos), rr, q] += 1
                        t.stats[D.COLS] += 1
                    col += n
                if op in "MIS=X":
                    qi += n
            assert col == len(named) and qi == L, r["name"]
            t.stats[D.COUNTED] += 1
            t.len_hist[min(L, D.LEN_BINS - 1)] += 1
            n_rev += rev
            n_gapped += any(op in "IDS" for _, op in ops)
    return t, n_rev, n_gapped


@pytest.mark.parametrize("sam", D.GOLDEN_SAMS)
def test_oracle_equals_the_reference_programs_md(sam):
    ref = D.toy_ref()
    recs, lines = D.sam_records("%s/%s.sam" % (T.GOLDEN, sam), ref)
    for opt in (D.opt_of(), D.opt_of(n_pos=5, min_mapq=20, exclude_flags=0x4)):
        want, n_rev, n_gapped = md_tables(lines, ref, opt)
        got = D.oracle(ref, opt, recs)
        D.assert_same(got, want, sam)
        assert got.stats[D.COUNTED] > 100 and got.stats[D.COLS] > 35 * got.stats[D.COUNTED] and got.sub5[:, [0, 1, 2, 3], [0, 1, 2, 3]].sum() > 0.9 * got.stats[D.COLS]
        if sam == "se_adna" and opt == D.opt_of():
            assert len(lines) == 606 and [int(got.stats[k]) for k in (D.COUNTED, D.COLS, D.COLS_SK_READ, D.COLS_SK_REF)] == [536, 50022, 72, 5]
            assert (n_rev, n_gapped) == (247, 143)


# ---------------------------------------------------------------------------------------------------------------- the library without a device
def test_default_options():
    o = nabwa.DamageOpt(1, 2, 3, 4, 5, 6)
    nabwa.lib().nabwa_damage_default_opt(C.byref(o))
    assert (o.n_pos, o.min_mapq, o.exclude_flags, o.require_flags, o.which_ref, o.pad) == (25, 0, 0xF04, 0, 0, 0)
    assert C.sizeof(nabwa.DamageOpt) == 24
    assert nabwa.damage_stat_names == D.STAT_NAMES and nabwa.DAMAGE_LEN_BINS == D.LEN_BINS


def test_argument_checks_come_before_the_device():
    L = nabwa.lib()
    o = nabwa.DamageOpt()
    L.nabwa_damage_default_opt(C.byref(o))
    h = C.c_void_p(0x1234)
    assert L.nabwa_damage_create(None, C.byref(o), C.byref(h)) == nabwa.EINVAL and not h.value           # no index; *out is null after a failure
    # the options are looked at before the index is (include/nabwa.h): `some` is never read
    some = C.create_string_buffer(4096)
    assert L.nabwa_damage_create(some, None, C.byref(h)) == nabwa.EINVAL
    assert L.nabwa_damage_create(some, C.byref(o), None) == nabwa.EINVAL
    for n_pos in (0, -1, 257, 2 ** 31 - 1):
        bad = nabwa.DamageOpt(n_pos, 0, 0xF04, 0, 0, 0)
        assert L.nabwa_damage_create(some, C.byref(bad), C.byref(h)) == nabwa.EINVAL and b"n_pos" in L.nabwa_last_error()
    for which in (-1, 2):
        bad = nabwa.DamageOpt(25, 0, 0xF04, 0, which, 0)
        assert L.nabwa_damage_create(some, C.byref(bad), C.byref(h)) == nabwa.EINVAL and b"which_ref" in L.nabwa_last_error()
    data, off = D.join(D.good_records(D.toy_ref(), 3))
    out = np.zeros(16, np.uint64)
    assert L.nabwa_damage_add(None, 3, T.ptr(data), T.ptr(off)) == nabwa.EINVAL
    assert L.nabwa_damage_fetch(None, None, None, None, T.ptr(out)) == nabwa.EINVAL
    assert L.nabwa_damage_clear(None) == nabwa.EINVAL
    assert L.nabwa_damage_times(None, T.ptr(out)) == nabwa.EINVAL
    L.nabwa_damage_destroy(None)


# ---------------------------------------------------------------------------------------------------------------- the tool
def test_tool_says_no_before_the_index_is_loaded(tmp_path):
    exe = os.path.join(os.path.dirname(nabwa.LIB_PATH), "nabwa_bam2bam")
    if not os.path.exists(exe):
        nabwa.build()
    outp, prof = str(tmp_path / "out.bam"), str(tmp_path / "damage.tsv")
    base = {k: v for k, v in os.environ.items() if not k.startswith("NABWA_")}

    def tool(args, env):
        return subprocess.run([exe, "-g", T.TOY, "-f", outp] + args + [str(tmp_path / "no_such.bam")], capture_output=True, text=True, env=dict(base, **env), timeout=120)
    for env in ({"NABWA_DAMAGE_POS": "0"}, {"NABWA_DAMAGE_POS": "257"}, {"NABWA_DAMAGE_POS": "ten"}, {"NABWA_DAMAGE_POS": "2.5"}, {"NABWA_DAMAGE_POS": ""},
                {"NABWA_DAMAGE_MAPQ": "-1"}, {"NABWA_DAMAGE_MAPQ": "256"}, {"NABWA_DAMAGE_MAPQ": "q20"}):
        r = tool(["--damage", prof], env)
        (k, v), = env.items()
        assert r.returncode == 1 and "%s=%s" % (k, v) in r.stderr and "genome length" not in r.stderr, r.stderr
    r = tool(["--damage"], {})                                                      # the switch takes a file
    assert r.returncode == 1
    r = tool([], {"NABWA_DAMAGE_POS": "0", "NABWA_DAMAGE_MAPQ": "q20", "NABWA_DEVICES": str(1 << 20)})      # without the switch the variables are not read
    assert "NABWA_DAMAGE" not in r.stderr and "--damage" not in r.stderr and r.returncode != 0              # (it ends at the index: no such device)
    r = tool(["--damage", prof], {"NABWA_DEVICES": str(1 << 20)})
    assert r.returncode == 2, r.stderr
    assert not os.path.exists(outp) and not os.path.exists(prof)
    r = subprocess.run([exe], capture_output=True, text=True, env=base, timeout=120)
    assert r.returncode == 1 and "--damage FILE" in r.stderr and "NABWA_DAMAGE_POS" in r.stderr and "NABWA_DAMAGE_MAPQ" in r.stderr
