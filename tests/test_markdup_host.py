"""What duplicate marking (nabwa_markdup_*, nabwa_bam_sort_ex, `nabwa_bam2bam --sort --mark-duplicates`) can be held to without a device: the
argument checks of the library, which come before the device is touched (and before the handle is looked at, so that any address stands in
for one here; the checks on a live handle are in tests/test_gpu_markdup.py), the default options, the names of the counters, and the tool's
refusals before the index is loaded."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np

import bamlib as B
import markdup_cases as M
import nabwa_testlib as T

nabwa = importlib.import_module("network-aware-bwa_amd")


def test_default_options_and_counter_names():
    o = nabwa.MarkDupOpt(1, 2, 3, 4)
    nabwa.lib().nabwa_markdup_default_opt(C.byref(o))
    assert (o.min_qual, o.single_ends, o.exclude_flags, o.pad) == (15, 0, 0xB00, 0)
    nabwa.lib().nabwa_markdup_default_opt(None)
    assert C.sizeof(nabwa.MarkDupOpt) == 16
    assert nabwa.markdup_stat_names == M.STAT_NAMES and nabwa.MARKDUP_ENDS == {"5p": M.ENDS_5P, "both": M.ENDS_BOTH}
    # the enum of include/nabwa.h, in its order
    text = open(os.path.join(T.ROOT, "include", "nabwa.h")).read()
    body = re.search(r"enum \{ (NABWA_MARKDUP_STAT_SEEN = 0,.*?NABWA_MARKDUP_N_STATS) \};", text, re.S).group(1)
    names = [x.strip().split(" ")[0] for x in body.split(",")]
    assert names == ["NABWA_MARKDUP_STAT_" + n.upper() for n in M.STAT_NAMES] + ["NABWA_MARKDUP_N_STATS"]
    assert re.search(r"#define NABWA_MARKDUP_ENDS_5P\s+0\n#define NABWA_MARKDUP_ENDS_BOTH\s+1\n", text)


def test_argument_checks_come_before_the_device():
    L = nabwa.lib()
    o = nabwa.MarkDupOpt()
    L.nabwa_markdup_default_opt(C.byref(o))
    h = C.c_void_p(0x1234)
    assert L.nabwa_markdup_create(0, None, C.byref(h)) == nabwa.EINVAL and not h.value              # *out is null after a failure
    assert L.nabwa_markdup_create(0, C.byref(o), None) == nabwa.EINVAL
    for q in (-1, 256, 2 ** 31 - 1):
        assert L.nabwa_markdup_create(1 << 20, C.byref(nabwa.MarkDupOpt(q, 0, 0xB00, 0)), C.byref(h)) == nabwa.EINVAL and b"min_qual" in L.nabwa_last_error()
    for e in (-1, 2):
        assert L.nabwa_markdup_create(1 << 20, C.byref(nabwa.MarkDupOpt(15, e, 0xB00, 0)), C.byref(h)) == nabwa.EINVAL and b"single_ends" in L.nabwa_last_error()
    data, off = B.pack(M.random_records(5, 1)[:5])
    out = np.zeros(16, np.uint64)
    assert L.nabwa_markdup_add(None, 5, T.ptr(data), T.ptr(off)) == nabwa.EINVAL
    assert L.nabwa_markdup_resolve(None, T.ptr(out), 16, T.ptr(out)) == nabwa.EINVAL
    assert L.nabwa_markdup_clear(None) == nabwa.EINVAL
    assert L.nabwa_markdup_times(None, T.ptr(out)) == nabwa.EINVAL
    L.nabwa_markdup_destroy(None)
    # what nabwa_markdup_add decides from its other arguments comes before the handle is looked at: `some` is never read
    some = C.create_string_buffer(4096)
    assert L.nabwa_markdup_add(some, -1, T.ptr(data), T.ptr(off)) == nabwa.EINVAL and b"n_rec" in L.nabwa_last_error()
    assert L.nabwa_markdup_add(some, 1 << 31, T.ptr(data), T.ptr(off)) == nabwa.EINVAL and b"n_rec" in L.nabwa_last_error()
    assert L.nabwa_markdup_add(some, 5, None, T.ptr(off)) == nabwa.EINVAL
    assert L.nabwa_markdup_add(some, 5, T.ptr(data), None) == nabwa.EINVAL
    bad = off.copy(); bad[0] = -1
    assert L.nabwa_markdup_add(some, 5, T.ptr(data), T.ptr(bad)) == nabwa.EINVAL and b"negative" in L.nabwa_last_error()
    bad = off.copy(); bad[3] = bad[2]
    assert L.nabwa_markdup_add(some, 5, T.ptr(data), T.ptr(bad)) == nabwa.EINVAL and b"record 2" in L.nabwa_last_error()
    bad = off.copy(); bad[3] = bad[2] + 35
    assert L.nabwa_markdup_add(some, 5, T.ptr(data), T.ptr(bad)) == nabwa.EINVAL and b"at least 36" in L.nabwa_last_error()
    assert L.nabwa_markdup_add(some, 0, None, T.ptr(off)) == nabwa.OK
    assert L.nabwa_markdup_resolve(some, T.ptr(out), -1, T.ptr(out)) == nabwa.EINVAL
    assert L.nabwa_markdup_times(some, None) == nabwa.EINVAL
    try:
        nabwa.MarkDup(single_ends="3p")
    except ValueError as e:
        assert "single_ends" in str(e)
    else:
        raise AssertionError("single_ends='3p' was taken")


def test_sort_with_permutation_checks_its_arguments_like_the_sort():
    L = nabwa.lib()
    data, off = B.pack(M.random_records(5, 2)[:5])
    total = int(off[-1])
    out, out_off, keys, perm = np.zeros(total, np.uint8), np.zeros(6, np.int64), np.zeros(5, np.uint64), np.zeros(5, np.uint32)
    a = (T.ptr(data), T.ptr(off), T.ptr(out))
    for dev in (0, 1 << 20):                                           # decided before the device is looked for
        assert L.nabwa_bam_sort_ex(dev, -1, *a, total, T.ptr(out_off), T.ptr(keys), T.ptr(perm)) == nabwa.EINVAL
        assert L.nabwa_bam_sort_ex(dev, 1 << 31, *a, total, None, None, T.ptr(perm)) == nabwa.EINVAL
        assert L.nabwa_bam_sort_ex(dev, 5, None, T.ptr(off), T.ptr(out), total, None, None, T.ptr(perm)) == nabwa.EINVAL
        assert L.nabwa_bam_sort_ex(dev, 5, T.ptr(data), None, T.ptr(out), total, None, None, T.ptr(perm)) == nabwa.EINVAL
        assert L.nabwa_bam_sort_ex(dev, 5, T.ptr(data), T.ptr(off), None, total, None, None, T.ptr(perm)) == nabwa.EINVAL
        assert L.nabwa_bam_sort_ex(dev, 5, *a, -1, None, None, T.ptr(perm)) == nabwa.EINVAL
        assert L.nabwa_bam_sort_ex(dev, 5, *a, total - 1, None, None, T.ptr(perm)) == nabwa.ECAP and str(total).encode() in L.nabwa_last_error()
        bad = off.copy(); bad[2] = bad[1]
        assert L.nabwa_bam_sort_ex(dev, 5, T.ptr(data), T.ptr(bad), T.ptr(out), total, None, None, T.ptr(perm)) == nabwa.EINVAL
        bad = off.copy(); bad[2] = bad[1] + 35
        assert L.nabwa_bam_sort_ex(dev, 5, T.ptr(data), T.ptr(bad), T.ptr(out), total, None, None, T.ptr(perm)) == nabwa.EINVAL
        assert L.nabwa_bam_sort_ex(dev, 0, None, T.ptr(off), None, 0, None, None, None) == nabwa.OK
    assert L.nabwa_bam_sort_run_ex(None, 5, *a, total, None, None, T.ptr(perm)) == nabwa.EINVAL
    assert not out.any() and not perm.any()


def test_tool_says_no_before_the_index_is_loaded(tmp_path):
    exe = os.path.join(os.path.dirname(nabwa.LIB_PATH), "nabwa_bam2bam")
    if not os.path.exists(exe):
        nabwa.build()
    outp = str(tmp_path / "out.bam")
    base = {k: v for k, v in os.environ.items() if not k.startswith("NABWA_")}

    def tool(args, env):
        return subprocess.run([exe, "-g", T.TOY, "-f", outp] + args + [str(tmp_path / "no_such.bam")], capture_output=True, text=True, env=dict(base, **env), timeout=120)
    for switch in ("--mark-duplicates", "--remove-duplicates"):
        r = tool([switch], {})
        assert r.returncode == 1 and "%s needs --sort" % switch in r.stderr and "genome length" not in r.stderr, r.stderr
        for env in ({"NABWA_MARKDUP_ENDS": "3p"}, {"NABWA_MARKDUP_ENDS": ""}, {"NABWA_MARKDUP_ENDS": "BOTH"}, {"NABWA_MARKDUP_QUAL": "-1"}, {"NABWA_MARKDUP_QUAL": "94"},
                    {"NABWA_MARKDUP_QUAL": "q20"}, {"NABWA_MARKDUP_QUAL": ""}, {"NABWA_MARKDUP_QUAL": "1.5"}):
            r = tool(["--sort", switch], env)
            (k, v), = env.items()
            assert r.returncode == 1 and "%s=%s" % (k, v) in r.stderr and "genome length" not in r.stderr, r.stderr
        r = tool(["--sort", switch], {"NABWA_DEVICES": str(1 << 20), "NABWA_SORT": "host"})      # no usable device: nothing is written, and no host path takes over
        assert r.returncode == 2 and switch in r.stderr and "genome length" not in r.stderr, r.stderr
    r = tool(["--sort", "--mark-duplicates", "--remove-duplicates"], {})
    assert r.returncode == 1 and "--mark-duplicates and --remove-duplicates" in r.stderr and "genome length" not in r.stderr
    r = tool(["--sort"], {"NABWA_MARKDUP_ENDS": "3p", "NABWA_MARKDUP_QUAL": "q20", "NABWA_DEVICES": str(1 << 20)})      # without the switch the variables are not read
    assert "NABWA_MARKDUP" not in r.stderr and r.returncode != 0
    assert not os.path.exists(outp)
    r = subprocess.run([exe], capture_output=True, text=True, env=base, timeout=120)
    assert r.returncode == 1 and "--mark-duplicates" in r.stderr and "--remove-duplicates" in r.stderr and "NABWA_MARKDUP_ENDS" in r.stderr and "NABWA_MARKDUP_QUAL" in r.stderr
    assert "no host" in r.stderr
