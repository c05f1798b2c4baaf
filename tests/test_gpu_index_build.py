"""`nabwa_index` -- the reference's `bwa index` (bwtindex.c:39-196) with both FM-indexes built on the GPU (index_build.hip).
All eight files (.pac .ann .amb .rpac .bwt .rbwt .sa .rsa) must be byte for byte what the reference writes:
 * against the committed toy index (tests/golden/toy.*);
 * against the compiled reference run on the spot (oracle/_ref/bwa_ref, when it travelled) for the packing-quirk inputs of
   test_index_pac.py and for texts that need many prefix-doubling rounds: a 100 kb homopolymer, a 171 bp unit repeated 2 000
   times, exact 50 kb segmental duplicates, a 10 Mbp genome with repeat families -- `-a is` and `-a bwtsw` both;
 * the colour-space index (-c);
and an index built here must give `nabwa_aln` the committed .sai.  The device-memory check refuses a build over the budget
before anything is allocated."""
import importlib
import os
import subprocess

import pytest

import indexgen
import nabwa_testlib as T

pytestmark = pytest.mark.gpu

nabwa = importlib.import_module("network-aware-bwa_amd")
TOOL = os.path.join(T.ROOT, "network-aware-bwa_amd", "nabwa_index")
ALN = os.path.join(T.ROOT, "network-aware-bwa_amd", "nabwa_aln")
REFBIN = os.path.join(T.ROOT, "oracle", "_ref", "bwa_ref")
ALL_FILES = ("pac", "ann", "amb", "rpac", "bwt", "rbwt", "sa", "rsa")
DOUBLING_CASES = ("homopolymer", "tandem", "segdup", "repeats10m")


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(TOOL):          # built with the library (csrc/Makefile: all)
        nabwa.build()
    assert os.path.exists(TOOL)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("index_inputs"))
    cases = dict(indexgen.quirk_cases(root))
    cases["homopolymer"] = indexgen.homopolymer(root)
    cases["tandem"] = indexgen.tandem(root)
    cases["segdup"] = indexgen.segdup(root)
    cases["repeats10m"] = indexgen.repeat_genome(root)
    return cases


def read(path):
    with open(path, "rb") as f:
        return f.read()


def run_tool(args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([TOOL] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=900)
    return r.returncode, r.stderr.decode(errors="replace")


def ref_index(args, prefix, fasta):
    if not os.path.exists(REFBIN):
        pytest.skip("the compiled reference (oracle/_ref/bwa_ref) did not travel")
    r = subprocess.run([REFBIN, "index"] + args + ["-p", prefix, fasta], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=1800)
    assert r.returncode == 0, r.stderr.decode(errors="replace")


def assert_same(got, want, exts):
    for ext in exts:
        a, b = read("%s.%s" % (got, ext)), read("%s.%s" % (want, ext))
        assert len(a) == len(b) and a == b, ".%s differs (%d vs %d bytes)" % (ext, len(a), len(b))


def test_toy_index_equals_golden(tmp_path):
    rc, err = run_tool(["-p", str(tmp_path / "toy"), os.path.join(T.GOLDEN, "toy.fa")])
    assert rc == 0, err
    assert_same(str(tmp_path / "toy"), T.TOY, ("pac", "ann", "amb", "bwt", "rbwt", "sa", "rsa"))
    assert "forward index" in err and "reverse index" in err and "device memory: peak" in err


@pytest.mark.parametrize("case", list(indexgen.QUIRK_CASES) + list(DOUBLING_CASES))
def test_index_equals_reference(tmp_path, inputs, case):
    ref_index(["-a", "is"], str(tmp_path / "ref"), inputs[case])
    rc, err = run_tool(["-p", str(tmp_path / "got"), inputs[case]])
    assert rc == 0, err
    assert_same(str(tmp_path / "got"), str(tmp_path / "ref"), ALL_FILES)


def test_bwtsw_on_10_mbp_agrees(tmp_path, inputs):
    """the reference's two construction algorithms write the same index, and so does the GPU builder under either -a"""
    fasta = inputs["repeats10m"]
    ref_index(["-a", "bwtsw"], str(tmp_path / "sw"), fasta)
    ref_index(["-a", "is"], str(tmp_path / "is"), fasta)
    assert_same(str(tmp_path / "sw"), str(tmp_path / "is"), ALL_FILES)
    rc, err = run_tool(["-a", "bwtsw", "-p", str(tmp_path / "got"), fasta])
    assert rc == 0, err
    assert_same(str(tmp_path / "got"), str(tmp_path / "sw"), ALL_FILES)


@pytest.mark.parametrize("case", ["gzip", "segdup"])
def test_colour_index_equals_reference(tmp_path, inputs, case):
    ref_index(["-c"], str(tmp_path / "ref"), inputs[case])
    rc, err = run_tool(["-c", "-p", str(tmp_path / "got"), inputs[case]])
    assert rc == 0, err
    assert_same(str(tmp_path / "got"), str(tmp_path / "ref"), ("nt.pac", "nt.ann", "nt.amb") + ALL_FILES)


def test_aln_on_a_gpu_built_index_writes_the_golden_sai(tmp_path):
    rc, err = run_tool(["-p", str(tmp_path / "toy"), os.path.join(T.GOLDEN, "toy.fa")])
    assert rc == 0, err
    r = subprocess.run([ALN, str(tmp_path / "toy"), os.path.join(T.GOLDEN, "reads_se.fq")], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    assert r.stdout == read(os.path.join(T.GOLDEN, "se_default.sai"))


def test_library_entries_build_the_toy_index(tmp_path):
    prefix = str(tmp_path / "toy")
    n = nabwa.index_fa2pac(os.path.join(T.GOLDEN, "toy.fa"), prefix)
    nabwa.index_build(prefix, device=0)
    assert_same(prefix, T.TOY, ("bwt", "rbwt", "sa", "rsa"))
    assert nabwa.index_build_estimate(n) >= 41 * (n + 1)


def test_over_budget_build_is_refused_before_allocating(tmp_path):
    prefix = str(tmp_path / "toy")
    n = nabwa.index_fa2pac(os.path.join(T.GOLDEN, "toy.fa"), prefix)
    cap = nabwa.index_build_estimate(n) - 1
    env = {"NABWA_INDEX_MAX_BYTES": str(cap)}
    rc, err = run_tool(["-p", str(tmp_path / "cli"), os.path.join(T.GOLDEN, "toy.fa")], env)
    assert rc == 2 and "needs up to" in err and "NABWA_INDEX_MAX_BYTES" in err, err
    assert not any(os.path.exists(str(tmp_path / "cli") + "." + e) for e in ("bwt", "rbwt", "sa", "rsa"))
    old = os.environ.get("NABWA_INDEX_MAX_BYTES")
    os.environ["NABWA_INDEX_MAX_BYTES"] = str(cap)
    try:
        with pytest.raises(nabwa.NabwaError) as e:
            nabwa.index_build(prefix, device=0)
        assert e.value.code == nabwa.ENOMEM
    finally:
        if old is None:
            del os.environ["NABWA_INDEX_MAX_BYTES"]
        else:
            os.environ["NABWA_INDEX_MAX_BYTES"] = old
    assert not os.path.exists(prefix + ".bwt")
