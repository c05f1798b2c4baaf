"""What the command-line tools share (csrc/tool_common.hpp), on the CPU through tests/emu/tool_common_main.cpp: the NABWA_DEVICES
parser, final_rename (utils.c:159-173), the bounded channel between two threads (Chan) and the ordered hand-off of several workers'
results (InOrder).  The thread cases run once more under ThreadSanitizer where g++ can build that."""
import os
import stat
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "tool_common_main.cpp")
BOUND = 10                                    # nabwa_aln's 2 * n_gpus + 2 with four GPUs


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tool_common") / "tool_common_test")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", out, SRC, "-lpthread"], check=True)
    return out


@pytest.fixture(scope="module")
def exe_tsan(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tool_common_tsan") / "tool_common_test")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=thread", "-o", out, SRC, "-lpthread"], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("g++ here does not build with -fsanitize=thread: " + r.stderr.strip()[-300:])
    r = subprocess.run([out, "devices"], capture_output=True, text=True, timeout=10)
    if r.returncode != 0 and "FATAL: ThreadSanitizer" in r.stderr:
        pytest.skip("ThreadSanitizer does not start on this machine: " + r.stderr.strip()[-300:])
    return out


# what the parser of the tools before this header gave (its loop, compiled alone): it stops at the first thing that is no number
@pytest.mark.parametrize("value, alone, with_device_5", [
    ("0,1,2", [0, 1, 2], [0, 1, 2]), ("0,0", [0, 0], [0, 0]), ("", [0], [5]), ("x", [0], [5]), ("1,,2", [1], [1]), ("3,", [3], [3]), (None, [0], [5])])
def test_devices_list(exe, value, alone, with_device_5):
    for device, want in ((None, alone), ("5", with_device_5)):
        env = {k: v for k, v in os.environ.items() if k not in ("NABWA_DEVICES", "NABWA_DEVICE")}
        if value is not None:
            env["NABWA_DEVICES"] = value
        if device is not None:
            env["NABWA_DEVICE"] = device
        r = subprocess.run([exe, "devices"], capture_output=True, text=True, env=env, timeout=10)
        assert r.returncode == 0 and [int(x) for x in r.stdout.split()] == want, (value, device, r.stdout, r.stderr)


def listing(top):
    return sorted(os.path.relpath(os.path.join(d, f), top) for d, _, fs in os.walk(top) for f in fs)


@pytest.mark.parametrize("name, becomes", [("out.bam__", "out.bam"), ("x.sai_", "x.sai"), ("____", None), ("dir/__", None), ("plain", None)])
@pytest.mark.parametrize("check", [0, 1])
def test_final_rename(exe, tmp_path, name, becomes, check):
    (tmp_path / "dir").mkdir()
    (tmp_path / name).write_text("x")
    r = subprocess.run([exe, "rename", name, str(check)], capture_output=True, text=True, cwd=str(tmp_path), timeout=10)
    assert r.returncode == 0 and r.stdout == ""
    assert r.stderr == ("[tool_common_main] finished, renaming %s to %s.\n" % (name, becomes) if becomes else "")
    assert listing(str(tmp_path)) == [becomes or name]


@pytest.mark.parametrize("why", ["directory not writable", "a directory has the new name"])
@pytest.mark.parametrize("check", [0, 1])
def test_final_rename_that_fails(exe, tmp_path, why, check):
    """check off: the line is printed and the run goes on (nabwa_aln, nabwa_samse / nabwa_sampe); on: the run ends (nabwa_bam2bam)"""
    d = tmp_path / "d"
    d.mkdir()
    (d / "out.bam__").write_text("x")
    if why == "directory not writable":
        if os.geteuid() == 0:
            pytest.skip("the superuser renames in a directory without write permission as well")
        os.chmod(str(d), stat.S_IRUSR | stat.S_IXUSR)
    else:
        (d / "out.bam").mkdir()
        (d / "out.bam" / "inside").write_text("y")
    try:
        r = subprocess.run([exe, "rename", "d/out.bam__", str(check)], capture_output=True, text=True, cwd=str(tmp_path), timeout=10)
    finally:
        os.chmod(str(d), stat.S_IRWXU)
    line = "[tool_common_main] finished, renaming d/out.bam__ to d/out.bam.\n"
    if check:
        assert r.returncode == 1 and r.stderr == line + "[tool_common_main] d/out.bam__: cannot rename\n"
    else:
        assert r.returncode == 0 and r.stderr == line
    assert "d/out.bam__" in listing(str(tmp_path)) and not os.path.isfile(str(d / "out.bam"))


def thread_cases(binary):
    for cap in (1, 2):
        r = subprocess.run([binary, "chan", str(cap)], capture_output=True, text=True, timeout=10)
        assert r.returncode == 0 and r.stdout == "ok\n", (cap, r.stderr[-2000:])
    for seed in (1, 2, 3):
        # 0..199 came out in order (the harness checks each); the first run of 8 waited before the consumer started, so results did
        # run ahead, and none was ever BOUND or more ahead of the one handed out next
        r = subprocess.run([binary, "inorder", str(BOUND), str(seed)], capture_output=True, text=True, timeout=10)
        assert r.returncode == 0 and r.stdout.startswith("max_lead "), (seed, r.stderr[-2000:])
        print(r.stdout.strip())
        assert 7 <= int(r.stdout.split()[1]) <= BOUND - 1
    r = subprocess.run([binary, "inorder_fail"], capture_output=True, text=True, timeout=10)      # a deadlock is a failure, not a hang
    assert r.returncode == 0 and r.stdout == "ok\n", r.stderr[-2000:]


def test_chan_and_inorder(exe):
    thread_cases(exe)


def test_chan_and_inorder_under_thread_sanitizer(exe_tsan):
    thread_cases(exe_tsan)
