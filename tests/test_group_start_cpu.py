"""The start bookkeeping of the interior term's waves (psdr_jit_amd/csrc/hip/group_start.h: when a wave starts samples, and which queue positions a start hands to
which lane) checked on the host by tests/cpp/group_start_check.cpp, which plays the loop of paths.h::run_paths with random path lengths and live masks: every live
position handed out exactly once and in order, grouped starts fill every idle lane while work is left, every wave's loop ends - for the thresholds 1, 16, 32, 48, 64,
queues of 0 to 1 000 positions and live fractions 0 to 1.  No GPU: compiled by g++ alone, once plainly and once with the address and undefined-behaviour sanitizers
(a stand-alone program; skipped where g++ cannot link their runtimes)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "group_start_check.cpp")


def _compile(exe, extra=()):
    return subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + ROOT] + list(extra) + [SRC, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _run(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout[-3000:]


def test_start_bookkeeping(tmp_path):
    exe = str(tmp_path / "group_start_check")
    r = _compile(exe)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "warning" not in r.stdout, r.stdout[-3000:]
    _run(exe)


def test_start_bookkeeping_under_sanitizers(tmp_path):
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    p = subprocess.run(["g++"] + flags + [str(probe), "-o", str(tmp_path / "probe")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtimes here")
    exe = str(tmp_path / "group_start_check_san")
    r = _compile(exe, flags)
    assert r.returncode == 0, r.stdout[-3000:]
    _run(exe)
