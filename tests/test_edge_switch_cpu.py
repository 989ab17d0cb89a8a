"""The side switch of a primary-edge sample (psdr_jit_amd/csrc/hip/edge_switch.h: does the lane's current path end at the hit in hand, and is that hit's vertex still
read) checked on the host by tests/cpp/edge_switch_check.cpp, which plays one lane's loop of paths.h::run_paths (MODE 1) in both schedules - the late switch of the
counted kernels and the early switch ahead of the loop's one make_its - with a stub for the shading: the same sampler draws, skip_levels arguments, first-vertex
builds and radiance per path, one first-vertex build per path, the one-iteration detour exactly where the last vertex is read, every lane ends - for max_depth 0 to 4
and every way each of the two paths can end.  No GPU: compiled by g++ alone, once plainly and once with the address and undefined-behaviour sanitizers (a stand-alone
program; skipped where g++ cannot link their runtimes)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "edge_switch_check.cpp")


def _compile(exe, extra=()):
    return subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + ROOT] + list(extra) + [SRC, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _run(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout[-3000:]


def test_both_schedules_play_the_same_sample(tmp_path):
    exe = str(tmp_path / "edge_switch_check")
    r = _compile(exe)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "warning" not in r.stdout, r.stdout[-3000:]
    _run(exe)


def test_both_schedules_under_sanitizers(tmp_path):
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    p = subprocess.run(["g++"] + flags + [str(probe), "-o", str(tmp_path / "probe")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtimes here")
    exe = str(tmp_path / "edge_switch_check_san")
    r = _compile(exe, flags)
    assert r.returncode == 0, r.stdout[-3000:]
    _run(exe)
