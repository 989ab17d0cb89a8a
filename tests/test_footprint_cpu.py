"""The footprints that reverse mode scatters a bitmap lookup's adjoint into (env::bitmap_footprint, env::bitmap_footprint_env in psdr_jit_amd/csrc/common/envmath.h) as the
transposes of the lookups that the forward kernels evaluate (bitmap_eval_tex, bitmap_eval_fn), tests/cpp/footprint_check.cpp: one-hot maps of 2 x 2, 2 x 5, 5 x 2, 3 x 7 and
16 x 8 texels (the host admits none below 2 x 2), u and v from a grid with 0, 1, 1 - 2^-24, negative values and values above 1, with and without a uv transform, flip_v
both ways.  No GPU: the program is compiled by g++ alone, once plainly and once with the address and undefined-behaviour sanitizers (a stand-alone program; skipped
where g++ cannot link their runtimes)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "footprint_check.cpp")


def _compile(exe, extra=()):
    return subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + ROOT] + list(extra) + [SRC, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _run(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout[-3000:]


def test_footprints_are_the_transposes_of_the_lookups(tmp_path):
    exe = str(tmp_path / "footprint_check")
    r = _compile(exe)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "warning" not in r.stdout, r.stdout[-3000:]
    _run(exe)


def test_footprints_are_the_transposes_of_the_lookups_under_sanitizers(tmp_path):
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    p = subprocess.run(["g++"] + flags + [str(probe), "-o", str(tmp_path / "probe")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtimes here")
    exe = str(tmp_path / "footprint_check_san")
    r = _compile(exe, flags)
    assert r.returncode == 0, r.stdout[-3000:]
    _run(exe)
