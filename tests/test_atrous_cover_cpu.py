"""The tile scheme the two a-trous denoiser units share (psdr_jit_amd/csrc/hip/atrous.h: the launch grid and the decode the kernels expand) walked on the host by
tests/cpp/atrous_cover_check.cpp - every workgroup and thread of every grid for frames 1 x 1 to 131 x 127 and strides 1 to 128: each pixel owned exactly once, no owner
outside the frame, halo words in the workgroup's coset, tap words inside the halo, tap masks exact, the grid's y extent within 65535.  No GPU: the program is compiled by
g++ alone, once plainly and once with the address and undefined-behaviour sanitizers (a stand-alone program; skipped where g++ cannot link their runtimes)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "atrous_cover_check.cpp")


def _compile(exe, extra=()):
    return subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + ROOT] + list(extra) + [SRC, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _run(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout[-3000:]


def test_every_pixel_has_one_owner_and_every_tap_its_word(tmp_path):
    exe = str(tmp_path / "atrous_cover_check")
    r = _compile(exe)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "warning" not in r.stdout, r.stdout[-3000:]
    _run(exe)


def test_every_pixel_has_one_owner_and_every_tap_its_word_under_sanitizers(tmp_path):
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    p = subprocess.run(["g++"] + flags + [str(probe), "-o", str(tmp_path / "probe")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtimes here")
    exe = str(tmp_path / "atrous_cover_check_san")
    r = _compile(exe, flags)
    assert r.returncode == 0, r.stdout[-3000:]
    _run(exe)
