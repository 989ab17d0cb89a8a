"""The builder of the sensors' camera-ray tables (psdr_jit_amd/csrc/hip/cam_table.h: the screen-space coverage of the scene per triangle, which the live-pixel mask folds
into one bit per pixel) checked on the host by tests/cpp/cam_table_check.cpp: conservative and tight against point-in-triangle tests in double, tiles as unions of
pixels, bands of rows, triangles behind and across the camera plane, the cell sizes.  No GPU: compiled by g++ alone, once plainly and once with the address and
undefined-behaviour sanitizers (a stand-alone program; skipped where g++ cannot link their runtimes)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "cam_table_check.cpp")


def _compile(exe, extra=()):
    return subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + ROOT] + list(extra) + [SRC, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _run(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout[-3000:]


def test_camera_table_builder(tmp_path):
    exe = str(tmp_path / "cam_table_check")
    r = _compile(exe)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "warning" not in r.stdout, r.stdout[-3000:]
    _run(exe)


def test_camera_table_builder_under_sanitizers(tmp_path):
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    p = subprocess.run(["g++"] + flags + [str(probe), "-o", str(tmp_path / "probe")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        pytest.skip("g++ cannot link the sanitizer runtimes here")
    exe = str(tmp_path / "cam_table_check_san")
    r = _compile(exe, flags)
    assert r.returncode == 0, r.stdout[-3000:]
    _run(exe)
