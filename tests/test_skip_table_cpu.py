"""The skip-ahead table of the path kernels on the CPU (psdr_jit_amd/csrc/hip/sampler.h is plain C++ on the host): a path that ends early skips the draws of the
depth levels it leaves, nd * k of them, and LaneRng::skip_levels applies that skip from a table of precomputed maps (k <= 8) or with the doubling loop (k > 8).
For nd in {2, 3, 5}, k = 1..12 and 1000 random (state, odd inc) each, the result equals LaneRng::advance(nd * k) bit for bit."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_skip_table(tmp_path):
    exe = str(tmp_path / "skip_table_check")
    src = os.path.join(ROOT, "tests", "cpp", "skip_table_check.cpp")
    r = subprocess.run(["g++", "-O2", "-std=c++17", src, "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.split() == ["ok", str(3 * 12 * 1000)], r.stdout[-500:]
