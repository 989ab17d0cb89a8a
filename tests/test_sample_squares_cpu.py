"""The sample-squares entry points (psdr_hip_render_c_sq / psdr_hip_render_d_fwd_sq, psdr.render_c_sq / render_d_fwd_sq, variance_from_sq, samples_behind): what can be
checked without a GPU - the two symbols are declared, exported and listed under the unchanged ABI 16 and an unchanged psdr_render_args; NULL arguments are refused before
any device call; the variance helper against numpy in float64; the three sample counts; the rejected argument.  The kernels: tests/test_gpu_sample_squares.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("psdr_hip_render_c_sq", "psdr_hip_render_d_fwd_sq")


@pytest.fixture(scope="module")
def psdr():
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    return psdr_jit_amd


def test_entry_points_declared_exported_listed(psdr):
    from psdr_jit_amd import cabi
    hdr = open(os.path.join(ROOT, "include", "psdr_hip.h")).read()
    declared = set(re.findall(r"\b(psdr_hip_[a-z0-9_]+)\s*\(", hdr))
    L = cabi.lib()
    for name in ENTRIES:
        assert name in declared, "include/psdr_hip.h does not declare %s" % name
        assert hasattr(L, name), "libpsdr_hip.so does not export %s" % name
        assert name in cabi.SYMBOLS
    # added under the ABI version the callers already check; no struct grew
    assert L.psdr_hip_abi_version() == 16 and "#define PSDR_HIP_ABI_VERSION 16" in hdr
    assert [f[0] for f in cabi.RenderArgs._fields_][-2:] == ["skip_static_edges", "shard_mode"]
    assert len(cabi.RenderArgs._fields_) == 18 and C.sizeof(cabi.RenderArgs) == 128
    body = hdr[hdr.index("typedef struct psdr_render_args"):]
    body = body[:body.index("} psdr_render_args;")]
    assert re.findall(r"int32_t\s+(\w+);", body)[-2:] == ["skip_static_edges", "shard_mode"]


def test_null_arguments_are_refused(psdr):
    """scene, args and every output pointer: refused with a message, before any device call (this test runs where there is no device)"""
    from psdr_jit_amd import cabi
    L = cabi.lib()
    a = cabi.make_args()
    buf = (C.c_float * 12)()
    p = C.addressof(buf)
    fake_scene = C.c_void_p(p)          # never dereferenced: a NULL beside it is refused first
    assert L.psdr_hip_render_c_sq(None, C.byref(a), p, p, None) != 0
    assert b"null" in L.psdr_hip_last_error()
    assert L.psdr_hip_render_c_sq(fake_scene, None, p, p, None) != 0
    assert L.psdr_hip_render_c_sq(fake_scene, C.byref(a), None, p, None) != 0
    assert L.psdr_hip_render_c_sq(fake_scene, C.byref(a), p, None, None) != 0
    assert L.psdr_hip_render_d_fwd_sq(None, C.byref(a), p, p, p, p, None) != 0
    assert L.psdr_hip_render_d_fwd_sq(fake_scene, None, p, p, p, p, None) != 0
    for k in range(4):
        outs = [p, p, p, p]
        outs[k] = None
        assert L.psdr_hip_render_d_fwd_sq(fake_scene, C.byref(a), *outs, None) != 0, k
        assert b"null" in L.psdr_hip_last_error()
    assert all(v == 0.0 for v in buf)


def test_variance_from_sq_against_numpy(psdr):
    import torch
    rng = np.random.default_rng(7)
    for n in (2, 4, 16, 1024 * 16):
        x = rng.normal(0.3, 1.0, size=(n, 50, 3)) * rng.uniform(0.1, 10.0, size=(1, 50, 3))          # n contributions per pixel and channel
        mean, sq = x.sum(axis=0), (x * x).sum(axis=0)
        want = x.var(axis=0, ddof=1) * n                                                              # the variance of a SUM of n independent contributions
        got = psdr.variance_from_sq(mean, sq, n)
        assert got.dtype == np.float64
        assert np.abs(got - want).max() <= 1e-12 * np.abs(sq).max()
        plain = (sq - mean * mean / n) * (n / (n - 1))
        assert np.abs(got - plain).max() <= 1e-12 * np.abs(plain).max()
        got_t = psdr.variance_from_sq(torch.from_numpy(mean), torch.from_numpy(sq), n)
        assert got_t.dtype == torch.float64 and np.abs(got_t.numpy() - plain).max() <= 1e-12 * np.abs(plain).max()
    for bad in (1, 0, -3):
        with pytest.raises(ValueError):
            psdr.variance_from_sq(np.ones(3), np.ones(3), bad)


def test_samples_behind(psdr):
    sc = psdr.Scene()
    sc.opts.width, sc.opts.height = 48, 32
    sc.opts.spp, sc.opts.sppe, sc.opts.sppse = 4, 8, 16
    assert psdr.samples_behind(sc, psdr.TERM_INTERIOR) == 4
    assert psdr.samples_behind(sc, psdr.TERM_PRIMARY) == 48 * 32 * 8
    assert psdr.samples_behind(sc, psdr.TERM_SECONDARY) == 48 * 32 * 16
    with pytest.raises(ValueError):
        psdr.samples_behind(sc, psdr.TERM_ALL)


def test_batch_edges_is_rejected(psdr):
    sc = psdr.Scene()
    with pytest.raises(ValueError):
        psdr.render_d_fwd_sq(psdr.PathTracer(1), sc, 0, seed=1, batch_pix=[1, 2], batch_edges=True)
