"""Edge terms of batch-pixel renderD (batch_edges): what can be checked without a GPU - the two entry points are declared in the
header, exported by the library and listed in the ctypes view; the keyword reaches every layer of the Python interface; the ABI
version did not move (the entry points were added under version 16, no struct changed)."""
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("psdr_hip_render_d_fwd_batch", "psdr_hip_render_d_bwd_batch")


@pytest.fixture(scope="module")
def psdr():
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    return psdr_jit_amd


def _header():
    with open(os.path.join(ROOT, "include", "psdr_hip.h")) as fh:
        return fh.read()


def test_batch_entry_points_declared_exported_listed(psdr):
    from psdr_jit_amd import cabi
    text = _header()
    L = cabi.lib()
    for name in NEW:
        assert re.search(r"^int\s+%s\s*\(" % name, text, re.M), "%s is not declared in include/psdr_hip.h" % name
        assert hasattr(L, name), "libpsdr_hip.so does not export %s" % name
        assert name in cabi.SYMBOLS
    # same parameters as the entry points they extend
    assert L.psdr_hip_render_d_fwd_batch.argtypes == L.psdr_hip_render_d_fwd.argtypes
    assert L.psdr_hip_render_d_bwd_batch.argtypes == L.psdr_hip_render_d_bwd.argtypes


def test_abi_version_stays_16(psdr):
    from psdr_jit_amd import cabi
    assert re.search(r"#define\s+PSDR_HIP_ABI_VERSION\s+16\b", _header())
    assert cabi.lib().psdr_hip_abi_version() == 16
    # the layout of the argument struct the new entry points share with the old ones is the ABI-16 one
    assert [f[0] for f in cabi.RenderArgs._fields_][-2:] == ["skip_static_edges", "shard_mode"]
    for name in NEW:
        assert hasattr(cabi.lib(), name)


def test_batch_edges_keyword_in_the_python_interface(psdr):
    for fn in (psdr.render_d_fwd, psdr.PathTracer.renderD, psdr.Direct.renderD, psdr.FieldExtractionIntegrator.renderD):
        p = inspect.signature(fn).parameters
        assert "batch_edges" in p and p["batch_edges"].default is False and "batch_pix" in p, fn


def test_batch_edges_without_a_pixel_list_is_refused_before_any_launch(psdr):
    """(the check sits in front of the device: it needs no GPU and no configured scene)"""
    with pytest.raises(ValueError, match="batch_pix"):
        psdr.render_d_fwd(psdr.PathTracer(1), psdr.Scene(), 0, seed=1, batch_edges=True)
    with pytest.raises(ValueError, match="batch_pix"):
        psdr.PathTracer(1).renderD(psdr.Scene(), 0, seed=1, batch_edges=True)
