"""The lean instantiations of the forward path kernels (psdr_jit_amd/csrc/hip/paths.h::Switches) against the general ones.

A forward-mode PathTracer call through a perspective sensor without the per-lane output runs k_paths<..., kLean>, in which those switches are compile-time
constants; PSDR_NO_LEAN=1 (read per call, like PSDR_NO_FORK) sends the same call to the general kernels.  Both trace the same samples with the same arithmetic, so
the two results differ by the order of the float atomics only - the bounds are the ones tests/test_gpu_configs.py uses for that kind of difference (forked against
serial launches): relative L2 below 2e-6 on the image and 2e-5 on the derivative.

  class 1 (scene in LDS, the kernels bench.py times)  the Cornell box, 32 x 32, 4 / 4 / 4 samples, depth 3: the three terms together and each alone, with and
                                                      without skip_static_edges
  class 2 (BVH, the decoupled form)                   config 5's scene at mesh level 1 - 82 triangles, the smallest level above kBruteForceMax = 64 -, 48 x 48
  orthographic sensor                                 the call the lean kernels must NOT take, and the only one whose second edge path does not start at one point
                                                      for the whole launch: the primary-edge term alone against the oracle, relative L2 < 1e-3 as in
                                                      test_gpu_configs.py::test_config3_depth3_small_per_term
"""
import ctypes as C

import numpy as np
import pytest

import product
import scenes

pytestmark = pytest.mark.gpu
TOL_IMAGE, TOL_DERIVATIVE = 2e-6, 2e-5
TOL_ORACLE = 1e-3


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    from psdr_jit_amd import cabi
    return torch, psdr_jit_amd, cabi


def _render_d(env, sc, n_pix, depth, seeds, terms=7, skip_static_edges=False):
    torch, _, cabi = env
    buf = torch.empty((2, n_pix, 3), dtype=torch.float32, device="cuda")
    a = cabi.make_args(max_depth=depth, seeds=seeds, terms=terms, skip_static_edges=skip_static_edges)
    cabi.check(cabi.lib().psdr_hip_render_d_fwd(sc._hip_handle(), C.byref(a), buf[0].data_ptr(), buf[1].data_ptr(), None))
    torch.cuda.synchronize()
    return buf.cpu().numpy()


@pytest.fixture(scope="module")
def cbox(env):
    return product.build_scene(scenes.cbox_scene(32, 32, 4, 4, 4, param="light_x"))


@pytest.fixture(scope="module")
def blob(env):
    spec = scenes.config5_scene(48, 48, 4, 4, 4, level=1, env_res=(64, 32), param="blob_x")
    assert sum(len(m.faces) for m in spec.meshes) > 64          # kBruteForceMax (scene_dev.h): a BVH scene, the decoupled path kernels
    return product.build_scene(spec)


def _lean_against_general(env, monkeypatch, sc, n_pix, terms, skip, seeds):
    lean = _render_d(env, sc, n_pix, 3, seeds, terms=terms, skip_static_edges=skip)
    monkeypatch.setenv("PSDR_NO_LEAN", "1")
    general = _render_d(env, sc, n_pix, 3, seeds, terms=terms, skip_static_edges=skip)
    monkeypatch.delenv("PSDR_NO_LEAN")
    e_img = product.rel_l2(lean[0], general[0]) if terms & 1 else float(np.abs(lean[0]).max() + np.abs(general[0]).max())
    e_der = product.rel_l2(lean[1], general[1])
    print("terms %d skip_static %d: image %.3g derivative %.3g (max |d| %.3g)" % (terms, skip, e_img, e_der, np.abs(general[1]).max()))
    assert np.abs(general[1]).max() > 0 and np.abs(lean[1]).max() > 0
    if terms & 1:
        assert np.abs(general[0]).max() > 0 and e_img < TOL_IMAGE
    else:
        assert e_img == 0.0                                      # the edge terms have no primal
    assert e_der < TOL_DERIVATIVE


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("terms", [7, 1, 2, 4])
def test_lean_kernels_class1(env, monkeypatch, cbox, terms, skip):
    _lean_against_general(env, monkeypatch, cbox, 32 * 32, terms, bool(skip), (51, 52, 53))


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("terms", [7, 1, 2, 4])
def test_lean_kernels_class2(env, monkeypatch, blob, terms, skip):
    _lean_against_general(env, monkeypatch, blob, 48 * 48, terms, bool(skip), (61, 62, 63))


def test_primary_edges_orthographic_sensor(env, orc):
    """the general kernel's second edge path through an OrthographicCamera: its origin is the sample's near-plane point, rebuilt from the parked edge sample"""
    spec = scenes.ortho_cbox_scene(32, 32, 4, 4, 4, param="box_x")
    sc = product.build_scene(spec)
    got = _render_d(env, sc, 32 * 32, 3, (71, 72, 73), terms=orc.TERM_PRIMARY)
    _, wd = orc.OracleScene(spec, [0]).render_d(max_depth=3, seeds=(71, 72, 73), terms=orc.TERM_PRIMARY)
    err = product.rel_l2(got[1], wd)
    print("orthographic primary edges: derivative %.3g (max |d| %.3g)" % (err, np.abs(wd).max()))
    assert np.abs(wd).max() > 0 and np.abs(got[0]).max() == 0.0
    assert err < TOL_ORACLE
