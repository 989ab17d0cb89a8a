"""Grouped starts of the interior term's waves (paths.h GROUPED STARTS, csrc/hip/group_start.h): a wave starts new samples once its threshold of lanes is idle, and a
start fills every idle lane - across the windows of the live-pixel hand-out and across the boundary of a fetch batch.  Which lane runs which sample changes; the
samples, their seeds and their arithmetic do not.  So every case of tests/group_start_cases.py is rendered (renderC and renderD)

  with the library's thresholds and with PSDR_GROUP_START = 16 and 64 (read per call), and each frame equals the one of a fresh child process with PSDR_GROUP_START=0 -
      lane by lane, the schedule before the threshold - to 1e-6 relative L2 (the same samples; only the order of the float atomics differs)
  and the frame with the library's thresholds equals the oracle's at 1e-3 relative L2, the bound of the other parity files.

The frames: 8 x 8 at spp 1 (64 positions, fewer live items than any threshold), 16 x 16 at spp 1 (one fetch batch), at spp 5 (five), 24 x 16 at spp 3 (a partial last
batch), a camera pulled back until fewer than one pixel in eight is live (a start needs more than three windows and crosses batches); max_depth 1 and 6, hide_emitters,
two shards, a continuing sampler, a pixel list with ids outside the frame.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import group_start_cases as cases
import product

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-3
TOL_SAME_SAMPLES = 1e-6
THRESHOLDS = (None, "16", "64")         # None: the library's own


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


@pytest.fixture(scope="module")
def lane_by_lane(env, tmp_path_factory):
    """the frames of group_start_cases.CASES with PSDR_GROUP_START=0: one child process"""
    out = str(tmp_path_factory.mktemp("group_start") / "lane_by_lane.npz")
    child_env = dict(os.environ, PSDR_GROUP_START="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "group_start_cases.py"), out], cwd=ROOT, env=child_env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    return dict(np.load(out))


@pytest.fixture(scope="module")
def grouped(env):
    """{threshold: {case: (renderC, renderD)}} of this process"""
    assert "PSDR_GROUP_START" not in os.environ, "the test sets the knob itself"
    frames = {}
    try:
        for g in THRESHOLDS:
            if g is not None:
                os.environ["PSDR_GROUP_START"] = g
            frames[g] = {name: cases.render_case(name) for name in cases.CASES}
    finally:
        os.environ.pop("PSDR_GROUP_START", None)
    return frames


_oracles = {}


def _oracle(orc, frame):
    if frame not in _oracles:
        _oracles[frame] = orc.OracleScene(cases.frame_spec(frame), [0])
    return _oracles[frame]


def test_far_camera_leaves_few_live_pixels(env):
    _, _, cabi = env
    spec, sc = cases.scene_of("far")
    n = spec.width * spec.height
    bits = np.zeros((n + 31) // 32, np.uint32)
    n_live = C.c_int64(0)
    cabi.check(cabi.lib().psdr_hip_scene_live_pixels(C.c_void_p(sc._hip_handle()), 0, bits.ctypes.data, C.byref(n_live)))
    print("far: %d of %d pixels live" % (n_live.value, n))
    # fewer than 8 live positions per 64-position window, over more than one 256-position batch: 64 idle lanes need more than three windows and a fetch
    assert 0 < n_live.value < n / 8
    assert n * spec.spp > 256


@pytest.mark.parametrize("name", list(cases.CASES))
def test_same_samples_as_lane_by_lane(lane_by_lane, grouped, name):
    old_c, old_d = lane_by_lane[name + "/c"], lane_by_lane[name + "/d"]
    assert np.abs(old_c).max() > 0 and np.abs(old_d[1]).max() > 0, name
    for g in THRESHOLDS:
        got_c, got_d = grouped[g][name]
        e = (product.rel_l2(got_c, old_c), product.rel_l2(got_d[0], old_d[0]), product.rel_l2(got_d[1], old_d[1]))
        print("%s, threshold %s: renderC %.3g, renderD %.3g / %.3g" % (name, g or "default", *e))
        assert max(e) <= TOL_SAME_SAMPLES, (name, g, e)


@pytest.mark.parametrize("name", [n for n in cases.CASES if not n.startswith("shard")])
def test_frames_equal_the_oracle(orc, grouped, name):
    frame, depth, kw, listed = cases.CASES[name]
    ref = _oracle(orc, frame)
    pix = cases.pixel_list(cases.frame_spec(frame)) if listed else None
    hide, skips = bool(kw.get("hide_emitters", False)), kw.get("skips", (0, 0, 0))
    want_c = ref.render_c(max_depth=depth, hide_emitters=hide, seed=cases.SEEDS[0], skip=skips[0], pix_ids=pix)
    want_img, want_d = ref.render_d(max_depth=depth, hide_emitters=hide, seeds=cases.SEEDS, skips=skips, pix_ids=pix)
    got_c, got_d = grouped[None][name]
    e = (product.rel_l2(got_c, want_c), product.rel_l2(got_d[0], want_img), product.rel_l2(got_d[1], want_d))
    print("%s: renderC %.3g, renderD %.3g / %.3g" % (name, *e))
    assert np.abs(want_c).max() > 0 and np.abs(want_d).max() > 0
    assert max(e) < TOL, (name, e)


def test_two_shards_sum_to_the_oracles_frame(orc, grouped):
    frame, depth, _, _ = cases.CASES["shard0"]
    ref = _oracle(orc, frame)
    want_c = ref.render_c(max_depth=depth, seed=cases.SEEDS[0])
    want_img, want_d = ref.render_d(max_depth=depth, seeds=cases.SEEDS)
    (c0, d0), (c1, d1) = grouped[None]["shard0"], grouped[None]["shard1"]
    assert np.abs(c0).max() > 0 and np.abs(c1).max() > 0
    e = (product.rel_l2(c0 + c1, want_c), product.rel_l2(d0[0] + d1[0], want_img), product.rel_l2(d0[1] + d1[1], want_d))
    print("two shards: renderC %.3g, renderD %.3g / %.3g" % e)
    assert max(e) < TOL, e
