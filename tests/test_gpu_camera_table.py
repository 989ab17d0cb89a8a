"""Camera rays resolved from the sensor's per-pixel triangle table (SensorDev::cam_tab, csrc/hip/cam_table.h, paths.h::run_paths) instead of the tracer.

On a brute-force scene seen through a perspective sensor a lane of the interior term's kernel looks its pixel up in a table of 64-bit candidate masks (bit = device
triangle slot), runs the tracer's exact test over the set bits and starts its path at the first vertex.  Which triangles are LOOKED AT changes; the hit - the
reference's test, smallest t, ties to the smallest id - must not.  The primary-edge kernel was measured with the same shortcut, lost, and keeps the traced route
(LABNOTES); its cases stay here - they hold whichever route the camera rays of an edge sample take.  So:

  conservative   every triangle the full tracer reports for a camera ray through a pixel is in that pixel's cell (jittered points, corners, edge midpoints), and
                 the table says something: far fewer bits per live cell than the scene has triangles
  exact          frames equal the oracle's at TOL (the bound of the other parity files: 1e-3 relative L2), and equal the same call with PSDR_NO_CAM_TABLE=1 in a
                 fresh process to 1e-6 relative L2 (the same samples; only the order of the float atomics differs)
  borders        edge samples at cell and frame borders (tests/camera_table_cases.py::border_camera)
  updates        a moved mesh and a moved camera rebuild the table; every sensor has its own
  callers        pixel lists with ids outside the frame, shards, spp = 1, a continuing sampler
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import camera_table_cases as cases
import product
import scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-3
TOL_SAME_SAMPLES = 1e-6


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
def traced(env, tmp_path_factory):
    """the frames of camera_table_cases.CASES with every camera ray through the tracer: one child process"""
    out = str(tmp_path_factory.mktemp("cam_table") / "traced.npz")
    child_env = dict(os.environ, PSDR_NO_CAM_TABLE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "camera_table_cases.py"), out], cwd=ROOT, env=child_env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    return dict(np.load(out))


_scenes = {}


def _case(name, orc):
    """(spec, product scene, oracle scene) of a case, made once"""
    if name not in _scenes:
        spec = cases.case_spec(name)
        _scenes[name] = (spec, product.build_scene(spec), orc.OracleScene(spec, [0]))
    return _scenes[name]


def _camera_rays(spec, sx, sy):
    """PerspectiveCamera::sample_primary_ray for sample-space points (sx, sy), in float64 from the camera's description"""
    cam = spec.cameras[0]
    tw = np.asarray(cam.to_world_left, np.float64) @ np.asarray(cam.to_world_raw, np.float64) @ np.asarray(cam.to_world_right, np.float64)
    tan = np.tan(np.radians(cam.fov_x / 2.0))
    d = np.stack([(1.0 - 2.0 * sx) * tan, (1.0 - 2.0 * sy) * tan * spec.height / spec.width, np.ones_like(sx)], axis=-1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d @ tw[:3, :3].T
    o = np.tile(tw[:3, 3][None, :], (d.shape[0], 1))
    return o.astype(np.float32), d.astype(np.float32)


def _hit_slots(env, sc, o, d):
    """device triangle slot of the full tracer's hit per ray, -1 = miss"""
    torch, _, cabi = env
    n = o.shape[0]
    to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    rec = torch.zeros((n, 24), dtype=torch.float32, device="cuda")
    hit = torch.empty((n,), dtype=torch.int32, device="cuda")
    cabi.check(cabi.lib().psdr_hip_ray_intersect_ad(C.c_void_p(sc._hip_handle()), n, to.data_ptr(), td.data_ptr(), None, None, rec.data_ptr(), None, hit.data_ptr(), None))
    torch.cuda.synchronize()
    return hit.cpu().numpy()


def _check_conservative(env, spec, sc, name):
    """-> (mean, max) set bits per live cell; asserts that no camera ray hits a triangle its pixel's cell does not list"""
    g, tab = cases.camera_table(sc)
    assert g >= 1, name
    W, H = spec.width, spec.height
    ys, xs = np.divmod(np.arange(W * H), W)
    below1 = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    rng = np.random.default_rng(17)
    jit = [(0.0, 0.0), (0.5, 0.0), (below1, 0.0), (0.0, 0.5), (below1, 0.5), (0.0, below1), (0.5, below1), (below1, below1)]       # corners and edge midpoints
    jit = [(np.full(W * H, a), np.full(W * H, b)) for a, b in jit] + [(rng.random(W * H), rng.random(W * H)) for _ in range(8)]
    cell = tab[ys // g, xs // g]
    n_hit = 0
    for jx, jy in jit:
        sx = ((xs.astype(np.float32) + jx.astype(np.float32)) / np.float32(W)).astype(np.float64)
        sy = ((ys.astype(np.float32) + jy.astype(np.float32)) / np.float32(H)).astype(np.float64)
        slot = _hit_slots(env, sc, *_camera_rays(spec, sx, sy))
        hit = slot >= 0
        listed = (cell[hit] >> slot[hit].astype(np.uint64)) & np.uint64(1)
        assert np.all(listed == 1), (name, int((listed == 0).sum()))
        n_hit += int(hit.sum())
    assert n_hit > 0, name
    bits = np.array([bin(int(x)).count("1") for x in tab.ravel()])
    live = bits > 0
    return float(bits[live].mean()), int(bits.max())


def test_table_is_conservative_and_not_trivial(env):
    far = scenes.cbox_scene(64, 64, 4, 0, 0, param="box_x")
    far.cameras[0].to_world_raw = np.asarray(scenes.translate(-900.0, 273.0, -2500.0), np.float32)
    for name, spec, n_tris in (("cbox", scenes.cbox_scene(96, 80, 8, 0, 0, param="box_x"), 36), ("microfacet", scenes.microfacet_cbox_scene(64, 48, 8, 0, 0, param="box_x"), 36),
                               ("far", far, 36)):
        sc = product.build_scene(spec)
        mean, most = _check_conservative(env, spec, sc, name)
        print("%s: %.2f bits per live cell, at most %d, of %d triangles" % (name, mean, most, n_tris))
        # (a table that listed half of the triangles per cell would leave the exact rounds with more work than the filter pass it replaces hands them)
        assert mean < n_tris / 2 and most < n_tris, (name, mean, most)
        # the live-pixel mask is the same coverage with the triangles folded together
        n = spec.width * spec.height
        bits = np.zeros((n + 31) // 32, np.uint32)
        n_live = C.c_int64(0)
        env[2].check(env[2].lib().psdr_hip_scene_live_pixels(C.c_void_p(sc._hip_handle()), 0, bits.ctypes.data, C.byref(n_live)))
        g, tab = cases.camera_table(sc)
        if g == 1 and n_live.value < n:
            live = ((bits[np.arange(n) >> 5] >> (np.arange(n) & 31).astype(np.uint32)) & 1).astype(bool)
            assert np.array_equal(live, tab.ravel() != 0), name
    # no table: a BVH scene (652 triangles), and a camera inside the room (walls, floor and ceiling cross the camera plane)
    inside = scenes.cbox_scene(64, 64, 4, 0, 0, param="box_x")
    inside.cameras[0].to_world_raw = np.asarray(scenes.translate(278.0, 273.0, 150.0), np.float32)
    for name, spec in (("sphere", scenes.sphere_scene(64, 64, 8, 0, 0)), ("inside", inside)):
        assert cases.camera_table(product.build_scene(spec))[0] == 0, name


@pytest.mark.parametrize("terms", cases.TERMS)
@pytest.mark.parametrize("name", ["cbox_light", "cbox_box", "microfacet"])
def test_frames_equal_the_oracle_and_the_traced_route(env, orc, traced, name, terms):
    spec, sc, ref = _case(name, orc)
    assert cases.camera_table(sc)[0] == 1
    got = cases.render_d(sc, spec.width * spec.height, terms)
    wimg, wd = ref.render_d(max_depth=cases.DEPTH, seeds=cases.SEEDS, terms=terms)
    old = traced["%s/%d" % (name, terms)]
    e_img = product.rel_l2(got[0], wimg) if terms & 1 else float(np.abs(got[0]).max())
    e_der, s_der = product.rel_l2(got[1], wd), product.rel_l2(got[1], old[1])
    s_img = product.rel_l2(got[0], old[0]) if terms & 1 else float(np.abs(old[0]).max())
    print("%s terms %d: oracle %.3g / %.3g, traced route %.3g / %.3g" % (name, terms, e_img, e_der, s_img, s_der))
    assert np.abs(wd).max() > 0
    assert e_img < TOL and e_der < TOL
    assert s_img <= TOL_SAME_SAMPLES and s_der <= TOL_SAME_SAMPLES


def test_edge_samples_at_cell_and_frame_borders(env, orc, traced):
    spec, sc, ref = _case("border", orc)
    assert cases.camera_table(sc)[0] == 1
    # the premise (camera_table_cases.border_camera): the ceiling's front edge lies inside the frame by less than EdgeEpsilon, the green wall's on a pixel boundary
    y_cam = float(spec.cameras[0].to_world_raw[1, 3])
    y_s = 0.5 - (float(np.float32(548.79999)) - y_cam) / (2.0 * 500.0 * np.tan(np.radians(30.0)))
    assert 0.0 < y_s < 1e-5, y_s
    assert float(spec.cameras[0].to_world_raw[0, 3]) == 0.0
    got = cases.render_d(sc, 64 * 64, 2)
    _, wd = ref.render_d(max_depth=cases.DEPTH, seeds=cases.SEEDS, terms=2)
    old = traced["border/2"]
    top = np.abs(wd.reshape(64, 64, 3)[0]).sum()
    print("border: oracle %.3g, traced route %.3g, top row |d| %.3g of %.3g" % (product.rel_l2(got[1], wd), product.rel_l2(got[1], old[1]), top, np.abs(wd).sum()))
    assert top > 0                         # the samples on the edge along the top border count ...
    assert np.abs(got[0]).max() == 0.0
    assert product.rel_l2(got[1], wd) < TOL and product.rel_l2(got[1], old[1]) <= TOL_SAME_SAMPLES
    assert product.rel_l2(got[1].reshape(64, 64, 3)[0], wd.reshape(64, 64, 3)[0]) < TOL       # ... as the oracle counts them
    for terms in (1, 7):
        got = cases.render_d(sc, 64 * 64, terms)
        wimg, wd = ref.render_d(max_depth=cases.DEPTH, seeds=cases.SEEDS, terms=terms)
        assert product.rel_l2(got[0], wimg) < TOL and product.rel_l2(got[1], wd) < TOL, terms


def test_updates_rebuild_the_table(env, orc):
    torch, psdr, cabi = env
    spec = scenes.cbox_scene(64, 48, 8, 8, 8, param="box_x")
    for m in spec.meshes:
        m.path = None                       # (the oracle and the product read the arrays, which the test moves)
    sc = product.build_scene(spec)
    g, tab0 = cases.camera_table(sc)
    assert g == 1

    def check(tag):
        _check_conservative(env, spec, sc, tag)
        got = cases.render_d(sc, 64 * 48, 7)
        wimg, wd = orc.OracleScene(spec, [0]).render_d(max_depth=cases.DEPTH, seeds=cases.SEEDS, terms=7)
        assert product.rel_l2(got[0], wimg) < TOL and product.rel_l2(got[1], wd) < TOL, tag
    # the small box moves 60 units to the right: its cells change
    v = np.asarray(spec.meshes[1].vertices, np.float32).copy()
    v[:, 0] += 60.0
    sc.param_map["Mesh[1]"]._set("vertex_positions", v, np.zeros_like(v))
    sc.configure([0])
    spec.meshes[1].vertices = v
    _, tab1 = cases.camera_table(sc)
    assert tab1.shape == tab0.shape and not np.array_equal(tab1, tab0)
    check("moved mesh")
    # the camera moves: every cell may change
    tw = np.asarray(spec.cameras[0].to_world_raw, np.float32).copy()
    tw[0, 3] += 120.0; tw[1, 3] -= 40.0
    sc.param_map["Sensor[0]"]._set("to_world", tw, np.zeros((4, 4), np.float32))
    sc.configure([0])
    spec.cameras[0].to_world_raw = tw
    _, tab2 = cases.camera_table(sc)
    assert not np.array_equal(tab2, tab1)
    check("moved camera")


def test_every_sensor_has_its_own_table(env, orc):
    spec = scenes.with_extra_sensors(scenes.cbox_scene(40, 40, 8, 8, 8, param="box_x"), "perspective")
    sc = product.build_scene(spec, active=(0, 1, 2))
    ref = orc.OracleScene(spec, [0, 1, 2])
    tabs = [cases.camera_table(sc, k) for k in range(3)]
    assert all(g == 1 for g, _ in tabs)
    assert not np.array_equal(tabs[0][1], tabs[1][1]) and not np.array_equal(tabs[1][1], tabs[2][1])
    for k in range(3):
        got = cases.render_d(sc, 40 * 40, 7, sensor_id=k)
        wimg, wd = ref.render_d(sensor=k, max_depth=cases.DEPTH, seeds=cases.SEEDS, terms=7)
        assert product.rel_l2(got[0], wimg) < TOL and product.rel_l2(got[1], wd) < TOL, k


def test_unchanged_callers(env, orc):
    torch, psdr, cabi = env
    spec, sc, ref = _case("cbox_box", orc)
    W, H = spec.width, spec.height
    # a pixel list with ids outside the frame (rows below it and ids far beyond): those lanes keep the traced route, in one wave with the others
    rng = np.random.default_rng(3)
    pix = np.concatenate([rng.integers(0, W * H, 300), np.arange(W * H, W * H + 40), [W * H * 3 + 5, W * (H + 7) + 2]]).astype(np.int32)
    rng.shuffle(pix)
    pix_t = torch.from_numpy(pix).cuda()
    got = cases.render_d(sc, len(pix), 1, pix_ids_ptr=pix_t.data_ptr(), n_pix=len(pix))
    wimg, wd = ref.render_d(max_depth=cases.DEPTH, seeds=cases.SEEDS, pix_ids=pix)
    assert np.abs(wimg).max() > 0 and product.rel_l2(got[0], wimg) < TOL and product.rel_l2(got[1], wd) < TOL
    # two shards sum to the frame
    whole = cases.render_d(sc, W * H, 7)
    parts = [cases.render_d(sc, W * H, 7, shard_rank=r, shard_count=2) for r in range(2)]
    assert product.rel_l2(parts[0] + parts[1], whole) <= 2e-6
    assert np.abs(parts[0]).max() > 0 and np.abs(parts[1]).max() > 0
    # a continuing sampler: the draws earlier calls consumed are skipped
    got = cases.render_d(sc, W * H, 7, skips=(1000, 500, 250))
    wimg, wd = ref.render_d(max_depth=cases.DEPTH, seeds=cases.SEEDS, skips=(1000, 500, 250))
    assert product.rel_l2(got[0], wimg) < TOL and product.rel_l2(got[1], wd) < TOL
    # spp = sppe = sppse = 1
    one = scenes.cbox_scene(96, 80, 1, 1, 1, param="box_x")
    got = cases.render_d(product.build_scene(one), W * H, 7)
    wimg, wd = orc.OracleScene(one, [0]).render_d(max_depth=cases.DEPTH, seeds=cases.SEEDS)
    assert product.rel_l2(got[0], wimg) < TOL and product.rel_l2(got[1], wd) < TOL
