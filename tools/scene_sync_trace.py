"""What psdr_hip_scene_create / _update / _update_edges did over a fixed list of Scene.configure() calls, as JSON - the record that a change of
csrc/hip/scene_build.hip which is meant to leave its behaviour alone is compared against (tests/golden/scene_sync_trace.json, tests/test_gpu_scene_sync_trace.py).

    python tools/scene_sync_trace.py [--out FILE]

Four small scenes at 32 x 32, 1 spp, through the public Python surface and the test aids only:
    cbox        the 36-triangle Cornell box: brute force, filter primitives, live-pixel mask
    bvh_env     tests/scenes.py::config5_scene at level 3 (1280 + 2 triangles, a tree) under an environment map, a bitmap on the floor's BSDF, PSDR_DEVICE_EDGES_MIN=0:
                lean configures, rows and primary edges from the device
    bvh_area    the same meshes under an area light: no lean configure, the live-pixel mask follows the triangles
    bvh_env_host  bvh_env once more under PSDR_HOST_GEOMETRY=1: the host writes every row
Per step: tree (built / refitted / kept), reallocated, bytes_uploaded, edge_path, edge_bytes and the three mismatch counts (device rows and edge arrays against the
host path's words, tree violations) - not the ms_* fields, and not sah_cost: the refit sums it on the device in arrival order.  Per scene one hit check: a fixed set of
rays through psdr_hip_trace, the number of hits and the sum of the triangle ids.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FIELDS = ("tree", "reallocated", "bytes_uploaded", "edge_path", "edge_bytes")


def _record(cabi, sc, name, extra=None):
    u = sc._last_update()
    row = {"step": name}
    row.update({k: (int(u[k]) if not isinstance(u[k], str) else u[k]) for k in FIELDS})
    v = C.c_int64(-1)
    cabi.check(cabi.lib().psdr_hip_scene_check_tree(C.c_void_p(sc._hip_handle()), C.byref(v)))
    row["rows_mismatch"] = int(sc._check_device_rows())
    row["edges_mismatch"] = int(sc._check_device_edges())
    row["tree_violations"] = int(v.value)
    if extra:
        row.update(extra)
    return row


def _hits(cabi, sc):
    import torch
    rng = np.random.default_rng(5)
    n = 4096
    o = rng.uniform([-100, 0, -200], [650, 500, 650], size=(n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    tri = torch.empty(n, dtype=torch.int32, device="cuda")
    uv = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    t = torch.empty(n, dtype=torch.float32, device="cuda")
    cabi.check(cabi.lib().psdr_hip_trace(sc._hip_handle(), n, to.data_ptr(), td.data_ptr(), tri.data_ptr(), uv.data_ptr(), t.data_ptr(), None))
    tri = tri.cpu().numpy().astype(np.int64)
    return {"n_hit": int((tri >= 0).sum()), "tri_sum": int(tri[tri >= 0].sum())}


def _translate(x, y=0.0, z=0.0):
    m = np.eye(4, dtype=np.float32)
    m[:3, 3] = [x, y, z]
    return m


def _bvh_spec(env):
    import scenes
    from oracle.oracle import EmitterSpec
    spec = scenes.config5_scene(32, 32, 1, 1, 1, level=3, env_res=(64, 32), param=None)
    spec.bsdfs[1].texture = scenes.ramp_texture(16, 8)
    if not env:
        spec.bsdfs.append(type(spec.bsdfs[0])((0.0, 0.0, 0.0), name="light"))
        spec.emitters = [EmitterSpec((20.0, 20.0, 8.0))]
        spec.meshes.append(scenes._mesh("cbox_luminaire.obj", 2, emitter=0, raw=scenes.translate(0.0, -100.0, 0.0)))
    return spec


def trace_scene(kind):
    """the steps of one scene -> {"steps": [...], "hits": {...}}"""
    import product
    import scenes
    from psdr_jit_amd import cabi
    bvh = kind != "cbox"
    spec = _bvh_spec(kind != "bvh_area") if bvh else scenes.cbox_scene(32, 32, 1, 1, 1, param=None)
    colour_key = "BSDF[0]" if bvh else "BSDF[4]"
    steps = []

    def step(name, extra=None):
        sc.configure([0])
        steps.append(_record(cabi, sc, name, extra))

    sc = product.build_scene(spec)
    steps.append(_record(cabi, sc, "create"))
    step("unchanged")
    mesh, cam, bs = sc.param_map["Mesh[0]"], sc.param_map["Sensor[0]"], sc.param_map[colour_key]
    zero4 = np.zeros((4, 4), np.float32)
    bs._set("reflectance", np.asarray([0.3, 0.6, 0.2], np.float32), np.zeros(3, np.float32))
    step("colour")
    v0 = np.asarray(spec.meshes[0].vertices, np.float32).copy()

    def move(k, name):
        v = v0.copy(); v[:, 1] *= k
        mesh._set("vertex_positions", v, np.zeros_like(v))
        step(name)

    move(0.99, "vertex_move")            # (a tree scene: refitted; under an environment map the configures are lean from here on)
    move(0.98, "vertex_move_2")          # (... and with PSDR_DEVICE_EDGES_MIN=0 the device selects the primary edges from this one on)
    tw = np.asarray(spec.cameras[0].to_world_raw, np.float32).copy()
    tw[0, 3] += 15.0
    cam._set("to_world", tw, zero4)
    step("camera_move")
    d = zero4.copy(); d[0, 3] = 100.0
    mesh._set("to_world_left", np.eye(4, dtype=np.float32), d)
    step("tangent_on")
    mesh._set("to_world_left", np.eye(4, dtype=np.float32), zero4)
    step("tangent_off")
    mesh._set("to_world_left", _translate(3.0, -2.0, 1.0), zero4)
    step("transform_move")
    if bvh:
        # the vertices change places: every triangle spans the mesh, the refitted tree costs many times the 1.4 x of the built one that calls for a new tree
        v2 = np.ascontiguousarray(v0[np.random.default_rng(1).permutation(len(v0))])
        mesh._set("vertex_positions", v2, np.zeros_like(v2))
        step("scramble")
        v0 = v2
        move(0.99, "vertex_move_after_build")
        move(0.98, "vertex_move_after_build_2")
        floor = sc.param_map["BSDF[1]"]
        tex = scenes.checker_texture(8, 8)
        floor._set("reflectance", np.ascontiguousarray(tex), np.zeros_like(tex))
        step("bitmap_resized")
        tex = (0.5 * tex).astype(np.float32)
        floor._set("reflectance", np.ascontiguousarray(tex), np.zeros_like(tex))
        step("bitmap_texels")
        rc, msg = sc._update_with_malformed_geometry(0, "faces")
        steps.append({"step": "malformed_update", "refused": bool(rc != 0), "names_the_list": "faces" in msg, "rows_mismatch": int(sc._check_device_rows())})
        step("after_poison")
        move(0.97, "vertex_move_after_poison")
        cam._set("to_world", np.asarray(spec.cameras[0].to_world_raw, np.float32), zero4)
        step("camera_back")
    return {"steps": steps, "hits": _hits(cabi, sc)}


def run():
    out = {}
    saved = {k: os.environ.get(k) for k in ("PSDR_DEVICE_EDGES_MIN", "PSDR_HOST_GEOMETRY")}
    try:
        os.environ.pop("PSDR_HOST_GEOMETRY", None)
        os.environ.pop("PSDR_DEVICE_EDGES_MIN", None)
        out["cbox"] = trace_scene("cbox")
        os.environ["PSDR_DEVICE_EDGES_MIN"] = "0"
        out["bvh_env"] = trace_scene("bvh_env")
        out["bvh_area"] = trace_scene("bvh_area")
        os.environ["PSDR_HOST_GEOMETRY"] = "1"
        out["bvh_env_host"] = trace_scene("bvh_env_host")
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("scene_sync_trace: needs a GPU")
    text = json.dumps(run(), indent=1, sort_keys=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
