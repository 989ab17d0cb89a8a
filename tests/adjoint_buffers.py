"""The psdr_grads buffers (include/psdr_hip.h) of one built scene, for the tests that call psdr_hip_render_d_bwd through the C ABI: every shape is stated here once,
from the spec and the configured snapshot.  Deliberately NOT derived from psdr_jit_amd.reverse - the package and the tests stay two independent statements of the
header (tests/test_reverse_plan_cpu.py compares them) - an undersized buffer is an out-of-bounds write on the GPU, not a wrong number."""
import ctypes as C

import numpy as np

ROWS = ("g_triangles", "g_bsdf", "g_emitter", "g_sec_edges", "g_prim_edges")       # always given; the first five members of cabi.Grads
OPTIONAL = ("g_tex", "g_camera", "g_env", "g_env_scale", "g_mat", "g_env_from_world", "g_uv_xf")


def n_bsdf_rows(spec):
    """the scene's own BSDFs, then one row per BSDF nested in a normal map (type 5)"""
    return len(spec.bsdfs) + sum(1 for b in spec.bsdfs if getattr(b, "type", 0) == 5)


def env_map(spec):
    maps = [e for e in spec.emitters if getattr(e, "type", 0) == 1]
    return maps[0] if maps else None


def shapes(sc, spec, tex_total=0, sensor_id=0):
    """{field: shape} of every float buffer; g_env only for a scene with an environment map"""
    snap = sc._snapshot()
    n_tris, n_sec = np.asarray(snap["d_triangles"]).shape[0], np.asarray(snap["d_sec_edges"]).shape[0]
    n_prim = np.asarray(sc.param_map["Sensor[%d]" % sensor_id]._primary_edges(True)).shape[0]
    n_b = n_bsdf_rows(spec)
    out = {"g_triangles": (n_tris, 22), "g_bsdf": (max(1, n_b), 3), "g_emitter": (max(1, len(spec.emitters)), 3), "g_sec_edges": (max(1, n_sec), 6),
           "g_prim_edges": (max(1, n_prim), 4), "g_tex": (max(1, int(tex_total)),), "g_camera": (16,), "g_env_scale": (1,), "g_mat": (max(1, n_b), 16),
           "g_env_from_world": (16,), "g_uv_xf": (3 * n_b + 1, 4)}
    if env_map(spec) is not None:
        H, W = env_map(spec).env_data.shape[:2]
        out["g_env"] = (H * W * 3,)
    return out


def tex_layout(sc, spec):
    """(offsets[3 * BSDF rows], total) as psdr_hip_scene_tex_layout reports them (needs the device scene)"""
    from psdr_jit_amd import cabi
    offs = (C.c_int64 * (3 * max(1, n_bsdf_rows(spec))))()
    total = C.c_int64(0)
    cabi.check(cabi.lib().psdr_hip_scene_tex_layout(C.c_void_p(sc._hip_handle()), offs, C.byref(total)))
    return offs, total.value


def allocate(sc, spec, want=(), device="cuda"):
    """zeroed row buffers plus the optional fields in `want` -> (cabi.Grads, {field: tensor}, texel offsets or None).  As the tests have always done it: g_tex is
    allocated when asked for but handed to the kernels only if the scene has texels, and the environment map's buffers exist only in a scene with such a map."""
    import torch
    from psdr_jit_amd import cabi
    assert set(want) <= set(OPTIONAL), want
    offs, total = tex_layout(sc, spec) if "g_tex" in want else (None, 0)
    shp = shapes(sc, spec, total)
    bufs = {f: torch.zeros(shp[f], dtype=torch.float32, device=device) for f in ROWS + tuple(w for w in OPTIONAL if w in want and w in shp)}
    if env_map(spec) is None:
        for f in ("g_env_scale", "g_env_from_world"):
            bufs.pop(f, None)
    g = cabi.Grads(*[bufs[f].data_ptr() for f in ROWS])
    for f in bufs:
        if f not in ROWS and (f != "g_tex" or total > 0):
            setattr(g, f, bufs[f].data_ptr())
    return g, bufs, offs


def to_f64(bufs):
    return {f: t.cpu().numpy().astype(np.float64) for f, t in bufs.items()}
