"""The routing of renderD's reverse mode, recorded on the CPU:  python tests/golden/make_reverse_routing.py  writes tests/golden/reverse_routing.json.

_RenderDFn.backward runs end to end without a GPU once four names are replaced: _core._render_d_bwd (here: fills every buffer it is handed with a ramp of its own
and records every argument that is not a pointer value), _core._tex_layout (a fixed layout), _stream_ptr (0) and chain.native_geometry_grads (records what it is
asked for, returns ramps).  What comes out - the recorded launch and the gradient of every leaf - says which slice of which buffer each leaf reads.  Every value
is a float32 slice of an integer ramp, a sum of three of them or a recorded argument, so two versions of the package agree exactly or route differently.

The JSON file is the record of the commit BEFORE the routing moved into psdr_jit_amd/reverse.py (this script uses only names both sides have);
tests/test_reverse_plan_cpu.py replays the same cases on the code under test and requires equality."""
import contextlib
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import adjoint_buffers  # noqa: E402
import product  # noqa: E402
import scenes  # noqa: E402

GOLDEN = os.path.join(HERE, "reverse_routing.json")
TEX_BLOCK = 64                                    # floats per bitmap slot of the stub texel layout
FIELDS = adjoint_buffers.ROWS + adjoint_buffers.OPTIONAL
# positions in _core._render_d_bwd's argument list (bindings.cpp)
ARG = {"g_triangles": 6, "g_bsdf": 7, "g_emitter": 8, "g_sec_edges": 9, "g_prim_edges": 10, "g_tex": 18, "g_camera": 19, "g_env": 20, "g_env_scale": 21,
       "g_mat": 22, "g_env_from_world": 23, "g_uv_xf": 26}


def _view(ptr, n, ctype=C.c_float):
    return np.ctypeslib.as_array((ctype * n).from_address(ptr))


@contextlib.contextmanager
def _patched(*triples):
    old = [(o, n, getattr(o, n)) for o, n, _ in triples]
    for o, n, v in triples:
        setattr(o, n, v)
    try:
        yield
    finally:
        for o, n, v in old:
            setattr(o, n, v)


def replay(sc, spec, leaves, integ=None, terms=7, sensor_id=0, batch_pix=-1, batch_edges=False, tex_negative=()):
    """one backward() through the stubs -> {"launch": ..., "geometry": ..., "grads": ...} (JSON-ready)"""
    import psdr_jit_amd as psdr
    from psdr_jit_amd import chain
    integ = integ if integ is not None else psdr.PathTracer(2)
    pm = sc.param_map
    n_rows = adjoint_buffers.n_bsdf_rows(spec)
    tex_offs = [-1 if i in tex_negative else TEX_BLOCK * i for i in range(3 * max(1, n_rows))]
    shapes = adjoint_buffers.shapes(sc, spec, TEX_BLOCK * len(tex_offs), sensor_id)
    size = {f: int(np.prod(shapes[f])) for f in shapes}
    n_prim = np.asarray(pm["Sensor[%d]" % sensor_id]._primary_edges(True)).shape[0]
    rec = {"launches": [], "geometry": [], "tex_layout_calls": 0}

    def tex_layout(scene):
        rec["tex_layout_calls"] += 1
        return tex_offs, TEX_BLOCK * len(tex_offs)

    def bwd(*a):
        assert len(a) == 29, len(a)
        for k in range(6, 10):                    # the five row buffers are one allocation, each as long as the header says
            assert a[k + 1] - a[k] == 4 * size[FIELDS[k - 6]], (FIELDS[k - 6], a[k + 1] - a[k], size[FIELDS[k - 6]])
        for i, f in enumerate(FIELDS):
            if a[ARG[f]]:
                assert size[f] < (1 << 18), (f, size[f])
                _view(a[ARG[f]], size[f])[:] = np.float32((i + 1) << 18) + np.arange(size[f], dtype=np.float32)
        rec["launches"].append({
            "sensor_id": a[2], "seeds": list(a[3]), "skips": list(a[4]), "stream": a[11], "rank": a[12], "world": a[13], "terms": a[14],
            "mesh_filter": _view(a[15], max(1, sc.num_meshes), C.c_uint8).tolist(), "skip_bsdf": bool(a[16]), "skip_emitter": bool(a[17]),
            "null": sorted(f for f in FIELDS if not a[ARG[f]]), "pix": _view(a[24], a[25], C.c_int32).tolist() if a[24] else None, "n_pix": a[25],
            "prim_edge_filter": _view(a[27], n_prim, C.c_uint8).tolist() if a[27] else None, "batch_edges": bool(a[28])})

    def geometry(scene, sid, wanted, g_tri, g_sec, g_prim, g_camera=None):
        where = {id(pm[k]): k for k in pm if k.startswith("Mesh[") or k.startswith("Sensor[")}
        arr = lambda x: None if x is None else {"shape": list(np.shape(x)), "dtype": str(np.asarray(x).dtype), "sum": float(np.asarray(x, np.float64).sum())}
        rec["geometry"].append({"sensor_id": sid, "wanted": [[where[id(o)], name] for o, name in wanted], "g_tri": arr(g_tri), "g_sec": arr(g_sec), "g_prim": arr(g_prim),
                                "g_camera": arr(g_camera)})
        out = {}
        for k, (o, name) in enumerate(wanted):
            shape = (o.num_vertices, 3) if name == "vertex_positions" else (4, 4)
            if where[id(o)].startswith("Mesh[") or where[id(o)] == "Sensor[%d]" % sid:          # (as the host core: no entry for a sensor that is not the one in use)
                out[(id(o), name)] = 1000.0 * (k + 1) + np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape)
        return out

    n = len(batch_pix) if not isinstance(batch_pix, int) else spec.width * spec.height
    img = ((torch.arange(3 * n) % 7) + 1).to(torch.float32).reshape(n, 3)                      # small integers: every sum below is exact in float32
    w = ((torch.arange(3 * n) % 5) + 1).to(torch.float32).reshape(n, 3)
    state = {"integrator": integ, "scene": sc, "sensor_id": sensor_id, "batch_pix": batch_pix, "terms": terms, "batch_edges": batch_edges, "active": [0],
             "leaves": leaves, "seed": 5, "samplers": [(0, 0, 0, 0)] * 3, "img": img}
    with _patched((psdr._core, "_render_d_bwd", bwd), (psdr._core, "_tex_layout", tex_layout),
                  (psdr, "_stream_ptr", lambda: 0), (chain, "native_geometry_grads", geometry)):
        out = psdr._RenderDFn.apply(state, *[t for _, _, t in leaves])
        wanted = [t for _, _, t in leaves if t.requires_grad]
        got = iter(torch.autograd.grad(out, wanted, grad_outputs=w, allow_unused=True))
    rec["grads"] = []
    for _o, name, t in leaves:
        g = next(got) if t.requires_grad else None
        rec["grads"].append([name, None if g is None else {"shape": list(g.shape), "values": g.detach().reshape(-1).to(torch.float64).tolist()}])
    return rec


def leaf(*shape, needs=True, value=0.5):
    return torch.full(shape, value, dtype=torch.float32).requires_grad_(needs)


def _scene(spec, active=(0,)):
    sc = product.build_scene(spec, host_only=True, active=active)
    return sc, sc.param_map


def _cbox(**kw):
    return scenes.cbox_scene(8, 8, 1, 1, 1, param=None, **kw)


def case_colours_and_radiance():
    """a colour as a 3-vector and as one number, a leaf whose gradient is not needed, an area light's radiance: no leaf moves an edge (interior term only)"""
    spec = _cbox()
    sc, pm = _scene(spec)
    return replay(sc, spec, [(pm["BSDF[1]"], "reflectance", leaf(1)), (pm["BSDF[2]"], "reflectance", leaf(3, needs=False)), (pm["BSDF[4]"], "reflectance", leaf(3)),
                             (pm["Emitter[0]"], "radiance", leaf(3))])


def case_radiance_as_one_number():
    spec = _cbox()
    sc, pm = _scene(spec)
    return replay(sc, spec, [(pm["Emitter[0]"], "radiance", leaf(1))])


def _mesh_leaves(pm, key, needs=True):
    m = pm[key]
    return [(m, "to_world", leaf(4, 4, needs=needs)), (m, "to_world_left", leaf(4, 4, needs=needs)), (m, "to_world_right", leaf(4, 4, needs=needs)),
            (m, "vertex_positions", leaf(m.num_vertices, 3, needs=needs))]


def _camera_leaves(pm, key="Sensor[0]"):
    return [(pm[key], n, leaf(4, 4)) for n in ("to_world", "to_world_left", "to_world_right")]


def case_mesh_geometry():
    """a mesh's four geometry leaves, all terms: the primary-edge rows of the other meshes are filtered out"""
    spec = _cbox()
    sc, pm = _scene(spec)
    return replay(sc, spec, _mesh_leaves(pm, "Mesh[1]"))


def case_mesh_geometry_interior_only():
    spec = _cbox()
    sc, pm = _scene(spec)
    return replay(sc, spec, _mesh_leaves(pm, "Mesh[1]"), terms=1)


def case_camera_alone():
    spec = _cbox()
    sc, pm = _scene(spec)
    return replay(sc, spec, _camera_leaves(pm))


def case_one_mesh_of_two():
    spec = _cbox()
    sc, pm = _scene(spec)
    return replay(sc, spec, _mesh_leaves(pm, "Mesh[1]")[:2] + _mesh_leaves(pm, "Mesh[2]", needs=False)[:2] + [(pm["BSDF[3]"], "reflectance", leaf(3))])


def case_one_mesh_of_two_with_camera():
    spec = _cbox()
    sc, pm = _scene(spec)
    return replay(sc, spec, _mesh_leaves(pm, "Mesh[1]")[:2] + _mesh_leaves(pm, "Mesh[2]", needs=False)[:2] + _camera_leaves(pm)[1:2])


def case_intensity():
    """the integrator's own m_intensity beside a colour and a mesh: it keeps the boundary terms and switches the primary-edge filter off"""
    import psdr_jit_amd as psdr
    spec = _cbox()
    sc, pm = _scene(spec)
    integ = psdr.PathTracer(1)
    return replay(sc, spec, [(integ, "m_intensity", leaf(value=2.0)), (pm["BSDF[4]"], "reflectance", leaf(3)), (pm["Mesh[3]"], "to_world_left", leaf(4, 4))], integ=integ)


def case_pixel_list():
    spec = _cbox()
    sc, pm = _scene(spec)
    return replay(sc, spec, [(pm["BSDF[4]"], "reflectance", leaf(3)), (pm["Mesh[1]"], "to_world_left", leaf(4, 4))], batch_pix=[3, 5, 5, 60])


def case_pixel_list_with_batch_edges():
    spec = _cbox()
    sc, pm = _scene(spec)
    return replay(sc, spec, [(pm["BSDF[4]"], "reflectance", leaf(3)), (pm["Mesh[1]"], "to_world_left", leaf(4, 4))], batch_pix=[3, 5, 5, 60], batch_edges=True)


def case_another_sensor():
    """reverse mode through Sensor[1]: its own pose and primary edges; the pose of Sensor[0] gets no gradient"""
    spec = scenes.with_extra_sensors(_cbox())
    sc, pm = _scene(spec, active=(0, 1, 2))
    return replay(sc, spec, _camera_leaves(pm, "Sensor[1]") + _camera_leaves(pm, "Sensor[0]")[:1] + [(pm["Mesh[2]"], "to_world", leaf(4, 4))], sensor_id=1)


def case_no_emitters():
    spec = _cbox()
    spec.emitters = []
    for m in spec.meshes:
        m.emitter = -1
    sc, pm = _scene(spec)
    return replay(sc, spec, [(pm["BSDF[0]"], "reflectance", leaf(3)), (pm["Mesh[0]"], "to_world_left", leaf(4, 4))])


def case_sphere():
    spec = scenes.sphere_scene(8, 8, 1, 1, 1)
    sc, pm = _scene(spec)
    return replay(sc, spec, _mesh_leaves(pm, "Mesh[1]")[1:] + [(pm["BSDF[6]"], "reflectance", leaf(1))])


def case_microfacet_constants():
    """every g_mat entry of a MicrofacetBSDF, the colours as vectors and as one number, on a one- and a two-sided BSDF"""
    spec = scenes.microfacet_cbox_scene(8, 8, 1, 0, 0, param=None, two_sided=True)
    sc, pm = _scene(spec)
    a, b = pm["BSDF[1]"], pm["BSDF[2]"]
    return replay(sc, spec, [(a, "diffuseReflectance", leaf(3)), (a, "roughness", leaf(1)), (a, "specularReflectance", leaf(3)),
                             (b, "diffuseReflectance", leaf(1)), (b, "roughness", leaf(1, needs=False)), (b, "specularReflectance", leaf(1))])


def case_conductor_constants():
    spec = scenes.conductor_cbox_scene(8, 8, 1, 0, 0, param=None)
    sc, pm = _scene(spec)
    cond = [pm[k] for k in sorted(pm) if k.startswith("BSDF[") and not k.startswith("BSDF[id=") and type(pm[k]).__name__ == "RoughConductorBSDF"]
    leaves = [(cond[0], "alpha_u", leaf(1)), (cond[0], "alpha_v", leaf(1)), (cond[0], "eta", leaf(3)), (cond[0], "k", leaf(3)), (cond[0], "specular_reflectance", leaf(3))]
    if len(cond) > 1:
        leaves += [(cond[1], "eta", leaf(1)), (cond[1], "k", leaf(1)), (cond[1], "specular_reflectance", leaf(1))]
    return replay(sc, spec, leaves)


def case_dielectric_constants():
    spec = scenes.dielectric_cbox_scene(8, 8, 1, 0, 0, param=None)
    sc, pm = _scene(spec)
    die = [pm[k] for k in sorted(pm) if k.startswith("BSDF[") and not k.startswith("BSDF[id=") and type(pm[k]).__name__ == "RoughDielectricBSDF"]
    return replay(sc, spec, [(die[0], "alpha_u", leaf(1)), (die[0], "alpha_v", leaf(1)), (die[0], "eta", leaf(1))])


def case_normalmap_nested_microfacet():
    """the BSDF nested in a normal map owns a row behind the scene's own: its colour, its GGX constants, a bitmap of its own; the map's texels and uv transform"""
    spec = scenes.normalmap_scene(8, 8, 1, 0, 0, nested="microfacet", nmap="bumpy")
    sc, pm = _scene(spec)
    nm, inner = pm["BSDF[0]"], pm["BSDF[0]"]._nested
    return replay(sc, spec, [(nm, "normal_map", leaf(4, 4, 3)), (nm, "normal_map@uv", leaf(4)), (inner, "diffuseReflectance", leaf(3)), (inner, "roughness", leaf(1)),
                             (inner, "specularReflectance", leaf(4, 4, 3)), (pm["BSDF[%d]" % (len(spec.bsdfs) - 1)], "diffuseReflectance", leaf(3))])


def case_normalmap_nested_diffuse():
    spec = scenes.normalmap_scene(8, 8, 1, 0, 0, nested="diffuse", nmap="tilted")
    sc, pm = _scene(spec)
    return replay(sc, spec, [(pm["BSDF[0]"], "normal_map", leaf(3)), (pm["BSDF[0]"]._nested, "reflectance", leaf(1)), (pm["BSDF[1]"], "reflectance", leaf(3))])


def case_bitmaps_microfacet():
    """a bitmap leaf in each of the three slots, the uv transform of each, and a slot the layout reports as constant (offset -1: zeros)"""
    spec = scenes.textured_microfacet_scene(8, 8, 1, 0, 0)
    sc, pm = _scene(spec)
    b = pm["BSDF[0]"]
    return replay(sc, spec, [(b, "diffuseReflectance", leaf(4, 4, 3)), (b, "diffuseReflectance@uv", leaf(4)), (b, "roughness", leaf(4, 4)), (b, "roughness@uv", leaf(4)),
                             (b, "specularReflectance", leaf(4, 4, 3)), (b, "specularReflectance@uv", leaf(4)), (pm["BSDF[1]"], "reflectance", leaf(2, 2, 3))], tex_negative=(3,))


def case_bitmaps_diffuse_under_a_map():
    spec = scenes.textured_scene(8, 8, 1, 0, 0, env=True)
    sc, pm = _scene(spec)
    return replay(sc, spec, [(pm["BSDF[0]"], "reflectance", leaf(4, 4, 3)), (pm["BSDF[1]"], "reflectance", leaf(3))])


def case_uv_transform_alone():
    """a uv leaf of a BSDF without any texel leaf: the texel buffer travels with it"""
    spec = scenes.textured_scene(8, 8, 1, 0, 0, env=True)
    sc, pm = _scene(spec)
    return replay(sc, spec, [(pm["BSDF[0]"], "reflectance@uv", leaf(4))])


def case_bitmaps_conductor():
    spec = scenes.textured_ggx_scene(8, 8, 1, 0, 0, kind="roughconductor")
    sc, pm = _scene(spec)
    b = pm["BSDF[0]"]
    return replay(sc, spec, [(b, "alpha_u", leaf(4, 4)), (b, "alpha_u@uv", leaf(4)), (b, "eta", leaf(4, 4, 3)), (b, "eta@uv", leaf(4)), (b, "k", leaf(4, 4, 3)), (b, "k@uv", leaf(4)),
                             (b, "specular_reflectance", leaf(3))])


def case_bitmaps_dielectric():
    spec = scenes.textured_ggx_scene(8, 8, 1, 0, 0, kind="roughdielectric")
    sc, pm = _scene(spec)
    b = pm["BSDF[0]"]
    return replay(sc, spec, [(b, "alpha_u", leaf(4, 4)), (b, "alpha_v", leaf(1)), (b, "eta", leaf(1))])


def case_per_vertex():
    spec = scenes.pervertex_scene(8, 8, 1, 0, 0)
    sc, pm = _scene(spec)
    b = pm["BSDF[%d]" % (len(spec.bsdfs) - 1)]
    return replay(sc, spec, [(b, "diffuseReflectance", leaf(5, 3)), (b, "roughness", leaf(5)), (b, "specularReflectance", leaf(5, 3))])


def _env_spec(**kw):
    env = (np.arange(4 * 8 * 3, dtype=np.float32).reshape(4, 8, 3) % 11) / 8 + 0.25
    return scenes.envmap_scene(8, 8, 1, 0, 0, param=None, env=env, **kw)


def _env_of(pm):
    return [pm[k] for k in sorted(pm) if k.startswith("Emitter[") and not k.startswith("Emitter[id=") and type(pm[k]).__name__ == "EnvironmentMap"][0]


def case_env_radiance():
    spec = _env_spec()
    sc, pm = _scene(spec)
    return replay(sc, spec, [(_env_of(pm), "radiance", leaf(4, 8, 3))])


def case_env_scale_alone():
    """the scale adjoint is assembled from the texel probes: the texel buffer travels with it"""
    spec = _env_spec()
    sc, pm = _scene(spec)
    return replay(sc, spec, [(_env_of(pm), "scale", leaf(1))])


def case_env_pose():
    """to_world_left through the adjoint of the inverse (a dyadic matrix: the 4 x 4 arithmetic is exact); the map's pose keeps the boundary terms"""
    spec = _env_spec()
    sc, pm = _scene(spec)
    L = torch.diag(torch.tensor([2.0, 0.5, 4.0, 1.0])).requires_grad_(True)
    return replay(sc, spec, [(_env_of(pm), "to_world_left", L)])


def case_env_uv_transform():
    spec = _env_spec()
    sc, pm = _scene(spec)
    return replay(sc, spec, [(_env_of(pm), "radiance@uv", leaf(4))])


def case_env_everything_with_an_area_light():
    spec = _env_spec(area_light=True)
    sc, pm = _scene(spec)
    e = _env_of(pm)
    light = [pm[k] for k in sorted(pm) if k.startswith("Emitter[") and not k.startswith("Emitter[id=") and pm[k] is not e][0]
    return replay(sc, spec, [(pm["BSDF[0]"], "reflectance", leaf(3)), (e, "radiance", leaf(4, 8, 3)), (e, "radiance@uv", leaf(4)), (e, "scale", leaf(1)),
                             (e, "to_world_left", torch.diag(torch.tensor([1.0, 2.0, 0.25, 1.0])).requires_grad_(True)), (light, "radiance", leaf(3))])


CASES = {name[len("case_"):]: fn for name, fn in sorted(globals().items()) if name.startswith("case_")}


if __name__ == "__main__":
    import subprocess
    record = {name: fn() for name, fn in CASES.items()}
    head = subprocess.run(["git", "rev-parse", "HEAD"], cwd=HERE, capture_output=True, text=True).stdout.strip()
    with open(GOLDEN, "w") as fh:
        json.dump({"commit": head, "cases": record}, fh, indent=None, separators=(",", ":"), sort_keys=True)
        fh.write("\n")
    print("wrote %s: %d cases at %s" % (GOLDEN, len(record), head))
