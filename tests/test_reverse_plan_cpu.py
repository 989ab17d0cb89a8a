"""The host side of renderD's reverse mode (psdr_jit_amd/reverse.py) without a GPU, on host-configured scenes.

1. Layouts agree: the shapes of the psdr_grads buffers from reverse.Layout, from tests/adjoint_buffers.py (the tests' own statement) and the counts spelled out from
   the spec are equal for every scene family reverse mode covers - an undersized buffer is an out-of-bounds write on the GPU, so this holds before any GPU run.
   (The texel layout is a number here; the real one is compared on the GPU by the tests that use g_tex.)
2. Routing equals the recorded one: tests/golden/make_reverse_routing.py replays backward() through stubs that fill every buffer with a ramp of its own;
   tests/golden/reverse_routing.json is its record of the commit before the routing moved into reverse.py.  Every launch argument and every gradient entry is
   compared exactly (integer ramps in float32: nothing to round)."""
import importlib.util
import json
import os

import numpy as np
import pytest

import adjoint_buffers
import product
import scenes

HERE = os.path.dirname(os.path.abspath(__file__))
_mod = importlib.util.spec_from_file_location("make_reverse_routing", os.path.join(HERE, "golden", "make_reverse_routing.py"))
routing = importlib.util.module_from_spec(_mod)
_mod.loader.exec_module(routing)


def _no_emitters():
    spec = scenes.cbox_scene(8, 8, 1, 1, 1, param=None)
    spec.emitters = []
    for m in spec.meshes:
        m.emitter = -1
    return spec


_FAMILIES = {
    "cbox": lambda: scenes.cbox_scene(8, 8, 1, 1, 1, param=None),
    "cbox_interior_only": lambda: scenes.cbox_scene(8, 8, 1, 0, 0, param=None),
    "three_sensors": lambda: scenes.with_extra_sensors(scenes.cbox_scene(8, 8, 1, 1, 1, param=None)),
    "microfacet": lambda: scenes.microfacet_cbox_scene(8, 8, 1, 1, 1, param=None),
    "microfacet_two_sided": lambda: scenes.microfacet_cbox_scene(8, 8, 1, 0, 0, param=None, two_sided=True),
    "normalmap_microfacet": lambda: scenes.normalmap_scene(8, 8, 1, 0, 0, nested="microfacet", nmap="bumpy"),
    "normalmap_diffuse": lambda: scenes.normalmap_scene(8, 8, 1, 1, 1, nested="diffuse", nmap="tilted"),
    "conductor": lambda: scenes.conductor_cbox_scene(8, 8, 1, 0, 0, param=None),
    "dielectric": lambda: scenes.dielectric_cbox_scene(8, 8, 1, 0, 0, param=None),
    "pervertex": lambda: scenes.pervertex_scene(8, 8, 1, 1, 1),
    "textured_diffuse": lambda: scenes.textured_scene(8, 8, 1, 0, 0, env=True),
    "textured_microfacet": lambda: scenes.textured_microfacet_scene(8, 8, 1, 0, 0),
    "textured_conductor": lambda: scenes.textured_ggx_scene(8, 8, 1, 0, 0, kind="roughconductor"),
    "envmap": lambda: scenes.envmap_scene(8, 8, 1, 1, 1, param=None),
    "envmap_area_light": lambda: scenes.envmap_scene(8, 8, 1, 0, 0, param=None, area_light=True, balls=True),
    "sphere": lambda: scenes.sphere_scene(8, 8, 1, 1, 1),
    "no_emitters": _no_emitters,
}


@pytest.mark.parametrize("family", list(_FAMILIES))
def test_layouts_agree(family):
    from psdr_jit_amd import reverse
    spec = _FAMILIES[family]()
    active = tuple(range(len(spec.cameras)))
    sc = product.build_scene(spec, host_only=True, active=active)
    pm, snap = sc.param_map, sc._snapshot()
    env = adjoint_buffers.env_map(spec)
    tex_total, env_texels = 777, int(np.prod(env.env_data.shape)) if env is not None else 0
    # the counts, written out from the spec
    n_hidden = sum(1 for b in spec.bsdfs if getattr(b, "type", 0) == 5)
    n_b = len(spec.bsdfs) + n_hidden
    n_tris = sum(len(m.faces) for m in spec.meshes) + (12 if env is not None else 0)          # (the map's bounding box)
    assert len(snap["bsdf_rows"]) == n_b
    for sensor_id in active:
        layout = reverse.Layout(sc, sensor_id)
        mine, theirs = layout.shapes(tex_total, env_texels), adjoint_buffers.shapes(sc, spec, tex_total, sensor_id)
        assert set(theirs) <= set(mine) and set(mine) - set(theirs) <= {"g_env"}
        for f in theirs:
            assert tuple(mine[f]) == tuple(theirs[f]), (family, sensor_id, f, mine[f], theirs[f])
        assert mine["g_triangles"] == (n_tris, 22) and mine["g_bsdf"] == (max(1, n_b), 3) and mine["g_mat"] == (max(1, n_b), 16)
        assert mine["g_emitter"] == (max(1, len(spec.emitters)), 3) and mine["g_uv_xf"] == (3 * n_b + 1, 4)
        assert mine["g_sec_edges"] == (max(1, np.asarray(snap["d_sec_edges"]).shape[0]), 6) and mine["g_tex"] == (tex_total,) and mine["g_env"] == (env_texels,)
        assert (layout.n_own, layout.n_hidden, layout.n_emitters, layout.n_meshes) == (len(spec.bsdfs), n_hidden, len(spec.emitters), sc.num_meshes)
        assert layout.edge_mesh.shape == (layout.n_prim,) and (layout.n_prim > 0) == (spec.sppe > 0)
        # the identity maps: the scene's own BSDFs in order, the nested ones behind them in the order of their maps; meshes and emitters by their index
        hidden = len(spec.bsdfs)
        for k, b in enumerate(spec.bsdfs):
            assert layout.bsdf_row(pm["BSDF[%d]" % k]) == k
            if getattr(b, "type", 0) == 5:
                assert layout.bsdf_row(pm["BSDF[%d]" % k]._nested) == hidden
                hidden += 1
        for k in range(sc.num_meshes):
            if "Mesh[%d]" % k in pm:
                assert layout.mesh_row(pm["Mesh[%d]" % k]) == k
        for k in range(len(spec.emitters)):
            assert layout.emitter_rows[id(pm["Emitter[%d]" % k])] == k
    import psdr_jit_amd as psdr
    with pytest.raises(RuntimeError):
        reverse.Layout(sc).bsdf_row(psdr.DiffuseBSDF([0.5, 0.5, 0.5]))
    with pytest.raises(RuntimeError):
        reverse.Layout(sc).mesh_row(psdr.Mesh())


with open(routing.GOLDEN) as _fh:
    _GOLDEN = json.load(_fh)


def test_the_record_covers_the_cases():
    assert set(_GOLDEN["cases"]) == set(routing.CASES) and len(_GOLDEN["commit"]) == 40


@pytest.mark.parametrize("case", sorted(routing.CASES))
def test_routing_equals_the_recorded_one(case):
    got = json.loads(json.dumps(routing.CASES[case]()))
    want = _GOLDEN["cases"][case]
    assert got["launches"] == want["launches"]
    assert got["geometry"] == want["geometry"]
    assert got["tex_layout_calls"] == want["tex_layout_calls"]
    assert [n for n, _ in got["grads"]] == [n for n, _ in want["grads"]]
    for (name, g), (_, w) in zip(got["grads"], want["grads"]):
        assert g == w, (case, name)
