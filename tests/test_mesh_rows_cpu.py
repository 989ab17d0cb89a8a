"""The host's mesh rows against a float64 restatement of the reference (tests/mesh_rows_f64.py), on a corpus of irregular meshes: open grids with holes, flat
shading, rotation x non-uniform scale x shear with tangents on two factors, several meshes, a 240-valence vertex, slivers, a zero-area face, an unused vertex,
edges disabled, a textured mesh, coordinates around 1e4.

The host's rows are what psdr_hip_scene_check_rows compares the device's rows with bit for bit (tests/test_gpu_mesh_rows.py): this test is what ties both to the
reference's formulas.  Bounds are first-order float32 error bounds, C x eps x a scale mesh_rows_f64.error_scales derives from the magnitudes of the inputs
(|to_world_left| |to_world_raw| |to_world_right| |(v, 1)| for a coordinate; that over |cross(e1, e2)| for a unit normal, ...), so a sliver's normal gets the bound
its conditioning allows and a well-shaped face a tight one.

Measured worst errors over the corpus and its three updates, as fractions of their bound at C = 1 (the test asserts <= C_ROWS = 4):
    positions 0.99 (secondary-edge p0 of the fan), edge vectors 0.92, unit face normals 0.37, vertex normals 0.26, areas 0.86,
    tangents: positions 0.71, edge vectors 0.61, face normals 0.43, vertex normals 0.26, areas 0.38.
Slivers (1e-6 of the median area, 16 faces of the "degenerate" case): unit normals off by up to 0.52 in absolute terms, inside the bound their conditioning gives.
Zero-area faces: area 0 and NaN unit normal (0/0, the reference's too), NaN tangents of the normal and the area, and the same NaN pattern as the float64 restatement in every row."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_rows_f64 as ref
import product

EPS = float(np.finfo(np.float32).eps)
C_ROWS = 4.0


def _host_scene(spec, moved, step):
    sc = product.build_scene(spec, host_only=True)
    ref.apply(sc, ref.updates(spec, moved, step))
    sc._configure_host([0])
    return sc


def _offsets(sc, spec):
    f_off, e_off, fo, eo = [], [], 0, 0
    for i, m in enumerate(spec.meshes):
        pm = sc.param_map["Mesh[%d]" % i]
        f_off.append(fo)
        e_off.append(eo if (m.enable_edges and spec.sppse > 0) else None)
        fo += len(m.faces)
        if m.enable_edges and spec.sppse > 0:
            eo += pm.num_edges()
    return f_off, e_off


def _worst(err, scale):
    """largest err / (eps x scale) over the finite entries"""
    r = np.abs(err) / (EPS * np.maximum(scale, 1e-300))
    r = r[np.isfinite(r)]
    return float(r.max()) if r.size else 0.0


def check_mesh(snap, spec, i, f_off, e_off, worst):
    """the rows of spec.meshes[i] in the snapshot against the float64 restatement; `worst` collects err / bound per quantity"""
    m = spec.meshes[i]
    factors, d_factors = ref.factors_of(m)
    F = np.asarray(m.faces, np.int64)
    E = ref.edge_list(F) if e_off is not None else None
    tri, d_tri, sec, d_sec = ref.mesh_rows(m.vertices, F, factors, m.d_vertices, d_factors, E)
    sc = ref.error_scales(m.vertices, F, factors, m.d_vertices, d_factors)
    got, d_got = (np.asarray(snap[k], np.float64)[f_off:f_off + len(F)] for k in ("triangles", "d_triangles"))
    # the NaN pattern first: 0/0 exactly where the reference divides 0 by 0 (zero-area faces, vertices whose faces all have zero area), nowhere else
    assert np.array_equal(np.isnan(got), np.isnan(tri)) and np.array_equal(np.isnan(d_got), np.isnan(d_tri)), "NaN pattern of the triangle rows"
    zero = sc["face_area"] == 0.0
    assert np.all(got[zero, 21] == 0.0) and np.all(np.isnan(got[zero, 18:21])) and np.all(np.isnan(d_got[zero, 18:22]))
    med = np.median(sc["face_area"][~zero])
    good = sc["face_area"] > 1e-6 * med                              # conditioning allows a bound on the normal
    sliver = ~zero & ~good
    pos = sc["pos"][F]                                               # [nf, 3] corner scales
    dpos = sc["dpos"][F]
    bounds = {
        "p0": (got[:, 0:3] - tri[:, 0:3], pos[:, [0]]),
        "e": (got[:, 3:9] - tri[:, 3:9], np.repeat(pos[:, [0]] + pos[:, 1:3], 3, axis=1)),
        "area": (got[:, 21] - tri[:, 21], sc["area"]),
        "d_p0": (d_got[:, 0:3] - d_tri[:, 0:3], dpos[:, [0]]),
        "d_e": (d_got[:, 3:9] - d_tri[:, 3:9], np.repeat(dpos[:, [0]] + dpos[:, 1:3], 3, axis=1)),
        "fn": ((got[:, 18:21] - tri[:, 18:21])[good], sc["fn"][good][:, None]),
        "d_fn": ((d_got[:, 18:21] - d_tri[:, 18:21])[good], sc["dfn"][good][:, None]),
        "d_area": ((d_got[:, 21] - d_tri[:, 21])[~zero], sc["darea"][~zero]),
    }
    fin = np.isfinite(sc["vn"][F])                                   # (corners of zero-area-only vertices: NaN on both sides, checked above)
    vn_err = np.stack([np.abs(got[:, 9 + 3 * c:12 + 3 * c] - tri[:, 9 + 3 * c:12 + 3 * c]).max(axis=1) for c in range(3)], axis=1)
    dvn_err = np.stack([np.abs(d_got[:, 9 + 3 * c:12 + 3 * c] - d_tri[:, 9 + 3 * c:12 + 3 * c]).max(axis=1) for c in range(3)], axis=1)
    bounds["vn"] = (vn_err[fin], sc["vn"][F][fin])
    bounds["d_vn"] = (dvn_err[fin], sc["dvn"][F][fin])
    for k, (err, scale) in bounds.items():
        err = np.asarray(err)
        scale = np.broadcast_to(scale, err.shape)
        assert np.all(np.isfinite(err)), k
        w = _worst(err, scale)
        worst[k] = max(worst.get(k, 0.0), w)
        assert w <= C_ROWS, (k, w)
    # slivers: a unit, finite normal within what their conditioning allows (checked above only for well-shaped faces)
    if sliver.any():
        fn = got[sliver, 18:21]
        assert np.all(np.isfinite(fn)) and np.allclose(np.linalg.norm(fn, axis=1), 1.0, atol=1e-5)
        err = np.abs(fn - tri[sliver, 18:21]).max(axis=1)
        assert np.all(err <= C_ROWS * EPS * sc["fn"][sliver]), (err, EPS * sc["fn"][sliver])
        worst["sliver_fn_abs"] = max(worst.get("sliver_fn_abs", 0.0), float(err.max()))
    # secondary-edge rows: p0 e1 n0 n1 p2 boundary, and the tangents the snapshot carries (d p0, d e1; the estimator uses no others)
    if e_off is None:
        return
    ne = len(E)
    s, ds = (np.asarray(snap[k], np.float64)[e_off:e_off + ne] for k in ("sec_edges", "d_sec_edges"))
    assert s.shape[0] == ne
    bnd = E[:, 3] < 0
    assert np.array_equal(s[:, 15], bnd.astype(np.float64))
    assert np.all(s[bnd, 9:12] == 0.0)                               # n1 of a boundary edge: the masked gather's zero
    ps = sc["pos"]
    for k, (err, scale) in {"sec_p0": (s[:, 0:3] - sec[:, 0:3], ps[E[:, 0]][:, None]), "sec_e1": (s[:, 3:6] - sec[:, 3:6], (ps[E[:, 0]] + ps[E[:, 1]])[:, None]),
                            "sec_p2": (s[:, 12:15] - sec[:, 12:15], ps[E[:, 4]][:, None]),
                            "sec_d_p0": (ds[:, 0:3] - d_sec[:, 0:3], sc["dpos"][E[:, 0]][:, None]),
                            "sec_d_e1": (ds[:, 3:6] - d_sec[:, 3:6], (sc["dpos"][E[:, 0]] + sc["dpos"][E[:, 1]])[:, None])}.items():
        w = _worst(err, np.broadcast_to(scale, err.shape))
        worst[k] = max(worst.get(k, 0.0), w)
        assert np.all(np.isfinite(err)) and w <= C_ROWS, (k, w)
    assert np.all(ds[:, 6:] == 0.0)
    g0, g1 = good[E[:, 2]], ~bnd & good[np.maximum(E[:, 3], 0)]
    for k, col, rows, fid in (("sec_n0", 6, g0, E[:, 2]), ("sec_n1", 9, g1, np.maximum(E[:, 3], 0))):
        err = (s[:, col:col + 3] - sec[:, col:col + 3])[rows]
        w = _worst(err, np.broadcast_to(sc["fn"][fid][rows][:, None], err.shape))
        worst[k] = max(worst.get(k, 0.0), w)
        assert w <= C_ROWS, (k, w)
    # (the same NaN pattern: n0 / n1 of the edges of a zero-area face)
    assert np.array_equal(np.isnan(s), np.isnan(sec))


CASES = ref.corpus()


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_rows_match_the_float64_reference(name):
    spec, moved = CASES[name]
    spec = copy.deepcopy(spec)
    assert sum(len(m.faces) for m in spec.meshes) > 64                # every case is a BVH scene (kBruteForceMax = 64)
    worst = {}
    for step in range(3):
        sc = _host_scene(spec, moved, step)
        snap = sc._snapshot()
        f_off, e_off = _offsets(sc, spec)
        for i in range(len(spec.meshes)):
            m = spec.meshes[i]
            if e_off[i] is not None:
                assert np.array_equal(np.asarray(sc.param_map["Mesh[%d]" % i].edge_indices(), np.int64), ref.edge_list(m.faces)), "edge list"
            check_mesh(snap, spec, i, f_off[i], e_off[i], worst)
    print(name, {k: round(v, 4) for k, v in sorted(worst.items())})


def test_chain_restatement_agrees_with_the_float64_reference():
    """psdr_jit_amd.chain.snapshot_tensors (the reverse-mode chain rule's restatement) against the new one: the same values, row for row"""
    import torch
    from psdr_jit_amd import chain
    spec, moved = CASES["sheared"]
    sc = product.build_scene(spec, host_only=True)
    leaf = lambda obj, name: torch.as_tensor(np.asarray(obj._get(name, False), np.float64), dtype=torch.float64).requires_grad_(True)
    tri, sec = chain.snapshot_tensors(sc, 0, leaf)[:2]
    m = spec.meshes[0]
    factors, _ = ref.factors_of(m)
    want, _, wsec, _ = ref.mesh_rows(m.vertices, m.faces, factors, edges=ref.edge_list(m.faces))
    got = tri.detach().numpy()[:len(m.faces)]
    assert np.allclose(got, want, rtol=0, atol=1e-12)
    assert np.allclose(sec.detach().numpy()[:len(wsec)], wsec[:, :6], rtol=0, atol=1e-12)
