"""A float64 restatement of the reference's mesh processing, and a corpus of irregular meshes to hold the product's rows against it.

The rows a configured mesh contributes (psdr_triangles, psdr_sec_edges; tests see them through Scene._snapshot()):
  * Mesh::configure (reference src/shape/mesh.cpp:317-341): to_world = to_world_left . to_world_raw . to_world_right, world vertices = transform_pos(to_world, raw)
    (include/psdr/core/transform.h:110-113: the homogeneous divide included);
  * process_mesh (mesh.cpp:23-62): p0 e1 e2; face normal = cross(e1, e2), face area = |face normal|; per vertex the sum of its faces' normals divided by the sum of
    their areas, normalised (0/0 for a vertex no face uses); then face normal /= area, area *= 0.5.  Rows of 22: p0 e1 e2 n0 n1 n2 fn area;
  * the edge list (mesh.cpp:102-150): std::map over (min, max) vertex ids in face order; per edge v0 v1, f0 = first face, f1 = second face or -1, opp = the vertex
    opposite the edge in the first face; rows in key order;
  * SecondaryEdgeInfo (mesh.cpp:355-369): p0 = V[v0], e1 = V[v1] - p0, n0 = fn[f0], n1 = fn[f1] (a masked gather: 0 on a boundary edge), p2 = V[opp],
    is_boundary = f1 < 0.  Rows of 16: p0 e1 n0 n1 p2 boundary (the snapshot's layout).

Forward tangents come from torch.func.jvp with the tangents Mesh._set(name, value, tangent) installs on vertex_positions and the three transform factors.
Nothing here uses psdr_jit_amd.chain or the oracle."""
import numpy as np
import torch

from oracle.oracle import BsdfSpec, CameraSpec, EmitterSpec, MeshSpec, SceneSpec

F64 = torch.float64
FACTORS = ("to_world_left", "to_world_raw", "to_world_right")


def edge_list(faces):
    """[n_edges, 5] v0 v1 f0 f1 opp, reference mesh.cpp:102-150"""
    em = {}
    for f, tri in enumerate(np.asarray(faces, np.int64).tolist()):
        for i in range(3):
            a, b, c = tri[i], tri[(i + 1) % 3], tri[(i + 2) % 3]
            key = (a, b) if a < b else (b, a)
            if key not in em:
                em[key] = [c]
            em[key].append(f)
    rows = [(k[0], k[1], v[1], v[2] if len(v) >= 3 else -1, v[0]) for k, v in sorted(em.items())]
    return np.asarray(rows, np.int64).reshape(-1, 5)


def _norm(x):
    # sqrt(dot): the reference's norm, whose derivative at 0 is 0/0 as drjit's is (torch.linalg.norm would return a subgradient there)
    return torch.sqrt((x * x).sum(-1))


def _rows(V, L, R, Rt, F, E):
    M = L @ R @ Rt
    h = V @ M[:3, :3].T + M[:3, 3]
    Vw = h / (V @ M[3, :3] + M[3, 3])[:, None]
    i0, i1, i2 = F[:, 0], F[:, 1], F[:, 2]
    p0 = Vw[i0]
    e1, e2 = Vw[i1] - p0, Vw[i2] - p0
    n = torch.linalg.cross(e1, e2)
    a = _norm(n)
    vs = torch.zeros_like(Vw)
    vw = torch.zeros(Vw.shape[0], dtype=F64)
    for idx in (i0, i1, i2):
        vs = vs.index_add(0, idx, n)
        vw = vw.index_add(0, idx, a)
    vn = vs / vw[:, None]
    vn = vn / _norm(vn)[:, None]
    fn = n / a[:, None]
    tri = torch.cat([p0, e1, e2, vn[i0], vn[i1], vn[i2], fn, (0.5 * a)[:, None]], dim=1)
    if E is None or E.shape[0] == 0:
        return tri, torch.zeros((0, 16), dtype=F64)
    bnd = E[:, 3] < 0
    sp0 = Vw[E[:, 0]]
    n1 = torch.where(bnd[:, None], torch.zeros(3, dtype=F64), fn[E[:, 3].clamp(min=0)])
    sec = torch.cat([sp0, Vw[E[:, 1]] - sp0, fn[E[:, 2]], n1, Vw[E[:, 4]], bnd.to(F64)[:, None]], dim=1)
    return tri, sec


def mesh_rows(vertices, faces, factors, d_vertices=None, d_factors=None, edges=None):
    """-> (tri, d_tri, sec, d_sec) float64 numpy: the triangle rows [n_faces, 22] and secondary-edge rows [n_edges, 16] of one mesh and their forward tangents.
    factors / d_factors: the three transform factors (left, raw, right) and their tangents; edges: [n, 5] v0 v1 f0 f1 opp or None (no edge rows)."""
    t = lambda x: torch.as_tensor(np.asarray(x, np.float64), dtype=F64)
    V = t(vertices).reshape(-1, 3)
    P = tuple(t(m).reshape(4, 4) for m in factors)
    dV = t(d_vertices).reshape(-1, 3) if d_vertices is not None else torch.zeros_like(V)
    dP = tuple(t(m).reshape(4, 4) for m in d_factors) if d_factors is not None else tuple(torch.zeros((4, 4), dtype=F64) for _ in range(3))
    F = torch.as_tensor(np.asarray(faces, np.int64)).reshape(-1, 3)
    E = torch.as_tensor(np.asarray(edges, np.int64)).reshape(-1, 5) if edges is not None else None
    (tri, sec), (d_tri, d_sec) = torch.func.jvp(lambda v, l, r, rt: _rows(v, l, r, rt, F, E), (V,) + P, (dV,) + dP)
    return tri.numpy(), d_tri.numpy(), sec.numpy(), d_sec.numpy()


def error_scales(vertices, faces, factors, d_vertices=None, d_factors=None):
    """First-order float32 error scales of the rows (float64 numpy), from the magnitudes of the inputs: the forward error bound of a product of matrices and a vector,
    |fl(A B C x) - A B C x| <~ |A| |B| |C| |x| x (a few units of roundoff), carried through the formulas of process_mesh.  Returns a dict of
      pos  [nv]      bound on a world coordinate's error in units of roundoff;       dpos [nv]  the same for its tangent;
      fn   [nf]      on the unit face normal's error (its conditioning: |dE| (|e1| + |e2|) / |n|);   dfn  [nf]  on its tangent;
      area [nf] / darea [nf], vn [nv] / dvn [nv] (per vertex: the normal sum's error over |sum of normals|)
    Every entry is a multiple of one unit of float32 roundoff: compare errors with C x eps x scale."""
    A = lambda x: np.abs(np.asarray(x, np.float64))
    L, R, Rt = (A(m).reshape(4, 4) for m in factors)
    dL, dR, dRt = (A(m).reshape(4, 4) for m in d_factors) if d_factors is not None else (np.zeros((4, 4)),) * 3
    V = np.asarray(vertices, np.float64).reshape(-1, 3)
    dV = A(d_vertices).reshape(-1, 3) if d_vertices is not None else np.zeros_like(V)
    Vh = np.concatenate([np.abs(V), np.ones((len(V), 1))], axis=1)
    Mabs = L @ R @ Rt
    dMabs = dL @ R @ Rt + L @ dR @ Rt + L @ R @ dRt
    pos = (Vh @ Mabs[:3].T).max(axis=1)
    dpos = (Vh @ dMabs[:3].T + dV @ Mabs[:3, :3].T).max(axis=1) + 1e-300
    # exact (float64) world geometry and its tangent, for the lengths the bounds scale with
    Vt = torch.as_tensor(V, dtype=F64)
    M = torch.as_tensor(np.asarray(factors[0], np.float64).reshape(4, 4) @ np.asarray(factors[1], np.float64).reshape(4, 4) @ np.asarray(factors[2], np.float64).reshape(4, 4))
    Vw = ((Vt @ M[:3, :3].T + M[:3, 3]) / (Vt @ M[3, :3] + M[3, 3])[:, None]).numpy()
    dM = sum(np.asarray(a, np.float64).reshape(4, 4) @ np.asarray(b, np.float64).reshape(4, 4) @ np.asarray(c, np.float64).reshape(4, 4)
             for a, b, c in ((d_factors[0], factors[1], factors[2]), (factors[0], d_factors[1], factors[2]), (factors[0], factors[1], d_factors[2]))) \
        if d_factors is not None else np.zeros((4, 4))
    dVr = np.asarray(d_vertices, np.float64).reshape(-1, 3) if d_vertices is not None else np.zeros_like(V)
    dVw = V @ dM[:3, :3].T + dM[:3, 3] + dVr @ M.numpy()[:3, :3].T        # (affine transforms: w = 1, dw = 0)
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    p0 = Vw[F[:, 0]]
    e1, e2 = Vw[F[:, 1]] - p0, Vw[F[:, 2]] - p0
    de1, de2 = dVw[F[:, 1]] - dVw[F[:, 0]], dVw[F[:, 2]] - dVw[F[:, 0]]
    n = np.cross(e1, e2)
    dn = np.cross(de1, e2) + np.cross(e1, de2)
    an = np.linalg.norm(n, axis=1)
    L1 = np.linalg.norm(e1, axis=1) + np.linalg.norm(e2, axis=1)
    dL1 = np.linalg.norm(de1, axis=1) + np.linalg.norm(de2, axis=1)
    dE = pos[F].max(axis=1)                  # a vertex coordinate's error scale over the face (roundoff units x magnitude)
    ddE = dpos[F].max(axis=1)
    n_err = dE * L1 + an                     # the normal's error: from its vertices, and its own rounding
    dn_err = ddE * L1 + dE * dL1 + np.linalg.norm(dn, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        fn = n_err / an
        dfn = dn_err / an + np.linalg.norm(dn, axis=1) / an * fn
        nv = len(V)
        S = np.zeros((nv, 3)); dS = np.zeros((nv, 3)); Se = np.zeros(nv); dSe = np.zeros(nv)
        for c in range(3):
            np.add.at(S, F[:, c], n); np.add.at(dS, F[:, c], dn)
            np.add.at(Se, F[:, c], n_err); np.add.at(dSe, F[:, c], dn_err)
        aS = np.linalg.norm(S, axis=1)
        vn = Se / aS
        dvn = dSe / aS + np.linalg.norm(dS, axis=1) / aS * vn
        darea = 0.5 * (dn_err + np.linalg.norm(dn, axis=1) * fn)        # d|n| = n.dn / |n|: the direction's error times |dn|, and dn's own
    return {"pos": pos, "dpos": dpos, "fn": fn, "dfn": dfn, "area": 0.5 * n_err, "darea": darea, "vn": vn, "dvn": dvn,
            "face_area": 0.5 * an}


# ------------------------------------------------------------------------------------------------------------------------------------------------------------
# The corpus: small scenes of more than 64 triangles (kBruteForceMax: the BVH path, on which configure() computes moved meshes' rows on the device), each
# with a light quad outside the view and a camera on -z looking at +z.

def _eye():
    return np.eye(4, dtype=np.float32)


def _translate(x, y, z):
    m = _eye()
    m[:3, 3] = [x, y, z]
    return m


def _grid(n, size=2.0, holes=(), bump=0.15, row_heights=None, seed=0, noise=0.2):
    """an n x n grid of quads (two triangles each) over [-size/2, size/2]^2 in z = bump x a smooth height field; `holes`: quads left out (boundary edges
    inside the grid); row_heights: the heights of the n rows of quads (default: equal)"""
    xs = np.linspace(-size / 2, size / 2, n + 1)
    if row_heights is None:
        ys = xs.copy()
    else:
        ys = -size / 2 + np.concatenate([[0.0], np.cumsum(row_heights)])
    X, Y = np.meshgrid(xs, ys, indexing="xy")
    rng = np.random.default_rng(seed)
    Z = bump * (np.sin(2.1 * X + 0.3) * np.cos(1.7 * Y) + noise * rng.standard_normal(X.shape))
    v = np.stack([X, Y, Z], axis=-1).reshape(-1, 3).astype(np.float32)
    f = []
    for j in range(n):
        for i in range(n):
            if (i, j) in holes:
                continue
            a, b, c, d = j * (n + 1) + i, j * (n + 1) + i + 1, (j + 1) * (n + 1) + i + 1, (j + 1) * (n + 1) + i
            if (i + j) % 2:
                f += [[a, b, c], [a, c, d]]
            else:
                f += [[a, b, d], [b, c, d]]
    return v, np.asarray(f, np.int32)


def _fan(k, radius=0.9, seed=1):
    """k triangles around one vertex (valence k), a slightly wavy disk"""
    ang = np.linspace(0.0, 2 * np.pi, k, endpoint=False)
    rng = np.random.default_rng(seed)
    r = radius * (1.0 + 0.05 * rng.standard_normal(k))
    ring = np.stack([r * np.cos(ang), r * np.sin(ang), 0.1 * np.sin(3 * ang)], axis=1)
    v = np.concatenate([[[0.0, 0.0, 0.05]], ring]).astype(np.float32)
    f = np.asarray([[0, 1 + i, 1 + (i + 1) % k] for i in range(k)], np.int32)
    return v, f


def _rotation(axis, deg):
    a = np.radians(deg)
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    m = np.eye(4)
    m[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    return m.astype(np.float32)


def _light(offset=(0.0, 0.0, 0.0)):
    """a 2-triangle emitter quad above the view (normal +z, toward the meshes)"""
    ox, oy, oz = offset
    v = np.array([[-1.5, 2.2, -2.0], [1.5, 2.2, -2.0], [1.5, 3.4, -2.0], [-1.5, 3.4, -2.0]], np.float32) + np.asarray(offset, np.float32)
    return MeshSpec(vertices=v, faces=np.array([[0, 1, 2], [0, 2, 3]], np.int32), bsdf=1, emitter=0)


def _scene(meshes, offset=(0.0, 0.0, 0.0), texture=None, size=24):
    bsdfs = [BsdfSpec((0.6, 0.5, 0.4), two_sided=True, name="grey", texture=texture), BsdfSpec((0.0, 0.0, 0.0), name="light")]
    cam = CameraSpec(60.0, 1e-3, 1e7, to_world_raw=_translate(offset[0], offset[1], offset[2] - 4.0))
    return SceneSpec(meshes + [_light(offset)], bsdfs, [EmitterSpec((6.0, 6.0, 6.0))], [cam], size, size, 2, 2, 2)


def _dv(v, seed):
    rng = np.random.default_rng(seed)
    return (0.2 * rng.standard_normal(v.shape)).astype(np.float32)


def corpus():
    """name -> (SceneSpec, [index of every mesh the updates move]).  Tangents installed: see each case."""
    cases = {}
    holes = {(2, 2), (3, 2), (5, 5), (0, 7)}
    # an open grid with holes (boundary edges on the border and around the holes), translated, a tangent on the translation and on the vertices
    v, f = _grid(8, holes=holes)
    dT = np.zeros((4, 4), np.float32); dT[0, 3] = 1.0; dT[2, 3] = -0.5
    cases["open_grid"] = (_scene([MeshSpec(vertices=v, faces=f, to_world_left=_translate(0.1, -0.2, 0.3), d_to_world_left=dT, d_vertices=_dv(v, 1))]), [0])
    # the same grid flat-shaded
    cases["flat_grid"] = (_scene([MeshSpec(vertices=v, faces=f, to_world_left=_translate(0.1, -0.2, 0.3), d_to_world_left=dT, d_vertices=_dv(v, 2),
                                           use_face_normals=True)]), [0])
    # rotation x non-uniform scale x shear; tangents on to_world_right and the vertices at once
    v, f = _grid(7, bump=0.3, seed=3)
    S = np.diag([1.3, 0.6, 2.0, 1.0]).astype(np.float32)
    H = _eye(); H[0, 1] = 0.4; H[2, 0] = -0.3; H[1, 2] = 0.25
    dH = np.zeros((4, 4), np.float32); dH[0, 1] = 1.0; dH[2, 2] = 0.5; dH[1, 3] = 0.3
    cases["sheared"] = (_scene([MeshSpec(vertices=v, faces=f, to_world_left=_rotation((1, 2, 0.5), 35.0), to_world_raw=S, to_world_right=H,
                                         d_to_world_right=dH, d_vertices=_dv(v, 4))]), [0])
    # two moved meshes with an unmoved one between them (non-zero vertex, face and edge offsets on the device)
    va, fa = _grid(5, size=0.9, seed=5)
    vb, fb = _grid(4, size=0.9, seed=6, holes={(1, 1)})
    vc, fc = _grid(5, size=0.9, seed=7, holes={(0, 0)})
    cases["three_meshes"] = (_scene([MeshSpec(vertices=va, faces=fa, to_world_left=_translate(-1.0, 0.0, 0.0), d_vertices=_dv(va, 8)),
                                     MeshSpec(vertices=vb, faces=fb, to_world_left=_translate(0.0, 0.1, 0.2)),
                                     MeshSpec(vertices=vc, faces=fc, to_world_left=_translate(1.0, 0.0, 0.1), d_to_world_left=dT)]), [0, 2])
    # a fan of 240 triangles around one vertex
    v, f = _fan(240)
    cases["fan"] = (_scene([MeshSpec(vertices=v, faces=f, d_vertices=_dv(v, 9))]), [0])
    # slivers (a row of quads 1e-6 as tall as the others), a zero-area face (two of its corners at the same raw position) and a vertex no face uses
    n = 8
    rows = np.full(n, 2.0 / n)
    rows[3] = 2.5e-7 * 2.0 / n
    v, f = _grid(n, row_heights=rows, bump=0.2, seed=10, noise=0.0)          # (a smooth height field: the thin row stays thin in z as well)
    extra = np.array([[0.3, -0.9, -0.2], [0.3, -0.9, -0.2], [0.6, -0.7, -0.2], [5.0, 5.0, 5.0]], np.float32)      # (the last one: unused)
    k = len(v)
    v = np.concatenate([v, extra])
    f = np.concatenate([f, np.array([[k, k + 1, k + 2]], np.int32)])
    cases["degenerate"] = (_scene([MeshSpec(vertices=v, faces=f, to_world_left=_rotation((0, 1, 0), 20.0), d_to_world_left=dT, d_vertices=_dv(v, 11))]), [0])
    # edges disabled on the moved mesh
    v, f = _grid(8, seed=12, holes={(4, 4)})
    cases["no_edges"] = (_scene([MeshSpec(vertices=v, faces=f, d_to_world_left=dT, enable_edges=False, d_vertices=_dv(v, 13))]), [0])
    # a textured mesh (uv per vertex, a textured diffuse BSDF)
    v, f = _grid(8, seed=14)
    uv = np.ascontiguousarray((v[:, :2] + 1.0) / 2.0).astype(np.float32)
    tex = np.stack(list(np.meshgrid(np.linspace(0.2, 0.9, 8), np.linspace(0.9, 0.2, 8))) + [np.full((8, 8), 0.5)], axis=-1).astype(np.float32)
    cases["textured"] = (_scene([MeshSpec(vertices=v, faces=f, uvs=uv, face_uvs=f.copy(), d_to_world_left=dT, d_vertices=_dv(v, 15))], texture=tex), [0])
    # geometry around 1e4: the raw vertices carry the offset, the camera and the light follow
    off = (1.0e4, -2.0e4, 1.5e4)
    v, f = _grid(8, seed=16, holes={(6, 1)})
    v = (v.astype(np.float64) + np.asarray(off)).astype(np.float32)
    cases["far"] = (_scene([MeshSpec(vertices=v, faces=f, d_to_world_left=dT, d_vertices=_dv(v, 17))], offset=off), [0])
    return cases


def factors_of(m):
    return (m.to_world_left, m.to_world_raw, m.to_world_right), (m.d_to_world_left, m.d_to_world_raw, m.d_to_world_right)


def updates(spec, moved, step):
    """the state of update `step` (0, 1, 2, ...): per moved mesh a new vertex field, transform or tangent, written into `spec` and returned as
    [(mesh index, parameter name, value, tangent)] for Mesh._set"""
    out = []
    for i in moved:
        m = spec.meshes[i]
        rng = np.random.default_rng(100 * step + i)
        kind = step % 3
        if kind == 0:              # the raw vertices deform (a smooth wave + noise) with a new tangent
            v = np.asarray(m.vertices, np.float64)
            c = v.mean(axis=0)
            w = v.copy()
            # (a function of the position alone: coincident corners stay coincident, the slivers stay slivers)
            w[:, 2] += 0.05 * np.sin(3.0 * (v[:, 0] - c[0]) + step) + 0.03 * np.cos(2.0 * (v[:, 1] - c[1]) - step)
            m.vertices = w.astype(np.float32)
            m.d_vertices = (0.3 * rng.standard_normal(v.shape)).astype(np.float32)
            out.append((i, "vertex_positions", m.vertices, m.d_vertices))
        elif kind == 1:            # the left factor moves (a rotation about the mesh's centre + a translation), its tangent changes
            Lm = np.asarray(m.to_world_left, np.float64)
            M = Lm @ np.asarray(m.to_world_raw, np.float64) @ np.asarray(m.to_world_right, np.float64)
            c = (np.asarray(m.vertices, np.float64) @ M[:3, :3].T + M[:3, 3]).mean(axis=0)
            T = _translate(*(c + 0.05 * rng.standard_normal(3))).astype(np.float64) @ _rotation(rng.standard_normal(3), 4.0 * (step + 1)) @ _translate(*(-c))
            m.to_world_left = (T @ Lm).astype(np.float32)
            d = np.zeros((4, 4), np.float32); d[:3, 3] = rng.standard_normal(3)
            m.d_to_world_left = d
            out.append((i, "to_world_left", m.to_world_left, m.d_to_world_left))
        else:                      # only a tangent changes: the one on the right factor
            d = (0.2 * rng.standard_normal((4, 4))).astype(np.float32); d[3] = 0.0
            m.d_to_world_right = d
            out.append((i, "to_world_right", np.asarray(m.to_world_right, np.float32), m.d_to_world_right))
    return out


def apply(sc, changes):
    for i, name, value, tangent in changes:
        key = "to_world" if name == "to_world_raw" else name
        sc.param_map["Mesh[%d]" % i]._set(key, np.ascontiguousarray(value, np.float32), np.ascontiguousarray(tangent, np.float32))
