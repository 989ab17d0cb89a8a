"""Reverse-mode vertex gradients against the oracle, vertex by vertex, with the tolerance taken from the oracle alone.

What an optimiser reads is G[k, a] = d <w, img> / d V[k, a] for every vertex k and axis a of a mesh.  The oracle gives the same number in
forward mode: MeshSpec.d_vertices takes any per-vertex tangent, the one-hot tangent e_(k,a) makes its forward derivative column (k, a) of the
Jacobian J, and G[k, a] = <w, J e_(k,a)>.

A summed gradient is dominated by the few samples whose discrete decisions (which triangle, which lobe) a float32 rounding flips, so the
weight is chosen per vertex and term: tests/lane_parity.py's rule for an unsettled row - its response to one of the eight one-ulp nudges of the
camera exceeds ROW_TOL of max(magnitude, floor) - is applied to the three columns (k, x / y / z) of a vertex, and

    w_k      = the random weights (uniform in [0.5, 1.5), one fixed draw), zero on the pixels that are unsettled in any of the three columns
    G[k, a]  = sum_p w_k[p] J e_(k,a) [p]           S[k, a] = sum_p w_k[p] |J e_(k,a)| [p]          S_full: S with the unmasked weights
    r[k, a]  = max over the nudges |G' - G| / S     the oracle's own answer to one ulp of input noise, through the SAME weights

An entry is NON-ZERO when S_full > 0 and RESOLVED when S >= S_full / 2; an entry with S_full == 0 must be exactly zero on the device.
compare() checks the resolved entries, e = |got - G| / S:
    per entry              e <= 16 x max(r[k, a], Q50, 4 * 2^-24)
    per family and term    median(e) <= 16 x max(Q50, 4 * 2^-24)               Q50 = the median of r over the resolved entries
16 is lane_parity's margin.  Unresolved entries are reported, not asserted; tests/test_vertex_adjoint_cpu.py states how many there may be.

Every family runs at 48 x 48, spp = sppe = sppse = 2, depth 3, seeds 5 / 6 / 7 for the interior / primary-edge / secondary-edge term (seed s
of renderD = the oracle's seeds (s, s, s)).

No GPU import: reference() needs the oracle only, compare() needs numpy only."""
import copy
import dataclasses

import numpy as np

import lane_parity as lp
import scenes

RES, DEPTH, SPP = 48, 3, 2
N = RES * RES
TERMS = ("interior", "primary", "secondary")
SEED = {"interior": 5, "primary": 6, "secondary": 7}
WEIGHT_SEED = 11
RESOLVED_SHARE = 0.5        # an entry is resolved when the settled pixels keep at least this share of S_full

# The checked vertices of the tutorial's small ball (162 vertices, in sphere_scene and in pervertex_scene): a fixed subset of 16, all with S_full > 0 in the
# interior term of both families (asserted in tests/test_vertex_adjoint_cpu.py).  Nine of them lie on edges that the primary-edge sampler draws and eight on
# edges that the secondary-edge sampler draws (three on both), so that the edge terms have entries to resolve; 2 and 50 are seen by the interior term alone.
BALL_162 = (2, 9, 22, 24, 33, 39, 50, 58, 59, 64, 73, 81, 94, 112, 133, 136)

# family -> (builder in tests/scenes.py, its keyword arguments, index of the mesh whose vertices are the leaf, the checked vertices or None = all)
FAMILIES = {
    "cbox": ("cbox_scene", dict(param=None), 1, None),                                         # class-1 sweep, brute-force tracer
    "sphere": ("sphere_scene", dict(), 1, BALL_162),                                         # BVH, smooth normals, two-stage secondary-edge adjoint
    "microfacet2s": ("microfacet_cbox_scene", dict(param=None, two_sided=True), 1, None),      # material sweep
    "dielectric": ("dielectric_cbox_scene", dict(param=None), 1, (0, 1, 2, 5, 6, 7)),           # (see DESIGN.md section 2 for vertices 3 and 4)
    "envmap_area": ("envmap_scene", dict(param=None, area_light=True), 0, None),               # class-2 sweep
    "normalmap": ("normalmap_scene", dict(param=None), 1, None),                               # normal-map sweep
    "pervertex": ("pervertex_scene", dict(param=None), 1, BALL_162),                         # smooth ball with a per-vertex BSDF
    "ortho": ("ortho_cbox_scene", dict(param=None), 1, None),                                  # orthographic camera
}

# Edge terms whose oracle record does not meet the conditions of tests/test_vertex_adjoint_cpu.py (half of the non-zero entries resolved, six at least): left
# out of the comparison, DESIGN.md section 2 says why.
LEFT_OUT = {("normalmap", "primary")}


def terms_of(family):
    return tuple(t for t in TERMS if (family, t) not in LEFT_OUT)


def clear_tangents(spec):
    """The spec (in place; -> spec) with every forward tangent (the d_* members of its meshes, BSDFs, emitters and cameras) back at its default"""
    for obj in list(spec.meshes) + list(spec.bsdfs) + list(spec.emitters) + list(spec.cameras):
        for f in dataclasses.fields(obj):
            if f.name.startswith("d_"):
                setattr(obj, f.name, f.default_factory() if f.default_factory is not dataclasses.MISSING else f.default)
    return spec


def build_case(family):
    """-> (spec without tangents, index of the leaf mesh, the checked vertices)"""
    name, kw, mesh, subset = FAMILIES[family]
    spec = clear_tangents(getattr(scenes, name)(RES, RES, SPP, SPP, SPP, **kw))
    nv = len(spec.meshes[mesh].vertices)
    vertices = tuple(range(nv)) if subset is None else tuple(subset)
    assert all(0 <= k < nv for k in vertices) and len(set(vertices)) == len(vertices)
    return spec, mesh, vertices


def weights():
    """The unmasked random weights [N, 3], float32: what the device multiplies the image with"""
    return (np.random.default_rng(WEIGHT_SEED).random((N, 3)) + 0.5).astype(np.float32)


def _columns(orc, spec, mesh, vertices, term):
    """The oracle's forward derivative of one term for the one-hot tangents e_(k,a), k in vertices -> [K, 3, N, 3] float64"""
    s = copy.copy(spec)
    s.meshes = list(spec.meshes)
    m = s.meshes[mesh] = copy.copy(spec.meshes[mesh])
    nv = len(m.vertices)
    bit = getattr(orc, "TERM_" + term.upper())
    out = np.empty((len(vertices), 3, N, 3), np.float64)
    for i, k in enumerate(vertices):
        for a in range(3):
            m.d_vertices = np.zeros((nv, 3), np.float32)
            m.d_vertices[k, a] = 1.0
            d = orc.OracleScene(s, [0]).render_d(max_depth=DEPTH, seeds=(SEED[term],) * 3, terms=bit)[1]
            out[i, a] = lp._clean(d)
    return out


def reference(orc, spec, mesh, vertices, term):
    """The oracle's record of one term of one family.
    -> {term, vertices, mask [K, N] (True: the pixel is settled in all three columns of the vertex), w [K, N, 3] float32 (= w_k),
        G, S, S_full, r [K, 3], nonzero, resolved [K, 3], Q50, G_nudged [8, K, 3], kept_share [K, 3] (S / S_full), lit [K, 3] (pixels in which the column is not zero)}"""
    assert (spec.width, spec.height, spec.spp, spec.sppe, spec.sppse) == (RES, RES, SPP, SPP, SPP)
    spec = clear_tangents(copy.deepcopy(spec))
    vertices = tuple(int(k) for k in vertices)
    delta = lp.rounding_delta(orc.OracleScene(spec, [0]), spec)
    base = _columns(orc, spec, mesh, vertices, term)
    nudges = [_columns(orc, lp.nudged(spec, n, delta), mesh, vertices, term) for n in range(len(lp.NUDGES))]
    return measure(base, nudges, term, vertices)


def measure(base, nudges, term, rows):
    """The record of K rows of A columns each (a vertex and its three axes; a texel, a vertex or a constant and its channels, tests/value_adjoint.py)
    from their forward-derivative columns: base [K, A, N, 3] on the scene itself, nudges the same on each of the eight nudged scenes -> reference()'s record"""
    base = np.asarray(base, np.float64)
    K, A = base.shape[:2]
    assert base.shape == (K, A, N, 3) and len(rows) == K and all(nd.shape == base.shape for nd in nudges)
    mask = np.ones((K, N), bool)
    for i in range(K):
        for a in range(A):
            col = base[i, a]
            spread = np.zeros(N)
            for nd in nudges:
                spread = np.maximum(spread, lp._rowmax(nd[i, a] - col))
            if (col != 0).any():
                unsettled = spread > lp.ROW_TOL * lp._scale(col)[1]
            else:                                       # a column that is zero on the base scene has no magnitude to compare with
                unsettled = spread > 0
            mask[i] &= ~unsettled
    w_full = weights()
    w = np.where(mask[:, :, None], w_full[None], np.float32(0.0)).astype(np.float32)
    w64, w_full64 = w.astype(np.float64), w_full.astype(np.float64)
    G = np.einsum("kpc,kapc->ka", w64, base)
    S = np.einsum("kpc,kapc->ka", w64, np.abs(base))
    S_full = np.einsum("pc,kapc->ka", w_full64, np.abs(base))
    G_nudged = np.stack([np.einsum("kpc,kapc->ka", w64, nd) for nd in nudges])
    nonzero = S_full > 0
    resolved = nonzero & (S >= RESOLVED_SHARE * S_full) & (S > 0)
    safe = np.where(S > 0, S, 1.0)
    r = np.where(S > 0, np.abs(G_nudged - G[None]).max(axis=0) / safe, 0.0)
    Q50 = float(np.median(r[resolved])) if resolved.any() else 0.0
    return dict(term=term, vertices=tuple(rows), mask=mask, w=w, G=G, S=S, S_full=S_full, r=r, nonzero=nonzero, resolved=resolved, Q50=Q50,
                G_nudged=G_nudged, kept_share=np.where(nonzero, S / np.where(nonzero, S_full, 1.0), 0.0), lit=(np.abs(base).max(axis=3) > 0).sum(axis=2))


def compare(got, rec):
    """got [K, 3] (in general [K, A], A the record's columns per row): the gradient of sum(img * w_k) with respect to vertex rec["vertices"][k], against reference()'s record.
    -> {term, entries (non-zero), resolved, p50, Q50, ratio50, worst (the largest e / max(r, Q50, floor) of one entry), worst_entry (vertex, axis),
        unresolved: [(vertex, axis, got, G, kept share)], failures: [str]}; the comparison passes when failures is empty."""
    fails = []
    row = dict(term=rec["term"], entries=int(rec["nonzero"].sum()), resolved=int(rec["resolved"].sum()), p50=0.0, Q50=rec["Q50"], ratio50=0.0,
               worst=0.0, worst_entry=None, unresolved=[], failures=fails)
    g = np.asarray(got, np.float64)
    if g.shape != rec["G"].shape:
        fails.append("%s: shape %r, expected %r" % (rec["term"], g.shape, rec["G"].shape))
        return row
    if not np.isfinite(g).all():
        fails.append("%s: %d entries are not finite" % (rec["term"], int((~np.isfinite(g)).sum())))
        return row
    V = rec["vertices"]
    what, col = rec.get("labels", ("vertex", "axis"))           # (tests/value_adjoint.py names its rows and columns itself)
    for i, a in zip(*np.nonzero(~rec["nonzero"])):                # zero in the oracle: zero here
        if g[i, a] != 0.0:
            fails.append("%s: %s %s %s %d is identically zero in the oracle, got %.3g" % (rec["term"], what, V[i], col, a, g[i, a]))
    for i, a in zip(*np.nonzero(rec["nonzero"] & ~rec["resolved"])):
        row["unresolved"].append((V[i], int(a), float(g[i, a]), float(rec["G"][i, a]), float(rec["kept_share"][i, a])))
    res = rec["resolved"]
    if not res.any():
        return row
    base50 = max(rec["Q50"], lp.ULP_FLOOR)
    e = np.where(res, np.abs(g - rec["G"]) / np.where(res, rec["S"], 1.0), 0.0)
    bound = lp.MARGIN * np.maximum(rec["r"], base50)
    ratio = np.where(res, e / np.maximum(rec["r"], base50), 0.0)
    i, a = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    row["worst"], row["worst_entry"] = float(ratio[i, a]), (V[i], int(a))
    for i, a in zip(*np.nonzero(res & ~(e <= bound))):
        fails.append("%s: %s %s %s %d: got %.9g, oracle %.9g, |difference| / S = %.3g > %g x max(r = %.3g, Q50 = %.3g, %.3g)"
                     % (rec["term"], what, V[i], col, a, g[i, a], rec["G"][i, a], e[i, a], lp.MARGIN, rec["r"][i, a], rec["Q50"], lp.ULP_FLOOR))
    row["p50"] = float(np.median(e[res]))
    row["ratio50"] = row["p50"] / base50
    if row["p50"] > lp.MARGIN * base50:
        fails.append("%s: median |difference| / S of the %d resolved entries %.3g > %g x max(Q50 = %.3g, %.3g)"
                     % (rec["term"], row["resolved"], row["p50"], lp.MARGIN, rec["Q50"], lp.ULP_FLOOR))
    return row


HEADER = "%-13s %-9s %8s %8s %10s %10s %8s %8s  %s" % ("family", "term", "entries", "resolved", "p50", "Q50", "p50/Q50", "worst", "(vertex, axis)")


def format_row(family, row):
    """One line: non-zero and resolved entries, the median error, Q50, their ratio, the largest per-entry ratio e / max(r, Q50, 4 * 2^-24) and its entry"""
    return "%-13s %-9s %8d %8d %10.2e %10.2e %8.2f %8.2f  %s" % (family, row["term"], row["entries"], row["resolved"], row["p50"], row["Q50"],
                                                                row["ratio50"], row["worst"], row["worst_entry"])


ORACLE_HEADER = "%-13s %-9s %8s %8s %10s %22s %32s" % ("family", "term", "entries", "resolved", "keep<half", "kept share min / p50", "r p50 / p90 / max")


def format_oracle_row(family, rec):
    """One line of the oracle's own table: non-zero entries, resolved ones, those that keep less than half of S_full, the smallest and median kept
    share over the non-zero entries, and the percentiles of r over the resolved ones"""
    nz, res = rec["nonzero"], rec["resolved"]
    share = rec["kept_share"][nz]
    r = rec["r"][res]
    return "%-13s %-9s %8d %8d %10d %22s %32s" % (
        family, rec["term"], int(nz.sum()), int(res.sum()), int((nz & ~res).sum()),
        "%.2f / %.2f" % (share.min(), np.median(share)) if share.size else "-",
        "%.1e / %.1e / %.1e" % (np.percentile(r, 50), np.percentile(r, 90), r.max()) if r.size else "-")

