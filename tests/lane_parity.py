"""Per-sample parity of radiance and of its derivatives, with the tolerance taken from the oracle alone.

At spp = 1 pixel p of an interior-term render IS lane p, for the image and for its forward derivative; at sppe = sppse = 1 a pixel of
an edge term holds at most a few samples.  So five outputs of one 128 x 128 frame are compared row by row:

    lanes    the general path kernel's per-lane radiance (psdr_hip_li_lanes / OracleScene.li_lanes)
    img      the interior term's image          d_int   its forward derivative          (render_d, TERM_INTERIOR)
    d_prim   the primary-edge term's derivative                                         (render_d, TERM_PRIMARY)
    d_sec    the secondary-edge term's derivative                                       (render_d, TERM_SECONDARY)

Which rows may differ, and how tightly the others must agree, comes from the oracle's own answer to a one-ulp change of its input:
the camera position is moved by (+-delta, +-delta, +-delta), delta = one float32 ulp of the largest coordinate in the scene, and the
eight nudged frames are compared with the base frame.  A row whose relative response r exceeds 1e-3 under some nudge sits on a
discrete decision (which triangle, which lobe) that float32 rounding flips: it is UNSETTLED.  The percentiles of r over the settled
rows say what one ulp of input noise does to a sample that takes the same decisions.

The comparison of a device output with the base frame then has two conditions:
  1. at most 2 % of the rows differ by more than 1e-3 (the oracle alone stays inside 1 %, tests/test_lane_parity_cpu.py);
  2. over the other non-zero rows, the 50th and 99th percentile of the relative error are at most 16 x max(Q_q, 4 * 2^-24), Q_q the
     same percentile of r: the device differs from the oracle by a few ulp at a handful of sites per bounce (libm, contraction).
  3. (lanes, img, d_int, where row p is lane p) the same median bound again within the rows of every first-hit BSDF that lights at
     least 64 rows of the output: over ALL its non-zero rows (a median needs no rows left out), p50 <= 16 x max(Q_50 of those rows,
     4 * 2^-24).  Conditions 1 and 2 alone do not resolve one material: at one sample per pixel the small GGX boxes light 100-200 of the
     16384 rows, so an error of 1e-3 on every one of them is "left out" far below the cap, and one of 1e-4 sits above the 99th percentile.
An output that is identically zero in the oracle (a material parameter's edge terms, a scene without edges) must be identically zero.

No GPU import at module level: reference() needs the oracle only, compare() needs numpy only."""
import copy
import itertools

import numpy as np

import scenes

OUTPUTS = ("lanes", "img", "d_int", "d_prim", "d_sec")
INTERIOR = ("lanes", "img", "d_int")        # row p = lane p
RES, DEPTH, SEED = 128, 3, 5
N = RES * RES
ROW_TOL = 1e-3              # a row is unsettled (oracle) / left out (device) beyond this relative difference
LEFT_OUT_CAP = 0.02         # condition 1, device
UNSETTLED_CAP = 0.01        # the oracle's own share (CPU test): half of the cap
MARGIN = 16.0               # condition 2
ULP_FLOOR = 4.0 * 2.0 ** -24
PERCENTILES = (50, 99)
LOBE_ROWS = 64              # condition 3: a first-hit BSDF counts as a lobe of an output when it lights at least this many rows

# family -> (builder in tests/scenes.py, its keyword arguments); every builder is called with (128, 128, 1, 1, 1, ...)
FAMILIES = {
    "cbox": ("cbox_scene", dict(param="box_x")),                                            # 36 triangles: the brute-force (LDS) tracer
    "sphere": ("sphere_scene", dict()),                                                     # 652 triangles: BVH
    "microfacet2s": ("microfacet_cbox_scene", dict(param="box_x", two_sided=True)),
    "conductor": ("conductor_cbox_scene", dict(param="alpha")),
    "dielectric": ("dielectric_cbox_scene", dict(param="eta")),
    "envmap_area": ("envmap_scene", dict(param="box_x", area_light=True)),
    "envmap_balls": ("envmap_scene", dict(param="albedo", balls=True)),
    "normalmap": ("normalmap_scene", dict(param="box_x")),
    "pervertex": ("pervertex_scene", dict(param="ball_x")),
    "ortho": ("ortho_cbox_scene", dict(param="box_x")),
    "textured_ggx": ("textured_ggx_scene", dict(kind="roughconductor", param="box_x")),
    "config5_l3": ("config5_scene", dict(level=3, env_res=(128, 64), param="albedo")),     # 1294 triangles, BVH + environment map
}


def build_spec(family):
    name, kw = FAMILIES[family]
    return getattr(scenes, name)(RES, RES, 1, 1, 1, **kw)


def _clean(a):
    return np.nan_to_num(np.asarray(a, np.float32), nan=0.0, posinf=0.0, neginf=0.0)


def rounding_delta(ref, spec):
    """One float32 ulp of the largest absolute coordinate among the world-space triangle vertices and the camera position"""
    ti = np.asarray(ref.triangle_info(), np.float32)
    p0, e1, e2 = ti[:, 0:3], ti[:, 3:6], ti[:, 6:9]
    cam = np.asarray(spec.cameras[0].to_world_raw, np.float32)[:3, 3]
    R = max(float(np.abs(p0).max()), float(np.abs(p0 + e1).max()), float(np.abs(p0 + e2).max()), float(np.abs(cam).max()))
    return np.spacing(np.float32(R))


NUDGES = tuple(itertools.product((1.0, -1.0), repeat=3))


def nudged(spec, k, delta):
    """The spec with cameras[0] moved by NUDGES[k] * delta, added in float32"""
    s = copy.deepcopy(spec)
    m = np.array(s.cameras[0].to_world_raw, dtype=np.float32)
    m[:3, 3] = m[:3, 3] + np.float32(delta) * np.asarray(NUDGES[k], np.float32)
    s.cameras[0].to_world_raw = m
    return s


def oracle_outputs(orc, spec, ref=None):
    """The five outputs of one scene on the oracle, scrubbed"""
    ref = ref if ref is not None else orc.OracleScene(spec, [0])
    out = {"lanes": _clean(ref.li_lanes(0, N, max_depth=DEPTH, seed=SEED))}
    img, d = ref.render_d(max_depth=DEPTH, seeds=(SEED, SEED, SEED), terms=orc.TERM_INTERIOR)
    out["img"], out["d_int"] = _clean(img), _clean(d)
    out["d_prim"] = _clean(ref.render_d(max_depth=DEPTH, seeds=(SEED, SEED, SEED), terms=orc.TERM_PRIMARY)[1])
    out["d_sec"] = _clean(ref.render_d(max_depth=DEPTH, seeds=(SEED, SEED, SEED), terms=orc.TERM_SECONDARY)[1])
    return out


def _rowmax(a):
    return np.abs(np.asarray(a, np.float64)).max(axis=1)


def _scale(base):
    """(mag, max(mag, floor)) of an output: floor = 1e-3 x the median non-zero row magnitude"""
    mag = _rowmax(base)
    nz = mag > 0
    floor = 1e-3 * float(np.median(mag[nz])) if nz.any() else 0.0
    return mag, np.maximum(mag, floor if floor > 0 else 1.0)


def _share(flag, among):
    return float(flag[among].mean()) if among.any() else 0.0


def first_hit_bsdf(orc, spec):
    """BSDF index of the surface behind each lane's camera ray (-1: none - the ray leaves the scene or meets the environment map's
    bounding cube), from the oracle's segmentation field"""
    ref = orc.OracleScene(spec, [0])
    ref.set_field("segmentation")
    seg = np.rint(ref.li_lanes(0, N, max_depth=DEPTH, seed=SEED)[:, 0]).astype(np.int64)
    ids = np.array([-1] + [m.bsdf for m in spec.meshes], np.int64)
    return np.where(seg < len(ids), ids[np.clip(seg, 0, len(ids) - 1)], -1)


def reference(orc, spec, keep_nudges=False):
    """The oracle's record of one family: per output the base frame, each row's response to the eight one-ulp nudges, the settled
    mask, Q_q and the first-hit BSDFs that count as lobes.
    -> {"delta", "surface", "first_hit", "bsdf_names", "out": {name: {base, mag, denom, spread, r, settled, nonzero, moved, moved_all, unsettled_share, Q, lobes}},
        ["nudges": the eight nudged frames]}"""
    ref = orc.OracleScene(spec, [0])
    delta = rounding_delta(ref, spec)
    base = oracle_outputs(orc, spec, ref)
    spread = {k: np.zeros(N) for k in OUTPUTS}
    kept = []
    for k in range(len(NUDGES)):
        o = oracle_outputs(orc, nudged(spec, k, delta))
        for name in OUTPUTS:
            spread[name] = np.maximum(spread[name], _rowmax(o[name].astype(np.float64) - base[name].astype(np.float64)))
        if keep_nudges:
            kept.append(o)
    # a lane that sees the environment map directly depends on its ray's direction alone, which no translation of the camera changes:
    # whether the nudge reaches the samples ("moved") is asked of the rows whose camera ray meets a surface
    first = first_hit_bsdf(orc, spec)
    surface = first >= 0
    rec = {"delta": float(delta), "surface": surface, "first_hit": first, "bsdf_names": [b.name or "bsdf%d" % i for i, b in enumerate(spec.bsdfs)], "out": {}}
    for name in OUTPUTS:
        mag, denom = _scale(base[name])
        r = spread[name] / denom
        settled, nonzero = r <= ROW_TOL, mag > 0
        sel = settled & nonzero
        Q = {q: (float(np.percentile(r[sel], q)) if sel.any() else 0.0) for q in PERCENTILES}
        lobes = {}                                   # first-hit BSDF -> (its non-zero rows, Q_50 of its non-zero settled rows)
        if name in INTERIOR:
            for b in np.unique(first[surface]):
                rows = nonzero & (first == b)
                if rows.sum() >= LOBE_ROWS and (rows & settled).any():
                    lobes[int(b)] = (rows, float(np.percentile(r[rows & settled], 50)))
        rec["out"][name] = dict(lobes=lobes, base=base[name], mag=mag, denom=denom, spread=spread[name], r=r, settled=settled, nonzero=nonzero,
                                moved=_share(spread[name] > 0, nonzero & surface if name in INTERIOR else nonzero),
                                moved_all=_share(spread[name] > 0, nonzero),
                                unsettled_share=float((~settled).mean()), Q=Q)
    if keep_nudges:
        rec["nudges"] = kept
    return rec


def compare(got, ref_record, outputs=OUTPUTS):
    """got: {output: [N, 3] array} (any subset of `outputs`) against reference()'s record.
    -> {output: {left_out, unsettled, p50, p99, Q50, Q99, ratio50, ratio99, lobe_ratio, lobe (the first-hit BSDF with the largest median ratio),
    failures: [str]}}; an output passes when failures is empty."""
    res = {}
    for name in outputs:
        if name not in got:
            continue
        o = ref_record["out"][name]
        g = _clean(got[name])
        fails = []
        row = dict(left_out=0.0, unsettled=o["unsettled_share"], failures=fails, lobe_ratio=0.0, lobe="-")
        for q in PERCENTILES:
            row["p%d" % q], row["Q%d" % q], row["ratio%d" % q] = 0.0, o["Q"][q], 0.0
        res[name] = row
        if g.shape != o["base"].shape:
            fails.append("%s: shape %r, expected %r" % (name, g.shape, o["base"].shape))
            continue
        if not o["nonzero"].any():                    # identically zero in the oracle: identically zero here
            nzg = int((_rowmax(g) > 0).sum())
            if nzg:
                fails.append("%s: identically zero in the oracle, %d non-zero rows (max |value| %.3g)" % (name, nzg, float(np.abs(g).max())))
                row["left_out"] = nzg / len(g)
            continue
        e = _rowmax(g.astype(np.float64) - o["base"].astype(np.float64)) / o["denom"]
        left = e > ROW_TOL
        row["left_out"] = float(left.mean())
        if row["left_out"] > LEFT_OUT_CAP:
            fails.append("%s: %.3f %% of the rows differ by more than %g (cap %.0f %%, the oracle's own unsettled share %.3f %%)"
                         % (name, 100 * row["left_out"], ROW_TOL, 100 * LEFT_OUT_CAP, 100 * o["unsettled_share"]))
        for b, (rows, Q50) in o["lobes"].items():
            p, bound_base = float(np.percentile(e[rows], 50)), max(Q50, ULP_FLOOR)
            if p / bound_base >= row["lobe_ratio"]:
                row["lobe_ratio"], row["lobe"] = p / bound_base, ref_record["bsdf_names"][b]
            if p > MARGIN * bound_base:
                fails.append("%s: first-hit BSDF %r (%d rows): median relative error %.3g > %g x max(Q50 = %.3g, %.3g)"
                             % (name, ref_record["bsdf_names"][b], int(rows.sum()), p, MARGIN, Q50, ULP_FLOOR))
        keep = o["nonzero"] & ~left
        if not keep.any():
            fails.append("%s: no non-zero row left to compare" % name)
            continue
        for q in PERCENTILES:
            p = float(np.percentile(e[keep], q))
            bound_base = max(o["Q"][q], ULP_FLOOR)
            row["p%d" % q], row["ratio%d" % q] = p, p / bound_base
            if p > MARGIN * bound_base:
                fails.append("%s: p%d of the kept rows' relative error %.3g > %g x max(Q%d = %.3g, %.3g)" % (name, q, p, MARGIN, q, o["Q"][q], ULP_FLOOR))
    return res


def failures(res):
    return [f for row in res.values() for f in row["failures"]]


HEADER = "%-13s %-7s %9s %10s %10s %10s %8s %10s %10s %8s  %s" % ("family", "output", "left-out%", "unsettled%", "p50", "Q50", "p50/Q50", "p99", "Q99", "p99/Q99", "worst lobe p50/Q50")


def format_rows(family, res):
    """One line per output: the shares in per cent, both percentiles and their ratios to max(Q_q, 4 * 2^-24), the largest per-BSDF median ratio"""
    return ["%-13s %-7s %9.3f %10.3f %10.2e %10.2e %8.2f %10.2e %10.2e %8.2f  %.2f %s"
            % (family, name, 100 * r["left_out"], 100 * r["unsettled"], r["p50"], r["Q50"], r["ratio50"], r["p99"], r["Q99"], r["ratio99"], r["lobe_ratio"], r["lobe"])
            for name, r in res.items()]
