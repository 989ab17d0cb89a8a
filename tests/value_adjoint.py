"""Reverse-mode gradients of the VALUE leaves - bitmap texels, per-vertex BSDF values, environment-map texels, BSDF and emitter constants - against the
oracle, entry by entry: tests/vertex_adjoint.py's measure with a texel, a vertex or a constant in the place of a mesh vertex.

A ROW is one texel, one vertex or one constant parameter; its A COLUMNS are its channels (3 for RGB, 1 for a roughness / alpha map or a scalar).  The oracle
gives column (k, a) of the Jacobian in forward mode under the one-hot tangent e_(k,a) of the leaf (d_texture, d_spec_texture, d_rough_texture, d_pv_*,
d_env_data, d_reflectance ...), and what an optimiser reads from leaf.grad is G[k, a] = <w, J e_(k,a)>.  Everything else is vertex_adjoint's: the weight w_k
is the one fixed random draw, zero on the pixels that a one-ulp nudge of the camera unsettles in any column of row k; S, S_full, r, non-zero, resolved and
compare() with MARGIN, ROW_TOL, ULP_FLOOR and RESOLVED_SHARE as they stand there.  No tolerance is added here.

Why entry by entry: the four bilinear weights of a footprint sum to 1 and so do the three barycentric weights, so the dot product of the gradient with a
tangent that is constant over the map - what the buffer-by-buffer tests take - is unchanged by ANY permutation of where the scatter lands inside the map.

The settings are vertex_adjoint's (48 x 48, spp = sppe = sppse = 2, depth 3, WEIGHT_SEED 11), interior term only, seed 5: every value leaf's edge terms are
identically zero in the oracle (tests/test_value_adjoint_cpu.py asserts it once per kind of leaf) and are not launched on the device.

No GPU import: reference() needs the oracle only, compare() needs numpy only."""
import copy

import numpy as np

import lane_parity as lp
import scenes
import vertex_adjoint as va

RES, DEPTH, SPP, N = va.RES, va.DEPTH, va.SPP, va.N
TERM, SEED = "interior", va.SEED["interior"]
BALL_162 = va.BALL_162
MAX_ROWS = 24               # of a leaf that is not checked whole

UV_XF = (0.4, 1.7, 0.13, -0.21)             # rotate, scale, translate of the 5 x 3 diffuse map: turned, repeated 1.7 times over the floor and shifted, so lookups wrap in u and in v
ENV_UV_XF = (0.3, 1.2, 0.27, -0.1)          # tests/test_gpu_adjoint.py's transform of the environment map

# the 8 x 8 diffuse map: every third texel and the two corners that skips (four corners, four texels on every border row and column)
EVERY_THIRD_8X8 = tuple(sorted(set(range(0, 64, 3)) | {7, 56}))
# the 16 x 16 normal map: every fifteenth texel - the four corners 0, 15, 240, 255 and the anti-diagonal between them
EVERY_15TH_16X16 = tuple(range(0, 256, 15))
# the 16 x 8 environment map (texel = y * 16 + x): both seam columns x = 0 and 15 in the first row pair (y = 0, 1: texels 0, 15, 16, 31), half way down (48, 63) and in the last row pair
# (py is clamped to H - 2 = 6: texels 96, 111 and, in the row that no sample of this scene reaches, 112, 127), all lit through bounces alone like texel 24; and thirteen of the texels that
# background pixels look at directly (rows 3 to 6, columns 5 to 10), x-neighbours among them.  Found once from S_full at depth 0 and at depth 3; tests/test_value_adjoint_cpu.py asserts
# what is said here.
ENV16_DIRECT = (54, 55, 56, 57, 69, 70, 71, 74, 87, 88, 101, 102, 106)
ENV16 = tuple(sorted((0, 15, 16, 31, 24, 48, 63, 96, 111, 112, 127) + ENV16_DIRECT))
# the same map under ENV_UV_XF: the band that the camera sees moves to columns 10 to 15 and wraps to column 0, so the seam columns are looked at directly in rows 5 to 7
ENV16_XF_DIRECT = (74, 75, 76, 77, 78, 80, 90, 91, 94, 95, 96, 107, 108, 111, 112, 123, 124, 127)
ENV16_XF = tuple(sorted((0, 15, 16, 31, 36, 52) + ENV16_XF_DIRECT))
# the 128 x 64 environment map (texel = y * 128 + x).  Found once, as BALL_162 was, from S_full of every texel at depth 0 (541 texels that background pixels look at: rows 29 to 51, columns
# 48 to 78) and at depth 3 (2318 lit texels).  Ten of the first kind - four x-neighbours in a row of the upper edge of that band (4022 to 4025: a wave's 32 pixels span about 14 texels there, more
# than the eight merge rounds), two more neighbours (5692, 5693) and four apart - seven lit through bounces alone, texel 896 of them in column 0 and 2175 in column 127, 2048 next to it across
# the seam, and 8191 in the last row, which nothing reaches.
ENV128_DIRECT = (4022, 4023, 4024, 4025, 4680, 5173, 5692, 5693, 6086, 6221)
ENV128_BOUNCE_ONLY = (896, 1388, 1505, 1810, 2133, 2175, 2690)
ENV128 = tuple(sorted(ENV128_DIRECT + ENV128_BOUNCE_ONLY + (2048, 8191)))
DARK_CANDIDATES = 16


def _floor_5x3():
    spec = scenes.textured_scene(RES, RES, SPP, SPP, SPP, texture=scenes.ramp_texture(5, 3), env=True)
    spec.bsdfs[0].tex_xf = [list(UV_XF), [0, 1, 0, 0], [0, 1, 0, 0]]
    return spec


def _env(w, h, xf=None):
    spec = scenes.envmap_scene(RES, RES, SPP, SPP, SPP, param=None, area_light=True, env=scenes.synthetic_envmap(w, h))
    if xf is not None:
        spec.emitters[0].env_uv_xf = tuple(xf)
    return spec


def _builder(name, **kw):
    return lambda: getattr(scenes, name)(RES, RES, SPP, SPP, SPP, **kw)


_mf = _builder("textured_microfacet_scene")
_cond = _builder("textured_ggx_scene", kind="roughconductor")
_diel = _builder("textured_ggx_scene", kind="roughdielectric")
_pv = _builder("pervertex_scene", param=None)

# leaf -> (kind, scene builder, (list of the spec, index in it, member), the checked rows or None = all).  A map's row is the texel y * W + x of the member's [H, W(, 3)] array, a per-vertex
# leaf's row the mesh-local vertex.  Kinds: "bitmap" (checked whole unless rows are given), "pervertex", "env".
LEAVES = {
    "diffuse5x3": ("bitmap", _floor_5x3, ("bsdfs", 0, "texture"), None),                                  # adjoint_mat.h footprint, CH = 3, with a uv transform, W != H
    "mf_diffuse8x8": ("bitmap", _mf, ("bsdfs", 0, "texture"), EVERY_THIRD_8X8),
    "mf_specular5x6": ("bitmap", _mf, ("bsdfs", 0, "spec_texture"), None),
    "mf_roughness9x7": ("bitmap", _mf, ("bsdfs", 0, "rough_texture"), None),                              # CH = 1
    "cond_eta4x5": ("bitmap", _cond, ("bsdfs", 0, "texture"), None),
    "cond_k6x4": ("bitmap", _cond, ("bsdfs", 0, "spec_texture"), None),
    "cond_alpha7x6": ("bitmap", _cond, ("bsdfs", 0, "rough_texture"), None),
    "diel_alpha7x6": ("bitmap", _diel, ("bsdfs", 0, "rough_texture"), None),
    "normalmap16x16": ("bitmap", _builder("normalmap_scene", param=None), ("bsdfs", 0, "texture"), EVERY_15TH_16X16),
    "pv_diffuse": ("pervertex", _pv, ("bsdfs", 5, "pv_diffuse"), BALL_162),
    "pv_specular": ("pervertex", _pv, ("bsdfs", 5, "pv_specular"), BALL_162),
    "pv_roughness": ("pervertex", _pv, ("bsdfs", 5, "pv_roughness"), BALL_162),
    "env16": ("env", lambda: _env(16, 8), ("emitters", 0, "env_data"), ENV16),                            # 1.5 KB of adjoints: the LDS route
    "env16_xf": ("env", lambda: _env(16, 8, ENV_UV_XF), ("emitters", 0, "env_data"), ENV16_XF),
    "env128": ("env", lambda: _env(128, 64), ("emitters", 0, "env_data"), ENV128),                        # 96 KB: the deferred wave merge and the plain atomics
}

# "constants": one row per constant of the Cornell families; (scene key, list of the spec, index, member, columns).  The one-hot tangent of the rough glass's eta moves
# inv_eta = 1 / eta with it, as the product's eta leaf does (scenes.dielectric_cbox_scene's 'eta').
CONSTANT_SCENES = {
    "gold": _builder("conductor_cbox_scene", param=None),
    "microfacet": _builder("microfacet_cbox_scene", param=None, two_sided=True),
    "glass": _builder("dielectric_cbox_scene", param=None),
    "cbox": _builder("cbox_scene", param=None),
}
CONSTANTS = (
    ("gold", "bsdfs", 5, "alpha_u", 1), ("gold", "bsdfs", 5, "alpha_v", 1), ("gold", "bsdfs", 5, "eta", 3), ("gold", "bsdfs", 5, "k", 3), ("gold", "bsdfs", 5, "specular", 3),
    ("microfacet", "bsdfs", 1, "specular", 3), ("microfacet", "bsdfs", 1, "reflectance", 3), ("microfacet", "bsdfs", 1, "roughness", 1),
    ("glass", "bsdfs", 5, "alpha_u", 1), ("glass", "bsdfs", 5, "alpha_v", 1), ("glass", "bsdfs", 5, "eta", 1),
    ("cbox", "emitters", 0, "radiance", 3),                 # the luminaire
    ("cbox", "bsdfs", 2, "reflectance", 3),                 # the white walls, floor and ceiling
)
ALL = tuple(LEAVES) + ("constants",)


def build_case(leaf):
    """-> (spec without tangents, (list, index, member), the checked rows, the leaf's value as an array, W or None)"""
    kind, builder, where, rows = LEAVES[leaf]
    spec = va.clear_tangents(builder())
    value = np.asarray(getattr(getattr(spec, where[0])[where[1]], where[2]), np.float32)
    n = value.shape[0] if kind == "pervertex" else value.shape[0] * value.shape[1]
    rows = tuple(range(n)) if rows is None else tuple(rows)
    assert all(0 <= k < n for k in rows) and len(set(rows)) == len(rows) and (len(rows) == n or len(rows) <= MAX_ROWS), leaf
    return spec, where, rows, value, (None if kind == "pervertex" else value.shape[1])


def columns_of(value, kind):
    return 1 if value.ndim == (1 if kind == "pervertex" else 2) else 3


def _render(orc, spec, depth=DEPTH, term=TERM):
    d = orc.OracleScene(spec, [0]).render_d(max_depth=depth, seeds=(SEED,) * 3, terms=getattr(orc, "TERM_" + term.upper()))[1]
    return lp._clean(d)


def _with_copy(spec, where):
    """a shallow copy of the spec whose object at `where` is its own -> (spec, object)"""
    s = copy.copy(spec)
    objs = list(getattr(spec, where[0]))
    obj = objs[where[1]] = copy.copy(objs[where[1]])
    setattr(s, where[0], objs)
    return s, obj


def one_hot_column(orc, spec, where, value, A, row, a, depth=DEPTH, term=TERM):
    """The oracle's forward derivative under the one-hot tangent of entry (row, a) of an array leaf of A columns per row -> [N, 3]"""
    s, obj = _with_copy(spec, where)
    d = np.zeros(value.shape, np.float32)
    d.reshape(-1, A)[row, a] = 1.0
    setattr(obj, "d_" + where[2], d)
    return _render(orc, s, depth, term)


def constant_column(orc, spec, const, a, term=TERM):
    """... of component a of one constant -> [N, 3]"""
    _, lst, idx, member, ncol = const
    s, obj = _with_copy(spec, (lst, idx, member))
    if ncol == 1:
        if member == "eta":                                 # RoughDielectric: (eta, 1 / eta, -)
            e = np.float32(obj.eta[0])
            t = (1.0, float(-np.float32(1.0) / (e * e)), 0.0)
        else:
            t = 1.0
    else:
        t = tuple(1.0 if c == a else 0.0 for c in range(3))
    setattr(obj, "d_" + member, t)
    return _render(orc, s, DEPTH, term)


def _record(base, nudges, rows, labels):
    rec = va.measure(base, nudges, TERM, rows)
    rec["labels"] = labels
    return rec


def reference(orc, leaf):
    """The oracle's record of one leaf (vertex_adjoint.reference's members; "vertices" holds the rows), plus: spec, where, value, W (a map's width), kind.
    For "constants": rows = indices into CONSTANTS, three columns each, the columns a scalar does not have identically zero; valid [K, 3] says which exist."""
    if leaf == "constants":
        specs = {k: va.clear_tangents(b()) for k, b in CONSTANT_SCENES.items()}
        deltas = {k: lp.rounding_delta(orc.OracleScene(s, [0]), s) for k, s in specs.items()}
        valid = np.array([[a < c[4] for a in range(3)] for c in CONSTANTS])

        def cols(version):
            out = np.zeros((len(CONSTANTS), 3, N, 3), np.float64)
            for i, c in enumerate(CONSTANTS):
                s = specs[c[0]] if version is None else lp.nudged(specs[c[0]], version, deltas[c[0]])
                for a in range(c[4]):
                    out[i, a] = constant_column(orc, s, c, a)
            return out
        rec = _record(cols(None), [cols(n) for n in range(len(lp.NUDGES))], tuple(range(len(CONSTANTS))), ("constant", "channel"))
        rec.update(specs=specs, valid=valid, kind="constants", W=None)
        return rec
    kind = LEAVES[leaf][0]
    spec, where, rows, value, W = build_case(leaf)
    assert (spec.width, spec.height, spec.spp, spec.sppe, spec.sppse) == (RES, RES, SPP, SPP, SPP)
    A = columns_of(value, kind)
    delta = lp.rounding_delta(orc.OracleScene(spec, [0]), spec)

    def cols(s):
        out = np.empty((len(rows), A, N, 3), np.float64)
        for i, k in enumerate(rows):
            for a in range(A):
                out[i, a] = one_hot_column(orc, s, where, value, A, k, a)
        return out
    rec = _record(cols(spec), [cols(lp.nudged(spec, n, delta)) for n in range(len(lp.NUDGES))], rows,
                  ("vertex" if kind == "pervertex" else "texel", "channel"))
    rec.update(spec=spec, where=where, value=value, W=W, kind=kind)
    return rec


def dark_candidates(leaf):
    """At most DARK_CANDIDATES unchecked rows of a leaf that is not checked whole, spread evenly (an environment map: over its last row, which the lookup's clamp
    py <= H - 2 reaches through the weight w1y alone): where all their columns are identically zero in the oracle, the device's gradient must be exactly zero"""
    kind, _, _, rows = LEAVES[leaf]
    if rows is None:
        return ()
    _, _, rows, value, W = build_case(leaf)
    n = value.shape[0] if kind == "pervertex" else value.shape[0] * value.shape[1]
    pool = [k for k in range(n - W if kind == "env" else 0, n) if k not in rows]
    return tuple(pool[:: max(1, len(pool) // DARK_CANDIDATES)][:DARK_CANDIDATES])


def dark_rows(orc, leaf):
    """The candidates whose every column is identically zero in the oracle (one render per entry, no nudges)"""
    cand = dark_candidates(leaf)
    if not cand:
        return ()
    spec, where, _, value, _ = build_case(leaf)
    A = columns_of(value, LEAVES[leaf][0])
    return tuple(k for k in cand if not any(one_hot_column(orc, spec, where, value, A, k, a).any() for a in range(A)))


def s_full_of_rows(orc, leaf, rows, depth=DEPTH):
    """S_full of whole rows of an RGB leaf (the three channels moved together, one render per row, no nudges) at one depth -> [len(rows)]: which texels the oracle lights at all (depth 3)
    and which of them background pixels look at directly (depth 0).  ENV128 was found from this over every texel of the map."""
    spec, where, _, value, _ = build_case(leaf)
    w = va.weights().astype(np.float64)
    out = np.zeros(len(rows))
    for i, k in enumerate(rows):
        s, obj = _with_copy(spec, where)
        d = np.zeros(value.shape, np.float32)
        d.reshape(-1, 3)[k] = 1.0
        setattr(obj, "d_" + where[2], d)
        out[i] = float((w * np.abs(_render(orc, s, depth))).sum())
    return out


compare = va.compare
HEADER = va.HEADER.replace("family", "leaf  ", 1).replace("(vertex, axis)", "(row, channel)")
format_row = va.format_row
ORACLE_HEADER = va.ORACLE_HEADER.replace("family", "leaf  ", 1) + " %22s" % "lit pixels min / p50"


def format_oracle_row(leaf, rec):
    """vertex_adjoint's line, and the smallest and median number of pixels in which a non-zero entry's column is not zero"""
    n = rec["lit"][rec["nonzero"]]
    return va.format_oracle_row(leaf, rec) + " %22s" % ("%d / %d" % (n.min(), np.median(n)) if n.size else "-")
