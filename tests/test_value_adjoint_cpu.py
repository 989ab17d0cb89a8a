"""The oracle's side of the per-entry measure of reverse mode into value leaves (tests/value_adjoint.py), without a GPU: the oracle resolves
every non-zero entry of every leaf (so the GPU test cannot hide a failure in what it leaves out), the rows named in value_adjoint are what their comments say, and the
comparison has teeth - the oracle's own gradients, moved about inside a map in ways that leave their sum unchanged, fail compare.  The existing reverse-mode tests contract
the gradient with a tangent that is constant over the map, which is that sum: each permutation below is asserted to keep it."""
import numpy as np
import pytest

import lane_parity as lp
import value_adjoint as vad

MIN_NONZERO = 12


@pytest.fixture(scope="module")
def records(orc):
    """leaf -> record, made once and left unchanged"""
    cache = {}

    def get(leaf):
        if leaf not in cache:
            cache[leaf] = vad.reference(orc, leaf)
        return cache[leaf]
    return get


def _columns(rec):
    return rec["G"].shape[1]


def _whole_map(leaf):
    return leaf != "constants" and vad.LEAVES[leaf][0] == "bitmap" and vad.LEAVES[leaf][3] is None


@pytest.mark.parametrize("leaf", vad.ALL)
def test_oracle_resolves_every_entry(records, leaf):
    rec = records(leaf)
    print()
    print(vad.ORACLE_HEADER)
    print(vad.format_oracle_row(leaf, rec))
    nz, res = rec["nonzero"], rec["resolved"]
    assert np.array_equal(nz, res), (leaf, int(nz.sum()), int(res.sum()))            # every non-zero entry is resolved
    assert (rec["S"][res] > 0).all() and np.isfinite(rec["r"]).all()
    if leaf == "constants":
        assert np.array_equal(nz, rec["valid"]), [vad.CONSTANTS[i] for i in np.nonzero((nz != rec["valid"]).any(axis=1))[0]]      # every listed constant, every channel
    else:
        assert int(nz.sum()) >= MIN_NONZERO, (leaf, int(nz.sum()))
    if leaf == "diffuse5x3":
        assert nz.all() and nz.size == 45


def test_the_rows_of_the_subsets_are_what_their_comments_say(orc):
    def xy(rows, W):
        return [(k % W, k // W) for k in rows]
    for rows, W, H in ((vad.EVERY_THIRD_8X8, 8, 8), (vad.EVERY_15TH_16X16, 16, 16)):
        assert len(rows) <= vad.MAX_ROWS and {0, W - 1, (H - 1) * W, H * W - 1} <= set(rows)
        p = xy(rows, W)
        assert any(x == 0 for x, y in p) and any(x == W - 1 for x, y in p) and any(y == 0 for x, y in p) and any(y == H - 1 for x, y in p)
    # the 16 x 8 environment map: both seam columns, the first and the last row pair, texels that background pixels see
    p = xy(vad.ENV16, 16)
    assert len(vad.ENV16) <= vad.MAX_ROWS
    for y in (0, 1, 6, 7):
        assert (0, y) in p and (15, y) in p
    direct = vad.s_full_of_rows(orc, "env16", vad.ENV16_DIRECT, 0)
    assert set(vad.ENV16_DIRECT) <= set(vad.ENV16) and len(vad.ENV16_DIRECT) >= 8 and (direct > 0).all()
    p = xy(vad.ENV16_XF, 16)
    assert len(vad.ENV16_XF) <= vad.MAX_ROWS and set(vad.ENV16_XF_DIRECT) <= set(vad.ENV16_XF) and (vad.s_full_of_rows(orc, "env16_xf", vad.ENV16_XF_DIRECT, 0) > 0).all()
    for y in (0, 1, 6, 7):
        assert (0, y) in p and (15, y) in p
    # the 128 x 64 one: 16 to 24 texels; at least 8 that background pixels look at, with two pairs of x-neighbours among them; at least 4 lit through bounces alone; columns 0 and 127
    assert 16 <= len(vad.ENV128) <= vad.MAX_ROWS and set(vad.ENV128_DIRECT) | set(vad.ENV128_BOUNCE_ONLY) <= set(vad.ENV128)
    assert len(vad.ENV128_DIRECT) >= 8 and (vad.s_full_of_rows(orc, "env128", vad.ENV128_DIRECT, 0) > 0).all()
    assert sum(1 for k in vad.ENV128_DIRECT if k + 1 in vad.ENV128_DIRECT and k % 128 != 127) >= 2
    assert len(vad.ENV128_BOUNCE_ONLY) >= 4 and not vad.s_full_of_rows(orc, "env128", vad.ENV128_BOUNCE_ONLY, 0).any() and (vad.s_full_of_rows(orc, "env128", vad.ENV128_BOUNCE_ONLY, vad.DEPTH) > 0).all()
    cols = {k % 128 for k in vad.ENV128}
    assert 0 in cols and 127 in cols


@pytest.mark.parametrize("leaf", [l for l in vad.LEAVES if vad.LEAVES[l][3] is not None])
def test_a_leaf_checked_in_part_has_dark_rows_among_the_unchecked(orc, leaf):
    """what the GPU test's exact-zero condition on unchecked rows rests on"""
    cand, dark = vad.dark_candidates(leaf), vad.dark_rows(orc, leaf)
    print("\n%-16s %d candidates, dark: %s" % (leaf, len(cand), dark))
    assert 0 < len(cand) <= vad.DARK_CANDIDATES and not set(cand) & set(vad.LEAVES[leaf][3]) and len(dark) >= 1


@pytest.mark.parametrize("leaf", ["diffuse5x3", "pv_roughness", "env16", "constants"])
def test_the_edge_terms_of_a_value_leaf_are_identically_zero(orc, records, leaf):
    """one entry of each kind of leaf (the first that the interior term lights): its primary-edge and secondary-edge columns are zero in every pixel, its interior column is not"""
    first = int(np.nonzero(records(leaf)["nonzero"][:, 0])[0][0])
    for term in ("interior", "primary", "secondary"):
        if leaf == "constants":
            const = vad.CONSTANTS[first]
            col = vad.constant_column(orc, vad.va.clear_tangents(vad.CONSTANT_SCENES[const[0]]()), const, 0, term)
        else:
            spec, where, rows, value, _ = vad.build_case(leaf)
            kind = vad.LEAVES[leaf][0]
            col = vad.one_hot_column(orc, spec, where, value, vad.columns_of(value, kind), rows[first], 0, term=term)
        assert col.shape == (vad.N, 3) and bool(col.any()) == (term == "interior"), (leaf, term)


@pytest.mark.parametrize("leaf", vad.ALL)
def test_compare_passes_on_the_oracle_itself_and_on_every_nudge(records, leaf):
    rec = records(leaf)
    row = vad.compare(rec["G"], rec)
    assert not row["failures"] and row["p50"] == 0.0 and row["worst"] == 0.0, (leaf, row)
    assert not row["unresolved"]
    for n, g in enumerate(rec["G_nudged"]):
        row = vad.compare(g, rec)
        assert not row["failures"], (leaf, n, row["failures"])


def _rel(rec):
    """|G| / S over the resolved entries (0 elsewhere)"""
    res = rec["resolved"]
    return np.where(res, np.abs(rec["G"]) / np.where(res, rec["S"], 1.0), 0.0)


def _keeps_the_sum(g, rec):
    """what a contraction with a constant tangent sees: unchanged by the damage"""
    return abs(g.sum() - rec["G"].sum()) < 1e-12 * np.abs(rec["G"]).sum()


def _fails(g, rec):
    return bool(vad.compare(g, rec)["failures"])


@pytest.mark.parametrize("leaf", [l for l in vad.ALL if _whole_map(l)])
def test_a_gradient_moved_inside_its_map_fails_and_keeps_its_sum(records, leaf):
    rec = records(leaf)
    W, A = rec["W"], _columns(rec)
    H = len(rec["vertices"]) // W
    G = rec["G"].reshape(H, W, A)
    for name, g in (("one texel along x", np.roll(G, 1, axis=1)), ("one texel along y", np.roll(G, 1, axis=0))):
        g = g.reshape(-1, A)
        assert _fails(g, rec) and _keeps_the_sum(g, rec), (leaf, name)
    k = int(np.argmax(_rel(rec).max(axis=1)))
    x, y = k % W, k // W
    lo, hi = (x - 1, x + 1) if 0 < x < W - 1 else ((x + 1, x + 2) if x == 0 else (x - 2, x - 1))      # the two x-neighbours of the largest texel
    if not 0 <= lo < hi < W:            # (a map two texels wide: the texel and its one neighbour)
        lo, hi = 0, 1
    g = G.copy()
    g[y, [lo, hi]] = g[y, [hi, lo]]
    assert _fails(g.reshape(-1, A), rec) and _keeps_the_sum(g.reshape(-1, A), rec), (leaf, "x-neighbours exchanged", x, y)
    if W != H:                                                   # W and H exchanged
        g = rec["G"].reshape(W, H, A).transpose(1, 0, 2).reshape(-1, A)
        assert _fails(g, rec) and _keeps_the_sum(g, rec), (leaf, "read as W x H")


@pytest.mark.parametrize("leaf", [l for l in vad.LEAVES if vad.LEAVES[l][0] == "pervertex"])
def test_two_vertices_rows_exchanged_fails(records, leaf):
    rec = records(leaf)
    order = np.argsort(-_rel(rec).max(axis=1), kind="stable")
    i, j = int(order[0]), int(order[1])
    assert rec["resolved"][i].any() and rec["resolved"][j].any()
    g = rec["G"].copy()
    g[[i, j]] = g[[j, i]]
    assert _fails(g, rec) and _keeps_the_sum(g, rec), (leaf, rec["vertices"][i], rec["vertices"][j])


ONE_CHANNEL = ("mf_roughness9x7", "cond_alpha7x6", "diel_alpha7x6", "pv_roughness")


@pytest.mark.parametrize("leaf", [l for l in vad.ALL if l not in ONE_CHANNEL])
def test_channels_exchanged_fails(records, leaf):
    """channels 0 and 2 of the largest row: a channel mix-up in one row"""
    rec = records(leaf)
    assert _columns(rec) == 3 and all(_columns(records(l)) == 1 for l in ONE_CHANNEL)
    if leaf == "constants":
        rel = np.where(rec["valid"].all(axis=1)[:, None], _rel(rec), 0.0)               # an RGB constant
    else:
        rel = _rel(rec)
    k = int(np.argmax(rel.max(axis=1)))
    g = rec["G"].copy()
    g[k, [0, 2]] = g[k, [2, 0]]
    assert _fails(g, rec) and _keeps_the_sum(g, rec), (leaf, rec["vertices"][k])


# A 1e-3 error on one row is below 16 x its own r on this leaf: a vertex of the ball lights one or two pixels, and the largest row's answer to a one-ulp nudge is r = 1.6e-4
# (|G| / S = 0.96), so its bound is 2.6e-3.  What the measure does not resolve there; the exchange of two rows and the zero entry still bite.
ONE_ROW_1E3_NOT_RESOLVED = {"pv_roughness"}


@pytest.mark.parametrize("leaf", vad.ALL)
def test_one_row_off_by_1e3_fails(records, leaf):
    """the row with the largest gradient (|G| / S is 1 up to rounding in most rows of these leaves: their columns have one sign) scaled by 1 + 1e-3"""
    rec = records(leaf)
    k = int(np.argmax(np.where(rec["resolved"], np.abs(rec["G"]), 0.0).max(axis=1)))
    g = rec["G"].copy()
    g[k] *= 1.0 + 1e-3
    print("\n%-16s row %s: |G| / S = %s, r = %s, Q50 = %.3g" % (leaf, rec["vertices"][k], _rel(rec)[k], rec["r"][k], rec["Q50"]))
    assert _fails(g, rec) == (leaf not in ONE_ROW_1E3_NOT_RESOLVED), (leaf, rec["vertices"][k])


# the leaves on which 16 x max(Q50, 4 * 2^-24) lies below 2e-4 x the median |G| / S: there a uniform error of 2e-4 must fail (the median condition); on the others the
# oracle's own one-ulp response is too large for the measure to resolve it (printed)
UNIFORM_2E4_RESOLVED = {
    "diffuse5x3", "mf_diffuse8x8", "mf_specular5x6", "mf_roughness9x7", "cond_eta4x5", "cond_k6x4", "cond_alpha7x6", "diel_alpha7x6", "normalmap16x16",
    "env16", "env16_xf", "env128", "constants",
}


@pytest.mark.parametrize("leaf", vad.ALL)
def test_a_uniform_2e4_error_fails(records, leaf):
    rec = records(leaf)
    bound, signal = lp.MARGIN * max(rec["Q50"], lp.ULP_FLOOR), 2e-4 * float(np.median(_rel(rec)[rec["resolved"]]))
    below = bound < signal
    print("\n%-16s 16 x max(Q50, floor) = %.3g, 2e-4 x median |G| / S = %.3g: %s" % (leaf, bound, signal, "resolved" if below else "NOT resolved"))
    assert below == (leaf in UNIFORM_2E4_RESOLVED), (leaf, bound, signal)
    if below:
        row = vad.compare(rec["G"] * (1.0 + 2e-4), rec)
        assert any("median" in f for f in row["failures"]), (leaf, row)


@pytest.mark.parametrize("leaf", vad.ALL)
def test_a_zero_entry_set_to_1e20_fails(records, leaf):
    """an entry whose column is identically zero in the oracle (a texel or vertex that no sample reaches; among the constants, a channel a scalar does not have)"""
    rec = records(leaf)
    dark = np.nonzero(~rec["nonzero"].any(axis=1))[0]
    if leaf == "constants":
        zero = np.argwhere(~rec["nonzero"])
    elif not len(dark):
        assert rec["nonzero"].all()                                  # a leaf lit in every checked entry has no such row
        return
    else:
        zero = np.array([[dark[len(dark) // 2], 0]])
    i, a = zero[len(zero) // 2]
    g = rec["G"].copy()
    assert g[i, a] == 0.0
    g[i, a] = 1e-20
    row = vad.compare(g, rec)
    assert len(row["failures"]) == 1 and "identically zero" in row["failures"][0], (leaf, row["failures"])
