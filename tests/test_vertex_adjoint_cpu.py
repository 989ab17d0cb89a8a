"""The oracle's side of the per-vertex measure of reverse mode (tests/vertex_adjoint.py), without a GPU: the oracle resolves
enough entries of every family and term for the GPU test to mean something (so that test cannot hide a failure in what it leaves out), and the
comparison has teeth - the oracle's own gradients, damaged in ways that one dot product with a translation lets through, fail compare."""
import numpy as np
import pytest

import lane_parity as lp
import vertex_adjoint as va

MIN_RESOLVED = 6


@pytest.fixture(scope="module")
def records(orc):
    """family -> {term: record}, every term (the left-out ones too), made once and left unchanged"""
    cache = {}

    def get(family):
        if family not in cache:
            spec, mesh, vertices = va.build_case(family)
            cache[family] = {term: va.reference(orc, spec, mesh, vertices, term) for term in va.TERMS}
        return cache[family]
    return get


def _meets_conditions(rec):
    nz, res = int(rec["nonzero"].sum()), int(rec["resolved"].sum())
    if nz == 0:
        return True
    share_ok = res == nz if rec["term"] == "interior" else 2 * res >= nz
    return share_ok and res >= MIN_RESOLVED


@pytest.mark.parametrize("family", list(va.FAMILIES))
def test_oracle_resolves_enough_entries(records, family):
    recs = records(family)
    print()
    print(va.ORACLE_HEADER)
    for term in va.TERMS:
        print(va.format_oracle_row(family, recs[term]) + ("   (left out)" if (family, term) in va.LEFT_OUT else ""))
    assert recs["interior"]["nonzero"].any()
    for term in va.terms_of(family):
        rec = recs[term]
        nz, res = int(rec["nonzero"].sum()), int(rec["resolved"].sum())
        if nz == 0:                                              # an identically zero term: zero under every nudge as well
            assert not rec["G"].any() and not rec["G_nudged"].any(), (family, term)
            continue
        if term == "interior":
            assert res == nz, (family, term, res, nz)            # every non-zero entry
        else:
            assert 2 * res >= nz, (family, term, res, nz)        # at least half of them
        assert res >= MIN_RESOLVED, (family, term, res)
        assert (rec["S"][rec["resolved"]] > 0).all() and np.isfinite(rec["r"]).all()
    for term in va.TERMS:                                        # a term is left out because it does not meet them, and for no other reason
        if (family, term) in va.LEFT_OUT:
            assert term != "interior" and not _meets_conditions(recs[term]), (family, term)


@pytest.mark.parametrize("family", [f for f, case in va.FAMILIES.items() if case[3] is not None and len(case[3]) == 16])
def test_the_subset_of_a_large_mesh_is_seen_by_the_interior_term(records, family):
    rec = records(family)["interior"]
    assert len(rec["vertices"]) == 16 and rec["vertices"] == tuple(sorted(set(rec["vertices"])))
    assert (rec["S_full"] > 0).any(axis=1).all(), [k for k, s in zip(rec["vertices"], rec["S_full"]) if not (s > 0).any()]


@pytest.mark.parametrize("family", list(va.FAMILIES))
def test_compare_passes_on_the_oracle_itself_and_on_every_nudge(records, family):
    for term in va.terms_of(family):
        rec = records(family)[term]
        row = va.compare(rec["G"], rec)
        assert not row["failures"] and row["p50"] == 0.0 and row["worst"] == 0.0, (family, term, row)
        assert row["entries"] - row["resolved"] == len(row["unresolved"])
        for n, g in enumerate(rec["G_nudged"]):
            row = va.compare(g, rec)
            assert not row["failures"], (family, term, n, row["failures"])


def _rel(rec):
    """|G| / S over the resolved entries (0 elsewhere)"""
    res = rec["resolved"]
    return np.where(res, np.abs(rec["G"]) / np.where(res, rec["S"], 1.0), 0.0)


def _lit_terms(records, family):
    return [(term, records(family)[term]) for term in va.terms_of(family) if records(family)[term]["resolved"].any()]


# A 1e-3 error on one vertex is below 16 x its own r in these terms: what the measure does not resolve there
ONE_VERTEX_1E3_NOT_RESOLVED = {("cbox", "interior"), ("dielectric", "primary"), ("pervertex", "interior")}


@pytest.mark.parametrize("family", list(va.FAMILIES))
def test_one_vertex_off_by_1e3_fails(records, family):
    """the three entries of the vertex with the largest |G| / S scaled by 1 + 1e-3, term by term: every term but the three listed above fails (in every family
    the largest |G| / S, 1 up to rounding, is reached in an edge term that does)"""
    lit = _lit_terms(records, family)
    bites = {}
    for term, rec in lit:
        k = int(np.argmax(_rel(rec).max(axis=1)))
        g = rec["G"].copy()
        g[k] *= 1.0 + 1e-3
        row = va.compare(g, rec)
        bites[term] = bool(row["failures"])
    assert any(bites.values()), family
    for term, _ in lit:
        assert bites[term] == ((family, term) not in ONE_VERTEX_1E3_NOT_RESOLVED), (family, term, bites[term])


@pytest.mark.parametrize("family", list(va.FAMILIES))
def test_two_vertices_rows_exchanged_fails(records, family):
    """the gradients of the two vertices with the largest |G| / S exchanged: what a fan or an index gone wrong does, and what a translation sums away"""
    for term, rec in _lit_terms(records, family):
        order = np.argsort(-_rel(rec).max(axis=1), kind="stable")
        i, j = int(order[0]), int(order[1])
        assert rec["resolved"][i].any() and rec["resolved"][j].any(), (family, term)
        g = rec["G"].copy()
        g[[i, j]] = g[[j, i]]
        assert va.compare(g, rec)["failures"], (family, term, rec["vertices"][i], rec["vertices"][j])


# the terms in which 16 x max(Q50, 4 * 2^-24) lies below 2e-4 x the median |G| / S: there a uniform error of 2e-4 must fail (the median condition);
# in the others the oracle's own one-ulp response is too large for the measure to resolve it
UNIFORM_2E4_RESOLVED = {
    ("cbox", "interior"), ("cbox", "primary"), ("cbox", "secondary"), ("sphere", "interior"), ("sphere", "secondary"),
    ("microfacet2s", "primary"), ("microfacet2s", "secondary"), ("dielectric", "secondary"),
    ("envmap_area", "interior"), ("envmap_area", "primary"), ("envmap_area", "secondary"), ("normalmap", "interior"), ("normalmap", "secondary"),
    ("pervertex", "primary"), ("pervertex", "secondary"), ("ortho", "interior"), ("ortho", "primary"),
}


@pytest.mark.parametrize("family", list(va.FAMILIES))
def test_a_uniform_2e4_error_fails(records, family):
    for term, rec in _lit_terms(records, family):
        below = lp.MARGIN * max(rec["Q50"], lp.ULP_FLOOR) < 2e-4 * float(np.median(_rel(rec)[rec["resolved"]]))
        assert below == ((family, term) in UNIFORM_2E4_RESOLVED), (family, term, rec["Q50"])
        if below:
            row = va.compare(rec["G"] * (1.0 + 2e-4), rec)
            assert any("median" in f for f in row["failures"]), (family, term, row)
    assert any(f == family for f, _ in UNIFORM_2E4_RESOLVED)        # every family has such a term


@pytest.mark.parametrize("family", list(va.FAMILIES))
def test_a_zero_entry_set_to_1e20_fails(records, family):
    """an entry whose column is identically zero in the oracle (a vertex that no sample of the term reaches) must be exactly zero"""
    seen = 0
    for term in va.terms_of(family):
        rec = records(family)[term]
        zero = np.argwhere(~rec["nonzero"])
        if not len(zero):
            continue
        seen += 1
        i, a = zero[len(zero) // 2]
        g = rec["G"].copy()
        assert g[i, a] == 0.0
        g[i, a] = 1e-20
        row = va.compare(g, rec)
        assert len(row["failures"]) == 1 and "identically zero" in row["failures"][0], (family, term, row["failures"])
    assert seen, family


def test_tangents_are_cleared_and_the_spec_is_left_alone(orc):
    """reference() renders the one-hot columns alone: the moving mesh's own tangent is gone, and the spec handed in is not changed"""
    import scenes
    spec = scenes.cbox_scene(va.RES, va.RES, va.SPP, va.SPP, va.SPP, param="box_x")
    plain, mesh, vertices = va.build_case("cbox")
    a = va.reference(orc, spec, 1, vertices[1:2], "primary")
    b = va.reference(orc, plain, mesh, vertices[1:2], "primary")
    assert np.array_equal(a["G"], b["G"]) and a["nonzero"].any()
    assert spec.meshes[1].d_to_world_left[0, 3] == 100.0 and spec.meshes[1].d_vertices is None and plain.meshes[mesh].d_vertices is None
