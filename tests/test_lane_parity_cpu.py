"""The oracle's side of the per-sample parity measure (tests/lane_parity.py), without a GPU:
the inputs stay honest (every family's unsettled share is at most half of the device's cap, and the one-ulp nudge moves the samples),
and the classifier has teeth (the oracle's own frames, damaged in the ways the image-level 1e-3 gate lets through, fail compare)."""
import numpy as np
import pytest

import lane_parity as lp


@pytest.fixture(scope="module")
def records(orc):
    cache = {}

    def get(family):
        if family not in cache:
            spec = lp.build_spec(family)
            cache[family] = (spec, lp.reference(orc, spec, keep_nudges=True))
        return cache[family]
    return get


@pytest.mark.parametrize("family", list(lp.FAMILIES))
def test_oracle_stays_inside_half_the_cap(records, family):
    spec, rec = records(family)
    print()
    print("%-13s %-7s %10s %8s %8s %10s %10s" % ("family", "output", "unsettled%", "moved%", "(all)%", "Q50", "Q99"))
    for name in lp.OUTPUTS:
        o = rec["out"][name]
        print("%-13s %-7s %10.3f %8.1f %8.1f %10.2e %10.2e" % (family, name, 100 * o["unsettled_share"], 100 * o["moved"], 100 * o["moved_all"], o["Q"][50], o["Q"][99]))
    for name in lp.OUTPUTS:
        o = rec["out"][name]
        assert o["unsettled_share"] <= lp.UNSETTLED_CAP, (family, name, o["unsettled_share"])
    # the nudge is not inert: it changes at least half of the lit samples (of those whose camera ray meets a surface - a sample that looks straight
    # into the environment map depends on the ray's direction alone, and moving the camera cannot change it; "(all)" prints the share without that)
    for name in ("lanes", "d_int"):
        o = rec["out"][name]
        assert o["nonzero"].any() and o["moved"] >= 0.5, (family, name, o["moved"])
    assert rec["out"]["img"]["nonzero"].any()


@pytest.mark.parametrize("family", list(lp.FAMILIES))
def test_compare_passes_on_the_oracle_itself_and_on_every_nudge(records, family):
    spec, rec = records(family)
    base = {name: rec["out"][name]["base"] for name in lp.OUTPUTS}
    res = lp.compare(base, rec)
    assert not lp.failures(res), lp.failures(res)
    assert all(r["left_out"] == 0.0 and r["p99"] == 0.0 for r in res.values())
    for k, frame in enumerate(rec["nudges"]):
        res = lp.compare(frame, rec)
        assert not lp.failures(res), (k, lp.failures(res))


def _lit_outputs(rec):
    return [name for name in lp.OUTPUTS if rec["out"][name]["nonzero"].any()]


@pytest.mark.parametrize("family", ["cbox", "conductor", "envmap_balls", "ortho"])
def test_a_uniform_2e4_error_fails(records, family):
    """every lit row of one output scaled by 1 + 2e-4: invisible to a 1e-3 image gate, and no row is left out - the percentiles catch it"""
    spec, rec = records(family)
    for name in _lit_outputs(rec):
        bad = {name: rec["out"][name]["base"] * np.float32(1.0 + 2e-4)}
        res = lp.compare(bad, rec)
        assert res[name]["failures"], (family, name)
        assert res[name]["left_out"] == 0.0 and any("p50" in f for f in res[name]["failures"])


LOBES = [("conductor", "gold"), ("conductor", "copper"), ("dielectric", "glass"), ("dielectric", "frosted"), ("pervertex", "pv"), ("microfacet2s", "cat"),
         ("microfacet2s", "white"), ("textured_ggx", "tex"), ("normalmap", "tex"), ("ortho", "cat"), ("envmap_balls", "cat")]


@pytest.mark.parametrize("scale", [1e-3, 2e-4])
@pytest.mark.parametrize("family,bsdf_name", LOBES)
def test_one_materials_lobe_off_fails(orc, records, family, bsdf_name, scale):
    """the rows whose first hit carries one chosen BSDF scaled by 1 + 1e-3, and by the 1 + 2e-4 of the uniform case: every GGX material of the families, the NormalMap, the
    bitmaps, two diffuse ones.  The small boxes light 100-200 of the 16384 rows at one sample per pixel: conditions 1 and 2 pass such a frame (asserted
    for the gold box below), the per-BSDF median of condition 3 does not."""
    spec, rec = records(family)
    bid = [b.name for b in spec.bsdfs].index(bsdf_name)
    rows = rec["first_hit"] == bid
    for name in ("lanes", "img"):
        o = rec["out"][name]
        assert bid in o["lobes"] and (rows & o["nonzero"]).sum() >= lp.LOBE_ROWS, (family, name, int((rows & o["nonzero"]).sum()))
        g = o["base"].copy()
        g[rows] *= np.float32(1.0 + scale)
        res = lp.compare({name: g}, rec)
        assert any(repr(bsdf_name) in f for f in res[name]["failures"]), (family, name, res[name])
    if (family, bsdf_name, scale) == ("conductor", "gold", 1e-3):
        assert len(res["img"]["failures"]) == 1 and 0 < res["img"]["left_out"] < lp.LEFT_OUT_CAP          # only the lobe's own condition speaks


@pytest.mark.parametrize("family", ["cbox", "sphere", "config5_l3"])
def test_three_per_cent_of_the_rows_wrong_fails(records, family):
    """3 % of the rows replaced by other rows' values: a branch taken by few samples gone wrong - the cap catches it"""
    spec, rec = records(family)
    rng = np.random.default_rng(7)
    for name in _lit_outputs(rec):
        o = rec["out"][name]
        lit = np.flatnonzero(o["nonzero"])
        if len(lit) < 0.2 * lp.N:                   # (an edge term lights few pixels: 3 % of all rows cannot be taken from them)
            continue
        dst = rng.choice(lit, size=int(0.03 * lp.N), replace=False)
        src = np.roll(dst, 1)
        g = o["base"].copy()
        g[dst] = o["base"][src] * np.float32(1.5)
        res = lp.compare({name: g}, rec)
        assert any("cap" in f for f in res[name]["failures"]), (family, name, res[name])


def test_a_zero_edge_output_with_one_lit_pixel_fails(records):
    """conductor / alpha: a material parameter moves no edge, both edge outputs are identically zero - one non-zero pixel is an error"""
    spec, rec = records("conductor")
    for name in ("d_prim", "d_sec"):
        o = rec["out"][name]
        assert not o["nonzero"].any()
        g = np.zeros_like(o["base"])
        assert not lp.compare({name: g}, rec)[name]["failures"]
        g[4321, 1] = 1e-20
        assert lp.compare({name: g}, rec)[name]["failures"]


def test_nudge_is_one_ulp_of_the_scene_extent(orc):
    """the orthographic camera sits at x = y = 0, where one ulp of its own coordinate is a denormal: delta follows the scene's extent"""
    spec = lp.build_spec("ortho")
    delta = lp.rounding_delta(orc.OracleScene(spec, [0]), spec)
    assert delta == np.spacing(np.float32(5.0))
    moved = [np.asarray(lp.nudged(spec, k, delta).cameras[0].to_world_raw)[:3, 3] - np.asarray(spec.cameras[0].to_world_raw)[:3, 3] for k in range(8)]
    assert len({tuple(np.sign(m)) for m in moved}) == 8 and all(np.all(np.abs(m[:2]) == delta) for m in moved)
    assert np.array_equal(np.asarray(spec.cameras[0].to_world_raw)[:3, 3], np.float32([0.0, 0.0, -5.0]))       # the spec handed in is not changed
