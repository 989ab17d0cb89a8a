"""What tests/test_gpu_sensors.py takes for granted, asserted on the CPU oracle: in each three-sensor scene of tests/sensor_cases.py the sensors really see
different things (edge counts, images), every derivative term of every sensor is non-zero, a tangent on one camera reaches that camera's image alone, and a
sensor that is not in configure's active list has no primary edges.  If one of these stopped holding, a product that rendered Sensor[0] whatever the sensor id
could pass the GPU file; so they are assertions here, not comments there."""
import numpy as np
import pytest

import product
import sensor_cases as cases

TERMS = (1, 2, 4)          # interior, primary edges, secondary edges


@pytest.fixture(scope="module", params=cases.FAMILIES)
def family(request, orc):
    spec = cases.family_spec(request.param)
    return request.param, spec, orc.OracleScene(spec, [0, 1, 2])


def test_sensors_keep_different_primary_edges(family):
    name, spec, ref = family
    kept = [ref.num_primary_edges(k) for k in range(3)]
    assert min(kept) > 0 and len(set(kept)) == 3, (name, kept)


def test_sensors_see_different_images(family):
    name, spec, ref = family
    imgs = [ref.render_c(sensor=k, max_depth=cases.DEPTH, seed=7) for k in range(3)]
    for a in range(3):
        assert imgs[a].mean() > 0, (name, a)
        for b in range(3):
            if a != b:
                assert product.rel_l2(imgs[a], imgs[b]) > 0.1, (name, a, b)


def test_every_term_of_every_sensor_is_non_zero(family):
    name, spec, ref = family
    for k in range(3):
        for t in TERMS:
            _, d = ref.render_d(sensor=k, max_depth=cases.DEPTH, seeds=(5, 5, 5), terms=t)
            assert np.abs(d).max() > 0, (name, k, t)


@pytest.mark.parametrize("name", cases.FAMILIES)
def test_a_camera_tangent_reaches_its_own_sensor_only(orc, name):
    ref = orc.OracleScene(cases.camera_tangent_spec(name, 1), [0, 1, 2])
    for t in TERMS:
        assert np.abs(ref.render_d(sensor=0, max_depth=cases.DEPTH, seeds=(5, 5, 5), terms=t)[1]).max() == 0.0, (name, t)
        assert np.abs(ref.render_d(sensor=1, max_depth=cases.DEPTH, seeds=(5, 5, 5), terms=t)[1]).max() > 0, (name, t)


def test_an_inactive_sensor_has_no_primary_edges(family, orc):
    name, spec, ref = family
    only1 = orc.OracleScene(spec, [1])
    for k in (0, 2):
        assert only1.num_primary_edges(k) == 0
        assert np.abs(only1.render_d(sensor=k, max_depth=cases.DEPTH, seeds=(5, 5, 5), terms=2)[1]).max() == 0.0, (name, k)
    assert only1.num_primary_edges(1) == ref.num_primary_edges(1)
    # the active sensor does not notice: image and derivative are those of the scene with all three active, bit for bit
    a, b = only1.render_d(sensor=1, max_depth=cases.DEPTH, seeds=(5, 5, 5)), ref.render_d(sensor=1, max_depth=cases.DEPTH, seeds=(5, 5, 5))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # configure() with an empty list: no sensor keeps primary edges
    none = orc.OracleScene(spec, [])
    assert [none.num_primary_edges(k) for k in range(3)] == [0, 0, 0]


def test_guiding_grids_of_two_sensors_differ(orc):
    spec = cases.family_spec("cbox")
    ref = orc.OracleScene(spec, [0, 1, 2])
    reso = [40, 4, 4, 16]
    g0, g1 = ref.guiding_build(0, reso, nrounds=1, seed=5).mass(), ref.guiding_build(1, reso, nrounds=1, seed=5).mass()
    assert product.rel_l2(g1, g0) > 0.1
