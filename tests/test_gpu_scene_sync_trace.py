"""scene_sync step by step against a recorded run: tools/scene_sync_trace.py drives four small scenes through create, an unchanged configure, a colour, vertex moves, a
camera move, a tangent switched on and off, a transform, a scramble that calls for a new tree, bitmap changes, a refused update with the configure that re-sends
everything, and the tree scene once more under PSDR_HOST_GEOMETRY=1.  tests/golden/scene_sync_trace.json is what the commit BEFORE scene_sync was cut into steps
printed; every later state of csrc/hip/scene_build.hip has to print the same - tree built / refitted / kept, reallocations, bytes sent, edge path and bytes, hit counts -
with no word of the device's rows, edge arrays or tree differing from the host's."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "scene_sync_trace.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def trace():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")
    import psdr_jit_amd  # noqa: F401
    import scene_sync_trace
    return scene_sync_trace.run()


def _steps(rec):
    return [(name, st) for name, sc in sorted(rec.items()) for st in sc["steps"]]


def test_the_recorded_trace_takes_every_branch(golden):
    """so that the comparison below cannot pass vacuously"""
    steps = _steps(golden)
    trees = {st.get("tree") for _, st in steps}
    assert {"built", "refitted", "kept"} <= trees, trees
    assert {"device", "host"} <= {st.get("edge_path") for _, st in steps}
    assert any(st.get("reallocated", 0) > 0 for _, st in steps)
    # a lean update that ended in a built tree (PSDR_HIP_NEED_ROWS, then the rows and the build): the scramble of the environment-lit tree scene, whose configures are
    # lean (the device selected the edges of the step before it) - and without the device's rows, under PSDR_HOST_GEOMETRY, the same step builds too
    by = {st["step"]: st for st in golden["bvh_env"]["steps"]}
    assert by["transform_move"]["edge_path"] == "device" and by["transform_move"]["tree"] == "refitted"
    assert by["scramble"]["tree"] == "built"
    # a refused update, and the configure after it builds everything again
    assert by["malformed_update"]["refused"] and by["malformed_update"]["names_the_list"] and by["after_poison"]["tree"] == "built"
    # the brute-force box never has a tree to refit
    assert {st["tree"] for st in golden["cbox"]["steps"]} <= {"built", "kept"}
    for name, st in steps:
        for k in ("rows_mismatch", "edges_mismatch", "tree_violations"):
            assert st.get(k, 0) == 0, (name, st)
    for name in golden:
        assert golden[name]["hits"]["n_hit"] > 0, name


def test_every_step_does_what_the_recorded_run_did(trace, golden):
    assert sorted(trace) == sorted(golden)
    for name in sorted(golden):
        got, want = trace[name]["steps"], golden[name]["steps"]
        assert [st["step"] for st in got] == [st["step"] for st in want], name
        for g, w in zip(got, want):
            assert sorted(g) == sorted(w), (name, g, w)
            for k in sorted(w):
                assert g[k] == w[k], (name, w["step"], k, g[k], w[k])
            for k in ("rows_mismatch", "edges_mismatch", "tree_violations"):
                assert g.get(k, 0) == 0, (name, g)
        assert trace[name]["hits"] == golden[name]["hits"], name
