"""Reverse-mode vertex gradients of the HIP kernels against the oracle, vertex by vertex and axis by axis, through the public surface: what an
optimiser reads from V.grad (tests/vertex_adjoint.py holds the measure and its reasoning; DESIGN.md section 2 the measured table).

The other reverse-mode tests take one dot product <w, J v> per case, v nearly always the rigid translation of a mesh: that multiplies the normal,
face-normal and area columns of the 22-wide triangle rows by zero and sums the position columns over the mesh, so an error in one triangle's
row, one vertex's fan, the vertex-normal chain or the area adjoint cancels or is never read.  Here mesh.vertex_positions = V is the leaf, renderD
is called term by term, and per checked vertex k sum(img * w_k).backward() gives V.grad[k], compared with the oracle's <w_k, J e_(k,a)>: the
reverse kernels, the chain rule from triangle / edge rows to vertices and vertex_positions itself.  w_k is zero on the pixels whose samples a
one-ulp nudge of the camera flips in the oracle, so the bound is 16 x the oracle's own response to that nudge (none calibrated on the kernels).
Each test prints its row of the table (pytest -s shows it)."""
import numpy as np
import pytest

import product
import vertex_adjoint as va

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def psdr():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists)")
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    return psdr_jit_amd


@pytest.fixture(scope="module")
def records(orc):
    """(family, term) -> (spec, leaf mesh, oracle record), made once and left unchanged"""
    cases, cache = {}, {}

    def get(family, term):
        if family not in cases:
            cases[family] = va.build_case(family)
        if (family, term) not in cache:
            spec, mesh, vertices = cases[family]
            cache[family, term] = (spec, mesh, va.reference(orc, spec, mesh, vertices, term))
        return cache[family, term]
    return get


def device_gradient(psdr, orc, spec, mesh_index, rec):
    """V.grad[k] of sum(img * w_k) for every checked vertex k of one term -> [K, 3]"""
    import torch
    sc = product.build_scene(spec)
    mesh = sc.param_map["Mesh[%d]" % mesh_index]
    V = torch.tensor(np.asarray(mesh._get("vertex_positions", False), np.float32).reshape(-1, 3)).requires_grad_()
    assert np.array_equal(V.detach().numpy(), np.asarray(spec.meshes[mesh_index].vertices, np.float32))
    mesh.vertex_positions = V
    sc.configure([0])
    img = psdr.PathTracer(va.DEPTH).renderD(sc, 0, seed=va.SEED[rec["term"]], terms=getattr(orc, "TERM_" + rec["term"].upper()))
    assert tuple(img.shape) == (va.N, 3)
    got = np.zeros((len(rec["vertices"]), 3))
    for i, k in enumerate(rec["vertices"]):
        w = torch.from_numpy(rec["w"][i]).to(img.device)
        (g,) = torch.autograd.grad((img * w).sum(), V, retain_graph=True)
        got[i] = g[k].double().cpu().numpy()
    return got


def _check(psdr, orc, records, family, term, label):
    spec, mesh, rec = records(family, term)
    row = va.compare(device_gradient(psdr, orc, spec, mesh, rec), rec)
    print()
    print(va.HEADER)
    print(va.format_row(label, row))
    for k, a, g, G, share in row["unresolved"]:
        print("    unresolved: vertex %d axis %d  device %.6g  oracle (settled pixels) %.6g  kept share %.2f" % (k, a, g, G, share))
    assert not row["failures"], row["failures"]


CASES = [(family, term) for family in va.FAMILIES for term in va.terms_of(family)]


@pytest.mark.parametrize("family,term", CASES)
def test_vertex_gradient_matches_oracle(psdr, orc, records, monkeypatch, family, term):
    monkeypatch.delenv("PSDR_ADJ_PROBE", raising=False)
    _check(psdr, orc, records, family, term, family)


@pytest.mark.parametrize("term", va.TERMS)
@pytest.mark.parametrize("family", ["cbox", "sphere"])
def test_vertex_gradient_matches_oracle_in_the_probe_form(psdr, orc, records, monkeypatch, family, term):
    """the record-and-probe form of the adjoint (PSDR_ADJ_PROBE is read per call)"""
    monkeypatch.setenv("PSDR_ADJ_PROBE", "1")
    _check(psdr, orc, records, family, term, family + "/probe")
