"""Reverse-mode gradients of the HIP kernels into value leaves - bitmap texels, per-vertex BSDF values, environment-map texels, BSDF and emitter constants - against the
oracle, texel by texel, vertex by vertex and channel by channel, through the public surface: what an optimiser reads from leaf.grad (tests/value_adjoint.py holds the measure
and its reasoning; DESIGN.md section 2 the measured table).

The other reverse-mode tests contract these gradients with a tangent that is constant over the map, or compare one random dot product with the kernels' own forward mode at
2e-3: the bilinear and the barycentric weights sum to one, so a scatter that lands in the wrong texel, vertex or channel passes them.  Here the leaf is a torch tensor handed to
the scene's own BSDF / emitter object, renderD is called once for the interior term, and per checked row k sum(img * w_k) is differentiated: leaf.grad, read in the leaf's own
shape, against the oracle's <w_k, J e_(k,a)>.  That covers the scatter sites of the adjoint kernels (adjoint_mat.h in the sweep form, adjoint.h in the probe form), the three
routes of the environment map's adjoint and the host's reshape of rows into leaves.  The bound is 16 x the oracle's own response to a one-ulp nudge (none calibrated on the kernels).
Each test prints its row of the table (pytest -s shows it)."""
import numpy as np
import pytest

import product
import value_adjoint as vad

pytestmark = pytest.mark.gpu

# (BSDF type of the spec, member of the spec) -> the attribute of the product's object that takes the leaf
BSDF_ATTR = {
    (0, "texture"): "reflectance", (0, "reflectance"): "reflectance",
    (1, "texture"): "diffuseReflectance", (1, "spec_texture"): "specularReflectance", (1, "rough_texture"): "roughness",
    (1, "reflectance"): "diffuseReflectance", (1, "specular"): "specularReflectance", (1, "roughness"): "roughness",
    (2, "texture"): "eta", (2, "spec_texture"): "k", (2, "rough_texture"): "alpha_u",
    (2, "alpha_u"): "alpha_u", (2, "alpha_v"): "alpha_v", (2, "eta"): "eta", (2, "k"): "k", (2, "specular"): "specular_reflectance",
    (3, "rough_texture"): "alpha_u", (3, "alpha_u"): "alpha_u", (3, "alpha_v"): "alpha_v", (3, "eta"): "eta",
    (4, "pv_specular"): "specularReflectance", (4, "pv_diffuse"): "diffuseReflectance", (4, "pv_roughness"): "roughness",
    (5, "texture"): "normal_map",
}
EMITTER_ATTR = {"env_data": "radiance", "radiance": "radiance"}


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
    """leaf -> (oracle record, the unchecked rows that are identically zero in the oracle), made once and left unchanged"""
    cache = {}

    def get(leaf):
        if leaf not in cache:
            cache[leaf] = (vad.reference(orc, leaf), () if leaf == "constants" else vad.dark_rows(orc, leaf))
        return cache[leaf]
    return get


def _target(sc, spec, where):
    """the scene's own object behind spec.<list>[index] and the name of the attribute that holds spec's member -> (object, attribute)"""
    lst, idx, member = where
    if lst == "emitters":
        return sc.param_map["Emitter[%d]" % idx], EMITTER_ATTR[member]
    b = spec.bsdfs[idx]
    return sc.param_map["BSDF[id=%s]" % (b.name or "bsdf%d" % idx)], BSDF_ATTR[getattr(b, "type", 0), member]


def _frame(psdr, sc):
    return psdr.PathTracer(vad.DEPTH).renderC(sc, 0, seed=vad.SEED)


def _scene_with_leaves(psdr, spec, leaves):
    """product.build_scene(spec) with torch leaves assigned the way an optimiser does (leaves: [(where, tensor)]); the two scenes render the same frame"""
    import torch
    plain = _frame(psdr, product.build_scene(spec))
    sc = product.build_scene(spec)
    for where, t in leaves:
        obj, attr = _target(sc, spec, where)
        setattr(obj, attr, t)
    sc.configure([0])
    assert torch.equal(_frame(psdr, sc), plain) and float(plain.abs().sum()) > 0
    return sc


def _render(psdr, orc, sc):
    img = psdr.PathTracer(vad.DEPTH).renderD(sc, 0, seed=vad.SEED, terms=orc.TERM_INTERIOR)
    assert tuple(img.shape) == (vad.N, 3)
    return img


def device_gradient(psdr, orc, rec, dark):
    """leaf.grad[row k] of sum(img * w_k) for every checked row k of an array leaf, read in the leaf's own shape -> [K, A]"""
    import torch
    value, W, kind = rec["value"], rec["W"], rec["kind"]
    leaf = torch.tensor(value).requires_grad_()
    assert tuple(leaf.shape) == value.shape
    sc = _scene_with_leaves(psdr, rec["spec"], [(rec["where"], leaf)])
    img = _render(psdr, orc, sc)
    A = rec["G"].shape[1]
    got = np.zeros((len(rec["vertices"]), A))
    for i, k in enumerate(rec["vertices"]):
        w = torch.from_numpy(rec["w"][i]).to(img.device)
        (g,) = torch.autograd.grad((img * w).sum(), leaf, retain_graph=True)
        assert tuple(g.shape) == value.shape
        g = g.double().cpu().numpy()
        entry = g[k] if kind == "pervertex" else g[k // W, k % W]          # [n, 3], [n], [H, W, 3], [H, W]
        got[i] = np.atleast_1d(entry)
        for z in dark:                                                       # an unchecked row that nothing reaches: exactly zero under every weight
            e = g[z] if kind == "pervertex" else g[z // W, z % W]
            assert not np.any(e), ("row %d is identically zero in the oracle" % z, e)
    return got


def device_gradient_of_constants(psdr, orc, rec):
    """the same for the rows of value_adjoint.CONSTANTS: per scene every listed constant is a leaf of one render -> [K, 3] (zero where a scalar has no channel)"""
    import torch
    got = np.zeros(rec["G"].shape)
    for key, spec in rec["specs"].items():
        mine = [(i, c) for i, c in enumerate(vad.CONSTANTS) if c[0] == key]
        leaves = []
        for i, (_, lst, idx, member, ncol) in mine:
            v = getattr(getattr(spec, lst)[idx], member)
            t = psdr.FloatD(float(v[0] if member == "eta" and ncol == 1 else v)).requires_grad_() if ncol == 1 else torch.tensor(np.asarray(v, np.float32)).requires_grad_()
            leaves.append(((lst, idx, member), t))
        sc = _scene_with_leaves(psdr, spec, leaves)
        img = _render(psdr, orc, sc)
        for (i, c), (_, t) in zip(mine, leaves):
            w = torch.from_numpy(rec["w"][i]).to(img.device)
            (g,) = torch.autograd.grad((img * w).sum(), t, retain_graph=True)
            assert tuple(g.shape) == tuple(t.shape) and g.numel() == c[4]
            got[i, :c[4]] = g.double().cpu().numpy().reshape(-1)
    return got


def _check(psdr, orc, records, leaf, label):
    rec, dark = records(leaf)
    got = device_gradient_of_constants(psdr, orc, rec) if leaf == "constants" else device_gradient(psdr, orc, rec, dark)
    row = vad.compare(got, rec)
    print()
    print(vad.HEADER)
    print(vad.format_row(label, row) + "   exactly zero on %d unchecked dark rows" % len(dark))
    assert not row["unresolved"]
    assert not row["failures"], row["failures"]


@pytest.mark.parametrize("leaf", vad.ALL)
def test_value_gradient_matches_oracle(psdr, orc, records, monkeypatch, leaf):
    monkeypatch.delenv("PSDR_ADJ_PROBE", raising=False)
    _check(psdr, orc, records, leaf, leaf)


@pytest.mark.parametrize("leaf", ["diffuse5x3", "pv_diffuse", "normalmap16x16", "env16", "env128"])
def test_value_gradient_matches_oracle_in_the_probe_form(psdr, orc, records, monkeypatch, leaf):
    """the record-and-probe form of the adjoint (PSDR_ADJ_PROBE is read per call): the scatter sites of adjoint.h"""
    monkeypatch.setenv("PSDR_ADJ_PROBE", "1")
    _check(psdr, orc, records, leaf, leaf + "/probe")
