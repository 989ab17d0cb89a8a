"""Per-sample parity of the HIP kernels with the oracle: radiance and forward derivatives, row by row, on every scene family
(tests/lane_parity.py holds the measure and its reasoning; DESIGN.md section 2 the measured table).

The image-level gate of the other parity tests (rel-L2 < 1e-3) stands four orders of magnitude above what the kernels do; a
systematic 1e-4 error in one material's lobe, a reciprocal that lost accuracy or a MIS weight that is wrong on a rare branch pass
it.  Here every family's 128 x 128 frame at spp = sppe = sppse = 1 is compared sample by sample: the general path kernel through
psdr_hip_li_lanes, the lean production kernels through render_d_fwd, term by term.

Bounds (none calibrated on the kernels): at most 2 % of an output's rows differ by more than 1e-3 of the row's magnitude - the
oracle's own share of rows that a one-ulp nudge of the camera flips is at most 1 % (test_lane_parity_cpu.py) - and over the other
non-zero rows the 50th / 99th percentile of the relative error is at most 16 x max(Q_q, 4 * 2^-24), Q_q the same percentile of the
oracle's response to that nudge; for lanes / img / d_int the median bound holds again within the rows of every first-hit BSDF that
lights 64 rows or more (one material's lobe is a per cent of a frame, below what the first two conditions resolve).  An output that
is identically zero in the oracle is identically zero here.
Each test prints its row of the table (pytest -s shows it)."""
import ctypes as C

import numpy as np
import pytest

import lane_parity as lp
import product

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


def device_outputs(psdr, orc, spec):
    """The five outputs of lane_parity.oracle_outputs on the device"""
    import torch
    from psdr_jit_amd import cabi
    sc = product.build_scene(spec)
    lanes = torch.empty((lp.N, 3), dtype=torch.float32, device="cuda")
    a = cabi.make_args(max_depth=lp.DEPTH, seeds=(lp.SEED, 0, 0))
    cabi.check(cabi.lib().psdr_hip_li_lanes(sc._hip_handle(), C.byref(a), 0, lp.N, lanes.data_ptr(), None))
    out = {"lanes": lanes.cpu().numpy()}
    integ = psdr.PathTracer(lp.DEPTH)
    img, d = psdr.render_d_fwd(integ, sc, 0, seed=lp.SEED, terms=orc.TERM_INTERIOR)
    out["img"], out["d_int"] = img.cpu().numpy(), d.cpu().numpy()
    for name, term in (("d_prim", orc.TERM_PRIMARY), ("d_sec", orc.TERM_SECONDARY)):
        img, d = psdr.render_d_fwd(integ, sc, 0, seed=lp.SEED, terms=term)
        assert float(img.abs().max()) == 0.0                # an edge term has no primal
        out[name] = d.cpu().numpy()
    return out


@pytest.fixture(scope="module")
def family_data(psdr, orc):
    """family -> (oracle record, device outputs), both made once and left unchanged"""
    cache = {}

    def get(family):
        if family not in cache:
            spec = lp.build_spec(family)
            cache[family] = (lp.reference(orc, spec), device_outputs(psdr, orc, spec))
        return cache[family]
    return get


@pytest.mark.parametrize("output", lp.OUTPUTS)
@pytest.mark.parametrize("family", list(lp.FAMILIES))
def test_rows_match_oracle(family_data, family, output):
    rec, got = family_data(family)
    assert got[output].shape == (lp.N, 3)
    res = lp.compare({output: got[output]}, rec, outputs=(output,))
    print()
    print(lp.HEADER)
    print("\n".join(lp.format_rows(family, res)))
    assert not res[output]["failures"], res[output]["failures"]
