"""The multi-scale image loss, what can be checked without a GPU: the four entry points are declared, exported and listed and the ABI did not move; they refuse bad
arguments before they touch a device; the float64 checker (tests/msloss_ref.py, which tests/test_gpu_msloss.py compares the kernels against) has a gradient that
equals central differences of its own loss and a pyramid that equals torch's avg_pool2d form; pyramid_shapes counts right."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import msloss_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("psdr_hip_msloss_create", "psdr_hip_msloss_eval", "psdr_hip_msloss_level", "psdr_hip_msloss_destroy")
SHAPES_37_19 = [(37, 19), (19, 10), (10, 5), (5, 3), (3, 2), (2, 1), (1, 1)]


@pytest.fixture(scope="module")
def psdr():
    import __graft_entry__
    __graft_entry__.build()
    import psdr_jit_amd
    return psdr_jit_amd


def test_entry_points_declared_exported_listed(psdr):
    from psdr_jit_amd import build, cabi
    with open(os.path.join(ROOT, "include", "psdr_hip.h")) as fh:
        text = fh.read()
    L = cabi.lib()
    for name in NEW:
        assert re.search(r"^int\s+%s\s*\(" % name, text, re.M), "%s is not declared in include/psdr_hip.h" % name
        assert hasattr(L, name), "libpsdr_hip.so does not export %s" % name
        assert name in cabi.SYMBOLS
        assert getattr(L, name).argtypes is not None, "%s has no argtypes" % name
    assert re.search(r"#define\s+PSDR_HIP_ABI_VERSION\s+16\b", text)
    assert L.psdr_hip_abi_version() == 16
    for name in ("MultiScaleLoss", "pyramid_shapes"):
        assert hasattr(psdr, name)
    units = {u[0]: u for u in build.hip_units()}
    assert units["msloss"][1].endswith("msloss.hip")
    deps = {os.path.relpath(d, ROOT) for d in units["msloss"][3]}
    assert {os.path.join("include", "psdr_hip.h"), os.path.join("psdr_jit_amd", "csrc", "hip", "op_common.h"), os.path.join("psdr_jit_amd", "isa_lint.py")} <= deps
    # the stream contract names the handle: rule 3 (creates) and rule 5 (handles that own work frames)
    assert re.search(r"\*\s+3\. Every psdr_hip_\*_create \([^)]*msloss[^)]*\)", text)
    assert re.search(r"\*\s+5\. [^\n]*msloss handle owns work frames", text)


def test_every_entry_point_refuses_bad_arguments_before_any_device_call(psdr):
    """no GPU is visible here: a call that reached the device would fail with a HIP error, not with the entry point's own message.  The non-NULL device pointers are host
    addresses that a refused call never reads, and so is the handle; a weight_channels of 2 .. 4 other than C and a level outside [0, L) are compared with the handle's
    own numbers, which only a real handle has: tests/test_gpu_msloss.py refuses those."""
    from psdr_jit_amd import cabi
    L = cabi.lib()
    host = np.zeros(64, dtype=np.int64)
    p, p2, p3, p4, p5 = (host.ctypes.data + 64 * i for i in range(5))
    lam = (C.c_float * 16)(*([1.0] * 16))

    def refused(rc, name, word):
        msg = L.psdr_hip_last_error().decode()
        assert rc != 0 and msg.startswith(name + ":") and word in msg and "hip" not in msg[len(name):].lower(), (name, word, rc, msg)

    name = "psdr_hip_msloss_create"
    h = C.c_void_p()
    refused(L.psdr_hip_msloss_create(16, 16, 5, 3, None, None), name, "NULL")
    for W, H in ((0, 16), (16, 0), (-3, 16), (16, -1), (16385, 1), (1, 16385), (4097, 4096), (1 << 30, 1 << 30)):
        refused(L.psdr_hip_msloss_create(W, H, 1, 3, C.byref(h), None), name, "%d x %d" % (W, H))
    for Cn in (0, -1, 5):
        refused(L.psdr_hip_msloss_create(16, 16, 5, Cn, C.byref(h), None), name, "C = %d" % Cn)
    for W, H, Lv in ((16, 16, 0), (16, 16, -1), (16, 16, 6), (37, 19, 8), (1, 1, 2), (9, 1, 6)):          # full depth: 5, 7, 1, 5
        refused(L.psdr_hip_msloss_create(W, H, Lv, 3, C.byref(h), None), name, "levels = %d" % Lv)
    assert not h.value                                        # a refused create leaves no handle behind

    fake = C.c_void_p(p5)                                     # (a refused call never looks into the handle)
    name = "psdr_hip_msloss_eval"
    fn = L.psdr_hip_msloss_eval
    refused(fn(None, p, p2, None, 0, 0, lam, p3, p4, None), name, "handle is NULL")
    refused(fn(fake, None, p2, None, 0, 0, lam, p3, p4, None), name, "NULL")
    refused(fn(fake, p, None, None, 0, 0, lam, p3, p4, None), name, "NULL")
    refused(fn(fake, p, p2, None, 0, 0, lam, None, p4, None), name, "NULL")
    for norm in (2, -1, 7):
        refused(fn(fake, p, p2, None, 0, norm, lam, p3, p4, None), name, "norm = %d" % norm)
    for wc in (-1, 5, 64):
        refused(fn(fake, p, p2, p3, wc, 0, lam, p3, p4, None), name, "weight_channels = %d" % wc)
    refused(fn(fake, p, p2, None, 1, 0, lam, p3, p4, None), name, "weight is NULL")

    name = "psdr_hip_msloss_level"
    refused(L.psdr_hip_msloss_level(None, 0, p, None), name, "handle is NULL")
    refused(L.psdr_hip_msloss_level(fake, 0, None, None), name, "out is NULL")
    refused(L.psdr_hip_msloss_destroy(None), "psdr_hip_msloss_destroy", "handle is NULL")
    assert not host.any()


def _inputs(rng, W, H, Cn):
    n = W * H
    return rng.standard_normal((n, Cn)), rng.standard_normal((n, Cn)), 0.5 + rng.random((n, 1)), 0.5 + rng.random((n, Cn))


@pytest.mark.parametrize("norm", ["l1", "l2"])
def test_checker_gradient_equals_central_differences(norm):
    """float64 throughout.  l2 is quadratic, so a central difference is exact up to rounding; l1 is piecewise linear, so it is exact as long as no d_l changes sign
    within +-h: with h = 1e-7 and |d_l| > 1e-5 everywhere (asserted) none does."""
    rng = np.random.default_rng(3)
    for (W, H, Cn, levels, lam) in ((7, 5, 2, None, None), (9, 1, 1, None, None), (6, 11, 3, 3, (1.0, 0.5, 2.0)), (5, 4, 4, None, (1.0, 0.0, 0.25, 3.0))):
        img, tgt, w1, wc = _inputs(rng, W, H, Cn)
        for weight in (None, w1, wc):
            loss, ll, grad, pyr = ref.evaluate(img, tgt, W, H, norm, weight, levels, lam)
            assert len(pyr) == len(ref.shapes(W, H, levels)) == len(ll)
            assert min(np.abs(d).min() for d in pyr) > 1e-5
            h = 1e-7 if norm == "l1" else 1e-4
            fd = np.zeros_like(img)
            for k in range(img.size):
                e = np.zeros(img.size)
                e[k] = h
                e = e.reshape(img.shape)
                fd.flat[k] = (ref.evaluate(img + e, tgt, W, H, norm, weight, levels, lam)[0] - ref.evaluate(img - e, tgt, W, H, norm, weight, levels, lam)[0]) / (2 * h)
            assert np.abs(fd - grad).max() <= 1e-8 * max(1.0, np.abs(grad).max()), (W, H, Cn, norm)
            # the target's gradient is the negative: the loss depends on img - target only
            assert ref.evaluate(img + 0.25, tgt + 0.25, W, H, norm, weight, levels, lam)[0] == pytest.approx(loss, rel=1e-13)


def test_checker_l1_gradient_is_zero_where_the_residual_is():
    img = np.array([[1.0], [2.0], [3.0], [5.0]])
    tgt = np.array([[1.0], [2.0], [4.0], [4.0]])          # d_0 = 0, 0, -1, 1; d_1 = 0, 0 (2 x 2 -> 1 x 1 has d_1 = 0)
    loss, ll, grad, pyr = ref.evaluate(img, tgt, 2, 2, "l1")
    assert pyr[1].tolist() == [[0.0]] and ll.tolist() == [0.5, 0.0] and loss == 0.5
    assert grad.reshape(-1).tolist() == [0.0, 0.0, -0.25, 0.25]


@pytest.mark.parametrize("shape", [(37, 19), (33, 33), (70, 45), (9, 1), (1, 1), (64, 96)])
def test_checker_pyramid_equals_avg_pool2d(shape):
    import torch
    import torch.nn.functional as F
    W, H = shape
    rng = np.random.default_rng(4)
    img, tgt, w1, wc = _inputs(rng, W, H, 3)
    for weight in (None, w1, wc):
        pyr = ref.pyramid(img, tgt, W, H, weight)
        assert [(d.shape[0]) for d in pyr] == [w * h for w, h in ref.shapes(W, H)]
        x = torch.from_numpy(((1.0 if weight is None else weight) * (img - tgt)).reshape(H, W, 3)).permute(2, 0, 1)[None]
        for l, d in enumerate(pyr):
            assert np.abs(x[0].permute(1, 2, 0).reshape(-1, 3).numpy() - d).max() <= 1e-14, (shape, l)
            if l + 1 < len(pyr):
                x = F.avg_pool2d(x, 2, ceil_mode=True, count_include_pad=False)
        assert tuple(x.shape[2:]) == (1, 1)


def test_pyramid_shapes(psdr):
    assert psdr.pyramid_shapes(37, 19) == SHAPES_37_19 == ref.shapes(37, 19)
    assert psdr.pyramid_shapes(37, 19, levels=3) == SHAPES_37_19[:3]
    assert psdr.pyramid_shapes(1, 1) == [(1, 1)] and psdr.pyramid_shapes(9, 1) == [(9, 1), (5, 1), (3, 1), (2, 1), (1, 1)]
    assert len(psdr.pyramid_shapes(257, 130)) == 10 and psdr.pyramid_shapes(257, 130)[5] == (9, 5)
    assert len(psdr.pyramid_shapes(512, 512)) == 10 and len(psdr.pyramid_shapes(2048, 2048)) == 12
    for bad in (dict(width=0, height=4), dict(width=4, height=-1), dict(width=37, height=19, levels=8), dict(width=37, height=19, levels=0), dict(width=4, height=4, levels=1.5)):
        with pytest.raises(ValueError):
            psdr.pyramid_shapes(**bad)
    # the constructor refuses wrong arguments before it looks for a device
    for kw in (dict(norm="huber"), dict(channels=5), dict(channels=0), dict(levels=8), dict(level_weights=(1.0, 2.0)), dict(level_weights=[float("nan")] * 7)):
        with pytest.raises(ValueError):
            psdr.MultiScaleLoss(37, 19, **kw)
    with pytest.raises(ValueError):
        psdr.MultiScaleLoss(0, 19)
    with pytest.raises(ValueError):
        psdr.MultiScaleLoss(4097, 4096)
