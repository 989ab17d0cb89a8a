"""The frames tests/test_gpu_group_start.py renders with grouped starts of the interior term's waves (paths.h GROUPED STARTS) and, in a fresh child process that runs this
file with PSDR_GROUP_START=0, lane by lane - the schedule before the threshold.  Small frames of the Cornell box at the sizes where the start bookkeeping can go wrong.

    python tests/group_start_cases.py OUT.npz       renders every case, writes {"<case>/c": [n, 3] renderC, "<case>/d": [2, n, 3] renderD (image, derivative)}
"""
import ctypes as C
import os
import sys

import numpy as np

if __name__ == "__main__":          # (run as a script: the repository root is not on the path yet)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import product                      # noqa: E402
import scenes                       # noqa: E402

SEEDS = (41, 42, 43)
FAR_Z = -2600.0                     # the README camera stands at z = -800 and sees the box in 36 % of its pixels


def frame_spec(name):
    """the scenes: (width, height, spp) of the README box, parameter = the small box's x"""
    if name == "far":               # the box covers a small corner of the frame's middle: a start looks through many windows, and batches, for its live positions
        spec = scenes.cbox_scene(48, 48, 2, 0, 0, param="box_x")
        spec.cameras[0].to_world_raw = np.asarray(scenes.translate(208.0, 273.0, FAR_Z), np.float32)
        return spec
    w, h, spp = {"8x8": (8, 8, 1), "16x16": (16, 16, 1), "16x16x5": (16, 16, 5), "24x16x3": (24, 16, 3)}[name]
    return scenes.cbox_scene(w, h, spp, 0, 0, param="box_x")


def pixel_list(spec):
    """a list with ids outside the frame (those lanes trace their camera ray) among ids inside it, some of them twice"""
    n = spec.width * spec.height
    rng = np.random.default_rng(5)
    pix = np.concatenate([rng.integers(0, n, 200), np.arange(n, n + 30), [3 * n + 5, spec.width * (spec.height + 7) + 2]]).astype(np.int32)
    rng.shuffle(pix)
    return pix


# case -> (frame, max_depth, further psdr_render_args fields, pixel list?)
CASES = {
    "8x8": ("8x8", 3, {}, False),                              # 64 positions: fewer live items than any threshold
    "16x16": ("16x16", 3, {}, False),                          # exactly one fetch batch
    "16x16x5": ("16x16x5", 3, {}, False),                      # five batches
    "24x16x3": ("24x16x3", 3, {}, False),                      # a partial last batch
    "far": ("far", 3, {}, False),                              # more than three windows per start, across batches
    "depth1": ("24x16x3", 1, {}, False),
    "depth6": ("24x16x3", 6, {}, False),
    "hide": ("16x16x5", 3, {"hide_emitters": True}, False),
    "shard0": ("16x16x5", 3, {"shard_rank": 0, "shard_count": 2}, False),
    "shard1": ("16x16x5", 3, {"shard_rank": 1, "shard_count": 2}, False),
    "skip": ("16x16x5", 3, {"skips": (1000, 500, 250)}, False),
    "list": ("24x16x3", 3, {}, True),
}


def render(sc, n_rows, depth, **kw):
    """-> (renderC [n_rows, 3], renderD [2, n_rows, 3])"""
    import torch
    from psdr_jit_amd import cabi
    buf = torch.zeros((3, n_rows, 3), dtype=torch.float32, device="cuda")
    a = cabi.make_args(max_depth=depth, seeds=SEEDS, **kw)
    cabi.check(cabi.lib().psdr_hip_render_c(C.c_void_p(sc._hip_handle()), C.byref(a), buf[0].data_ptr(), None))
    cabi.check(cabi.lib().psdr_hip_render_d_fwd(C.c_void_p(sc._hip_handle()), C.byref(a), buf[1].data_ptr(), buf[2].data_ptr(), None))
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    return out[0], out[1:]


_built = {}


def scene_of(frame):
    if frame not in _built:
        spec = frame_spec(frame)
        _built[frame] = (spec, product.build_scene(spec))
    return _built[frame]


def render_case(name):
    import torch
    frame, depth, kw, listed = CASES[name]
    spec, sc = scene_of(frame)
    if not listed:
        return render(sc, spec.width * spec.height, depth, **kw)
    pix = torch.from_numpy(pixel_list(spec)).cuda()
    return render(sc, int(pix.numel()), depth, pix_ids_ptr=pix.data_ptr(), n_pix=int(pix.numel()), **kw)


def main(out):
    frames = {}         # (the libraries are the ones the calling test's fixture has built)
    for name in CASES:
        frames[name + "/c"], frames[name + "/d"] = render_case(name)
    np.savez(out, **frames)


if __name__ == "__main__":
    assert os.environ.get("PSDR_GROUP_START") == "0", "run with PSDR_GROUP_START=0"
    main(sys.argv[1])
