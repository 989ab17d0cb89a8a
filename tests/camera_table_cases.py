"""The frames tests/test_gpu_camera_table.py renders twice - with the sensor's camera-ray table and, in a fresh child process that runs this file with
PSDR_NO_CAM_TABLE=1 (the switch is read once per process, where PSDR_NO_LIVE_MASK is), with every camera ray through the tracer.

    python tests/camera_table_cases.py OUT.npz       renders every case, writes {"<case>/<terms>": [2, n_pix, 3] (image, derivative)}
"""
import ctypes as C
import os
import sys

import numpy as np

if __name__ == "__main__":          # (run as a script: the repository root is not on the path yet)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import product                      # noqa: E402
import scenes                       # noqa: E402

DEPTH = 3
SEEDS = (31, 32, 33)
TERMS = (1, 2, 7)


def border_camera():
    """A camera of the Cornell box whose frame the silhouette edges cross and touch: at x = 0 the green wall's front edge (x = 0, z = 0) projects onto the boundary
    between pixel columns 31 and 32 of a 64-pixel row; the floor's and the ceiling's front edges leave the frame through its right border; and the ceiling's front
    edge (y = 548.79999, z = 0) runs ALONG the top border, 3e-6 inside it - less than EdgeEpsilon = 1e-5, so the outer point p - eps n of each of its samples lies
    outside [0, 1)^2 while the sample itself counts"""
    y = np.float32(548.79999) - 500.0 * np.tan(np.radians(30.0)) * (1.0 - 2.0 * 3e-6)
    return scenes.translate(0.0, float(np.float32(y)), -500.0)


def case_spec(name):
    if name == "cbox_light":
        return scenes.cbox_scene(96, 80, 8, 8, 8, param="light_x")
    if name == "cbox_box":
        return scenes.cbox_scene(96, 80, 8, 8, 8, param="box_x")
    if name == "microfacet":
        return scenes.microfacet_cbox_scene(64, 48, 8, 8, 8, param="box_x")
    if name == "border":
        # the parameter moves the camera along its diagonal, to_world_left = T(100 P, 100 P, 0): every silhouette edge has a normal velocity, whatever its direction
        spec = scenes.cbox_scene(64, 64, 8, 8, 8, param="camera_x")
        spec.cameras[0].d_to_world_left[1, 3] = 100.0
        spec.cameras[0].to_world_raw = np.asarray(border_camera(), np.float32)
        return spec
    raise ValueError(name)


CASES = ("cbox_light", "cbox_box", "microfacet", "border")


def render_d(sc, n_rows, terms, depth=DEPTH, seeds=SEEDS, **kw):
    """psdr_hip_render_d_fwd -> [2, n_rows, 3] (image, derivative); kw: further psdr_render_args fields (cabi.make_args)"""
    import torch
    from psdr_jit_amd import cabi
    buf = torch.zeros((2, n_rows, 3), dtype=torch.float32, device="cuda")
    a = cabi.make_args(max_depth=depth, seeds=seeds, terms=terms, **kw)
    cabi.check(cabi.lib().psdr_hip_render_d_fwd(C.c_void_p(sc._hip_handle()), C.byref(a), buf[0].data_ptr(), buf[1].data_ptr(), None))
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def camera_table(sc, sensor=0):
    """-> (cell size in pixels or 0 = no table, table [cells_h, cells_w] uint64)"""
    from psdr_jit_amd import cabi
    g, cw, ch = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    L = cabi.lib()
    cabi.check(L.psdr_hip_scene_camera_table(C.c_void_p(sc._hip_handle()), sensor, C.byref(g), C.byref(cw), C.byref(ch), None))
    tab = np.zeros((ch.value, cw.value), np.uint64)
    if g.value:
        cabi.check(L.psdr_hip_scene_camera_table(C.c_void_p(sc._hip_handle()), sensor, None, None, None, tab.ctypes.data))
    return g.value, tab


def main(out):
    frames = {}         # (the libraries are the ones the calling test's fixture has built)
    for name in CASES:
        spec = case_spec(name)
        sc = product.build_scene(spec)
        assert camera_table(sc)[0] == 0, "PSDR_NO_CAM_TABLE=1 must leave the sensor without a table"
        for terms in TERMS:
            frames["%s/%d" % (name, terms)] = render_d(sc, spec.width * spec.height, terms)
    np.savez(out, **frames)


if __name__ == "__main__":
    assert os.environ.get("PSDR_NO_CAM_TABLE"), "run with PSDR_NO_CAM_TABLE=1"
    main(sys.argv[1])
