"""Wall times of Scene.unit_ray_intersectAD for 1 M rays on two scenes (events, warmed up):

  cbox   the README Cornell box (the C3 scene), camera rays through a 1024 x 1024 grid of pixel centres: coherent, most rays of a wave on
         one or two triangles (the floor, the walls) - the contended case of the reverse kernel's accumulation
  blob   BASELINE config 5 (81 920-triangle blob on a floor, BVH class), random rays from random points inside the box: incoherent

Rows: the C record (psdr_hip_ray_intersect), the AD record (psdr_hip_ray_intersect_ad), forward_grad(its.t, P) and backward() through the
Python surface (host chain rule included), and the reverse kernel alone (psdr_hip_ray_intersect_adj) for several PSDR_ISECT_ADJ_ROUNDS
(0 = per-lane atomics only).      python tools/time_intersect_ad.py [--out file.json]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__  # noqa: E402

__graft_entry__.build()
import psdr_jit_amd as psdr  # noqa: E402
from psdr_jit_amd import cabi, _core  # noqa: E402
import product  # noqa: E402
import scenes  # noqa: E402

N_REP, N_WARM = 20, 3
ROUNDS = (0, 1, 2, 4, 8, 16, 32, 64)


def gpu_ms(fn, rep=N_REP):
    for _ in range(N_WARM):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(rep):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / rep


def wall_ms(fn, rep=5):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(rep):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / rep * 1e3


def camera_rays(res):
    tan = np.tan(np.radians(30.0))
    ys, xs = np.meshgrid((np.arange(res) + 0.5) / res, (np.arange(res) + 0.5) / res, indexing="ij")
    d = np.stack([(1.0 - 2.0 * xs) * tan, (1.0 - 2.0 * ys) * tan, np.ones_like(xs)], axis=-1).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.tile(np.array([[208.0, 273.0, -800.0]]), (d.shape[0], 1)).astype(np.float32), d.astype(np.float32)


def box_rays(n, seed=0):
    rng = np.random.default_rng(seed)
    o = rng.uniform([10.0, 10.0, 10.0], [540.0, 540.0, 540.0], (n, 3)).astype(np.float32)
    d = rng.normal(0.0, 1.0, (n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d.astype(np.float32)


def run(name, sc, mesh_key, o_np, d_np):
    dev = torch.device("cuda")
    n = o_np.shape[0]
    h = sc._hip_handle()
    L = cabi.lib()
    o, d = torch.from_numpy(o_np).to(dev), torch.from_numpy(d_np).to(dev)
    rec, rec_ad = torch.zeros((n, 24), device=dev), torch.zeros((n, 24), device=dev)
    hit = torch.empty((n,), dtype=torch.int32, device=dev)
    res = {"rays": n}
    res["c_record_ms"] = gpu_ms(lambda: _core._ray_intersect(sc, n, o.data_ptr(), d.data_ptr(), rec.data_ptr(), 0))
    res["ad_record_ms"] = gpu_ms(lambda: cabi.check(L.psdr_hip_ray_intersect_ad(h, n, o.data_ptr(), d.data_ptr(), None, None, rec_ad.data_ptr(), None, hit.data_ptr(), None)))
    valid = rec_ad[:, 0] > 0
    res["hit_fraction"] = float(valid.float().mean())
    g_rec = (torch.rand((n, 24), device=dev) - 0.5) * valid[:, None]
    g_rec[:, [0, 1, 3]] = 0.0
    n_tris = int(sc._snapshot_counts()[0])
    g_tri = torch.zeros(n_tris * 22, device=dev)
    g_o, g_d = torch.zeros((n, 3), device=dev), torch.zeros((n, 3), device=dev)
    for r in ROUNDS:
        os.environ["PSDR_ISECT_ADJ_ROUNDS"] = str(r)
        res["adj_ms_rounds_%d" % r] = gpu_ms(lambda: cabi.check(L.psdr_hip_ray_intersect_adj(h, n, o.data_ptr(), d.data_ptr(), hit.data_ptr(), g_rec.data_ptr(), None,
                                                                                             g_tri.data_ptr(), g_o.data_ptr(), g_d.data_ptr(), None)))
    os.environ.pop("PSDR_ISECT_ADJ_ROUNDS")
    # the Python surface: a translation leaf P on one mesh, o and d requiring grad
    P = torch.zeros((), requires_grad=True)
    sc.param_map[mesh_key].set_transform(psdr.Matrix4fD([[1., 0., 0., P], [0., 1., 0., 0.], [0., 0., 1., 0.], [0., 0., 0., 1.]]))
    sc.configure([0])
    oo, dd = o.clone().requires_grad_(), d.clone().requires_grad_()
    its = sc.unit_ray_intersectAD(psdr.RayC(oo, dd))
    loss = its.t.sum() + its.p.sum() + its.sh_frame.n.sum() + its.wi.sum() + its.uv.sum()
    res["backward_ms"] = wall_ms(lambda: loss.backward(retain_graph=True))
    res["forward_grad_ms"] = wall_ms(lambda: psdr.forward_grad(its.t, P))
    res["python_ad_call_ms"] = wall_ms(lambda: sc.unit_ray_intersectAD(psdr.RayC(oo, dd)))
    print("%-5s %d rays, %.0f %% hit:  C record %.3f ms   AD record %.3f ms   reverse kernel %s   backward() %.2f ms   forward_grad %.2f ms   unit_ray_intersectAD() %.2f ms"
          % (name, n, 100 * res["hit_fraction"], res["c_record_ms"], res["ad_record_ms"],
             " ".join("r%d %.3f" % (r, res["adj_ms_rounds_%d" % r]) for r in ROUNDS), res["backward_ms"], res["forward_grad_ms"], res["python_ad_call_ms"]))
    return res


def main():
    out = {}
    sc = product.build_scene(scenes.cbox_scene(64, 64, 1, 0, 0, param=None))
    out["cbox_camera_1024sq"] = run("cbox", sc, "Mesh[3]", *camera_rays(1024))
    sc = product.build_scene(scenes.config5_scene(64, 64, 1, 1, 1, param=None))
    out["config5_random_1M"] = run("blob", sc, "Mesh[0]", *box_rays(1 << 20))
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
