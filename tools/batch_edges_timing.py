"""Edge terms of a pixel list: the batch entry points (psdr_hip_render_d_fwd_batch / _bwd_batch, samples off the list dropped before their rays) against
what could be done before they existed - the full-frame edge terms plus a gather (forward) / a scatter of the weights plus the full-frame reverse pass.

  python tools/batch_edges_timing.py [--res 512] [--spp 32] [--reps 15] [--out FILE.json]

Scenes: the README Cornell box (brute force, Mesh[0] x-translation) and the sphere box (BVH), PathTracer(3).  Lists: (i) the 64 x 64 tile of the frame with the
most pixels that carry a non-zero full-frame edge derivative ("a crop on a silhouette"), (ii) 4096 random pixels, (iii) the identity list.  The two forms
alternate inside one process after a warm-up; every call is timed with device events (map build, gather / scatter included) and the table gives the
median and the min-max spread in ms.  skip_static_edges = 1 as the Python layer sets it (0 with --trace-static)."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import psdr_jit_amd as psdr  # noqa: F401  (loads the libraries)
from psdr_jit_amd import cabi
import product
import scenes

PRIMARY, SECONDARY = 2, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace-static", action="store_true")
    ap.add_argument("--out", default="")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("batch_edges_timing.py measures on the GPU: none visible")
    L = cabi.lib()
    res, spp, n = opt.res, opt.spp, opt.res * opt.res
    rows = []
    for scene_name, spec in (("cornell box", scenes.cbox_scene(res, res, spp, spp, spp, param="light_x")), ("sphere box", scenes.sphere_scene(res, res, spp, spp, spp))):
        sc = product.build_scene(spec)
        h = sc._hip_handle()
        snap = sc._snapshot()
        n_tris, n_sec = np.asarray(snap["d_triangles"]).shape[0], np.asarray(snap["d_sec_edges"]).shape[0]
        n_prim = np.asarray(sc.param_map["Sensor[0]"]._primary_edges(True)).shape[0]
        z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda")
        gbuf = [z(n_tris, 22), z(max(1, len(spec.bsdfs)), 3), z(max(1, len(spec.emitters)), 3), z(max(1, n_sec), 6), z(max(1, n_prim), 4)]
        grads = cabi.Grads(*[t.data_ptr() for t in gbuf])
        full = z(2, n, 3)

        def args(terms, pix=None):
            return cabi.make_args(max_depth=opt.depth, seeds=(1, 2, 3), terms=terms, skip_static_edges=not opt.trace_static,
                                  pix_ids_ptr=pix.data_ptr() if pix is not None else 0, n_pix=int(pix.numel()) if pix is not None else 0)
        a = args(PRIMARY | SECONDARY)
        cabi.check(L.psdr_hip_render_d_fwd(h, C.byref(a), full[0].data_ptr(), full[1].data_ptr(), None))
        live = (full[1].abs().amax(dim=1) > 0).reshape(res, res)
        tiles = live.reshape(res // 64, 64, res // 64, 64).sum(dim=(1, 3))
        ty, tx = divmod(int(tiles.argmax()), res // 64)
        crop = torch.arange(n, device="cuda", dtype=torch.int32).reshape(res, res)[64 * ty:64 * ty + 64, 64 * tx:64 * tx + 64].reshape(-1).contiguous()
        rnd = torch.from_numpy(np.random.default_rng(5).choice(n, 4096, replace=False).astype(np.int32)).cuda()
        ident = torch.arange(n, device="cuda", dtype=torch.int32)
        for list_name, pix in (("crop 64x64 at tile (%d, %d)" % (ty, tx), crop), ("4096 random", rnd), ("identity", ident)):
            npix = int(pix.numel())
            kept = int(live.reshape(-1)[pix.long()].sum())
            out = z(2, npix, 3)
            w = torch.rand((npix, 3), device="cuda") + 0.5
            for terms, term_name in ((PRIMARY, "primary"), (SECONDARY, "secondary"), (PRIMARY | SECONDARY, "both")):
                a_full, a_list = args(terms), args(terms, pix)

                def fwd_base():
                    cabi.check(L.psdr_hip_render_d_fwd(h, C.byref(a_full), full[0].data_ptr(), full[1].data_ptr(), None))
                    return full[1].index_select(0, pix.long())

                def fwd_batch():
                    cabi.check(L.psdr_hip_render_d_fwd_batch(h, C.byref(a_list), out[0].data_ptr(), out[1].data_ptr(), None))
                    return out[1]

                def bwd_base():
                    Wp = torch.zeros((n, 3), dtype=torch.float32, device="cuda").index_add_(0, pix.long(), w)
                    cabi.check(L.psdr_hip_render_d_bwd(h, C.byref(a_full), Wp.data_ptr(), C.byref(grads), None))
                    return torch.cat([gbuf[k].reshape(-1) for k in (0, 3, 4)])

                def bwd_batch():
                    cabi.check(L.psdr_hip_render_d_bwd_batch(h, C.byref(a_list), w.data_ptr(), C.byref(grads), None))
                    return torch.cat([gbuf[k].reshape(-1) for k in (0, 3, 4)])
                for mode, base, batch in (("forward", fwd_base, fwd_batch), ("reverse", bwd_base, bwd_batch)):
                    t = {"base": [], "batch": []}
                    res_ = {}
                    for it in range(opt.warmup + opt.reps):
                        for key, fn in (("base", base), ("batch", batch)):
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            r = fn()
                            e1.record()
                            torch.cuda.synchronize()
                            if it >= opt.warmup:
                                t[key].append(e0.elapsed_time(e1))
                            res_[key] = r.detach().clone()
                    diff = float((res_["base"].double() - res_["batch"].double()).abs().max()) / max(1e-30, float(res_["base"].double().abs().max()))
                    row = {"scene": scene_name, "list": list_name, "n_pix": npix, "pixels_with_edge_derivative": kept, "term": term_name, "mode": mode, "max_rel_diff": diff}
                    for key in ("base", "batch"):
                        v = np.asarray(t[key])
                        row[key + "_ms"] = {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}
                    rows.append(row)
                    print("%-11s %-28s %-9s %-7s full+gather %7.3f [%7.3f, %7.3f]  batch %7.3f [%7.3f, %7.3f]  ratio %.2f  diff %.1e  (%d of %d pixels carry an edge derivative)" % (
                        scene_name, list_name, term_name, mode, row["base_ms"]["median"], row["base_ms"]["min"], row["base_ms"]["max"],
                        row["batch_ms"]["median"], row["batch_ms"]["min"], row["batch_ms"]["max"], row["batch_ms"]["median"] / row["base_ms"]["median"], diff, kept, npix), flush=True)
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as fh:
            json.dump({"res": res, "spp": spp, "depth": opt.depth, "reps": opt.reps, "skip_static_edges": not opt.trace_static, "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
