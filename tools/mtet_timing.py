"""Marching tetrahedra (psdr.MarchingTetrahedra: extract with its one synchronisation, mt(sdf, pos) plus its backward) against the same operator written with torch ops only,
the form DMTet implementations use: sign tests over a tet index array, table look-ups, torch.unique over sorted edge pairs, and index_add_ in the backward of the
interpolation.  A yardstick, not a comparison against this code.

  python tools/mtet_timing.py [--sizes 64 128 256] [--reps 10] [--warmup 2] [--out FILE.json] [--no-bunny]

Workloads: the distance to a sphere, and the bunny's signed distance (psdr.signed_distance of tests/data's bunny_low.obj at the lattice's points), on lattices of n^3
vertices over [-1, 1]^3.  The evaluation of the bunny's signed distance is timed by itself and not counted.
Candidates, alternating inside one process after the warm-up:
  extract       mt.extract(sdf)                         masks, both scans, the read of the two counts (the one synchronisation), the emit of edges and faces
  v+backward    mt(sdf, pos).backward(g)                one launch forward, one launch for the fourteen-slot gather
  torch extract the torch form of the topology          (its boolean indexing and torch.unique synchronise as well)
  torch v+bwd   the torch form of the interpolation and autograd's backward through index_select
Two clocks per candidate: `call` is a host clock around one call that ends in a device synchronise (median of --reps calls, min - max); `queued` is device events around --reps
calls queued back to back, divided by --reps (for the two extracts the calls wait inside, so this is the same quantity measured on the device).
The byte floor: the bytes every pass must move at least once - extract: 15 per lattice vertex (sdf, mask written and re-read, base, the emit's reads), 18 per cell (sdf through
the cache counted once per pass, the face count written and re-read, the offsets written and read) and 8 per edge row, 12 per face row; positions: 20 per mesh vertex plus the
32 bytes of the two ends, at most the whole lattice's 16 Nv; the gather: 37 per lattice vertex plus 12 per mesh vertex - divided by the 6.29 TB/s of a device copy (README)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import psdr_jit_amd as psdr

COPY_RATE = 6.29e12          # bytes per second of a device copy (README)
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))


def tet_table():
    """(pairs int64 [6, 16, 2, 3, 2], n_tri int64 [16]): the triangles of (tet k, inside mask) as pairs of tet-local corners, from the rules of include/psdr_hip.h and wound
    geometrically on the unit cell"""
    pairs, n_tri = np.zeros((6, 16, 2, 3, 2), np.int64), np.zeros(16, np.int64)
    for k, perm in enumerate(PERMS):
        q = np.zeros((4, 3))
        for step, axis in enumerate(perm):
            q[step + 1] = q[step]
            q[step + 1, axis] += 1
        for mask in range(1, 15):
            ins = [i for i in range(4) if mask >> i & 1]
            outs = [i for i in range(4) if not mask >> i & 1]
            if len(ins) == 2:
                (i, j), (a, b) = ins, outs
                quad = [(i, a), (i, b), (j, b), (j, a)]
                tris = [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
            else:
                lone, others = (ins[0], outs) if len(ins) == 1 else (outs[0], ins)
                tris = [[(lone, o) for o in others]]
            n_tri[mask] = len(tris)
            direction = q[outs].mean(0) - q[ins].mean(0)
            for t, tri in enumerate(tris):
                mid = np.array([(q[a] + q[b]) / 2 for a, b in tri])
                if np.dot(np.cross(mid[1] - mid[0], mid[2] - mid[0]), direction) < 0:
                    tri = [tri[0], tri[2], tri[1]]
                pairs[k, mask, t] = [(min(p), max(p)) for p in tri]
    return pairs, n_tri


def tet_corners(shape, device):
    """int64 [6 cells, 4] on the device: built once, as a DMTet grid is"""
    nx, ny, nz = shape
    c = torch.arange((nx - 1) * (ny - 1) * (nz - 1), device=device)
    low = c % (nx - 1) + nx * ((c // (nx - 1)) % (ny - 1) + ny * (c // ((nx - 1) * (ny - 1))))
    stride = (1, nx, nx * ny)
    off = torch.tensor([[0, stride[p[0]], stride[p[0]] + stride[p[1]], 1 + nx + nx * ny] for p in PERMS], device=device)
    return (low[:, None, None] + off[None]).reshape(-1, 4)


class TorchMtet:
    def __init__(self, shape, device):
        self.nv = shape[0] * shape[1] * shape[2]
        self.tets = tet_corners(shape, device)
        self.k = torch.arange(len(self.tets), device=device) % 6
        pairs, n_tri = tet_table()
        self.pairs, self.n_tri = torch.from_numpy(pairs).to(device), torch.from_numpy(n_tri).to(device)
        self.pow2 = torch.tensor([1, 2, 4, 8], device=device)

    def extract(self, sdf):
        with torch.no_grad():
            occ = sdf < 0
            m = (occ[self.tets].long() * self.pow2).sum(1)
            n = self.n_tri[m]
            valid = n > 0
            tv, mv, kv, nvld = self.tets[valid], m[valid], self.k[valid], n[valid]
            local = self.pairs[kv, mv]                                            # [Tv, 2, 3, 2]
            ends = torch.gather(tv[:, None, None, :].expand(-1, 2, 3, -1), 3, local)
            keep = torch.arange(2, device=sdf.device)[None, :] < nvld[:, None]
            ends = ends[keep]                                                     # [F, 3, 2]
            key = ends[..., 0] * self.nv + ends[..., 1]
            uniq, inverse = torch.unique(key.reshape(-1), sorted=True, return_inverse=True)
            return torch.stack([uniq // self.nv, uniq % self.nv], 1), inverse.reshape(-1, 3)

    @staticmethod
    def vertices(sdf, pos, edges):
        sa, sb = sdf.index_select(0, edges[:, 0]), sdf.index_select(0, edges[:, 1])
        pa, pb = pos.index_select(0, edges[:, 0]), pos.index_select(0, edges[:, 1])
        return pa + (sa / (sa - sb))[:, None] * (pb - pa)


def clocks(cands, reps, warmup):
    t = {k: [] for k, _ in cands}
    for k in range(warmup + reps):
        for key, fn in cands:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if k >= warmup:
                t[key].append(1e3 * (time.perf_counter() - t0))
    out = {}
    for key, fn in cands:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        a = np.asarray(t[key])
        out[key] = {"call_median_ms": float(np.median(a)), "call_min_ms": float(a.min()), "call_max_ms": float(a.max()), "queued_ms": e0.elapsed_time(e1) / reps}
    return out


def measure(name, shape, sdf, pos, reps, warmup):
    mt = psdr.MarchingTetrahedra(shape)
    tm = TorchMtet(shape, sdf.device)
    topo = mt.extract(sdf)
    V, F = topo.num_vertices, topo.num_faces
    t_edges, t_faces = tm.extract(sdf)
    same = (len(t_edges), len(t_faces)) == (V, F) and torch.equal(torch.unique(t_edges[:, 0] * tm.nv + t_edges[:, 1]),
                                                                  torch.unique(topo.edges[:, 0].long() * tm.nv + topo.edges[:, 1].long()))
    g = torch.from_numpy(np.random.default_rng(3).uniform(-1.0, 1.0, (V, 3)).astype(np.float32)).to(sdf.device)
    ls, lp = sdf.clone().requires_grad_(), pos.clone().requires_grad_()

    def ours():
        ls.grad = lp.grad = None
        mt(ls, lp).backward(g)

    def theirs():
        ls.grad = lp.grad = None
        tm.vertices(ls, lp, t_edges).backward(g)

    res = clocks([("extract", lambda: mt.extract(sdf)), ("v+backward", ours), ("torch extract", lambda: tm.extract(sdf)), ("torch v+bwd", theirs)], reps, warmup)
    nv, nc = mt.num_lattice, (shape[0] - 1) * (shape[1] - 1) * (shape[2] - 1)
    floors = {"extract": 1e3 * (15.0 * nv + 18.0 * nc + 8.0 * V + 12.0 * F) / COPY_RATE,
              "v+backward": 1e3 * (20.0 * V + min(32.0 * V, 16.0 * nv) + 37.0 * nv + 12.0 * V) / COPY_RATE}
    res.update({"case": name, "shape": list(shape), "V": V, "F": F, "torch_counts_and_edges_agree": bool(same), "reps": reps, "warmup": warmup, "floor_ms": floors,
                "plan": list(psdr.launch_plan_mt(shape))})
    print("%s: shape %s, V = %d, F = %d, the torch form agrees: %s" % (name, shape, V, F, same))
    for key in ("extract", "v+backward", "torch extract", "torch v+bwd"):
        r = res[key]
        print("  %-14s call %10.4f ms [%10.4f, %10.4f]   queued %10.4f ms" % (key, r["call_median_ms"], r["call_min_ms"], r["call_max_ms"], r["queued_ms"]))
    for ours_key, theirs_key in (("extract", "torch extract"), ("v+backward", "torch v+bwd")):
        res["%s: torch / ours (call)" % ours_key] = res[theirs_key]["call_median_ms"] / res[ours_key]["call_median_ms"]
        res["%s: over the byte floor (queued)" % ours_key] = res[ours_key]["queued_ms"] / floors[ours_key]
        print("  %-14s torch / ours %.1f per call, %.1f queued; byte floor %.4f ms, ours at %.1f x" % (ours_key, res["%s: torch / ours (call)" % ours_key],
              res[theirs_key]["queued_ms"] / res[ours_key]["queued_ms"], floors[ours_key], res["%s: over the byte floor (queued)" % ours_key]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-bunny", action="store_true")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mtet_timing.py measures on the GPU: none visible")
    res = []
    if not opt.no_bunny:
        import subdiv_ref
        bf, _bn, bv, _ft, _vt = subdiv_ref.load_obj(subdiv_ref.BUNNY)
        bf = np.asarray(bf).reshape(-1, 3)
        bv = (1.6 * ((bv - bv.min(0)) / (bv.max(0) - bv.min(0)).max() - 0.5 * (bv.max(0) - bv.min(0)) / (bv.max(0) - bv.min(0)).max())).astype(np.float32)      # centred, 1.6 wide
        faces = torch.from_numpy(np.ascontiguousarray(bf, np.int32)).cuda()
    for n in opt.sizes:
        shape = (n, n, n)
        reps = opt.reps if n <= 128 else max(3, opt.reps // 3)
        pos = psdr.lattice_points(shape, -1.0, 1.0).cuda()
        sphere = (pos.double() - torch.tensor([0.031, -0.047, 0.052], device="cuda", dtype=torch.float64)).norm(dim=1).sub(0.642).float()
        res.append(measure("sphere %d^3" % n, shape, sphere, pos, reps, opt.warmup))
        if not opt.no_bunny:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sdf = psdr.signed_distance(pos, torch.from_numpy(bv), faces).sdf
            torch.cuda.synchronize()
            ms = 1e3 * (time.perf_counter() - t0)
            print("bunny %d^3: signed_distance of %d points against %d faces took %.1f ms (not counted)" % (n, len(pos), len(bf), ms))
            r = measure("bunny %d^3" % n, shape, sdf, pos, reps, opt.warmup)
            r["signed_distance_ms_not_counted"] = ms
            res.append(r)
    print(json.dumps(res))
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
