// edge_switch.h — when the first path of a primary-edge sample is known to have ended, and whether its last hit still has to be built (paths.h::run_paths, MODE 1;
// tests/cpp/edge_switch_check.cpp plays one lane's loop in both schedules with these functions on the host: g++ alone).
//
// An edge sample is two paths on one lane, ray_n's then ray_p's (side 0, side 1).  The loop learns that a path has ended in its vertex block, AFTER it has built the
// vertex of the hit in hand (make_its); the LATE switch therefore builds the second path's first vertex in a make_its of its own, under the thin mask of the lanes that
// switch.  But whether a path ends at the hit in hand is known before that vertex is built, from values in registers:
//     the extension ray was not traced (invalid BSDF sample) or hit nothing,
//     the camera ray missed, or max_depth == 0,
//     the hit is the path's last one (depth + 1 >= max_depth) -
// and the vertex of a last hit is read for one term only, Le(vertex) x throughput x MIS weight, which is zero unless the hit mesh is an emitter.  A lane whose first
// path ends without that term switches sides EARLY, ahead of the loop's one make_its, and hands its parked ray_p hit to it in the same iteration.  The rare lane that
// needs the vertex (needs_itx) goes through the vertex block as ever and switches one iteration later.
//     es_last_hit       the hit in hand is the path's last vertex: the emitter test is wanted (one LDS row + the mesh record)
//     es_path_end       the decision: ends, needs_itx
//     es_end_depth      the depth the vertex block would leave behind at the path's end (the sampler's skip reads it)
#pragma once

#if defined(__HIPCC__)
#define PSDR_ES_HD __host__ __device__ inline
#else
#define PSDR_ES_HD inline
#endif

namespace psdr {

struct EdgeSwitch { bool ends, needs_itx; };

// depth: -1 = the ray in hand is the camera ray, k >= 0 = the extension ray of vertex k.  hit: the ray was traced and hit a triangle
PSDR_ES_HD bool es_last_hit(int depth, int max_depth, bool bs_valid, bool hit) {
    return bs_valid && hit && (depth < 0 ? max_depth == 0 : depth + 1 >= max_depth);
}

// hit_emitter: the hit triangle's mesh is an emitter (read only where es_last_hit holds)
PSDR_ES_HD EdgeSwitch es_path_end(int depth, int max_depth, bool bs_valid, bool hit, bool hit_emitter) {
    EdgeSwitch r;
    const bool last = es_last_hit(depth, max_depth, bs_valid, hit);
    r.ends = !(bs_valid && hit) || last;
    // a camera hit with max_depth == 0 IS the path (res = Le of the vertex, or a first-hit integrator's value); a later last hit adds Le x thr x weight
    r.needs_itx = last && (depth < 0 || hit_emitter);
    return r;
}

PSDR_ES_HD int es_end_depth(int depth) { return depth < 0 ? 0 : depth + 1; }

} // namespace psdr
