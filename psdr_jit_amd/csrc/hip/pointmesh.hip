// pointmesh.hip — the point-to-mesh distance: for every point the nearest face, for every face the nearest point, the loss and its gradient with respect to the points and
// the vertices (Python surface: psdr_jit_amd/pointmesh.py).
//
// The definition (include/psdr_hip.h, THE POINT-TO-MESH DISTANCE, states it in full).  closest() below is the pair function: Ericson's region cascade for the closest point of a
// closed triangle, as barycentrics (s, t), and dist2 = |e|^2 with e = (p - a) - (s ab + t ac), the difference form.  Both scans and the evaluation kernels call this one function.
//
// The cascade as selects.  Over ALL pairs of a scan nearly every pair ends in a vertex region (93 % on the bunny), while the winners are interior (83 %): a cascade of
// branches would diverge in every wave and pay every branch on every pair.  closest() computes d1 .. d6 and va, vb, vc once, forms the seven predicates, selects one numerator
// pair and one denominator, and divides twice - the quotients are those of the definition, bit for bit, because every region's s and t is one correctly rounded division (or a
// constant, or 1 - t) of the selected operands.  A denominator of 0 gives the quotient 0.
//
// The scans (k_scan<Q, FACE_QUERIES>).  A lane holds Q queries in registers; the candidates of the workgroup's slice go through LDS a
// tile at a time and every lane reads the same address: a broadcast.
//   points as queries (FACE_QUERIES = false): the candidates are face records (a, ab, ac, b, c: 16 floats, written once per call by k_records), four float4 per face;
//   faces as queries  (FACE_QUERIES = true):  a lane holds its faces' records in registers, the candidates are points as x / y / z planes, one float4 of a plane = four points.
// A lane walks its candidates in ascending order and replaces its best on a strict `<`; the best leaves the lane as the key (float bits of dist2) << 32 | index and the slices
// are merged by one integer atomicMin per query (associative and commutative: the result does not depend on the order), after a clear to all ones on the call's stream.  A
// candidate beyond the slice's end (the padding of a partial last tile: zeros, so that the arithmetic stays finite) has its dist2 replaced by +infinity, which never passes `<`;
// neither does a NaN, so with non-finite inputs the index stays the slice's first candidate: in range.  The scan carries dist2 only; k_unpack evaluates the winning pair once
// more for its barycentrics.
// The evaluation: k_eval_points (a lane per point: its own pair, then the faces that chose it through the inverted index, ascending), k_eval_faces (a lane per face: the [3, 3]
// corner record - its own pair, then the points that chose it, ascending), k_eval_vertices (a lane per vertex: the corner records that name it, in the topology's order), and
// k_finish.  No float atomics, no host synchronisation; the same input gives the same bits.  No contraction in this unit (the build's -ffp-contract=off, and the pair function is
// written with __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn).
#include <cmath>
#include <cstdint>
#include <string>

#include "../../../include/psdr_hip.h"
#include "mesh_pair.h"
#include "nn_scan.h"

namespace {

constexpr int kThreads = 256;                   // 4 waves
constexpr int kSumThreads = 1024;               // k_finish: one workgroup, 16 waves
constexpr int kTile = pm::kTile;                // candidates per LDS tile: 16 KiB of face records, or three planes of 1 KiB of points
constexpr int kWideQueries = pm::kWideQueries;  // queries per lane of the wide scan
static_assert(kThreads == scan::kThreads, "plan_of splits for the scan's workgroup");

__device__ __forceinline__ float quotient(float num, float den) { return den == 0.f ? 0.f : __fdiv_rn(num, den); }

// THE PAIR FUNCTION: the closest point of the closed triangle f to p as (s, t), and dist2.  Selects only; later selects overrule earlier ones, so that the first test of the
// definition's cascade that holds decides
__device__ __forceinline__ float closest(Vec p, const Face &f, float &s, float &t, Vec &e) {
    const Vec ap = sub(p, f.a), bp = sub(p, f.b), cp = sub(p, f.c);
    const float d1 = dot(f.ab, ap), d2 = dot(f.ac, ap), d3 = dot(f.ab, bp), d4 = dot(f.ac, bp), d5 = dot(f.ab, cp), d6 = dot(f.ac, cp);
    const float vc = cross2(d1, d4, d3, d2), vb = cross2(d5, d2, d1, d6), va = cross2(d3, d6, d5, d4);
    const float d43 = __fsub_rn(d4, d3), d56 = __fsub_rn(d5, d6);
    const bool r1 = d1 <= 0.f && d2 <= 0.f;
    const bool r2 = d3 >= 0.f && d4 <= d3;
    const bool r3 = vc <= 0.f && d1 >= 0.f && d3 <= 0.f;
    const bool r4 = d6 >= 0.f && d5 <= d6;
    const bool r5 = vb <= 0.f && d2 >= 0.f && d6 <= 0.f;
    const bool r6 = va <= 0.f && d43 >= 0.f && d56 >= 0.f;
    // the operands of the two divisions: region 7, overruled by 6, 5, 3 in turn (3 before 5 before 6 in the cascade); a vertex region overrules the quotients below
    float ns = vb, nt = vc, den = __fadd_rn(__fadd_rn(va, vb), vc);
    if (r6) { ns = 0.f; nt = d43; den = __fadd_rn(d43, d56); }
    if (r5) { ns = 0.f; nt = d2; den = __fsub_rn(d2, d6); }
    if (r3) { ns = d1; nt = 0.f; den = __fsub_rn(d1, d3); }
    const float qs = quotient(ns, den), qt = quotient(nt, den);
    s = qs;
    t = qt;
    if (r6 && !r5 && !r3) s = __fsub_rn(1.f, qt);
    // vertex c (test 4) stands behind edge ab (test 3) and ahead of edges ac and bc
    if (r4 && !r3) { s = 0.f; t = 1.f; }
    if (r2) { s = 1.f; t = 0.f; }
    if (r1) { s = 0.f; t = 0.f; }
    e = residual(ap, f, s, t);
    return dot(e, e);
}

__device__ __forceinline__ Face face_of(float4 q0, float4 q1, float4 q2, float4 q3) {
    return {{q0.x, q0.y, q0.z}, {q0.w, q1.x, q1.y}, {q1.z, q1.w, q2.x}, {q2.y, q2.z, q2.w}, {q3.x, q3.y, q3.z}};
}

// the per-face records of the first scan: [F] x four float4 (a, ab, ac, b, c, 0)
__global__ void __launch_bounds__(kThreads) k_records(const float *__restrict__ v, int nv, const int *__restrict__ faces, int nf, float4 *__restrict__ rec) {
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= nf) return;
    const Face r = load_face(v, nv, faces, f);
    rec[4LL * f] = make_float4(r.a.x, r.a.y, r.a.z, r.ab.x);
    rec[4LL * f + 1] = make_float4(r.ab.y, r.ab.z, r.ac.x, r.ac.y);
    rec[4LL * f + 2] = make_float4(r.ac.z, r.b.x, r.b.y, r.b.z);
    rec[4LL * f + 3] = make_float4(r.c.x, r.c.y, r.c.z, 0.f);
}

// n queries against the candidates [blockIdx.y slice_len, ...) of m.  FACE_QUERIES false: the queries are the points p, the candidates the face records rec;
// true: the queries are the faces (v, faces), the candidates the points p
template <int Q, bool FACE_QUERIES> __global__ void __launch_bounds__(kThreads) k_scan(const float *__restrict__ p, const float *__restrict__ v, int nv, const int *__restrict__ faces,
                                                                                      const float4 *__restrict__ rec, int n, int m, int slice_len, int slices,
                                                                                      unsigned long long *__restrict__ keys) {
    constexpr int kQuads = FACE_QUERIES ? 3 * kTile / 4 : 4 * kTile;
    __shared__ float4 s_c[kQuads];
    const int j0 = blockIdx.y * slice_len;
    const int j1 = min(m, j0 + slice_len);
    Vec qp[FACE_QUERIES ? 1 : Q];
    Face qf[FACE_QUERIES ? Q : 1];
    float best[Q];
    int bj[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int i = (blockIdx.x * Q + q) * kThreads + threadIdx.x;
        const int at = min(i, n - 1);                              // (a lane beyond n scans a copy of the last query and stores nothing)
        if constexpr (FACE_QUERIES) qf[q] = load_face(v, nv, faces, at);
        else qp[q] = load3(p, at);
        best[q] = INFINITY;
        bj[q] = j0;
    }
    for (int base = j0; base < j1; base += kTile) {
        __syncthreads();                                       // (the previous tile has been read)
        for (int t = threadIdx.x; t < kTile; t += kThreads) {
            const int j = base + t;
            const bool live = j < j1;
            if constexpr (FACE_QUERIES) {
                float *s_x = reinterpret_cast<float *>(s_c), *s_y = s_x + kTile, *s_z = s_y + kTile;
                s_x[t] = live ? p[3LL * j] : 0.f;
                s_y[t] = live ? p[3LL * j + 1] : 0.f;
                s_z[t] = live ? p[3LL * j + 2] : 0.f;
            } else {
                const float4 *src = rec + 4LL * min(j, m - 1);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float4 r = src[k];
                    s_c[4 * t + k] = make_float4(live ? r.x : 0.f, live ? r.y : 0.f, live ? r.z : 0.f, live ? r.w : 0.f);
                }
            }
        }
        __syncthreads();
        const int count = min(kTile, j1 - base);
        const int groups = (count + 3) >> 2;
        for (int g = 0; g < groups; ++g) {
            float cx[4], cy[4], cz[4];
            if constexpr (FACE_QUERIES) {
                const float4 x4 = s_c[g], y4 = s_c[kTile / 4 + g], z4 = s_c[2 * (kTile / 4) + g];
                cx[0] = x4.x; cx[1] = x4.y; cx[2] = x4.z; cx[3] = x4.w;
                cy[0] = y4.x; cy[1] = y4.y; cy[2] = y4.z; cy[3] = y4.w;
                cz[0] = z4.x; cz[1] = z4.y; cz[2] = z4.z; cz[3] = z4.w;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int t = 4 * g + u;
                const bool live = t < count;                   // (uniform over the workgroup)
                Face cf;
                Vec cp;
                if constexpr (FACE_QUERIES) cp = {cx[u], cy[u], cz[u]};
                else cf = face_of(s_c[4 * t], s_c[4 * t + 1], s_c[4 * t + 2], s_c[4 * t + 3]);
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    float s, tt;
                    Vec e;
                    float d2;
                    if constexpr (FACE_QUERIES) d2 = closest(cp, qf[q], s, tt, e);
                    else d2 = closest(qp[q], cf, s, tt, e);
                    d2 = live ? d2 : INFINITY;
                    if (d2 < best[q]) { best[q] = d2; bj[q] = base + t; }
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int i = (blockIdx.x * Q + q) * kThreads + threadIdx.x;
        if (i < n) merge_key(keys, i, pack_key(best[q], bj[q]), slices);
    }
}

// one pair per query: the winner's index and dist2 from the key, its barycentrics from the pair function once more
__global__ void __launch_bounds__(kThreads) k_unpack(const unsigned long long *__restrict__ keys, const float *__restrict__ p, int np, const float *__restrict__ v, int nv,
                                                     const int *__restrict__ faces, int nf, int face_queries, int *__restrict__ idx, float *__restrict__ bary, float *__restrict__ dist2) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    const int n = face_queries ? nf : np, m = face_queries ? np : nf;
    if (i >= n) return;
    const unsigned long long key = keys[i];
    const int j = key_index(key, m);
    float s, t;
    Vec e;
    closest(load3(p, face_queries ? j : i), load_face(v, nv, faces, face_queries ? i : j), s, t, e);
    idx[i] = j;
    bary[3LL * i] = __fsub_rn(__fsub_rn(1.f, s), t);
    bary[3LL * i + 1] = s;
    bary[3LL * i + 2] = t;
    dist2[i] = key_dist2(key);
}

struct Eval {
    const float *p, *v;
    const int *faces;
    int np, nv, nf;
    const int *face_of_point;           // [np] or NULL: the point -> face direction is off
    const float *bary_p, *dist2_p;      // [np, 3], [np]
    const int *point_of_face;           // [nf] or NULL: the face -> point direction is off
    const float *bary_f, *dist2_f;      // [nf, 3], [nf]
    const int *p_begin, *p_list;        // [np + 1], [nf]: the faces that chose a point, ascending
    const int *f_begin, *f_list;        // [nf + 1], [np]: the points that chose a face, ascending
    const int *vc_begin, *vc_corner;    // [nv + 1], [3 nf]: the corners 3 f + c that name a vertex, ascending
    float k_pf, k_fp;                   // squared: 2 w / count; else w / count (divided by sqrt(s) per pair)
    int squared;
    float *grad_p, *grad_v, *corners;   // [np, 3], [nv, 3], [nf, 9], or NULL: a value-only call
    double *partial_p, *partial_f;      // one sum per workgroup
};

// k r of the pair (point i, face f) with the stored barycentrics (s, t) and dist2: r is the pair function's e, bit for bit what the scan's winner had
__device__ __forceinline__ Vec pair_term(const Eval &E, int i, int f, float s, float t, float d2, float k) {
    const Face face = load_face(E.v, E.nv, E.faces, f);
    const Vec e = residual(sub(load3(E.p, i), face.a), face, s, t);
    const float c = coefficient(k, d2, E.squared);
    return {c * e.x, c * e.y, c * e.z};
}

__global__ void __launch_bounds__(kThreads) k_eval_points(Eval E) {
    __shared__ double s_red[kThreads / 64];
    const int i = blockIdx.x * kThreads + threadIdx.x;
    float val = 0.f;
    if (i < E.np) {
        Vec g = {0.f, 0.f, 0.f};
        bool have = false;
        if (E.face_of_point) {
            const float d2 = E.dist2_p[i];
            val = E.squared ? d2 : sqrtf(d2);
            if (E.grad_p) {
                g = pair_term(E, i, clamped(E.face_of_point[i], E.nf), E.bary_p[3LL * i + 1], E.bary_p[3LL * i + 2], d2, E.k_pf);
                have = true;
            }
        }
        if (E.point_of_face && E.grad_p) {
            const int b0 = min(max(E.p_begin[i], 0), E.nf), b1 = min(max(E.p_begin[i + 1], b0), E.nf);
            Vec sum = {0.f, 0.f, 0.f};
            for (int k = b0; k < b1; ++k) {
                const int f = clamped(E.p_list[k], E.nf);
                const Vec r = pair_term(E, i, f, E.bary_f[3LL * f + 1], E.bary_f[3LL * f + 2], E.dist2_f[f], E.k_fp);
                sum.x += r.x;
                sum.y += r.y;
                sum.z += r.z;
            }
            g.x = have ? g.x + sum.x : sum.x;
            g.y = have ? g.y + sum.y : sum.y;
            g.z = have ? g.z + sum.z : sum.z;
        }
        if (E.grad_p) {
            float *o = E.grad_p + 3LL * i;
            o[0] = g.x;
            o[1] = g.y;
            o[2] = g.z;
        }
    }
    if (E.face_of_point) {                                  // (uniform over the launch)
        const double t = block_sum<kThreads>((double) val, s_red);
        if (threadIdx.x == 0) E.partial_p[blockIdx.x] = t;
    }
}

__global__ void __launch_bounds__(kThreads) k_eval_faces(Eval E) {
    __shared__ double s_red[kThreads / 64];
    const int f = blockIdx.x * kThreads + threadIdx.x;
    float val = 0.f;
    if (f < E.nf) {
        float own[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        bool have = false;
        if (E.point_of_face) {
            const float d2 = E.dist2_f[f];
            val = E.squared ? d2 : sqrtf(d2);
            if (E.corners) {
                const float *b = E.bary_f + 3LL * f;
                add_corners(own, pair_term(E, clamped(E.point_of_face[f], E.np), f, b[1], b[2], d2, E.k_fp), b);
                have = true;
            }
        }
        if (E.face_of_point && E.corners) {
            const int b0 = min(max(E.f_begin[f], 0), E.np), b1 = min(max(E.f_begin[f + 1], b0), E.np);
            float sum[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            for (int k = b0; k < b1; ++k) {
                const int i = clamped(E.f_list[k], E.np);
                const float *b = E.bary_p + 3LL * i;
                add_corners(sum, pair_term(E, i, f, b[1], b[2], E.dist2_p[i], E.k_pf), b);
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) own[k] = have ? own[k] + sum[k] : sum[k];
        }
        if (E.corners) {
#pragma unroll
            for (int k = 0; k < 9; ++k) E.corners[9LL * f + k] = own[k];
        }
    }
    if (E.point_of_face) {                                  // (uniform over the launch)
        const double t = block_sum<kThreads>((double) val, s_red);
        if (threadIdx.x == 0) E.partial_f[blockIdx.x] = t;
    }
}

__global__ void __launch_bounds__(kThreads) k_eval_vertices(Eval E) {
    gather_corners<kThreads>(E);
}

__global__ void __launch_bounds__(kSumThreads) k_finish(const double *__restrict__ partial, int blocks_p, int blocks_f, int np, int nf, float w_pf, float w_fp, float *__restrict__ out) {
    __shared__ double s_red[kSumThreads / 64];
    finish_two<kSumThreads>(partial, blocks_p, blocks_f, np, nf, w_pf, w_fp, out, s_red);
}

} // namespace

extern "C" {

int psdr_hip_pointmesh_plan(int32_t n_queries, int32_t n_candidates, int32_t *tile, int32_t *queries_per_lane, int32_t *slices, int32_t *slice_len) {
    const std::string who = "psdr_hip_pointmesh_plan: ";
    if (!in_range(n_queries)) return psdr::api_fail(who + range_text("n_queries", n_queries));
    if (!in_range(n_candidates)) return psdr::api_fail(who + range_text("n_candidates", n_candidates));
    if (!tile || !queries_per_lane || !slices || !slice_len) return psdr::api_fail(who + "NULL argument");
    const Plan p = plan_of<kTile, kWideQueries>(n_queries, n_candidates);
    *tile = p.tile;
    *queries_per_lane = p.qpl;
    *slices = p.slices;
    *slice_len = p.slice_len;
    return 0;
}

int psdr_hip_pointmesh_nearest(const float *p, int32_t n_points, const float *v, int32_t n_vertices, const int32_t *faces, int32_t n_faces, int32_t direction,
                               float *records, uint64_t *keys, int32_t *index, float *bary, float *dist2, void *stream) {
    const std::string who = "psdr_hip_pointmesh_nearest: ";
    if (!in_range(n_points)) return psdr::api_fail(who + range_text("n_points", n_points));
    if (!in_range(n_vertices)) return psdr::api_fail(who + range_text("n_vertices", n_vertices));
    if (!in_range(n_faces)) return psdr::api_fail(who + range_text("n_faces", n_faces));
    if (direction != 0 && direction != 1) return psdr::api_fail(who + "direction = " + std::to_string(direction) + ", must be 0 (points are the queries) or 1 (faces are)");
    if (!p || !v || !faces || !keys || !index || !bary || !dist2) return psdr::api_fail(who + "NULL argument");
    if (direction == 0 && !records) return psdr::api_fail(who + "direction 0 needs the records work array, NULL given");
    const int n = direction ? n_faces : n_points, m = direction ? n_points : n_faces;
    const Plan pl = plan_of<kTile, kWideQueries>(n, m);
    hipStream_t st = (hipStream_t) stream;
    unsigned long long *k = reinterpret_cast<unsigned long long *>(keys);
    const hipError_t e = clear_keys(k, n, pl, st);
    if (e != hipSuccess) return psdr::api_fail(who + hipGetErrorString(e));
    float4 *rec = reinterpret_cast<float4 *>(records);
    const dim3 grid = scan_grid(n, pl);
    if (direction == 0) {
        k_records<<<blocks_of<kThreads>(n_faces), kThreads, 0, st>>>(v, n_vertices, faces, n_faces, rec);
        if (pl.qpl == 1) k_scan<1, false><<<grid, kThreads, 0, st>>>(p, v, n_vertices, faces, rec, n, m, pl.slice_len, pl.slices, k);
        else k_scan<kWideQueries, false><<<grid, kThreads, 0, st>>>(p, v, n_vertices, faces, rec, n, m, pl.slice_len, pl.slices, k);
    } else {
        if (pl.qpl == 1) k_scan<1, true><<<grid, kThreads, 0, st>>>(p, v, n_vertices, faces, rec, n, m, pl.slice_len, pl.slices, k);
        else k_scan<kWideQueries, true><<<grid, kThreads, 0, st>>>(p, v, n_vertices, faces, rec, n, m, pl.slice_len, pl.slices, k);
    }
    k_unpack<<<blocks_of<kThreads>(n), kThreads, 0, st>>>(k, p, n_points, v, n_vertices, faces, n_faces, direction, index, bary, dist2);
    return launch_status(who);
}

int psdr_hip_pointmesh_eval(const float *p, int32_t n_points, const float *v, int32_t n_vertices, const int32_t *faces, int32_t n_faces,
                            const int32_t *face_of_point, const float *bary_p, const float *dist2_p, const int32_t *point_of_face, const float *bary_f, const float *dist2_f,
                            const int32_t *p_begin, const int32_t *p_list, const int32_t *f_begin, const int32_t *f_list, const int32_t *vc_begin, const int32_t *vc_corner,
                            const float *weights, int32_t squared, double *partial, float *corners, float *out, float *grad_p, float *grad_v, void *stream) {
    const std::string who = "psdr_hip_pointmesh_eval: ";
    if (!in_range(n_points)) return psdr::api_fail(who + range_text("n_points", n_points));
    if (!in_range(n_vertices)) return psdr::api_fail(who + range_text("n_vertices", n_vertices));
    if (!in_range(n_faces)) return psdr::api_fail(who + range_text("n_faces", n_faces));
    if (!p || !v || !faces || !weights || !partial || !out) return psdr::api_fail(who + "NULL argument");
    for (int k = 0; k < 2; ++k)
        if (!std::isfinite(weights[k]) || weights[k] < 0.f) return psdr::api_fail(who + "weights[" + std::to_string(k) + "] = " + std::to_string(weights[k]) + ", must be finite and not negative");
    if (!grad_p != !grad_v) return psdr::api_fail(who + "grad_p and grad_v must both be given or both be NULL");
    if (grad_p && (grad_p == p || grad_p == v || grad_v == p || grad_v == v || grad_p == grad_v)) return psdr::api_fail(who + "grad_p and grad_v must be arrays of their own");
    const bool on_pf = weights[0] > 0.f, on_fp = weights[1] > 0.f;
    if (on_pf && (!face_of_point || !bary_p || !dist2_p)) return psdr::api_fail(who + "weights[0] > 0 needs face_of_point, bary_p and dist2_p");
    if (on_fp && (!point_of_face || !bary_f || !dist2_f)) return psdr::api_fail(who + "weights[1] > 0 needs point_of_face, bary_f and dist2_f");
    if (grad_p && (!corners || !vc_begin || !vc_corner)) return psdr::api_fail(who + "the gradients need corners, vc_begin and vc_corner");
    if (grad_p && on_pf && (!f_begin || !f_list)) return psdr::api_fail(who + "the gradient of the point -> face term needs f_begin and f_list, the inverted index of face_of_point");
    if (grad_p && on_fp && (!p_begin || !p_list)) return psdr::api_fail(who + "the gradient of the face -> point term needs p_begin and p_list, the inverted index of point_of_face");
    const double unit = squared ? 2.0 : 1.0;
    const int bp = on_pf ? blocks_of<kThreads>(n_points) : 0, bf = on_fp ? blocks_of<kThreads>(n_faces) : 0;
    Eval E;
    E.p = p; E.v = v; E.faces = faces;
    E.np = n_points; E.nv = n_vertices; E.nf = n_faces;
    E.face_of_point = on_pf ? face_of_point : nullptr; E.bary_p = bary_p; E.dist2_p = dist2_p;
    E.point_of_face = on_fp ? point_of_face : nullptr; E.bary_f = bary_f; E.dist2_f = dist2_f;
    E.p_begin = p_begin; E.p_list = p_list; E.f_begin = f_begin; E.f_list = f_list; E.vc_begin = vc_begin; E.vc_corner = vc_corner;
    E.k_pf = (float) (unit * (double) weights[0] / (double) n_points);
    E.k_fp = (float) (unit * (double) weights[1] / (double) n_faces);
    E.squared = squared ? 1 : 0;
    E.grad_p = grad_p; E.grad_v = grad_v; E.corners = grad_p ? corners : nullptr;
    E.partial_p = partial; E.partial_f = partial + bp;
    hipStream_t st = (hipStream_t) stream;
    if (on_pf || grad_p) k_eval_points<<<blocks_of<kThreads>(n_points), kThreads, 0, st>>>(E);
    if (on_fp || grad_p) k_eval_faces<<<blocks_of<kThreads>(n_faces), kThreads, 0, st>>>(E);
    if (grad_p) k_eval_vertices<<<blocks_of<kThreads>(n_vertices), kThreads, 0, st>>>(E);
    k_finish<<<1, kSumThreads, 0, st>>>(partial, bp, bf, n_points, n_faces, weights[0], weights[1], out);
    return launch_status(who);
}

} // extern "C"
