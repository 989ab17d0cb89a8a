// sdf.hip — the signed distance to a mesh: the generalized winding number of every point (the sign), the signed distance, and the vector-Jacobian product of the signed distance
// with respect to the points and the vertices (Python surface: psdr_jit_amd/sdf.py).
//
// The definition (include/psdr_hip.h, THE SIGNED DISTANCE, states it in full).  theta() below is the pair function: the half solid angle of a face seen from a point, by Van
// Oosterom & Strackee's formula, theta = atan2(Nm, Dn) with the principal value 0 where Nm == 0.  The magnitude is not computed here: the nearest face, its barycentrics and
// dist2 are those of psdr_hip_pointmesh_nearest (pointmesh.hip), which the caller runs as it is.
//
// The scan (k_scan<Q>).  A lane holds Q points in registers; the faces of the workgroup's slice go through LDS a tile at a time as records
// of three float4 (the three corners, written once per call by k_records) and every lane reads the same address: a broadcast.  A lane adds its candidates in ascending f into a
// double and leaves the slice's sum as a float in partial[slice][i]: every entry is written by exactly one lane, nothing is cleared and nothing is atomic.  k_merge adds the
// slices in ascending order in double, scales by 1 / (2 pi), rounds once, and - given dist2 - writes the signed distance.  The split is the point-to-mesh plan's (nn_scan.h).
// The gradient: k_grad_points (a lane per point), k_grad_faces (a lane per face: the [3, 3] corner record over the points that chose the face, ascending, through the inverted
// index), k_grad_vertices (a lane per vertex: the corner records that name it, in the topology's order).  No float atomics, no host synchronisation; the same input gives the
// same bits.  No contraction in this unit (the build's -ffp-contract=off, and the pair function is written with __fmul_rn / __fadd_rn / __fsub_rn); sqrtf is the correctly
// rounded square root, the compiler's default for HIP (__fsqrt_rn is not: the headers map it to the native one).
#include <cmath>
#include <cstdint>
#include <string>

#include "../../../include/psdr_hip.h"
#include "mesh_pair.h"
#include "nn_scan.h"

namespace {

constexpr int kThreads = 256;                   // 4 waves
constexpr int kTile = pm::kTile;                // faces per LDS tile: 12 KiB of records
constexpr int kWideQueries = pm::kWideQueries;  // the plan's queries per lane are 1 or this
static_assert(kThreads == scan::kThreads, "plan_of splits for the scan's workgroup");
constexpr double kInvTwoPi = 0.15915494309189533576888376337251436;

__device__ __forceinline__ float length(Vec p) { return sqrtf(dot(p, p)); }

// THE PAIR FUNCTION: the half solid angle of the face (A, B, C) seen from p, in (-pi, pi]
__device__ __forceinline__ float theta(Vec p, Vec A, Vec B, Vec C) {
    const Vec a = sub(A, p), b = sub(B, p), c = sub(C, p);
    const float la = length(a), lb = length(b), lc = length(c);
    const Vec n = {cross2(b.y, c.z, b.z, c.y), cross2(b.z, c.x, b.x, c.z), cross2(b.x, c.y, b.y, c.x)};
    const float nm = dot(a, n);
    const float dn = __fadd_rn(__fadd_rn(__fmul_rn(__fmul_rn(la, lb), lc), __fmul_rn(dot(a, b), lc)), __fadd_rn(__fmul_rn(dot(b, c), la), __fmul_rn(dot(c, a), lb)));
    const float t = atan2f(nm, dn);                            // (finite for nm == 0 too: a select, not a branch per pair)
    return nm == 0.f ? 0.f : t;
}

// the per-face records of the scan: [F] x three float4 (A, B, C, 0, 0, 0), vertex ids clamped into [0, nv)
__global__ void __launch_bounds__(kThreads) k_records(const float *__restrict__ v, int nv, const int *__restrict__ faces, int nf, float4 *__restrict__ rec) {
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= nf) return;
    const Vec A = load3(v, clamped(faces[3LL * f], nv)), B = load3(v, clamped(faces[3LL * f + 1], nv)), C = load3(v, clamped(faces[3LL * f + 2], nv));
    rec[3LL * f] = make_float4(A.x, A.y, A.z, B.x);
    rec[3LL * f + 1] = make_float4(B.y, B.z, C.x, C.y);
    rec[3LL * f + 2] = make_float4(C.z, 0.f, 0.f, 0.f);
}

// n points against the faces [blockIdx.y slice_len, ...) of m: partial[blockIdx.y][i] = the sum of theta over the slice, added in ascending f
template <int Q> __global__ void __launch_bounds__(kThreads) k_scan(const float *__restrict__ p, const float4 *__restrict__ rec, int n, int m, int slice_len, float *__restrict__ partial) {
    __shared__ float4 s_c[3 * kTile];
    const int j0 = blockIdx.y * slice_len;
    const int j1 = min(m, j0 + slice_len);
    Vec qp[Q];
    double acc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int i = (blockIdx.x * Q + q) * kThreads + threadIdx.x;
        qp[q] = load3(p, min(i, n - 1));                       // (a lane beyond n scans a copy of the last point and stores nothing)
        acc[q] = 0.0;
    }
    for (int base = j0; base < j1; base += kTile) {
        const int count = min(kTile, j1 - base);
        __syncthreads();                                       // (the previous tile has been read)
        for (int t = threadIdx.x; t < 3 * count; t += kThreads) s_c[t] = rec[3LL * base + t];          // (base + count <= m: in range)
        __syncthreads();
        for (int t = 0; t < count; ++t) {
            const float4 r0 = s_c[3 * t], r1 = s_c[3 * t + 1], r2 = s_c[3 * t + 2];
            const Vec A = {r0.x, r0.y, r0.z}, B = {r0.w, r1.x, r1.y}, C = {r1.z, r1.w, r2.x};
#pragma unroll
            for (int q = 0; q < Q; ++q) acc[q] += (double) theta(qp[q], A, B, C);
        }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int i = (blockIdx.x * Q + q) * kThreads + threadIdx.x;
        if (i < n) partial[(size_t) blockIdx.y * (size_t) n + i] = (float) acc[q];
    }
}

// w[i] = (sum over the slices in ascending order, in double) / (2 pi), rounded once; with dist2: sdf[i] = -sqrt(dist2[i]) where orientation w[i] > 1 / 2, else +sqrt(dist2[i])
__global__ void __launch_bounds__(kThreads) k_merge(const float *__restrict__ partial, int n, int slices, const float *__restrict__ dist2, float orientation,
                                                    float *__restrict__ w, float *__restrict__ sdf) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int k = 0; k < slices; ++k) s += (double) partial[(size_t) k * (size_t) n + i];
    const float wi = (float) (s * kInvTwoPi);
    w[i] = wi;
    if (sdf) {
        const float d = sqrtf(dist2[i]);
        sdf[i] = __fmul_rn(orientation, wi) > 0.5f ? -d : d;
    }
}

struct Grad {
    const float *p, *v;
    const int *faces;
    int np, nv, nf;
    const int *face;                    // [np]: a(i)
    const float *bary, *sdf, *g;        // [np, 3], [np], [np]
    const int *f_begin, *f_list;        // [nf + 1], [np]: the points that chose a face, ascending
    const int *vc_begin, *vc_corner;    // [nv + 1], [3 nf]: the corners 3 f + c that name a vertex, ascending
    float *corners, *grad_p, *grad_v;   // [nf, 9], [np, 3], [nv, 3]
};

// (g_i / s_i) r of the pair (point i, face f): r is the point-to-mesh pair function's e = (p - a) - (s ab + t ac) with the stored barycentrics; 0 where s_i == 0
__device__ __forceinline__ Vec pair_term(const Grad &G, int i, int f) {
    const Face face = load_face(G.v, G.nv, G.faces, f);
    const Vec ap = sub(load3(G.p, i), face.a);
    const float s = G.bary[3LL * i + 1], t = G.bary[3LL * i + 2];
    const Vec e = residual(ap, face, s, t);
    const float sd = G.sdf[i];
    const float k = sd == 0.f ? 0.f : __fdiv_rn(G.g[i], sd);
    return {__fmul_rn(k, e.x), __fmul_rn(k, e.y), __fmul_rn(k, e.z)};
}

__global__ void __launch_bounds__(kThreads) k_grad_points(Grad G) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= G.np) return;
    const Vec kr = pair_term(G, i, clamped(G.face[i], G.nf));
    float *o = G.grad_p + 3LL * i;
    o[0] = kr.x;
    o[1] = kr.y;
    o[2] = kr.z;
}

__global__ void __launch_bounds__(kThreads) k_grad_faces(Grad G) {
    const int f = blockIdx.x * kThreads + threadIdx.x;
    if (f >= G.nf) return;
    const int b0 = min(max(G.f_begin[f], 0), G.np), b1 = min(max(G.f_begin[f + 1], b0), G.np);
    float sum[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = b0; k < b1; ++k) {
        const int i = clamped(G.f_list[k], G.np);
        const Vec kr = pair_term(G, i, f);
        const float *b = G.bary + 3LL * i;
#pragma unroll
        for (int c = 0; c < 3; ++c) {          // (mesh_pair.h: add_corners, in place)
            sum[3 * c] = __fadd_rn(sum[3 * c], -__fmul_rn(kr.x, b[c]));
            sum[3 * c + 1] = __fadd_rn(sum[3 * c + 1], -__fmul_rn(kr.y, b[c]));
            sum[3 * c + 2] = __fadd_rn(sum[3 * c + 2], -__fmul_rn(kr.z, b[c]));
        }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) G.corners[9LL * f + k] = sum[k];
}

__global__ void __launch_bounds__(kThreads) k_grad_vertices(Grad G) {
    gather_corners<kThreads>(G);
}

} // namespace

extern "C" {

int psdr_hip_sdf_winding(const float *p, int32_t n_points, const float *v, int32_t n_vertices, const int32_t *faces, int32_t n_faces, float *records, float *partial,
                         const float *dist2, int32_t orientation, float *w, float *sdf, void *stream) {
    const std::string who = "psdr_hip_sdf_winding: ";
    if (!in_range(n_points)) return psdr::api_fail(who + range_text("n_points", n_points));
    if (!in_range(n_vertices)) return psdr::api_fail(who + range_text("n_vertices", n_vertices));
    if (!in_range(n_faces)) return psdr::api_fail(who + range_text("n_faces", n_faces));
    if (orientation != 1 && orientation != -1) return psdr::api_fail(who + "orientation = " + std::to_string(orientation) + ", must be +1 (counter-clockwise seen from outside) or -1");
    if (!p || !v || !faces || !records || !partial || !w) return psdr::api_fail(who + "NULL argument");
    if (!dist2 != !sdf) return psdr::api_fail(who + "dist2 and sdf must both be given or both be NULL");
    const Plan pl = plan_of<kTile, kWideQueries>(n_points, n_faces);
    hipStream_t st = (hipStream_t) stream;
    float4 *rec = reinterpret_cast<float4 *>(records);
    const dim3 grid = scan_grid(n_points, pl);
    k_records<<<blocks_of<kThreads>(n_faces), kThreads, 0, st>>>(v, n_vertices, faces, n_faces, rec);
    if (pl.qpl == 1) k_scan<1><<<grid, kThreads, 0, st>>>(p, rec, n_points, n_faces, pl.slice_len, partial);
    else k_scan<kWideQueries><<<grid, kThreads, 0, st>>>(p, rec, n_points, n_faces, pl.slice_len, partial);
    k_merge<<<blocks_of<kThreads>(n_points), kThreads, 0, st>>>(partial, n_points, pl.slices, dist2, (float) orientation, w, sdf);
    return launch_status(who);
}

int psdr_hip_sdf_grad(const float *p, int32_t n_points, const float *v, int32_t n_vertices, const int32_t *faces, int32_t n_faces, const int32_t *face, const float *bary,
                      const float *sdf, const float *g, const int32_t *f_begin, const int32_t *f_list, const int32_t *vc_begin, const int32_t *vc_corner, float *corners,
                      float *grad_p, float *grad_v, void *stream) {
    const std::string who = "psdr_hip_sdf_grad: ";
    if (!in_range(n_points)) return psdr::api_fail(who + range_text("n_points", n_points));
    if (!in_range(n_vertices)) return psdr::api_fail(who + range_text("n_vertices", n_vertices));
    if (!in_range(n_faces)) return psdr::api_fail(who + range_text("n_faces", n_faces));
    if (!p || !v || !faces || !face || !bary || !sdf || !g || !f_begin || !f_list || !vc_begin || !vc_corner || !corners || !grad_p || !grad_v) return psdr::api_fail(who + "NULL argument");
    if (grad_p == p || grad_p == v || grad_v == p || grad_v == v || grad_p == grad_v || grad_p == g || grad_p == sdf) return psdr::api_fail(who + "grad_p and grad_v must be arrays of their own");
    Grad G;
    G.p = p; G.v = v; G.faces = faces;
    G.np = n_points; G.nv = n_vertices; G.nf = n_faces;
    G.face = face; G.bary = bary; G.sdf = sdf; G.g = g;
    G.f_begin = f_begin; G.f_list = f_list; G.vc_begin = vc_begin; G.vc_corner = vc_corner;
    G.corners = corners; G.grad_p = grad_p; G.grad_v = grad_v;
    hipStream_t st = (hipStream_t) stream;
    k_grad_points<<<blocks_of<kThreads>(n_points), kThreads, 0, st>>>(G);
    k_grad_faces<<<blocks_of<kThreads>(n_faces), kThreads, 0, st>>>(G);
    k_grad_vertices<<<blocks_of<kThreads>(n_vertices), kThreads, 0, st>>>(G);
    return launch_status(who);
}

} // extern "C"
