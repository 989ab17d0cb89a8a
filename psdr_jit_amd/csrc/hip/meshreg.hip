// meshreg.hip — three regularisers of a triangle mesh (uniform Laplacian, normal consistency, edge length) and their gradient with respect to the vertex positions in one
// fused pass (Python surface: psdr_jit_amd/meshreg.py).
//
// The definition (include/psdr_hip.h states it in full).  V float32 [n, 3]; E the distinct undirected edges (a < b), sorted; hinges (a, b, c, d): the edges with exactly two
// faces, c and d the opposite vertices of the first and second face; N(i), deg_i from the Laplacian CSR.
//   laplacian = (1 / n_L) sum_i |delta_i|^2,  delta_i = v_i - (1 / deg_i) sum_{j in N(i)} v_j  (0 at deg_i = 0);  d / dv_k = (2 / n_L) (delta_k - sum_{j in N(k)} delta_j / deg_j)
//   normal    = (1 / h) sum_hinges 1/2 |u1 - u2|^2,  n1 = (b - a) x (c - a), n2 = (d - a) x (b - a), u = n / |n|;  a hinge with |n1|^2 or |n2|^2 < 2^-100 adds nothing
//   edge      = (1 / e) sum_edges (|v_a - v_b| - L0)^2;  L0 == 0: |v_a - v_b|^2, nothing divided;  L0 > 0 and |d|^2 < 2^-100: L0^2 and no gradient
//   loss      = w_lap laplacian + w_nor normal + w_edge edge;  a term of weight 0 is not evaluated
//
// Store, then sum (no scatter, no atomics).  Three launches, two without a gradient:
//   k_elem    one lane per element.  The grid is three runs of whole workgroups - vertices, edges, hinges - so that a workgroup holds one kind of element; the runs of
//             terms that are off are not launched.  A vertex lane writes delta_i and delta_i / deg_i, an edge lane the gradient of its summand with respect to v_a (v_b's
//             is its negative), a hinge lane the gradients of its summand with respect to its four corners.  The workgroup adds its lanes' summands in a fixed order (the
//             wave by shuffles, the four waves in order) into its own partial sum.
//   k_gather  one lane per vertex: delta_k minus its neighbours' delta_j / deg_j through the Laplacian CSR, the edge and hinge contributions through the inverted indices
//             (per vertex the (element, role) pairs in ascending order, built on the host), each sum scaled once, the terms added in the order laplacian, normal, edge.
//             A hub of valence k lengthens its own wave only.  It needs nothing from k_finish.
//   k_finish  one workgroup: the partial sums of each run in a fixed order, the divisions by the counts, out = (loss, laplacian, normal, edge).
// The contributions are float4 (16-byte aligned: one load per gathered vector, never across a cache line).  No host synchronisation, no copy to the host: the same input
// gives the same bits.  No contraction in this unit (the build's -ffp-contract=off): every fma is explicit.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../../include/psdr_hip.h"
#include "op_common.h"

namespace {

constexpr int kThreads = 256;           // k_elem, k_gather: 4 waves
constexpr int kSumThreads = 1024;       // k_finish: one workgroup, 16 waves
constexpr int kMaxCount = 1 << 26;      // n, e, h: 16 h floats and 4 h + 3 packed roles stay below 2^31
constexpr float kTiny = 0x1p-100f;      // a squared length below it: a degenerate hinge or edge

struct Mesh {
    int n, e, h;
    int n_lap;                          // vertices with deg > 0
    const int *row_begin, *col;         // the Laplacian CSR
    const int *edges, *hinges;          // [e][2], [h][4]
    const int *ev_begin, *ev_code;      // per vertex: 2 edge + role (0: a, 1: b), ascending
    const int *hv_begin, *hv_code;      // per vertex: 4 hinge + role (0 .. 3: a, b, c, d), ascending
    float4 *D, *Q;                      // [n]: delta_i, delta_i / deg_i
    float4 *GE;                         // [e]: d summand / d v_a
    float4 *GH;                         // [h][4]: d summand / d corner
    float *partial;                     // one sum per workgroup of k_elem
};

struct Call {
    int blocks_v, blocks_e, blocks_h;   // k_elem's three runs; 0: the term is off (weight 0, or nothing to sum)
    float w_lap, w_nor, w_edge;
    float s_lap, s_nor, s_edge;         // the gradient's scales: 2 w_lap / n_L, w_nor / h, w_edge / e
    float L0;
};

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 load3(const float *p) { return V3{p[0], p[1], p[2]}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator*(float s, V3 a) { return V3{s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ V3 operator/(V3 a, float s) { return V3{a.x / s, a.y / s, a.z / s}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
// a b - c d with the rounding error of c d given back (Kahan): a cross product of nearly parallel vectors keeps its digits
__device__ __forceinline__ float dop(float a, float b, float c, float d) {
    const float w = c * d, err = fmaf(-c, d, w);
    return fmaf(a, b, -w) + err;
}
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return V3{dop(a.y, b.z, a.z, b.y), dop(a.z, b.x, a.x, b.z), dop(a.x, b.y, a.y, b.x)}; }
__device__ __forceinline__ float4 f4(V3 a) { return make_float4(a.x, a.y, a.z, 0.f); }

__device__ __forceinline__ float vertex_elem(const Mesh &M, const float *__restrict__ v, int i) {
    const int b0 = M.row_begin[i], b1 = M.row_begin[i + 1];
    V3 delta{0.f, 0.f, 0.f}, q{0.f, 0.f, 0.f};
    if (b1 > b0) {
        V3 s{0.f, 0.f, 0.f};
#pragma unroll 4
        for (int k = b0; k < b1; ++k) s = s + load3(v + 3LL * M.col[k]);
        const float deg = (float) (b1 - b0);
        delta = load3(v + 3LL * i) - s / deg;
        q = delta / deg;
    }
    M.D[i] = f4(delta);
    M.Q[i] = f4(q);
    return dot(delta, delta);
}

__device__ __forceinline__ float edge_elem(const Mesh &M, const float *__restrict__ v, int k, float L0) {
    const int a = M.edges[2LL * k], b = M.edges[2LL * k + 1];
    const V3 d = load3(v + 3LL * a) - load3(v + 3LL * b);
    const float l2 = dot(d, d);
    float val;
    V3 g;
    if (L0 == 0.f) {
        val = l2;
        g = 2.f * d;
    } else if (l2 < kTiny) {
        val = L0 * L0;
        g = V3{0.f, 0.f, 0.f};
    } else {
        const float l = sqrtf(l2), r = l - L0;
        val = r * r;
        g = ((2.f * r) / l) * d;
    }
    M.GE[k] = f4(g);
    return val;
}

__device__ __forceinline__ float hinge_elem(const Mesh &M, const float *__restrict__ v, int k) {
    const int4 id = reinterpret_cast<const int4 *>(M.hinges)[k];
    const V3 pa = load3(v + 3LL * id.x);
    const V3 e0 = load3(v + 3LL * id.y) - pa, p = load3(v + 3LL * id.z) - pa, q = load3(v + 3LL * id.w) - pa;
    const V3 n1 = cross(e0, p), n2 = cross(q, e0);
    const float l1 = dot(n1, n1), l2 = dot(n2, n2);
    float val = 0.f;
    V3 ga{0.f, 0.f, 0.f}, gb = ga, gc = ga, gd = ga;
    if (!(l1 < kTiny) && !(l2 < kTiny)) {
        const float r1 = sqrtf(l1), r2 = sqrtf(l2);
        const V3 u1 = n1 / r1, u2 = n2 / r2, w = u1 - u2;
        val = 0.5f * dot(w, w);
        // d/dn1 = P1 w / |n1|, d/dn2 = -P2 w / |n2|, P = I - u u^T: written on w, so that a flat hinge loses no digits
        const float c1 = dot(u1, w), c2 = dot(u2, w);
        const V3 g1 = V3{fmaf(-c1, u1.x, w.x), fmaf(-c1, u1.y, w.y), fmaf(-c1, u1.z, w.z)} / r1;
        const V3 g2 = V3{fmaf(-c2, u2.x, w.x), fmaf(-c2, u2.y, w.y), fmaf(-c2, u2.z, w.z)} / (-r2);
        gb = cross(p, g1) + cross(g2, q);
        gc = cross(g1, e0);
        gd = cross(e0, g2);
        ga = V3{0.f, 0.f, 0.f} - ((gb + gc) + gd);
    }
    float4 *o = M.GH + 4LL * k;
    o[0] = f4(ga);
    o[1] = f4(gb);
    o[2] = f4(gc);
    o[3] = f4(gd);
    return val;
}

__global__ void __launch_bounds__(kThreads) k_elem(Mesh M, Call c, const float *__restrict__ v) {
    __shared__ float s_red[kThreads / 64];
    // the workgroup's kind is uniform: which of the three runs it lies in
    int blk = blockIdx.x;
    float val = 0.f;
    if (blk < c.blocks_v) {
        const int i = blk * kThreads + threadIdx.x;
        if (i < M.n) val = vertex_elem(M, v, i);
    } else if ((blk -= c.blocks_v) < c.blocks_e) {
        const int k = blk * kThreads + threadIdx.x;
        if (k < M.e) val = edge_elem(M, v, k, c.L0);
    } else {
        blk -= c.blocks_e;
        const int k = blk * kThreads + threadIdx.x;
        if (k < M.h) val = hinge_elem(M, v, k);
    }
    const float t = block_sum<kThreads>(val, s_red);
    if (threadIdx.x == 0) M.partial[blockIdx.x] = t;
}

__device__ __forceinline__ void add4(V3 &s, const float4 g) { s.x += g.x; s.y += g.y; s.z += g.z; }

__global__ void __launch_bounds__(kThreads) k_gather(Mesh M, Call c, float *__restrict__ grad) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= M.n) return;
    V3 g{0.f, 0.f, 0.f};
    bool have = false;
    if (c.blocks_v) {
        V3 s{0.f, 0.f, 0.f};
        const int b1 = M.row_begin[i + 1];
#pragma unroll 4
        for (int k = M.row_begin[i]; k < b1; ++k) add4(s, M.Q[M.col[k]]);
        const float4 d = M.D[i];
        g = c.s_lap * (V3{d.x, d.y, d.z} - s);
        have = true;
    }
    if (c.blocks_h) {
        V3 s{0.f, 0.f, 0.f};
        const int b1 = M.hv_begin[i + 1];
#pragma unroll 4
        for (int k = M.hv_begin[i]; k < b1; ++k) add4(s, M.GH[M.hv_code[k]]);
        const V3 t = c.s_nor * s;
        g = have ? g + t : t;
        have = true;
    }
    if (c.blocks_e) {
        V3 s{0.f, 0.f, 0.f};
        const int b1 = M.ev_begin[i + 1];
#pragma unroll 4
        for (int k = M.ev_begin[i]; k < b1; ++k) {
            const int code = M.ev_code[k];
            const float4 ge = M.GE[code >> 1];
            if (code & 1) { s.x -= ge.x; s.y -= ge.y; s.z -= ge.z; } else add4(s, ge);
        }
        const V3 t = c.s_edge * s;
        g = have ? g + t : t;
    }
    float *o = grad + 3LL * i;
    o[0] = g.x;
    o[1] = g.y;
    o[2] = g.z;
}

// a lane adds every 1024th partial sum of a run in ascending order, then the workgroup's fixed order
__device__ float run_sum(const float *p, int count, float *s_red) {
    float a = 0.f;
    for (int t = threadIdx.x; t < count; t += kSumThreads) a += p[t];
    return block_sum<kSumThreads>(a, s_red);
}

__global__ void __launch_bounds__(kSumThreads) k_finish(Mesh M, Call c, float *__restrict__ out) {
    __shared__ float s_red[kSumThreads / 64];
    const float sv = run_sum(M.partial, c.blocks_v, s_red);
    const float se = run_sum(M.partial + c.blocks_v, c.blocks_e, s_red);
    const float sh = run_sum(M.partial + c.blocks_v + c.blocks_e, c.blocks_h, s_red);
    if (threadIdx.x == 0) {
        const float lap = c.blocks_v ? sv / (float) M.n_lap : 0.f;
        const float nor = c.blocks_h ? sh / (float) M.h : 0.f;
        const float edge = c.blocks_e ? se / (float) M.e : 0.f;
        float loss = 0.f;
        bool have = false;
        if (c.blocks_v) { loss = c.w_lap * lap; have = true; }
        if (c.blocks_h) { const float t = c.w_nor * nor; loss = have ? loss + t : t; have = true; }
        if (c.blocks_e) { const float t = c.w_edge * edge; loss = have ? loss + t : t; }
        out[0] = loss;
        out[1] = lap;
        out[2] = nor;
        out[3] = edge;
    }
}

// the host-side check of one per-vertex list of (element, role) pairs against the element table it inverts: "" or what is wrong with it
std::string check_index(const char *name, int32_t n, int32_t count, int32_t roles, const int32_t *table, const int32_t *begin, const int32_t *elem, const int32_t *role) {
    const std::string s(name);
    if (!begin) return s + "begin is NULL";
    if (begin[0] != 0) return s + "begin[0] = " + std::to_string(begin[0]) + ", must be 0";
    for (int32_t i = 0; i < n; ++i)
        if (begin[i + 1] < begin[i]) return s + "begin is not monotonic at vertex " + std::to_string(i);
    const long long want = (long long) roles * count;
    if (begin[n] != want) return s + "begin ends at " + std::to_string(begin[n]) + " entries, must be " + std::to_string(want) + " (" + std::to_string(roles) + " per element)";
    if (want > 0 && (!elem || !role)) return s + (elem ? "role" : "elem") + " is NULL";
    for (int32_t i = 0; i < n; ++i)
        for (int32_t k = begin[i]; k < begin[i + 1]; ++k) {
            if (elem[k] < 0 || elem[k] >= count)
                return s + "elem[" + std::to_string(k) + "] = " + std::to_string(elem[k]) + " of vertex " + std::to_string(i) + " is outside [0, " + std::to_string(count) + ")";
            if (role[k] < 0 || role[k] >= roles)
                return s + "role[" + std::to_string(k) + "] = " + std::to_string(role[k]) + " of vertex " + std::to_string(i) + " is outside [0, " + std::to_string(roles) + ")";
            if (table[(long long) roles * elem[k] + role[k]] != i)
                return s + "entry " + std::to_string(k) + " of vertex " + std::to_string(i) + " names element " + std::to_string(elem[k]) + ", role " + std::to_string(role[k]) +
                       ", which is vertex " + std::to_string(table[(long long) roles * elem[k] + role[k]]);
            if (k > begin[i] && (long long) elem[k] * roles + role[k] <= (long long) elem[k - 1] * roles + role[k - 1])
                return s + "the entries of vertex " + std::to_string(i) + " are not in ascending order at entry " + std::to_string(k);
        }
    return "";
}

} // namespace

struct psdr_hip_meshreg {
    Mesh M{};
    int *d_ints = nullptr;             // row_begin | ev_begin | hv_begin | col | edges | ev_code | hinges | hv_code
    float4 *d_vec = nullptr;           // D | Q | GE | GH
    float *d_partial = nullptr;
    ~psdr_hip_meshreg() {
        if (d_ints) (void) hipFree(d_ints);
        if (d_vec) (void) hipFree(d_vec);
        if (d_partial) (void) hipFree(d_partial);
    }
};

extern "C" {

int psdr_hip_meshreg_create(int32_t n, int32_t e, int32_t h, const int32_t *edges, const int32_t *hinges, const int32_t *row_begin, const int32_t *col,
                            const int32_t *ev_begin, const int32_t *ev_elem, const int32_t *ev_role, const int32_t *hv_begin, const int32_t *hv_elem, const int32_t *hv_role,
                            psdr_hip_meshreg **out, void *stream) {
    const std::string who = "psdr_hip_meshreg_create: ";
    if (!out) return psdr::api_fail(who + "out is NULL");
    *out = nullptr;
    if (n <= 0 || n > kMaxCount) return psdr::api_fail(who + "n = " + std::to_string(n) + ", must lie in [1, 2^26]");
    if (e < 0 || e > kMaxCount) return psdr::api_fail(who + "e = " + std::to_string(e) + ", must lie in [0, 2^26]");
    if (h < 0 || h > kMaxCount) return psdr::api_fail(who + "h = " + std::to_string(h) + ", must lie in [0, 2^26]");
    if (e > 0 && !edges) return psdr::api_fail(who + "edges is NULL");
    if (h > 0 && !hinges) return psdr::api_fail(who + "hinges is NULL");
    for (int32_t k = 0; k < e; ++k) {
        const int32_t a = edges[2LL * k], b = edges[2LL * k + 1];
        if (a < 0 || b >= n || a >= b)
            return psdr::api_fail(who + "edge " + std::to_string(k) + " = (" + std::to_string(a) + ", " + std::to_string(b) + "), must be 0 <= a < b < " + std::to_string(n));
    }
    for (int32_t k = 0; k < h; ++k) {
        const int32_t *q = hinges + 4LL * k;
        for (int r = 0; r < 4; ++r)
            if (q[r] < 0 || q[r] >= n)
                return psdr::api_fail(who + "hinge " + std::to_string(k) + " names vertex " + std::to_string(q[r]) + ", which is outside [0, " + std::to_string(n) + ")");
        if (q[0] >= q[1] || q[2] == q[0] || q[2] == q[1] || q[3] == q[0] || q[3] == q[1])
            return psdr::api_fail(who + "hinge " + std::to_string(k) + " = (" + std::to_string(q[0]) + ", " + std::to_string(q[1]) + ", " + std::to_string(q[2]) + ", " + std::to_string(q[3]) +
                                  "): its edge must be a < b and its opposite vertices off the edge");
    }
    if (!row_begin) return psdr::api_fail(who + "row_begin is NULL");
    if (row_begin[0] != 0) return psdr::api_fail(who + "row_begin[0] = " + std::to_string(row_begin[0]) + ", must be 0");
    for (int32_t i = 0; i < n; ++i)
        if (row_begin[i + 1] < row_begin[i]) return psdr::api_fail(who + "row_begin is not monotonic at row " + std::to_string(i));
    const int32_t nnz = row_begin[n];
    if (nnz > 0 && !col) return psdr::api_fail(who + "col is NULL");
    int32_t n_lap = 0;
    for (int32_t i = 0; i < n; ++i) {
        n_lap += row_begin[i + 1] > row_begin[i];
        for (int32_t k = row_begin[i]; k < row_begin[i + 1]; ++k)
            if (col[k] < 0 || col[k] >= n || col[k] == i)
                return psdr::api_fail(who + "col[" + std::to_string(k) + "] = " + std::to_string(col[k]) + " of row " + std::to_string(i) + " is outside [0, " + std::to_string(n) + ") or the row itself");
    }
    std::string bad = check_index("ev_", n, e, 2, edges, ev_begin, ev_elem, ev_role);
    if (!bad.empty()) return psdr::api_fail(who + bad);
    bad = check_index("hv_", n, h, 4, hinges, hv_begin, hv_elem, hv_role);
    if (!bad.empty()) return psdr::api_fail(who + bad);
    // the lists are sound: from here on the device is touched
    hipStream_t s = (hipStream_t) stream;
    psdr_hip_meshreg *m = new psdr_hip_meshreg();
    const size_t rb = (size_t) n + 1, z = (size_t) nnz, e2 = 2 * (size_t) e, h4 = 4 * (size_t) h;
    // hinges first among the tables: its rows are read as int4, and hipMalloc's base is aligned
    std::vector<int32_t> ints(h4 + 3 * rb + z + 2 * e2 + h4);
    size_t o_hinges = 0, o_rb = h4, o_evb = o_rb + rb, o_hvb = o_evb + rb, o_col = o_hvb + rb, o_edges = o_col + z, o_evc = o_edges + e2, o_hvc = o_evc + e2;
    for (size_t k = 0; k < h4; ++k) ints[o_hinges + k] = hinges[k];
    for (size_t k = 0; k < rb; ++k) { ints[o_rb + k] = row_begin[k]; ints[o_evb + k] = ev_begin[k]; ints[o_hvb + k] = hv_begin[k]; }
    for (size_t k = 0; k < z; ++k) ints[o_col + k] = col[k];
    for (size_t k = 0; k < e2; ++k) { ints[o_edges + k] = edges[k]; ints[o_evc + k] = 2 * ev_elem[k] + ev_role[k]; }
    for (size_t k = 0; k < h4; ++k) ints[o_hvc + k] = 4 * hv_elem[k] + hv_role[k];
    const size_t n_vec = 2 * (size_t) n + (size_t) e + h4, n_part = (size_t) blocks_of<kThreads>(n) + blocks_of<kThreads>(e) + blocks_of<kThreads>(h);
    hipError_t err = hipMalloc((void **) &m->d_ints, ints.size() * sizeof(int32_t));
    if (err == hipSuccess) err = hipMalloc((void **) &m->d_vec, n_vec * sizeof(float4));
    if (err == hipSuccess) err = hipMalloc((void **) &m->d_partial, n_part * sizeof(float));
    if (err == hipSuccess) err = hipMemcpyAsync(m->d_ints, ints.data(), ints.size() * sizeof(int32_t), hipMemcpyHostToDevice, s);
    if (err == hipSuccess) err = hipStreamSynchronize(s);        // the staging array goes away with this call; every eval writes the work frames it reads
    if (err != hipSuccess) { delete m; return psdr::api_fail(who + hipGetErrorString(err)); }
    Mesh &M = m->M;
    M.n = n; M.e = e; M.h = h; M.n_lap = n_lap;
    M.hinges = m->d_ints + o_hinges;
    M.row_begin = m->d_ints + o_rb; M.ev_begin = m->d_ints + o_evb; M.hv_begin = m->d_ints + o_hvb;
    M.col = m->d_ints + o_col; M.edges = m->d_ints + o_edges; M.ev_code = m->d_ints + o_evc; M.hv_code = m->d_ints + o_hvc;
    M.D = m->d_vec; M.Q = M.D + n; M.GE = M.Q + n; M.GH = M.GE + e;
    M.partial = m->d_partial;
    *out = m;
    return 0;
}

int psdr_hip_meshreg_destroy(psdr_hip_meshreg *m) {
    if (!m) return psdr::api_fail("psdr_hip_meshreg_destroy: handle is NULL");
    delete m;
    return 0;
}

int psdr_hip_meshreg_eval(psdr_hip_meshreg *m, const float *v, const float *weights, float target_length, float *out, float *grad, void *stream) {
    const std::string who = "psdr_hip_meshreg_eval: ";
    if (!m) return psdr::api_fail(who + "handle is NULL");
    if (!v || !weights || !out) return psdr::api_fail(who + "NULL argument");
    if (grad && grad == v) return psdr::api_fail(who + "grad must be an array of its own, not v");
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(weights[k]) || weights[k] < 0.f) return psdr::api_fail(who + "weights[" + std::to_string(k) + "] = " + std::to_string(weights[k]) + ", must be finite and not negative");
    if (!std::isfinite(target_length) || target_length < 0.f) return psdr::api_fail(who + "target_length = " + std::to_string(target_length) + ", must be finite and not negative");
    const Mesh &M = m->M;
    Call c{};
    c.w_lap = weights[0]; c.w_nor = weights[1]; c.w_edge = weights[2];
    c.L0 = target_length;
    c.blocks_v = c.w_lap > 0.f && M.n_lap > 0 ? blocks_of<kThreads>(M.n) : 0;
    c.blocks_h = c.w_nor > 0.f ? blocks_of<kThreads>(M.h) : 0;
    c.blocks_e = c.w_edge > 0.f ? blocks_of<kThreads>(M.e) : 0;
    c.s_lap = c.blocks_v ? (float) (2.0 * (double) c.w_lap / (double) M.n_lap) : 0.f;
    c.s_nor = c.blocks_h ? (float) ((double) c.w_nor / (double) M.h) : 0.f;
    c.s_edge = c.blocks_e ? (float) ((double) c.w_edge / (double) M.e) : 0.f;
    hipStream_t st = (hipStream_t) stream;
    const int blocks = c.blocks_v + c.blocks_e + c.blocks_h;
    if (blocks) k_elem<<<blocks, kThreads, 0, st>>>(M, c, v);
    if (grad) k_gather<<<blocks_of<kThreads>(M.n), kThreads, 0, st>>>(M, c, grad);
    k_finish<<<1, kSumThreads, 0, st>>>(M, c, out);
    return launch_status(who);
}

} // extern "C"
