// chamfer.hip — the Chamfer distance between two point sets: the exact nearest neighbour of every point in the other set by a brute-force scan, the loss and its gradient
// with respect to both sets (Python surface: psdr_jit_amd/chamfer.py).
//
// The definition (include/psdr_hip.h states it in full).  x float32 [n, 3], y float32 [m, 3], 1 <= n, m <= 2^26.
//   d2(i, j)    = (dx dx + dy dy) + dz dz,  dx = x_i0 - y_j0 ...: the difference form, every operation one float32 rounding, nothing fused
//   a(i)        = the lowest j that minimises d2(i, j);  dist2_xy[i] = d2(i, a(i));  b(j), dist2_yx[j]: the same with the roles swapped
//   loss        = w_xy (1 / n) sum_i rho(dist2_xy[i]) + w_yx (1 / m) sum_j rho(dist2_yx[j]);  rho(s) = s (squared) or sqrt(s), whose derivative at 0 is defined as 0
//   d / dx_i    = k_xy(dist2_xy[i]) (x_i - y_a(i)) + sum over {j : b(j) = i}, ascending j, of k_yx(dist2_yx[j]) (x_i - y_j);  k(s) = 2 w / count (squared) or
//                 (w / count) / sqrt(s), 0 at s = 0;  y_j receives the mirror image.  The indices are constants.
//
// The scan (k_scan<Q>).  A lane holds Q queries in registers; the candidates of the workgroup's slice go through LDS a tile at a time as x / y / z planes, and every lane
// reads the same float4 of a plane: a broadcast, four candidates per read, each serving the lane's Q queries.  A lane walks its candidates in ascending j and replaces its
// best on a strict `<`, which is the tie rule inside a slice; the best leaves the lane as the 64-bit key (float bits of d2) << 32 | j - d2 >= +0, so keys order as
// unsigned integers - and the slices are merged by one integer minimum per query (atomicMin on the key array: an integer minimum is associative and commutative, the
// result does not depend on the order).  With one slice the key is stored.  The grid is query blocks x candidate slices (psdr_hip_chamfer_plan): 10 000 queries alone
// are 10 workgroups on 256 CUs.  A partial last tile is padded with +infinity coordinates: d2 = +inf never passes `<`.  A d2 that is NaN never passes it either, so with
// non-finite inputs the index stays the slice's first candidate: in range.
// The evaluation (k_eval, one launch per point set): a lane per point - its own term from (index, dist2), then the points of the other set that chose it through the
// inverted index (per point the j in ascending order, built by the caller with a stable sort), one store of the gradient, no atomics; the workgroup adds rho(dist2) in a
// fixed order into its partial sum (in double, so that the mean carries one rounding).  k_finish: one workgroup adds the partial sums of each direction in a fixed order.
// The grid search (psdr_hip_chamfer_grid_*; kernels and plan: nn_grid.h): the same index and dist2, bit for bit, after testing only the candidates
// of the cells round a query; offered beside the scan, which stays as it is.
// No host synchronisation; the same input gives the same bits.  No contraction in this unit (the build's -ffp-contract=off, and the distance is written with __fmul_rn / __fadd_rn).
#include <cmath>
#include <cstdint>
#include <string>

#include "../../../include/psdr_hip.h"
#include "nn_scan.h"
#include "nn_grid.h"

namespace {

constexpr int kThreads = 256;           // 4 waves
constexpr int kSumThreads = 1024;       // k_finish: one workgroup, 16 waves
constexpr int kTile = 1024;             // candidates per LDS tile: three planes of 4 KiB
constexpr int kWideQueries = 4;         // queries per lane of the wide scan
static_assert(kThreads == scan::kThreads, "plan_of splits for the scan's workgroup");

template <int Q> __global__ void __launch_bounds__(kThreads) k_scan(const float *__restrict__ x, int n, const float *__restrict__ y, int m, int slice_len, int slices,
                                                                    unsigned long long *__restrict__ keys) {
    __shared__ float4 s_c[3][kTile / 4];
    float *s_x = reinterpret_cast<float *>(s_c[0]), *s_y = reinterpret_cast<float *>(s_c[1]), *s_z = reinterpret_cast<float *>(s_c[2]);
    const int j0 = blockIdx.y * slice_len;
    const int j1 = min(m, j0 + slice_len);
    float qx[Q], qy[Q], qz[Q], best[Q];
    int bj[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int i = (blockIdx.x * Q + q) * kThreads + threadIdx.x;
        const bool live = i < n;
        qx[q] = live ? x[3LL * i] : 0.f;
        qy[q] = live ? x[3LL * i + 1] : 0.f;
        qz[q] = live ? x[3LL * i + 2] : 0.f;
        best[q] = INFINITY;
        bj[q] = j0;
    }
    for (int base = j0; base < j1; base += kTile) {
        __syncthreads();                                       // (the previous tile has been read)
        for (int t = threadIdx.x; t < kTile; t += kThreads) {
            const int j = base + t;
            const bool live = j < j1;
            s_x[t] = live ? y[3LL * j] : INFINITY;
            s_y[t] = live ? y[3LL * j + 1] : INFINITY;
            s_z[t] = live ? y[3LL * j + 2] : INFINITY;
        }
        __syncthreads();
        const int groups = (min(kTile, j1 - base) + 3) >> 2;
        for (int g = 0; g < groups; ++g) {
            const float4 cx = s_c[0][g], cy = s_c[1][g], cz = s_c[2][g];
            const float ax[4] = {cx.x, cx.y, cx.z, cx.w}, ay[4] = {cy.x, cy.y, cy.z, cy.w}, az[4] = {cz.x, cz.y, cz.z, cz.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = base + 4 * g + u;
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const float d2 = pair_d2(qx[q], qy[q], qz[q], ax[u], ay[u], az[u]);
                    if (d2 < best[q]) { best[q] = d2; bj[q] = j; }
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

__global__ void __launch_bounds__(kThreads) k_unpack(const unsigned long long *__restrict__ keys, int n, int m, int *__restrict__ idx, float *__restrict__ dist2) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = keys[i];
    idx[i] = key_index(key, m);
    dist2[i] = key_dist2(key);
}

// one point set p [n, 3] against the other set o [m, 3]
struct Side {
    const float *p, *o;
    int n, m;
    const int *idx;                     // [n] the point's nearest in o, or NULL: its own direction is off
    const float *dist2;                 // [n]
    const int *inv_begin, *inv_list;    // [n + 1], [m]: the points of o that chose this one, ascending, or NULL: the other direction is off
    const float *o_dist2;               // [m] their squared distances
    float k_own, k_inv;                 // squared: 2 w / count; else w / count (divided by sqrt(s) per point)
    float *grad;                        // [n, 3] or NULL
    double *partial;                    // one sum per workgroup (only when idx)
};

__global__ void __launch_bounds__(kThreads) k_eval(Side S, int squared) {
    __shared__ double s_red[kThreads / 64];
    const int i = blockIdx.x * kThreads + threadIdx.x;
    float val = 0.f;
    if (i < S.n) {
        const float px = S.p[3LL * i], py = S.p[3LL * i + 1], pz = S.p[3LL * i + 2];
        float gx = 0.f, gy = 0.f, gz = 0.f;
        bool have = false;
        if (S.idx) {
            const float s = S.dist2[i];
            val = squared ? s : sqrtf(s);
            if (S.grad) {
                const int a = min(max(S.idx[i], 0), S.m - 1);
                const float k = coefficient(S.k_own, s, squared);
                gx = k * (px - S.o[3LL * a]);
                gy = k * (py - S.o[3LL * a + 1]);
                gz = k * (pz - S.o[3LL * a + 2]);
                have = true;
            }
        }
        if (S.inv_begin && S.grad) {
            const int b0 = min(max(S.inv_begin[i], 0), S.m), b1 = min(max(S.inv_begin[i + 1], b0), S.m);
            float sx = 0.f, sy = 0.f, sz = 0.f;
#pragma unroll 4
            for (int t = b0; t < b1; ++t) {
                const int j = min(max(S.inv_list[t], 0), S.m - 1);
                const float k = coefficient(S.k_inv, S.o_dist2[j], squared);
                sx += k * (px - S.o[3LL * j]);
                sy += k * (py - S.o[3LL * j + 1]);
                sz += k * (pz - S.o[3LL * j + 2]);
            }
            gx = have ? gx + sx : sx;
            gy = have ? gy + sy : sy;
            gz = have ? gz + sz : sz;
        }
        if (S.grad) {
            float *g = S.grad + 3LL * i;
            g[0] = gx;
            g[1] = gy;
            g[2] = gz;
        }
    }
    if (S.idx) {                                            // (uniform over the launch)
        const double t = block_sum<kThreads>((double) val, s_red);
        if (threadIdx.x == 0) S.partial[blockIdx.x] = t;
    }
}

__global__ void __launch_bounds__(kSumThreads) k_finish(const double *__restrict__ partial, int blocks_x, int blocks_y, int n, int m, float w_xy, float w_yx, float *__restrict__ out) {
    __shared__ double s_red[kSumThreads / 64];
    finish_two<kSumThreads>(partial, blocks_x, blocks_y, n, m, w_xy, w_yx, out, s_red);
}

} // namespace

extern "C" {

int psdr_hip_chamfer_plan(int32_t n, int32_t m, int32_t *tile, int32_t *queries_per_lane, int32_t *slices, int32_t *slice_len) {
    const std::string who = "psdr_hip_chamfer_plan: ";
    if (!in_range(n)) return psdr::api_fail(who + range_text("n", n));
    if (!in_range(m)) return psdr::api_fail(who + range_text("m", m));
    if (!tile || !queries_per_lane || !slices || !slice_len) return psdr::api_fail(who + "NULL argument");
    const Plan p = plan_of<kTile, kWideQueries>(n, m);
    *tile = p.tile;
    *queries_per_lane = p.qpl;
    *slices = p.slices;
    *slice_len = p.slice_len;
    return 0;
}

int psdr_hip_chamfer_nearest(const float *x, int32_t n, const float *y, int32_t m, uint64_t *keys, int32_t *index, float *dist2, void *stream) {
    const std::string who = "psdr_hip_chamfer_nearest: ";
    if (!in_range(n)) return psdr::api_fail(who + range_text("n", n));
    if (!in_range(m)) return psdr::api_fail(who + range_text("m", m));
    if (!x || !y || !keys || !index || !dist2) return psdr::api_fail(who + "NULL argument");
    const Plan p = plan_of<kTile, kWideQueries>(n, m);
    hipStream_t st = (hipStream_t) stream;
    unsigned long long *k = reinterpret_cast<unsigned long long *>(keys);
    const hipError_t e = clear_keys(k, n, p, st);
    if (e != hipSuccess) return psdr::api_fail(who + hipGetErrorString(e));
    const dim3 grid = scan_grid(n, p);
    if (p.qpl == 1) k_scan<1><<<grid, kThreads, 0, st>>>(x, n, y, m, p.slice_len, p.slices, k);
    else k_scan<kWideQueries><<<grid, kThreads, 0, st>>>(x, n, y, m, p.slice_len, p.slices, k);
    k_unpack<<<blocks_of<kThreads>(n), kThreads, 0, st>>>(k, n, m, index, dist2);
    return launch_status(who);
}

int psdr_hip_chamfer_eval(const float *x, int32_t n, const float *y, int32_t m, const int32_t *index_xy, const float *dist2_xy, const int32_t *index_yx, const float *dist2_yx,
                          const int32_t *x_begin, const int32_t *x_list, const int32_t *y_begin, const int32_t *y_list, const float *weights, int32_t squared,
                          double *partial, float *out, float *grad_x, float *grad_y, void *stream) {
    const std::string who = "psdr_hip_chamfer_eval: ";
    if (!in_range(n)) return psdr::api_fail(who + range_text("n", n));
    if (!in_range(m)) return psdr::api_fail(who + range_text("m", m));
    if (!x || !y || !weights || !partial || !out) return psdr::api_fail(who + "NULL argument");
    for (int k = 0; k < 2; ++k)
        if (!std::isfinite(weights[k]) || weights[k] < 0.f) return psdr::api_fail(who + "weights[" + std::to_string(k) + "] = " + std::to_string(weights[k]) + ", must be finite and not negative");
    if (!grad_x != !grad_y) return psdr::api_fail(who + "grad_x and grad_y must both be given or both be NULL");
    if (grad_x && (grad_x == x || grad_x == y || grad_y == x || grad_y == y || grad_x == grad_y)) return psdr::api_fail(who + "grad_x and grad_y must be arrays of their own");
    const bool on_xy = weights[0] > 0.f, on_yx = weights[1] > 0.f;
    if (on_xy && (!index_xy || !dist2_xy)) return psdr::api_fail(who + "weights[0] > 0 needs index_xy and dist2_xy");
    if (on_yx && (!index_yx || !dist2_yx)) return psdr::api_fail(who + "weights[1] > 0 needs index_yx and dist2_yx");
    if (grad_x && on_xy && (!y_begin || !y_list)) return psdr::api_fail(who + "the gradient of the x -> y term needs y_begin and y_list, the inverted index of index_xy");
    if (grad_x && on_yx && (!x_begin || !x_list)) return psdr::api_fail(who + "the gradient of the y -> x term needs x_begin and x_list, the inverted index of index_yx");
    const double unit = squared ? 2.0 : 1.0;
    const float k_xy = (float) (unit * (double) weights[0] / (double) n), k_yx = (float) (unit * (double) weights[1] / (double) m);
    const int bx = on_xy ? blocks_of<kThreads>(n) : 0, by = on_yx ? blocks_of<kThreads>(m) : 0;
    hipStream_t st = (hipStream_t) stream;
    Side X{x, y, n, m, on_xy ? index_xy : nullptr, dist2_xy, on_yx ? x_begin : nullptr, x_list, dist2_yx, k_xy, k_yx, grad_x, partial};
    Side Y{y, x, m, n, on_yx ? index_yx : nullptr, dist2_yx, on_xy ? y_begin : nullptr, y_list, dist2_xy, k_yx, k_xy, grad_y, partial + bx};
    if (on_xy || grad_x) k_eval<<<blocks_of<kThreads>(n), kThreads, 0, st>>>(X, squared ? 1 : 0);
    if (on_yx || grad_y) k_eval<<<blocks_of<kThreads>(m), kThreads, 0, st>>>(Y, squared ? 1 : 0);
    k_finish<<<1, kSumThreads, 0, st>>>(partial, bx, by, n, m, weights[0], weights[1], out);
    return launch_status(who);
}

int psdr_hip_chamfer_grid_plan(int32_t n, int32_t m, int32_t *res, int32_t *max_shells, int64_t *cells, int64_t *planes_at, int64_t *begin_at, int64_t *points_at,
                               int64_t *grid_words, int64_t *work_words, int32_t *fallback_groups, int32_t *fallback_slices, int32_t *fallback_slice_len, int32_t *lanes_per_query) {
    const std::string who = "psdr_hip_chamfer_grid_plan: ";
    if (!in_range(n)) return psdr::api_fail(who + range_text("n", n));
    if (!in_range(m)) return psdr::api_fail(who + range_text("m", m));
    if (!res || !max_shells || !cells || !planes_at || !begin_at || !points_at || !grid_words || !work_words || !fallback_groups || !fallback_slices || !fallback_slice_len || !lanes_per_query)
        return psdr::api_fail(who + "NULL argument");
    const grid::GridPlan p = grid::grid_plan_of(n, m);
    *res = p.res;
    *max_shells = p.max_shells;
    *cells = p.cells;
    *planes_at = p.planes_at;
    *begin_at = p.begin_at;
    *points_at = p.points_at;
    *grid_words = p.grid_words;
    *work_words = p.work_words;
    *fallback_groups = p.fb_groups;
    *fallback_slices = p.fb_slices;
    *fallback_slice_len = p.fb_slice_len;
    *lanes_per_query = p.lanes;
    return 0;
}

int psdr_hip_chamfer_grid_build(const float *y, int32_t m, uint32_t *grid_blob, int64_t grid_words, int32_t *work, int64_t work_words, void *stream) {
    const std::string who = "psdr_hip_chamfer_grid_build: ";
    if (!in_range(m)) return psdr::api_fail(who + range_text("m", m));
    if (!y || !grid_blob || !work) return psdr::api_fail(who + "NULL argument");
    const grid::GridPlan p = grid::grid_plan_of(1, m);
    if (grid_words < p.grid_words) return psdr::api_fail(who + "grid_words = " + std::to_string(grid_words) + ", the plan of m = " + std::to_string(m) + " needs " + std::to_string(p.grid_words));
    if (work_words < p.work_words) return psdr::api_fail(who + "work_words = " + std::to_string(work_words) + ", the plan of m = " + std::to_string(m) + " needs " + std::to_string(p.work_words));
    hipStream_t st = (hipStream_t) stream;
    unsigned int *g = grid_blob, *box_keys = reinterpret_cast<unsigned int *>(work);
    int *begin = reinterpret_cast<int *>(grid_blob + p.begin_at), *cell_of = work + grid::kWorkHead, *rank = cell_of + m, *sums = rank + m;
    float4 *points = reinterpret_cast<float4 *>(grid_blob + p.points_at);
    const int cells = (int) p.cells, by_m = blocks_of<grid::kThreads>(m);
    grid::k_grid_clear<<<blocks_of<grid::kThreads>(cells), grid::kThreads, 0, st>>>(box_keys, begin, cells);
    grid::k_grid_box<<<by_m < grid::kBoxGroups ? by_m : grid::kBoxGroups, grid::kThreads, 0, st>>>(y, m, box_keys);
    grid::k_grid_setup<<<1, grid::kThreads, 0, st>>>(g, box_keys, p.res, (int) p.planes_at);
    grid::k_grid_count<<<by_m, grid::kThreads, 0, st>>>(y, m, g, p.res, begin, cell_of, rank);
    grid::k_grid_scan_sums<<<p.scan_groups, grid::kThreads, 0, st>>>(begin, cells, sums);
    grid::k_grid_scan_top<<<1, 1024, 0, st>>>(sums, p.scan_groups);
    grid::k_grid_scan_chunk<<<p.scan_groups, grid::kThreads, 0, st>>>(begin, cells, sums);
    grid::k_grid_scatter<<<by_m, grid::kThreads, 0, st>>>(y, m, cell_of, rank, begin, points);
    return launch_status(who);
}

int psdr_hip_chamfer_grid_nearest(const float *x, int32_t n, const float *y, int32_t m, const uint32_t *grid_blob, int64_t grid_words, uint64_t *keys, int32_t *list,
                                  int32_t *index, float *dist2, uint64_t *stats, void *stream) {
    const std::string who = "psdr_hip_chamfer_grid_nearest: ";
    if (!in_range(n)) return psdr::api_fail(who + range_text("n", n));
    if (!in_range(m)) return psdr::api_fail(who + range_text("m", m));
    if (!x || !y || !grid_blob || !keys || !list || !index || !dist2 || !stats) return psdr::api_fail(who + "NULL argument");
    const grid::GridPlan p = grid::grid_plan_of(n, m);
    if (grid_words < p.grid_words) return psdr::api_fail(who + "grid_words = " + std::to_string(grid_words) + ", the plan of m = " + std::to_string(m) + " needs " + std::to_string(p.grid_words));
    hipStream_t st = (hipStream_t) stream;
    unsigned long long *k = reinterpret_cast<unsigned long long *>(keys), *s = reinterpret_cast<unsigned long long *>(stats);
    const hipError_t e = hipMemsetAsync(s, 0, 2 * sizeof(unsigned long long), st);
    if (e != hipSuccess) return psdr::api_fail(who + hipGetErrorString(e));
    const int *begin = reinterpret_cast<const int *>(grid_blob + p.begin_at);
    const float4 *points = reinterpret_cast<const float4 *>(grid_blob + p.points_at);
    if (p.lanes == 1) grid::k_grid_search<1><<<blocks_of<grid::kThreads>(n), grid::kThreads, 0, st>>>(x, n, m, grid_blob, p.res, p.max_shells, (int) p.planes_at, begin, points, k, list, s);
    else grid::k_grid_search<grid::kGroupLanes><<<blocks_of<grid::kThreads / grid::kGroupLanes>(n), grid::kThreads, 0, st>>>(x, n, m, grid_blob, p.res, p.max_shells, (int) p.planes_at, begin, points, k, list, s);
    grid::k_grid_fallback<<<dim3((unsigned) p.fb_groups, (unsigned) p.fb_slices), grid::kThreads, 0, st>>>(x, n, y, m, p.fb_slice_len, list, s, k);
    k_unpack<<<blocks_of<kThreads>(n), kThreads, 0, st>>>(k, n, m, index, dist2);
    return launch_status(who);
}

} // extern "C"
