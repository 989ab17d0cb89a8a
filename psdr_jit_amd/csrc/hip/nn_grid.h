// nn_grid.h — the exact nearest-neighbour search through a uniform grid over the candidates (chamfer.hip's psdr_hip_chamfer_grid_*; the Python
// statement of the plan: psdr_jit_amd/pointgrid.py: grid_plan; the numpy restatement of everything below: tests/pointgrid_ref.py).  include/psdr_hip.h states the contract:
// the results are the scan's, bit for bit.  Stated once here:
//   GridPlan, grid_plan_of      the resolution and the shell budget (functions of m alone), the lanes per query (of n), the layout of the grid blob and of the build's work array, the fallback's grid
//   cell_of_coord               the cell function of one axis, c(v) = clamp((int) floor((v - lo) * inv), 0, dim - 1): monotone non-decreasing in v
//   k_grid_*                    the build (box by integer atomics on order-preserving keys, constants and planes, histogram, exclusive scan, scatter), the shell walk
//                               with its stopping rule, and the fallback scan over the compacted list of the queries the walk could not certify
// EVERY LOOP of every kernel has an iteration bound that does not depend on the floats in the data: strides over integer counts, shells <= max_shells, cells of a shell,
// cell ranges clamped into [0, m], a plane search of at most kWalk steps.  That is why non-finite input can neither fault nor hang; every index that is read from the blob
// is clamped into range before it is used.
// Internal linkage throughout (see op_common.h).
#pragma once
#include <cstdint>

#include "nn_scan.h"

namespace {

namespace grid {

constexpr int kThreads = 256;           // lanes of every workgroup here: 4 waves
constexpr int kPerCell = 2;             // candidates per cell the resolution aims at: res = the largest r with kPerCell r^3 <= m
constexpr int kMaxRes = 256;            // cells per axis at most: 2^24 cells, a cell_begin array of 64 MiB
constexpr int kMinShells = 4;           // the shell budget is res / 4 within [kMinShells, kMaxShells]: a quarter of the box at most, and where the grid is coarse
constexpr int kMaxShells = 16;          // as many shells as the grid is fine; beyond the budget the fallback takes the query (a walk of 16 shells reads ~7 000 cell ranges, far below m there)
constexpr int kWalk = 8;                // steps that the search for a plane may take: the first 2^-22 max(|lo|, |hi|) long, each twice the one before
constexpr int kHeader = 16;             // 32-bit words ahead of the planes: lo[3], inv[3], width[3] (float), dim[3] (int), 4 unused
constexpr int kScanChunk = 2048;        // cells per workgroup of the exclusive scan: 8 per lane
constexpr int kBoxGroups = 256;         // workgroups of the box reduction at most
constexpr int kTile = 1024;             // candidates per LDS tile of the fallback scan (k_scan's)
constexpr int kFallbackGroups = 64;     // the fallback's fixed grid: query-block striders x candidate slices
constexpr int kFallbackSlices = 32;
constexpr int kGroupLanes = 8;          // lanes that share a query's walk for n <= kGroupMax queries, else 1
constexpr int kGroupMax = 65536;        // 8 x 65 536 lanes: the 256 CUs' 2 048 lanes each
constexpr int kWorkHead = 8;            // 32-bit words ahead of the per-candidate work arrays: the six box keys

// The grid blob, 32-bit words: [0, kHeader) the header; [planes_at, + 6 res) the planes, plane (axis a, side, k) at planes_at + (2 a + side) res + k; [begin_at, + cells)
// cell_begin, cell (c0 res + c1) res + c2; [points_at, + 4 m) the candidates in cell order as float4 (x, y, z, the bits of the original index).  begin_at and points_at are
// multiples of 4.  The build's work array: [0, kWorkHead) the box keys; [kWorkHead, + m) every candidate's cell; [.. + m) its rank inside the cell; then scan_groups sums.
struct GridPlan {
    int res, max_shells;
    long long cells;                    // res^3 + 1
    long long planes_at, begin_at, points_at, grid_words, work_words;
    int scan_groups, fb_groups, fb_slices, fb_slice_len;
    int lanes;                          // lanes per query of the walk: a function of n
};

inline GridPlan grid_plan_of(int n, int m) {
    GridPlan p;
    p.lanes = n <= kGroupMax ? kGroupLanes : 1;
    int r = 1;
    while (r < kMaxRes && (long long) kPerCell * (r + 1) * (r + 1) * (r + 1) <= (long long) m) ++r;
    p.res = r;
    p.max_shells = r / 4 < kMinShells ? kMinShells : (r / 4 > kMaxShells ? kMaxShells : r / 4);
    p.cells = (long long) r * r * r + 1;
    p.planes_at = kHeader;
    p.begin_at = (p.planes_at + 6LL * r + 3) / 4 * 4;
    p.points_at = (p.begin_at + p.cells + 3) / 4 * 4;
    p.grid_words = p.points_at + 4LL * m;
    p.scan_groups = (int) ((p.cells + kScanChunk - 1) / kScanChunk);
    p.work_words = kWorkHead + 2LL * m + p.scan_groups;
    const int tiles = (m + kTile - 1) / kTile;
    const int want = tiles < kFallbackSlices ? tiles : kFallbackSlices;
    p.fb_slice_len = (tiles + want - 1) / want * kTile;
    p.fb_slices = (m + p.fb_slice_len - 1) / p.fb_slice_len;
    p.fb_groups = kFallbackGroups;
    return p;
}

// an order-preserving map of the floats onto the unsigned integers (-0 counts as +0), and back
__device__ __forceinline__ unsigned int order_key(float v) {
    const unsigned int u = __float_as_uint(__fadd_rn(v, 0.f));
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_float(unsigned int k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// c(v): float subtraction, multiplication by inv > 0, floor, the clamp and the conversion are all monotone non-decreasing, so c is.  The clamp happens in float (a NaN
// goes to cell 0), so that the conversion never sees a value outside [0, dim - 1].
__device__ __forceinline__ int cell_of_coord(float v, float lo, float inv, int dim) {
    float t = floorf(__fmul_rn(__fsub_rn(v, lo), inv));
    t = t >= 0.f ? t : 0.f;
    t = fminf(t, (float) (dim - 1));
    return (int) t;
}

struct Header {
    float lo[3], inv[3];
    int dim[3];
};

__device__ __forceinline__ Header load_header(const unsigned int *__restrict__ g, int res) {
    Header h;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        h.lo[a] = __uint_as_float(g[a]);
        h.inv[a] = __uint_as_float(g[3 + a]);
        h.dim[a] = min(max((int) g[9 + a], 1), res);
    }
    return h;
}

// the exclusive prefix of v over the workgroup, in lane order; s: THREADS entries of LDS
template <int THREADS> __device__ int block_exclusive(int v, int *s) {
    s[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < THREADS; o <<= 1) {
        const int t = (int) threadIdx.x >= o ? s[threadIdx.x - o] : 0;
        __syncthreads();
        s[threadIdx.x] += t;
        __syncthreads();
    }
    const int r = s[threadIdx.x] - v;
    __syncthreads();
    return r;
}

// ---- the build

__global__ void __launch_bounds__(kThreads) k_grid_clear(unsigned int *__restrict__ box_keys, int *__restrict__ begin, int cells) {
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t < cells) begin[t] = 0;
    if (t < 3) box_keys[t] = 0xffffffffu;
    else if (t < 6) box_keys[t] = 0u;
}

// the box: an integer minimum and maximum are associative and commutative, the result does not depend on the order
__global__ void __launch_bounds__(kThreads) k_grid_box(const float *__restrict__ y, int m, unsigned int *__restrict__ box_keys) {
    unsigned int lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    for (int j = blockIdx.x * kThreads + threadIdx.x; j < m; j += gridDim.x * kThreads) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const unsigned int k = order_key(y[3LL * j + a]);
            lo[a] = min(lo[a], k);
            hi[a] = max(hi[a], k);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo[a] = min(lo[a], (unsigned int) __shfl_down((int) lo[a], o, 64));
            hi[a] = max(hi[a], (unsigned int) __shfl_down((int) hi[a], o, 64));
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            atomicMin(box_keys + a, lo[a]);
            atomicMax(box_keys + 3 + a, hi[a]);
        }
    }
}

// one workgroup: the constants of every axis, then the planes.  Plane (a, 0, k), 1 <= k < dim: a float b with c(b) < k, so that every candidate of a cell >= k along a
// has a coordinate > b; found from lo + k width by steps downwards (a step to the neighbouring float would not do: where |b| is far below |lo|, fl(b - lo) does not
// move with it), the first 2^-22 max(|lo|, |hi|) long and each twice the one before; -infinity (no certificate) when kWalk steps do not reach one.  Whatever the steps,
// a plane is only ever one for which c(b) < k has been EVALUATED.  Plane (a, 1, k), 0 <= k < dim - 1: the mirror image, a float b with c(b) > k, from
// lo + (k + 1) width upwards, else +infinity.
__global__ void __launch_bounds__(kThreads) k_grid_setup(unsigned int *__restrict__ g, const unsigned int *__restrict__ box_keys, int res, int planes_at) {
    __shared__ float s_lo[3], s_inv[3], s_width[3], s_step[3];
    __shared__ int s_dim[3];
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        const float lo = key_float(box_keys[a]), hi = key_float(box_keys[3 + a]);
        const float extent = __fsub_rn(hi, lo);
        const float inv = __fdiv_rn((float) res, extent);
        const bool many = inv > 0.f && inv < INFINITY;         // an axis of zero extent, or an inv that is not finite (or not positive): one cell
        s_lo[a] = lo;
        s_inv[a] = inv;
        s_width[a] = __fdiv_rn(extent, (float) res);
        s_dim[a] = many ? res : 1;
        s_step[a] = __fmul_rn(fmaxf(fabsf(lo), fabsf(hi)), 0x1p-22f);
        g[a] = __float_as_uint(lo);
        g[3 + a] = __float_as_uint(inv);
        g[6 + a] = __float_as_uint(s_width[a]);
        g[9 + a] = (unsigned int) s_dim[a];
    }
    if (threadIdx.x >= 12 && threadIdx.x < kHeader) g[threadIdx.x] = 0u;
    __syncthreads();
    for (int t = threadIdx.x; t < 6 * res; t += kThreads) {
        const int a = t / (2 * res), side = (t / res) & 1, k = t % res;
        const float lo = s_lo[a], inv = s_inv[a], width = s_width[a];
        const int dim = s_dim[a];
        float plane = side ? INFINITY : -INFINITY;
        if (side == 0 && k >= 1 && k < dim) {
            float b = __fadd_rn(lo, __fmul_rn((float) k, width)), d = s_step[a];
            for (int w = 0; w <= kWalk; ++w) {
                if (cell_of_coord(b, lo, inv, dim) < k) { plane = b; break; }
                b = __fsub_rn(b, d);
                d = __fadd_rn(d, d);
            }
        }
        if (side == 1 && k < dim - 1) {
            float b = __fadd_rn(lo, __fmul_rn((float) (k + 1), width)), d = s_step[a];
            for (int w = 0; w <= kWalk; ++w) {
                if (cell_of_coord(b, lo, inv, dim) > k) { plane = b; break; }
                b = __fadd_rn(b, d);
                d = __fadd_rn(d, d);
            }
        }
        g[planes_at + t] = __float_as_uint(plane);
    }
}

// every candidate's cell and its rank inside the cell (the value the integer atomicAdd returns: not deterministic, and nothing depends on it)
__global__ void __launch_bounds__(kThreads) k_grid_count(const float *__restrict__ y, int m, const unsigned int *__restrict__ g, int res, int *__restrict__ begin,
                                                         int *__restrict__ cell_of, int *__restrict__ rank) {
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= m) return;
    const Header h = load_header(g, res);
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = cell_of_coord(y[3LL * j + a], h.lo[a], h.inv[a], h.dim[a]);
    const int cell = (c[0] * res + c[1]) * res + c[2];
    cell_of[j] = cell;
    rank[j] = atomicAdd(begin + cell, 1);
}

// the exclusive scan of the counts, in place, in three launches: the sum of every chunk, the exclusive prefix of those sums (one workgroup), the prefix inside a chunk
__global__ void __launch_bounds__(kThreads) k_grid_scan_sums(const int *__restrict__ begin, int cells, int *__restrict__ sums) {
    __shared__ int s_red[kThreads / 64];
    const int at = blockIdx.x * kScanChunk + threadIdx.x * (kScanChunk / kThreads);
    int v = 0;
#pragma unroll
    for (int u = 0; u < kScanChunk / kThreads; ++u)
        if (at + u < cells) v += begin[at + u];
    const int t = block_sum<kThreads>(v, s_red);
    if (threadIdx.x == 0) sums[blockIdx.x] = t;
}

__global__ void __launch_bounds__(1024) k_grid_scan_top(int *__restrict__ sums, int groups) {
    __shared__ int s_scan[1024];
    const int per = (groups + 1023) / 1024;
    const int t0 = min(groups, (int) threadIdx.x * per), t1 = min(groups, t0 + per);
    int v = 0;
    for (int t = t0; t < t1; ++t) v += sums[t];
    int run = block_exclusive<1024>(v, s_scan);
    for (int t = t0; t < t1; ++t) {
        const int c = sums[t];
        sums[t] = run;
        run += c;
    }
}

__global__ void __launch_bounds__(kThreads) k_grid_scan_chunk(int *__restrict__ begin, int cells, const int *__restrict__ sums) {
    __shared__ int s_scan[kThreads];
    constexpr int kPer = kScanChunk / kThreads;
    const int at = blockIdx.x * kScanChunk + threadIdx.x * kPer;
    int c[kPer], v = 0;
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
        c[u] = at + u < cells ? begin[at + u] : 0;
        v += c[u];
    }
    int run = sums[blockIdx.x] + block_exclusive<kThreads>(v, s_scan);
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
        if (at + u < cells) begin[at + u] = run;
        run += c[u];
    }
}

__global__ void __launch_bounds__(kThreads) k_grid_scatter(const float *__restrict__ y, int m, const int *__restrict__ cell_of, const int *__restrict__ rank,
                                                           const int *__restrict__ begin, float4 *__restrict__ points) {
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= m) return;
    const int at = min(max(begin[cell_of[j]] + rank[j], 0), m - 1);
    points[at] = make_float4(y[3LL * j], y[3LL * j + 1], y[3LL * j + 2], __int_as_float(j));
}

// ---- the search

// kLanes lanes per query: kGroupLanes up to kGroupMax queries, where the device is not full and a lane per query walks a chain of dependent loads - cell_begin, then the
// candidates - shell after shell, so that the launch lasts as long as its longest chain; one lane per query beyond, where the lanes' idle turns would cost more than the
// chains (DESIGN.md section 7q has the figures).  The group visits the cells of the query's clamped cell's shells 0, 1, ... by Chebyshev distance; a column
// (c0 + d0, c1 + d1) on the shell's rim contributes one run of cells along the last axis - contiguous in cell order, so one range of the sorted candidates - an inner
// column its two end cells; the lanes take the (2 s + 1)^2 columns of a shell in turn and merge their bests by shuffles (the lexicographic minimum over (d2, j) does not
// depend on the order).  After shell s the cells that remain lie, along some axis a, at >= c_a + s + 1 or at <= c_a - s - 1; a side beyond the grid holds nothing.  For a
// side inside the grid, g = fl(plane - x_a) (upper) or fl(x_a - plane) (lower): if g >= 0, every candidate y of those cells has |fl(x_a - y_a)| >= g, hence d2 >= fl(g g)
// (rounding is monotone, and a sum of non-negative terms does not round below an addend).  The group stops when every such side has g >= 0 and fl(g g) > best -
// strictly: on equality a lower index may wait out there.  A NaN passes neither comparison.  A group that has not stopped after max_shells shells appends its query to
// the list (one integer atomicAdd) and leaves all ones in its key.  stats[0]: the list's length; stats[1]: the pairs tested.  Control flow is uniform inside a group, so
// the shuffles only ever read lanes that are active.
template <int kLanes> __global__ void __launch_bounds__(kThreads) k_grid_search(const float *__restrict__ x, int n, int m, const unsigned int *__restrict__ g, int res, int max_shells,
                                                          int planes_at, const int *__restrict__ begin, const float4 *__restrict__ points,
                                                          unsigned long long *__restrict__ keys, int *__restrict__ list, unsigned long long *__restrict__ stats) {
    const int i = blockIdx.x * (kThreads / kLanes) + threadIdx.x / kLanes, sub = threadIdx.x % kLanes;
    unsigned long long pairs = 0;
    if (i < n) {
        const Header h = load_header(g, res);
        const float q[3] = {x[3LL * i], x[3LL * i + 1], x[3LL * i + 2]};
        int c[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] = cell_of_coord(q[a], h.lo[a], h.inv[a], h.dim[a]);
        float best = INFINITY;
        int bj = 0;
        bool certified = false;
        for (int s = 0; s < max_shells && !certified; ++s) {
            const int side = 2 * s + 1;
            for (int col = sub; col < side * side; col += kLanes) {
                const int d0 = col / side - s, d1 = col % side - s;
                const int c0 = c[0] + d0, c1 = c[1] + d1;
                if (c0 < 0 || c0 >= h.dim[0] || c1 < 0 || c1 >= h.dim[1]) continue;
                const bool rim = max(abs(d0), abs(d1)) == s;
                const int row = (c0 * res + c1) * res;
                for (int part = 0; part < (rim ? 1 : 2); ++part) {
                    int z0, z1;                                                         // cells [z0, z1] of the column
                    if (rim) { z0 = max(c[2] - s, 0); z1 = min(c[2] + s, h.dim[2] - 1); }
                    else { z0 = z1 = part ? c[2] + s : c[2] - s; }
                    if (z0 < 0 || z1 >= h.dim[2] || z0 > z1) continue;
                    const int b0 = min(max(begin[row + z0], 0), m), b1 = min(max(begin[row + z1 + 1], b0), m);
                    pairs += (unsigned long long) (b1 - b0);
#pragma unroll 4
                    for (int t = b0; t < b1; ++t) {
                        const float4 p = points[t];
                        const int j = __float_as_int(p.w);
                        const float d2 = pair_d2(q[0], q[1], q[2], p.x, p.y, p.z);
                        if (d2 < best || (d2 == best && j < bj)) { best = d2; bj = j; }
                    }
                }
            }
#pragma unroll
            for (int o = 1; o < kLanes; o <<= 1) {
                const float d2 = __shfl_xor(best, o, 64);
                const int j = __shfl_xor(bj, o, 64);
                if (d2 < best || (d2 == best && j < bj)) { best = d2; bj = j; }
            }
            bool ok = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int up = c[a] + s + 1, down = c[a] - s - 1;
                if (up < h.dim[a]) {
                    const float gap = __fsub_rn(__uint_as_float(g[planes_at + (2 * a) * res + up]), q[a]);
                    ok = ok && gap >= 0.f && __fmul_rn(gap, gap) > best;
                }
                if (down >= 0) {
                    const float gap = __fsub_rn(q[a], __uint_as_float(g[planes_at + (2 * a + 1) * res + down]));
                    ok = ok && gap >= 0.f && __fmul_rn(gap, gap) > best;
                }
            }
            certified = ok;
        }
        if (sub == 0) {
            if (certified) keys[i] = pack_key(best, bj);
            else {
                keys[i] = ~0ull;
                const unsigned long long slot = atomicAdd(stats, 1ull);
                if (slot < (unsigned long long) n) list[slot] = i;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pairs += __shfl_down(pairs, o, 64);
    if ((threadIdx.x & 63) == 0 && pairs) atomicAdd(stats + 1, pairs);
}

// The queries of the list against ALL m candidates in their original order: k_scan's inner loop (a tile of candidates in LDS as x / y / z planes, every lane reads the
// same float4, ascending j, a strict `<`), one query per lane.  The grid is fixed: workgroup (bx, by) takes the query blocks bx, bx + gridDim.x, ... of the list, whose
// length it reads on the device, against slice by of the candidates, and the slices merge by the integer minimum of the keys (the search left all ones).
__global__ void __launch_bounds__(kThreads) k_grid_fallback(const float *__restrict__ x, int n, const float *__restrict__ y, int m, int slice_len,
                                                            const int *__restrict__ list, unsigned long long *__restrict__ stats, unsigned long long *__restrict__ keys) {
    __shared__ float4 s_c[3][kTile / 4];
    float *s_x = reinterpret_cast<float *>(s_c[0]), *s_y = reinterpret_cast<float *>(s_c[1]), *s_z = reinterpret_cast<float *>(s_c[2]);
    const unsigned long long listed = stats[0];
    const int count = listed < (unsigned long long) n ? (int) listed : n;
    const int j0 = blockIdx.y * slice_len;
    const int j1 = min(m, j0 + slice_len);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && count) atomicAdd(stats + 1, (unsigned long long) count * (unsigned long long) m);
    for (int first = blockIdx.x * kThreads; first < count; first += gridDim.x * kThreads) {
        const bool live = first + (int) threadIdx.x < count;
        const int i = live ? min(max(list[first + threadIdx.x], 0), n - 1) : 0;
        const float qx = live ? x[3LL * i] : 0.f, qy = live ? x[3LL * i + 1] : 0.f, qz = live ? x[3LL * i + 2] : 0.f;
        float best = INFINITY;
        int bj = j0;
        for (int base = j0; base < j1; base += kTile) {
            __syncthreads();                                       // (the previous tile has been read)
            for (int t = threadIdx.x; t < kTile; t += kThreads) {
                const int j = base + t;
                const bool have = j < j1;
                s_x[t] = have ? y[3LL * j] : INFINITY;
                s_y[t] = have ? y[3LL * j + 1] : INFINITY;
                s_z[t] = have ? y[3LL * j + 2] : INFINITY;
            }
            __syncthreads();
            const int groups = (min(kTile, j1 - base) + 3) >> 2;
            for (int gr = 0; gr < groups; ++gr) {
                const float4 cx = s_c[0][gr], cy = s_c[1][gr], cz = s_c[2][gr];
                const float ax[4] = {cx.x, cx.y, cx.z, cx.w}, ay[4] = {cy.x, cy.y, cy.z, cy.w}, az[4] = {cz.x, cz.y, cz.z, cz.w};
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float d2 = pair_d2(qx, qy, qz, ax[u], ay[u], az[u]);
                    if (d2 < best) { best = d2; bj = base + 4 * gr + u; }
                }
            }
        }
        if (live) atomicMin(keys + i, pack_key(best, bj));
    }
}

} // namespace grid

} // namespace
