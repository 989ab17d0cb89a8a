// nn_scan.h — what the units that scan query blocks x candidate slices (chamfer.hip, pointmesh.hip, sdf.hip) share, stated once:
//   Plan, plan_of<TILE, WIDE>   the split of n queries against m candidates (psdr_jit_amd/_opcommon.py: slice_plan states it in Python; the *_cpu tests sweep one against the other)
//   pm::kTile, pm::kWideQueries the point-to-mesh constants, which pointmesh.hip and sdf.hip both instantiate plan_of with
//   pack_key, key_index, key_dist2, merge_key, clear_keys: a query's best as (float bits of dist2) << 32 | index, and the merge of the slices by one integer minimum
//   coefficient, run_sum, finish_two: the factor of a pair's gradient term, and the last launch of a two-term loss
// Internal linkage throughout (see op_common.h).  A new operator includes this file; it does not copy from it.
#pragma once
#include "op_common.h"

namespace {

namespace scan {
constexpr int kThreads = 256;           // lanes of a scan workgroup: 4 waves
constexpr int kNarrowMax = 1024;        // n <= kNarrowMax: one query per lane (the wide scan would leave its other registers idle)
constexpr int kTargetGroups = 2048;     // workgroups the grid aims at: 8 per CU, the most that 256 CUs hold of 256-thread workgroups
}

namespace pm {
constexpr int kTile = 256;              // candidates per LDS tile of the point-to-mesh scans
constexpr int kWideQueries = 2;         // queries per lane of their wide scan
}

struct Plan { int tile, qpl, slices, slice_len; };

// the split, a pure function of (queries, candidates)
template <int TILE, int WIDE> inline Plan plan_of(int n, int m) {
    Plan p;
    p.tile = TILE;
    p.qpl = n > scan::kNarrowMax ? WIDE : 1;
    const int per_group = scan::kThreads * p.qpl;
    const int qblocks = (n + per_group - 1) / per_group;
    const int tiles = (m + TILE - 1) / TILE;
    int want = (scan::kTargetGroups + qblocks - 1) / qblocks;
    if (want > tiles) want = tiles;
    const int tiles_per_slice = (tiles + want - 1) / want;
    p.slice_len = tiles_per_slice * TILE;
    p.slices = (m + p.slice_len - 1) / p.slice_len;           // no empty slice: slice s is [s slice_len, min(m, (s + 1) slice_len))
    return p;
}

// the grid of a scan: query blocks x candidate slices
inline dim3 scan_grid(int n, const Plan &p) {
    const int per_group = scan::kThreads * p.qpl;
    return dim3((unsigned) ((n + per_group - 1) / per_group), (unsigned) p.slices);
}

// dist2 >= +0, so keys order as unsigned integers: by dist2, then by index
__device__ __forceinline__ unsigned long long pack_key(float dist2, int j) { return ((unsigned long long) __float_as_uint(dist2) << 32) | (unsigned int) j; }
__device__ __forceinline__ int key_index(unsigned long long key, int m) { return (int) min((unsigned int) (key & 0xffffffffu), (unsigned int) (m - 1)); }
__device__ __forceinline__ float key_dist2(unsigned long long key) { return __uint_as_float((unsigned int) (key >> 32)); }

// d2 of a (query, candidate) pair of points in the difference form: every operation one float32 rounding, nothing fused, in this order (the chamfer section of
// include/psdr_hip.h); the one statement of it, which the scan and the grid search (nn_grid.h) both use
__device__ __forceinline__ float pair_d2(float qx, float qy, float qz, float ax, float ay, float az) {
    const float dx = __fsub_rn(qx, ax), dy = __fsub_rn(qy, ay), dz = __fsub_rn(qz, az);
    return __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
}

// a slice's best for query i: stored where there is one slice, else merged by an integer minimum (associative and commutative: the result does not depend on the order)
__device__ __forceinline__ void merge_key(unsigned long long *__restrict__ keys, int i, unsigned long long key, int slices) {
    if (slices == 1) keys[i] = key;
    else atomicMin(keys + i, key);
}

// before a scan of several slices: all ones, above every key (the float half of a key is at most +infinity's bits)
inline hipError_t clear_keys(unsigned long long *keys, int n, const Plan &p, hipStream_t st) {
    return p.slices > 1 ? hipMemsetAsync(keys, 0xff, (size_t) n * sizeof(unsigned long long), st) : hipSuccess;
}

// k(s): squared: 2 w / count; else (w / count) / sqrt(s), 0 at s = 0
__device__ __forceinline__ float coefficient(float k, float s, int squared) { return squared ? k : (s > 0.f ? k / sqrtf(s) : 0.f); }

// a lane adds every THREADS-th partial sum of a direction in ascending order, then the workgroup's fixed order
template <int THREADS> __device__ double run_sum(const double *p, int count, double *s_red) {
    double a = 0.0;
    for (int t = threadIdx.x; t < count; t += THREADS) a += p[t];
    return block_sum<THREADS>(a, s_red);
}

// the body of k_finish, one workgroup of THREADS lanes: out = (loss, term a, term b) from the partial sums of the two directions (blocks_a of them, then blocks_b; a
// direction that is off has none), term = sum / count, loss = w_a term a + w_b term b over the directions that are on
template <int THREADS> __device__ __forceinline__ void finish_two(const double *__restrict__ partial, int blocks_a, int blocks_b, int n_a, int n_b, float w_a, float w_b,
                                                                  float *__restrict__ out, double *s_red) {
    const double sa = run_sum<THREADS>(partial, blocks_a, s_red);
    const double sb = run_sum<THREADS>(partial + blocks_a, blocks_b, s_red);
    if (threadIdx.x == 0) {
        const float ta = blocks_a ? (float) (sa / (double) n_a) : 0.f, tb = blocks_b ? (float) (sb / (double) n_b) : 0.f;
        float loss = 0.f;
        if (blocks_a) loss = w_a * ta;
        if (blocks_b) { const float t = w_b * tb; loss = blocks_a ? loss + t : t; }
        out[0] = loss;
        out[1] = ta;
        out[2] = tb;
    }
}

} // namespace
