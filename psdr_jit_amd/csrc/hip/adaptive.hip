// adaptive.hip — adaptive sampling's two data-parallel pieces (Python surface: psdr_jit_amd/adaptive.py):
//   psdr_hip_adaptive_counts   a per-pixel weight map -> per-pixel sample counts that spend an exact budget, and their offsets
//   psdr_hip_adaptive_expand   offsets -> the pixel list, sorted by pixel, that the batch entry points render
//   psdr_hip_adaptive_merge    the rows of such a list folded back into a frame (segment sum, optional pilot frame mixed in)
//   psdr_hip_adaptive_merge_adj  the transpose of the fold
// Integer and segment work only: no float atomics anywhere, every sum has one order, so the same input gives the same bits.
//
// The allocation (the definition a CPU restatement reproduces bit for bit, tests/test_adaptive_cpu.py::allocate):
//   w_i = the weight if finite and > 0, else 0;  wmax = max w_i;  q_i = (uint32) floor((double) w_i / (double) wmax * 2^bits)   (wmax = 0: q_i = 1)
//   C = exclusive prefix sum of q in uint64 over n + 1 positions, S = C_n;  B' = budget - n min_count
//   counts_i = min_count + floor(B' C_{i+1} / S) - floor(B' C_i / S)          offsets_i = i min_count + floor(B' C_i / S)
// (the offsets telescope: no second scan).  bits is chosen by the host so that B' S < 2^62.
//
// The scan has two levels.  A workgroup owns a tile of kTile = 2048 consecutive pixels, 8 per thread:
//   k_tile_max    the maximum of every tile -> scratch                                  (max is exact: its order does not matter)
//   k_tile_sums   every workgroup reduces the tile maxima to wmax, quantises its tile and stores the tile's sum of q -> scratch
//   k_allocate    level 2: every workgroup adds the tile sums in front of its own (and all of them, S) - integer sums, exact in any order;
//                 level 1: the prefix inside the tile - per thread serial, wave64 shuffle scan over the threads' sums, the four wave totals through LDS
// so no workgroup waits for another inside a launch (no look-back, no spin), at the price of reading at most kMaxTiles words per workgroup from L2.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../../include/psdr_hip.h"
#include "op_common.h"
#define ACHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return psdr::api_fail(std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

namespace {

typedef unsigned long long u64;

constexpr int kThreads = 256;                    // 4 waves
constexpr int kItems = 8;                        // consecutive pixels per thread
constexpr int kTile = kThreads * kItems;         // 2048 pixels per workgroup
constexpr int kMaxN = 1 << 24;
constexpr int kMaxTiles = kMaxN / kTile;         // 8192
constexpr int kMaxChannels = 4;

// scratch: [wmax, pad] | tile maxima float[kMaxTiles] | tile sums u64[kMaxTiles]
constexpr size_t kOffMax = 16, kOffSums = kOffMax + sizeof(float) * kMaxTiles, kScratchBytes = kOffSums + sizeof(u64) * kMaxTiles;

__device__ inline float clean(float w) { return (w > 0.f && w <= __FLT_MAX__) ? w : 0.f; }        // NaN, Inf, <= 0 -> 0
__device__ inline unsigned quantise(float w, float wmax, double scale) {
    return wmax > 0.f ? (unsigned) floor((double) w / (double) wmax * scale) : 1u;
}

// the same value in every thread; `lds` holds one word per wave and may be reused after the call returns in every thread
__device__ inline float block_max(float v, float *lds) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    float m = lds[0];
    for (int w = 1; w < kThreads / 64; ++w) m = fmaxf(m, lds[w]);
    return m;
}
__device__ inline u64 block_sum(u64 v, u64 *lds) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 s = 0;
    for (int w = 0; w < kThreads / 64; ++w) s += lds[w];
    return s;
}
// exclusive prefix of `v` over the threads of the workgroup, in thread order
__device__ inline u64 block_exclusive_scan(u64 v, u64 *lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const u64 up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    __syncthreads();
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    u64 before = 0;
    for (int w = 0; w < wave; ++w) before += lds[w];
    return before + inc - v;
}

__global__ void __launch_bounds__(kThreads) k_tile_max(const float *weights, int n, float *tile_max) {
    __shared__ float lds[kThreads / 64];
    const long long base = (long long) blockIdx.x * kTile + threadIdx.x * kItems;
    float m = 0.f;
    for (int k = 0; k < kItems; ++k)
        if (base + k < n) m = fmaxf(m, clean(weights[base + k]));
    m = block_max(m, lds);
    if (threadIdx.x == 0) tile_max[blockIdx.x] = m;
}

__device__ inline float reduce_tile_max(const float *tile_max, int n_tiles, float *lds) {
    float m = 0.f;
    for (int k = threadIdx.x; k < n_tiles; k += kThreads) m = fmaxf(m, tile_max[k]);
    return block_max(m, lds);
}

__global__ void __launch_bounds__(kThreads) k_tile_sums(const float *weights, int n, int n_tiles, double scale, const float *tile_max, float *wmax_out, u64 *tile_sum) {
    __shared__ float ldsf[kThreads / 64];
    __shared__ u64 lds[kThreads / 64];
    const float wmax = reduce_tile_max(tile_max, n_tiles, ldsf);
    if (blockIdx.x == 0 && threadIdx.x == 0) *wmax_out = wmax;
    const long long base = (long long) blockIdx.x * kTile + threadIdx.x * kItems;
    u64 s = 0;
    for (int k = 0; k < kItems; ++k)
        if (base + k < n) s += quantise(clean(weights[base + k]), wmax, scale);
    s = block_sum(s, lds);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = s;
}

__global__ void __launch_bounds__(kThreads) k_allocate(const float *weights, int n, int n_tiles, double scale, const float *wmax_in, const u64 *tile_sum,
                                                       u64 spare /* B' */, int min_count, int *counts, int *offsets) {
    __shared__ u64 lds[kThreads / 64];
    const float wmax = *wmax_in;
    // level 2: the tiles in front of this one, and all of them
    u64 front = 0, all = 0;
    for (int k = threadIdx.x; k < n_tiles; k += kThreads) {
        const u64 t = tile_sum[k];
        all += t;
        if (k < (int) blockIdx.x) front += t;
    }
    front = block_sum(front, lds);
    all = block_sum(all, lds);
    const bool uniform = !(wmax > 0.f) || all == 0;          // (all == 0 with wmax > 0 cannot happen: the maximum itself quantises to 2^bits)
    const u64 S = uniform ? (u64) n : all;
    const long long base = (long long) blockIdx.x * kTile + threadIdx.x * kItems;
    unsigned q[kItems];
    u64 mine = 0;
    for (int k = 0; k < kItems; ++k) {
        q[k] = base + k < n ? (uniform ? 1u : quantise(clean(weights[base + k]), wmax, scale)) : 0u;
        mine += q[k];
    }
    // level 1: the threads in front of this one inside the tile
    u64 c = (uniform ? (u64) blockIdx.x * kTile : front) + block_exclusive_scan(mine, lds);
    u64 f = spare * c / S;                                   // floor(B' C_i / S); B' C <= B' S < 2^62
    for (int k = 0; k < kItems; ++k) {
        const long long i = base + k;
        if (i >= n) break;
        c += q[k];
        const u64 f_next = spare * c / S;
        counts[i] = min_count + (int) (f_next - f);
        offsets[i] = (int) ((u64) i * (u64) min_count + f);
        if (i == n - 1) offsets[n] = (int) ((u64) n * (u64) min_count + f_next);          // = budget: C_n = S
        f = f_next;
    }
}

// the pixel of entry k: the largest p in [0, n) with offsets[p] <= k (pixels without entries repeat an offset and are stepped over)
__device__ inline int pixel_of(const int *offsets, int n, int k) {
    int lo = 0, hi = n;                       // invariant: offsets[lo] <= k (offsets[0] = 0); the answer is in [lo, hi)
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] <= k) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(kThreads) k_expand(const int *offsets, int n, int total, int *pix_ids) {
    const long long k = (long long) blockIdx.x * kThreads + threadIdx.x;
    if (k < total) pix_ids[k] = pixel_of(offsets, n, (int) k);
}

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// one wave per pixel: lane l adds entries l, l + 64, ... of the segment in that order, then the 64 partial sums go down a fixed shuffle tree
template <int CH> __global__ void __launch_bounds__(kThreads) k_merge(const int *offsets, int n, int total, const float *rows, double rows_n, const float *base, double base_n,
                                                                     int square, float *out) {
    const long long p = ((long long) blockIdx.x * kThreads + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (p >= n) return;
    const int b = clampi(offsets[p], 0, total), e = clampi(offsets[p + 1], b, total);          // (a list that does not belong to these offsets reads no row outside it)
    float acc[CH];
    for (int c = 0; c < CH; ++c) acc[c] = 0.f;
    for (long long k = b + lane; k < e; k += 64)
        for (int c = 0; c < CH; ++c) acc[c] += rows[k * CH + c];
    for (int o = 32; o > 0; o >>= 1)
        for (int c = 0; c < CH; ++c) acc[c] += __shfl_down(acc[c], o, 64);
    if (lane != 0) return;
    const double n_tot = base_n + rows_n * (double) (e - b);
    for (int c = 0; c < CH; ++c) {
        const double bp = base ? (double) base[p * CH + c] : 0.;
        double v = 0.;
        if (n_tot > 0.) {
            if (square) { const double wb = base_n / n_tot, wr = rows_n / n_tot; v = wb * wb * bp + wr * wr * (double) acc[c]; }
            else v = (base_n * bp + rows_n * (double) acc[c]) / n_tot;
        }
        out[p * CH + c] = (float) v;
    }
}

template <int CH> __global__ void __launch_bounds__(kThreads) k_merge_adj_rows(const int *offsets, int n, int total, const float *d_out, double rows_n, double base_n, float *d_rows) {
    const long long k = (long long) blockIdx.x * kThreads + threadIdx.x;
    if (k >= total) return;
    const int p = pixel_of(offsets, n, (int) k);
    const int cnt = clampi(offsets[p + 1], 0, total) - clampi(offsets[p], 0, total);
    const double n_tot = base_n + rows_n * (double) cnt;
    const double s = n_tot > 0. ? rows_n / n_tot : 0.;
    for (int c = 0; c < CH; ++c) d_rows[k * CH + c] = (float) ((double) d_out[(long long) p * CH + c] * s);
}

__global__ void __launch_bounds__(kThreads) k_merge_adj_base(const int *offsets, int n, int total, int channels, const float *d_out, double rows_n, double base_n, float *d_base) {
    const long long i = (long long) blockIdx.x * kThreads + threadIdx.x;
    if (i >= (long long) n * channels) return;
    const int p = (int) (i / channels);
    const int cnt = clampi(offsets[p + 1], 0, total) - clampi(offsets[p], 0, total);
    const double n_tot = base_n + rows_n * (double) cnt;
    d_base[i] = (float) (n_tot > 0. ? (double) d_out[i] * (base_n / n_tot) : 0.);
}

int ceil_log2(long long v) { int b = 0; while ((1ll << b) < v) ++b; return b; }          // v >= 1

int blocks_for(long long items) { return (int) ((items + kThreads - 1) / kThreads); }

const char *check_fold(const void *offsets, int32_t n, int64_t total, int32_t channels, float rows_n, float base_n) {
    if (!offsets) return "offsets is NULL";
    if (n <= 0) return "n must be positive";
    if (total < 0 || total > INT32_MAX) return "total must lie in [0, 2^31 - 1]";
    if (channels < 1 || channels > kMaxChannels) return "channels must lie in [1, 4]";
    if (!(rows_n > 0.f) || !std::isfinite(rows_n)) return "rows_n must be finite and positive";
    if (!(base_n >= 0.f) || !std::isfinite(base_n)) return "base_n must be finite and not negative";
    return nullptr;
}

} // namespace

extern "C" {

int64_t psdr_hip_adaptive_scratch_bytes(void) { return (int64_t) kScratchBytes; }

int psdr_hip_adaptive_bits(int32_t n, int64_t budget) {
    if (n <= 0 || budget < 0) return -1;
    const int b = 62 - ceil_log2(n) - ceil_log2(budget > 1 ? budget : 1);
    return b < 20 ? b : 20;
}

int psdr_hip_adaptive_counts(const float *weights, int32_t n, int64_t budget, int32_t min_count, int32_t *counts, int32_t *offsets, void *scratch, void *stream) {
    const std::string me = "psdr_hip_adaptive_counts: ";
    if (!weights || !counts || !offsets || !scratch) return psdr::api_fail(me + "NULL argument");
    if (n <= 0 || n > kMaxN) return psdr::api_fail(me + "n = " + std::to_string(n) + ", must lie in [1, 2^24]");
    if (budget < 0) return psdr::api_fail(me + "budget = " + std::to_string(budget) + " is negative");
    if (budget > INT32_MAX) return psdr::api_fail(me + "budget = " + std::to_string(budget) + " is above 2^31 - 1 (a pixel list has an int32 length)");
    if (min_count < 0) return psdr::api_fail(me + "min_count = " + std::to_string(min_count) + " is negative");
    if ((int64_t) n * min_count > budget) return psdr::api_fail(me + "budget = " + std::to_string(budget) + " is below n * min_count = " + std::to_string((int64_t) n * min_count));
    const int bits = psdr_hip_adaptive_bits(n, budget);
    if (bits < 8) return psdr::api_fail(me + "n = " + std::to_string(n) + " with budget = " + std::to_string(budget) + " leaves " + std::to_string(bits) + " bits for a weight, fewer than 8");
    // the arguments are sound: from here on the device is touched
    hipStream_t s = (hipStream_t) stream;
    const int n_tiles = (n + kTile - 1) / kTile;
    float *wmax = (float *) scratch, *tile_max = (float *) ((char *) scratch + kOffMax);
    u64 *tile_sum = (u64 *) ((char *) scratch + kOffSums);
    const double scale = (double) (1u << bits);
    k_tile_max<<<n_tiles, kThreads, 0, s>>>(weights, n, tile_max);
    k_tile_sums<<<n_tiles, kThreads, 0, s>>>(weights, n, n_tiles, scale, tile_max, wmax, tile_sum);
    k_allocate<<<n_tiles, kThreads, 0, s>>>(weights, n, n_tiles, scale, wmax, tile_sum, (u64) (budget - (int64_t) n * min_count), min_count, counts, offsets);
    ACHK(hipGetLastError());
    return 0;
}

int psdr_hip_adaptive_expand(const int32_t *offsets, int32_t n, int64_t total, int32_t *pix_ids, void *stream) {
    const std::string me = "psdr_hip_adaptive_expand: ";
    if (!offsets) return psdr::api_fail(me + "offsets is NULL");
    if (n <= 0) return psdr::api_fail(me + "n = " + std::to_string(n) + ", must be positive");
    if (total < 0 || total > INT32_MAX) return psdr::api_fail(me + "total = " + std::to_string(total) + ", must lie in [0, 2^31 - 1]");
    if (total == 0) return 0;                  // an empty list: nothing to write
    if (!pix_ids) return psdr::api_fail(me + "pix_ids is NULL");
    k_expand<<<blocks_for(total), kThreads, 0, (hipStream_t) stream>>>(offsets, n, (int) total, pix_ids);
    ACHK(hipGetLastError());
    return 0;
}

int psdr_hip_adaptive_merge(const int32_t *offsets, int32_t n, int64_t total, int32_t channels, const float *rows, float rows_n, const float *base, float base_n,
                            int32_t square, float *out, void *stream) {
    const std::string me = "psdr_hip_adaptive_merge: ";
    if (const char *why = check_fold(offsets, n, total, channels, rows_n, base_n)) return psdr::api_fail(me + why);
    if (!out) return psdr::api_fail(me + "out is NULL");
    if (total > 0 && !rows) return psdr::api_fail(me + "rows is NULL");
    if (!base && base_n != 0.f) return psdr::api_fail(me + "base is NULL and base_n is not 0");
    if (square != 0 && square != 1) return psdr::api_fail(me + "square must be 0 or 1");
    hipStream_t s = (hipStream_t) stream;
    const int blocks = blocks_for((long long) n * 64), t = (int) total;
    switch (channels) {
        case 1: k_merge<1><<<blocks, kThreads, 0, s>>>(offsets, n, t, rows, rows_n, base, base_n, square, out); break;
        case 2: k_merge<2><<<blocks, kThreads, 0, s>>>(offsets, n, t, rows, rows_n, base, base_n, square, out); break;
        case 3: k_merge<3><<<blocks, kThreads, 0, s>>>(offsets, n, t, rows, rows_n, base, base_n, square, out); break;
        default: k_merge<4><<<blocks, kThreads, 0, s>>>(offsets, n, t, rows, rows_n, base, base_n, square, out); break;
    }
    ACHK(hipGetLastError());
    return 0;
}

int psdr_hip_adaptive_merge_adj(const int32_t *offsets, int32_t n, int64_t total, int32_t channels, const float *d_out, float rows_n, float base_n, float *d_rows,
                                float *d_base, void *stream) {
    const std::string me = "psdr_hip_adaptive_merge_adj: ";
    if (const char *why = check_fold(offsets, n, total, channels, rows_n, base_n)) return psdr::api_fail(me + why);
    if (!d_out) return psdr::api_fail(me + "d_out is NULL");
    if (total > 0 && !d_rows) return psdr::api_fail(me + "d_rows is NULL");
    hipStream_t s = (hipStream_t) stream;
    const int t = (int) total;
    if (t > 0) {
        switch (channels) {
            case 1: k_merge_adj_rows<1><<<blocks_for(t), kThreads, 0, s>>>(offsets, n, t, d_out, rows_n, base_n, d_rows); break;
            case 2: k_merge_adj_rows<2><<<blocks_for(t), kThreads, 0, s>>>(offsets, n, t, d_out, rows_n, base_n, d_rows); break;
            case 3: k_merge_adj_rows<3><<<blocks_for(t), kThreads, 0, s>>>(offsets, n, t, d_out, rows_n, base_n, d_rows); break;
            default: k_merge_adj_rows<4><<<blocks_for(t), kThreads, 0, s>>>(offsets, n, t, d_out, rows_n, base_n, d_rows); break;
        }
    }
    if (d_base) k_merge_adj_base<<<blocks_for((long long) n * channels), kThreads, 0, s>>>(offsets, n, t, channels, d_out, rows_n, base_n, d_base);
    ACHK(hipGetLastError());
    return 0;
}

} // extern "C"
