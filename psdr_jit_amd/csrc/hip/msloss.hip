// msloss.hip — the multi-scale (image pyramid) loss and its gradient in one fused pass (Python surface: psdr_jit_amd/msloss.py).
//
// The definition (include/psdr_hip.h states it in full).  Frame W x H, pixel (x, y) at row y W + x; img, target [W H, C], C in 1..4; weight absent, [W H] or [W H, C].
//   d_0 = weight (img - target);   level l + 1 is ceil(W_l / 2) x ceil(H_l / 2), its pixel (i, j) the mean of those of d_l(2i .. 2i + 1, 2j .. 2j + 1) that exist
//   level_loss_l = sum rho(d_l) / (C W_l H_l),  rho = |x| (rho'(0) = 0) or x^2;   loss = sum_l lambda_l level_loss_l
//   dloss / dimg = weight G_0,   G_l = (lambda_l / (C W_l H_l)) rho'(d_l) + G_{l+1}(parent) / (number of the parent's children),   G_L = 0
//
// Three launches.  Tiles are 32 x 32 level-0 pixels aligned to 32, so a tile's 2 x 2 blocks are the frame's own and a tile owns one pixel of level 5.
//   k_up    one workgroup per tile: d_0 into LDS as C planes, levels 1 .. 5 reduced there, every level written to the handle's pyramid, and per level the tile's
//           sum of rho in a fixed order (a lane's own elements, the wave by shuffles, the four waves in order).
//   k_top   one workgroup: adds the tiles' partial sums in a fixed order, takes the ceil(W / 32) x ceil(H / 32) level-5 image through the remaining levels (in the
//           pyramid: global memory, one barrier per level), writes loss and level losses, and sweeps G back down to level 5: one value per tile and channel.
//   k_down  one workgroup per tile: G of levels 5 .. 1 in LDS from the pyramid's d_l, then weight G_0 written as the gradient.  It reads d_l back (4/3 of a frame)
//           rather than both images again (2 frames): the pyramid is written anyway, psdr_hip_msloss_level serves it.
// Missing children are staged as 0 and the divisor is the number that exist (1, 2 or 4: a power of two), so partial tiles and odd edges need no second code path.
// No atomics, no host synchronisation, no copy to the host: the same input gives the same bits.  No contraction in this unit (the build's -ffp-contract=off).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../../include/psdr_hip.h"
#include "op_common.h"

namespace {

constexpr int kThreads = 256;           // k_up, k_down: 4 waves, 4 pixels of the tile per lane
constexpr int kTopThreads = 1024;       // k_top: one workgroup, 16 waves
constexpr int kTile = 32, kTileLog = 5;
constexpr int kTileLevels = kTileLog + 1;                  // levels 0 .. 5 live inside a tile
constexpr int kCoarse = 341;                               // 256 + 64 + 16 + 4 + 1: a plane of levels 1 .. 5
constexpr int kPlane = kTile * kTile + kCoarse + 1;        // 1366 = 21 * 64 + 22: the C planes of one pixel fall on different LDS banks
constexpr int kMaxLevels = 16;
constexpr int kMaxSide = 16384;
constexpr long long kMaxPixels = 1LL << 24;

__host__ __device__ constexpr int coarse_off(int l) { return l == 1 ? 0 : l == 2 ? 256 : l == 3 ? 320 : l == 4 ? 336 : 340; }      // level l = 1 .. 5 inside a plane's coarse part

struct Pyr {
    int L, Lt;                          // levels; levels inside a tile = min(L, 6)
    int tiles_x, tiles_y;
    int w[kMaxLevels], h[kMaxLevels];
    long long off[kMaxLevels];          // level l of the residual pyramid: float offset into `pyr` ([W_l H_l, C] each)
    long long goff[kMaxLevels];         // level l >= 5 of the stored coarse gradient: float offset into `gpyr`
    float inv_n[kMaxLevels];            // 1 / (C W_l H_l)
    float lambda[kMaxLevels];
    float coef[kMaxLevels];             // lambda_l / (C W_l H_l), rounded once from double
    float *pyr, *gpyr, *partial;        // partial: [tiles][6]
};

template <int NORM> __device__ __forceinline__ float rho(float d) { return NORM == PSDR_MSLOSS_L1 ? fabsf(d) : d * d; }
template <int NORM> __device__ __forceinline__ float drho(float d) { return NORM == PSDR_MSLOSS_L1 ? (float) (d > 0.f) - (float) (d < 0.f) : 2.f * d; }

// WC: 0 no weight, 1 one channel, 2 C channels
template <int C, int NORM, int WC> __global__ void __launch_bounds__(kThreads)
k_up(Pyr P, const float *__restrict__ img, const float *__restrict__ target, const float *__restrict__ weight) {
    __shared__ float s[C * kPlane];
    __shared__ float s_red[kThreads / 64];
    const int tx = blockIdx.x, ty = blockIdx.y;
    const int W = P.w[0], H = P.h[0];
    float acc[kTileLevels];
#pragma unroll
    for (int l = 0; l < kTileLevels; ++l) acc[l] = 0.f;
    // level 0: the tile's rows as flat runs of 32 C floats, so that consecutive lanes read consecutive words
    float *pyr0 = P.pyr + P.off[0];
    for (int e = threadIdx.x; e < kTile * kTile * C; e += kThreads) {
        const int y = e / (kTile * C), k = e - y * (kTile * C), x = k / C, c = k - x * C;
        const int gx = tx * kTile + x, gy = ty * kTile + y;
        float d = 0.f;
        if (gx < W && gy < H) {
            const long long p = (long long) gy * W + gx;
            d = img[p * C + c] - target[p * C + c];
            if (WC == 1) d = weight[p] * d;
            if (WC == 2) d = weight[p * C + c] * d;
            pyr0[p * C + c] = d;
            acc[0] += rho<NORM>(d);
        }
        s[c * kPlane + y * kTile + x] = d;
    }
    __syncthreads();
#pragma unroll
    for (int l = 1; l < kTileLevels; ++l) {
        if (l < P.Lt) {
            const int n = kTile >> l, Wl = P.w[l], Hl = P.h[l];
            const int src = l == 1 ? 0 : kTile * kTile + coarse_off(l - 1), ns = n * 2;
            const int dst = kTile * kTile + coarse_off(l);
            float *pyrl = P.pyr + P.off[l];
            for (int e = threadIdx.x; e < n * n * C; e += kThreads) {
                const int j = e / (n * C), k = e - j * (n * C), i = k / C, c = k - i * C;
                const int gi = tx * n + i, gj = ty * n + j;
                const float *q = s + c * kPlane + src + (2 * j) * ns + 2 * i;
                // the children that exist, of the frame's level l - 1 (missing ones are staged zeros)
                const int cx = 2 * gi + 1 < P.w[l - 1] ? 2 : 1, cy = 2 * gj + 1 < P.h[l - 1] ? 2 : 1;
                const float d = ((q[0] + q[1]) + (q[ns] + q[ns + 1])) * (1.f / (float) (cx * cy));
                const bool in = gi < Wl && gj < Hl;
                s[c * kPlane + dst + j * n + i] = in ? d : 0.f;
                if (in) {
                    pyrl[((long long) gj * Wl + gi) * C + c] = d;
                    acc[l] += rho<NORM>(d);
                }
            }
            __syncthreads();
        }
    }
    float *part = P.partial + ((long long) ty * P.tiles_x + tx) * kTileLevels;
#pragma unroll
    for (int l = 0; l < kTileLevels; ++l) {
        if (l < P.Lt) {
            const float t = block_sum<kThreads>(acc[l], s_red);
            if (threadIdx.x == 0) part[l] = t;
        }
    }
}

template <int C, int NORM> __global__ void __launch_bounds__(kTopThreads) k_top(Pyr P, float *__restrict__ out, int want_grad) {
    __shared__ float s_red[kTopThreads / 64];
    __shared__ float s_ll[kMaxLevels];
    const int tiles = P.tiles_x * P.tiles_y;
    // the tiles' partial sums of levels 0 .. Lt - 1: a lane adds every 1024th tile in ascending order, then the workgroup's fixed order
    for (int l = 0; l < P.Lt; ++l) {
        float a = 0.f;
        for (int t = threadIdx.x; t < tiles; t += kTopThreads) a += P.partial[(long long) t * kTileLevels + l];
        const float sum = block_sum<kTopThreads>(a, s_red);
        if (threadIdx.x == 0) s_ll[l] = sum * P.inv_n[l];
    }
    // the levels above the tiles, in the pyramid itself
    for (int l = P.Lt; l < P.L; ++l) {
        const int Wl = P.w[l], Hl = P.h[l], Ws = P.w[l - 1], Hs = P.h[l - 1];
        const float *src = P.pyr + P.off[l - 1];
        float *dst = P.pyr + P.off[l];
        float a = 0.f;
        for (int e = threadIdx.x; e < Wl * Hl * C; e += kTopThreads) {
            const int p = e / C, c = e - p * C, j = p / Wl, i = p - j * Wl;
            const bool bx = 2 * i + 1 < Ws, by = 2 * j + 1 < Hs;
            const float *q = src + ((long long) (2 * j) * Ws + 2 * i) * C + c;
            const float q00 = q[0], q10 = bx ? q[C] : 0.f, q01 = by ? q[(long long) Ws * C] : 0.f, q11 = bx && by ? q[(long long) Ws * C + C] : 0.f;
            const float d = ((q00 + q10) + (q01 + q11)) * (1.f / (float) ((bx ? 2 : 1) * (by ? 2 : 1)));
            dst[e] = d;
            a += rho<NORM>(d);
        }
        const float sum = block_sum<kTopThreads>(a, s_red);            // (its barriers also order this level's writes before the next level's reads)
        if (threadIdx.x == 0) s_ll[l] = sum * P.inv_n[l];
    }
    if (threadIdx.x == 0) {
        float loss = 0.f;
        for (int l = 0; l < P.L; ++l) {
            out[1 + l] = s_ll[l];
            loss += P.lambda[l] * s_ll[l];
        }
        out[0] = loss;
    }
    if (!want_grad) return;
    // G of levels L - 1 .. 5 (nothing when the tiles reach the top level)
    for (int l = P.L - 1; l >= kTileLog && P.L > kTileLevels; --l) {
        const int Wl = P.w[l], Hl = P.h[l];
        const float *d = P.pyr + P.off[l];
        float *g = P.gpyr + P.goff[l];
        for (int e = threadIdx.x; e < Wl * Hl * C; e += kTopThreads) {
            float v = P.coef[l] * drho<NORM>(d[e]);
            if (l + 1 < P.L) {
                const int p = e / C, c = e - p * C, j = p / Wl, i = p - j * Wl;
                const int pi = i >> 1, pj = j >> 1, Wp = P.w[l + 1];
                const int cx = 2 * pi + 1 < Wl ? 2 : 1, cy = 2 * pj + 1 < Hl ? 2 : 1;
                v += P.gpyr[P.goff[l + 1] + ((long long) pj * Wp + pi) * C + c] * (1.f / (float) (cx * cy));
            }
            g[e] = v;
        }
        __syncthreads();
    }
}

template <int C, int NORM, int WC> __global__ void __launch_bounds__(kThreads)
k_down(Pyr P, const float *__restrict__ weight, float *__restrict__ grad) {
    __shared__ float s[C * kCoarse];           // G of levels 1 .. 5
    const int tx = blockIdx.x, ty = blockIdx.y;
#pragma unroll
    for (int l = kTileLevels - 1; l >= 1; --l) {
        if (l < P.Lt) {
            const int n = kTile >> l, Wl = P.w[l], Hl = P.h[l];
            const float *dl = P.pyr + P.off[l];
            for (int e = threadIdx.x; e < n * n * C; e += kThreads) {
                const int j = e / (n * C), k = e - j * (n * C), i = k / C, c = k - i * C;
                const int gi = tx * n + i, gj = ty * n + j;
                if (gi < Wl && gj < Hl) {
                    const long long p = (long long) gj * Wl + gi;
                    float v;
                    if (l == kTileLog && P.L > kTileLevels) v = P.gpyr[P.goff[l] + p * C + c];          // k_top's: it holds this level's own term already
                    else {
                        v = P.coef[l] * drho<NORM>(dl[p * C + c]);
                        if (l + 1 < P.Lt) {
                            const int pi = gi >> 1, pj = gj >> 1;
                            const int cx = 2 * pi + 1 < Wl ? 2 : 1, cy = 2 * pj + 1 < Hl ? 2 : 1;
                            v += s[c * kCoarse + coarse_off(l + 1) + (j >> 1) * (n >> 1) + (i >> 1)] * (1.f / (float) (cx * cy));
                        }
                    }
                    s[c * kCoarse + coarse_off(l) + j * n + i] = v;
                }
            }
            __syncthreads();
        }
    }
    const int W = P.w[0], H = P.h[0];
    const float *d0 = P.pyr + P.off[0];
    for (int e = threadIdx.x; e < kTile * kTile * C; e += kThreads) {
        const int y = e / (kTile * C), k = e - y * (kTile * C), x = k / C, c = k - x * C;
        const int gx = tx * kTile + x, gy = ty * kTile + y;
        if (gx < W && gy < H) {
            const long long p = (long long) gy * W + gx;
            float v = P.coef[0] * drho<NORM>(d0[p * C + c]);
            if (P.Lt > 1) {
                const int pi = gx >> 1, pj = gy >> 1;
                const int cx = 2 * pi + 1 < W ? 2 : 1, cy = 2 * pj + 1 < H ? 2 : 1;
                v += s[c * kCoarse + (y >> 1) * (kTile / 2) + (x >> 1)] * (1.f / (float) (cx * cy));
            }
            if (WC == 1) v = weight[p] * v;
            if (WC == 2) v = weight[p * C + c] * v;
            grad[p * C + c] = v;
        }
    }
}

template <int C, int NORM> void launch_cn(const Pyr &P, int wc, const float *img, const float *target, const float *weight, float *out, float *grad, hipStream_t st) {
    const dim3 grid(P.tiles_x, P.tiles_y);
    switch (wc) {
    case 0: k_up<C, NORM, 0><<<grid, kThreads, 0, st>>>(P, img, target, weight); break;
    case 1: k_up<C, NORM, 1><<<grid, kThreads, 0, st>>>(P, img, target, weight); break;
    default: k_up<C, NORM, 2><<<grid, kThreads, 0, st>>>(P, img, target, weight); break;
    }
    k_top<C, NORM><<<1, kTopThreads, 0, st>>>(P, out, grad != nullptr);
    if (!grad) return;
    switch (wc) {
    case 0: k_down<C, NORM, 0><<<grid, kThreads, 0, st>>>(P, weight, grad); break;
    case 1: k_down<C, NORM, 1><<<grid, kThreads, 0, st>>>(P, weight, grad); break;
    default: k_down<C, NORM, 2><<<grid, kThreads, 0, st>>>(P, weight, grad); break;
    }
}

template <int C> void launch_c(const Pyr &P, int norm, int wc, const float *img, const float *target, const float *weight, float *out, float *grad, hipStream_t st) {
    if (norm == PSDR_MSLOSS_L1) launch_cn<C, PSDR_MSLOSS_L1>(P, wc, img, target, weight, out, grad, st);
    else launch_cn<C, PSDR_MSLOSS_L2>(P, wc, img, target, weight, out, grad, st);
}

int full_levels(int W, int H) {
    int L = 1;
    while (W > 1 || H > 1) { W = (W + 1) / 2; H = (H + 1) / 2; ++L; }
    return L;
}

} // namespace

struct psdr_hip_msloss {
    Pyr P{};
    int C = 0;
    bool evaluated = false;            // psdr_hip_msloss_level has something to copy
    float *block = nullptr;            // pyramid | coarse gradient | partial sums
    ~psdr_hip_msloss() { if (block) (void) hipFree(block); }
};

extern "C" {

int psdr_hip_msloss_create(int32_t W, int32_t H, int32_t levels, int32_t C, psdr_hip_msloss **out, void *stream) {
    const std::string who = "psdr_hip_msloss_create: ";
    if (!out) return psdr::api_fail(who + "out is NULL");
    *out = nullptr;
    if (W < 1 || H < 1 || W > kMaxSide || H > kMaxSide || (long long) W * H > kMaxPixels)
        return psdr::api_fail(who + "a frame of " + std::to_string(W) + " x " + std::to_string(H) + " pixels; both sides must lie in [1, 16384] and their product may be at most 2^24");
    if (C < 1 || C > 4) return psdr::api_fail(who + "C = " + std::to_string(C) + ", must be in [1, 4]");
    const int full = full_levels(W, H);
    if (levels < 1 || levels > full)
        return psdr::api_fail(who + "levels = " + std::to_string(levels) + ", must be in [1, " + std::to_string(full) + "] for " + std::to_string(W) + " x " + std::to_string(H));
    // the arguments are sound: from here on the device is touched
    psdr_hip_msloss *h = new psdr_hip_msloss();
    Pyr &P = h->P;
    h->C = C;
    P.L = levels;
    P.Lt = std::min<int>(levels, kTileLevels);
    P.tiles_x = (W + kTile - 1) / kTile;
    P.tiles_y = (H + kTile - 1) / kTile;
    long long n_pyr = 0, n_g = 0;
    for (int l = 0, w = W, hh = H; l < levels; ++l, w = (w + 1) / 2, hh = (hh + 1) / 2) {
        P.w[l] = w;
        P.h[l] = hh;
        P.off[l] = n_pyr;
        n_pyr += (long long) w * hh * C;
        P.goff[l] = n_g;
        if (l >= kTileLog) n_g += (long long) w * hh * C;
        P.inv_n[l] = (float) (1.0 / ((double) C * w * hh));
        P.lambda[l] = 1.f;
        P.coef[l] = P.inv_n[l];
    }
    const long long n_part = (long long) P.tiles_x * P.tiles_y * kTileLevels;
    hipError_t e = hipMalloc((void **) &h->block, (size_t) (n_pyr + n_g + n_part) * sizeof(float));
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t) stream);          // (nothing was queued: the frames are written by every eval before they are read)
    if (e != hipSuccess) { delete h; return psdr::api_fail(who + hipGetErrorString(e)); }
    P.pyr = h->block;
    P.gpyr = P.pyr + n_pyr;
    P.partial = P.gpyr + n_g;
    *out = h;
    return 0;
}

int psdr_hip_msloss_destroy(psdr_hip_msloss *h) {
    if (!h) return psdr::api_fail("psdr_hip_msloss_destroy: handle is NULL");
    delete h;
    return 0;
}

int psdr_hip_msloss_eval(psdr_hip_msloss *h, const float *img, const float *target, const float *weight, int32_t weight_channels, int32_t norm,
                         const float *level_weights, float *out, float *grad, void *stream) {
    const std::string who = "psdr_hip_msloss_eval: ";
    if (!h) return psdr::api_fail(who + "handle is NULL");
    if (!img || !target || !out) return psdr::api_fail(who + "NULL argument");
    if (norm != PSDR_MSLOSS_L1 && norm != PSDR_MSLOSS_L2) return psdr::api_fail(who + "norm = " + std::to_string(norm) + ", must be PSDR_MSLOSS_L1 (0) or PSDR_MSLOSS_L2 (1)");
    if (weight_channels < 0 || weight_channels > 4) return psdr::api_fail(who + "weight_channels = " + std::to_string(weight_channels) + ", must be 0, 1 or C");
    if (weight_channels > 1 && weight_channels != h->C)
        return psdr::api_fail(who + "weight_channels = " + std::to_string(weight_channels) + ", must be 0, 1 or C = " + std::to_string(h->C));
    if (weight_channels != 0 && !weight) return psdr::api_fail(who + "weight is NULL with weight_channels = " + std::to_string(weight_channels));
    if (grad && (grad == img || grad == target || grad == weight || grad == out)) return psdr::api_fail(who + "grad must be an array of its own");
    Pyr P = h->P;
    for (int l = 0; l < P.L; ++l) {
        const float lam = level_weights ? level_weights[l] : 1.f;
        if (!std::isfinite(lam)) return psdr::api_fail(who + "level_weights[" + std::to_string(l) + "] is not finite");
        P.lambda[l] = lam;
        P.coef[l] = (float) ((double) lam / ((double) h->C * P.w[l] * P.h[l]));
    }
    const int wc = weight_channels == 0 ? 0 : (weight_channels == 1 ? 1 : 2);          // (C = 1 with one channel: either form reads weight[p])
    hipStream_t st = (hipStream_t) stream;
    switch (h->C) {
    case 1: launch_c<1>(P, norm, wc, img, target, weight, out, grad, st); break;
    case 2: launch_c<2>(P, norm, wc, img, target, weight, out, grad, st); break;
    case 3: launch_c<3>(P, norm, wc, img, target, weight, out, grad, st); break;
    default: launch_c<4>(P, norm, wc, img, target, weight, out, grad, st); break;
    }
    if (launch_status(who)) return 1;
    h->evaluated = true;
    return 0;
}

int psdr_hip_msloss_level(psdr_hip_msloss *h, int32_t level, float *out, void *stream) {
    const std::string who = "psdr_hip_msloss_level: ";
    if (!h) return psdr::api_fail(who + "handle is NULL");
    if (!out) return psdr::api_fail(who + "out is NULL");
    if (level < 0 || level >= h->P.L) return psdr::api_fail(who + "level = " + std::to_string(level) + ", must be in [0, " + std::to_string(h->P.L) + ")");
    if (!h->evaluated) return psdr::api_fail(who + "the handle holds no residuals: psdr_hip_msloss_eval has not been called on it");
    const size_t bytes = (size_t) h->P.w[level] * h->P.h[level] * h->C * sizeof(float);
    const hipError_t e = hipMemcpyAsync(out, h->P.pyr + h->P.off[level], bytes, hipMemcpyDeviceToDevice, (hipStream_t) stream);
    if (e != hipSuccess) return psdr::api_fail(who + hipGetErrorString(e));
    return 0;
}

} // extern "C"
