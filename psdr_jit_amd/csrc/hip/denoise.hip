// denoise.hip — the edge-avoiding a-trous denoiser and its transpose (Python surface: psdr_jit_amd/denoise.py).
//
// The operator (include/psdr_hip.h states it in full).  Frame W x H, pixel p = y W + x; image x [W H, C], C in 1..4; guides g [W H, G], G in 0..8, pre-scaled.
// Level l = 0 .. L - 1 has stride s = 2^l and the taps (i, j) in {-2 .. 2}^2, h = [1, 4, 6, 4, 1] / 16:
//   q = p + s (i, j) exists only inside the frame;  d2 = sum_k (g_k(p) - g_k(q))^2;  w_l(p, q) = h(i) h(j) exp(-d2) if d2 is finite, else 0;  the centre tap is h(0)^2 always
//   N_l(p) = sum_q w_l(p, q) >= 9/64;   A_l x (p) = sum_q w_l(p, q) x(q) / N_l(p);   D = A_{L-1} ... A_0
//   w_l is symmetric, so A_l^T y (q) = sum_p w_l(q, p) (y(p) / N_l(p)): the same gather with the source pre-divided;  D^T = A_0^T ... A_{L-1}^T
// 1 / N_l depends on the guides alone: psdr_hip_denoise_create computes its L planes once, every apply and every transpose multiplies by them.
//
// One kernel template, k_level, serves the normalisers, the apply and the transpose at every stride, on the tile scheme of atrous.h: it stages the G guide planes and
// the C value planes, (G + C) 432 words, 20.7 KB at G = 8, C = 4: seven workgroups fit a CU.  The normaliser's launch and the apply's add the 25 taps in the same order.
// No fast-math and no contraction in this unit: the tests rest on IEEE division and exp(-0) = 1.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../../include/psdr_hip.h"
#include "atrous.h"

using namespace psdr::atrous;

namespace {

constexpr int kMaxC = 4;

enum { kNorm = 0, kApply = 1, kAdjoint = 2 };

struct Level : Frame {
    const float *guides;          // [G][W H]
    const float *inv_n;           // [W H], this level's 1 / N (kNorm: unused)
    const float *src;             // [W H, C] (kNorm: unused)
    float *dst;                   // [W H, C] (kNorm: [W H], 1 / N)
};

// VC: value channels (0 for kNorm)
template <int G, int VC, int MODE> __global__ void __launch_bounds__(kThreads) k_level(Level A) {
    constexpr int kPlanes = G + VC;
    __shared__ float lds[kPlanes > 0 ? kPlanes * kHalo : 1];
    ATROUS_TILE(A, blockIdx, return);                                          // s, n, the coset (a, b), wd x hd, the tile's origin (tx0, ty0)
    if constexpr (kPlanes > 0) {
        for (int idx = threadIdx.x; idx < kHalo; idx += kThreads) {
            ATROUS_HALO_SLOT(A, idx);                                          // inside, q
            ATROUS_STAGE_GUIDES(G, lds, A.guides, idx);
            if constexpr (VC > 0) {
                const float scale = MODE == kAdjoint ? (inside ? A.inv_n[q] : 0.f) : 1.f;
#pragma unroll
                for (int c = 0; c < VC; ++c) {
                    const float v = inside ? A.src[(size_t) q * VC + c] : 0.f;
                    lds[(G + c) * kHalo + idx] = MODE == kAdjoint ? v * scale : v;
                }
            }
        }
        __syncthreads();
    }
    ATROUS_PIXEL(A, threadIdx.x, return);                                      // the thread's pixel p, its halo word `centre`, okx / oky
    float gc[G > 0 ? G : 1];
#pragma unroll
    for (int k = 0; k < G; ++k) gc[k] = lds[k * kHalo + centre];
    float acc[VC > 0 ? VC : 1];
#pragma unroll
    for (int c = 0; c < (VC > 0 ? VC : 1); ++c) acc[c] = 0.f;
#pragma unroll
    for (int j = -2; j <= 2; ++j) {
#pragma unroll
        for (int i = -2; i <= 2; ++i) {
            const bool ok = okx[i + 2] && oky[j + 2];
            const int slot = centre + j * kHX + i;                                  // a tap outside the frame reads a staged 0 and weighs 0
            float e = 1.f;
            if (i != 0 || j != 0) {
                const float d2 = guide_d2<G>(gc, lds, slot);
                e = d2 <= __FLT_MAX__ ? expf(-d2) : 0.f;                            // (NaN and Inf fail the comparison)
            }
            const float w = ok ? tap_weight(i, j) * e : 0.f;
            if constexpr (MODE == kNorm) acc[0] += w;
            else {
#pragma unroll
                for (int c = 0; c < VC; ++c) acc[c] += w * lds[(G + c) * kHalo + slot];
            }
        }
    }
    if constexpr (MODE == kNorm) A.dst[p] = 1.f / acc[0];
    else {
        const float scale = MODE == kApply ? A.inv_n[p] : 1.f;
#pragma unroll
        for (int c = 0; c < VC; ++c) A.dst[(size_t) p * VC + c] = MODE == kApply ? acc[c] * scale : acc[c];
    }
}

template <int G, int VC, int MODE> void launch_form(Level A, hipStream_t st) {
    const Grid grid = level_grid(A);
    k_level<G, VC, MODE><<<dim3(grid.x, grid.y), kThreads, 0, st>>>(A);
}

template <int G, int MODE> void launch_c(int C, const Level &A, hipStream_t st) {
    if constexpr (MODE == kNorm) launch_form<G, 0, kNorm>(A, st);
    else switch (C) {
        case 1: launch_form<G, 1, MODE>(A, st); break;
        case 2: launch_form<G, 2, MODE>(A, st); break;
        case 3: launch_form<G, 3, MODE>(A, st); break;
        default: launch_form<G, 4, MODE>(A, st); break;
    }
}

template <int MODE> void launch_level(int G, int C, const Level &A, hipStream_t st) {
    dispatch_g(G, [&](auto g) { launch_c<decltype(g)::value, MODE>(C, A, st); });
}

} // namespace

struct psdr_hip_denoise : Handle {           // the block: guide planes [G][n] | 1 / N_l [L][n] | two work frames [n, kMaxC]
    float *inv_n = nullptr, *work[2] = {nullptr, nullptr};
};

namespace {

// D (kApply: levels 0 .. L - 1) or D^T (kAdjoint: L - 1 .. 0)
template <int MODE> int run_levels(psdr_hip_denoise *h, const float *in, int C, float *out, hipStream_t st) {
    ping_pong(h->L, MODE == kApply, in, out, h->work, [&](int l, const float *src, float *dst) {
        launch_level<MODE>(h->G, C, Level{{h->W, h->H, 1 << l, 0, 0}, h->planes, h->inv_n + l * h->pixels(), src, dst}, st);
    });
    ATROUS_CHK(hipGetLastError());
    return 0;
}

const char *check_call(const psdr_hip_denoise *h, const float *in, int32_t C, const float *out) {
    if (!h) return "handle is NULL";
    if (!in || !out) return "NULL argument";
    if (C < 1 || C > kMaxC) return "C must lie in [1, 4]";
    if (in == out) return "in and out must be different arrays";
    return nullptr;
}

} // namespace

extern "C" {

int psdr_hip_denoise_create(const float *guides, int32_t G, int32_t W, int32_t H, int32_t L, psdr_hip_denoise **out, void *stream) {
    const char *me = "psdr_hip_denoise_create";
    const std::string why = check_create(me, guides, G, W, H, L, out);
    if (out) *out = nullptr;
    if (!why.empty()) return psdr::api_fail(why);
    // the arguments are sound: from here on the device is touched
    hipStream_t st = (hipStream_t) stream;
    psdr_hip_denoise *h = new psdr_hip_denoise();
    hipError_t e = h->init(guides, G, W, H, L, (size_t) L + 2 * kMaxC, st);
    if (e == hipSuccess) {
        const size_t n = h->pixels();
        h->inv_n = h->planes + (size_t) G * n;
        h->work[0] = h->inv_n + (size_t) L * n;
        h->work[1] = h->work[0] + (size_t) kMaxC * n;
        for (int l = 0; l < L; ++l) launch_level<kNorm>(G, 0, Level{{W, H, 1 << l, 0, 0}, h->planes, nullptr, nullptr, h->inv_n + (size_t) l * n}, st);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(st);          // the handle is usable on any stream and `guides` is the caller's again when the call returns
    }
    if (e != hipSuccess) { delete h; return psdr::api_fail(std::string(me) + ": " + hipGetErrorString(e)); }
    *out = h;
    return 0;
}

int psdr_hip_denoise_destroy(psdr_hip_denoise *h) {
    if (!h) return psdr::api_fail("psdr_hip_denoise_destroy: handle is NULL");
    delete h;
    return 0;
}

int psdr_hip_denoise_apply(psdr_hip_denoise *h, const float *in, int32_t C, float *out, void *stream) {
    if (const char *why = check_call(h, in, C, out)) return psdr::api_fail(std::string("psdr_hip_denoise_apply: ") + why);
    return run_levels<kApply>(h, in, C, out, (hipStream_t) stream);
}

int psdr_hip_denoise_apply_adj(psdr_hip_denoise *h, const float *d_out, int32_t C, float *d_in, void *stream) {
    if (const char *why = check_call(h, d_out, C, d_in)) return psdr::api_fail(std::string("psdr_hip_denoise_apply_adj: ") + why);
    return run_levels<kAdjoint>(h, d_out, C, d_in, (hipStream_t) stream);
}

} // extern "C"
