// denoise.hip — the edge-avoiding a-trous denoiser and its transpose (Python surface: psdr_jit_amd/denoise.py).
//
// The operator (include/psdr_hip.h states it in full).  Frame W x H, pixel p = y W + x; image x [W H, C], C in 1..4; guides g [W H, G], G in 0..8, pre-scaled.
// Level l = 0 .. L - 1 has stride s = 2^l and the taps (i, j) in {-2 .. 2}^2, h = [1, 4, 6, 4, 1] / 16:
//   q = p + s (i, j) exists only inside the frame;  d2 = sum_k (g_k(p) - g_k(q))^2;  w_l(p, q) = h(i) h(j) exp(-d2) if d2 is finite, else 0;  the centre tap is h(0)^2 always
//   N_l(p) = sum_q w_l(p, q) >= 9/64;   A_l x (p) = sum_q w_l(p, q) x(q) / N_l(p);   D = A_{L-1} ... A_0
//   w_l is symmetric, so A_l^T y (q) = sum_p w_l(q, p) (y(p) / N_l(p)): the same gather with the source pre-divided;  D^T = A_0^T ... A_{L-1}^T
// 1 / N_l depends on the guides alone: psdr_hip_denoise_create computes its L planes once, every apply and every transpose multiplies by them.
//
// One kernel template, k_level, serves the normalisers, the apply and the transpose at every stride.  The pixels with x = a, y = b (mod s) form a decimated image in which
// the level's taps are at unit stride.  A 256-thread workgroup owns a 32 x 8 tile of one such coset and stages the (32 + 4) x (8 + 4) halo of the G guide planes and the
// C value planes in LDS as planes: lane l of a half-wave reads word base + l, so consecutive lanes hit consecutive banks.  (G + C) 432 words, 20.7 KB at G = 8, C = 4:
// seven workgroups fit a CU's 160 KB.  The staging loads are s pixels apart in global memory; a form without LDS, 64 x 4 neighbouring pixels per workgroup and every
// tap a cached load, was measured against this one level by level and not kept (DESIGN.md section 7d has the table).
// The 25 taps are added in one order (j outer, i inner), the normaliser's launch and the apply's alike.  No atomics, no scatter, one launch per level: the same input
// gives the same bits.  No fast-math in this unit: the tests rest on IEEE division and exp(-0) = 1.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../../include/psdr_hip.h"

namespace psdr { int api_fail(const std::string &msg); }        // api.hip: the message psdr_hip_last_error() returns, -> 1
#define DCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return psdr::api_fail(std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

namespace {

constexpr int kThreads = 256;                               // 4 waves
constexpr int kTX = 32, kTY = 8;                            // a workgroup's tile of a coset
constexpr int kHX = kTX + 4, kHY = kTY + 4, kHalo = kHX * kHY;          // 36 x 12 = 432 words per plane
constexpr int kMaxG = 8, kMaxC = 4, kMaxL = 8;
constexpr int kMaxPixels = 1 << 24;

enum { kNorm = 0, kApply = 1, kAdjoint = 2 };

struct Level {
    int W, H, s;
    int tiles_x;                  // blockIdx.x = tile row * tiles_x + tile column, sized for coset (0, 0), the largest
    int cosets_x;                 // min(s, W): blockIdx.y = b cosets_x + a
    const float *guides;          // [G][W H]
    const float *inv_n;           // [W H], this level's 1 / N (kNorm: unused)
    const float *src;             // [W H, C] (kNorm: unused)
    float *dst;                   // [W H, C] (kNorm: [W H], 1 / N)
};

__device__ inline float tap_weight(int i, int j) {          // h(i) h(j), exact: k / 256
    const int hi = i == 0 ? 6 : ((i == 1 || i == -1) ? 4 : 1), hj = j == 0 ? 6 : ((j == 1 || j == -1) ? 4 : 1);
    return (float) (hi * hj) * (1.f / 256.f);
}

// VC: value channels (0 for kNorm)
template <int G, int VC, int MODE> __global__ void __launch_bounds__(kThreads) k_level(Level A) {
    constexpr int kPlanes = G + VC;
    __shared__ float lds[kPlanes > 0 ? kPlanes * kHalo : 1];
    const int s = A.s, n = A.W * A.H;
    const int a = (int) blockIdx.y % A.cosets_x, b = (int) blockIdx.y / A.cosets_x;
    const int wd = (A.W - a + s - 1) / s, hd = (A.H - b + s - 1) / s;          // the coset's decimated image (a < W, b < H: at least 1 x 1)
    const int tx0 = ((int) blockIdx.x % A.tiles_x) * kTX, ty0 = ((int) blockIdx.x / A.tiles_x) * kTY;
    if (tx0 >= wd || ty0 >= hd) return;                                        // a smaller coset than (0, 0): the whole workgroup leaves
    if constexpr (kPlanes > 0) {
        for (int idx = threadIdx.x; idx < kHalo; idx += kThreads) {
            const int hx = tx0 - 2 + idx % kHX, hy = ty0 - 2 + idx / kHX;
            const bool inside = hx >= 0 && hx < wd && hy >= 0 && hy < hd;
            const int q = inside ? (b + hy * s) * A.W + a + hx * s : 0;        // (inside: a frame pixel, below 2^24)
#pragma unroll
            for (int k = 0; k < G; ++k) lds[k * kHalo + idx] = inside ? A.guides[(size_t) k * n + q] : 0.f;
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
    const int lx = threadIdx.x % kTX, ly = threadIdx.x / kTX;
    const int dx = tx0 + lx, dy = ty0 + ly;
    if (dx >= wd || dy >= hd) return;                                          // (after the only barrier)
    const int p = (b + dy * s) * A.W + a + dx * s;                             // the thread's pixel
    const int centre = (ly + 2) * kHX + lx + 2;                                // and its word in a halo plane
    bool okx[5], oky[5];                                                       // tap column i - 2 / row j - 2 lies inside the frame
#pragma unroll
    for (int t = 0; t < 5; ++t) { okx[t] = (unsigned) (dx + t - 2) < (unsigned) wd; oky[t] = (unsigned) (dy + t - 2) < (unsigned) hd; }
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
            const int slot = centre + j * kHX + i;                                  // always inside the halo; a tap outside the frame reads a staged 0 and weighs 0
            float e = 1.f;
            if (i != 0 || j != 0) {
                float d2 = 0.f;
#pragma unroll
                for (int k = 0; k < G; ++k) {
                    const float d = gc[k] - lds[k * kHalo + slot];
                    d2 += d * d;
                }
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

// guides [n, G] -> planes [G][n]
__global__ void __launch_bounds__(kThreads) k_planes(const float *guides, int n, int G, float *planes) {
    const long long t = (long long) blockIdx.x * kThreads + threadIdx.x;
    if (t >= (long long) n * G) return;
    const int k = (int) (t / n), p = (int) (t % n);
    planes[t] = guides[(size_t) p * G + k];
}

template <int G, int VC, int MODE> void launch_form(const Level &A, hipStream_t st) {
    Level B = A;
    const int wd = (A.W + A.s - 1) / A.s, hd = (A.H + A.s - 1) / A.s;          // coset (0, 0)
    B.tiles_x = (wd + kTX - 1) / kTX;
    B.cosets_x = A.s < A.W ? A.s : A.W;
    const int cosets_y = A.s < A.H ? A.s : A.H;          // (at most 128 x 128 cosets: below the 65535 of a grid's y dimension)
    const long long tiles = (long long) B.tiles_x * ((hd + kTY - 1) / kTY);
    k_level<G, VC, MODE><<<dim3((unsigned) tiles, (unsigned) (B.cosets_x * cosets_y)), kThreads, 0, st>>>(B);
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
    switch (G) {
        case 0: launch_c<0, MODE>(C, A, st); break;
        case 1: launch_c<1, MODE>(C, A, st); break;
        case 2: launch_c<2, MODE>(C, A, st); break;
        case 3: launch_c<3, MODE>(C, A, st); break;
        case 4: launch_c<4, MODE>(C, A, st); break;
        case 5: launch_c<5, MODE>(C, A, st); break;
        case 6: launch_c<6, MODE>(C, A, st); break;
        case 7: launch_c<7, MODE>(C, A, st); break;
        default: launch_c<8, MODE>(C, A, st); break;
    }
}

} // namespace

struct psdr_hip_denoise {
    int W = 0, H = 0, G = 0, L = 0;
    float *d_mem = nullptr;            // guide planes [G][n] | 1 / N_l [L][n] | two work frames [n, kMaxC]
    float *planes = nullptr, *inv_n = nullptr, *work[2] = {nullptr, nullptr};
    ~psdr_hip_denoise() { if (d_mem) (void) hipFree(d_mem); }
};

namespace {

// the L levels in the order of D (kApply: 0 .. L - 1) or of D^T (kAdjoint: L - 1 .. 0), ping-pong through the work frames; the last launch writes `out`
template <int MODE> int run_levels(psdr_hip_denoise *h, const float *in, int C, float *out, hipStream_t st) {
    const size_t n = (size_t) h->W * h->H;
    const float *src = in;
    for (int k = 0; k < h->L; ++k) {
        const int l = MODE == kApply ? k : h->L - 1 - k;
        float *dst = k == h->L - 1 ? out : h->work[k & 1];
        Level A{h->W, h->H, 1 << l, 0, 0, h->planes, h->inv_n + (size_t) l * n, src, dst};
        launch_level<MODE>(h->G, C, A, st);
        src = dst;
    }
    DCHK(hipGetLastError());
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
    const std::string me = "psdr_hip_denoise_create: ";
    if (!out) return psdr::api_fail(me + "out is NULL");
    *out = nullptr;
    if (G < 0 || G > kMaxG) return psdr::api_fail(me + "G = " + std::to_string(G) + ", must lie in [0, 8]");
    if (G > 0 && !guides) return psdr::api_fail(me + "guides is NULL");
    if (W < 1 || H < 1) return psdr::api_fail(me + "W = " + std::to_string(W) + ", H = " + std::to_string(H) + ", must be positive");
    if ((int64_t) W * H > kMaxPixels) return psdr::api_fail(me + "W H = " + std::to_string((int64_t) W * H) + " is above 2^24");
    if (L < 1 || L > kMaxL) return psdr::api_fail(me + "L = " + std::to_string(L) + ", must lie in [1, 8]");
    // the arguments are sound: from here on the device is touched
    hipStream_t st = (hipStream_t) stream;
    psdr_hip_denoise *h = new psdr_hip_denoise();
    h->W = W; h->H = H; h->G = G; h->L = L;
    const size_t n = (size_t) W * H;
    const hipError_t e = hipMalloc((void **) &h->d_mem, ((size_t) G + L + 2 * kMaxC) * n * sizeof(float));
    if (e != hipSuccess) { delete h; return psdr::api_fail(me + hipGetErrorString(e)); }
    h->planes = h->d_mem;
    h->inv_n = h->planes + (size_t) G * n;
    h->work[0] = h->inv_n + (size_t) L * n;
    h->work[1] = h->work[0] + (size_t) kMaxC * n;
    if (G > 0) k_planes<<<(unsigned) ((n * G + kThreads - 1) / kThreads), kThreads, 0, st>>>(guides, (int) n, G, h->planes);
    for (int l = 0; l < L; ++l) {
        Level A{W, H, 1 << l, 0, 0, h->planes, nullptr, nullptr, h->inv_n + (size_t) l * n};
        launch_level<kNorm>(G, 0, A, st);
    }
    const hipError_t e2 = hipGetLastError();
    if (e2 != hipSuccess) { delete h; return psdr::api_fail(me + hipGetErrorString(e2)); }
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
