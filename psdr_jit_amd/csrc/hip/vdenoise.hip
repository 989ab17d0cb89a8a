// vdenoise.hip — the variance-guided a-trous denoiser, its frozen operator and that operator's transpose (Python surface: psdr_jit_amd/vdenoise.py).
//
// The operator (include/psdr_hip.h states it in full).  Frame W x H, pixel p = y W + x; image x [W H, C], C in {1, 3}; variance v [W H] of the pixel's luminance estimate;
// guides g [W H, G], G in 0..8, pre-scaled; luminance coefficients a[C]; k = 1 / sigma_l^2 >= 0, eps > 0.  State (x_l, v_l), x_0 = x, v_0 = v.  Level l = 0 .. L - 1 has
// stride s = 2^l and the taps (i, j) in {-2 .. 2}^2, h = [1, 4, 6, 4, 1] / 16:
//   lum_l(p) = a_0 x_l,0(p) + a_1 x_l,1(p) + a_2 x_l,2(p)                   (this order, no contraction)
//   vt_l(p)  = the [1, 2, 1] x [1, 2, 1] average of v_l over the UNIT-stride 3 x 3 taps inside the frame, divided by the sum of the coefficients that were inside
//   q = p + s (i, j) exists only inside the frame;  d2 = sum_k (g_k(p) - g_k(q))^2;  z = k (lum_l(p) - lum_l(q))^2 / (vt_l(p) + vt_l(q) + eps)
//   w_l(p, q) = h(i) h(j) exp(-(d2 + z)) if 0 <= d2 + z < inf and vt_l(p) + vt_l(q) + eps is finite, else 0;  the centre tap is h(0)^2 always;  a tap of weight 0 adds nothing, whatever x(q) or v(q) hold
//   N_l(p) = sum_q w_l(p, q);   x_{l+1}(p) = sum_q w_l(p, q) x_l(q) / N_l(p);   v_{l+1}(p) = sum_q w_l(p, q)^2 v_l(q) / N_l(p)^2
// An apply RECORDS lum_l, vt_l and 1 / N_l, three planes per level.  The frozen operator D_x = A_{L-1} ... A_0 forms the weights from the record and is linear in what it
// is applied to; w_l is symmetric, so A_l^T y (q) = sum_p w_l(q, p) (y(p) / N_l(p)): the same gather with the source pre-multiplied by 1 / N_l, no scatter, no atomics.
//
// k_prefilter: v_l -> vt_l, one thread per pixel, nine cached loads.  k_vlevel<G, C, mode>: one launch per level, on the tile scheme of atrous.h; it stages the G guides,
// the C values, lum, vt and, in apply mode, v - at most 14 planes of 432 words, 24.2 KB, six workgroups to a CU.  Apply mode forms lum while it stages; the frozen modes
// read the recorded plane, and form z and w with the SAME float32 expression sequence (one function, weight()), so that frozen(x) after apply(x, v) gives apply's bits.
// The 25 taps are unrolled and added in one order (j outer, i inner).  No fast-math, no contraction in this unit: with k = 0 the image part gives the bits of denoise.hip.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../../include/psdr_hip.h"
#include "atrous.h"

using namespace psdr::atrous;

namespace {

constexpr int kMaxC = 3;

enum { kApply = 0, kFrozen = 1, kFrozenAdj = 2 };

struct VLevel : Frame {
    const float *guides;          // [G][W H]
    const float *src;             // [W H, C]
    const float *v;               // [W H], v_l (kApply only)
    const float *vt;              // [W H], the record's vt_l (kApply: k_prefilter has just written it)
    float *lum;                   // [W H], the record's lum_l: kApply writes it, the frozen modes read it
    float *inv_n;                 // [W H], the record's 1 / N_l: kApply writes it, the frozen modes read it
    float *dst;                   // [W H, C]
    float *v_out;                 // [W H], v_{l+1} (kApply only)
    float a[3];                   // luminance coefficients (kApply only)
    float k, eps;
};

// exp(-(d2 + z)), the one expression sequence of all three modes
__device__ inline float weight(float d2, float lp, float lq, float vp, float vq, float k, float eps) {
    const float dl = lp - lq;
    const float den = (vp + vq) + eps;
    const float z = k * (dl * dl) / den;
    const float t = d2 + z;
    return (t >= 0.f && t <= __FLT_MAX__ && fabsf(den) <= __FLT_MAX__) ? expf(-t) : 0.f;          // (NaN, Inf and a negative argument fail the comparisons)
}

template <int G, int C, int MODE> __global__ void __launch_bounds__(kThreads) k_vlevel(VLevel A) {
    constexpr int kLum = G + C, kVt = G + C + 1, kV = G + C + 2;
    constexpr int kPlanes = G + C + (MODE == kApply ? 3 : 2);
    __shared__ float lds[kPlanes * kHalo];
    ATROUS_TILE(A, blockIdx, return);                                          // s, n, the coset (a, b), wd x hd, the tile's origin (tx0, ty0)
    for (int idx = threadIdx.x; idx < kHalo; idx += kThreads) {
        ATROUS_HALO_SLOT(A, idx);                                              // inside, q
        ATROUS_STAGE_GUIDES(G, lds, A.guides, idx);
        const float scale = MODE == kFrozenAdj ? (inside ? A.inv_n[q] : 0.f) : 1.f;
        float x[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            x[c] = inside ? A.src[(size_t) q * C + c] : 0.f;
            lds[(G + c) * kHalo + idx] = MODE == kFrozenAdj ? x[c] * scale : x[c];
        }
        if constexpr (MODE == kApply) {
            float lum = A.a[0] * x[0];
#pragma unroll
            for (int c = 1; c < C; ++c) lum = lum + A.a[c] * x[c];
            lds[kLum * kHalo + idx] = lum;
            lds[kV * kHalo + idx] = inside ? A.v[q] : 0.f;
        } else {
            lds[kLum * kHalo + idx] = inside ? A.lum[q] : 0.f;
        }
        lds[kVt * kHalo + idx] = inside ? A.vt[q] : 0.f;
    }
    __syncthreads();
    ATROUS_PIXEL(A, threadIdx.x, return);                                      // the thread's pixel p, its halo word `centre`, okx / oky
    float gc[G > 0 ? G : 1];
#pragma unroll
    for (int g = 0; g < G; ++g) gc[g] = lds[g * kHalo + centre];
    const float lc = lds[kLum * kHalo + centre], vc = lds[kVt * kHalo + centre];
    float acc[C], acc_n = 0.f, acc_v = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.f;
#pragma unroll
    for (int j = -2; j <= 2; ++j) {
#pragma unroll
        for (int i = -2; i <= 2; ++i) {
            const bool ok = okx[i + 2] && oky[j + 2];
            const int slot = centre + j * kHX + i;                                  // a tap outside the frame weighs 0
            float e = 1.f;
            if (i != 0 || j != 0) {
                const float d2 = guide_d2<G>(gc, lds, slot);
                e = weight(d2, lc, lds[kLum * kHalo + slot], vc, lds[kVt * kHalo + slot], A.k, A.eps);
            }
            const float w = ok ? tap_weight(i, j) * e : 0.f;
            const bool live = w > 0.f;                                              // a tap of weight 0 adds nothing: a cut-off pixel's NaN stays where it is
            if constexpr (MODE == kApply) {
                acc_n += w;
                acc_v += live ? (w * w) * lds[kV * kHalo + slot] : 0.f;
            }
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += live ? w * lds[(G + c) * kHalo + slot] : 0.f;
        }
    }
    if constexpr (MODE == kApply) {
        const float inv = 1.f / acc_n;                                             // one IEEE division; N >= h(0)^2
        A.lum[p] = lc;
        A.inv_n[p] = inv;
        A.v_out[p] = (acc_v * inv) * inv;
#pragma unroll
        for (int c = 0; c < C; ++c) A.dst[(size_t) p * C + c] = acc[c] * inv;
    } else if constexpr (MODE == kFrozen) {
        const float inv = A.inv_n[p];
#pragma unroll
        for (int c = 0; c < C; ++c) A.dst[(size_t) p * C + c] = acc[c] * inv;
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) A.dst[(size_t) p * C + c] = acc[c];
    }
}

// v_l -> vt_l: coefficients 1 2 1 / 2 4 2 / 1 2 1 (the common 1 / 16 cancels) over the taps inside the frame, row by row, divided by their sum
__global__ void __launch_bounds__(kThreads) k_prefilter(const float *v, int W, int H, float *vt) {
    const int p = (int) (blockIdx.x * kThreads + threadIdx.x);
    if (p >= W * H) return;
    const int x = p % W, y = p / W;
    float acc = 0.f, sum = 0.f;
#pragma unroll
    for (int j = -1; j <= 1; ++j) {
#pragma unroll
        for (int i = -1; i <= 1; ++i) {
            const bool ok = (unsigned) (x + i) < (unsigned) W && (unsigned) (y + j) < (unsigned) H;
            const float c = (float) ((i == 0 ? 2 : 1) * (j == 0 ? 2 : 1));
            if (ok) { acc += c * v[p + j * W + i]; sum += c; }
        }
    }
    vt[p] = acc / sum;
}

template <int G, int C, int MODE> void launch_form(VLevel A, hipStream_t st) {
    const Grid grid = level_grid(A);
    k_vlevel<G, C, MODE><<<dim3(grid.x, grid.y), kThreads, 0, st>>>(A);
}

template <int G, int MODE> void launch_c(int C, const VLevel &A, hipStream_t st) {
    if (C == 1) launch_form<G, 1, MODE>(A, st);
    else launch_form<G, 3, MODE>(A, st);
}

template <int MODE> void launch_level(int G, int C, const VLevel &A, hipStream_t st) {
    dispatch_g(G, [&](auto g) { launch_c<decltype(g)::value, MODE>(C, A, st); });
}

} // namespace

struct psdr_hip_vdenoise : Handle {          // the block: guide planes [G][n] | record [L][3][n]: lum_l, vt_l, 1 / N_l | two work frames [n, kMaxC] | two variance frames [n]
    bool recorded = false;
    float k = 0.f, eps = 0.f;          // of the record
    float *record = nullptr, *work[2] = {nullptr, nullptr}, *vwork[2] = {nullptr, nullptr};
};

namespace {

const char *check_frozen(const psdr_hip_vdenoise *h, const float *in, int32_t C, const float *out) {
    if (!h) return "handle is NULL";
    if (!in || !out) return "NULL argument";
    if (C != 1 && C != 3) return "C must be 1 or 3";
    if (in == out) return "in and out must be different arrays";
    if (!h->recorded) return "the handle holds no record: an apply makes one";
    return nullptr;
}

// D_x (kFrozen: the recorded levels 0 .. L - 1) or D_x^T (kFrozenAdj: L - 1 .. 0)
template <int MODE> int run_frozen(psdr_hip_vdenoise *h, const float *in, int C, float *out, hipStream_t st) {
    const size_t n = h->pixels();
    ping_pong(h->L, MODE == kFrozen, in, out, h->work, [&](int l, const float *src, float *dst) {
        float *rec = h->record + (size_t) l * 3 * n;
        launch_level<MODE>(h->G, C, VLevel{{h->W, h->H, 1 << l, 0, 0}, h->planes, src, nullptr, rec + n, rec, rec + 2 * n, dst, nullptr, {0.f, 0.f, 0.f}, h->k, h->eps}, st);
    });
    ATROUS_CHK(hipGetLastError());
    return 0;
}

} // namespace

extern "C" {

int psdr_hip_vdenoise_create(const float *guides, int32_t G, int32_t W, int32_t H, int32_t L, psdr_hip_vdenoise **out, void *stream) {
    const char *me = "psdr_hip_vdenoise_create";
    const std::string why = check_create(me, guides, G, W, H, L, out);
    if (out) *out = nullptr;
    if (!why.empty()) return psdr::api_fail(why);
    // the arguments are sound: from here on the device is touched
    psdr_hip_vdenoise *h = new psdr_hip_vdenoise();
    hipError_t e = h->init(guides, G, W, H, L, 3 * (size_t) L + 2 * kMaxC + 2, (hipStream_t) stream);
    if (e == hipSuccess) {
        const size_t n = h->pixels();
        h->record = h->planes + (size_t) G * n;
        h->work[0] = h->record + 3 * (size_t) L * n;
        h->work[1] = h->work[0] + (size_t) kMaxC * n;
        h->vwork[0] = h->work[1] + (size_t) kMaxC * n;
        h->vwork[1] = h->vwork[0] + n;
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t) stream);          // the handle is usable on any stream and `guides` is the caller's again when the call returns
    }
    if (e != hipSuccess) { delete h; return psdr::api_fail(std::string(me) + ": " + hipGetErrorString(e)); }
    *out = h;
    return 0;
}

int psdr_hip_vdenoise_destroy(psdr_hip_vdenoise *h) {
    if (!h) return psdr::api_fail("psdr_hip_vdenoise_destroy: handle is NULL");
    delete h;
    return 0;
}

int psdr_hip_vdenoise_apply(psdr_hip_vdenoise *h, const float *in, int32_t C, const float *var, const float *lum, float k, float eps, float *out, float *var_out, void *stream) {
    const std::string me = "psdr_hip_vdenoise_apply: ";
    if (!h) return psdr::api_fail(me + "handle is NULL");
    if (!in || !var || !lum || !out) return psdr::api_fail(me + "NULL argument");
    if (C != 1 && C != 3) return psdr::api_fail(me + "C must be 1 or 3");
    if (in == out) return psdr::api_fail(me + "in and out must be different arrays");
    if (var == var_out) return psdr::api_fail(me + "var and var_out must be different arrays");
    if (!(k >= 0.f) || !(k <= __FLT_MAX__)) return psdr::api_fail(me + "k = " + std::to_string(k) + ", must be finite and not negative");
    if (!(eps > 0.f) || !(eps <= __FLT_MAX__)) return psdr::api_fail(me + "eps = " + std::to_string(eps) + ", must be finite and positive");
    for (int c = 0; c < C; ++c)
        if (!(std::fabs(lum[c]) <= __FLT_MAX__)) return psdr::api_fail(me + "lum[" + std::to_string(c) + "] is not finite");
    hipStream_t st = (hipStream_t) stream;
    const size_t n = (size_t) h->W * h->H;
    h->recorded = false;                                   // a failed launch leaves no half-written record behind
    const float *src = in, *vsrc = var;
    for (int l = 0; l < h->L; ++l) {
        const bool last = l == h->L - 1;
        float *dst = last ? out : h->work[l & 1];
        float *vdst = last && var_out ? var_out : h->vwork[l & 1];
        float *rec = h->record + (size_t) l * 3 * n;
        k_prefilter<<<(unsigned) ((n + kThreads - 1) / kThreads), kThreads, 0, st>>>(vsrc, h->W, h->H, rec + n);
        VLevel A{h->W, h->H, 1 << l, 0, 0, h->planes, src, vsrc, rec + n, rec, rec + 2 * n, dst, vdst, {lum[0], C > 1 ? lum[1] : 0.f, C > 1 ? lum[2] : 0.f}, k, eps};
        launch_level<kApply>(h->G, C, A, st);
        src = dst;
        vsrc = vdst;
    }
    ATROUS_CHK(hipGetLastError());
    h->k = k; h->eps = eps;
    h->recorded = true;
    return 0;
}

int psdr_hip_vdenoise_frozen(psdr_hip_vdenoise *h, const float *in, int32_t C, float *out, void *stream) {
    if (const char *why = check_frozen(h, in, C, out)) return psdr::api_fail(std::string("psdr_hip_vdenoise_frozen: ") + why);
    return run_frozen<kFrozen>(h, in, C, out, (hipStream_t) stream);
}

int psdr_hip_vdenoise_frozen_adj(psdr_hip_vdenoise *h, const float *d_out, int32_t C, float *d_in, void *stream) {
    if (const char *why = check_frozen(h, d_out, C, d_in)) return psdr::api_fail(std::string("psdr_hip_vdenoise_frozen_adj: ") + why);
    return run_frozen<kFrozenAdj>(h, d_out, C, d_in, (hipStream_t) stream);
}

int psdr_hip_vdenoise_record(psdr_hip_vdenoise *h, float *out, void *stream) {
    const std::string me = "psdr_hip_vdenoise_record: ";
    if (!h) return psdr::api_fail(me + "handle is NULL");
    if (!out) return psdr::api_fail(me + "NULL argument");
    if (!h->recorded) return psdr::api_fail(me + "the handle holds no record: an apply makes one");
    ATROUS_CHK(hipMemcpyAsync(out, h->record, 3 * (size_t) h->L * h->W * h->H * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t) stream));
    return 0;
}

} // extern "C"
