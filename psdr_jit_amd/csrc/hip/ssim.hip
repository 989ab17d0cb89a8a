// ssim.hip — the structural-similarity loss 1 - mean SSIM and its image gradient in one fused pass (Python surface: psdr_jit_amd/ssim.py).
//
// The definition (include/psdr_hip.h states it in full).  Frame W x H, pixel (x, y) at row y W + x; img = x, target = y [W H, C], C in 1..4; mask m absent or [W H].
//   G v = the K x K Gaussian window sum of v, vertical pass of the horizontal pass, pixels outside the frame count as 0 (F.conv2d(padding = R), R = K / 2)
//   mu_x = G x, mu_y = G y, E_xx = G(x x), E_yy = G(y y), E_xy = G(x y);   s_xx = E_xx - mu_x mu_x, s_yy likewise, s_xy = E_xy - mu_x mu_y
//   a1 = 2 (mu_x mu_y) + C1, a2 = 2 s_xy + C2, b1 = (mu_x mu_x + mu_y mu_y) + C1, b2 = (s_xx + s_yy) + C2;   S = (a1 a2) / (b1 b2)
//   N = C sum m_eff;  mean = sum m_eff S / N;  loss = 1 - mean
//   P = m_eff [2 mu_y (a2 - a1) - 2 mu_x S (b2 - b1)] / (b1 b2),  Q = -m_eff S / b2,  T = m_eff 2 a1 / (b1 b2)
//   dloss / dimg = -(G P + 2 x G Q + y G T) / N:  the window is symmetric, so the adjoint of a zero-padded window sum is the same window sum - a gather, no atomics
//
// Three launches.  Tiles are 32 x 16 pixels, 256 lanes; the window size K and the channel count C are template arguments, the taps kernel arguments.
//   k_stat  one workgroup per tile: the tile and its R-pixel halo of x and y into LDS as 2 C channel planes (flat runs of (32 + 2 R) C floats per row; pixels outside the
//           frame are staged as 0, so partial tiles, frames smaller than the halo and the zero padding are one code path); per channel the horizontal pass of the five
//           quantities into LDS over 16 + 2 R rows, the vertical pass into registers (a lane owns two rows of one column and shares K - 1 of their K + 1 reads); S, P, Q, T
//           written to the handle; per tile the sums of m_eff S and m_eff in a fixed order (a lane's own elements, the wave by shuffles, the four waves in order).
//   k_sum   one workgroup: adds the tiles' partial sums in a fixed order, writes out = (1 - mean, mean) and leaves -1 / N (0 if N = 0) in the handle.
//   k_grad  one workgroup per tile: P, Q, T with their halo into LDS as 3 C planes, the same two passes, combined with x and y and the handle's scale.
// No atomics, no host synchronisation, no copy to the host: the same input gives the same bits.  No contraction in this unit (the build's -ffp-contract=off); the window
// sums use explicit fmaf, everything else is the definition's own sequence of products, sums and quotients - so that img == target gives a1 a2 == b1 b2 and S == 1.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../../include/psdr_hip.h"
#include "op_common.h"

namespace {

constexpr int kThreads = 256;           // k_stat, k_grad: 4 waves, two pixels of the tile per lane and channel
constexpr int kSumThreads = 1024;       // k_sum: one workgroup, 16 waves
constexpr int kTW = 32, kTH = 16;       // the tile: a wave covers 32 columns of 2 rows, 32 C consecutive floats per row
constexpr int kMaxK = 11;
constexpr int kMaxSide = 16384;
constexpr long long kMaxPixels = 1LL << 24;

// one staged channel plane: (16 + 2 R) rows of 32 + 2 R words, padded to 11 mod 32 words so that the C planes a flat run of a row is dealt to (about 32 / C
// consecutive columns each) start 11 banks apart: no conflict at C <= 3, two-way at C = 4, which a 4-byte LDS write absorbs
__host__ __device__ constexpr int plane_words(int K) { return (kTH + K - 1) * (kTW + K - 1) + ((11 - (kTH + K - 1) * (kTW + K - 1) % 32) + 32) % 32; }
__host__ __device__ constexpr int pass_words(int K) { return (kTH + K - 1) * kTW; }        // one quantity after the horizontal pass: 16 + 2 R rows of the tile's 32 columns

struct Frame {
    int W, H, tiles_x, tiles_y;
    int valid;                          // padding == PSDR_SSIM_VALID
    float c1, c2;
    float g[kMaxK];                     // the taps: kernel arguments, no copy in a call
    float *S, *P, *Q, *T;               // [W H, C] each
    float *partial;                     // [tiles][2]: sum m_eff S, sum m_eff
    float *scale;                       // -1 / N of the last eval, 0 if N == 0
};

// the tile's rows and halo of NSRC arrays into NSRC * C planes: plane n C + c holds channel c of array n.  Consecutive lanes read consecutive words of a row.
template <int C, int K, int NSRC> __device__ __forceinline__ void stage(float *s, const float *const (&src)[NSRC], int W, int H, int tx, int ty) {
    constexpr int R = K / 2, SW = kTW + 2 * R, SH = kTH + 2 * R, PL = plane_words(K);
    for (int e = threadIdx.x; e < SH * SW * C; e += kThreads) {
        const int r = e / (SW * C), k = e - r * (SW * C), i = k / C, c = k - i * C;
        const int gx = tx * kTW - R + i, gy = ty * kTH - R + r;
        const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;
        const long long off = ((long long) gy * W + gx) * C + c;
#pragma unroll
        for (int n = 0; n < NSRC; ++n) s[(n * C + c) * PL + r * SW + i] = in ? src[n][off] : 0.f;
    }
}

// the vertical pass: the lane's column i, rows j0 and j0 + 1 of the tile; row j of the tile needs rows j .. j + 2 R of the horizontal pass
template <int K, int NQ> __device__ __forceinline__ void vertical(const float *h, const float (&g)[kMaxK], int i, int j0, float (&acc)[2][NQ]) {
    constexpr int HP = pass_words(K);
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[0][q] = acc[1][q] = 0.f;
#pragma unroll
    for (int k = 0; k <= K; ++k) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const float v = h[q * HP + (j0 + k) * kTW + i];
            if (k < K) acc[0][q] = fmaf(g[k], v, acc[0][q]);
            if (k >= 1) acc[1][q] = fmaf(g[k - 1], v, acc[1][q]);
        }
    }
}

template <int C, int K> __global__ void __launch_bounds__(kThreads)
k_stat(Frame F, const float *__restrict__ img, const float *__restrict__ target, const float *__restrict__ mask) {
    constexpr int R = K / 2, SW = kTW + 2 * R, SH = kTH + 2 * R, PL = plane_words(K), HP = pass_words(K);
    __shared__ float s[2 * C * PL];
    __shared__ float h[5 * HP];
    __shared__ float s_red[kThreads / 64];
    const int tx = blockIdx.x, ty = blockIdx.y, W = F.W, H = F.H;
    const float *const src[2] = {img, target};
    stage<C, K, 2>(s, src, W, H, tx, ty);
    __syncthreads();
    const int i = threadIdx.x & (kTW - 1), j0 = 2 * (threadIdx.x / kTW);
    float vS[2][C], vP[2][C], vQ[2][C], vT[2][C], m[2];
    bool in[2];
    long long pix[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int gx = tx * kTW + i, gy = ty * kTH + j0 + t;
        in[t] = gx < W && gy < H;
        pix[t] = (long long) gy * W + gx;
        m[t] = in[t] ? (mask ? mask[pix[t]] : 1.f) : 0.f;
        if (F.valid && !(gx >= R && gx < W - R && gy >= R && gy < H - R)) m[t] = 0.f;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        // the horizontal pass of x, y, x x, y y, x y over the tile's columns and all staged rows
        for (int e = threadIdx.x; e < SH * kTW; e += kThreads) {
            const int r = e / kTW, col = e - r * kTW;
            const float *px = s + c * PL + r * SW + col, *py = s + (C + c) * PL + r * SW + col;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float x = px[k], y = py[k], g = F.g[k];
                a0 = fmaf(g, x, a0);
                a1 = fmaf(g, y, a1);
                a2 = fmaf(g, x * x, a2);
                a3 = fmaf(g, y * y, a3);
                a4 = fmaf(g, x * y, a4);
            }
            h[e] = a0;
            h[HP + e] = a1;
            h[2 * HP + e] = a2;
            h[3 * HP + e] = a3;
            h[4 * HP + e] = a4;
        }
        __syncthreads();
        float acc[2][5];
        vertical<K, 5>(h, F.g, i, j0, acc);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            // the definition's own sequence: every line one rounding per operation (a factor 2 is exact)
            const float mx = acc[t][0], my = acc[t][1];
            const float mxx = mx * mx, myy = my * my, mxy = mx * my;
            const float sxx = acc[t][2] - mxx, syy = acc[t][3] - myy, sxy = acc[t][4] - mxy;
            const float a1 = 2.f * mxy + F.c1, a2 = 2.f * sxy + F.c2;
            const float b1 = (mxx + myy) + F.c1, b2 = (sxx + syy) + F.c2;
            const float den = b1 * b2;
            const float S = (a1 * a2) / den;
            const float br = (2.f * my) * (a2 - a1) - ((2.f * mx) * S) * (b2 - b1);
            vS[t][c] = S;
            vP[t][c] = m[t] * (br / den);
            vQ[t][c] = -(m[t] * (S / b2));
            vT[t][c] = m[t] * ((2.f * a1) / den);
        }
        __syncthreads();                                   // (h is read: the next channel's horizontal pass may overwrite it)
    }
    float fs = 0.f, fm = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        if (in[t]) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const long long o = pix[t] * C + c;
                F.S[o] = vS[t][c];
                F.P[o] = vP[t][c];
                F.Q[o] = vQ[t][c];
                F.T[o] = vT[t][c];
                fs += m[t] * vS[t][c];
            }
            fm += m[t];
        }
    }
    const float ts = block_sum<kThreads>(fs, s_red);
    const float tm = block_sum<kThreads>(fm, s_red);
    if (threadIdx.x == 0) {
        float *part = F.partial + 2 * ((long long) ty * F.tiles_x + tx);
        part[0] = ts;
        part[1] = tm;
    }
}

template <int C> __global__ void __launch_bounds__(kSumThreads) k_sum(Frame F, float *__restrict__ out) {
    __shared__ float s_red[kSumThreads / 64];
    const int tiles = F.tiles_x * F.tiles_y;
    // a lane adds every 1024th tile in ascending order, then the workgroup's fixed order
    float a = 0.f, b = 0.f;
    for (int t = threadIdx.x; t < tiles; t += kSumThreads) {
        a += F.partial[2 * (long long) t];
        b += F.partial[2 * (long long) t + 1];
    }
    const float ss = block_sum<kSumThreads>(a, s_red);
    const float sm = block_sum<kSumThreads>(b, s_red);
    if (threadIdx.x == 0) {
        const float N = (float) C * sm;
        const float mean = N > 0.f ? ss / N : 0.f;
        out[0] = N > 0.f ? 1.f - mean : 0.f;
        out[1] = mean;
        *F.scale = N > 0.f ? -(1.f / N) : 0.f;
    }
}

template <int C, int K> __global__ void __launch_bounds__(kThreads)
k_grad(Frame F, const float *__restrict__ img, const float *__restrict__ target, float *__restrict__ grad) {
    constexpr int R = K / 2, SW = kTW + 2 * R, SH = kTH + 2 * R, PL = plane_words(K), HP = pass_words(K);
    __shared__ float s[3 * C * PL];
    __shared__ float h[3 * HP];
    const int tx = blockIdx.x, ty = blockIdx.y, W = F.W, H = F.H;
    const float *const src[3] = {F.P, F.Q, F.T};
    stage<C, K, 3>(s, src, W, H, tx, ty);
    __syncthreads();
    const int i = threadIdx.x & (kTW - 1), j0 = 2 * (threadIdx.x / kTW);
    float v[2][C][3];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        for (int e = threadIdx.x; e < SH * kTW; e += kThreads) {
            const int r = e / kTW, col = e - r * kTW;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const float *p = s + (q * C + c) * PL + r * SW + col;
                float a = 0.f;
#pragma unroll
                for (int k = 0; k < K; ++k) a = fmaf(F.g[k], p[k], a);
                h[q * HP + e] = a;
            }
        }
        __syncthreads();
        float acc[2][3];
        vertical<K, 3>(h, F.g, i, j0, acc);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int q = 0; q < 3; ++q) v[t][c][q] = acc[t][q];
        __syncthreads();
    }
    const float scale = *F.scale;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int gx = tx * kTW + i, gy = ty * kTH + j0 + t;
        if (gx < W && gy < H) {
            const long long p = (long long) gy * W + gx;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const long long o = p * C + c;
                const float a = v[t][c][0] + (2.f * img[o]) * v[t][c][1];
                grad[o] = (a + target[o] * v[t][c][2]) * scale;
            }
        }
    }
}

template <int C, int K> void launch_ck(const Frame &F, const float *img, const float *target, const float *mask, float *out, float *grad, hipStream_t st) {
    const dim3 grid(F.tiles_x, F.tiles_y);
    k_stat<C, K><<<grid, kThreads, 0, st>>>(F, img, target, mask);
    k_sum<C><<<1, kSumThreads, 0, st>>>(F, out);
    if (grad) k_grad<C, K><<<grid, kThreads, 0, st>>>(F, img, target, grad);
}

template <int C> void launch_c(const Frame &F, int K, const float *img, const float *target, const float *mask, float *out, float *grad, hipStream_t st) {
    switch (K) {
    case 3: launch_ck<C, 3>(F, img, target, mask, out, grad, st); break;
    case 5: launch_ck<C, 5>(F, img, target, mask, out, grad, st); break;
    case 7: launch_ck<C, 7>(F, img, target, mask, out, grad, st); break;
    case 9: launch_ck<C, 9>(F, img, target, mask, out, grad, st); break;
    default: launch_ck<C, 11>(F, img, target, mask, out, grad, st); break;
    }
}

} // namespace

struct psdr_hip_ssim {
    Frame F{};
    int C = 0, K = 0;
    bool evaluated = false;            // psdr_hip_ssim_map has something to copy
    float *block = nullptr;            // S | P | Q | T | partial sums | scale
    ~psdr_hip_ssim() { if (block) (void) hipFree(block); }
};

extern "C" {

int psdr_hip_ssim_create(int32_t W, int32_t H, int32_t C, int32_t window, const float *taps, float c1, float c2, int32_t padding, psdr_hip_ssim **out, void *stream) {
    const std::string who = "psdr_hip_ssim_create: ";
    if (!out) return psdr::api_fail(who + "out is NULL");
    *out = nullptr;
    if (!taps) return psdr::api_fail(who + "taps is NULL");
    if (W < 1 || H < 1 || W > kMaxSide || H > kMaxSide || (long long) W * H > kMaxPixels)
        return psdr::api_fail(who + "a frame of " + std::to_string(W) + " x " + std::to_string(H) + " pixels; both sides must lie in [1, 16384] and their product may be at most 2^24");
    if (C < 1 || C > 4) return psdr::api_fail(who + "C = " + std::to_string(C) + ", must be in [1, 4]");
    if (window < 3 || window > kMaxK || window % 2 == 0) return psdr::api_fail(who + "window = " + std::to_string(window) + ", must be odd and in [3, 11]");
    double sum = 0.0;
    for (int k = 0; k < window; ++k) {
        if (!std::isfinite(taps[k])) return psdr::api_fail(who + "taps[" + std::to_string(k) + "] is not finite");
        sum += (double) taps[k];
    }
    if (!(std::fabs(sum - 1.0) <= 1e-5)) return psdr::api_fail(who + "the taps sum to " + std::to_string(sum) + ", must be 1 within 1e-5");
    if (!std::isfinite(c1) || !(c1 > 0.f)) return psdr::api_fail(who + "c1 = " + std::to_string(c1) + ", must be finite and positive");
    if (!std::isfinite(c2) || !(c2 > 0.f)) return psdr::api_fail(who + "c2 = " + std::to_string(c2) + ", must be finite and positive");
    if (padding != PSDR_SSIM_SAME && padding != PSDR_SSIM_VALID)
        return psdr::api_fail(who + "padding = " + std::to_string(padding) + ", must be PSDR_SSIM_SAME (0) or PSDR_SSIM_VALID (1)");
    if (padding == PSDR_SSIM_VALID && (W < window || H < window))
        return psdr::api_fail(who + "valid padding needs a frame of at least window x window pixels, got " + std::to_string(W) + " x " + std::to_string(H) + " with window = " + std::to_string(window));
    // the arguments are sound: from here on the device is touched
    psdr_hip_ssim *h = new psdr_hip_ssim();
    Frame &F = h->F;
    h->C = C;
    h->K = window;
    F.W = W;
    F.H = H;
    F.tiles_x = (W + kTW - 1) / kTW;
    F.tiles_y = (H + kTH - 1) / kTH;
    F.valid = padding == PSDR_SSIM_VALID;
    F.c1 = c1;
    F.c2 = c2;
    for (int k = 0; k < kMaxK; ++k) F.g[k] = k < window ? taps[k] : 0.f;
    const long long n_map = (long long) W * H * C, n_part = 2LL * F.tiles_x * F.tiles_y;
    hipError_t e = hipMalloc((void **) &h->block, (size_t) (4 * n_map + n_part + 1) * sizeof(float));
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t) stream);          // (nothing was queued: every eval writes the maps, the partial sums and the scale before it reads them)
    if (e != hipSuccess) { delete h; return psdr::api_fail(who + hipGetErrorString(e)); }
    F.S = h->block;
    F.P = F.S + n_map;
    F.Q = F.P + n_map;
    F.T = F.Q + n_map;
    F.partial = F.T + n_map;
    F.scale = F.partial + n_part;
    *out = h;
    return 0;
}

int psdr_hip_ssim_destroy(psdr_hip_ssim *h) {
    if (!h) return psdr::api_fail("psdr_hip_ssim_destroy: handle is NULL");
    delete h;
    return 0;
}

int psdr_hip_ssim_eval(psdr_hip_ssim *h, const float *img, const float *target, const float *mask, float *out, float *grad, void *stream) {
    const std::string who = "psdr_hip_ssim_eval: ";
    if (!h) return psdr::api_fail(who + "handle is NULL");
    if (!img || !target || !out) return psdr::api_fail(who + "NULL argument");
    if (grad && (grad == img || grad == target)) return psdr::api_fail(who + "grad must be an array of its own, not img or target");
    hipStream_t st = (hipStream_t) stream;
    switch (h->C) {
    case 1: launch_c<1>(h->F, h->K, img, target, mask, out, grad, st); break;
    case 2: launch_c<2>(h->F, h->K, img, target, mask, out, grad, st); break;
    case 3: launch_c<3>(h->F, h->K, img, target, mask, out, grad, st); break;
    default: launch_c<4>(h->F, h->K, img, target, mask, out, grad, st); break;
    }
    if (launch_status(who)) return 1;
    h->evaluated = true;
    return 0;
}

int psdr_hip_ssim_map(psdr_hip_ssim *h, float *out, void *stream) {
    const std::string who = "psdr_hip_ssim_map: ";
    if (!h) return psdr::api_fail(who + "handle is NULL");
    if (!out) return psdr::api_fail(who + "out is NULL");
    if (!h->evaluated) return psdr::api_fail(who + "the handle holds no map: psdr_hip_ssim_eval has not been called on it");
    const size_t bytes = (size_t) h->F.W * h->F.H * h->C * sizeof(float);
    const hipError_t e = hipMemcpyAsync(out, h->F.S, bytes, hipMemcpyDeviceToDevice, (hipStream_t) stream);
    if (e != hipSuccess) return psdr::api_fail(who + hipGetErrorString(e));
    return 0;
}

} // extern "C"
