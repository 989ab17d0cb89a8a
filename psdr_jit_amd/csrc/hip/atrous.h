// atrous.h — what the a-trous units (denoise.hip, vdenoise.hip) share: the tile scheme of one level, stated once.
//
// A level of stride s = 2^l has the taps q = p + s (i, j), (i, j) in {-2 .. 2}^2, h = [1, 4, 6, 4, 1] / 16.  The pixels with x = a, y = b (mod s) form a decimated image
// (a coset, wd x hd pixels) in which those taps are at unit stride.  A 256-thread workgroup owns a 32 x 8 tile of one coset and stages the (32 + 4) x (8 + 4) halo of every
// plane it needs in LDS as planes of 432 words: lane l of a half-wave reads word base + l, so consecutive lanes hit consecutive banks, whatever the row stride of 36.
// blockIdx.y is the coset, blockIdx.x the tile; the grid is sized for coset (0, 0), the largest, and a workgroup without a tile in a smaller coset leaves at once.  The
// staging loads are s pixels apart in global memory; a form without LDS, 64 x 4 neighbouring pixels per workgroup and every tap a cached load, was measured against this
// one level by level and not kept (DESIGN.md section 7d has the table).  A slot of the halo outside the coset is staged as 0 and its tap weighs 0.
// The 25 taps are added in one order (j outer, i inner) by every kernel of both units.  No atomics, no scatter, one launch per level: the same input gives the same bits,
// and with the luminance weight off vdenoise.hip gives the bits of denoise.hip - which rests on both decoding cosets, staging halos and forming d2 through THIS file.
// No fast-math and no contraction in these units: the tests rest on IEEE division and exp(-0) = 1.
//
// The first part - the launch grid and the decode macros - is plain C++, no HIP include: tests/cpp/atrous_cover_check.cpp compiles it with g++ and walks whole grids through
// the decode the kernels expand.
#pragma once
#include <cstdint>
#include <string>

namespace psdr {
namespace atrous {

constexpr int kThreads = 256;                               // 4 waves
constexpr int kTX = 32, kTY = 8;                            // a workgroup's tile of a coset
constexpr int kHX = kTX + 4, kHY = kTY + 4, kHalo = kHX * kHY;          // 36 x 12 = 432 words per plane
constexpr int kMaxG = 8, kMaxL = 8;
constexpr int kMaxPixels = 1 << 24;

// the head of a level kernel's argument: the frame, the stride, and how the grid numbers tiles and cosets (level_grid fills the last two)
struct Frame {
    int W, H, s;
    int tiles_x;                  // blockIdx.x = tile row * tiles_x + tile column, sized for coset (0, 0), the largest
    int cosets_x;                 // min(s, W): blockIdx.y = b cosets_x + a
};

struct Grid { unsigned x, y; };
inline Grid level_grid(Frame &F) {
    const int wd = (F.W + F.s - 1) / F.s, hd = (F.H + F.s - 1) / F.s;          // coset (0, 0)
    F.tiles_x = (wd + kTX - 1) / kTX;
    F.cosets_x = F.s < F.W ? F.s : F.W;
    const int cosets_y = F.s < F.H ? F.s : F.H;          // (at most 128 x 128 cosets: below the 65535 of a grid's y dimension)
    const long long tiles = (long long) F.tiles_x * ((hd + kTY - 1) / kTY);
    return Grid{(unsigned) tiles, (unsigned) (F.cosets_x * cosets_y)};
}

// The device-side decode, three steps that a level kernel takes in this order.  They are macros that declare the kernel's locals, not functions: the compiler
// optimises a function on its own before it inlines it, and with the decode in functions most instantiations of k_level / k_vlevel came out with other instruction
// streams than with the statements in place (other register counts in 27 of them, another occupancy in two).  Expanded in place, both units compile to what each
// compiled to when it held its own copy.  F: the kernel's argument (a Frame); LEAVE: the statement that ends the workgroup's or the thread's work (`return`).
#if defined(__HIPCC__)
#define ATROUS_UNROLL _Pragma("unroll")
#else
#define ATROUS_UNROLL
#endif
//
// 1. the workgroup: s, n = W H, its coset (a, b), that coset's decimated image wd x hd (a < W, b < H: at least 1 x 1), its tile's origin (tx0, ty0);
//    a smaller coset than (0, 0) lacks the last tiles, and such a workgroup leaves as a whole.  block: blockIdx
#define ATROUS_TILE(F, block, LEAVE) \
    const int s = (F).s, n = (F).W * (F).H; \
    const int a = (int) (block).y % (F).cosets_x, b = (int) (block).y / (F).cosets_x; \
    const int wd = ((F).W - a + s - 1) / s, hd = ((F).H - b + s - 1) / s; \
    const int tx0 = ((int) (block).x % (F).tiles_x) * psdr::atrous::kTX, ty0 = ((int) (block).x / (F).tiles_x) * psdr::atrous::kTY; \
    if (tx0 >= wd || ty0 >= hd) LEAVE
// 2. word idx of a halo plane: `inside` and the frame pixel q staged there (below 2^24); where the halo leaves the coset, inside is false, q = 0 and the kernels stage 0
#define ATROUS_HALO_SLOT(F, idx) \
    const int hx = tx0 - 2 + (idx) % psdr::atrous::kHX, hy = ty0 - 2 + (idx) / psdr::atrous::kHX; \
    const bool inside = hx >= 0 && hx < wd && hy >= 0 && hy < hd; \
    const int q = inside ? (b + hy * s) * (F).W + a + hx * s : 0
//    ... and the G guide planes [G][n] of that word into the first G planes of lds
#define ATROUS_STAGE_GUIDES(G, lds, guides, idx) \
    ATROUS_UNROLL \
    for (int k = 0; k < (G); ++k) (lds)[k * psdr::atrous::kHalo + (idx)] = inside ? (guides)[(size_t) k * n + q] : 0.f
// 3. (after the only barrier) the thread: its place (dx, dy) in the coset - where the tile sticks out of the coset it leaves -, its pixel p, its word `centre` in a halo
//    plane (tap (i, j) is word centre + j kHX + i, always inside the halo), and whether tap column i = t - 2 (okx[t]) / row j = t - 2 (oky[t]) lies inside the frame
#define ATROUS_PIXEL(F, thread, LEAVE) \
    const int lx = (thread) % psdr::atrous::kTX, ly = (thread) / psdr::atrous::kTX; \
    const int dx = tx0 + lx, dy = ty0 + ly; \
    if (dx >= wd || dy >= hd) LEAVE; \
    const int p = (b + dy * s) * (F).W + a + dx * s; \
    const int centre = (ly + 2) * psdr::atrous::kHX + lx + 2; \
    bool okx[5], oky[5]; \
    ATROUS_UNROLL \
    for (int t = 0; t < 5; ++t) { okx[t] = (unsigned) (dx + t - 2) < (unsigned) wd; oky[t] = (unsigned) (dy + t - 2) < (unsigned) hd; }

// what psdr_hip_*_create refuses before it touches the device: the message, or nothing
inline std::string check_create(const char *name, const void *guides, int32_t G, int32_t W, int32_t H, int32_t L, const void *out) {
    const std::string me = std::string(name) + ": ";
    if (!out) return me + "out is NULL";
    if (G < 0 || G > kMaxG) return me + "G = " + std::to_string(G) + ", must lie in [0, 8]";
    if (G > 0 && !guides) return me + "guides is NULL";
    if (W < 1 || H < 1) return me + "W = " + std::to_string(W) + ", H = " + std::to_string(H) + ", must be positive";
    if ((int64_t) W * H > kMaxPixels) return me + "W H = " + std::to_string((int64_t) W * H) + " is above 2^24";
    if (L < 1 || L > kMaxL) return me + "L = " + std::to_string(L) + ", must lie in [1, 8]";
    return std::string();
}

// the levels in the order of an operator (0 .. L - 1) or of its transpose (L - 1 .. 0), ping-pong through the two work frames; the last launch writes `out`
template <class Launch> void ping_pong(int L, bool forward, const float *in, float *out, float *const work[2], Launch &&launch) {
    const float *src = in;
    for (int k = 0; k < L; ++k) {
        float *dst = k == L - 1 ? out : work[k & 1];
        launch(forward ? k : L - 1 - k, src, dst);
        src = dst;
    }
}

} // namespace atrous
} // namespace psdr

#if defined(__HIPCC__)
#include <type_traits>

#include "op_common.h"

#define ATROUS_CHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return psdr::api_fail(std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

namespace psdr {
namespace atrous {
namespace {

__device__ inline float tap_weight(int i, int j) {          // h(i) h(j), exact: k / 256
    const int hi = i == 0 ? 6 : ((i == 1 || i == -1) ? 4 : 1), hj = j == 0 ? 6 : ((j == 1 || j == -1) ? 4 : 1);
    return (float) (hi * hj) * (1.f / 256.f);
}

// d2 of a tap: the centre pixel's guides gc against halo word `slot`, channel by channel in this order
template <int G> __device__ __forceinline__ float guide_d2(const float *gc, const float *lds, int slot) {
    float d2 = 0.f;
#pragma unroll
    for (int k = 0; k < G; ++k) {
        const float d = gc[k] - lds[k * kHalo + slot];
        d2 += d * d;
    }
    return d2;
}

// guides [n, G] -> planes [G][n]
__global__ void __launch_bounds__(kThreads) k_planes(const float *guides, int n, int G, float *planes) {
    const long long t = (long long) blockIdx.x * kThreads + threadIdx.x;
    if (t >= (long long) n * G) return;
    const int k = (int) (t / n), p = (int) (t % n);
    planes[t] = guides[(size_t) p * G + k];
}

// the runtime G in 0..8 as a compile-time constant: f(std::integral_constant<int, G>)
template <class F> void dispatch_g(int G, F &&f) {
    switch (G) {
        case 0: f(std::integral_constant<int, 0>()); break;
        case 1: f(std::integral_constant<int, 1>()); break;
        case 2: f(std::integral_constant<int, 2>()); break;
        case 3: f(std::integral_constant<int, 3>()); break;
        case 4: f(std::integral_constant<int, 4>()); break;
        case 5: f(std::integral_constant<int, 5>()); break;
        case 6: f(std::integral_constant<int, 6>()); break;
        case 7: f(std::integral_constant<int, 7>()); break;
        default: f(std::integral_constant<int, 8>()); break;
    }
}

// the common head of the two handles: the frame and one device block that begins with the guide planes [G][n]
struct Handle {
    int W = 0, H = 0, G = 0, L = 0;
    float *d_mem = nullptr, *planes = nullptr;
    ~Handle() { if (d_mem) (void) hipFree(d_mem); }
    size_t pixels() const { return (size_t) W * H; }
    // allocates the block, G + `rest` floats per pixel, and launches the copy of the guides into its planes; what follows the planes begins at planes + G n
    hipError_t init(const float *guides, int G_, int W_, int H_, int L_, size_t rest, hipStream_t st) {
        W = W_; H = H_; G = G_; L = L_;
        const size_t n = pixels();
        const hipError_t e = hipMalloc((void **) &d_mem, ((size_t) G + rest) * n * sizeof(float));
        if (e != hipSuccess) return e;
        planes = d_mem;
        if (G > 0) k_planes<<<(unsigned) ((n * G + kThreads - 1) / kThreads), kThreads, 0, st>>>(guides, (int) n, G, planes);
        return hipSuccess;
    }
};

} // namespace
} // namespace atrous
} // namespace psdr
#endif
