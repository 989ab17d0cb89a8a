// latreg.hip — the three regularisers of a signed distance on a regular lattice (Eikonal, Laplacian, sign-change cross-entropy) and their gradient with respect to the
// lattice's values in one fused stencil (Python surface: psdr_jit_amd/latreg.py).
//
// The definition (include/psdr_hip.h, THE LATTICE REGULARISERS, states it in full).  The lattice is marching tetrahedra's: u = x + nx (y + ny z), inside(u) = sdf[u] < 0.
//   eikonal   = (1 / Nc) sum_cells (n - 1)^2, n the length of the cell's mean forward differences; a cell with n = 0 adds 1 and no gradient
//   laplacian = (1 / Nv) sum_u r_u^2, r_u the sum over the axes along which u has both neighbours of ((s_- - s_u) + (s_+ - s_u)) / h_a^2
//   sign      = (1 / V) sum_u m_u softplus(k |s_u|), m_u the crossing edges among u's fourteen, V = (1 / 2) sum_u m_u held constant in the gradient
//   loss      = w_eik eikonal + w_lap laplacian + w_sign sign;  a term of weight 0 is not evaluated
//
// The schedule: a haloed LDS tile.  The gradient at a vertex reads a radius-2 cross and a 3^3 cube of sdf, so neighbouring lanes share almost all they read; a workgroup of
// 256 lanes owns a tile of 32 x 8 x 4 vertices (x fastest: a row of the tile is one coalesced 128-byte run of sdf, and 32 consecutive floats of LDS fall into 32 banks), loads
// it once with its halo - every halo load guarded by the extents - and forms the two intermediates IN LDS as well: r on the tile grown by one (34 x 10 x 6) and the three
// per-cell Eikonal factors on the cells that touch the tile (33 x 9 x 5), each computed once per workgroup rather than 7 and 8 times per vertex.  39.8 KB of LDS per workgroup:
// four workgroups fit a compute unit's 160 KB.  A window that slides along z with the column in registers would read less halo (1.7 x against 3.4 x the tile, the surplus
// served by the caches) but needs the two intermediates as rings of planes with a barrier per plane; store-then-gather through global memory writes and re-reads 4 Nv floats
// of intermediates, more than the whole byte floor of 8 Nv.  The tile was chosen for having neither.
//
// The passes.  Three launches, two without a gradient:
//   k_value   a workgroup per tile (halo 1): a lane adds, over its 4 vertices in ascending z, the cell anchored at the vertex, r_u^2 and m_u softplus(k |s_u|), and m_u; the
//             workgroup adds its lanes in a fixed order (a wave by shuffles, the four waves in order) into its own four partial sums (scratch).
//   k_finish  one workgroup: the partial sums in a fixed order in float64, the divisions by the counts, out = (loss, eikonal, laplacian, sign), crossings = V.
//   k_grad    a workgroup per tile (halo 2): r and the Eikonal factors into LDS, then a lane per vertex gathers its 8 cells, its 6 neighbours' r and its 14 edge neighbours
//             and writes grad[u] once; it reads V from `crossings` on the device.
// Every address is computed from lattice coordinates, never from data.  No host synchronisation, no atomics: the same input gives the same bits.  No contraction in this unit
// (the build's -ffp-contract=off).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../../include/psdr_hip.h"
#include "op_common.h"

namespace {

constexpr int kTX = 32, kTY = 8, kTZ = 4;       // the tile: must be the plan's
constexpr int kThreads = kTX * kTY;             // 4 waves, a lane per (x, y) of the tile, kTZ vertices each
constexpr int kSumThreads = 1024;               // k_finish: one workgroup, 16 waves
constexpr int kMaxLattice = 1 << 24;

struct Lattice {
    int nx, ny, nz, nv, nc;             // extents, vertices, cells
    int bx, by, bz, blocks;             // tiles along the axes, and their product
};

struct Call {
    int eik, lap, sgn;                  // which terms are evaluated
    float i4x, i4y, i4z;                // 1 / (4 h_a)
    float i2x, i2y, i2z;                // 1 / h_a^2
    float k;                            // sign_scale
    float w_eik, w_lap, w_sgn;
    float s_eik, s_lap, s_sgn;          // the gradient's scales: w_eik / Nc, 2 w_lap / Nv, w_sign k (divided by V on the device)
};

// the LDS image of a tile grown by H: local coordinates (lx, ly, lz) run from -H
template <int H> struct Tile {
    static constexpr int WX = kTX + 2 * H, WY = kTY + 2 * H, WZ = kTZ + 2 * H, SIZE = WX * WY * WZ;
    static __device__ __forceinline__ int at(int lx, int ly, int lz) { return (lx + H) + WX * ((ly + H) + WY * (lz + H)); }
};

__device__ __forceinline__ bool inside_of(float s) { return s < 0.f; }          // a zero is outside

__device__ __forceinline__ void tile_origin(const Lattice &L, int &x0, int &y0, int &z0) {
    const int b = blockIdx.x;
    x0 = (b % L.bx) * kTX;
    y0 = ((b / L.bx) % L.by) * kTY;
    z0 = (b / (L.bx * L.by)) * kTZ;
}

// rows along x are consecutive lanes; a position outside the lattice holds 0 and is never used
template <int H> __device__ __forceinline__ void load_tile(const float *__restrict__ sdf, const Lattice &L, int x0, int y0, int z0, float *__restrict__ sS) {
    using T = Tile<H>;
    for (int i = threadIdx.x; i < T::SIZE; i += kThreads) {
        const int x = x0 + i % T::WX - H, y = y0 + (i / T::WX) % T::WY - H, z = z0 + i / (T::WX * T::WY) - H;
        float v = 0.f;
        if (x >= 0 && x < L.nx && y >= 0 && y < L.ny && z >= 0 && z < L.nz) v = sdf[x + L.nx * (y + L.ny * z)];
        sS[i] = v;
    }
}

// r at the lattice vertex (x, y, z) = tile-local (lx, ly, lz): the axes along which it has both neighbours, in the order x, y, z
template <int H> __device__ __forceinline__ float r_of(const float *__restrict__ sS, const Lattice &L, const Call &c, int x, int y, int z, int lx, int ly, int lz) {
    using T = Tile<H>;
    const float s0 = sS[T::at(lx, ly, lz)];
    float r = 0.f;
    if (x >= 1 && x <= L.nx - 2) r += ((sS[T::at(lx - 1, ly, lz)] - s0) + (sS[T::at(lx + 1, ly, lz)] - s0)) * c.i2x;
    if (y >= 1 && y <= L.ny - 2) r += ((sS[T::at(lx, ly - 1, lz)] - s0) + (sS[T::at(lx, ly + 1, lz)] - s0)) * c.i2y;
    if (z >= 1 && z <= L.nz - 2) r += ((sS[T::at(lx, ly, lz - 1)] - s0) + (sS[T::at(lx, ly, lz + 1)] - s0)) * c.i2z;
    return r;
}

// the cell anchored at tile-local (lx, ly, lz): its summand (n - 1)^2 and q_a = 2 (n - 1) (g_a / n) / (4 h_a); n = 0: 1 and q = 0
template <int H> __device__ __forceinline__ float cell_of(const float *__restrict__ sS, const Call &c, int lx, int ly, int lz, float &qx, float &qy, float &qz) {
    using T = Tile<H>;
    const float s000 = sS[T::at(lx, ly, lz)], s100 = sS[T::at(lx + 1, ly, lz)], s010 = sS[T::at(lx, ly + 1, lz)], s110 = sS[T::at(lx + 1, ly + 1, lz)];
    const float s001 = sS[T::at(lx, ly, lz + 1)], s101 = sS[T::at(lx + 1, ly, lz + 1)], s011 = sS[T::at(lx, ly + 1, lz + 1)], s111 = sS[T::at(lx + 1, ly + 1, lz + 1)];
    const float gx = ((((s100 - s000) + (s110 - s010)) + (s101 - s001)) + (s111 - s011)) * c.i4x;
    const float gy = ((((s010 - s000) + (s110 - s100)) + (s011 - s001)) + (s111 - s101)) * c.i4y;
    const float gz = ((((s001 - s000) + (s101 - s100)) + (s011 - s010)) + (s111 - s110)) * c.i4z;
    const float n = sqrtf((gx * gx + gy * gy) + gz * gz);
    if (n == 0.f) {
        qx = qy = qz = 0.f;
        return 1.f;
    }
    const float d = n - 1.f, t = 2.f * d;
    qx = (t * (gx / n)) * c.i4x;
    qy = (t * (gy / n)) * c.i4y;
    qz = (t * (gz / n)) * c.i4z;
    return d * d;
}

// m_u: the edges of the seven classes to either side of (x, y, z) whose far end lies in the lattice and on the other side of zero
template <int H> __device__ __forceinline__ int crossings_of(const float *__restrict__ sS, const Lattice &L, int x, int y, int z, int lx, int ly, int lz, bool in0) {
    using T = Tile<H>;
    int m = 0;
#pragma unroll
    for (int b = 1; b < 8; ++b) {
        const int dx = b & 1, dy = b >> 1 & 1, dz = b >> 2 & 1;
        if (x + dx < L.nx && y + dy < L.ny && z + dz < L.nz && inside_of(sS[T::at(lx + dx, ly + dy, lz + dz)]) != in0) ++m;
        if (x - dx >= 0 && y - dy >= 0 && z - dz >= 0 && inside_of(sS[T::at(lx - dx, ly - dy, lz - dz)]) != in0) ++m;
    }
    return m;
}

// partial: [4][blocks] - the workgroups' sums of the Eikonal, Laplacian and sign summands, and (as int32) of m_u
__global__ void __launch_bounds__(kThreads) k_value(const float *__restrict__ sdf, Lattice L, Call c, float *__restrict__ partial) {
    using T = Tile<1>;
    __shared__ float sS[T::SIZE];
    __shared__ float s_red[kThreads / 64];
    __shared__ int s_redi[kThreads / 64];
    int x0, y0, z0;
    tile_origin(L, x0, y0, z0);
    load_tile<1>(sdf, L, x0, y0, z0, sS);
    __syncthreads();
    const int lx = threadIdx.x % kTX, ly = threadIdx.x / kTX;
    const int x = x0 + lx, y = y0 + ly;
    float e = 0.f, l = 0.f, g = 0.f;
    int count = 0;
    if (x < L.nx && y < L.ny) {
#pragma unroll
        for (int lz = 0; lz < kTZ; ++lz) {
            const int z = z0 + lz;
            if (z >= L.nz) break;
            if (c.eik && x < L.nx - 1 && y < L.ny - 1 && z < L.nz - 1) {
                float qx, qy, qz;
                e += cell_of<1>(sS, c, lx, ly, lz, qx, qy, qz);
            }
            if (c.lap) {
                const float r = r_of<1>(sS, L, c, x, y, z, lx, ly, lz);
                l += r * r;
            }
            if (c.sgn) {
                const float s = sS[T::at(lx, ly, lz)];
                const int m = crossings_of<1>(sS, L, x, y, z, lx, ly, lz, inside_of(s));
                if (m > 0) {
                    const float t = c.k * fabsf(s);
                    g += (float) m * (t + log1pf(expf(-t)));
                    count += m;
                }
            }
        }
    }
    const float te = block_sum<kThreads>(e, s_red), tl = block_sum<kThreads>(l, s_red), tg = block_sum<kThreads>(g, s_red);
    const int tc = block_sum<kThreads>(count, s_redi);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = te;
        partial[L.blocks + blockIdx.x] = tl;
        partial[2 * L.blocks + blockIdx.x] = tg;
        reinterpret_cast<int *>(partial)[3 * L.blocks + blockIdx.x] = tc;
    }
}

// a lane adds every 1024th partial sum of a run in ascending order, then the workgroup's fixed order
__device__ double run_sum(const float *p, int count, double *s_red) {
    double a = 0.0;
    for (int t = threadIdx.x; t < count; t += kSumThreads) a += (double) p[t];
    return block_sum<kSumThreads>(a, s_red);
}

__global__ void __launch_bounds__(kSumThreads) k_finish(Lattice L, Call c, const float *__restrict__ partial, float *__restrict__ out, int *__restrict__ crossings) {
    __shared__ double s_red[kSumThreads / 64];
    __shared__ long long s_redi[kSumThreads / 64];
    const double se = run_sum(partial, c.eik ? L.blocks : 0, s_red);
    const double sl = run_sum(partial + L.blocks, c.lap ? L.blocks : 0, s_red);
    const double sg = run_sum(partial + 2 * L.blocks, c.sgn ? L.blocks : 0, s_red);
    long long m = 0;
    if (c.sgn)
        for (int t = threadIdx.x; t < L.blocks; t += kSumThreads) m += reinterpret_cast<const int *>(partial)[3 * L.blocks + t];
    m = block_sum<kSumThreads>(m, s_redi);
    if (threadIdx.x == 0) {
        const int V = (int) (m / 2);    // every crossing edge was counted at both ends; V <= 7 Nv fits
        const float eik = c.eik ? (float) (se / (double) L.nc) : 0.f;
        const float lap = c.lap ? (float) (sl / (double) L.nv) : 0.f;
        const float sgn = c.sgn && V > 0 ? (float) (sg / (double) V) : 0.f;
        float loss = 0.f;
        bool have = false;
        if (c.eik) { loss = c.w_eik * eik; have = true; }
        if (c.lap) { const float t = c.w_lap * lap; loss = have ? loss + t : t; have = true; }
        if (c.sgn) { const float t = c.w_sgn * sgn; loss = have ? loss + t : t; }
        out[0] = loss;
        out[1] = eik;
        out[2] = lap;
        out[3] = sgn;
        crossings[0] = V;
    }
}

__global__ void __launch_bounds__(kThreads) k_grad(const float *__restrict__ sdf, Lattice L, Call c, const int *__restrict__ crossings, float *__restrict__ grad) {
    using T = Tile<2>;
    constexpr int RX = kTX + 2, RY = kTY + 2, RZ = kTZ + 2;             // r on the tile grown by one: local coordinates from -1
    constexpr int QX = kTX + 1, QY = kTY + 1, QZ = kTZ + 1;             // the cells that touch the tile: anchors from -1
    __shared__ float sS[T::SIZE];
    __shared__ float sR[RX * RY * RZ];
    __shared__ float sQ[3][QX * QY * QZ];
    int x0, y0, z0;
    tile_origin(L, x0, y0, z0);
    load_tile<2>(sdf, L, x0, y0, z0, sS);
    __syncthreads();
    if (c.lap) {
        for (int i = threadIdx.x; i < RX * RY * RZ; i += kThreads) {
            const int lx = i % RX - 1, ly = (i / RX) % RY - 1, lz = i / (RX * RY) - 1;
            const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
            const bool in = x >= 0 && x < L.nx && y >= 0 && y < L.ny && z >= 0 && z < L.nz;
            sR[i] = in ? r_of<2>(sS, L, c, x, y, z, lx, ly, lz) : 0.f;
        }
    }
    if (c.eik) {
        for (int i = threadIdx.x; i < QX * QY * QZ; i += kThreads) {
            const int lx = i % QX - 1, ly = (i / QX) % QY - 1, lz = i / (QX * QY) - 1;
            const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
            float qx = 0.f, qy = 0.f, qz = 0.f;
            if (x >= 0 && x < L.nx - 1 && y >= 0 && y < L.ny - 1 && z >= 0 && z < L.nz - 1) cell_of<2>(sS, c, lx, ly, lz, qx, qy, qz);
            sQ[0][i] = qx;
            sQ[1][i] = qy;
            sQ[2][i] = qz;
        }
    }
    __syncthreads();
    const int lx = threadIdx.x % kTX, ly = threadIdx.x / kTX;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= L.nx || y >= L.ny) return;
    float sign_scale = 0.f;
    if (c.sgn) {
        const int V = crossings[0];
        sign_scale = V > 0 ? c.s_sgn / (float) V : 0.f;
    }
#pragma unroll
    for (int lz = 0; lz < kTZ; ++lz) {
        const int z = z0 + lz;
        if (z >= L.nz) break;
        float g = 0.f;
        bool have = false;
        if (c.eik) {
            // the 8 cells around the vertex, anchors from (-1, -1, -1) with x fastest; the vertex is the high end of an axis where the anchor lies one below
            float ax = 0.f, ay = 0.f, az = 0.f;
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const int ox = (b & 1) - 1, oy = (b >> 1 & 1) - 1, oz = (b >> 2 & 1) - 1;
                const int q = (lx + ox + 1) + QX * ((ly + oy + 1) + QY * (lz + oz + 1));
                ax = ox ? ax + sQ[0][q] : ax - sQ[0][q];
                ay = oy ? ay + sQ[1][q] : ay - sQ[1][q];
                az = oz ? az + sQ[2][q] : az - sQ[2][q];
            }
            g = c.s_eik * ((ax + ay) + az);
            have = true;
        }
        if (c.lap) {
            // its own r through every axis it is interior along, and the r of each neighbour that is interior along the axis that joins them
            const int i = (lx + 1) + RX * ((ly + 1) + RY * (lz + 1));
            const float r0 = sR[i];
            float tx = 0.f, ty = 0.f, tz = 0.f;
            if (x >= 1 && x <= L.nx - 2) tx = -2.f * r0;
            if (x - 1 >= 1) tx += sR[i - 1];
            if (x + 1 <= L.nx - 2) tx += sR[i + 1];
            if (y >= 1 && y <= L.ny - 2) ty = -2.f * r0;
            if (y - 1 >= 1) ty += sR[i - RX];
            if (y + 1 <= L.ny - 2) ty += sR[i + RX];
            if (z >= 1 && z <= L.nz - 2) tz = -2.f * r0;
            if (z - 1 >= 1) tz += sR[i - RX * RY];
            if (z + 1 <= L.nz - 2) tz += sR[i + RX * RY];
            const float t = c.s_lap * ((tx * c.i2x + ty * c.i2y) + tz * c.i2z);
            g = have ? g + t : t;
            have = true;
        }
        if (c.sgn) {
            const float s = sS[T::at(lx, ly, lz)];
            const bool in0 = inside_of(s);
            const int m = crossings_of<2>(sS, L, x, y, z, lx, ly, lz, in0);
            float t = 0.f;
            if (m > 0) {
                const float sig = 1.f / (1.f + expf(-(c.k * fabsf(s))));
                t = ((float) m * sig) * sign_scale;
                if (in0) t = -t;
            }
            g = have ? g + t : t;
        }
        grad[x + L.nx * (y + L.ny * z)] = g;
    }
}

inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// refuses a bad lattice; fills L
inline bool lattice(const std::string &who, int32_t nx, int32_t ny, int32_t nz, Lattice *L) {
    if (nx < 2 || ny < 2 || nz < 2) {
        psdr::api_fail(who + "shape = (" + std::to_string(nx) + ", " + std::to_string(ny) + ", " + std::to_string(nz) + "), every extent must be at least 2");
        return false;
    }
    const bool fits = nx <= kMaxLattice && ny <= kMaxLattice && nz <= kMaxLattice && (long long) nx * ny <= kMaxLattice;          // (then the product of all three fits 64 bits)
    const long long nv = fits ? (long long) nx * ny * nz : 0;
    if (!fits || nv > kMaxLattice) {
        psdr::api_fail(who + "shape = (" + std::to_string(nx) + ", " + std::to_string(ny) + ", " + std::to_string(nz) + "), more than 2^24 lattice vertices");
        return false;
    }
    L->nx = nx; L->ny = ny; L->nz = nz;
    L->nv = (int) nv;
    L->nc = (nx - 1) * (ny - 1) * (nz - 1);
    L->bx = ceil_div(nx, kTX); L->by = ceil_div(ny, kTY); L->bz = ceil_div(nz, kTZ);
    L->blocks = L->bx * L->by * L->bz;          // at most 2^24 / 4 (extents 2, 2, 2^22): far below an int32 and a grid's limit
    return true;
}

} // namespace

extern "C" {

int psdr_hip_latreg_plan(int32_t nx, int32_t ny, int32_t nz, int32_t *tile_x, int32_t *tile_y, int32_t *tile_z, int32_t *workgroups, int32_t *scratch_floats) {
    const std::string who = "psdr_hip_latreg_plan: ";
    Lattice L;
    if (!lattice(who, nx, ny, nz, &L)) return 1;
    if (!tile_x || !tile_y || !tile_z || !workgroups || !scratch_floats) return psdr::api_fail(who + "NULL argument");
    *tile_x = kTX;
    *tile_y = kTY;
    *tile_z = kTZ;
    *workgroups = L.blocks;
    *scratch_floats = 4 * L.blocks;
    return 0;
}

int psdr_hip_latreg_eval(const float *sdf, int32_t nx, int32_t ny, int32_t nz, const double *spacing, const float *weights, float sign_scale, float *scratch, float *out,
                         int32_t *crossings, float *grad, void *stream) {
    const std::string who = "psdr_hip_latreg_eval: ";
    Lattice L;
    if (!lattice(who, nx, ny, nz, &L)) return 1;
    if (!sdf || !spacing || !weights || !scratch || !out || !crossings) return psdr::api_fail(who + "NULL argument");
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(spacing[a]) || !(spacing[a] > 0.0)) return psdr::api_fail(who + "spacing[" + std::to_string(a) + "] = " + std::to_string(spacing[a]) + ", must be finite and positive");
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(weights[k]) || weights[k] < 0.f) return psdr::api_fail(who + "weights[" + std::to_string(k) + "] = " + std::to_string(weights[k]) + ", must be finite and not negative");
    if (!std::isfinite(sign_scale) || sign_scale < 0.f) return psdr::api_fail(who + "sign_scale = " + std::to_string(sign_scale) + ", must be finite and not negative");
    const void *arrays[5] = {sdf, scratch, out, crossings, grad};
    for (int i = 0; i < 5; ++i)
        for (int j = i + 1; j < 5; ++j)
            if (arrays[i] && arrays[i] == arrays[j]) return psdr::api_fail(who + "scratch, out, crossings and grad must be arrays of their own, none of them sdf");
    Call c{};
    c.eik = weights[0] > 0.f; c.lap = weights[1] > 0.f; c.sgn = weights[2] > 0.f;
    c.i4x = (float) (1.0 / (4.0 * spacing[0])); c.i4y = (float) (1.0 / (4.0 * spacing[1])); c.i4z = (float) (1.0 / (4.0 * spacing[2]));
    c.i2x = (float) (1.0 / (spacing[0] * spacing[0])); c.i2y = (float) (1.0 / (spacing[1] * spacing[1])); c.i2z = (float) (1.0 / (spacing[2] * spacing[2]));
    const float *r = &c.i4x;
    for (int a = 0; a < 6; ++a)
        if (!std::isfinite(r[a]) || !(r[a] > 0.f)) return psdr::api_fail(who + "spacing[" + std::to_string(a % 3) + "] = " + std::to_string(spacing[a % 3]) + ": 1 / (4 h) and 1 / h^2 must be positive float32 numbers");
    c.k = sign_scale;
    c.w_eik = weights[0]; c.w_lap = weights[1]; c.w_sgn = weights[2];
    c.s_eik = (float) ((double) weights[0] / (double) L.nc);
    c.s_lap = (float) (2.0 * (double) weights[1] / (double) L.nv);
    c.s_sgn = (float) ((double) weights[2] * (double) sign_scale);
    hipStream_t st = (hipStream_t) stream;
    k_value<<<L.blocks, kThreads, 0, st>>>(sdf, L, c, scratch);
    k_finish<<<1, kSumThreads, 0, st>>>(L, c, scratch, out, crossings);
    if (grad) k_grad<<<L.blocks, kThreads, 0, st>>>(sdf, L, c, crossings, grad);
    return launch_status(who);
}

} // extern "C"
