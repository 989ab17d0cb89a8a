// mtet.hip — isosurface extraction by marching tetrahedra: a signed distance on a lattice to a triangle mesh, the positions of the mesh's vertices and the vector-Jacobian
// product of those positions with respect to the lattice's values and positions (Python surface: psdr_jit_amd/mtet.py).
//
// The definition (include/psdr_hip.h, THE ISOSURFACE, states it in full).  Every cell is split into Kuhn's six tetrahedra, every edge of every tetrahedron is one of seven
// classes anchored at its low end (slot 7 u + c), the mesh's vertices are the crossing slots in ascending order, and a tetrahedron gives 0, 1 or 2 triangles by a table over
// (tet k, 4-bit inside mask).  The table is made at compile time (make_tables below) from the rules of the definition and integer geometry on the unit cell: the winding is a
// function of (k, mask) alone, never a test on the positions.
//
// The passes.  psdr_hip_mtet_count: k_vertex_mask (a lane per lattice vertex: the 7-bit crossing mask, neighbouring values re-read through the cache, and the workgroup's sum of
// popcounts), the scan of the workgroup sums, k_scatter (base[u] = the exclusive scan of the popcounts); then the same three steps per cell for the face counts (0 .. 12: the six
// tetrahedra of a cell are emitted by one lane, in ascending k, so one offset per cell is enough and faces still come in ascending tet id).  psdr_hip_mtet_emit: k_emit_edges and
// k_emit_faces; the index of slot 7 u + c is base[u] + popcount(mask[u] & ((1 << c) - 1)).  psdr_hip_mtet_vertices: a lane per mesh vertex.  psdr_hip_mtet_vertices_adj: a lane
// per lattice vertex gathers its own seven slots and the seven slots it is the far end of, in that fixed order: no sort, no inverted index, no float atomics.
// The scans are reduce / scan of the workgroup sums / scatter in plain launches, 256 entries per workgroup, so Nv <= 2^24 = 256^3 needs at most two passes over workgroup sums;
// no workgroup ever waits for another.  Waves are 64 wide (the wave scan walks 6 shuffle steps).  No contraction in this unit (the build's -ffp-contract=off, and the formulas
// are written with __fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>

#include "../../../include/psdr_hip.h"
#include "op_common.h"

namespace {

constexpr int kThreads = 256;           // 4 waves; also the entries a workgroup scans: must be the plan's tile
constexpr int kWave = 64;
constexpr int kMaxLattice = 1 << 24;    // Nv: every count (V <= 7 Nv, F <= 12 cells) and every 3 F offset fits an int32

// ---- the tables, made at compile time from the definition

constexpr int kPerm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};       // (a, b, c) of tet k: xyz, xzy, yxz, yzx, zxy, zyx
constexpr int kClassBits[7] = {1, 2, 4, 3, 5, 6, 7};                                                   // d_c as x | y << 1 | z << 2

constexpr int class_of(int bits) { return bits == 1 ? 0 : bits == 2 ? 1 : bits == 4 ? 2 : bits == 3 ? 3 : bits == 5 ? 4 : bits == 6 ? 5 : 6; }

struct Tables {
    unsigned char corner[6][4];         // corner i of tet k as an offset from the cell's low corner, x | y << 1 | z << 2
    unsigned int tri[6][16][2];         // the triangles of (k, inside mask), wound: three slots of 6 bits each, (anchor's corner offset) | class << 3
    int degenerate;                     // the number of triangles whose winding the geometry left open: 0 (static_assert below)
};

constexpr Tables make_tables() {
    Tables T = {};
    for (int k = 0; k < 6; ++k) {
        T.corner[k][0] = 0;
        T.corner[k][1] = (unsigned char) (1 << kPerm[k][0]);
        T.corner[k][2] = (unsigned char) (T.corner[k][1] | (1 << kPerm[k][1]));
        T.corner[k][3] = 7;
        for (int mask = 1; mask < 15; ++mask) {
            int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, n_in = 0, n_out = 0;
            for (int i = 0; i < 4; ++i) {
                if (mask >> i & 1) in[n_in++] = i;
                else out[n_out++] = i;
            }
            int pairs[2][3][2] = {};     // triangle, slot, (corner, corner)
            int n_tri = 1;
            if (n_in == 2) {
                // inside i < j, outside k < l: the quad e_ik, e_il, e_jl, e_jk split along e_ik - e_jl
                const int i = in[0], j = in[1], kk = out[0], l = out[1];
                const int q[4][2] = {{i, kk}, {i, l}, {j, l}, {j, kk}};
                const int pick[2][3] = {{0, 1, 2}, {0, 2, 3}};
                n_tri = 2;
                for (int t = 0; t < 2; ++t)
                    for (int s = 0; s < 3; ++s) { pairs[t][s][0] = q[pick[t][s]][0]; pairs[t][s][1] = q[pick[t][s]][1]; }
            } else {
                // one corner i alone on its side: the slots to the other three in tet-local order
                const int i = n_in == 1 ? in[0] : out[0];
                const int *others = n_in == 1 ? out : in;
                for (int s = 0; s < 3; ++s) { pairs[0][s][0] = i; pairs[0][s][1] = others[s]; }
            }
            // from the inside corners to the outside corners, scaled by n_in n_out
            int D[3] = {0, 0, 0};
            for (int a = 0; a < 3; ++a) {
                for (int i = 0; i < n_out; ++i) D[a] += n_in * (T.corner[k][out[i]] >> a & 1);
                for (int i = 0; i < n_in; ++i) D[a] -= n_out * (T.corner[k][in[i]] >> a & 1);
            }
            for (int t = 0; t < n_tri; ++t) {
                int P[3][3] = {};        // twice the slots' midpoints on the unit cell
                for (int s = 0; s < 3; ++s)
                    for (int a = 0; a < 3; ++a) P[s][a] = (T.corner[k][pairs[t][s][0]] >> a & 1) + (T.corner[k][pairs[t][s][1]] >> a & 1);
                const int e1[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]}, e2[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
                const int N[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
                const int side = N[0] * D[0] + N[1] * D[1] + N[2] * D[2];
                if (side == 0) ++T.degenerate;
                const int order[3] = {0, side > 0 ? 1 : 2, side > 0 ? 2 : 1};       // counter-clockwise seen from the outside corners
                unsigned int code = 0;
                for (int s = 0; s < 3; ++s) {
                    int lo = pairs[t][order[s]][0], hi = pairs[t][order[s]][1];
                    if (lo > hi) { const int x = lo; lo = hi; hi = x; }
                    const int anchor = T.corner[k][lo], cls = class_of(T.corner[k][hi] ^ anchor);           // (corner offsets grow with the local index: the difference is the xor)
                    code |= (unsigned int) (anchor | cls << 3) << (6 * s);
                }
                T.tri[k][mask][t] = code;
            }
        }
    }
    return T;
}

constexpr Tables kHostTables = make_tables();
static_assert(kHostTables.degenerate == 0, "a triangle of the marching-tetrahedra table has no winding");
__constant__ Tables d_tables = make_tables();

// ---- the lattice

struct Lattice {
    int nx, ny, nz, nv, nc;             // extents, vertices, cells
};

__device__ __forceinline__ bool inside_of(float s) { return s < 0.f; }          // a zero is outside and so is a NaN

__device__ __forceinline__ int offset_of(const Lattice &L, int bits) { return (bits & 1) + L.nx * ((bits >> 1 & 1) + L.ny * (bits >> 2 & 1)); }

__device__ __forceinline__ int faces_of(int m4) { return min(__popc(m4), 4 - __popc(m4)); }          // 0 or 4 inside: 0; 1 or 3: 1; 2: 2

// ---- scans: exclusive, 256 entries per workgroup; every lane of the workgroup calls

__device__ __forceinline__ int block_exclusive(int v, int *block_total) {
    __shared__ int s_wave[kThreads / kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int incl = v;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int t = __shfl_up(incl, d, kWave);
        if (lane >= d) incl += t;
    }
    if (lane == kWave - 1) s_wave[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kThreads / kWave; ++w) {
        const int s = s_wave[w];
        if (w < wave) before += s;
        total += s;
    }
    *block_total = total;
    return before + incl - v;
}

// mask[u]: bit c set where slot 7 u + c exists and its two ends differ; sums[workgroup] = the workgroup's crossing slots
__global__ void __launch_bounds__(kThreads) k_vertex_mask(const float *__restrict__ sdf, Lattice L, unsigned char *__restrict__ mask, int *__restrict__ sums) {
    const int u = blockIdx.x * kThreads + threadIdx.x;
    int m = 0;
    if (u < L.nv) {
        const int x = u % L.nx, y = (u / L.nx) % L.ny, z = u / (L.nx * L.ny);
        const bool in0 = inside_of(sdf[u]);
#pragma unroll
        for (int c = 0; c < 7; ++c) {
            const int b = kClassBits[c];
            const bool exists = x + (b & 1) < L.nx && y + (b >> 1 & 1) < L.ny && z + (b >> 2 & 1) < L.nz;
            if (exists && inside_of(sdf[u + offset_of(L, b)]) != in0) m |= 1 << c;
        }
        mask[u] = (unsigned char) m;
    }
    int total;
    block_exclusive(__popc(m), &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// the 8 inside bits of a cell's corners, bit x | y << 1 | z << 2
__device__ __forceinline__ int cell_corners(const float *__restrict__ sdf, const Lattice &L, int cell, int *low) {
    const int cx = cell % (L.nx - 1), cy = (cell / (L.nx - 1)) % (L.ny - 1), cz = cell / ((L.nx - 1) * (L.ny - 1));
    const int v = cx + L.nx * (cy + L.ny * cz);
    int in8 = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) in8 |= (int) inside_of(sdf[v + offset_of(L, b)]) << b;
    *low = v;
    return in8;
}

__device__ __forceinline__ int tet_mask(int in8, int k) {
    return (in8 >> d_tables.corner[k][0] & 1) | (in8 >> d_tables.corner[k][1] & 1) << 1 | (in8 >> d_tables.corner[k][2] & 1) << 2 | (in8 >> d_tables.corner[k][3] & 1) << 3;
}

// fcount[cell] = the faces of the cell's six tetrahedra (0 .. 12); sums[workgroup] = the workgroup's faces
__global__ void __launch_bounds__(kThreads) k_cell_count(const float *__restrict__ sdf, Lattice L, unsigned char *__restrict__ fcount, int *__restrict__ sums) {
    const int cell = blockIdx.x * kThreads + threadIdx.x;
    int n = 0;
    if (cell < L.nc) {
        int low;
        const int in8 = cell_corners(sdf, L, cell, &low);
        if (in8 != 0 && in8 != 255) {
#pragma unroll
            for (int k = 0; k < 6; ++k) n += faces_of(tet_mask(in8, k));
        }
        fcount[cell] = (unsigned char) n;
    }
    int total;
    block_exclusive(n, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kThreads) k_block_sums(const int *__restrict__ in, int n, int *__restrict__ sums) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    int total;
    block_exclusive(i < n ? in[i] : 0, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// out[i] = (offsets ? offsets[workgroup] : 0) + the sum of the workgroup's entries before i; total (one workgroup only): the sum of all entries
__global__ void __launch_bounds__(kThreads) k_scan_block(const int *__restrict__ in, int n, const int *__restrict__ offsets, int *__restrict__ out, int *__restrict__ total_out) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    int total;
    const int before = block_exclusive(i < n ? in[i] : 0, &total);
    if (i < n) out[i] = (offsets ? offsets[blockIdx.x] : 0) + before;
    if (total_out && threadIdx.x == 0) *total_out = total;
}

// out[i] = offsets[workgroup] + the workgroup's counts before i; the count of an entry is its popcount (the vertex masks) or its value (the cells' face counts)
template <bool POPCOUNT> __global__ void __launch_bounds__(kThreads) k_scatter(const unsigned char *__restrict__ counts, int n, const int *__restrict__ offsets, int *__restrict__ out) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    const int raw = i < n ? counts[i] : 0;
    int total;
    const int before = block_exclusive(POPCOUNT ? __popc(raw) : raw, &total);
    if (i < n) out[i] = offsets[blockIdx.x] + before;
}

// ---- emit

__device__ __forceinline__ int slot_index(const unsigned char *__restrict__ mask, const int *__restrict__ base, int u, int c) { return base[u] + __popc(mask[u] & ((1 << c) - 1)); }

__global__ void __launch_bounds__(kThreads) k_emit_edges(Lattice L, const unsigned char *__restrict__ mask, const int *__restrict__ base, int nv_mesh, int *__restrict__ edges) {
    const int u = blockIdx.x * kThreads + threadIdx.x;
    if (u >= L.nv) return;
    const int m = mask[u];
    int i = base[u];
#pragma unroll
    for (int c = 0; c < 7; ++c) {
        if (!(m >> c & 1)) continue;
        if (i >= 0 && i < nv_mesh) {                            // (a mask that another sdf made cannot write out of the rows given)
            edges[2 * i] = u;
            edges[2 * i + 1] = u + offset_of(L, kClassBits[c]);
        }
        ++i;
    }
}

__global__ void __launch_bounds__(kThreads) k_emit_faces(const float *__restrict__ sdf, Lattice L, const unsigned char *__restrict__ mask, const int *__restrict__ base,
                                                         const int *__restrict__ cbase, int nf_mesh, int *__restrict__ faces) {
    const int cell = blockIdx.x * kThreads + threadIdx.x;
    if (cell >= L.nc) return;
    int low;
    const int in8 = cell_corners(sdf, L, cell, &low);
    if (in8 == 0 || in8 == 255) return;
    int f = cbase[cell];
    for (int k = 0; k < 6; ++k) {
        const int m4 = tet_mask(in8, k);
        const int n = faces_of(m4);
        for (int t = 0; t < n; ++t, ++f) {
            if (f < 0 || f >= nf_mesh) continue;
            const unsigned int code = d_tables.tri[k][m4][t];
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const int slot = code >> (6 * s) & 63;
                faces[3 * f + s] = slot_index(mask, base, low + offset_of(L, slot & 7), slot >> 3);
            }
        }
    }
}

// ---- positions and their transpose

struct Vec { float x, y, z; };

__device__ __forceinline__ Vec load3(const float *__restrict__ a, int i) { return {a[3LL * i], a[3LL * i + 1], a[3LL * i + 2]}; }
__device__ __forceinline__ Vec sub(Vec p, Vec q) { return {__fsub_rn(p.x, q.x), __fsub_rn(p.y, q.y), __fsub_rn(p.z, q.z)}; }
__device__ __forceinline__ float dot(Vec p, Vec q) { return __fadd_rn(__fadd_rn(__fmul_rn(p.x, q.x), __fmul_rn(p.y, q.y)), __fmul_rn(p.z, q.z)); }
__device__ __forceinline__ int clamped(int i, int count) { return min(max(i, 0), count - 1); }

// p = p_a + t (p_b - p_a), t = s_a / (s_a - s_b), from the anchor
__global__ void __launch_bounds__(kThreads) k_vertices(const float *__restrict__ sdf, const float *__restrict__ pos, int nv_lattice, const int *__restrict__ edges, int nv_mesh,
                                                       float *__restrict__ out) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= nv_mesh) return;
    const int a = clamped(edges[2 * i], nv_lattice), b = clamped(edges[2 * i + 1], nv_lattice);
    const float sa = sdf[a], sb = sdf[b];
    const float t = __fdiv_rn(sa, __fsub_rn(sa, sb));
    const Vec pa = load3(pos, a), d = sub(load3(pos, b), pa);
    out[3LL * i] = __fadd_rn(pa.x, __fmul_rn(t, d.x));
    out[3LL * i + 1] = __fadd_rn(pa.y, __fmul_rn(t, d.y));
    out[3LL * i + 2] = __fadd_rn(pa.z, __fmul_rn(t, d.z));
}

struct Adjoint {
    const float *sdf, *pos, *g;         // [Nv], [Nv, 3], [V, 3]
    const unsigned char *mask;          // [Nv]
    const int *base;                    // [Nv]
    int nv_mesh;
    float *gs, *gp;                     // [Nv], [Nv, 3]
};

// what the slot (a, b) with the incoming g gives its end `u` (far: u is b); added to (gs, gp)
__device__ __forceinline__ void slot_term(const Adjoint &A, int a, int b, int index, bool far, float &gs, Vec &gp) {
    if (index < 0 || index >= A.nv_mesh) return;
    const float sa = A.sdf[a], sb = A.sdf[b];
    const float den = __fsub_rn(sa, sb);
    const float t = __fdiv_rn(sa, den);
    const Vec d = sub(load3(A.pos, b), load3(A.pos, a)), g = load3(A.g, index);
    const float w = __fdiv_rn(dot(g, d), __fmul_rn(den, den));
    gs = __fadd_rn(gs, __fmul_rn(far ? sa : -sb, w));
    const float k = far ? t : __fsub_rn(1.f, t);
    gp.x = __fadd_rn(gp.x, __fmul_rn(k, g.x));
    gp.y = __fadd_rn(gp.y, __fmul_rn(k, g.y));
    gp.z = __fadd_rn(gp.z, __fmul_rn(k, g.z));
}

__global__ void __launch_bounds__(kThreads) k_vertices_adj(Adjoint A, Lattice L) {
    const int u = blockIdx.x * kThreads + threadIdx.x;
    if (u >= L.nv) return;
    const int x = u % L.nx, y = (u / L.nx) % L.ny, z = u / (L.nx * L.ny);
    float gs = 0.f;
    Vec gp = {0.f, 0.f, 0.f};
    const int m = A.mask[u];
    int index = A.base[u];
#pragma unroll
    for (int c = 0; c < 7; ++c) {                             // its own seven slots, ascending
        if (!(m >> c & 1)) continue;
        slot_term(A, u, u + offset_of(L, kClassBits[c]), index, false, gs, gp);
        ++index;
    }
#pragma unroll
    for (int c = 0; c < 7; ++c) {                             // the seven slots it is the far end of, ascending class
        const int b = kClassBits[c];
        if (x < (b & 1) || y < (b >> 1 & 1) || z < (b >> 2 & 1)) continue;
        const int a = u - offset_of(L, b);
        if (!(A.mask[a] >> c & 1)) continue;
        slot_term(A, a, u, slot_index(A.mask, A.base, a, c), true, gs, gp);
    }
    A.gs[u] = gs;
    A.gp[3LL * u] = gp.x;
    A.gp[3LL * u + 1] = gp.y;
    A.gp[3LL * u + 2] = gp.z;
}

// ---- host

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
    return true;
}

inline int passes_of(int blocks) { return blocks <= kThreads ? 1 : 2; }

// the exclusive scan of sums[0 .. blocks) into offsets, the sum of all into *total (device)
inline void scan_sums(int *sums, int *offsets, int blocks, int *sums1, int *offsets1, int *total, hipStream_t st) {
    if (blocks <= kThreads) {
        k_scan_block<<<1, kThreads, 0, st>>>(sums, blocks, nullptr, offsets, total);
        return;
    }
    const int blocks1 = blocks_of<kThreads>(blocks);          // <= 256: Nv <= 256^3
    k_block_sums<<<blocks1, kThreads, 0, st>>>(sums, blocks, sums1);
    k_scan_block<<<1, kThreads, 0, st>>>(sums1, blocks1, nullptr, offsets1, total);
    k_scan_block<<<blocks1, kThreads, 0, st>>>(sums, blocks, offsets1, offsets, nullptr);
}

inline int launched(const std::string &who) {
    return launch_status(who);
}

} // namespace

extern "C" {

int psdr_hip_mtet_plan(int32_t nx, int32_t ny, int32_t nz, int32_t *tile, int32_t *vertex_blocks, int32_t *cell_blocks, int32_t *vertex_passes, int32_t *cell_passes,
                       int32_t *scratch_ints) {
    const std::string who = "psdr_hip_mtet_plan: ";
    Lattice L;
    if (!lattice(who, nx, ny, nz, &L)) return 1;
    if (!tile || !vertex_blocks || !cell_blocks || !vertex_passes || !cell_passes || !scratch_ints) return psdr::api_fail(who + "NULL argument");
    *tile = kThreads;
    *vertex_blocks = blocks_of<kThreads>(L.nv);
    *cell_blocks = blocks_of<kThreads>(L.nc);
    *vertex_passes = passes_of(*vertex_blocks);
    *cell_passes = passes_of(*cell_blocks);
    *scratch_ints = 2 * (*vertex_blocks + blocks_of<kThreads>(*vertex_blocks));          // sums and offsets of both passes; the cells (fewer) use the same ints after the vertices
    return 0;
}

int psdr_hip_mtet_count(const float *sdf, int32_t nx, int32_t ny, int32_t nz, uint8_t *mask, int32_t *base, uint8_t *cell_faces, int32_t *cell_base, int32_t *scratch,
                        int32_t *totals, void *stream) {
    const std::string who = "psdr_hip_mtet_count: ";
    Lattice L;
    if (!lattice(who, nx, ny, nz, &L)) return 1;
    if (!sdf || !mask || !base || !cell_faces || !cell_base || !scratch || !totals) return psdr::api_fail(who + "NULL argument");
    const void *outs[7] = {sdf, mask, base, cell_faces, cell_base, scratch, totals};
    for (int i = 0; i < 7; ++i)
        for (int j = i + 1; j < 7; ++j)
            if (outs[i] == outs[j]) return psdr::api_fail(who + "mask, base, cell_faces, cell_base, scratch and totals must be arrays of their own");
    hipStream_t st = (hipStream_t) stream;
    const int bv = blocks_of<kThreads>(L.nv), bc = blocks_of<kThreads>(L.nc), bv1 = blocks_of<kThreads>(bv);
    int *sums = scratch, *offsets = sums + bv, *sums1 = offsets + bv, *offsets1 = sums1 + bv1;
    k_vertex_mask<<<bv, kThreads, 0, st>>>(sdf, L, mask, sums);
    scan_sums(sums, offsets, bv, sums1, offsets1, totals, st);
    k_scatter<true><<<bv, kThreads, 0, st>>>(mask, L.nv, offsets, base);
    k_cell_count<<<bc, kThreads, 0, st>>>(sdf, L, cell_faces, sums);
    scan_sums(sums, offsets, bc, sums1, offsets1, totals + 1, st);
    k_scatter<false><<<bc, kThreads, 0, st>>>(cell_faces, L.nc, offsets, cell_base);
    return launched(who);
}

int psdr_hip_mtet_emit(const float *sdf, int32_t nx, int32_t ny, int32_t nz, const uint8_t *mask, const int32_t *base, const int32_t *cell_base, int32_t num_vertices,
                       int32_t num_faces, int32_t *edges, int32_t edge_rows, int32_t *faces, int32_t face_rows, void *stream) {
    const std::string who = "psdr_hip_mtet_emit: ";
    Lattice L;
    if (!lattice(who, nx, ny, nz, &L)) return 1;
    if (num_vertices < 1 || (long long) num_vertices > 7LL * L.nv) return psdr::api_fail(who + "num_vertices = " + std::to_string(num_vertices) + ", must lie in [1, 7 Nv]");
    if (num_faces < 1 || (long long) num_faces > 12LL * L.nc) return psdr::api_fail(who + "num_faces = " + std::to_string(num_faces) + ", must lie in [1, 12 cells]");
    if (edge_rows != num_vertices) return psdr::api_fail(who + "edge_rows = " + std::to_string(edge_rows) + " disagrees with the total num_vertices = " + std::to_string(num_vertices));
    if (face_rows != num_faces) return psdr::api_fail(who + "face_rows = " + std::to_string(face_rows) + " disagrees with the total num_faces = " + std::to_string(num_faces));
    if (!sdf || !mask || !base || !cell_base || !edges || !faces) return psdr::api_fail(who + "NULL argument");
    if (edges == faces || (const void *) edges == sdf || (const void *) edges == mask || edges == base || edges == cell_base || (const void *) faces == sdf ||
        (const void *) faces == mask || faces == base || faces == cell_base)
        return psdr::api_fail(who + "edges and faces must be arrays of their own");
    hipStream_t st = (hipStream_t) stream;
    k_emit_edges<<<blocks_of<kThreads>(L.nv), kThreads, 0, st>>>(L, mask, base, num_vertices, edges);
    k_emit_faces<<<blocks_of<kThreads>(L.nc), kThreads, 0, st>>>(sdf, L, mask, base, cell_base, num_faces, faces);
    return launched(who);
}

int psdr_hip_mtet_vertices(const float *sdf, const float *pos, int32_t nx, int32_t ny, int32_t nz, const int32_t *edges, int32_t num_vertices, float *v, void *stream) {
    const std::string who = "psdr_hip_mtet_vertices: ";
    Lattice L;
    if (!lattice(who, nx, ny, nz, &L)) return 1;
    if (num_vertices < 1 || (long long) num_vertices > 7LL * L.nv) return psdr::api_fail(who + "num_vertices = " + std::to_string(num_vertices) + ", must lie in [1, 7 Nv]");
    if (!sdf || !pos || !edges || !v) return psdr::api_fail(who + "NULL argument");
    if (v == sdf || v == pos || (const void *) v == edges) return psdr::api_fail(who + "v must be an array of its own");
    k_vertices<<<blocks_of<kThreads>(num_vertices), kThreads, 0, (hipStream_t) stream>>>(sdf, pos, L.nv, edges, num_vertices, v);
    return launched(who);
}

int psdr_hip_mtet_vertices_adj(const float *sdf, const float *pos, int32_t nx, int32_t ny, int32_t nz, const uint8_t *mask, const int32_t *base, int32_t num_vertices,
                               const float *g, float *grad_sdf, float *grad_pos, void *stream) {
    const std::string who = "psdr_hip_mtet_vertices_adj: ";
    Lattice L;
    if (!lattice(who, nx, ny, nz, &L)) return 1;
    if (num_vertices < 1 || (long long) num_vertices > 7LL * L.nv) return psdr::api_fail(who + "num_vertices = " + std::to_string(num_vertices) + ", must lie in [1, 7 Nv]");
    if (!sdf || !pos || !mask || !base || !g || !grad_sdf || !grad_pos) return psdr::api_fail(who + "NULL argument");
    if (grad_sdf == grad_pos || grad_sdf == sdf || grad_sdf == pos || grad_sdf == g || grad_pos == sdf || grad_pos == pos || grad_pos == g ||
        (const void *) grad_sdf == mask || (const void *) grad_sdf == base || (const void *) grad_pos == mask || (const void *) grad_pos == base)
        return psdr::api_fail(who + "grad_sdf and grad_pos must be arrays of their own");
    Adjoint A;
    A.sdf = sdf; A.pos = pos; A.g = g;
    A.mask = mask; A.base = base;
    A.nv_mesh = num_vertices;
    A.gs = grad_sdf; A.gp = grad_pos;
    k_vertices_adj<<<blocks_of<kThreads>(L.nv), kThreads, 0, (hipStream_t) stream>>>(A, L);
    return launched(who);
}

} // extern "C"
