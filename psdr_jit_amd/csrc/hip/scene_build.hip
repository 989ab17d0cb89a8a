// scene_build.hip — psdr_hip_scene_create / psdr_hip_scene_update: from a configured-scene snapshot to the device-resident scene.
//
// Replaces what the reference does at the end of every Scene::configure() (src/scene/scene.cpp:311-599): the jit uploads of the
// concatenated scene arrays and Scene_OptiX::configure (src/scene/scene_optix.cpp:265-332), which rebuilds the OptiX geometry
// acceleration structure on the device (optixAccelBuild, :310).  The reference's usage pattern is set_transform -> configure ->
// renderD -> backward once per optimisation step (README.md:87-106), so this is on the path of every step:
//
//   * nothing geometric changed (a colour, a texel, the camera, a forward tangent): the tree and the triangle order stay, only the
//     sections of the scene blob the change touches are rewritten in the pinned host copy and sent;
//   * vertices moved, topology unchanged: the triangle sections are rewritten and the 4-wide tree is REFITTED on the device, bottom
//     up, one small kernel launch per level of the tree (k_refit_level), with the builder's own box and quantisation code (bvh.h), so
//     a refitted node holds the bytes the builder would produce for the same topology.  The refit also evaluates the tree's SAH cost;
//   * the cost exceeds kRebuildFactor x the cost at build time, or the triangle count changed: the tree is built again (bvh.h::
//     build_bvh, host threads) and every section is rewritten.
// The hit of a ray is defined by the exact triangle test alone (trav4.h), so none of this can change a result - only how many nodes a
// ray visits (tests/test_gpu_configure.py: hits after refits against the oracle's brute-force definition, bit-equal).
#include <chrono>
#include <cstdio>

#include "scene_obj.h"
#include "bvh.h"
#include "filter.h"
#include "cam_table.h"
#include "blob_rows.h"
#include "blob_layout.h"
#include "../host/hnum.h"
#include "../host/edge_select.h"

using namespace psdr;

static int fail(const std::string &msg) { return psdr::api_fail(msg); }

constexpr double kRebuildFactor = 1.4;          // a refitted tree whose SAH cost exceeds this multiple of the cost it was built with is built again

static inline double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// The live-pixel mask of one sensor from the scene's screen-space coverage (cam_table.h): bit (y * width + x) = some triangle comes within a quarter of a pixel
// of the pixel's square.
static void fill_live_mask(const ScreenTris &st, int W, int H, std::vector<unsigned> &mask) {
    mask.assign(((size_t) W * H + 31) / 32, 0u);
    cover_rows(st, W, H, [&](int, int row, int c0, int c1) {
        // bits [b0, b1] of the mask, a word at a time (a wall of the Cornell box at 2048 x 2048 is four million pixels per triangle)
        const size_t b0 = (size_t) row * W + c0, b1 = (size_t) row * W + c1;
        for (size_t wi = b0 >> 5; wi <= (b1 >> 5); ++wi) {
            const unsigned lo_bit = wi == (b0 >> 5) ? (unsigned) (b0 & 31) : 0u, hi_bit = wi == (b1 >> 5) ? (unsigned) (b1 & 31) : 31u;
            const unsigned m_hi = hi_bit == 31u ? 0xffffffffu : ((1u << (hi_bit + 1u)) - 1u);
            mask[wi] |= m_hi & ~((1u << lo_bit) - 1u);
        }
    });
}

// The camera-ray table of one sensor (SensorDev::cam_tab, cam_table.h): the same coverage, one bit per traversal slot and cell, made where it is read - one thread
// per cell, from the traversal rows of the blob (slot order) and the sensor's world_to_sample, in the host's own double arithmetic.  At most kBruteForceMax
// triangles, none of them across the camera plane (the host has checked): their projections wait in LDS.
struct W2S { float m[16]; };
__global__ void k_cam_table(const float4 *__restrict__ blob, int trav_off, int n_tris, const W2S w2s, int W, int H, int shift, int cells_w, int cells_h,
                            unsigned long long *__restrict__ table) {
    __shared__ double sX[3 * kBruteForceMax], sY[3 * kBruteForceMax];
    __shared__ int s_front[kBruteForceMax];
    for (int k = threadIdx.x; k < n_tris; k += blockDim.x) {
        const float4 a = blob[trav_off + 3 * k], b = blob[trav_off + 3 * k + 1], c = blob[trav_off + 3 * k + 2];
        const float p0[3] = {a.x, a.y, a.z}, e1[3] = {a.w, b.x, b.y}, e2[3] = {b.z, b.w, c.x};
        s_front[k] = project_triangle(w2s.m, p0, e1, e2, W, H, &sX[3 * k], &sY[3 * k]) == 0;
    }
    __syncthreads();
    const int cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= cells_w * cells_h) return;
    const int g = 1 << shift, x0 = (cell % cells_w) << shift, y0 = (cell / cells_w) << shift;
    const int x1 = x0 + g - 1 < W - 1 ? x0 + g - 1 : W - 1, y1 = y0 + g - 1 < H - 1 ? y0 + g - 1 : H - 1;
    unsigned long long word = 0ull;
    for (int k = 0; k < n_tris; ++k)
        if (s_front[k] && covers_cell(&sX[3 * k], &sY[3 * k], W, H, x0, x1, y0, y1)) word |= 1ull << k;
    table[cell] = word;
}

// ------------------------------------------------------------------------------------------------
// refit of the 4-wide tree (bvh.h::Bvh4Result layout) after the triangles moved
//
// One thread per node of one level (`ids`: node indices of equal height above the leaves, children always in an earlier launch): the
// float box of every child - the union of a leaf's padded triangle boxes (from the traversal rows the update has just sent), or the box
// an earlier level stored for an inner child - then the node's ten box words by bvh.h::bvh_quantise, the child codes untouched.
// `cost` accumulates sum half_area(child box) x (triangles of a leaf | 1): the tree's SAH cost up to the division by the root's area.
__global__ void k_refit_level(float4 *__restrict__ blob, int nodes_off, int trav_off, const int *__restrict__ ids, int count, unsigned leaf_bit,
                              float *__restrict__ fbox, double *__restrict__ cost) {
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    double c = 0.0;
    if (tid < count) {
        const int node = ids[tid];
        float *q = reinterpret_cast<float *>(blob + nodes_off + (kNodeFloats / 4) * (size_t) node);
        const uint32_t *codes = reinterpret_cast<const uint32_t *>(q) + kNodeCodeOff;
        float los[kBvhW][3], his[kBvhW][3];
        float ulo[3] = {3e38f, 3e38f, 3e38f}, uhi[3] = {-3e38f, -3e38f, -3e38f};
        int nc = 0;
        for (int k = 0; k < kBvhW; ++k) {
            const uint32_t code = codes[k];
            if (code == 0xffffffffu) break;
            ++nc;
            float lo[3], hi[3];
            float weight = 1.f;
            if (code & leaf_bit) {
                const int payload = (int) (code & (leaf_bit - 1u)), first = payload >> 2, cnt = (payload & 3) + 1;
                weight = (float) cnt;
                for (int a = 0; a < 3; ++a) { lo[a] = 3e38f; hi[a] = -3e38f; }
                for (int t = 0; t < cnt; ++t) {
                    const float4 w0 = blob[trav_off + 3 * (size_t) (first + t)], w1 = blob[trav_off + 3 * (size_t) (first + t) + 1], w2 = blob[trav_off + 3 * (size_t) (first + t) + 2];
                    const float p0[3] = {w0.x, w0.y, w0.z}, e1[3] = {w0.w, w1.x, w1.y}, e2[3] = {w1.z, w1.w, w2.x};
                    float tl[3], th[3];
                    bvh_tri_box(p0, e1, e2, tl, th);
                    for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], tl[a]); hi[a] = fmaxf(hi[a], th[a]); }
                }
            } else {
                const float *b = fbox + 6 * (size_t) code;
                for (int a = 0; a < 3; ++a) { lo[a] = b[a]; hi[a] = b[3 + a]; }
            }
            for (int a = 0; a < 3; ++a) { los[k][a] = lo[a]; his[k][a] = hi[a]; ulo[a] = fminf(ulo[a], lo[a]); uhi[a] = fmaxf(uhi[a], hi[a]); }
            c += (double) bvh_half_area(lo, hi) * (double) weight;
        }
        if (nc > 0) {
            bvh_quantise(los, his, nc, q);
            float *b = fbox + 6 * (size_t) node;
            for (int a = 0; a < 3; ++a) { b[a] = ulo[a]; b[3 + a] = uhi[a]; }
        }
    }
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if ((threadIdx.x & 63) == 0 && c != 0.0) atomicAdd(cost, c);
}

// ------------------------------------------------------------------------------------------------
// the tree: built on the host (bvh.h), its topology kept for refits
static int tree_build(psdr_hip_scene *sc, const psdr_triangles &tr, std::vector<float> &nodes_out) {
    const int n = tr.n_triangles;
    BvhResult bvh;
    build_bvh(tr.p0, tr.e1, tr.e2, n, bvh);
    Bvh4Result bvh4;
    build_bvh4(bvh, n, bvh4);
    sc->order = bvh.order;
    sc->orig2slot.assign((size_t) n, 0);
    for (int slot = 0; slot < n; ++slot) sc->orig2slot[(size_t) bvh.order[(size_t) slot]] = slot;
    sc->tree_tris = n;
    sc->tree_max_stack = bvh4.max_stack; sc->tree_ref_bits = bvh4.ref_bits;
    sc->n_leaves = bvh.n_leaves; sc->max_depth = bvh4.max_depth;
    sc->T.n_nodes = bvh4.n_nodes; sc->T.ref_bits = bvh4.ref_bits;
    sc->cost_built = bvh4.cost;
    // refit schedule: node ids by height above the leaves (counting sort), one launch per height
    int levels = 0;
    for (int h : bvh4.height) levels = std::max(levels, h + 1);
    sc->refit_level_begin.assign((size_t) levels + 1, 0);
    for (int h : bvh4.height) sc->refit_level_begin[(size_t) h + 1]++;
    for (int l = 0; l < levels; ++l) sc->refit_level_begin[(size_t) l + 1] += sc->refit_level_begin[(size_t) l];
    std::vector<int> ids((size_t) std::max(1, bvh4.n_nodes)), at(sc->refit_level_begin.begin(), sc->refit_level_begin.end());
    for (int i = 0; i < bvh4.n_nodes; ++i) ids[(size_t) at[(size_t) bvh4.height[(size_t) i]]++] = i;
    if (sc->refit_order.upload(ids.data(), ids.size() * sizeof(int))) return 1;
    if (sc->refit_box.ensure(sizeof(float) * 6 * (size_t) std::max(1, bvh4.n_nodes))) return 1;
    if (sc->refit_cost.ensure(sizeof(double))) return 1;
    nodes_out.swap(bvh4.nodes);
    return 0;
}

// refit the device tree from the traversal rows in the device blob; -> *cost = the refitted tree's SAH cost (normalised like Bvh4Result::cost)
static int tree_refit(psdr_hip_scene *sc, double *cost) {
    const SceneTables &T = sc->T;
    hipStream_t st = nullptr;
    HIPCHK(hipMemsetAsync(sc->refit_cost.p, 0, sizeof(double), st));
    const unsigned leaf_bit = 1u << (T.ref_bits - 1);
    for (size_t l = 0; l + 1 < sc->refit_level_begin.size(); ++l) {
        const int begin = sc->refit_level_begin[l], count = sc->refit_level_begin[l + 1] - begin;
        if (count <= 0) continue;
        hipLaunchKernelGGL(k_refit_level, dim3((unsigned) ((count + 127) / 128)), dim3(128), 0, st, (float4 *) sc->blob.p, T.nodes_off, T.trav_off,
                           sc->refit_order.as<int>() + begin, count, leaf_bit, (float *) sc->refit_box.p, (double *) sc->refit_cost.p);
    }
    HIPCHK(hipGetLastError());
    double sum = 0.0;
    float root[6];
    HIPCHK(hipMemcpyAsync(&sum, sc->refit_cost.p, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(root, sc->refit_box.p, sizeof(root), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const double area = std::max((double) bvh_half_area(root, root + 3), 1e-300);
    *cost = sum / area;
    return 0;
}

// a device array outside the blob: (re)allocated when its size changed, copied unless the caller vouches for the content
template <typename P> static int sync_named(psdr_hip_scene *sc, const std::string &key, const void *src, size_t bytes, bool same, const P *&out, psdr_update_info &info) {
    out = nullptr;
    if (!src) return 0;
    DevBuf &b = sc->buf(key);
    bool moved = false;
    if (b.ensure(bytes, &moved)) return 1;
    if (moved) info.reallocated++;
    if (moved || !same) {
        HIPCHK(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));          // (synchronous: the sources are the caller's arrays or temporaries of scene_sync)
        info.bytes_uploaded += (int64_t) bytes;
    }
    out = reinterpret_cast<const P *>(b.p);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// GEOMETRY ON THE DEVICE (round 6; psdr_mesh_geometry, include/psdr_hip.h).  The reference's Mesh::configure / process_mesh run on drjit device arrays
// (src/shape/mesh.cpp:23-62, 317-400); until this round a moved vertex made the HOST recompute every row of its mesh and psdr_hip_scene_update rewrite and send
// them (34 MB for config 5).  Here the rows of the moved meshes are computed by five small kernels from the raw vertices and the composed transform, in the
// host's own dual-number code (csrc/host/hnum.h, __host__ __device__; -ffp-contract=off and correctly rounded division / square root on both sides), so the
// sections hold the bits the host would have written (psdr_hip_scene_check_rows compares them):
//   k_geo_world    world[v]  = xform_pos(to_world, raw[v])                              Mesh::configure, mesh.cpp:330-340
//   k_geo_face     fn[f]     = cross(e1, e2), area2[f] = |fn|                           process_mesh, mesh.cpp:26-33
//   k_geo_vnormal  vn[v]     = normalize(sum fn / sum area2) over the vertex' faces in the reference's scatter order     mesh.cpp:34-44
//   k_geo_rows     traversal / shading / tangent rows of the blob, at the slot of the triangle (leaf order)
//   k_geo_sec      secondary-edge rows (mesh.cpp:355-369, scene.cpp:546-571); their CDF stays with the host (a sequential float prefix sum the parity tests pin)
struct GeoMeshDev { float tw[16], d_tw[16]; int v_off, n_v, f_off, n_f, e_off, n_e, mesh_id, flat, moved, pad[3]; };
using psdr_host::DF; using psdr_host::D3; using psdr_host::DM4;

__device__ inline D3 geo_ld(const float *a, size_t i) { const float *q = a + 6 * i; return D3{DF(q[0], q[1]), DF(q[2], q[3]), DF(q[4], q[5])}; }
__device__ inline void geo_st(float *a, size_t i, const D3 &v) { float *q = a + 6 * i; q[0] = v.x.v; q[1] = v.x.d; q[2] = v.y.v; q[3] = v.y.d; q[4] = v.z.v; q[5] = v.z.d; }

__global__ void k_geo_world(const GeoMeshDev *__restrict__ M, const int *__restrict__ vmesh, const float *__restrict__ raw, const float *__restrict__ d_raw,
                            float *__restrict__ world, int nv) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const GeoMeshDev &m = M[vmesh[v]];
    if (!m.moved) return;
    DM4 tw;
    for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) tw.m[i][j] = DF(m.tw[4 * i + j], m.d_tw[4 * i + j]);
    const D3 p{DF(raw[3 * (size_t) v], d_raw[3 * (size_t) v]), DF(raw[3 * (size_t) v + 1], d_raw[3 * (size_t) v + 1]), DF(raw[3 * (size_t) v + 2], d_raw[3 * (size_t) v + 2])};
    geo_st(world, (size_t) v, psdr_host::xform_pos(tw, p));
}

__global__ void k_geo_face(const GeoMeshDev *__restrict__ M, const int *__restrict__ fmesh, const int *__restrict__ faces, const float *__restrict__ world,
                           float *__restrict__ fnrm, float *__restrict__ farea, int nf) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    if (!M[fmesh[f]].moved) return;
    const D3 p0 = geo_ld(world, (size_t) faces[3 * (size_t) f]), e1 = geo_ld(world, (size_t) faces[3 * (size_t) f + 1]) - p0, e2 = geo_ld(world, (size_t) faces[3 * (size_t) f + 2]) - p0;
    const D3 n = psdr_host::dcross(e1, e2);
    const DF a = psdr_host::dnorm(n);
    geo_st(fnrm, (size_t) f, n);
    farea[2 * (size_t) f] = a.v; farea[2 * (size_t) f + 1] = a.d;
}

__global__ void k_geo_vnormal(const GeoMeshDev *__restrict__ M, const int *__restrict__ vmesh, const int *__restrict__ vf_begin, const int *__restrict__ vf_item,
                              const float *__restrict__ fnrm, const float *__restrict__ farea, float *__restrict__ vn, int nv) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    if (!M[vmesh[v]].moved) return;
    D3 acc; DF w;
    for (int k = vf_begin[v]; k < vf_begin[v + 1]; ++k) {
        const size_t f = (size_t) (vf_item[k] >> 2);
        acc = acc + geo_ld(fnrm, f);
        w = w + DF(farea[2 * f], farea[2 * f + 1]);
    }
    geo_st(vn, (size_t) v, psdr_host::dnormalize(acc / w));
}

__device__ inline float geo_ibits(int v) { return __int_as_float(v); }
__device__ inline float4 geo_f4(float x, float y, float z, float w) { using psdr_host::canon_nan; return make_float4(canon_nan(x), canon_nan(y), canon_nan(z), canon_nan(w)); }
__device__ inline float geo_c(float x) { return psdr_host::canon_nan(x); }

__global__ void k_geo_rows(float4 *__restrict__ blob, SceneTables T, const GeoMeshDev *__restrict__ M, const int *__restrict__ fmesh, const int *__restrict__ faces,
                           const float *__restrict__ world, const float *__restrict__ fnrm, const float *__restrict__ farea, const float *__restrict__ vn, int nf, int values, int tangents) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    const GeoMeshDev &m = M[fmesh[f]];
    if (!m.moved) return;
    const int slot = reinterpret_cast<const int *>(blob + T.map_off)[f];
    const int i0 = faces[3 * (size_t) f], i1 = faces[3 * (size_t) f + 1], i2 = faces[3 * (size_t) f + 2];
    const D3 p0 = geo_ld(world, (size_t) i0), e1 = geo_ld(world, (size_t) i1) - p0, e2 = geo_ld(world, (size_t) i2) - p0;
    const D3 n0 = geo_ld(vn, (size_t) i0), n1 = geo_ld(vn, (size_t) i1), n2 = geo_ld(vn, (size_t) i2);
    const DF a2 = DF(farea[2 * (size_t) f], farea[2 * (size_t) f + 1]);
    const D3 fn = geo_ld(fnrm, (size_t) f) / a2;
    const DF area = a2 * DF(0.5f);
    if (values) {
        float4 *t = blob + T.trav_off + 3 * (size_t) slot;
        t[0] = geo_f4(p0.x.v, p0.y.v, p0.z.v, e1.x.v);
        t[1] = geo_f4(e1.y.v, e1.z.v, e2.x.v, e2.y.v);
        t[2] = make_float4(geo_c(e2.z.v), geo_ibits(f), 0.f, 0.f);
        float4 *w = blob + T.shade_off + 6 * (size_t) slot;          // (words 4 and 5 - the uv of the three corners - do not depend on the vertices)
        w[0] = geo_f4(n0.x.v, n0.y.v, n0.z.v, area.v);
        w[1] = make_float4(geo_c(n1.x.v), geo_c(n1.y.v), geo_c(n1.z.v), geo_ibits(m.mesh_id));
        w[2] = make_float4(geo_c(n2.x.v), geo_c(n2.y.v), geo_c(n2.z.v), geo_ibits(m.flat ? 1 : 0));
        w[3] = make_float4(geo_c(fn.x.v), geo_c(fn.y.v), geo_c(fn.z.v), geo_ibits(f));
    }
    if (tangents && T.has_tangent) {
        float4 *w = blob + T.tan_off + 6 * (size_t) slot;
        w[0] = geo_f4(p0.x.d, p0.y.d, p0.z.d, e1.x.d);
        w[1] = geo_f4(e1.y.d, e1.z.d, e2.x.d, e2.y.d);
        w[2] = geo_f4(e2.z.d, n0.x.d, n0.y.d, n0.z.d);
        w[3] = geo_f4(n1.x.d, n1.y.d, n1.z.d, n2.x.d);
        w[4] = geo_f4(n2.y.d, n2.z.d, fn.x.d, fn.y.d);
        w[5] = geo_f4(fn.z.d, area.d, 0.f, 0.f);
    }
}

// edges: [ne][6] = v0 v1 opp (global vertex ids), f0 f1 (global face ids, f1 = -1: boundary), mesh index
__global__ void k_geo_sec(float4 *__restrict__ blob, int sec_off, const GeoMeshDev *__restrict__ M, const int *__restrict__ edges, const float *__restrict__ world,
                          const float *__restrict__ fnrm, const float *__restrict__ farea, int ne) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= ne) return;
    const int *e = edges + 6 * (size_t) r;
    if (!M[e[5]].moved) return;
    const D3 a = geo_ld(world, (size_t) e[0]), b = geo_ld(world, (size_t) e[1]), c = geo_ld(world, (size_t) e[2]);
    const float e1[3] = {b.x.v - a.x.v, b.y.v - a.y.v, b.z.v - a.z.v}, de1[3] = {b.x.d - a.x.d, b.y.d - a.y.d, b.z.d - a.z.d};
    const D3 n0 = geo_ld(fnrm, (size_t) e[3]) / DF(farea[2 * (size_t) e[3]], farea[2 * (size_t) e[3] + 1]);
    float n1[3] = {0.f, 0.f, 0.f};
    if (e[4] >= 0) { const D3 q = geo_ld(fnrm, (size_t) e[4]) / DF(farea[2 * (size_t) e[4]], farea[2 * (size_t) e[4] + 1]); n1[0] = q.x.v; n1[1] = q.y.v; n1[2] = q.z.v; }
    float4 *w = blob + sec_off + 6 * (size_t) r;
    w[0] = geo_f4(a.x.v, a.y.v, a.z.v, e1[0]);
    w[1] = geo_f4(e1[1], e1[2], n0.x.v, n0.y.v);
    w[2] = geo_f4(n0.z.v, n1[0], n1[1], n1[2]);
    w[3] = make_float4(geo_c(c.x.v), geo_c(c.y.v), geo_c(c.z.v), geo_ibits(e[4] < 0 ? 1 : 0));
    w[4] = geo_f4(a.x.d, a.y.d, a.z.d, de1[0]);
    w[5] = geo_f4(de1[1], de1[2], 0.f, 0.f);
}

// The topology lists of one mesh, checked before anything is filled or uploaded: the kernels above index the world vertices, face normals and areas with these
// ids unchecked, so one bad id is an out-of-bounds device read.  -> 1 (fail() with the list named) on the first violation.
static int validate_geometry(const psdr_mesh_geometry &g, int mesh) {
    const int nv = g.n_vertices, nf = g.n_faces;
    auto bad = [&](const char *what) { return fail("psdr_mesh_geometry[" + std::to_string(mesh) + "]: " + what); };
    if (nv < 0 || nf < 0 || g.n_edges < 0) return bad("negative count");
    for (size_t i = 0; i < 3 * (size_t) nf; ++i)
        if (g.faces[i] < 0 || g.faces[i] >= nv) return bad("faces: vertex id outside the mesh's vertices");
    if (g.vf_begin[0] != 0) return bad("vf_begin[0] is not 0");
    for (int v = 0; v < nv; ++v)
        if (g.vf_begin[v + 1] < g.vf_begin[v]) return bad("vf_begin decreases");
    if ((size_t) g.vf_begin[nv] != 3 * (size_t) nf) return bad("vf_begin[n_vertices] is not 3 * n_faces");
    for (size_t k = 0; k < 3 * (size_t) nf; ++k)
        if (g.vf_item[k] < 0 || (g.vf_item[k] >> 2) >= nf) return bad("vf_item: face id outside the mesh's faces");
    for (size_t e = 0; e < (size_t) g.n_edges; ++e) {
        const int32_t *q = g.edges + 5 * e;            // v0 v1 f0 f1 opp
        if (q[0] < 0 || q[0] >= nv || q[1] < 0 || q[1] >= nv || q[4] < 0 || q[4] >= nv) return bad("edges: v0 / v1 / opp outside the mesh's vertices");
        if (q[2] < 0 || q[2] >= nf || q[3] < -1 || q[3] >= nf) return bad("edges: f0 / f1 outside the mesh's faces (f1 = -1: boundary)");
    }
    return 0;
}

// uploads what the kernels need (topology when a mesh's version changed, raw vertices and transforms of the moved meshes) and runs them; -> 1 on error.
// `usable` = false (nothing done) when the snapshot's geometry does not describe the scene's triangles and edges one to one.
static int geometry_on_device(psdr_hip_scene *sc, const psdr_scene_snapshot *s, bool values, bool tangents, bool sec_rows, psdr_update_info &info, bool &usable) {
    usable = false;
    const psdr_mesh_geometry *G = s->geometry;
    if (!G) return 0;
    const int nm = s->n_meshes;
    size_t NV = 0, NF = 0, NE = 0;
    for (int i = 0; i < nm; ++i) {
        if (G[i].n_faces != s->meshes[i].n_faces || (size_t) s->meshes[i].face_offset != NF || !G[i].vertices_raw || !G[i].d_vertices_raw || !G[i].faces || !G[i].vf_begin || !G[i].vf_item) return 0;
        if (G[i].n_edges > 0 && !G[i].edges) return 0;
        NV += (size_t) G[i].n_vertices; NF += (size_t) G[i].n_faces; NE += (size_t) G[i].n_edges;
    }
    if (NF != (size_t) s->tris.n_triangles || NE != (size_t) std::max(0, s->sec_edges.n_edges) || NV == 0) return 0;
    // ---- topology: kept while every mesh reports the version (and the counts) the device saw last
    bool same_topo = sc->geo_versions.size() == (size_t) nm && sc->geo_counts.size() == 3 * (size_t) nm;
    for (int i = 0; same_topo && i < nm; ++i)
        same_topo = sc->geo_versions[(size_t) i] == G[i].topology_version && sc->geo_counts[3 * (size_t) i] == G[i].n_vertices && sc->geo_counts[3 * (size_t) i + 1] == G[i].n_faces &&
                    sc->geo_counts[3 * (size_t) i + 2] == G[i].n_edges;
    // (the lists are read only when the topology travels; a kept topology was checked when it did)
    if (!same_topo)
        for (int i = 0; i < nm; ++i)
            if (validate_geometry(G[i], i)) return 1;
    std::vector<GeoMeshDev> mt((size_t) nm);
    {
        size_t vo = 0, fo = 0, eo = 0;
        for (int i = 0; i < nm; ++i) {
            GeoMeshDev &m = mt[(size_t) i];
            std::memcpy(m.tw, G[i].to_world, 64); std::memcpy(m.d_tw, G[i].d_to_world, 64);
            m.v_off = (int) vo; m.n_v = G[i].n_vertices; m.f_off = (int) fo; m.n_f = G[i].n_faces; m.e_off = (int) eo; m.n_e = G[i].n_edges;
            m.mesh_id = G[i].mesh_id; m.flat = G[i].use_face_normals; m.moved = (G[i].moved || !same_topo || !sc->geo_world_current) ? 1 : 0; m.pad[0] = m.pad[1] = m.pad[2] = 0;
            vo += (size_t) G[i].n_vertices; fo += (size_t) G[i].n_faces; eo += (size_t) G[i].n_edges;
        }
    }
    auto up = [&](const char *key, const void *src, size_t bytes) -> int {
        DevBuf &b = sc->buf(key);
        if (b.ensure(bytes)) return 1;
        if (src) { HIPCHK(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice)); info.bytes_uploaded += (int64_t) bytes; }         // (synchronous: the sources are locals of this function)
        return 0;
    };
    if (!same_topo) {
        std::vector<int> faces(3 * NF), vmesh(NV), fmesh(NF), vfb(NV + 1), vfi(3 * NF), edges(6 * std::max<size_t>(1, NE));
        size_t k = 0;
        vfb[0] = 0;
        for (int i = 0; i < nm; ++i) {
            const GeoMeshDev &m = mt[(size_t) i];
            for (int v = 0; v < m.n_v; ++v) vmesh[(size_t) m.v_off + (size_t) v] = i;
            for (int f = 0; f < m.n_f; ++f) {
                fmesh[(size_t) m.f_off + (size_t) f] = i;
                for (int c = 0; c < 3; ++c) faces[3 * ((size_t) m.f_off + (size_t) f) + c] = m.v_off + G[i].faces[3 * (size_t) f + c];
            }
            // (vf_begin of a mesh counts from 0; items are (local face << 2 | corner): both move to the global numbering)
            for (int v = 0; v < m.n_v; ++v) {
                for (int q = G[i].vf_begin[v]; q < G[i].vf_begin[v + 1]; ++q) { const int it = G[i].vf_item[q]; vfi[k++] = (((it >> 2) + m.f_off) << 2) | (it & 3); }
                vfb[(size_t) m.v_off + (size_t) v + 1] = (int) k;
            }
            for (int e = 0; e < m.n_e; ++e) {
                const int *q = G[i].edges + 5 * (size_t) e;
                int *d = &edges[6 * ((size_t) m.e_off + (size_t) e)];
                d[0] = m.v_off + q[0]; d[1] = m.v_off + q[1]; d[2] = m.v_off + q[4]; d[3] = m.f_off + q[2]; d[4] = q[3] >= 0 ? m.f_off + q[3] : -1; d[5] = i;
            }
        }
        if (up("geo.faces", faces.data(), faces.size() * 4) || up("geo.vmesh", vmesh.data(), vmesh.size() * 4) || up("geo.fmesh", fmesh.data(), fmesh.size() * 4) ||
            up("geo.vf_begin", vfb.data(), vfb.size() * 4) || up("geo.vf_item", vfi.data(), vfi.size() * 4) || up("geo.edges", edges.data(), edges.size() * 4)) return 1;
        if (up("geo.raw", nullptr, 12 * NV) || up("geo.d_raw", nullptr, 12 * NV) || up("geo.world", nullptr, 24 * NV) || up("geo.vn", nullptr, 24 * NV) ||
            up("geo.fnrm", nullptr, 24 * NF) || up("geo.farea", nullptr, 8 * NF)) return 1;
        HIPCHK(hipStreamSynchronize(nullptr));                     // (the staging vectors go out of scope)
        sc->geo_versions.resize((size_t) nm); sc->geo_counts.resize(3 * (size_t) nm);
        for (int i = 0; i < nm; ++i) {
            sc->geo_versions[(size_t) i] = G[i].topology_version;
            sc->geo_counts[3 * (size_t) i] = G[i].n_vertices; sc->geo_counts[3 * (size_t) i + 1] = G[i].n_faces; sc->geo_counts[3 * (size_t) i + 2] = G[i].n_edges;
        }
    }
    // ---- this update's inputs: the mesh table, raw vertices and their tangents of the moved meshes
    if (up("geo.meshes", mt.data(), mt.size() * sizeof(GeoMeshDev))) return 1;
    float *raw = (float *) sc->buf("geo.raw").p, *d_raw = (float *) sc->buf("geo.d_raw").p;
    bool any = false;
    for (int i = 0; i < nm; ++i) {
        const GeoMeshDev &m = mt[(size_t) i];
        if (!m.moved || m.n_v == 0) continue;
        any = true;
        HIPCHK(hipMemcpyAsync(raw + 3 * (size_t) m.v_off, G[i].vertices_raw, 12 * (size_t) m.n_v, hipMemcpyHostToDevice, nullptr));
        HIPCHK(hipMemcpyAsync(d_raw + 3 * (size_t) m.v_off, G[i].d_vertices_raw, 12 * (size_t) m.n_v, hipMemcpyHostToDevice, nullptr));
        info.bytes_uploaded += (int64_t) (24 * (size_t) m.n_v);
    }
    usable = true;
    if (!any) return 0;
    const GeoMeshDev *Md = sc->buf("geo.meshes").as<GeoMeshDev>();
    const int *vmesh = sc->buf("geo.vmesh").as<int>(), *fmesh = sc->buf("geo.fmesh").as<int>(), *faces = sc->buf("geo.faces").as<int>();
    float *world = (float *) sc->buf("geo.world").p, *vn = (float *) sc->buf("geo.vn").p, *fnrm = (float *) sc->buf("geo.fnrm").p, *farea = (float *) sc->buf("geo.farea").p;
    const unsigned bv = (unsigned) ((NV + 255) / 256), bf = (unsigned) ((NF + 255) / 256), be = (unsigned) ((NE + 255) / 256);
    hipLaunchKernelGGL(k_geo_world, dim3(bv), dim3(256), 0, nullptr, Md, vmesh, raw, d_raw, world, (int) NV);
    hipLaunchKernelGGL(k_geo_face, dim3(bf), dim3(256), 0, nullptr, Md, fmesh, faces, world, fnrm, farea, (int) NF);
    hipLaunchKernelGGL(k_geo_vnormal, dim3(bv), dim3(256), 0, nullptr, Md, vmesh, sc->buf("geo.vf_begin").as<int>(), sc->buf("geo.vf_item").as<int>(), fnrm, farea, vn, (int) NV);
    if (values || tangents)
        hipLaunchKernelGGL(k_geo_rows, dim3(bf), dim3(256), 0, nullptr, (float4 *) sc->blob.p, sc->T, Md, fmesh, faces, world, fnrm, farea, vn, (int) NF, values ? 1 : 0, tangents ? 1 : 0);
    if (sec_rows && NE > 0)
        hipLaunchKernelGGL(k_geo_sec, dim3(be), dim3(256), 0, nullptr, (float4 *) sc->blob.p, sc->E.off, Md, sc->buf("geo.edges").as<int>(), world, fnrm, farea, (int) NE);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(nullptr));                         // (the mesh table is a local; the kernels take ~0.1 ms)
    sc->geo_world_current = true;                                  // (world / fnrm / farea hold this state of EVERY mesh: what the primary-edge selection below reads)
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// PRIMARY EDGES ON THE DEVICE (psdr_hip_scene_update_edges, include/psdr_hip.h).  The reference selects a sensor's primary edges on drjit device arrays in every
// Scene::configure (src/sensor/perspective.cpp:52-151: the silhouette test, then compressD); here the host walked every edge of every mesh and sent the kept rows.
// With the world vertices, face normals and areas of geometry_on_device resident, three small kernels do it per sensor, calling the host's own keep test and row
// (csrc/host/edge_select.h, compiled for both sides):
//   k_pe_flags   one flag per enabled edge + the number kept per 256-thread workgroup (wave64 ballot / popcount)
//   k_pe_bases   exclusive scan of the workgroup counts (one workgroup; integers, so the order of the partial sums is immaterial), the total behind them
//   k_pe_rows    rank of a kept edge = workgroup base + kept edges of the earlier waves + popcount of the ballot below its lane: the position an in-order walk over
//                meshes and edges gives it (no atomics: they would not preserve the order the host's chain rule and ids index by); writes the row, the PMF entry,
//                the length and the (mesh, v0, v1) ids
// The distribution is completed by cdf_on_device (below); the kept lengths (the PMF words) and ids come back for the float sum and the host's chain rule.
// ---- the CDF of an edge distribution on the device.  DiscreteDistribution::init (reference src/core/pmf.cpp:6-15; csrc/host/scene_host.cpp Distrb::init) is a SEQUENTIAL
// double-precision running sum over the float entries, rounded to float per entry.  A parallel scan gives those bits only where every partial sum is exact in double, whatever the
// order: the entries are multiples of 2^(emin - 150) below 2^(emax - 126) (emin / emax: smallest / largest biased exponent of a non-zero entry), so a sum of n of them is such a
// multiple below 2^(emax - 126 + ceil(log2 n)) - exact when (emax - emin + 1) + 24 + ceil(log2 n) <= 53.  The kernels that write the entries record the exponent range
// (cdf_note_exponent), k_cdf_bases checks the bound ON THE DEVICE; where it does not hold (or an entry is negative, infinite or NaN) the sequential form runs on the HOST, over the
// lengths that came back for the float sum anyway, and the cmf goes up (4 B per entry) - a single lane walking the table on the device was 50 x slower than that.
__device__ inline void cdf_note_exponent(int *range, float x) {
    const unsigned u = __float_as_uint(x);
    if (u == 0u) return;                                     // (+0 adds nothing)
    int e = (int) ((u >> 23) & 0xffu);
    if (e == 0) e = 1;                                       // (subnormals: multiples of 2^-149, as the entries of exponent 1)
    if ((u >> 31) != 0u) e = 255;                            // (a negative entry: the host refuses it; here it only rules the scan out)
    atomicMin(&range[0], e); atomicMax(&range[1], e);        // (integers: the result does not depend on the order)
}
__device__ inline bool cdf_scan_is_exact(const int *range, int n) {
    const int emin = range[0], emax = range[1];
    if (emax == 0) return true;                              // every entry is zero
    if (emax >= 255) return false;
    int lg = 0;
    while ((1ll << lg) < (long long) n) ++lg;
    return (emax - emin + 1) + 24 + lg <= 53;
}
__device__ inline double cdf_wave_inclusive(double x, int lane) {
    for (int off = 1; off < 64; off <<= 1) { const double y = __shfl_up(x, off); if (lane >= off) x += y; }
    return x;
}
// sums of 256 entries each
__global__ void __launch_bounds__(256) k_cdf_partial(const float *__restrict__ pmf, int n, double *__restrict__ bsum) {
    __shared__ double ws[4];
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double x = cdf_wave_inclusive(i < n ? (double) pmf[i] : 0.0, lane);
    if (lane == 63) ws[wave] = x;
    __syncthreads();
    if (threadIdx.x == 0) bsum[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}
// one workgroup: the bound; exact -> exclusive scan of the block sums in place, *mode = 1; otherwise *mode = 2 and nothing is written
__global__ void __launch_bounds__(256) k_cdf_bases(double *__restrict__ bsum, int nb, const int *__restrict__ range, int n, int *__restrict__ mode) {
    __shared__ double ws[4];
    __shared__ double carry;
    const bool exact = cdf_scan_is_exact(range, n);           // (uniform: every lane reads the same two words)
    if (!exact) { if (threadIdx.x == 0) *mode = 2; return; }       // (the caller runs the sequential form: one lane over 26 000 entries took 1.6 ms here, the host 0.03 ms)
    if (threadIdx.x == 0) { carry = 0.0; *mode = 1; }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int begin = 0; begin < nb; begin += 256) {
        const int i = begin + threadIdx.x;
        const double c = i < nb ? bsum[i] : 0.0;
        const double x = cdf_wave_inclusive(c, lane);
        if (lane == 63) ws[wave] = x;
        __syncthreads();
        double before = carry;
        for (int w = 0; w < wave; ++w) before += ws[w];
        if (i < nb) bsum[i] = before + x - c;
        __syncthreads();
        if (threadIdx.x == 255) carry = before + x;
        __syncthreads();
    }
}
__global__ void __launch_bounds__(256) k_cdf_apply(const float *__restrict__ pmf, float *__restrict__ cmf, const double *__restrict__ bsum, const int *__restrict__ mode, int n) {
    __shared__ double ws[4];
    if (*mode != 1) return;                                   // (the sequential form writes the cmf)
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double x = cdf_wave_inclusive(i < n ? (double) pmf[i] : 0.0, lane);
    if (lane == 63) ws[wave] = x;
    __syncthreads();
    double before = bsum[blockIdx.x];
    for (int w = 0; w < wave; ++w) before += ws[w];
    if (i < n) cmf[i] = (float) (before + x);
}
// the guide table of scene_obj.h::build_cdf_guide, one bucket bound per thread, in the same float arithmetic
__global__ void k_cdf_guide(const float *__restrict__ cmf, int size, float sum, int nb, int *__restrict__ guide) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k > nb) return;
    const float s = ((float) k / (float) nb) * sum;
    int lo = 0, len = size - 1;                               // first i in [0, size - 1) with !(cmf[i] < s), else size - 1
    while (len > 0) {
        const int half = len >> 1;
        if (cmf[lo + half] < s) { lo += half + 1; len -= half + 1; } else len = half;
    }
    guide[k] = lo;
}
// buckets build_cdf_guide gives a table of `size` entries (0: no table)
static int cdf_guide_buckets(int size, int per_bucket) {
    if (size < 256) return 0;
    int nb = 1;
    while (nb * per_bucket <= size) nb <<= 1;
    return nb;
}
// cmf[0..n) and the guide table of pmf[0..n) (device pointers; host_pmf: the same entries on the host; sum: their sequential float sum); scratch sized for `cap` entries.
// *mode: 1 parallel scan on the device, 2 sequential form on the host (its cmf is sent: counted in info.bytes_uploaded and `bytes`)
static int cdf_on_device(psdr_hip_scene *sc, const float *pmf, float *cmf, const float *host_pmf, int n, int cap, float sum, const int *range, const std::string &guide_key, const int *&guide,
                         int &guide_n, int *mode, psdr_update_info &info, int64_t &bytes) {
    guide = nullptr; guide_n = 0;
    const int nb = (n + 255) / 256, nb_cap = (std::max(cap, n) + 255) / 256;
    DevBuf &bs = sc->buf("cdf.bsum"), &md = sc->buf("cdf.mode");
    if (bs.bytes < sizeof(double) * (size_t) (nb_cap + 1) && bs.ensure(sizeof(double) * (size_t) (nb_cap + 1))) return 1;
    if (md.ensure(sizeof(int))) return 1;
    hipLaunchKernelGGL(k_cdf_partial, dim3((unsigned) nb), dim3(256), 0, nullptr, pmf, n, (double *) bs.p);
    hipLaunchKernelGGL(k_cdf_bases, dim3(1), dim3(256), 0, nullptr, (double *) bs.p, nb, range, n, (int *) md.p);
    hipLaunchKernelGGL(k_cdf_apply, dim3((unsigned) nb), dim3(256), 0, nullptr, pmf, cmf, (const double *) bs.p, (const int *) md.p, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(mode, md.p, sizeof(int), hipMemcpyDeviceToHost));
    if (*mode != 1) {
        std::vector<float> c((size_t) n);
        double acc = 0.0;
        for (int i = 0; i < n; ++i) { acc += (double) host_pmf[i]; c[(size_t) i] = (float) acc; }
        HIPCHK(hipMemcpy(cmf, c.data(), sizeof(float) * (size_t) n, hipMemcpyHostToDevice));
        info.bytes_uploaded += (int64_t) (4 * (size_t) n); bytes += (int64_t) (4 * (size_t) n);
        *mode = 2;
    }
    const int gb = cdf_guide_buckets(n, 4);
    if (gb > 0) {
        DevBuf &g = sc->buf(guide_key);
        const size_t want = sizeof(int) * (size_t) (cdf_guide_buckets(std::max(cap, n), 4) + 1);          // (sized for the capacity: the table of a later selection fits)
        if (g.bytes < sizeof(int) * (size_t) (gb + 1) && g.ensure(want)) return 1;
        hipLaunchKernelGGL(k_cdf_guide, dim3((unsigned) ((gb + 1 + 255) / 256)), dim3(256), 0, nullptr, (const float *) cmf, n, sum, gb, (int *) g.p);
        HIPCHK(hipGetLastError());
        guide = g.as<int>(); guide_n = gb;
    }
    return 0;
}

// PMF entries of the secondary-edge distribution (Scene::m_sec_edge_distrb, reference src/scene/scene.cpp:559-563): the edge lengths, in the host's explicit-fmaf arithmetic
// (edge_select.h::edge_length3).  edges: the [ne][6] list of k_geo_sec
__global__ void k_se_length(const int *__restrict__ edges, const float *__restrict__ world, float *__restrict__ pmf, int *__restrict__ range, int ne) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= ne) return;
    const float *a = world + 6 * (size_t) edges[6 * (size_t) r], *b = world + 6 * (size_t) edges[6 * (size_t) r + 1];
    const float pa[3] = {a[0], a[2], a[4]}, pb[3] = {b[0], b[2], b[4]};
    const float len = psdr_host::edge_length3(pa, pb);
    pmf[r] = len;
    cdf_note_exponent(range, len);
}
__global__ void k_cdf_range_reset(int *__restrict__ range) { range[0] = 0x7fffffff; range[1] = 0; }

struct PeEdge { int v0, v1, f0, f1, mf; };          // global vertex / face ids (f1 = -1: boundary), mesh index << 3 | bit 0 uv seam | bit 1 has uv | bit 2 face normals
struct PeMesh { int mesh_id, v_off; };              // per mesh: Mesh id and first global vertex (the ids of a kept edge are mesh-local)
struct PeCam { float w2s[16], d_w2s[16], pos[3]; int pe_off, pecdf_off; };

__device__ inline bool pe_keep_edge(const PeEdge &e, const PeCam &cam, const int *__restrict__ faces, const float *__restrict__ world, const float *__restrict__ fnrm, const float *__restrict__ farea) {
    float t0[6], t1[6];
    auto face = [&](int f, float *t) {
        const float *p = world + 6 * (size_t) faces[3 * (size_t) f], *n = fnrm + 6 * (size_t) f;
        const float a2 = farea[2 * (size_t) f];
        t[0] = p[0]; t[1] = p[2]; t[2] = p[4];
        t[3] = psdr_host::canon_nan(n[0] / a2); t[4] = psdr_host::canon_nan(n[2] / a2); t[5] = psdr_host::canon_nan(n[4] / a2);
    };
    face(e.f0, t0);
    if (e.f1 >= 0) face(e.f1, t1);
    return psdr_host::edge_keep(cam.pos, t0, e.f1 >= 0 ? t1 : nullptr, (e.mf & 4) != 0, (e.mf & 2) != 0, (e.mf & 1) != 0);
}

__global__ void __launch_bounds__(256) k_pe_flags(const PeEdge *__restrict__ edges, PeCam cam, const int *__restrict__ faces, const float *__restrict__ world, const float *__restrict__ fnrm,
                                                  const float *__restrict__ farea, unsigned char *__restrict__ flags, int *__restrict__ block_count, int ne) {
    __shared__ int wc[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool keep = i < ne && pe_keep_edge(edges[i], cam, faces, world, fnrm, farea);
    if (i < ne) flags[i] = keep ? 1 : 0;
    const unsigned long long b = __ballot(keep);
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) block_count[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// counts[0..nb) -> exclusive bases in place, counts[nb] = the total
__global__ void __launch_bounds__(256) k_pe_bases(int *__restrict__ counts, int nb, int *__restrict__ range) {
    __shared__ int wsum[4];
    __shared__ int carry;
    if (threadIdx.x == 0) { carry = 0; range[0] = 0x7fffffff; range[1] = 0; }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int begin = 0; begin < nb; begin += 256) {
        const int i = begin + threadIdx.x;
        const int c = i < nb ? counts[i] : 0;
        int x = c;                                          // inclusive scan inside the wave
        for (int off = 1; off < 64; off <<= 1) { const int y = __shfl_up(x, off); if (lane >= off) x += y; }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        int before = carry;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        if (i < nb) counts[i] = before + x - c;
        __syncthreads();
        if (threadIdx.x == 255) carry = before + x;
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[nb] = carry;
}

__global__ void __launch_bounds__(256) k_pe_rows(const PeEdge *__restrict__ edges, const PeMesh *__restrict__ meshes, PeCam cam, const float *__restrict__ world, const unsigned char *__restrict__ flags, const int *__restrict__ bases,
                                                 int *__restrict__ range, float4 *__restrict__ blob, int *__restrict__ ids, int ne) {
    __shared__ int wc[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool keep = i < ne && flags[i] != 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(keep);
    if (lane == 0) wc[wave] = __popcll(b);
    __syncthreads();
    if (!keep) return;
    int r = bases[blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) r += wc[w];
    const PeEdge e = edges[i];
    DM4 w2s;
    for (int a = 0; a < 4; ++a) for (int c = 0; c < 4; ++c) w2s.m[a][c] = DF(cam.w2s[4 * a + c], cam.d_w2s[4 * a + c]);
    const psdr_host::PrimEdgeRow row = psdr_host::edge_row(w2s, geo_ld(world, (size_t) e.v0), geo_ld(world, (size_t) e.v1));
    float4 *w = blob + cam.pe_off + 3 * (size_t) r;
    w[0] = make_float4(row.p0[0], row.p0[1], row.p1[0], row.p1[1]);
    w[1] = make_float4(row.d_p0[0], row.d_p0[1], row.d_p1[0], row.d_p1[1]);
    w[2] = make_float4(row.normal[0], row.normal[1], row.length, 0.f);
    reinterpret_cast<float *>(blob + cam.pecdf_off)[r] = row.length;            // pmf; the cmf follows it at [total + r] (cdf_on_device)
    const PeMesh m = meshes[e.mf >> 3];
    ids[3 * (size_t) r] = m.mesh_id; ids[3 * (size_t) r + 1] = e.v0 - m.v_off; ids[3 * (size_t) r + 2] = e.v1 - m.v_off;
    cdf_note_exponent(range, row.length);
}

// total number of edges of the meshes with edges: what every sensor's edge arrays are sized to under psdr_hip_scene_update_edges
static size_t pe_capacity(const psdr_scene_snapshot *s, const psdr_edge_topology *topo) {
    size_t cap = 0;
    if (s->sppe > 0) for (int i = 0; i < s->n_meshes; ++i) if (topo[i].enabled) cap += (size_t) std::max(0, topo[i].n_edges);
    return cap;
}

// the edge list the kernels read: sent when a mesh's topology version (or a count / flag it is laid out by) changed; -> 1 on error
static int pe_sync_topology(psdr_hip_scene *sc, const psdr_scene_snapshot *s, const psdr_edge_topology *topo, int64_t &edge_bytes) {
    const psdr_mesh_geometry *G = s->geometry;
    const int nm = s->n_meshes;
    std::vector<uint64_t> key;
    size_t NE = 0;
    for (int i = 0; i < nm; ++i) {
        const bool on = s->sppe > 0 && topo[i].enabled && topo[i].n_edges > 0;
        for (uint64_t x : {topo[i].topology_version, (uint64_t) (on ? topo[i].n_edges : 0), (uint64_t) G[i].n_vertices, (uint64_t) G[i].n_faces, (uint64_t) G[i].mesh_id,
                           (uint64_t) ((G[i].use_face_normals ? 4 : 0) | (topo[i].uv_seam ? 2 : 0))}) key.push_back(x);
        if (on) NE += (size_t) topo[i].n_edges;
    }
    if (key == sc->pe_topo_key && sc->pe_n == (int) NE) return 0;
    sc->pe_topo_key.clear();
    std::vector<PeEdge> ed(std::max<size_t>(1, NE));
    std::vector<PeMesh> pm((size_t) std::max(1, nm));
    size_t vo = 0, fo = 0, k = 0;
    for (int i = 0; i < nm; ++i) {
        const bool on = s->sppe > 0 && topo[i].enabled && topo[i].n_edges > 0;
        if (on && !topo[i].edges) return fail("psdr_edge_topology[" + std::to_string(i) + "]: edges is null");
        const int nv = G[i].n_vertices, nf = G[i].n_faces;
        for (int e = 0; on && e < topo[i].n_edges; ++e) {
            const int32_t *q = topo[i].edges + 5 * (size_t) e;            // v0 v1 f0 f1 opp
            if (q[0] < 0 || q[0] >= nv || q[1] < 0 || q[1] >= nv || q[2] < 0 || q[2] >= nf || q[3] < -1 || q[3] >= nf)
                return fail("psdr_edge_topology[" + std::to_string(i) + "]: edge " + std::to_string(e) + " refers outside the mesh's vertices / faces");
            PeEdge &d = ed[k++];
            d.v0 = (int) vo + q[0]; d.v1 = (int) vo + q[1]; d.f0 = (int) fo + q[2]; d.f1 = q[3] >= 0 ? (int) fo + q[3] : -1;
            d.mf = (i << 3) | (topo[i].uv_seam && topo[i].uv_seam[e] ? 1 : 0) | (topo[i].uv_seam ? 2 : 0) | (G[i].use_face_normals ? 4 : 0);
        }
        pm[(size_t) i] = PeMesh{G[i].mesh_id, (int) vo};
        vo += (size_t) nv; fo += (size_t) nf;
    }
    const size_t nb = (NE + 255) / 256;
    DevBuf &be = sc->buf("pe.edges");
    if (be.ensure(sizeof(PeEdge) * ed.size())) return 1;
    HIPCHK(hipMemcpy(be.p, ed.data(), sizeof(PeEdge) * ed.size(), hipMemcpyHostToDevice));
    DevBuf &bm = sc->buf("pe.meshes");
    if (bm.ensure(sizeof(PeMesh) * pm.size())) return 1;
    HIPCHK(hipMemcpy(bm.p, pm.data(), sizeof(PeMesh) * pm.size(), hipMemcpyHostToDevice));
    edge_bytes += (int64_t) (sizeof(PeEdge) * ed.size() + sizeof(PeMesh) * pm.size());
    if (sc->buf("pe.flags").ensure(std::max<size_t>(1, NE)) || sc->buf("pe.block").ensure(sizeof(int) * (nb + 1)) || sc->buf("pe.ids").ensure(sizeof(int) * 3 * std::max<size_t>(1, NE)) ||
        sc->buf("pe.range").ensure(2 * sizeof(int))) return 1;
    sc->pe_n = (int) NE;
    sc->pe_topo_key = key;
    return 0;
}

// selects sensor k's primary edges on the device and completes its distribution; d.pe_off / d.pecdf_off are set.  -> 1 on error
static int primary_edges_on_device(psdr_hip_scene *sc, const psdr_sensor_rec &r, int k, SensorDev &d, psdr_update_info &info, int64_t &edge_bytes, bool &cdf_sequential) {
    const int NE = sc->pe_n;
    std::vector<int32_t> &ids = sc->pe_ids[(size_t) k];
    ids.clear();
    d.n_edges = 0; d.edge_sum = 0.f; d.pe_guide = nullptr; d.pe_guide_n = 0;
    if (NE <= 0) return 0;
    PeCam cam;
    std::memcpy(cam.w2s, r.world_to_sample, 64); std::memcpy(cam.d_w2s, r.d_world_to_sample, 64);
    for (int q = 0; q < 3; ++q) cam.pos[q] = r.cam_pos[q];
    cam.pe_off = d.pe_off; cam.pecdf_off = d.pecdf_off;
    const int nb = (NE + 255) / 256;
    const PeEdge *edges = sc->buf("pe.edges").as<PeEdge>();
    const float *world = sc->buf("geo.world").as<float>(), *fnrm = sc->buf("geo.fnrm").as<float>(), *farea = sc->buf("geo.farea").as<float>();
    unsigned char *flags = (unsigned char *) sc->buf("pe.flags").p;
    int *block = (int *) sc->buf("pe.block").p, *dids = (int *) sc->buf("pe.ids").p;
    hipLaunchKernelGGL(k_pe_flags, dim3((unsigned) nb), dim3(256), 0, nullptr, edges, cam, sc->buf("geo.faces").as<int>(), world, fnrm, farea, flags, block, NE);
    int *range = (int *) sc->buf("pe.range").p;
    hipLaunchKernelGGL(k_pe_bases, dim3(1), dim3(256), 0, nullptr, block, nb, range);
    hipLaunchKernelGGL(k_pe_rows, dim3((unsigned) nb), dim3(256), 0, nullptr, edges, sc->buf("pe.meshes").as<PeMesh>(), cam, world, (const unsigned char *) flags, (const int *) block, range, (float4 *) sc->blob.p, dids, NE);
    HIPCHK(hipGetLastError());
    int total = 0;
    HIPCHK(hipMemcpy(&total, block + nb, sizeof(int), hipMemcpyDeviceToHost));
    if (total < 0 || total > NE) return fail("primary edges on the device: kept count out of range");
    if (total == 0) return 0;
    std::vector<float> len((size_t) total);
    ids.resize(3 * (size_t) total);
    float *pmf = (float *) sc->blob.p + 4 * (size_t) d.pecdf_off;
    HIPCHK(hipMemcpy(len.data(), pmf, sizeof(float) * (size_t) total, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ids.data(), dids, sizeof(int) * 3 * (size_t) total, hipMemcpyDeviceToHost));
    // DiscreteDistribution::init (reference src/core/pmf.cpp:6-15): `sum` is a sequential FLOAT sum - from the lengths that came back (4 B per kept edge, device to host); the
    // cmf and its search table are made on the device (cdf_on_device): nothing proportional to the edge count goes up
    float sum = 0.f;
    for (int i = 0; i < total; ++i) sum += len[(size_t) i];
    d.n_edges = total; d.edge_sum = sum;
    int mode = 0;
    if (cdf_on_device(sc, pmf, pmf + total, len.data(), total, NE, sum, range, "sensor." + std::to_string(k) + ".guide", d.pe_guide, d.pe_guide_n, &mode, info, edge_bytes)) return 1;
    if (mode == 2) cdf_sequential = true;
    return 0;
}

struct WordRange { size_t b, e; };
// psdr_hip_scene_update_edges: per mesh the edge topology, per sensor where its primary edges come from (PSDR_EDGES_*)
struct EdgeRequest { const psdr_edge_topology *topo; const int32_t *mode; };

// ---------------------------------------------------------------------------------------------------------------------------
// FROM A SNAPSHOT TO A RENDERABLE DEVICE SCENE: scene_sync (below) is the list of SceneSync's steps.  Up to and including plan_layout nothing of the handle
// is written except by tree_build, and every step that can answer PSDR_HIP_NEED_ROWS there runs only when no tree is built: such an answer leaves the handle as it was.
// commit_tables is the first write of sc->T / sc->E; the three later PSDR_HIP_NEED_ROWS answers (geometry: they need what geometry_on_device found) go
// through SceneSync::need_rows, which puts both back.  Any other non-zero return leaves old and new sections mixed: the caller poisons the handle (update_entry).
static int sync_validate(const psdr_scene_snapshot *s) {
    if (s->tris.n_triangles <= 0) return fail("Missing meshes!");
    if (s->n_sensors <= 0) return fail("Missing sensor!");
    for (int i = 0; i < s->n_bsdfs; ++i) {
        const psdr_bsdf_rec &b = s->bsdfs[i];
        if (b.type < 0 || b.type > 5) return fail("Unknown BSDF type!");
        if (b.type == 5 && (b.nested_bsdf < 0 || b.nested_bsdf >= s->n_bsdfs || s->bsdfs[b.nested_bsdf].type == 5)) return fail("NormalMap: invalid nested BSDF");
    }
    return 0;
}

// the search table of a distribution (scene_obj.h::build_cdf_guide), built on the host and sent under `key`: ptr / count (none: NULL / 0), its bytes added to *bytes
static int sync_guide(psdr_hip_scene *sc, const std::string &key, const float *cmf, int n, float sum, int per_bucket, const int *&ptr, int &count, int64_t *bytes, psdr_update_info &info) {
    ptr = nullptr; count = 0;
    if (n <= 0 || !cmf) return 0;
    std::vector<int> guide;
    build_cdf_guide(cmf, n, sum, guide, per_bucket);
    if (guide.empty()) return 0;
    if (sync_named(sc, key, guide.data(), guide.size() * sizeof(int), false, ptr, info)) return 1;
    count = (int) guide.size() - 1;
    if (bytes) *bytes += (int64_t) (guide.size() * sizeof(int));
    return 0;
}

struct SceneSync {
    psdr_hip_scene *sc;
    const psdr_scene_snapshot *s;
    const EdgeRequest *ereq;
    bool fresh;                          // the handle is new
    const psdr_triangles &tr;
    SceneTables &T;                      // sc->T / sc->E: the old tables up to commit_tables, then this snapshot's
    SecEdgeTables &E;
    // what the caller vouches for (PSDR_SAME_* relative to the snapshot of the previous create / update of this handle; all false when a tree is built)
    bool same_tris = false, same_tan = false, same_sec = false, same_prim = false, same_env = false, same_env_tan = false, same_bitmaps = false;
    bool build = false, rows_valid = true, uses_bvh = false, has_tan = false;
    bool geo = false;                    // the triangle sections are rewritten: moved triangles, or tangent arrays gained or lost (every section behind them shifts)
    // the edge request: room per sensor, who makes the secondary-edge distribution, whether any edge section is the device's
    size_t pe_cap = 0;
    bool cap_layout = false, sec_dev_any = false, dev_edges = false;
    int env_emitter = -1;
    std::vector<float> new_nodes;
    std::vector<FilterPrim> filt;        // filter primitives of the brute-force tracer (their number depends on the geometry: coplanar neighbours become quads)
    int n_filt = 0;
    BlobLayout L;
    SceneTables Told{};
    SecEdgeTables Eold{};
    float *H = nullptr;                  // the pinned host copy of the blob
    std::vector<WordRange> dirty;        // sections of H that were written and have to be sent
    bool blob_moved = false, dev_geo = false;
    int sec_cdf_mode = 0, edge_path = 0;
    int64_t sec_bytes = 0, edge_bytes = 0;          // sec_bytes: what goes up for the secondary-edge DISTRIBUTION (pmf, cmf, search table)
    std::vector<int> tabs_to_fill;                  // sensors whose camera-ray table is made once the rows are on the device (launch_cam_tables)
    psdr_update_info info{};

    SceneSync(psdr_hip_scene *sc_, const psdr_scene_snapshot *s_, const EdgeRequest *ereq_, bool fresh_) : sc(sc_), s(s_), ereq(ereq_), fresh(fresh_), tr(s_->tris), T(sc_->T), E(sc_->E) {}
    void mark(size_t b, size_t e) { if (e > b) dirty.push_back({b, e}); }
    int need_rows() { T = Told; E = Eold; return PSDR_HIP_NEED_ROWS; }       // (the only rollback: the tables as they were)

    // build / refit / keep, what the caller vouches for, the edge request - from the snapshot, the request and the old handle alone, and what they already refuse
    int plan_request(unsigned same, bool force_build) {
        const int n = s->tris.n_triangles;
        build = fresh || force_build || n != sc->tree_tris;
        uses_bvh = n > kBruteForceMax;
        has_tan = s->tris.d_p0 != nullptr;
        // rows_valid = 0 (updates only; psdr_scene_snapshot): the caller relies on the device computing the moved meshes' rows.  Whatever needs the rows themselves - a tree to
        // build, a section that moves, a live-pixel mask to rebuild - answers PSDR_HIP_NEED_ROWS before anything has been changed
        rows_valid = fresh || s->rows_valid != 0;
        if (!rows_valid && (build || s->geometry == nullptr || n <= kBruteForceMax)) return PSDR_HIP_NEED_ROWS;
        if (build) same = 0;
        same_tris = (same & PSDR_SAME_TRIANGLES) != 0; same_tan = (same & PSDR_SAME_TRI_TANGENTS) != 0; same_sec = (same & PSDR_SAME_SEC_EDGES) != 0;
        same_prim = (same & PSDR_SAME_PRIM_EDGES) != 0; same_env = (same & PSDR_SAME_ENV_TEXELS) != 0; same_env_tan = (same & PSDR_SAME_ENV_TANGENT) != 0;
        same_bitmaps = (same & PSDR_SAME_BITMAPS) != 0;
        // (a snapshot that gains or loses its tangent arrays shifts every section behind them: treated like moved triangles)
        geo = !same_tris || (has_tan ? 1 : 0) != T.has_tangent;
        for (int i = 0; i < s->n_emitters; ++i) if (s->emitters[i].type == 1) env_emitter = i;
        // (psdr_hip_scene_update_edges: every sensor's edge arrays are sized ONCE, to the number of edges of the meshes with edges - the kept count changes from
        //  configure to configure, the sections behind it must not move)
        //  ... and a scene that has been given that size keeps it under psdr_hip_scene_update too: the two calls alternate (a configure that changes nothing about the edges takes the plain one),
        //  and a section that moved would be written and sent again
        pe_cap = ereq ? pe_capacity(s, ereq->topo) : (fresh ? 0 : sc->pe_cap);
        for (int i = 0; !ereq && i < s->n_sensors; ++i) if ((size_t) std::max(0, s->sensors[i].n_edges) > pe_cap) pe_cap = 0;
        cap_layout = ereq != nullptr || pe_cap > 0;
        // (... and the secondary-edge distribution: under that call a snapshot without sec_edges.pmf / cmf leaves the lengths and their CDF to the device)
        sec_dev_any = ereq && s->sec_edges.n_edges > 0 && s->sec_edges.pmf == nullptr;
        dev_edges = sec_dev_any;         // some sensor's edges are selected on the device or kept from an earlier selection: their host copy in H is behind
        for (int i = 0; i < s->n_sensors; ++i) {
            if (ereq && ereq->mode[i] != PSDR_EDGES_HOST) dev_edges = true;
            else if (ereq && (size_t) std::max(0, s->sensors[i].n_edges) > pe_cap) return fail("psdr_hip_scene_update_edges: a sensor carries more primary edges than the meshes have edges");
        }
        // the device selects (or keeps) primary edges only where nothing else about the scene moves - first of all the tree: refused before one is built (plan_layout
        // refuses the rest, once the layout is known)
        if (dev_edges && (fresh || build)) return PSDR_HIP_NEED_ROWS;
        return 0;
    }

    // the layout of the blob for this snapshot, and every PSDR_HIP_NEED_ROWS answer that follows from it and the old tables: sc->T / sc->E are still the old ones
    int plan_layout() {
        if (geo) build_filter_prims(tr.p0, tr.e1, tr.e2, sc->order.data(), tr.n_triangles, filt);
        n_filt = geo ? (int) filt.size() : T.n_filt;
        BlobCounts k;
        k.n_tris = tr.n_triangles; k.n_nodes = T.n_nodes; k.node_words = kNodeFloats / 4; k.has_tan = has_tan; k.n_filt = n_filt;
        k.n_meshes = s->n_meshes; k.n_bsdfs = s->n_bsdfs; k.n_emitters = s->n_emitters; k.n_face_distrb = s->n_face_distrb; k.n_sec_edges = s->sec_edges.n_edges;
        for (int i = 0; i < s->n_sensors; ++i) k.sensor_edges.push_back(s->sensors[i].n_edges);
        k.pe_cap = pe_cap; k.capped = cap_layout;
        // a section keeps its content only when the caller vouches for it AND it stays where it was
        if (!blob_layout(k, L)) return fail("scene too large for 32-bit blob offsets");
        const bool blob_fits = sc->blob.p && sc->blob.bytes >= 16 * L.words, forced_host = std::getenv("PSDR_HOST_GEOMETRY") != nullptr;
        if (dev_edges) {
            // ... the blob stays where it is (the host's copy of such a section is behind), the world vertices of every mesh are resident or about to be computed.
            // Otherwise: PSDR_HIP_NEED_ROWS, nothing changed - the caller comes back with PSDR_EDGES_HOST for every sensor
            bool ok = uses_bvh && s->geometry != nullptr && blob_fits && !forced_host;
            for (int i = 0; ok && i < s->n_sensors; ++i)
                if (ereq->mode[i] == PSDR_EDGES_KEEP)
                    ok = (size_t) i < sc->sensors.size() && sc->sensors[(size_t) i].pe_off == L.pe[(size_t) i].first && sc->sensors[(size_t) i].pecdf_off == L.pe[(size_t) i].second &&
                         sc->pe_ids.size() == (size_t) s->n_sensors;
            if (sec_dev_any) ok = ok && sec_section_kept(L, E);       // (the section stays where it is: the host's copy of it is behind)
            if (!ok) return PSDR_HIP_NEED_ROWS;
        }
        if (!rows_valid && !(blob_fits && layout_kept(L, T, E, has_tan) && env_emitter >= 0 && T.env_emitter >= 0 && !forced_host)) return PSDR_HIP_NEED_ROWS;
        return 0;
    }

    // the first write of the tables: offsets from the layout, counts and frame from the snapshot, the traversal stack's split
    void commit_tables() {
        Told = T; Eold = E;
        assign_offsets(L, T, E);
        E.sum = s->sec_edges.sum;
        T.n_filt = n_filt;
        T.n_tris = s->tris.n_triangles; T.n_meshes = s->n_meshes; T.n_bsdfs = s->n_bsdfs; T.n_emitters = s->n_emitters;
        T.n_fcdf = s->n_face_distrb; T.has_tangent = has_tan ? 1 : 0;
        T.emitter_sum = s->emitter_sum;
        T.width = s->width; T.height = s->height; T.spp = s->spp; T.sppe = s->sppe; T.sppse = s->sppse;
        T.env_emitter = env_emitter;
        // traversal stack: the first kStackLds entries of a lane in LDS, deeper ones in a per-lane global array (trav4.h);
        // scenes that are traced by brute force (<= kBruteForceMax triangles) need neither
        // kStackLdsMax + kTravRows = 40 KB per workgroup: four workgroups per CU (round 6: 12 stack rows + 2 rows of tree top, until then 8 + 6 - trav4.h).  Round 5 measured both sides of that choice on config 5 (LABNOTES): FEWER workgroups cost a lot
        // (3 per CU: +17 %, 2: +55 %), a FIFTH brings nothing (a 30 KB layout - no hit rows, 4 stack rows - lost exactly what its shorter stack costs at equal
        // occupancy), and stack rows going to the global tail cost 1.2 % (6 rows), 6.8 % (4), 9.5 % (2).
        // PSDR_STACK_LDS = 2 ... kStackLdsMax (test knob, read when a scene is created or rebuilt): fewer rows, so that small test scenes reach the global tail too
        // (tests/test_gpu_configs.py: the forked terms of a renderD against the serial call)
        int kStackLds = kStackLdsMax;
        if (const char *e = std::getenv("PSDR_STACK_LDS")) kStackLds = std::max(2, std::min(kStackLdsMax, std::atoi(e)));
        T.stack_lds = uses_bvh ? std::min(kStackLds, sc->tree_max_stack) : 0;
        T.stack_depth = uses_bvh ? T.stack_lds + kTravRows : kColdRows;   // BVH: + parked rays, best hits and the pair ring of the traversal (trav4.h); brute force: cold path state (paths.h)
    }

    // the blob: device allocation with head room, pinned host copy; the nodes of a new tree and the slot map go into the copy
    int blob() {
        const size_t w = L.words;
        const int n = T.n_tris;
        if (!sc->blob.p || sc->blob.bytes < 16 * w) {
            // (room for the sensors' edge arrays at the size psdr_hip_scene_update_edges gives them - every edge of the meshes with edges - so that the first such update does not move the blob)
            size_t reserve = 0;
            if (!ereq && uses_bvh && s->geometry && s->sppe > 0) {
                size_t ne_all = 0;
                for (int i = 0; i < s->n_meshes; ++i) ne_all += (size_t) std::max(0, s->geometry[i].n_edges);
                reserve = (size_t) s->n_sensors * (3 * ne_all + words_for_floats(2 * std::max<size_t>(1, ne_all)));
            }
            const size_t cap = 16 * (w + w / 4 + 64 + reserve);
            void *fresh_p = nullptr;
            HIPCHK(hipMalloc(&fresh_p, cap));
            if (sc->blob.p) {
                // the nodes a refit has written exist on the device only: they move with the allocation
                if (!build && uses_bvh) HIPCHK(hipMemcpy((char *) fresh_p + 16 * (size_t) T.nodes_off, (const char *) sc->blob.p + 16 * (size_t) Told.nodes_off, 16 * (size_t) (kNodeFloats / 4) * (size_t) T.n_nodes, hipMemcpyDeviceToDevice));
                HIPCHK(hipFree(sc->blob.p));
                info.reallocated++;
            }
            sc->blob.p = fresh_p; sc->blob.bytes = cap;
            blob_moved = true;
        }
        if (sc->hblob.ensure(sc->blob.bytes)) return 1;
        H = (float *) sc->hblob.p;
        if (build) {
            std::memcpy(H + 4 * (size_t) T.nodes_off, new_nodes.data(), sizeof(float) * new_nodes.size());
            mark((size_t) T.nodes_off, (size_t) T.nodes_off + new_nodes.size() / 4);
        }
        if (build || blob_moved || T.map_off != Told.map_off) {
            for (int i = 0; i < n; ++i) H[4 * (size_t) T.map_off + (size_t) i] = ibits(sc->orig2slot[(size_t) i]);
            mark((size_t) T.map_off, (size_t) T.map_off + words_for_floats((size_t) n));
        }
        return 0;
    }

    // moved meshes: their rows computed on the device (geometry_on_device above) when nothing else about the layout changed; the host then writes none of them
    int geometry() {
        const bool layout_same = !fresh && !build && !blob_moved && uses_bvh && layout_kept(L, Told, Eold, has_tan);
        const bool forced_host = std::getenv("PSDR_HOST_GEOMETRY") != nullptr;         // test knob, read per call: the host writes the rows (what psdr_hip_scene_check_rows compares with)
        if (layout_same && !forced_host && s->geometry != nullptr && (geo || !same_tan || !same_sec)) {
            if (geometry_on_device(sc, s, geo, has_tan && !same_tan, !same_sec, info, dev_geo)) return 1;
            if (!dev_geo && !rows_valid) return need_rows();
        }
        // (triangles the host writes below leave the device's world vertices behind: the next geometry_on_device recomputes every mesh)
        if (!dev_geo && (geo || !same_tan)) sc->geo_world_current = false;
        if (dev_edges && !sc->geo_world_current) return need_rows();
        if (sec_dev_any && !same_sec && !dev_geo) return need_rows();
        return 0;
    }

    // (the pinned host copy of a section the device wrote is behind the device's; it is only ever sent after the host has rewritten the whole section from the snapshot -
    //  a change of the section itself, or a moved allocation, both of which write it first)
    void tri_rows() {
        const size_t n = (size_t) tr.n_triangles;
        if (!dev_geo && (geo || blob_moved || T.trav_off != Told.trav_off || T.shade_off != Told.shade_off)) {
            parallel_for(n, 8192, [&](size_t b0, size_t e0) {
                for (size_t slot = b0; slot < e0; ++slot)
                    pack_tri_rows(tr, (size_t) sc->order[slot], H + 4 * ((size_t) T.trav_off + kTravWords * slot), H + 4 * ((size_t) T.shade_off + kShadeWords * slot));
            });
            mark((size_t) T.trav_off, (size_t) T.trav_off + (kTravWords + kShadeWords) * n);
        }
        if (has_tan && !dev_geo && (!same_tan || blob_moved || T.tan_off != Told.tan_off || !Told.has_tangent)) {
            parallel_for(n, 8192, [&](size_t b0, size_t e0) {
                for (size_t slot = b0; slot < e0; ++slot) pack_tan_row(tr, (size_t) sc->order[slot], H + 4 * ((size_t) T.tan_off + kTanWords * slot));
            });
            mark((size_t) T.tan_off, (size_t) T.tan_off + kTanWords * n);
        }
    }

    // filter primitives and bounding sphere of the brute-force tracer
    void filter() {
        const int n = tr.n_triangles;
        if (geo && uses_bvh) {
            // (the bounding sphere and the filter primitives belong to the brute-force tracer, scene_dev.h::trace2: a BVH scene has neither - and the serial pass over its
            //  triangles' vertices was 0.5 ms of every moved-vertex update of config 5)
            T.center[0] = T.center[1] = T.center[2] = 0.f; T.radius = 0.f; T.filt_kmax = 0.f; T.filt_hasb[0] = T.filt_hasb[1] = 0u;
        } else if (geo) {
            // bounding sphere of the scene (for the absolute slack of the quad filter)
            double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
            for (int i = 0; i < n; ++i)
                for (int v = 0; v < 3; ++v)
                    for (int k = 0; k < 3; ++k) {
                        const double x = (double) tr.p0[3 * (size_t) i + k] + (v == 1 ? (double) tr.e1[3 * (size_t) i + k] : v == 2 ? (double) tr.e2[3 * (size_t) i + k] : 0.0);
                        lo[k] = std::min(lo[k], x); hi[k] = std::max(hi[k], x);
                    }
            double r2 = 0.0;
            for (int k = 0; k < 3; ++k) { T.center[k] = (float) (0.5 * (lo[k] + hi[k])); r2 += 0.25 * (hi[k] - lo[k]) * (hi[k] - lo[k]); }
            T.radius = (float) (std::sqrt(r2) * 1.0001);
            T.filt_kmax = 0.f;
            T.filt_hasb[0] = T.filt_hasb[1] = 0u;
            for (size_t i = 0; i < filt.size(); ++i) {
                // dot-product form of the filter (scene_dev.h::trace2): with oc = o - centre, m = oc x d and p = p0 - centre
                //   u-numerator = m.e2 + d.(p x e2)   v-numerator = d.(e1 x p) - m.e1   -det = d.(e1 x e2)   t-numerator = oc.(e1 x e2) - p.(e1 x e2)
                const FilterPrim &f = filt[i];
                const size_t fw = T.filt_off + 6 * i;
                {
                    const size_t base = i & ~(size_t) 31, cnt = std::min<size_t>(32, filt.size() - base);
                    if (f.slot_b >= 0) T.filt_hasb[i >> 5] |= 1u << (cnt - 1 - (i - base));
                }
                const double p[3] = {(double) f.p0[0] - (double) T.center[0], (double) f.p0[1] - (double) T.center[1], (double) f.p0[2] - (double) T.center[2]};
                const double e1[3] = {f.e1[0], f.e1[1], f.e1[2]}, e2[3] = {f.e2[0], f.e2[1], f.e2[2]};
                auto crs = [](const double *a, const double *b, double *c) { c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0]; };
                double A[3], B[3], N[3];
                crs(p, e2, A); crs(e1, p, B); crs(e1, e2, N);
                const double npn = -(p[0] * N[0] + p[1] * N[1] + p[2] * N[2]);
                const double K = std::max({std::sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]), std::sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]), (double) f.k16 * 32768.0});
                T.filt_kmax = std::max(T.filt_kmax, (float) (K * 1.0001));
                put4(H, fw, f.e2[0], f.e2[1], f.e2[2], (float) A[0]);
                put4(H, fw + 1, (float) A[1], (float) A[2], f.e1[0], f.e1[1]);
                put4(H, fw + 2, f.e1[2], (float) B[0], (float) B[1], (float) B[2]);
                put4(H, fw + 3, (float) N[0], (float) N[1], (float) N[2], (float) npn);
                put4(H, fw + 4, f.umax, f.vmax, f.smax, f.da);
                put4(H, fw + 5, f.db, f.da + f.db, (float) (K * (1.0001 / 32768.0)), ibits(f.slot_a | ((f.slot_b < 0 ? 0xff : f.slot_b) << 8)));
            }
            mark((size_t) T.filt_off, (size_t) T.filt_off + 6 * filt.size());
        } else if (blob_moved) mark((size_t) T.filt_off, (size_t) T.filt_off + 6 * (size_t) T.n_filt);       // (same triangles: same offset, the host copy is current)
    }

    // the small tables - mesh, BSDF and emitter records, emitter and face distributions: always written
    void small_tables() {
        std::memset(H + 4 * L.small_begin, 0, 16 * (L.small_end - L.small_begin));
        for (int i = 0; i < s->n_meshes; ++i) {
            const psdr_mesh_rec &m = s->meshes[i];
            put4(H, T.mesh_off + 2 * (size_t) i, ibits(m.bsdf_id), ibits(m.emitter_id), ibits(m.face_offset), ibits(m.n_faces));
            put4(H, T.mesh_off + 2 * (size_t) i + 1, m.inv_total_area, ibits(m.distrb_offset), m.distrb_sum, 0.f);
        }
        sc->simple_mats = true; sc->has_nmap = false;
        for (int i = 0; i < s->n_bsdfs; ++i) {
            const psdr_bsdf_rec &b = s->bsdfs[i];
            // (a NormalMap, type 5, is its nested BSDF seen through the map: the nested record is an entry of its own and decides)
            if (b.type == 5) sc->has_nmap = true;
            put4(H, T.bsdf_off + 2 * (size_t) i, b.reflectance[0], b.reflectance[1], b.reflectance[2], ibits((b.two_sided ? 1 : 0) | (b.tex_data ? 2 : 0) | (b.type == 1 ? 4 : 0) | (b.type == 2 ? 8 : 0) | (b.type == 3 ? 16 : 0) | (b.spec_tex_data ? 32 : 0) | (b.rough_tex_data ? 64 : 0) | (b.type == 4 ? 128 : 0) | (b.type == 5 ? 256 : 0)));
            put4(H, T.bsdf_off + 2 * (size_t) i + 1, b.d_reflectance[0], b.d_reflectance[1], b.d_reflectance[2], ibits(b.type == 5 ? b.nested_bsdf : -1));
        }
        for (int i = 0; i < s->n_emitters; ++i) {
            const psdr_emitter_rec &e = s->emitters[i];
            put4(H, T.emit_off + 2 * (size_t) i, e.radiance[0], e.radiance[1], e.radiance[2], e.sampling_weight);
            put4(H, T.emit_off + 2 * (size_t) i + 1, e.d_radiance[0], e.d_radiance[1], e.d_radiance[2], ibits(e.mesh_id));
            pack_distrb(H + 4 * (size_t) T.ecdf_off, (size_t) s->n_emitters, (size_t) i, s->emitter_pmf ? s->emitter_pmf[i] : 1.f, s->emitter_cmf ? s->emitter_cmf[i] : 1.f);
        }
        for (int i = 0; i < s->n_face_distrb; ++i) pack_distrb(H + 4 * (size_t) T.fcdf_off, (size_t) s->n_face_distrb, (size_t) i, s->face_pmf[i], s->face_cmf[i]);
        mark(L.small_begin, L.small_end);
    }

    // secondary edges: rows and distribution from the host, rows from the device and the distribution from the host, or both from the device
    int sec_edges() {
        const psdr_sec_edges &se = s->sec_edges;
        const bool write_sec = !same_sec || blob_moved || !sec_section_kept(L, Eold);
        if (sec_dev_any && write_sec && !dev_geo) return fail("psdr_hip_scene_update_edges: no secondary-edge distribution in the snapshot and none to compute");
        if (sec_dev_any && !write_sec) E.sum = Eold.sum;               // (the device's distribution stands: its sum is the one it was given then)
        if (write_sec && se.n_edges > 0 && dev_geo && sec_dev_any) {
            // the rows are the device's, and so is the distribution over them: lengths, then the cmf and its search table (cdf_on_device); the lengths come back for the float sum
            const int ne = se.n_edges;
            DevBuf &rg = sc->buf("sec.range");
            if (rg.ensure(2 * sizeof(int))) return 1;
            float *pmf = (float *) sc->blob.p + 4 * (size_t) E.cdf_off;
            hipLaunchKernelGGL(k_cdf_range_reset, dim3(1), dim3(1), 0, nullptr, (int *) rg.p);
            hipLaunchKernelGGL(k_se_length, dim3((unsigned) ((ne + 255) / 256)), dim3(256), 0, nullptr, sc->buf("geo.edges").as<int>(), sc->buf("geo.world").as<float>(), pmf, (int *) rg.p, ne);
            HIPCHK(hipGetLastError());
            std::vector<float> len((size_t) ne);
            HIPCHK(hipMemcpy(len.data(), pmf, sizeof(float) * (size_t) ne, hipMemcpyDeviceToHost));
            float sum = 0.f;
            for (int i = 0; i < ne; ++i) sum += len[(size_t) i];
            E.sum = sum;
            if (cdf_on_device(sc, pmf, pmf + ne, len.data(), ne, ne, sum, (const int *) rg.p, "sec.guide", E.guide, E.guide_n, &sec_cdf_mode, info, sec_bytes)) return 1;
        } else if (write_sec && se.n_edges > 0 && dev_geo) {
            // (the rows are the device's; the distribution over the edges - a sequential float prefix sum - comes from the host)
            std::memcpy(H + 4 * (size_t) E.cdf_off, se.pmf, sizeof(float) * (size_t) se.n_edges);
            std::memcpy(H + 4 * (size_t) E.cdf_off + (size_t) se.n_edges, se.cmf, sizeof(float) * (size_t) se.n_edges);
            mark((size_t) E.cdf_off, L.sec_end);
            sec_bytes += (int64_t) (8 * (size_t) se.n_edges);
        } else if (write_sec && se.n_edges > 0) {
            parallel_for((size_t) se.n_edges, 8192, [&](size_t b0, size_t e0) {
                for (size_t i = b0; i < e0; ++i) {
                    pack_sec_row(se, i, H + 4 * ((size_t) E.off + kSecWords * i));
                    pack_distrb(H + 4 * (size_t) E.cdf_off, (size_t) se.n_edges, i, se.pmf[i], se.cmf[i]);
                }
            });
            mark((size_t) E.off, L.sec_end);
            sec_bytes += (int64_t) (8 * (size_t) se.n_edges);
        }
        if (write_sec && sec_cdf_mode != 0) return 0;              // (cdf_on_device has made the table)
        if (!write_sec) { E.guide = Eold.guide; E.guide_n = Eold.guide_n; return 0; }
        // every sample of the secondary-edge term starts with this search (17 dependent loads for config 5's 122 885 edges)
        return sync_guide(sc, "sec.guide", se.cmf, se.n_edges, se.sum, 4, E.guide, E.guide_n, &sec_bytes, info);
    }

    // sensor k: matrices, primary edges (the host's arrays, selected on the device, or kept), live-pixel mask.  od: the sensor as it was (NULL: there was none)
    int sensor(int k, const SensorDev *od, const std::vector<float> &w2s_old) {
        const psdr_sensor_rec &r = s->sensors[k];
        SensorDev &d = sc->sensors[(size_t) k];
        std::memcpy(d.sample_to_camera.m, r.sample_to_camera, 64); std::memcpy(d.to_world.m, r.to_world, 64);
        std::memcpy(d.d_to_world.m, r.d_to_world, 64); std::memcpy(d.world_to_sample.m, r.world_to_sample, 64);
        std::memcpy(d.d_world_to_sample.m, r.d_world_to_sample, 64);
        for (int q = 0; q < 3; ++q) { d.cam_pos[q] = r.cam_pos[q]; d.cam_dir[q] = r.cam_dir[q]; }
        d.inv_area = r.inv_area; d.n_edges = r.n_edges; d.edge_sum = r.edge_sum; d.ortho = r.orthographic;
        d.pe_off = L.pe[(size_t) k].first; d.pecdf_off = L.pe[(size_t) k].second;
        const int pe_mode = ereq ? ereq->mode[k] : PSDR_EDGES_HOST;
        // (a sensor without edges before and after, where it was: nothing to write)
        const bool still_empty = r.n_edges <= 0 && od && od->n_edges <= 0 && !blob_moved && od->pe_off == d.pe_off && od->pecdf_off == d.pecdf_off;
        const bool write_pe = pe_mode == PSDR_EDGES_HOST && !still_empty && (!same_prim || blob_moved || !od || od->pe_off != d.pe_off || od->pecdf_off != d.pecdf_off || od->n_edges != d.n_edges);
        if (pe_mode == PSDR_EDGES_DEVICE) {
            bool sequential = false;
            if (primary_edges_on_device(sc, r, k, d, info, edge_bytes, sequential)) return 1;
            edge_path = std::max(edge_path, sequential ? 2 : 1);
        } else if (pe_mode == PSDR_EDGES_KEEP) {
            d.n_edges = od->n_edges; d.edge_sum = od->edge_sum; d.pe_guide = od->pe_guide; d.pe_guide_n = od->pe_guide_n;
        } else if (write_pe) {
            const size_t ne = (size_t) std::max(0, r.n_edges);
            sc->pe_ids[(size_t) k].clear();
            edge_bytes += (int64_t) (16 * (kPeWords * ne + words_for_floats(2 * (size_t) std::max(1, r.n_edges))));
            parallel_for(ne, 8192, [&](size_t ib, size_t ie) {
                for (size_t i = ib; i < ie; ++i) {
                    pack_pe_row(r, i, H + 4 * ((size_t) d.pe_off + kPeWords * i));
                    pack_distrb(H + 4 * (size_t) d.pecdf_off, ne, i, r.edge_pmf[i], r.edge_cmf[i]);
                }
            });
            // (two ranges: under psdr_hip_scene_update_edges the section has room for every edge and the CDF starts behind that room)
            mark((size_t) d.pe_off, (size_t) d.pe_off + kPeWords * ne);
            mark((size_t) d.pecdf_off, (size_t) d.pecdf_off + words_for_floats(2 * (size_t) std::max(1, r.n_edges)));
            // a sample of the primary-edge term starts with this search (15 dependent loads for config 5's 26 592 edges)
            if (sync_guide(sc, "sensor." + std::to_string(k) + ".guide", r.edge_cmf, r.n_edges, r.edge_sum, 4, d.pe_guide, d.pe_guide_n, &edge_bytes, info)) return 1;
        } else { d.pe_guide = od->pe_guide; d.pe_guide_n = od->pe_guide_n; }
        // live-pixel mask: a function of the triangles, this sensor's world_to_sample and the frame size
        std::memcpy(&sc->sensor_w2s[16 * (size_t) k], r.world_to_sample, 64);
        const bool same_view = od && !geo && 16 * (size_t) k + 16 <= w2s_old.size() && std::memcmp(&w2s_old[16 * (size_t) k], r.world_to_sample, 64) == 0 &&
                               Told.width == T.width && Told.height == T.height && (Told.env_emitter >= 0) == (T.env_emitter >= 0) &&
                               ((long long) Told.width * Told.height * std::max(1, Told.spp) < (1ll << 31)) == ((long long) T.width * T.height * std::max(1, T.spp) < (1ll << 31));
        // ... and so is the camera-ray table (brute-force scenes, perspective sensors), with the same lifetime
        if (same_view && (od->ortho != 0) == (d.ortho != 0)) { d.live = od->live; d.cam_tab = od->cam_tab; d.tab_shift = od->tab_shift; d.tab_w = od->tab_w; return 0; }
        d.live = nullptr; d.cam_tab = nullptr; d.tab_shift = 0; d.tab_w = 0;
        std::vector<unsigned> live;
        static const bool no_live = std::getenv("PSDR_NO_LIVE_MASK") != nullptr;       // documented switch (include/psdr_hip.h): render the provably-zero samples as well
        static const bool no_tab = std::getenv("PSDR_NO_CAM_TABLE") != nullptr;        // documented switch (include/psdr_hip.h): every camera ray through the tracer
        bool use = !no_live && T.env_emitter < 0 && (long long) s->width * s->height * std::max(1, s->spp) < (1ll << 31);
        const bool use_tab = !no_tab && T.env_emitter < 0 && s->tris.n_triangles <= kBruteForceMax && !d.ortho;
        ScreenTris st;
        const bool projected = (use || use_tab) && project_tris(s->tris.p0, s->tris.e1, s->tris.e2, s->tris.n_triangles, r.world_to_sample, s->width, s->height, st);
        use = use && projected;
        if (use) {       // worth a window of bit tests per regeneration only when a good part of the frame is dead (the sphere box, all of it live: +1.7 % with the mask)
            fill_live_mask(st, s->width, s->height, live);
            long long n_set = 0;
            for (unsigned x : live) n_set += __builtin_popcount(x);
            use = n_set * 4 <= (long long) s->width * s->height * 3;
        }
        if (use) { if (sync_named(sc, "sensor." + std::to_string(k) + ".live", live.data(), live.size() * sizeof(unsigned), false, d.live, info)) return 1; }
        else live.clear();
        sc->live_host[(size_t) k].swap(live);
        // (made on the device once the triangle rows of this state are there - launch_cam_tables: nothing is sent, and the allocation is scratch the device fills itself)
        if (!sc->cam_tabs[(size_t) k]) sc->cam_tabs[(size_t) k] = std::make_unique<DevBuf>();
        DevBuf &tab = *sc->cam_tabs[(size_t) k];
        if (use_tab && projected) {
            d.tab_shift = cam_table_shift(s->width, s->height);
            d.tab_w = (s->width + (1 << d.tab_shift) - 1) >> d.tab_shift;
            const size_t cells = (size_t) d.tab_w * (size_t) ((s->height + (1 << d.tab_shift) - 1) >> d.tab_shift);
            if (tab.ensure(cells * sizeof(uint64_t))) return 1;
            d.cam_tab = tab.as<unsigned long long>();
            tabs_to_fill.push_back(k);
        } else if (tab.p) { HIPCHK(hipFree(tab.p)); tab.p = nullptr; tab.bytes = 0; }
        return 0;
    }

    int sensors() {
        const std::vector<SensorDev> sensors_old = sc->sensors;
        const std::vector<float> w2s_old = sc->sensor_w2s;
        sc->sensors.assign((size_t) s->n_sensors, SensorDev{});
        sc->sensor_w2s.assign(16 * (size_t) s->n_sensors, 0.f);
        sc->live_host.resize((size_t) s->n_sensors);
        sc->cam_tabs.resize((size_t) s->n_sensors);
        sc->pe_ids.resize((size_t) s->n_sensors);
        edge_path = sec_cdf_mode;
        bool any_sensor_dev = false;
        for (int k = 0; ereq && k < s->n_sensors; ++k) any_sensor_dev = any_sensor_dev || ereq->mode[k] == PSDR_EDGES_DEVICE;
        if (any_sensor_dev && pe_sync_topology(sc, s, ereq->topo, edge_bytes)) return 1;
        info.bytes_uploaded += edge_bytes;
        edge_bytes += sec_bytes;
        for (int k = 0; k < s->n_sensors; ++k)
            if (sensor(k, (size_t) k < sensors_old.size() ? &sensors_old[(size_t) k] : nullptr, w2s_old)) return 1;
        return 0;
    }

    // environment map (global memory, outside the blob)
    int environment() {
        if (T.env_emitter < 0) { T.env = EnvDev{}; return 0; }
        const psdr_envmap_rec *er = s->envmap;
        if (!er || !er->radiance || !er->cell_pmf || !er->cell_cmf || er->width < 2 || er->height < 2) return fail("EnvironmentMap emitter without a configured psdr_envmap_rec");
        EnvDev &ED = T.env;
        const size_t cells = (size_t) er->reso[0] * er->reso[1], texels = (size_t) 3 * er->width * er->height;
        const bool keep = same_env && Told.env_emitter >= 0 && Told.env.width == er->width && Told.env.height == er->height && Told.env.num_cells == (int) cells;
        const bool had_d = Told.env_emitter >= 0 && Told.env.d_radiance != nullptr;
        const int *old_guide = Told.env.cell_guide; const int old_guide_n = Told.env.guide_n;
        if (sync_named(sc, "env.radiance", er->radiance, texels * sizeof(float), keep, ED.radiance, info)) return 1;
        if (sync_named(sc, "env.cell_pmf", er->cell_pmf, cells * sizeof(float), keep, ED.cell_pmf, info)) return 1;
        if (sync_named(sc, "env.cell_cmf", er->cell_cmf, cells * sizeof(float), keep, ED.cell_cmf, info)) return 1;
        if (sync_named(sc, "env.d_radiance", er->d_radiance, texels * sizeof(float), keep && same_env_tan && had_d, ED.d_radiance, info)) return 1;
        if (keep) { ED.cell_guide = old_guide; ED.guide_n = old_guide_n; }
        else if (sync_guide(sc, "env.guide", er->cell_cmf, (int) cells, er->cell_sum, 32, ED.cell_guide, ED.guide_n, nullptr, info)) return 1;
        ED.width = er->width; ED.height = er->height; ED.reso0 = er->reso[0]; ED.reso1 = er->reso[1]; ED.num_cells = (int) cells;
        ED.scale = er->scale; ED.cell_sum = er->cell_sum;
        std::memcpy(ED.to_world.m, er->to_world, 64); std::memcpy(ED.from_world.m, er->from_world, 64);
        std::memcpy(ED.d_from_world.m, er->d_from_world, 64); ED.d_scale = er->d_scale;
        for (int k = 0; k < 3; ++k) { ED.lower[k] = er->lower[k]; ED.upper[k] = er->upper[k]; }
        for (int k = 0; k < 4; ++k) { ED.xf[k] = er->radiance_xf[k]; ED.d_xf[k] = er->d_radiance_xf[k]; }
        return 0;
    }

    // bitmap parameters: three slots per BSDF - [0] reflectance / diffuse reflectance (rgb), [1] specular (rgb), [2] roughness (1 channel)
    int bitmaps() {
        T.tex = nullptr;
        sc->tex_total = 0;
        sc->tex_layout.clear();
        bool any_tex = false;
        for (int i = 0; i < s->n_bsdfs; ++i) any_tex |= s->bsdfs[i].tex_data != nullptr || s->bsdfs[i].spec_tex_data != nullptr || s->bsdfs[i].rough_tex_data != nullptr;
        if (!any_tex) return 0;
        std::vector<TexDev> td((size_t) 3 * s->n_bsdfs, TexDev{nullptr, nullptr, 0, 0, -1, {0.f, 1.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}});
        for (int i = 0; i < s->n_bsdfs; ++i) {
            const psdr_bsdf_rec &b = s->bsdfs[i];
            const float *src[3] = {b.tex_data, b.spec_tex_data, b.rough_tex_data}, *dsrc[3] = {b.d_tex_data, b.d_spec_tex_data, b.d_rough_tex_data};
            const int tw[3] = {b.tex_width, b.spec_tex_width, b.rough_tex_width}, th[3] = {b.tex_height, b.spec_tex_height, b.rough_tex_height};
            for (int k = 0; k < 3; ++k) {
                if (!src[k]) continue;
                if (k > 0 && b.type != 1 && b.type != 2 && !(b.type == 3 && k == 2)) return fail("this BSDF type has no second / third bitmap parameter");
                if (tw[k] < 2 || th[k] < 2) return fail("Bitmap: invalid resolution!");
                const size_t nt = (size_t) (k == 2 ? 1 : 3) * tw[k] * th[k];
                const std::string key = "tex." + std::to_string(i) + "." + std::to_string(k);
                TexDev &t = td[3 * (size_t) i + k];
                const bool had = sc->named.count(key) != 0, had_d = sc->named.count(key + ".d") != 0;
                if (sync_named(sc, key, src[k], nt * sizeof(float), same_bitmaps && had, t.data, info)) return 1;
                if (sync_named(sc, key + ".d", dsrc[k], nt * sizeof(float), same_bitmaps && had_d, t.d_data, info)) return 1;
                t.w = tw[k]; t.h = th[k];
                t.g_off = sc->tex_total; sc->tex_total += (long long) nt;
                for (int q = 0; q < 4; ++q) { t.xf[q] = b.tex_xf[k][q]; t.d_xf[q] = b.d_tex_xf[k][q]; }
            }
        }
        if (sync_named(sc, "tex.table", td.data(), td.size() * sizeof(TexDev), false, T.tex, info)) return 1;
        sc->tex_layout.resize(td.size());
        for (size_t i = 0; i < td.size(); ++i) sc->tex_layout[i] = td[i].g_off;
        return 0;
    }

    int materials() {
        T.mat = nullptr;
        bool any = false;
        for (int i = 0; i < s->n_bsdfs; ++i) any |= s->bsdfs[i].type != 0;
        if (!any) return 0;
        std::vector<MatDev> md((size_t) s->n_bsdfs);
        for (int i = 0; i < s->n_bsdfs; ++i) {
            const psdr_bsdf_rec &b = s->bsdfs[i];
            MatDev &m = md[(size_t) i];
            for (int k = 0; k < 3; ++k) { m.specular[k] = b.specular[k]; m.d_specular[k] = b.d_specular[k]; }
            m.roughness = b.roughness; m.d_roughness = b.d_roughness;
            m.alpha_u = b.alpha_u; m.alpha_v = b.alpha_v; m.d_alpha_u = b.d_alpha_u; m.d_alpha_v = b.d_alpha_v;
            for (int k = 0; k < 3; ++k) { m.eta[k] = b.eta[k]; m.d_eta[k] = b.d_eta[k]; m.k[k] = b.k[k]; m.d_k[k] = b.d_k[k]; }
        }
        return sync_named(sc, "mat.table", md.data(), md.size() * sizeof(MatDev), false, T.mat, info);
    }

    // MicrofacetPerVertex: parameter arrays per BSDF + the mesh-local vertex ids of every triangle slot
    int per_vertex() {
        const int n = tr.n_triangles;
        T.pv = nullptr; T.tri_fi = nullptr;
        bool any_pv = false;
        for (int i = 0; i < s->n_bsdfs; ++i) any_pv |= s->bsdfs[i].type == 4;
        if (!any_pv) return 0;
        if (!tr.face_indices) return fail("MicrofacetPerVertex needs psdr_triangles.face_indices");
        std::vector<PvDev> pd((size_t) s->n_bsdfs, PvDev{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, {-1, -1, -1}});
        if (sc->tex_layout.size() < (size_t) 3 * s->n_bsdfs) sc->tex_layout.resize((size_t) 3 * s->n_bsdfs, -1);
        for (int i = 0; i < s->n_bsdfs; ++i) {
            const psdr_bsdf_rec &b = s->bsdfs[i];
            if (b.type != 4) continue;
            if (b.pv_count <= 0 || !b.pv_specular || !b.pv_diffuse || !b.pv_roughness) return fail("MicrofacetPerVertex: missing per-vertex data");
            const size_t nv = (size_t) b.pv_count;
            const std::string key = "pv." + std::to_string(i) + ".";
            PvDev &p = pd[(size_t) i];
            const float *srcs[6] = {b.pv_specular, b.d_pv_specular, b.pv_diffuse, b.d_pv_diffuse, b.pv_roughness, b.d_pv_roughness};
            const float **dsts[6] = {&p.spec, &p.d_spec, &p.diff, &p.d_diff, &p.rough, &p.d_rough};
            const size_t lens[6] = {3 * nv, 3 * nv, 3 * nv, 3 * nv, nv, nv};
            for (int q = 0; q < 6; ++q) {
                const std::string kq = key + std::to_string(q);
                const bool had = sc->named.count(kq) != 0;
                if (sync_named(sc, kq, srcs[q], lens[q] * sizeof(float), same_bitmaps && had, *dsts[q], info)) return 1;
            }
            p.n = b.pv_count;
            // adjoint blocks in psdr_grads.g_tex, numbered like Microfacet's maps: 0 diffuse, 1 specular, 2 roughness
            const size_t sizes[3] = {3 * nv, 3 * nv, nv};
            for (int k = 0; k < 3; ++k) { p.g_off[k] = sc->tex_total; sc->tex_layout[3 * (size_t) i + k] = sc->tex_total; sc->tex_total += (long long) sizes[k]; }
        }
        // every mesh that uses a per-vertex BSDF must index inside its arrays
        for (int i = 0; i < n; ++i) {
            const int bid = s->meshes[tr.mesh_id[i]].bsdf_id;
            if (bid >= 0 && s->bsdfs[bid].type == 4)
                for (int k = 0; k < 3; ++k)
                    if (tr.face_indices[3 * (size_t) i + k] < 0 || tr.face_indices[3 * (size_t) i + k] >= s->bsdfs[bid].pv_count) return fail("MicrofacetPerVertex: fewer values than mesh vertices");
        }
        const bool had_fi = sc->named.count("tri_fi") != 0;
        if (geo || !had_fi) {
            std::vector<int> fi((size_t) 3 * n);
            for (int slot = 0; slot < n; ++slot)
                for (int k = 0; k < 3; ++k) fi[3 * (size_t) slot + k] = tr.face_indices[3 * (size_t) sc->order[(size_t) slot] + k];
            if (sync_named(sc, "tri_fi", fi.data(), fi.size() * sizeof(int), false, T.tri_fi, info)) return 1;
        } else T.tri_fi = sc->buf("tri_fi").as<int>();
        return sync_named(sc, "pv.table", pd.data(), pd.size() * sizeof(PvDev), false, T.pv, info);
    }

    // hot triangles of the reverse-mode accumulators: emitter meshes first, then by area, at most kHotMax (an update keeps the choice of the build: it only decides which rows accumulate in LDS)
    int hot_triangles() {
        const int n = tr.n_triangles;
        constexpr int kHotMax = 720;                                   // 720 x 22 floats = 62 KB of LDS
        std::vector<int> ord((size_t) n);
        std::vector<float> key((size_t) n);
        for (int i = 0; i < n; ++i) {
            ord[(size_t) i] = i;
            const float *a1 = tr.e1 + 3 * (size_t) i, *a2 = tr.e2 + 3 * (size_t) i;
            const float cx = a1[1] * a2[2] - a1[2] * a2[1], cy = a1[2] * a2[0] - a1[0] * a2[2], cz = a1[0] * a2[1] - a1[1] * a2[0];
            const bool emit = s->meshes[tr.mesh_id[i]].emitter_id >= 0;
            key[(size_t) i] = std::sqrt(cx * cx + cy * cy + cz * cz) * (emit ? 1e30f : 1.f);
        }
        sc->n_hot = std::min(n, kHotMax);
        // the n_hot largest keys, ties to the smaller index (what a stable sort of all keys puts first)
        auto before = [&](int x, int y) { return key[(size_t) x] > key[(size_t) y] || (key[(size_t) x] == key[(size_t) y] && x < y); };
        std::partial_sort(ord.begin(), ord.begin() + sc->n_hot, ord.end(), before);
        std::vector<int> hmap((size_t) std::max(1, n), -1), hinv((size_t) std::max(1, sc->n_hot), 0);
        for (int h = 0; h < sc->n_hot; ++h) { hmap[(size_t) ord[(size_t) h]] = h; hinv[(size_t) h] = ord[(size_t) h]; }
        return sc->hot_map.upload(hmap.data(), hmap.size() * sizeof(int)) || sc->hot_inv.upload(hinv.data(), hinv.size() * sizeof(int)) ? 1 : 0;
    }

    // send the sections that were written (adjacent ones as one copy)
    int send() {
        if (blob_moved) { dirty.clear(); dirty.push_back({0, L.words}); }
        std::sort(dirty.begin(), dirty.end(), [](const WordRange &a, const WordRange &b) { return a.b < b.b; });
        auto send = [&](size_t b, size_t e) -> int {
            if (e <= b) return 0;
            HIPCHK(hipMemcpyAsync((char *) sc->blob.p + 16 * b, (const char *) H + 16 * b, 16 * (e - b), hipMemcpyHostToDevice, nullptr));
            info.bytes_uploaded += (int64_t) (16 * (e - b));
            return 0;
        };
        for (size_t i = 0; i < dirty.size();) {
            size_t b = dirty[i].b, e = dirty[i].e, j = i + 1;
            while (j < dirty.size() && dirty[j].b <= e) { e = std::max(e, dirty[j].e); ++j; }
            if (blob_moved && !build && uses_bvh) {
                // (after a move of the allocation the nodes a refit wrote were carried over on the device: the host copy of a refitted tree is stale)
                const size_t nb = (size_t) T.nodes_off, ne = nb + (size_t) (kNodeFloats / 4) * (size_t) T.n_nodes;
                if (send(b, std::min(e, nb)) || send(std::max(b, ne), e)) return 1;
            } else if (send(b, e)) return 1;
            i = j;
        }
        return 0;
    }

    // the camera-ray tables the sensors asked for (sensor()), from the triangle rows of this state: after the sections were sent and the device's rows computed
    int launch_cam_tables() {
        for (int k : tabs_to_fill) {
            const SensorDev &d = sc->sensors[(size_t) k];
            const int cells_h = (s->height + (1 << d.tab_shift) - 1) >> d.tab_shift, cells = d.tab_w * cells_h;
            W2S w2s;
            std::memcpy(w2s.m, s->sensors[k].world_to_sample, 64);
            hipLaunchKernelGGL(k_cam_table, dim3((cells + 255) / 256), dim3(256), 0, (hipStream_t) nullptr, sc->blob.as<float4>(), T.trav_off, T.n_tris, w2s, s->width, s->height,
                               d.tab_shift, d.tab_w, cells_h, (unsigned long long *) sc->cam_tabs[(size_t) k]->p);
        }
        HIPCHK(hipGetLastError());
        return 0;
    }

    // scene class, launch geometry
    int launch_geometry() {
        const size_t stack_bytes = (size_t) T.stack_depth * kBlock * sizeof(int);
        const size_t blob_bytes = (size_t) T.blob_words * 16;
        // keeps >= 4 workgroups per CU (160 KiB LDS); the environment-map and texture code lives in the LDS=false kernels only (shade.h)
        bool no_lds = false;
    #ifdef PSDR_DEV_KNOBS
        no_lds = std::getenv("PSDR_NO_LDS") != nullptr;      // measurement knob: run small scenes through the global-memory classes
    #endif
        sc->lds = !no_lds && !uses_bvh && blob_bytes + stack_bytes <= 40 * 1024 && T.env_emitter < 0 && T.tex == nullptr && T.mat == nullptr && T.pv == nullptr;      // (LDS class = brute-force scenes)
        sc->lean = !sc->lds && T.tex == nullptr && T.mat == nullptr && T.pv == nullptr;
        // class 3: the same staging for small scenes WITH materials / bitmap parameters (the material and texture tables stay in global
        // memory; the triangle, BSDF, emitter and edge tables are what every path vertex reads)
        sc->lds_mat = !no_lds && !sc->lds && !uses_bvh && blob_bytes + stack_bytes <= 40 * 1024 && T.env_emitter < 0 && T.pv == nullptr;
        sc->smem_bytes = ((sc->lds || sc->lds_mat) ? blob_bytes : 0) + stack_bytes;
        if (sc->smem_bytes > 64 * 1024) return fail("BVH too deep for the LDS traversal stack");
        if (fresh) {
            if (sc->counters.upload(nullptr, sizeof(Counters))) return 1;
            if (sc->queues.upload(nullptr, sizeof(unsigned long long) * kQueueRing)) return 1;
        }
        if (!build) return 0;
        int dev = 0, cus = 256;
        if (hipGetDevice(&dev) == hipSuccess) { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount; }
        // workgroups per launch: a multiple of what fits on the device (persistent workgroups pull work until the launch's queue is empty; the ones that start late find it empty)
        // (measured, round 4: brute-force scenes 4 per CU - what is resident at most - C3 forward -0.5 %, its backward pass 8.28 -> 8.06 ms; BVH scenes 8: config 5 218.7 ms, with 4 220.1)
        int per_cu = uses_bvh ? 8 : 4;
    #ifdef PSDR_DEV_KNOBS
        if (const char *e = std::getenv("PSDR_GRID_PER_CU")) per_cu = std::max(1, std::atoi(e));
    #endif
        sc->grid = cus * per_cu;
        T.gstack = nullptr; T.gstack_stride = 0;
        if (uses_bvh && sc->tree_max_stack > T.stack_lds) {
            // stack entries beyond the LDS part: one int per entry and lane of the largest grid any kernel is launched with - kTermSlices of them, because the
            // three terms of a renderD run as concurrent launches on forked streams (api.hip::render_impl) and a slice is indexed by workgroup and thread only
            const size_t stride = (size_t) sc->grid * kBlock;
            sc->gstack_slice = stride * (size_t) (sc->tree_max_stack - T.stack_lds);
            if (sc->gstack.ensure(sizeof(int) * sc->gstack_slice * (size_t) kTermSlices)) return 1;
            T.gstack = (int *) sc->gstack.p; T.gstack_stride = (int) stride;
        }
        return 0;
    }
};

// Everything between a snapshot and a renderable device scene.  fresh: the handle is new.  same: PSDR_SAME_* bits the caller vouches for
// (relative to the snapshot of the previous create / update of this handle); force_build: build the tree even if the triangle count fits.
static int scene_sync(psdr_hip_scene *sc, const psdr_scene_snapshot *s, unsigned same, bool fresh, bool force_build, psdr_update_info *info_out, const EdgeRequest *ereq = nullptr) {
    const auto t_start = std::chrono::steady_clock::now();
    if (int rc = sync_validate(s)) return rc;
    SceneSync c{sc, s, ereq, fresh};
    if (int rc = c.plan_request(same, force_build)) return rc;
    if (!fresh) {
        // the previous calls on this scene read what is about to be overwritten: wait for the last of them (configure() is a synchronisation point in the reference as well)
        std::lock_guard<std::mutex> lk(sc->mu);
        if (sc->ev && sc->have_last) HIPCHK(hipEventSynchronize(sc->ev));
    }
    const auto t_tree = std::chrono::steady_clock::now();
    if (c.build) {
        if (tree_build(sc, s->tris, c.new_nodes)) return 1;
        c.info.tree = 2;
    }
    c.info.ms_tree = ms_since(t_tree);
    const auto t_fill = std::chrono::steady_clock::now();
    if (int rc = c.plan_layout()) return rc;
    c.commit_tables();
    if (int rc = c.blob()) return rc;
    if (int rc = c.geometry()) return rc;
    c.tri_rows();
    c.filter();
    c.small_tables();
    if (c.sec_edges() || c.sensors() || c.environment() || c.bitmaps() || c.materials() || c.per_vertex()) return 1;
    if (c.build && c.hot_triangles()) return 1;
    c.info.ms_fill = ms_since(t_fill);
    const auto t_up = std::chrono::steady_clock::now();
    if (c.send()) return 1;
    c.info.ms_upload = ms_since(t_up);

    // ---- the tree follows the triangles
    c.info.sah_cost_built = sc->cost_built;
    c.info.sah_cost = sc->cost_built;
    if (!c.build && c.geo && c.uses_bvh) {
        const auto t_refit = std::chrono::steady_clock::now();
        double cost = 0.0;
        if (tree_refit(sc, &cost)) return 1;
        c.info.tree = 1;
        c.info.sah_cost = cost;
        c.info.ms_tree += ms_since(t_refit);
        // the topology no longer fits the geometry: build again (everything that depends on the triangle order is rewritten)
        if (!(cost <= kRebuildFactor * sc->cost_built)) {
            if (!c.rows_valid) return PSDR_HIP_NEED_ROWS;         // (the rows on the device are this state's, the tables are complete: the caller comes back with its rows and the tree is built then)
            return scene_sync(sc, s, 0, false, true, info_out, ereq);
        }
    }
    if (c.launch_geometry()) return 1;
    if (c.launch_cam_tables()) return 1;
    HIPCHK(hipStreamSynchronize(nullptr));
    c.info.ms_total = ms_since(t_start);
    sc->edge_path = c.edge_path; sc->edge_bytes = c.edge_bytes;
    sc->pe_cap = c.cap_layout ? c.pe_cap : 0;
    sc->last_info = c.info;
    if (info_out) *info_out = c.info;
    return 0;
}

// psdr_hip_scene_update / _update_edges.  scene_sync rewrites the handle in place (tables, offsets, named buffers, sensors) while it uploads: a failure midway - a validation
// message, out of memory, an LDS budget - leaves old and new sections mixed.  Such a handle is POISONED: the render entry points refuse it, and the next update ignores what
// the caller vouches for (its `same` bits are relative to a snapshot the device never fully received) and builds everything again.
static int update_entry(psdr_hip_scene *scene, const psdr_scene_snapshot *s, uint32_t same, psdr_update_info *info, const EdgeRequest *ereq) {
    const bool was_poisoned = scene->poisoned;
    const int rc = scene_sync(scene, s, was_poisoned ? 0u : same, false, was_poisoned, info, ereq);
    if (rc == PSDR_HIP_NEED_ROWS) return rc;                  // (nothing was changed, or only rows that are this state's: see psdr_scene_snapshot.rows_valid)
    scene->poisoned = rc != 0;
    if (rc) scene->tree_tris = -1;
    return rc;
}

extern "C" {

int psdr_hip_scene_create(const psdr_scene_snapshot *s, psdr_hip_scene **out) {
    if (!s || !out) return fail("psdr_hip_scene_create: null argument");
    if (s->abi_version != PSDR_HIP_ABI_VERSION) return fail("psdr_hip_scene_create: ABI version mismatch");
    auto sc = std::make_unique<psdr_hip_scene>();
    if (scene_sync(sc.get(), s, 0, true, true, nullptr)) return 1;
    *out = sc.release();
    return 0;
}

int psdr_hip_scene_update(psdr_hip_scene *scene, const psdr_scene_snapshot *s, uint32_t same, psdr_update_info *info) {
    if (!scene || !s) return fail("psdr_hip_scene_update: null argument");
    if (s->abi_version != PSDR_HIP_ABI_VERSION) return fail("psdr_hip_scene_update: ABI version mismatch");
    return update_entry(scene, s, same, info, nullptr);
}

int psdr_hip_scene_update_edges(psdr_hip_scene *scene, const psdr_scene_snapshot *s, uint32_t same, const psdr_edge_topology *topo, const int32_t *sensor_mode, psdr_update_info *info) {
    if (!scene || !s || !topo || !sensor_mode) return fail("psdr_hip_scene_update_edges: null argument");
    if (s->abi_version != PSDR_HIP_ABI_VERSION) return fail("psdr_hip_scene_update_edges: ABI version mismatch");
    for (int i = 0; i < s->n_sensors; ++i)
        if (sensor_mode[i] < PSDR_EDGES_HOST || sensor_mode[i] > PSDR_EDGES_KEEP) return fail("psdr_hip_scene_update_edges: unknown sensor mode");
    const EdgeRequest er{topo, sensor_mode};
    return update_entry(scene, s, same, info, &er);
}

int psdr_hip_scene_primary_edges(const psdr_hip_scene *sc, int32_t sensor_id, int32_t *count, int32_t *ids, int32_t cap, float *edge_sum) {
    if (!sc || !count) return fail("null argument");
    if (sensor_id < 0 || sensor_id >= (int) sc->sensors.size()) return fail("Invalid sensor id!");
    const int n = sc->sensors[(size_t) sensor_id].n_edges;
    *count = n;
    if (edge_sum) *edge_sum = sc->sensors[(size_t) sensor_id].edge_sum;
    if (ids) {
        const std::vector<int32_t> *v = (size_t) sensor_id < sc->pe_ids.size() ? &sc->pe_ids[(size_t) sensor_id] : nullptr;
        if (!v || v->size() != 3 * (size_t) n) return fail("psdr_hip_scene_primary_edges: this sensor's edges were not selected on the device");
        if (cap < n) return fail("psdr_hip_scene_primary_edges: ids has room for fewer edges than the sensor keeps");
        if (n > 0) std::memcpy(ids, v->data(), sizeof(int32_t) * 3 * (size_t) n);
    }
    return 0;
}

int psdr_hip_scene_edge_path(const psdr_hip_scene *sc, int32_t *path, int64_t *edge_bytes) {
    if (!sc) return fail("null scene");
    if (path) *path = sc->edge_path;
    if (edge_bytes) *edge_bytes = sc->edge_bytes;
    return 0;
}

// Test aid (synchronises, downloads the sections): every sensor's primary-edge rows and distribution and the secondary-edge distribution of the device blob against
// what the host path would write from `snapshot`.  -> number of 32-bit words that differ (a count or a sum that differs counts too).
int psdr_hip_scene_check_edges(const psdr_hip_scene *sc, const psdr_scene_snapshot *s, int64_t *mismatches) {
    if (!sc || !s || !mismatches) return fail("null argument");
    *mismatches = 0;
    if ((size_t) s->n_sensors != sc->sensors.size()) return fail("psdr_hip_scene_check_edges: another sensor count than the device scene's");
    HIPCHK(hipDeviceSynchronize());
    long long bad = 0;
    auto fetch = [&](size_t off_floats, size_t n, std::vector<float> &dst) -> int {
        dst.resize(n);
        if (n) HIPCHK(hipMemcpy(dst.data(), (const float *) sc->blob.p + off_floats, sizeof(float) * n, hipMemcpyDeviceToHost));
        return 0;
    };
    auto diff = [&](const float *dev, const float *host, size_t n) { for (size_t i = 0; i < n; ++i) bad += std::memcmp(dev + i, host + i, 4) != 0 ? 1 : 0; };
    // the search table of a distribution against the one the host path builds from the host's cmf (scene_obj.h::build_cdf_guide)
    auto guide_diff = [&](const float *cmf, int n, float sum, const int *dev_guide, int dev_n) -> int {
        std::vector<int> want, got;
        build_cdf_guide(cmf, n, sum, want, 4);
        const int want_n = want.empty() ? 0 : (int) want.size() - 1;
        if (want_n != dev_n || (want_n > 0 && !dev_guide)) { bad += 1 + std::abs(want_n - dev_n); return 0; }
        if (want_n == 0) return 0;
        got.resize(want.size());
        HIPCHK(hipMemcpy(got.data(), dev_guide, sizeof(int) * got.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < want.size(); ++i) bad += want[i] != got[i] ? 1 : 0;
        return 0;
    };
    std::vector<float> rows, cdf;
    for (int k = 0; k < s->n_sensors; ++k) {
        const psdr_sensor_rec &r = s->sensors[k];
        const SensorDev &d = sc->sensors[(size_t) k];
        const int n = std::max(0, r.n_edges);
        if (d.n_edges != n) { bad += 1 + std::abs(d.n_edges - n); continue; }
        if (n == 0) continue;
        bad += std::memcmp(&d.edge_sum, &r.edge_sum, 4) != 0 ? 1 : 0;
        if (fetch(4 * (size_t) d.pe_off, 12 * (size_t) n, rows) || fetch(4 * (size_t) d.pecdf_off, 2 * (size_t) n, cdf)) return 1;
        for (size_t i = 0; i < (size_t) n; ++i) {
            float h[4 * kPeWords];
            pack_pe_row(r, i, h);
            diff(&rows[12 * i], h, 12);
        }
        diff(cdf.data(), r.edge_pmf, (size_t) n); diff(cdf.data() + n, r.edge_cmf, (size_t) n);
        if (guide_diff(r.edge_cmf, n, r.edge_sum, d.pe_guide, d.pe_guide_n)) return 1;
    }
    const psdr_sec_edges &se = s->sec_edges;
    if (std::max(0, se.n_edges) != std::max(0, sc->E.n)) bad += 1 + std::abs(se.n_edges - sc->E.n);
    else if (se.n_edges > 0) {
        bad += std::memcmp(&sc->E.sum, &se.sum, 4) != 0 ? 1 : 0;
        if (fetch(4 * (size_t) sc->E.cdf_off, 2 * (size_t) se.n_edges, cdf)) return 1;
        diff(cdf.data(), se.pmf, (size_t) se.n_edges); diff(cdf.data() + se.n_edges, se.cmf, (size_t) se.n_edges);
        if (guide_diff(se.cmf, se.n_edges, se.sum, sc->E.guide, sc->E.guide_n)) return 1;
    }
    *mismatches = bad;
    return 0;
}

int psdr_hip_scene_destroy(psdr_hip_scene *scene) { delete scene; return 0; }
int psdr_hip_bvh_node_bytes(void) { return kNodeFloats * 4; }

int psdr_hip_scene_stats(const psdr_hip_scene *sc, int32_t *n_nodes, int32_t *n_leaves, int32_t *max_depth, int32_t *lds_bytes) {
    if (!sc) return fail("null scene");
    if (n_nodes) *n_nodes = sc->T.n_nodes;
    if (n_leaves) *n_leaves = sc->n_leaves;
    if (max_depth) *max_depth = sc->max_depth;
    if (lds_bytes) *lds_bytes = (int32_t) sc->smem_bytes * (sc->lds ? 1 : -1);
    return 0;
}

int psdr_hip_scene_last_update(const psdr_hip_scene *sc, psdr_update_info *info) {
    if (!sc || !info) return fail("null argument");
    *info = sc->last_info;
    return 0;
}

// Test aid (synchronises, downloads the sections): the triangle rows (traversal, shading, tangent) and the secondary-edge rows of the device blob against the rows the host
// path would write from `snapshot` - the check that the kernels of geometry_on_device produce the host's bits.  -> number of 32-bit words that differ.
int psdr_hip_scene_check_rows(const psdr_hip_scene *sc, const psdr_scene_snapshot *s, int64_t *mismatches) {
    if (!sc || !s || !mismatches) return fail("null argument");
    *mismatches = 0;
    const SceneTables &T = sc->T;
    const psdr_triangles &tr = s->tris;
    const int n = tr.n_triangles;
    if (n != T.n_tris) return fail("psdr_hip_scene_check_rows: another triangle count than the device scene's");
    HIPCHK(hipDeviceSynchronize());
    auto fetch = [&](int off_words, size_t words, std::vector<float> &dst) -> int {
        dst.resize(4 * words);
        if (words) HIPCHK(hipMemcpy(dst.data(), (const char *) sc->blob.p + 16 * (size_t) off_words, 16 * words, hipMemcpyDeviceToHost));
        return 0;
    };
    std::vector<float> trav, shade, tan, sec;
    if (fetch(T.trav_off, 3 * (size_t) n, trav) || fetch(T.shade_off, 6 * (size_t) n, shade)) return 1;
    if (T.has_tangent && fetch(T.tan_off, 6 * (size_t) n, tan)) return 1;
    long long bad = 0;
    auto diff = [&](const float *dev, const float *host, size_t n) { for (size_t i = 0; i < n; ++i) bad += std::memcmp(dev + i, host + i, 4) != 0 ? 1 : 0; };
    for (int slot = 0; slot < n; ++slot) {
        const size_t o = (size_t) sc->order[(size_t) slot];
        float h_trav[4 * kTravWords], h_shade[4 * kShadeWords], h_tan[4 * kTanWords];
        pack_tri_rows(tr, o, h_trav, h_shade);
        diff(&trav[12 * (size_t) slot], h_trav, 12);
        diff(&shade[24 * (size_t) slot], h_shade, 16);          // (words 4 and 5 - the uv of the three corners - do not depend on the vertices: the device never writes them)
        if (T.has_tangent && tr.d_p0) {
            pack_tan_row(tr, o, h_tan);
            diff(&tan[24 * (size_t) slot], h_tan, 24);
        }
    }
    const psdr_sec_edges &se = s->sec_edges;
    if (se.n_edges > 0 && se.n_edges == sc->E.n) {
        if (fetch(sc->E.off, 6 * (size_t) se.n_edges, sec)) return 1;
        for (size_t i = 0; i < (size_t) se.n_edges; ++i) {
            float h[4 * kSecWords];
            pack_sec_row(se, i, h);
            diff(&sec[24 * i], h, 24);
        }
    }
    *mismatches = bad;
    return 0;
}

// Checks the device tree against the device triangles (test aid, synchronises): every node's quantised child boxes must contain the padded
// boxes of all triangles below the child, and every triangle slot must hang under exactly one leaf.
int psdr_hip_scene_check_tree(const psdr_hip_scene *sc, int64_t *violations) {
    if (!sc || !violations) return fail("null argument");
    *violations = 0;
    const SceneTables &T = sc->T;
    if (T.n_tris <= kBruteForceMax) return 0;
    HIPCHK(hipDeviceSynchronize());
    std::vector<float> nodes((size_t) kNodeFloats * (size_t) T.n_nodes), trav(12 * (size_t) T.n_tris);
    HIPCHK(hipMemcpy(nodes.data(), (const char *) sc->blob.p + 16 * (size_t) T.nodes_off, nodes.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(trav.data(), (const char *) sc->blob.p + 16 * (size_t) T.trav_off, trav.size() * sizeof(float), hipMemcpyDeviceToHost));
    const unsigned leaf_bit = 1u << (T.ref_bits - 1);
    // float box of every node; children come after their parent in memory, so a reverse sweep sees the children first
    std::vector<float> box(6 * (size_t) T.n_nodes);
    long long bad = 0;
    std::vector<int> seen((size_t) T.n_tris, 0);
    for (int i = T.n_nodes - 1; i >= 0; --i) {
        const float *q = &nodes[(size_t) kNodeFloats * (size_t) i];
        const uint32_t *u = reinterpret_cast<const uint32_t *>(q);
        float ulo[3] = {3e38f, 3e38f, 3e38f}, uhi[3] = {-3e38f, -3e38f, -3e38f};
        for (int k = 0; k < kBvhW; ++k) {
            const uint32_t code = u[kNodeCodeOff + k];
            if (code == 0xffffffffu) continue;
            float lo[3] = {3e38f, 3e38f, 3e38f}, hi[3] = {-3e38f, -3e38f, -3e38f};
            if (code & leaf_bit) {
                const int payload = (int) (code & (leaf_bit - 1u)), first = payload >> 2, cnt = (payload & 3) + 1;
                for (int t = first; t < first + cnt; ++t) {
                    if (t < 0 || t >= T.n_tris) { ++bad; continue; }
                    seen[(size_t) t]++;
                    const float *r = &trav[12 * (size_t) t];
                    const float p0[3] = {r[0], r[1], r[2]}, e1[3] = {r[3], r[4], r[5]}, e2[3] = {r[6], r[7], r[8]};
                    float tl[3], th[3];
                    bvh_tri_box(p0, e1, e2, tl, th);
                    for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], tl[a]); hi[a] = std::max(hi[a], th[a]); }
                }
            } else {
                if ((int) code <= i || (int) code >= T.n_nodes) { ++bad; continue; }
                for (int a = 0; a < 3; ++a) { lo[a] = box[6 * (size_t) code + a]; hi[a] = box[6 * (size_t) code + 3 + a]; }
            }
            // the quantised box of child k as the traversal decodes it
            for (int a = 0; a < 3; ++a) {
                const double step = std::ldexp(1.0, (int) ((u[3] >> (8 * a)) & 0xffu) - 127);
                constexpr int WW = kBvhW / 4;
                const uint32_t wl = u[4 + a * WW + (k >> 2)], wh = u[4 + (3 + a) * WW + (k >> 2)];
                const double ql = (double) q[a] + step * (double) ((wl >> (8 * (k & 3))) & 0xffu), qh = (double) q[a] + step * (double) ((wh >> (8 * (k & 3))) & 0xffu);
                if (!(ql <= (double) lo[a] && qh >= (double) hi[a])) ++bad;
            }
            for (int a = 0; a < 3; ++a) { ulo[a] = std::min(ulo[a], lo[a]); uhi[a] = std::max(uhi[a], hi[a]); }
        }
        for (int a = 0; a < 3; ++a) { box[6 * (size_t) i + a] = ulo[a]; box[6 * (size_t) i + 3 + a] = uhi[a]; }
    }
    for (int t = 0; t < T.n_tris; ++t) if (seen[(size_t) t] != 1) ++bad;
    *violations = bad;
    return 0;
}

int psdr_hip_scene_live_pixels(const psdr_hip_scene *sc, int32_t sensor_id, uint32_t *bits, int64_t *n_live) {
    if (!sc) return fail("null scene");
    if (sensor_id < 0 || sensor_id >= (int) sc->live_host.size()) return fail("Invalid sensor id!");
    const std::vector<unsigned> &m = sc->live_host[(size_t) sensor_id];
    const long long npx = (long long) sc->T.width * sc->T.height;
    long long count = 0;
    for (long long i = 0; i < (npx + 31) / 32; ++i) {
        unsigned w = m.empty() ? 0xffffffffu : m[(size_t) i];
        if (i == (npx + 31) / 32 - 1 && (npx & 31)) w &= (1u << (npx & 31)) - 1u;
        if (bits) bits[i] = w;
        count += __builtin_popcount(w);
    }
    if (n_live) *n_live = count;
    return 0;
}

int psdr_hip_scene_camera_table(const psdr_hip_scene *sc, int32_t sensor_id, int32_t *cell, int32_t *cells_w, int32_t *cells_h, uint64_t *table) {
    if (!sc) return fail("null scene");
    if (sensor_id < 0 || sensor_id >= (int) sc->sensors.size()) return fail("Invalid sensor id!");
    const SensorDev &d = sc->sensors[(size_t) sensor_id];
    const bool none = d.cam_tab == nullptr;
    const int g = none ? 0 : 1 << d.tab_shift, ch = none ? 0 : (sc->T.height + g - 1) / g;
    if (cell) *cell = g;
    if (cells_w) *cells_w = none ? 0 : d.tab_w;
    if (cells_h) *cells_h = ch;
    if (table && !none) HIPCHK(hipMemcpy(table, d.cam_tab, sizeof(uint64_t) * (size_t) d.tab_w * (size_t) ch, hipMemcpyDeviceToHost));     // (a test aid: synchronises)
    return 0;
}

} // extern "C"
