// render_kernels.h — the gfx950 kernel templates.  The heavy ones of a render call: k_paths (interior and primary-edge term),
// k_interior_adjoint, k_interior_adjoint_mat and k_secondary_edges, their device helpers, their wave-count knobs and the lists of their
// instantiations.  The small ones: k_guiding_round, k_trace, k_intersect, k_intersect_ad, k_intersect_adj.
//
// Kernel structure (one thread = one sample lane of the reference's wavefront arrays):
//   * persistent workgroups of 256 threads (4 wave64): every wave pulls batches of 256 work items from a global queue and hands
//     them to whichever of its lanes have finished their path (ballot / popcount regeneration, paths.h), so the lanes of a wave
//     belong to different pixels at different bounces;
//   * at start each workgroup stages the scene blob into LDS (small scenes) with 16-byte loads;
//   * each lane re-derives its RNG state (sampler.h) and traces / shades its whole path in registers (brute-force scenes) or as a
//     traversal worker on the wave's shared ray queue (BVH scenes, trav4.h);
//   * a finished path adds its value (and tangent) to its pixel with one float atomic per channel, as the reference does
//     (scatter_reduce, integrator.cpp:127-129).  Round 1 combined the lanes of a pixel with a segmented scan first; with persistent
//     regeneration the finishing lanes of a wave rarely share a pixel, and the atomics are not what the kernels wait for: the C3
//     interior kernel takes 1.698 ms with them and 1.685 ms with the adds compiled out (round 4, -0.8 %), so nothing is aggregated.
// There is no host synchronisation inside a render call (the reference syncs before each of its 7+
// OptiX launches, scene_optix.cpp:345).
//
// Included by render_units.hip, which instantiates one PSDR_TU<k> list per kernel unit, and by api.hip, which declares all of them
// extern and launches them.  Nothing of the host half lives here: a kernel object changes only when this file or a kernel header does.
#pragma once
#include <hip/hip_runtime.h>

#include "edges.h"
#include "paths.h"
#include "adjoint.h"
#include "adjoint_mat.h"
#include "isect_ad.h"

using namespace psdr;

// ------------------------------------------------------------------------------------------------
// device helpers shared by the kernels
template <int LDS>
PSDR_DEV SceneView<LDS> make_view(const float4 *blob, const SceneTables &T, float4 *smem) {
    const float4 *B = blob;
    if (in_lds(LDS)) {
        for (int i = threadIdx.x; i < T.blob_words; i += kBlock) smem[i] = blob[i];
        __syncthreads();
        B = smem;
    }
    SceneView<LDS> S;
    S.B = B; S.G = blob; S.T = &T;
    S.stack = reinterpret_cast<int *>(smem + (in_lds(LDS) ? T.blob_words : 0)) + threadIdx.x;
    S.c_nodes = S.c_tris = S.c_rays = S.c_hits = 0u;
    S.mis = -1; S.field = -1; S.field_object = -1; S.intensity = 1.f; S.d_intensity = 0.f; S.mode = 0; S.rec = nullptr; S.rec_i = 0; S.rec_n = 0; S.ext = nullptr; S.ext_n = 0; S.probe_kind = 0; S.probe_id = 0; S.probe_comp = 0;
    S.lk = nullptr; S.lk_n = 0; S.lk_max = 0; S.ext_max = 0; S.probe_u = 0.f; S.probe_v = 0.f;
    t4_init_lds(S);
    return S;
}

template <int LDS> PSDR_DEV void flush_counters(const SceneView<LDS> &S, Counters *ctr) {
    unsigned long long v[4] = {S.c_rays, S.c_nodes, S.c_tris, S.c_hits};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        unsigned long long x = v[k];
        for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off);
        if ((threadIdx.x & 63) == 0) atomicAdd(reinterpret_cast<unsigned long long *>(ctr) + k, x);
    }
}

template <int LDS> PSDR_DEV float *scratch_base(float4 *smem, const SceneTables &T) {
    return reinterpret_cast<float *>(smem + (in_lds(LDS) ? T.blob_words : 0)) + T.stack_depth * kBlock;
}

// BVH scenes of the global-memory classes take the decoupled form (traversal refilled per ray, paths.h); brute-force scenes and the
// LDS class keep the lock-step form
template <bool AD, int LDS, bool COUNT, int MODE, int VAR>
PSDR_DEV void run_paths_any(SceneView<LDS> &S, const SensorDev &cam, const PathParams &P) {
    if constexpr (!in_lds(LDS)) {
#ifndef PSDR_NO_ASYNC        // measurement knob: the lock-step form on BVH scenes too
        if (S.T->n_tris > kBruteForceMax) { run_paths_async<AD, LDS, COUNT, MODE, VAR>(S, cam, P); return; }
#endif
    }
    run_paths<AD, LDS, COUNT, MODE, VAR>(S, cam, P);
}

// ------------------------------------------------------------------------------------------------
// interior term (MODE 0) and primary-edge term (MODE 1): persistent lanes with path regeneration, paths.h
// VAR: kGeneral - every kind of call; kLean - forward mode, PathTracer, perspective sensor, no per-lane output, fixed at compile time (paths.h::Switches)
template <bool AD, int LDS, bool COUNT, int MODE, int VAR>
#ifndef PSDR_GLOBAL_C_WAVES
#define PSDR_GLOBAL_C_WAVES 4
#endif
#ifndef PSDR_GLOBAL_AD_WAVES     // class 0: 2 / 3 waves measured on the envmap notebook's glossy bunny (512², 32 spp): interior 4.93 / 5.53 ms
#define PSDR_GLOBAL_AD_WAVES 2
#endif
#ifndef PSDR_LDS_AD_WAVES       // classes 1 / 3 (scene in LDS), AD kernel: 2 / 3 / 4 waves per SIMD measured on C3 1.67 / 1.79 / 2.11 ms (the tangents spill at 168 registers)
#define PSDR_LDS_AD_WAVES 2
#endif
#ifndef PSDR_LDS_C_WAVES
#define PSDR_LDS_C_WAVES 4
#endif
#ifndef PSDR_LEAN_AD_WAVES       // class 2 (BVH scenes): 1 / 2 / 3 / 4 waves per SIMD measured on config 5's interior kernel 47.9 / 31.6 / 34.5 / 37.1 ms, sphere box 13.2 / 7.6 / 8.2 / 8.8 ms -
#define PSDR_LEAN_AD_WAVES 2     // the (value, tangent) path state spills less at 256 registers than it gains from a third wave; the C-mode kernels want their four (3: +16 %, 2: +60 %)
#endif
__global__ __launch_bounds__(kBlock, (AD ? (in_lds(LDS) ? PSDR_LDS_AD_WAVES : (LDS == 2 ? PSDR_LEAN_AD_WAVES : PSDR_GLOBAL_AD_WAVES)) : (in_lds(LDS) ? PSDR_LDS_C_WAVES : PSDR_GLOBAL_C_WAVES))) void k_paths(const float4 *__restrict__ blob, const SceneTables T, const SensorDev cam,
                                                  const PathParams P, Counters *ctr) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    SceneView<LDS> S = make_view<LDS>(blob, T, smem);
    using sw = Switches<VAR>;
    static_assert(!(COUNT && sw::lean), "the counted instantiations are general ones");
    if constexpr (!sw::lean) { S.mis = P.mis; S.field = P.field; S.field_object = P.field_object; }      // (lean: make_view's -1 / -1, the PathTracer)
    S.intensity = P.intensity; S.d_intensity = P.d_intensity;
    if (MODE == 1 && sw::adj_w(P) != nullptr && P.lds_acc) {
        // reverse mode of the primary-edge term: 8.4 M samples add into a 42 x 4 table - accumulate per workgroup in LDS
        float *acc = scratch_base<LDS>(smem, T);
        for (int i = threadIdx.x; i < 4 * P.n_prim; i += kBlock) acc[i] = 0.f;
        __syncthreads();
        PathParams Q = P;
        Q.g_prim = acc;
        run_paths_any<AD, LDS, COUNT, MODE, VAR>(S, cam, Q);
        __syncthreads();
        for (int i = threadIdx.x; i < 4 * P.n_prim; i += kBlock) if (acc[i] != 0.f) atomicAdd(&P.g_prim[i], acc[i]);
    } else {
        run_paths_any<AD, LDS, COUNT, MODE, VAR>(S, cam, P);
    }
    if (COUNT) flush_counters(S, ctr);
#if PSDR_DIAG == 13
    if (!COUNT && MODE == 0) flush_counters(S, ctr);      // (the census of paths.h)
#elif PSDR_DIAG == 14
    if (!COUNT && MODE == 1) flush_counters(S, ctr);      // (the census of the side switch, paths.h)
#endif
}

// reverse mode of the interior term (adjoint.h)
#ifndef PSDR_ADJ_REC_LDS        // measurement knob: 1 = the per-lane records stay in LDS whenever they fit 160 KB (rounds 2-4)
#define PSDR_ADJ_REC_LDS 0
#endif
// waves per SIMD of the interior adjoint kernels.  Class 2 (BVH scenes): 2 - with the per-lane records in global memory two workgroups fit a CU (40 KB of traversal
// rows + the hot accumulators <= 80 KB), and at <= 256 registers both run: config 5's interior adjoint 46.0 -> 29.3 ms.  The other classes keep the compiler's choice.
#ifndef PSDR_ADJ_WAVES
#define PSDR_ADJ_WAVES(cls) ((cls) == 2 ? 2 : 1)
#endif
#ifndef PSDR_SEC_ADJ_WAVES
#define PSDR_SEC_ADJ_WAVES 1
#endif
#ifndef PSDR_SEC_HOT_MAX        // triangle rows the secondary-edge adjoint keeps in LDS on large scenes (9 floats each)
#define PSDR_SEC_HOT_MAX 256
#endif
template <int LDS>
__global__ __launch_bounds__(kBlock, PSDR_ADJ_WAVES(LDS)) void k_interior_adjoint(const float4 *__restrict__ blob, const SceneTables T, const SensorDev cam,
                                                             const AdjointParams P) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    SceneView<LDS> S = make_view<LDS>(blob, T, smem);
    S.mis = P.mis; S.field = P.field; S.field_object = P.field_object; S.intensity = P.intensity; S.d_intensity = P.d_intensity; S.uv_adj = P.g_uv_xf != nullptr;
    if constexpr (!has_mat(LDS)) { if (P.sweep) { run_interior_adjoint_sweep<LDS>(S, cam, P, scratch_base<LDS>(smem, T)); return; } }
    run_interior_adjoint<LDS>(S, cam, P, scratch_base<LDS>(smem, T));
}

// the material sweep (adjoint_mat.h) in a kernel of its own: its registers are not shared with the record-and-probe form
template <int LDS>
__global__ __launch_bounds__(kBlock) void k_interior_adjoint_mat(const float4 *__restrict__ blob, const SceneTables T, const SensorDev cam,
                                                                 const AdjointParams P) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    SceneView<LDS> S = make_view<LDS>(blob, T, smem);
    S.mis = P.mis; S.field = P.field; S.field_object = P.field_object; S.intensity = P.intensity; S.d_intensity = P.d_intensity; S.uv_adj = P.g_uv_xf != nullptr;
    run_interior_adjoint_sweep_mat<LDS>(S, cam, P, scratch_base<LDS>(smem, T));
}

struct GuidingDev {          // HyperCubeDistribution<3>, reference src/core/cube_distrb.cpp:10-64
    const float *pmf, *cmf;
    const int *guide;        // search bounds per sample bucket (shade.h::sample_reuse_guided), [guide_n + 1]; guide_n = 0: none
    int guide_n;
    float sum;
    int reso[3], num_cells;
    float unit[3];
};

PSDR_DEV float guiding_sample_reuse(const GuidingDev &G, Vec3f &s) {
    float pdf;
    const int idx = sample_reuse_guided<true>(G.guide, G.guide_n, G.num_cells, G.sum, [&](int i) { return G.pmf[i]; }, [&](int i) { return G.cmf[i]; }, s.z, pdf);
    const int c0 = idx / (G.reso[1] * G.reso[2]);
    const int rem = idx - c0 * (G.reso[1] * G.reso[2]);
    const int c1 = rem / G.reso[2], c2 = rem - c1 * G.reso[2];
    s.x = (s.x + (float) c0) * G.unit[0];
    s.y = (s.y + (float) c1) * G.unit[1];
    s.z = (s.z + (float) c2) * G.unit[2];
    return pdf * (float) G.num_cells;
}

// secondary-edge term, reference path.cpp:274-294.
// Only ~1 in 6 boundary-segment samples of the README scene passes the cheap validity test of
// sample_boundary_segment_direct (silhouette condition + light facing), and only those trace rays.  Each lane
// therefore keeps drawing candidates (RNG seed + three draws + the validity test, no ray) until the wave holds
// enough valid ones, and the traced part (3 rays) runs with nearly all lanes active (stage r01a: 17 %).
// waves per SIMD of the secondary-edge kernel (forward): its candidate rounds are chains of dependent loads, so it wants occupancy - measured on
// config 5 (class 2) 2 / 3 / 4 waves: 48.6 / 38.3 / 33.2 ms (the compiler's own choice was 2), on C3 (class 1) 3 / 4 / 5: 0.79 / 0.72 / 0.76 ms, on the
// Microfacet box (class 3) 0.83 -> 0.75 ms, on the glossy bunny under the ballroom map (class 0) 1.85 -> 1.52 ms; the reverse-mode instantiation keeps
// the compiler's choice (1 = no constraint; 2-4 measured: +1-3 %)
#ifndef PSDR_SEC_WAVES
#define PSDR_SEC_WAVES 4
#endif
// SQ (forward mode, uncounted): a sample's square goes to P.dsq where the sample goes to P.dout (psdr_hip_render_d_fwd_sq).  A compile-time switch, so the plain
// instantiations are the code they were (their names gain the fourth argument)
template <int LDS, bool COUNT, bool ADJ, bool SQ = false>
__global__ __launch_bounds__(kBlock, (ADJ ? PSDR_SEC_ADJ_WAVES : PSDR_SEC_WAVES)) void k_secondary_edges(
                                                            const float4 *__restrict__ blob, const SceneTables T, const SecEdgeTables E,
                                                            const SensorDev cam, const PathParams P, const GuidingDev G, const int use_guiding,
                                                            Counters *ctr) {
    static_assert(!(SQ && (ADJ || COUNT)), "the squares exist in forward mode, uncounted");
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    SceneView<LDS> S = make_view<LDS>(blob, T, smem);
    const int lane_id = threadIdx.x & 63;
    const unsigned long long lt_mask = (1ull << lane_id) - 1ull;
    long long q_next = 0, q_end = 0;
    bool exhausted = false;
    bool have = false;
    BoundarySegSampleDirect bss;
    bss.valid = false; bss.pdf = 1.f; bss.p0 = Vec3d(Dual(0.f)); bss.edge = bss.edge2 = bss.p2 = bss.n = Vec3f(0.f); bss.emitter_slot = -1; bss.edge_id = 0; bss.s1 = 0.f;
    float pdf0 = 1.f;
    // reverse mode (adj_layout.h): the three recorded hits of a lane; the camera-pose adjoint, 12 entries every sample adds to; `hot_acc`: both tables
    // (lds_acc: g_sec and g_tri point into it) or the hot triangles' rows
    float *sec_recs = nullptr, *acc_cam = nullptr, *hot_acc = nullptr, *g_sec = P.g_sec, *g_tri = P.g_tri;
    if constexpr (ADJ) {
        float *scratch = scratch_base<LDS>(smem, T);
        const SecAdjLdsLayout L = sec_adj_lds_layout(P.lds_acc != 0, P.n_sec, T.n_tris, P.n_hot);
        sec_recs = scratch + L.rec; acc_cam = scratch + L.cam; hot_acc = scratch + L.acc;
        if (P.lds_acc) { g_sec = scratch + L.sec; g_tri = scratch + L.tri; }
        for (int i = threadIdx.x; i < L.total - L.acc; i += kBlock) hot_acc[i] = 0.f;
        if (P.g_cam != nullptr && threadIdx.x < 16) acc_cam[threadIdx.x] = 0.f;
        __syncthreads();
    }
    // Candidates: one in six passes the silhouette / light-facing test.
    auto draw = [&](long long item, BoundarySegSampleDirect &out, float &pdf_out) -> bool {
        const long long chunk = (item >> 8) * P.shard_count + P.shard_rank;
        const long long lane = P.begin + (chunk << 8) + (item & 255);
        if (lane >= P.end) return false;
        LaneRng rng;
        rng.seed(P.seed + (unsigned long long) lane, (unsigned long long) lane, P.skip);
        Vec3f s3;
        s3.x = rng.next_1d(); s3.y = rng.next_1d(); s3.z = rng.next_1d();
        pdf_out = use_guiding ? guiding_sample_reuse(G, s3) : 1.f;
        out = sample_boundary_segment_direct<LDS>(S, E, s3);
        return out.valid;
    };
    auto refill_queue = [&]() {
        if (q_next >= q_end && !exhausted) {
            unsigned long long base = 0;
            if (lane_id == 0) base = atomicAdd(P.counter, (unsigned long long) kFetchBatch);
            base = __shfl(base, 0);
            if ((long long) base >= P.n_local) exhausted = true;
            else { q_next = (long long) base; q_end = q_next + kFetchBatch < P.n_local ? q_next + kFetchBatch : P.n_local; }
        }
    };
    // reverse mode, closed form: the tangent is value0 . n.(e1 du + e2 dv) with (u, v) = Moeller-Trumbore(emitter triangle; x1, sd), sd = normalize(p0 - x1)
    // and x1 = the camera ray's hit sliding along that ray - two adjoint solves instead of 21-33 replays
    auto scatter_closed = [&](int idx, const SecAdjInfo &I, const BoundarySegSampleDirect &seg, float pdf_seg) {
        if constexpr (ADJ) {
            const float v0c[3] = {I.value0.x, I.value0.y, I.value0.z};
            float gsum = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float k = P.adj_w[3 * (long long) idx + c];
                if (pdf_seg > kEpsilon) k /= pdf_seg;
                if (T.sppse > 1) k /= (float) T.sppse;
                if (finite_(v0c[c])) gsum += k * v0c[c];
            }
            if (gsum != 0.f && finite_(gsum)) {
                auto add3 = [&](float *tab, int row, const Vec3f &val) {
                    if (val.x != 0.f && finite_(val.x)) atomicAdd(&tab[row], val.x);
                    if (val.y != 0.f && finite_(val.y)) atomicAdd(&tab[row + 1], val.y);
                    if (val.z != 0.f && finite_(val.z)) atomicAdd(&tab[row + 2], val.z);
                };
                // triangle rows: hot ones per workgroup in LDS (config 5: 93 -> 42 ms; 51 of the 93 were the scatter, most of it the 108 floats of the scene box)
                auto add_tri = [&](int orig, int comp, const Vec3f &val) {
                    const int hot = (!P.lds_acc && P.n_hot > 0) ? P.hot_map[orig] : -1;
                    if (hot >= 0 && hot < P.n_hot) add3(hot_acc, 9 * hot + comp, val); else add3(g_tri, 22 * orig + comp, val);
                };
                Vec3f a2, b2, c2, a1, b1, c1;
                load_geom<false, LDS>(S, I.slot2, a2, b2, c2);
                load_geom<false, LDS>(S, I.slot1, a1, b1, c1);
                Vec3f p0b, e1b, e2b, ob, db;
                mt_adjoint(a2, b2, c2, I.x1, I.sd, gsum * dot(I.n, b2), gsum * dot(I.n, c2), 0.f, p0b, e1b, e2b, ob, db);
                const int orig2 = __float_as_int(S.ld(T.shade_off + 6 * I.slot2 + 3).w), orig1 = __float_as_int(S.ld(T.shade_off + 6 * I.slot1 + 3).w);
                add_tri(orig2, 0, p0b); add_tri(orig2, 3, e1b); add_tri(orig2, 6, e2b);
                const Vec3f q = detach(seg.p0) - I.x1;
                const Vec3f qb = (db - I.sd * dot(I.sd, db)) / norm(q);          // through sd = normalize(p0 - x1)
                add3(g_sec, 6 * seg.edge_id, qb); add3(g_sec, 6 * seg.edge_id + 3, qb * seg.s1);
                const Vec3f xb = ob - qb;                                         // the camera hit x1 = o + t d
                Vec3f p0c, e1c, e2c, oc2, dc2;
                mt_adjoint(a1, b1, c1, I.cam_o, I.cam_d, 0.f, 0.f, dot(I.cam_d, xb), p0c, e1c, e2c, oc2, dc2);
                add_tri(orig1, 0, p0c); add_tri(orig1, 3, e1c); add_tri(orig1, 6, e2c);
                if (P.g_cam != nullptr) {
                    const float t1 = dot(I.x1 - I.cam_o, I.cam_d);
                    const Vec3f obt = xb + oc2, dbt = xb * t1 + dc2;
                    const Vec3f pc = xform_pos(cam.sample_to_camera, Vec3f(I.qx, I.qy, 0.f));
                    const Vec3f o_cam = cam.ortho ? pc : Vec3f(0.f), d_cam = cam.ortho ? Vec3f(0.f, 0.f, 1.f) : normalize(pc);
                    const float occ[4] = {o_cam.x, o_cam.y, o_cam.z, 1.f}, dcc[4] = {d_cam.x, d_cam.y, d_cam.z, 0.f};
                    const float obv[3] = {obt.x, obt.y, obt.z}, dbv[3] = {dbt.x, dbt.y, dbt.z};
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const float val = obv[r] * occ[c] + dbv[r] * dcc[c];
                            if (val != 0.f && finite_(val)) atomicAdd(&acc_cam[4 * r + c], val);
                        }
                }
            }
        }
    };
    // THE PIPELINED FORM (round 6; forward mode and the closed-form reverse mode).  A valid segment costs three rays, each of which can end it: the ray to its emitter
    // sample, the opposite ray to the surface point p1 the sensor sees it on, the camera ray through p1.  Traced one ray at a time by the lanes that still hold a segment
    // (eval_boundary_segment), the three traversals of a wave run at 58, ~40 and ~25 of 64 lanes, each with the tail of its slowest walk: lane utilisation 0.29 on the
    // 82 k-triangle scene of config 5.  Here a lane's segment is in one of two stages - FIRST RAYS (the emitter ray, which may stop at any occluder in front of the sample,
    // and the opposite ray, posted TOGETHER: the second one is speculative, and wasted when the first fails) and CAMERA RAY - and every call of trace2 carries the rays of
    // ALL lanes, whatever their stage: a lane whose segment ended takes the next candidate in the same iteration.  Candidates: every lane draws in every round, the indices
    // of the valid ones (one in six) wait in a per-wave pool in LDS (a segment is a function of its item's index); the pool sits in rows the traversal uses - stack rows of
    // BVH scenes, the cold path-state rows of brute-force scenes - so what is left of it rides in a register across a trace (fewer than 64 entries by construction).
    constexpr int kPoolCap = 192;            // < 64 needed + <= 64 new per round
    const bool pooled = T.stack_depth >= kPoolCap / 64 && P.n_local < (1ll << 31);
    // (BVH scenes.  Brute-force scenes keep round 5's form - the pool, then the three rays one after the other: their trace2 pays for a speculative second ray in full,
    //  C3's kernel 0.60 -> 0.62 ms pipelined)
    const bool pipelined = pooled && T.n_tris > kBruteForceMax && (!ADJ || P.sec_closed);
    lds_uint_t *pool_base = (lds_uint_t *) (S.stack - threadIdx.x) + (threadIdx.x & ~63);
    // entry i of this wave's pool: row i / 64 of the area, in the wave's OWN 64 columns - the rows are per-lane rows of all four waves (traversal stacks, parked rays), and
    // another wave may be in the middle of a trace while this one collects candidates
    auto pool_at = [&](int i) -> lds_uint_t & { return pool_base[(i >> 6) * kBlock + (i & 63)]; };
    int pool_n = 0;
    if (pipelined) {
        int stage = 0;
        unsigned spare = 0u;
        Hit h2, h1c;
        h2.slot = -1; h2.u = h2.v = h2.t = 0.f; h1c = h2;
        Vec3f p1(0.f);
        if constexpr (ADJ) { S.mode = 0; S.probe_kind = 99; S.probe_id = -1; }          // (zero tangents everywhere: only the primal factors are wanted)
        for (;;) {
            // ---- candidates for the lanes without a segment
            const int n_need = __popcll(__ballot(stage == 0));
            while (pool_n < n_need) {
                refill_queue();
                if (q_next >= q_end) break;
                const long long item = q_next + lane_id;
                bool ok = false;
                if (item < q_end) { BoundarySegSampleDirect tmp; float tpdf; ok = draw(item, tmp, tpdf); }
                const unsigned long long m_ok = __ballot(ok);
                if (ok) pool_at(pool_n + __popcll(m_ok & lt_mask)) = (unsigned) item;
                pool_n += __popcll(m_ok);
                const long long left = q_end - q_next;
                q_next += left < 64 ? left : 64;
            }
            wave_sync();
            {
                const unsigned long long m_need = __ballot(stage == 0);
                const int n_take = pool_n < n_need ? pool_n : n_need, rank = __popcll(m_need & lt_mask);
                if (stage == 0 && rank < n_take) {
                    if (draw((long long) pool_at(pool_n - n_take + rank), bss, pdf0)) stage = 1;
                    if constexpr (ADJ) bss.p0 = promote(detach(bss.p0));
                }
                pool_n -= n_take;
                if (lane_id < pool_n) spare = pool_at(lane_id);
            }
            wave_sync();
            if (__ballot(stage != 0) == 0ull) { if (exhausted && q_next >= q_end && pool_n == 0) break; continue; }
            // ---- the rays of every lane's stage in one call
            const Vec3f p0v = detach(bss.p0), dirv = normalize(bss.p2 - p0v);
            Vec3f oB = p0v, dB = -dirv;
            SensorDirectSample sds; sds.valid = false; sds.qx = sds.qy = 0.f; sds.pixel_idx = -1; sds.sensor_val = 0.f;
            RayT<true> camera_ray; camera_ray.o = Vec3d(Dual(0.f)); camera_ray.d = Vec3d(Dual(0.f));
            if (stage == 2) {
                sec_camera_sample<true>(T, cam, p1, sds, camera_ray, -1);
                oB = detach(camera_ray.o); dB = detach(camera_ray.d);
            }
            Hit hA, hB;
            // (the emitter ray only has to know whether its closest hit lies at the sample: any hit clearly in front of it settles that - as the next-event rays of the paths)
            trace2<LDS, COUNT>(S, p0v, dirv, stage == 1, oB, dB, stage != 0, hA, hB, (norm(bss.p2 - p0v) - kShadowEpsilon) * 0.9999f);
            if (lane_id < pool_n) pool_at(lane_id) = spare;
            wave_sync();
            if (stage == 1) {
                stage = 0;
                RayT<false> r2; r2.o = p0v; r2.d = dirv;
                if (COUNT) { if (hA.slot >= 0) S.c_hits++; if (hB.slot >= 0) S.c_hits++; }
                const Its<false> its2 = make_its<false, LDS, true>(S, hA, r2, false);
                if (sec_light_hit_ok(S, its2, bss.p2) && hB.slot >= 0) {
                    RayT<false> r1; r1.o = p0v; r1.d = -dirv;
                    const Its<false> its1c = make_its<false, LDS, true>(S, hB, r1, false);
                    SensorDirectSample s1; RayT<true> c1;
                    if (its1c.valid && sec_camera_sample<true>(T, cam, its1c.p, s1, c1, -1)) { stage = 2; h2 = hA; h1c = hB; p1 = its1c.p; }
                }
            } else if (stage == 2) {
                stage = 0;
                RayT<false> r2; r2.o = p0v; r2.d = dirv;
                RayT<false> r1; r1.o = p0v; r1.d = -dirv;
                if (COUNT) { if (hB.slot >= 0) S.c_hits++; }
                const Its<false> its2 = make_its<false, LDS, true>(S, h2, r2, false);
                const Its<false> its1c = make_its<false, LDS, true>(S, h1c, r1, false);
                const Its<true> its1 = make_its<true, LDS, true>(S, hB, camera_ray, false);
                Vec3f v;
                SecAdjInfo I;
                const int idx = sec_value<true, LDS>(S, bss, its2, its1c, its1, camera_ray, sds, v, ADJ ? &I : nullptr);
                if (idx >= 0) {
                    if constexpr (ADJ) scatter_closed(idx, I, bss, pdf0);
                    else {
                        float o[3] = {v.x, v.y, v.z};
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            if (pdf0 > kEpsilon) o[c] /= pdf0;
                            if (T.sppse > 1) o[c] /= (float) T.sppse;
                            if (finite_(o[c]) && o[c] != 0.f) {
                                atomicAdd(&P.dout[3 * (long long) idx + c], o[c]);
                                if constexpr (SQ) atomicAdd(&P.dsq[3 * (long long) idx + c], o[c] * o[c]);
                            }
                        }
                    }
                }
            }
        }
        if constexpr (ADJ) { S.mode = 0; S.probe_kind = 0; }
    } else
    for (;;) {
        if (pooled && T.n_tris <= kBruteForceMax) {
            // brute-force scenes (round 5): every lane draws in every round, the valid items' indices wait in the pool, a wave's worth is taken at a time
            while (pool_n < 64) {
                refill_queue();
                if (q_next >= q_end) break;
                const long long item = q_next + lane_id;
                bool ok = false;
                if (item < q_end) { BoundarySegSampleDirect tmp; float tpdf; ok = draw(item, tmp, tpdf); }
                const unsigned long long m_ok = __ballot(ok);
                if (ok) pool_at(pool_n + __popcll(m_ok & lt_mask)) = (unsigned) item;
                pool_n += __popcll(m_ok);
                const long long left = q_end - q_next;
                q_next += left < 64 ? left : 64;
            }
            wave_sync();
            const int n_take = pool_n < 64 ? pool_n : 64;
            have = false;
            if (lane_id < n_take) have = draw((long long) pool_at(pool_n - n_take + lane_id), bss, pdf0);
            pool_n -= n_take;
            wave_sync();
            if (n_take == 0) { if (exhausted && q_next >= q_end) break; continue; }
        } else {
        for (int round = 0; round < 16; ++round) {
            const unsigned long long need = __ballot(!have);
            if (__popcll(need) <= 6) break;
            refill_queue();
            if (q_next >= q_end) break;
            const int rank = __popcll(need & lt_mask);
            const long long item = q_next + rank;
            if (!have && item < q_end) have = draw(item, bss, pdf0);
            const int n_need = __popcll(need);
            q_next += n_need < (int) (q_end - q_next) ? n_need : (q_end - q_next);
        }
        if (__ballot(have) == 0ull) { if (exhausted && q_next >= q_end) break; continue; }
        }
        if constexpr (ADJ) if (have) {
            // reverse mode: record the three rays once, then probe the quantities the tangent is linear in
            float *rec = sec_recs + threadIdx.x;
            S.rec = rec; S.mode = 1; S.rec_n = 0; S.rec_i = 0; S.probe_kind = 0;
            BoundarySegSampleDirect b0 = bss;
            b0.p0 = promote(detach(bss.p0));
            Vec3f v;
            if (P.sec_closed) {
                S.mode = 0; S.probe_kind = 99; S.probe_id = -1;         // (zero tangents everywhere: only the primal factors are wanted)
                SecAdjInfo I;
                const int idx = eval_boundary_segment<true, LDS, false>(S, cam, b0, v, -1, &I);
                if (idx >= 0) scatter_closed(idx, I, bss, pdf0);
                S.mode = 0; S.probe_kind = 0;
                have = false;
                continue;
            }
            const int idx = eval_boundary_segment<true, LDS, false>(S, cam, b0, v);
            if (idx >= 0) {
                float w3[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float k = P.adj_w[3 * (long long) idx + c];
                    if (pdf0 > kEpsilon) k /= pdf0;
                    if (T.sppse > 1) k /= (float) T.sppse;
                    w3[c] = k;
                }
                S.mode = 2;
                // (probe kind 99 matches nothing: the replays see zero tangents except the one the probe sets - with kind 0 the
                // snapshot's FORWARD tangents of the triangles would leak into the adjoint of the edge point)
                S.probe_kind = 99; S.probe_id = -1;
                auto probe = [&](const BoundarySegSampleDirect &b) -> float {
                    S.rec_i = 0;
                    Vec3f t;
                    const int id = eval_boundary_segment<true, LDS, false>(S, cam, b, t);
                    if (id < 0) return 0.f;
                    float g = 0.f;
                    if (finite_(t.x)) g += w3[0] * t.x;
                    if (finite_(t.y)) g += w3[1] * t.y;
                    if (finite_(t.z)) g += w3[2] * t.z;
                    return g;
                };
                for (int c = 0; c < 3; ++c) {
                    BoundarySegSampleDirect bp = b0;
                    if (c == 0) bp.p0.x.d = 1.f; else if (c == 1) bp.p0.y.d = 1.f; else bp.p0.z.d = 1.f;
                    const float g = probe(bp);
                    if (g != 0.f) { atomicAdd(&g_sec[6 * bss.edge_id + c], g); atomicAdd(&g_sec[6 * bss.edge_id + 3 + c], bss.s1 * g); }
                }
                for (int which = 0; which < 3; which += 2) {       // hit 0: emitter triangle, hit 2: camera-ray triangle
                    const int slot = __float_as_int(rec[4 * which * kBlock]);
                    if (slot < 0) continue;
                    const int orig = __float_as_int(S.ld(T.shade_off + 6 * slot + 3).w);
                    S.probe_kind = 1; S.probe_id = slot;
                    for (int comp = 0; comp < 9; ++comp) {
                        S.probe_comp = comp;
                        const float g = probe(b0);
                        if (g != 0.f) atomicAdd(&g_tri[22 * orig + comp], g);
                    }
                    S.probe_kind = 99;
                }
                if (P.g_cam != nullptr)                            // the camera ray through p1 moves with the pose (path.cpp:214)
                    for (int comp = 0; comp < 12; ++comp) {
                        S.rec_i = 0;
                        Vec3f t;
                        const int id = eval_boundary_segment<true, LDS, false>(S, cam, b0, t, comp);
                        if (id < 0) continue;
                        float g = 0.f;
                        if (finite_(t.x)) g += w3[0] * t.x;
                        if (finite_(t.y)) g += w3[1] * t.y;
                        if (finite_(t.z)) g += w3[2] * t.z;
                        if (g != 0.f) atomicAdd(&acc_cam[comp], g);
                    }
            }
            S.mode = 0; S.probe_kind = 0;
            have = false;
        }
        if (have) {
            Vec3f v;
            const int idx = eval_boundary_segment<true, LDS, COUNT>(S, cam, bss, v);
            if (idx >= 0) {
                float o[3] = {v.x, v.y, v.z};
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (pdf0 > kEpsilon) o[c] /= pdf0;
                    if (T.sppse > 1) o[c] /= (float) T.sppse;
                    if (finite_(o[c]) && o[c] != 0.f) {
                        atomicAdd(&P.dout[3 * (long long) idx + c], o[c]);
                        if constexpr (SQ) atomicAdd(&P.dsq[3 * (long long) idx + c], o[c] * o[c]);
                    }
                }
            }
            have = false;
        }
    }
    if constexpr (ADJ) if (P.g_cam != nullptr) {
        __syncthreads();
        if (threadIdx.x < 12 && acc_cam[threadIdx.x] != 0.f) atomicAdd(&P.g_cam[threadIdx.x], acc_cam[threadIdx.x]);
    }
    if constexpr (ADJ) if (P.lds_acc) {
        __syncthreads();
        for (int i = threadIdx.x; i < 6 * P.n_sec; i += kBlock) if (g_sec[i] != 0.f) atomicAdd(&P.g_sec[i], g_sec[i]);
        for (int i = threadIdx.x; i < 22 * T.n_tris; i += kBlock) if (g_tri[i] != 0.f) atomicAdd(&P.g_tri[i], g_tri[i]);
    } else if (P.n_hot > 0) {
        __syncthreads();
        for (int i = threadIdx.x; i < 9 * P.n_hot; i += kBlock) if (hot_acc[i] != 0.f) atomicAdd(&P.g_tri[22 * P.hot_inv[i / 9] + i % 9], hot_acc[i]);
    }
    if (COUNT) flush_counters(S, ctr);
}

// ------------------------------------------------------------------------------------------------
// the small kernel templates: no unit instantiates them explicitly, the host unit does where it launches them (api.hip)
// guiding grid: PathTracer::preprocess_secondary_edges, reference path.cpp:130-168 (one round per launch)
template <int LDS>
__global__ __launch_bounds__(kBlock) void k_guiding_round(const float4 *__restrict__ blob, const SceneTables T, const SecEdgeTables E,
                                                          const SensorDev cam, const GuidingDev G, const int per_cell, const int seed,
                                                          const int round, float *__restrict__ mass) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    SceneView<LDS> S = make_view<LDS>(blob, T, smem);
    const long long n = (long long) G.num_cells * per_cell;
    const long long n_chunks = (n + kBlock - 1) / kBlock;
    for (long long chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const long long lane = chunk * kBlock + threadIdx.x;
        if (lane < n) {
            const int cell = (int) (lane / per_cell);
            const int c0 = cell / (G.reso[1] * G.reso[2]);
            const int rem = cell - c0 * (G.reso[1] * G.reso[2]);
            const int c1 = rem / G.reso[2], c2 = rem - c1 * G.reso[2];
            LaneRng rng;
            rng.seed((unsigned long long) lane + (unsigned long long) (long long) seed, (unsigned long long) lane, (unsigned long long) (3 * round));
            Vec3f s3;
            s3.x = rng.next_1d(); s3.y = rng.next_1d(); s3.z = rng.next_1d();
            s3 = Vec3f((s3.x + (float) c0) * G.unit[0], (s3.y + (float) c1) * G.unit[1], (s3.z + (float) c2) * G.unit[2]);
            Vec3f v;
            eval_secondary_edge<false, LDS, false>(S, E, cam, s3, v);
            float o[3] = {v.x, v.y, v.z};
#pragma unroll
            for (int c = 0; c < 3; ++c) { if (!finite_(o[c])) o[c] = 0.f; if (per_cell > 1) o[c] /= (float) per_cell; }
            const float m = fmaxf(o[0], fmaxf(o[1], o[2]));
            if (m != 0.f) atomicAdd(&mass[cell], m);
        }
    }
}

// batch closest-hit query (parity aid for the traversal alone)
template <int LDS>
__global__ __launch_bounds__(kBlock) void k_trace(const float4 *__restrict__ blob, const SceneTables T, int n, const float *__restrict__ o,
                                                  const float *__restrict__ d, int *__restrict__ out_tri, float *__restrict__ out_uv, float *__restrict__ out_t,
                                                  int pairs) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    SceneView<LDS> S = make_view<LDS>(blob, T, smem);
    if (pairs) {
        // lane i carries rays 2i and 2i+1 through the two-ray path (trace2) that the path kernels use
        const long long np = ((long long) n + 1) / 2;
        for (long long i = (long long) blockIdx.x * kBlock + threadIdx.x; i < ((np + kBlock - 1) / kBlock) * kBlock; i += (long long) gridDim.x * kBlock) {
            const long long ia = 2 * i, ib = 2 * i + 1;
            const bool actA = ia < n, actB = ib < n;
            const long long ja = actA ? ia : 0, jb = actB ? ib : 0;
            Hit hA, hB;
            trace2<LDS, false>(S, Vec3f(o[3 * ja], o[3 * ja + 1], o[3 * ja + 2]), Vec3f(d[3 * ja], d[3 * ja + 1], d[3 * ja + 2]), actA,
                               Vec3f(o[3 * jb], o[3 * jb + 1], o[3 * jb + 2]), Vec3f(d[3 * jb], d[3 * jb + 1], d[3 * jb + 2]), actB, hA, hB);
            if (actA) { out_tri[ia] = hA.slot >= 0 ? __float_as_int(S.ld(T.trav_off + 3 * hA.slot + 2).y) : -1; out_uv[2 * ia] = hA.u; out_uv[2 * ia + 1] = hA.v; out_t[ia] = hA.t; }
            if (actB) { out_tri[ib] = hB.slot >= 0 ? __float_as_int(S.ld(T.trav_off + 3 * hB.slot + 2).y) : -1; out_uv[2 * ib] = hB.u; out_uv[2 * ib + 1] = hB.v; out_t[ib] = hB.t; }
        }
        return;
    }
    for (long long i = (long long) blockIdx.x * kBlock + threadIdx.x; i < (long long) ((n + kBlock - 1) / kBlock) * kBlock; i += (long long) gridDim.x * kBlock) {
        if (i < n) {
            const Hit h = trace<LDS, false>(S, Vec3f(o[3 * i], o[3 * i + 1], o[3 * i + 2]), Vec3f(d[3 * i], d[3 * i + 1], d[3 * i + 2]));
            int id = -1;
            if (h.slot >= 0) id = __float_as_int(S.ld(T.trav_off + 3 * h.slot + 2).y);
            out_tri[i] = id; out_uv[2 * i] = h.u; out_uv[2 * i + 1] = h.v; out_t[i] = h.t;
        }
    }
}

// Scene::ray_intersect<false> for a batch of rays (the reference exposes it as Scene.unit_ray_intersect, psdr.cpp:404):
// 24 floats per ray - valid, mesh id, t, J, p, n (geometric), sh_frame.s/t/n, wi (local), uv
template <int LDS>
__global__ __launch_bounds__(kBlock) void k_intersect(const float4 *__restrict__ blob, const SceneTables T, int n, const float *__restrict__ o,
                                                      const float *__restrict__ d, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    SceneView<LDS> S = make_view<LDS>(blob, T, smem);
    for (long long i = (long long) blockIdx.x * kBlock + threadIdx.x; i < (long long) ((n + kBlock - 1) / kBlock) * kBlock; i += (long long) gridDim.x * kBlock) {
        if (i < n) {
            RayT<false> r;
            r.o = Vec3f(o[3 * i], o[3 * i + 1], o[3 * i + 2]); r.d = Vec3f(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
            const Hit h = trace<LDS, false>(S, r.o, r.d);
            const Its<false> its = make_its<false, LDS, true>(S, h, r, false);
            float *q = out + 24 * i;
            if (!its.valid) { for (int k = 0; k < 24; ++k) q[k] = 0.f; q[1] = -1.f; continue; }
            // its.uv = bilinear2(uv0, uv1 - uv0, uv2 - uv0, barycentrics), scene.cpp:756-759 (the path kernels keep it only when a texture needs it)
            const float4 c = S.ld(T.shade_off + 6 * its.slot + 4), e = S.ld(T.shade_off + 6 * its.slot + 5);
            const float tu = fma_(c.z - c.x, h.u, fma_(e.x - c.x, h.v, c.x)), tv = fma_(c.w - c.y, h.u, fma_(e.y - c.y, h.v, c.y));
            const float v[24] = {1.f, (float) its.mesh, its.t, its.J, its.p.x, its.p.y, its.p.z, its.n.x, its.n.y, its.n.z,
                                 its.fs.x, its.fs.y, its.fs.z, its.ft.x, its.ft.y, its.ft.z, its.fn.x, its.fn.y, its.fn.z,
                                 its.wi.x, its.wi.y, its.wi.z, tu, tv};
            for (int k = 0; k < 24; ++k) q[k] = v[k];
        }
    }
}

// Scene::ray_intersect<true> for a batch of rays (Scene.unit_ray_intersectAD, reference psdr.cpp:405, scene.cpp:774-797): the record of
// k_intersect from the differentiable re-intersection of the hit triangle (isect_ad.h), its forward tangent (rays' tangents d_o / d_d, NULL =
// zero; triangle rows' tangents = the scene's installed tangent rows) when out_d is given, and the hit's slot (-1 = miss) for k_intersect_adj
template <int LDS>
__global__ __launch_bounds__(kBlock) void k_intersect_ad(const float4 *__restrict__ blob, const SceneTables T, int n, const float *__restrict__ o,
                                                         const float *__restrict__ d, const float *__restrict__ d_o, const float *__restrict__ d_d,
                                                         float *__restrict__ out, float *__restrict__ out_d, int *__restrict__ out_hit) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    SceneView<LDS> S = make_view<LDS>(blob, T, smem);
    for (long long i = (long long) blockIdx.x * kBlock + threadIdx.x; i < (long long) ((n + kBlock - 1) / kBlock) * kBlock; i += (long long) gridDim.x * kBlock) {
        if (i < n) {
            const Vec3f ro(o[3 * i], o[3 * i + 1], o[3 * i + 2]), rd(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
            const Hit h = trace<LDS, false>(S, ro, rd);
            float *q = out + 24 * i;
            float *qd = out_d ? out_d + 24 * i : nullptr;
            out_hit[i] = h.slot;
            if (h.slot < 0) {
                for (int k = 0; k < 24; ++k) q[k] = 0.f;
                q[1] = -1.f;
                if (qd) for (int k = 0; k < 24; ++k) qd[k] = 0.f;
                continue;
            }
            const Vec3f to = d_o ? Vec3f(d_o[3 * i], d_o[3 * i + 1], d_o[3 * i + 2]) : Vec3f(0.f);
            const Vec3f td = d_d ? Vec3f(d_d[3 * i], d_d[3 * i + 1], d_d[3 * i + 2]) : Vec3f(0.f);
            IsectGeom<Dual> g;
            IsectConst c;
            isect_load<true, LDS>(S, h.slot, g, c);
            IsectOut<Dual> r;
            isect_ad_eval<Dual>(make_dual(ro, to), make_dual(rd, td), g, c, r);
            const Dual rec[22] = {r.t, Dual(1.f), r.p.x, r.p.y, r.p.z, g.fn.x, g.fn.y, g.fn.z, r.fs.x, r.fs.y, r.fs.z, r.ft.x, r.ft.y, r.ft.z,
                                  r.fn.x, r.fn.y, r.fn.z, r.wi.x, r.wi.y, r.wi.z, r.tu, r.tv};
            q[0] = 1.f; q[1] = (float) c.mesh;
            for (int k = 0; k < 22; ++k) q[2 + k] = rec[k].v;
            if (qd) { qd[0] = 0.f; qd[1] = 0.f; for (int k = 0; k < 22; ++k) qd[2 + k] = rec[k].d; }
        }
    }
}

#ifndef PSDR_ISECT_ADJ_ROUNDS     // wave reductions per 64 rays before the lanes left over add their own rows (tools/time_intersect_ad.py, LABNOTES.md:
#define PSDR_ISECT_ADJ_ROUNDS 16  // C3 camera rays 14.96 / 2.67 / 0.40 / 0.40 ms at 0 / 2 / 4 / 16 rounds, config-5 random rays 15.6 / 10.3 / 7.5 / 3.7 ms)
#endif
// The transpose of k_intersect_ad from the saved hit slots (no traversal): per ray the adjoints of o and d (plain stores), and the adjoints of
// the hit triangle's row [p0 e1 e2 n0 n1 n2 face_normal] added into g_tri[orig * 22 + ...] (ORIGINAL triangle order, psdr_grads.g_triangles).
// Camera-like batches put most rays of a wave on one or two triangles: per round the wave takes the row of its first pending lane, sums the
// 21 components over the lanes that share it (butterfly shuffles) and one lane adds them; after `rounds` rounds the lanes still pending (a
// wave of incoherent rays: little contention) add their rows with one atomic per component.  rounds = 0: per-lane atomics only.
template <int LDS>
__global__ __launch_bounds__(kBlock) void k_intersect_adj(const float4 *__restrict__ blob, const SceneTables T, int n, const float *__restrict__ o,
                                                          const float *__restrict__ d, const int *__restrict__ hit, const float *__restrict__ g_rec,
                                                          const unsigned char *__restrict__ mesh_filter, float *__restrict__ g_tri,
                                                          float *__restrict__ g_o, float *__restrict__ g_d, int rounds) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    const float4 *B = blob;
    if (in_lds(LDS)) {
        for (int k = threadIdx.x; k < T.blob_words; k += kBlock) smem[k] = blob[k];
        __syncthreads();
        B = smem;
    }
    const int lane = threadIdx.x & 63;
    for (long long i = (long long) blockIdx.x * kBlock + threadIdx.x; i < (long long) ((n + kBlock - 1) / kBlock) * kBlock; i += (long long) gridDim.x * kBlock) {
        bool pend = false;
        int row = -1;
        float gt[kIsectRowComps];
#pragma unroll
        for (int k = 0; k < kIsectRowComps; ++k) gt[k] = 0.f;
        if (i < n) {
            const int slot = hit[i];
            Vec3f go(0.f), gd(0.f);
            if (slot >= 0 && slot < T.n_tris) {           // (a slot outside the scene's range is not loaded)
                float gr[24];
                bool any = false;
#pragma unroll
                for (int k = 0; k < 24; ++k) { gr[k] = g_rec[24 * i + k]; if (!finite_(gr[k])) gr[k] = 0.f; }
#pragma unroll
                for (int k = 2; k < 24; ++k) any = any || (k != 3 && gr[k] != 0.f);
                if (any) {
                    const int w = T.trav_off + 3 * slot, ws = T.shade_off + 6 * slot;
                    const float4 a = B[w], b = B[w + 1], cc = B[w + 2];
                    const float4 s0 = B[ws], s1 = B[ws + 1], s2 = B[ws + 2], s3 = B[ws + 3], s4 = B[ws + 4], s5 = B[ws + 5];
                    IsectGeom<float> g;
                    g.p0 = Vec3f(a.x, a.y, a.z); g.e1 = Vec3f(a.w, b.x, b.y); g.e2 = Vec3f(b.z, b.w, cc.x);
                    g.n0 = Vec3f(s0.x, s0.y, s0.z); g.n1 = Vec3f(s1.x, s1.y, s1.z); g.n2 = Vec3f(s2.x, s2.y, s2.z); g.fn = Vec3f(s3.x, s3.y, s3.z);
                    IsectConst c;
                    c.uv[0] = s4.x; c.uv[1] = s4.y; c.uv[2] = s4.z; c.uv[3] = s4.w; c.uv[4] = s5.x; c.uv[5] = s5.y;
                    c.flat = (__float_as_int(s2.w) & 1) != 0;
                    c.mesh = __float_as_int(s1.w);
                    isect_ad_adjoint(Vec3f(o[3 * i], o[3 * i + 1], o[3 * i + 2]), Vec3f(d[3 * i], d[3 * i + 1], d[3 * i + 2]), g, c, gr, gt, go, gd);
                    if (!finite_(go.x)) go.x = 0.f;
                    if (!finite_(go.y)) go.y = 0.f;
                    if (!finite_(go.z)) go.z = 0.f;
                    if (!finite_(gd.x)) gd.x = 0.f;
                    if (!finite_(gd.y)) gd.y = 0.f;
                    if (!finite_(gd.z)) gd.z = 0.f;
                    const bool wanted = g_tri != nullptr && c.mesh >= 0 && c.mesh < T.n_meshes && (mesh_filter == nullptr || mesh_filter[c.mesh] != 0);
                    row = __float_as_int(cc.y);                 // the original triangle id (k_trace)
                    if (wanted && row >= 0 && row < T.n_tris) {
                        pend = true;
#pragma unroll
                        for (int k = 0; k < kIsectRowComps; ++k) if (!finite_(gt[k])) gt[k] = 0.f;
                    }
                }
            }
            if (g_o) { g_o[3 * i] = go.x; g_o[3 * i + 1] = go.y; g_o[3 * i + 2] = go.z; }
            if (g_d) { g_d[3 * i] = gd.x; g_d[3 * i + 1] = gd.y; g_d[3 * i + 2] = gd.z; }
        }
        // every lane of the wave is here (the loop runs over whole blocks): wave-wide reductions of the lanes that share a row
        for (int r = 0; r < rounds; ++r) {
            const unsigned long long m = __ballot(pend);
            if (m == 0ull) break;
            const int leader = __ffsll((long long) m) - 1;
            const int lead_row = __builtin_amdgcn_readlane(row, leader);
            const bool mine = pend && row == lead_row;
#pragma unroll
            for (int k = 0; k < kIsectRowComps; ++k) {
                float x = mine ? gt[k] : 0.f;
                for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
                if (lane == leader && x != 0.f && finite_(x)) atomicAdd(&g_tri[(long long) lead_row * 22 + k], x);
            }
            pend = pend && !mine;
        }
        if (pend) {
#pragma unroll
            for (int k = 0; k < kIsectRowComps; ++k) if (gt[k] != 0.f) atomicAdd(&g_tri[(long long) row * 22 + k], gt[k]);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Split build (psdr_jit_amd/build.py): the heavy kernel templates of each scene class are instantiated in translation units of
// their own - render_units.hip compiled with -DPSDR_TU=1..10, kernels only - and compiled in parallel; the host unit (api.hip: host
// code + the small kernels) declares those instantiations extern.  PSDR_TU<k>() defines list k, PSDR_TU<k>(extern) declares it.
#define PSDR_INST_PATHS_V(PFX, AD_, C_, CNT_, M_, V_) PFX template __global__ void k_paths<AD_, C_, CNT_, M_, V_>(const float4 *, const SceneTables, const SensorDev, const PathParams, Counters *);
#define PSDR_INST_PATHS(PFX, AD_, C_, CNT_, M_) PSDR_INST_PATHS_V(PFX, AD_, C_, CNT_, M_, kGeneral)
#define PSDR_INST_LEAN3(PFX, C_) PSDR_INST_PATHS_V(PFX, true, C_, false, 0, kLean) PSDR_INST_PATHS_V(PFX, false, C_, false, 0, kLean) PSDR_INST_PATHS_V(PFX, false, C_, false, 1, kLean)
#define PSDR_INST_ADJ(PFX, C_) PFX template __global__ void k_interior_adjoint<C_>(const float4 *, const SceneTables, const SensorDev, const AdjointParams);
#define PSDR_INST_ADJM(PFX, C_) PFX template __global__ void k_interior_adjoint_mat<C_>(const float4 *, const SceneTables, const SensorDev, const AdjointParams);
#define PSDR_INST_SEC(PFX, C_, CNT_, ADJ_) PFX template __global__ void k_secondary_edges<C_, CNT_, ADJ_, false>(const float4 *, const SceneTables, const SecEdgeTables, const SensorDev, const PathParams, const GuidingDev, const int, Counters *);
#define PSDR_INST_SEC_SQ(PFX, C_) PFX template __global__ void k_secondary_edges<C_, false, false, true>(const float4 *, const SceneTables, const SecEdgeTables, const SensorDev, const PathParams, const GuidingDev, const int, Counters *);
#define PSDR_INST_PATHS6(PFX, C_) PSDR_INST_PATHS(PFX, true, C_, false, 0) PSDR_INST_PATHS(PFX, false, C_, false, 0) PSDR_INST_PATHS(PFX, false, C_, false, 1) \
                                  PSDR_INST_PATHS(PFX, true, C_, true, 0) PSDR_INST_PATHS(PFX, false, C_, true, 0) PSDR_INST_PATHS(PFX, false, C_, true, 1)
#define PSDR_TU1(PFX) PSDR_INST_PATHS(PFX, true, 0, false, 0) PSDR_INST_PATHS(PFX, false, 0, false, 0) PSDR_INST_PATHS(PFX, false, 0, false, 1)
#define PSDR_TU6(PFX) PSDR_INST_PATHS(PFX, true, 0, true, 0) PSDR_INST_PATHS(PFX, false, 0, true, 0) PSDR_INST_PATHS(PFX, false, 0, true, 1) PSDR_INST_SEC_SQ(PFX, 0)
#define PSDR_TU2(PFX) PSDR_INST_ADJ(PFX, 0) PSDR_INST_SEC(PFX, 0, false, false) PSDR_INST_SEC(PFX, 0, true, false) PSDR_INST_SEC(PFX, 0, false, true)
#define PSDR_TU8(PFX) PSDR_INST_ADJM(PFX, 0)         // the material sweep, a unit of its own for the same reason as PSDR_TU7: its not-inlined bsdf_back lambda shows the allocator defect
#define PSDR_TU3(PFX) PSDR_INST_PATHS6(PFX, 1) PSDR_INST_ADJ(PFX, 1) PSDR_INST_SEC(PFX, 1, false, false) PSDR_INST_SEC(PFX, 1, true, false) PSDR_INST_SEC(PFX, 1, false, true)
#define PSDR_TU4(PFX) PSDR_INST_PATHS6(PFX, 2) PSDR_INST_SEC(PFX, 2, false, false) PSDR_INST_SEC(PFX, 2, true, false) PSDR_INST_SEC(PFX, 2, false, true)
#define PSDR_TU7(PFX) PSDR_INST_ADJ(PFX, 2)          // a unit of its own: when the ISA lint sends it to the second allocator (build.py), the class-2 path kernels do not pay for it
// the lean path kernels (paths.h::Switches) of the classes that have them: 1 (the Cornell boxes) and 2 (BVH scenes), the uncounted instantiations
// (the secondary-edge kernel with the squares, k_secondary_edges<C, false, false, true>, rides in the shortest unit of each class: 6, 9, 10 and 5)
#define PSDR_TU9(PFX) PSDR_INST_LEAN3(PFX, 1) PSDR_INST_SEC_SQ(PFX, 1)
#define PSDR_TU10(PFX) PSDR_INST_LEAN3(PFX, 2) PSDR_INST_SEC_SQ(PFX, 2)
#define PSDR_TU5(PFX) PSDR_INST_PATHS(PFX, true, 3, false, 0) PSDR_INST_PATHS(PFX, false, 3, false, 0) PSDR_INST_PATHS(PFX, false, 3, false, 1) PSDR_INST_SEC(PFX, 3, false, false) PSDR_INST_SEC_SQ(PFX, 3)
