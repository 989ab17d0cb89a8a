// adj_layout.h — the dynamic LDS of the reverse-mode kernels behind the traversal rows (render_kernels.h::scratch_base): where every section lies, in floats, as a
// function of counts alone, and what the host decides from those sizes (adj_plan, sec_adj_plan).  The one place the launch (api.hip::render_bwd_impl) and the kernels
// (adjoint.h::adj_carve, render_kernels.h::k_secondary_edges) take the layout from.  Integers only, no HIP include: tests/cpp/adj_layout_check.cpp compiles it with g++
// and holds hand-counted cases.
//
// Interior adjoint (k_interior_adjoint, k_interior_adjoint_mat), sections in order:
//   per-lane records lane_words x 256, or none (in global memory) | misc 32 | material rows n_bsdfs x mat_row | hot triangle rows n_hot x 22
//   | BSDF colours n_bsdfs x 3 | emitter radiances n_emitters x 3 | texel adjoints of a small environment map env_lds
// Secondary-edge adjoint (k_secondary_edges<., ., true>):
//   three recorded hits 12 x 256 | camera pose 16 | the whole tables 6 n_sec + 22 n_tris, or the hot triangles' [p0 e1 e2] 9 n_hot
// Primary-edge adjoint (k_paths, MODE 1): one table 4 n_prim
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define PSDR_ADJ_HD __host__ __device__ __forceinline__
#else
#define PSDR_ADJ_HD inline
#endif

namespace psdr {

constexpr int kAdjBlock = 256;      // lanes of a workgroup (scene_dev.h::kBlock, asserted in adjoint.h)
constexpr int kAdjTriRow = 22;      // a triangle's adjoint row [p0 e1 e2 n0 n1 n2 face_normal area]
constexpr int kMatOut = 16;         // a BSDF's row of psdr_grads.g_mat
constexpr int kMatRow = 28;         // ... and of its LDS accumulator when uv transforms are differentiated: the g_mat row, then [rot, scale, tx, ty] of its three bitmaps (g_uv_xf)
// THE row width of the material accumulator, for the launch (g->g_uv_xf) and the kernels (P.g_uv_xf) alike
PSDR_ADJ_HD int adj_mat_row(bool want_uv_xf) { return want_uv_xf ? kMatRow : kMatOut; }

// the misc block: accumulators every path adds to
constexpr int kAdjMisc = 32;
constexpr int kAdjCam = 0;          // [12] camera pose: rows 0-2 of to_world
constexpr int kAdjEnvScale = 12;    // [1] environment-map scale
constexpr int kAdjEnvXf = 16;       // [11] environment from_world: rows 0-2, columns 0-2 (stride 4)
constexpr int kAdjEnvUv = 28;       // [4] the environment map's uv transform
static_assert(kAdjCam + 12 <= kAdjEnvScale && kAdjEnvScale < kAdjEnvXf && kAdjEnvXf + 11 <= kAdjEnvUv && kAdjEnvUv + 4 <= kAdjMisc, "the misc slots are disjoint");

// per-lane records of one path, sized from the path depth D by the launch: 1 + 2 D hits of 4 words, 2 D light-sample slots,
// 4 D + 4 lookups of 3 words (per vertex: the BSDF's bitmaps and, under a normal map, the nested BSDF's; per bounce: two environment lookups)
PSDR_ADJ_HD int adj_hit_words(int depth) { return 4 * (1 + 2 * depth); }
PSDR_ADJ_HD int adj_ext_words(int depth) { return 2 * depth > 2 ? 2 * depth : 2; }
PSDR_ADJ_HD int adj_lk_entries(int depth) { return 4 * depth + 4; }
// scenes without bitmap / per-vertex parameters and without an environment map make no lookups, carry no lookup record and keep more workgroups per CU
PSDR_ADJ_HD int adj_lane_words(int depth, bool with_lookups) { return adj_hit_words(depth) + adj_ext_words(depth) + (with_lookups ? 3 * adj_lk_entries(depth) : 0); }
// the reverse sweeps keep, per lane: 3 words per vertex (slot, u, v) and 11 per bounce (light sample, shadow hit, constants, throughput)
PSDR_ADJ_HD int adj_sweep_words(int depth) { return 3 * (depth + 1) + 11 * (depth > 0 ? depth : 1); }

struct AdjLdsLayout {       // float offsets from scratch_base
    int rec, misc, mat, hot, bsdf, emit, env, total;
    int mat_row;
};
// rec_lane_words: the record words per lane held in LDS (0: the records are global)
PSDR_ADJ_HD AdjLdsLayout adj_lds_layout(int rec_lane_words, int n_bsdfs, int mat_row, int n_hot, int n_emitters, int env_lds) {
    AdjLdsLayout L;
    L.mat_row = mat_row;
    L.rec = 0;                                   L.misc = L.rec + rec_lane_words * kAdjBlock;
    L.mat = L.misc + kAdjMisc;                   L.hot = L.mat + n_bsdfs * mat_row;
    L.bsdf = L.hot + n_hot * kAdjTriRow;         L.emit = L.bsdf + n_bsdfs * 3;
    L.env = L.emit + n_emitters * 3;             L.total = L.env + env_lds;
    return L;
}

// the secondary-edge adjoint records three hits per lane, followed by 16 floats of camera-pose accumulators
constexpr int kSecAdjLaneWords = 12;
constexpr int kSecAdjScratch = kSecAdjLaneWords * kAdjBlock + 16;
struct SecAdjLdsLayout {
    int rec, cam, acc, total;
    int sec, tri;       // lds_acc: the whole tables g_sec [6 n_sec] and g_tri [22 n_tris] inside `acc`; else `acc` holds 9 floats per hot triangle
};
PSDR_ADJ_HD SecAdjLdsLayout sec_adj_lds_layout(bool lds_acc, int n_sec, int n_tris, int n_hot) {
    SecAdjLdsLayout L;
    L.rec = 0; L.cam = L.rec + kSecAdjLaneWords * kAdjBlock; L.acc = kSecAdjScratch;
    L.sec = L.acc; L.tri = L.acc + (lds_acc ? 6 * n_sec : 0);
    L.total = lds_acc ? L.tri + kAdjTriRow * n_tris : L.acc + 9 * n_hot;
    return L;
}

// ---------------------------------------------------------------------------------------------------------------------------
// host: what a launch decides from these sizes
inline size_t adj_lds_bytes(size_t floats) { return 4 * floats; }
constexpr size_t kAdjLdsCap = 160 * 1024;       // the LDS of a CU: one workgroup may ask for all of it
constexpr size_t kAdjLdsTwoWg = 80 * 1024;      // ... and at half of it two workgroups fit a CU
constexpr int kAdjMinHot = 64;                  // hot triangle rows (emitters + the largest triangles) a plan keeps room for before it takes a budget
constexpr size_t kAdjEnvLdsMax = 32 * 1024;     // an environment map's texel adjoints accumulate in LDS up to this size (e.g. 64 x 32 texels)
enum AdjForm { kAdjProbe = 0, kAdjSweep = 1, kAdjSweepMat = 2 };      // AdjointParams::sweep

struct AdjPlanIn {
    size_t smem_base = 0;           // bytes in front of scratch_base: the blob (class 1) and the traversal rows
    int depth = 0, form = kAdjProbe;
    bool with_lookups = false;      // the scene can make bitmap / per-vertex / environment lookups (probe form: the lookup record)
    int n_bsdfs = 0, n_emitters = 0, n_hot = 0;     // n_hot: the scene's hot triangles
    size_t env_texels = 0;          // width x height of the environment map, 0 without one
    bool want_env = false, want_uv_xf = false;      // g_env, g_uv_xf are asked for
    bool rec_lds_knob = false;      // PSDR_ADJ_REC_LDS: the records stay in LDS whenever they fit
};
struct AdjPlan {
    const char *error = nullptr;    // not null: no launch
    int lane_words = 0, env_lds = 0, mat_row = 0, n_hot_used = 0;
    bool rec_in_lds = false;        // else the records go to a global array of the scene (any depth works, at global-memory latency)
    size_t budget = 0, smem = 0;    // bytes: what the workgroup may use, what it asks for
    AdjLdsLayout L{};
};
inline AdjPlan adj_plan(const AdjPlanIn &in) {
    AdjPlan p;
    const bool sweeps = in.form != kAdjProbe;
    p.lane_words = sweeps ? adj_sweep_words(in.depth) : adj_lane_words(in.depth, in.with_lookups);
    // a small environment map accumulates in LDS: all samples of a wave look up the same few texels, and same-address atomics in global memory serialise (sweeps only)
    if (sweeps && in.want_env && adj_lds_bytes(in.env_texels * 3) <= kAdjEnvLdsMax) p.env_lds = (int) (in.env_texels * 3);
    p.mat_row = adj_mat_row(in.want_uv_xf);
    p.error = "scene too large for the adjoint kernel's LDS accumulators";
    const size_t cap_words = kAdjLdsCap / 4;
    if ((size_t) in.n_bsdfs > cap_words || (size_t) in.n_emitters > cap_words) return p;       // (and the int arithmetic of the layout stays in range)
    const bool rec_fits_int = (size_t) p.lane_words <= cap_words / kAdjBlock;
    auto bytes = [&](bool with_rec, int n_hot) {
        return in.smem_base + adj_lds_bytes((size_t) adj_lds_layout(with_rec ? p.lane_words : 0, in.n_bsdfs, p.mat_row, n_hot, in.n_emitters, p.env_lds).total);
    };
    // the records live in LDS when they fit beside the accumulators - unless they are what keeps a SECOND workgroup off the CU: the kernels need <= 256 registers
    // (two waves per SIMD fit), and one wave per SIMD cannot hide the latency of the sweep's traces
    const bool two_wg_with_rec = rec_fits_int && bytes(true, kAdjMinHot) <= kAdjLdsTwoWg, two_wg_without = bytes(false, kAdjMinHot) <= kAdjLdsTwoWg;
    p.rec_in_lds = (two_wg_with_rec || !two_wg_without || in.rec_lds_knob) && rec_fits_int && bytes(true, kAdjMinHot) <= kAdjLdsCap;
    const size_t fixed = bytes(p.rec_in_lds, 0);
    if (fixed > kAdjLdsCap) return p;
    // two workgroups per CU when the fixed part allows it, with at least kAdjMinHot hot rows; the hot rows take what is left of the budget
    p.budget = bytes(p.rec_in_lds, kAdjMinHot) <= kAdjLdsTwoWg ? kAdjLdsTwoWg : kAdjLdsCap;
    const size_t room = (p.budget - fixed) / adj_lds_bytes(kAdjTriRow);
    p.n_hot_used = (size_t) in.n_hot < room ? in.n_hot : (int) room;
    p.L = adj_lds_layout(p.rec_in_lds ? p.lane_words : 0, in.n_bsdfs, p.mat_row, p.n_hot_used, in.n_emitters, p.env_lds);
    p.smem = in.smem_base + adj_lds_bytes((size_t) p.L.total);
    p.error = nullptr;
    return p;
}
// secondary edges: both tables in LDS when they fit 48 KB; else (closed form only: it writes p0, e1, e2) the rows of up to `hot_max` hot triangles
constexpr size_t kSecAdjTablesMax = 48 * 1024;
struct SecAdjPlan { int lds_acc = 0, n_hot = 0; size_t bytes = 0; SecAdjLdsLayout L{}; };
inline SecAdjPlan sec_adj_plan(int n_sec, int n_tris, int scene_n_hot, bool closed, int hot_max) {
    SecAdjPlan p;
    p.lds_acc = adj_lds_bytes(6 * (size_t) n_sec + kAdjTriRow * (size_t) n_tris) <= kSecAdjTablesMax ? 1 : 0;
    p.n_hot = (!p.lds_acc && closed) ? (scene_n_hot < hot_max ? scene_n_hot : hot_max) : 0;
    p.L = sec_adj_lds_layout(p.lds_acc != 0, n_sec, n_tris, p.n_hot);
    p.bytes = adj_lds_bytes((size_t) p.L.total);
    return p;
}
// primary edges: the table of 4 floats per edge accumulates in LDS up to 2048 edges
constexpr int kPrimAdjLdsMax = 2048;
inline size_t prim_adj_lds_floats(int n_prim) { return n_prim <= kPrimAdjLdsMax ? 4 * (size_t) n_prim : 0; }

} // namespace psdr
