// The LDS layout of the reverse-mode kernels and the launch's plan (psdr_jit_amd/csrc/hip/adj_layout.h) against numbers written here: offsets and sizes counted by hand
// from the per-section sizes of DESIGN.md section 4, and the plan's invariants over a grid of inputs.
// Host compile only: g++ -O2 -std=c++17 -I<repo> tests/cpp/adj_layout_check.cpp
//
// Per-section sizes in floats (4 bytes): records lane_words x 256 | misc 32 | material rows n_bsdfs x (16, or 28 with g_uv_xf) | hot rows n_hot x 22 | colours n_bsdfs x 3
// | emitters n_emitters x 3 | environment texels.  Record words per lane at depth D: the sweeps 3 (D + 1) + 11 max(D, 1); the probe form 4 (1 + 2 D) hit words
// + max(2 D, 2) light-sample slots + (scenes that make lookups) 3 (4 D + 4).  64 hot rows = 1408 floats = 5632 bytes.  80 KB = 81920, 160 KB = 163840 bytes.
#include <cstdio>
#include <cstring>

#include "psdr_jit_amd/csrc/hip/adj_layout.h"

using namespace psdr;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static bool offsets(const AdjLdsLayout &L, int rec, int misc, int mat, int hot, int bsdf, int emit, int env, int total) {
    const bool ok = L.rec == rec && L.misc == misc && L.mat == mat && L.hot == hot && L.bsdf == bsdf && L.emit == emit && L.env == env && L.total == total;
    if (!ok) std::printf("  got rec %d misc %d mat %d hot %d bsdf %d emit %d env %d total %d\n", L.rec, L.misc, L.mat, L.hot, L.bsdf, L.emit, L.env, L.total);
    return ok;
}

static void check_words_and_slots() {
    CHECK(adj_sweep_words(0) == 14 && adj_sweep_words(1) == 17 && adj_sweep_words(3) == 45 && adj_sweep_words(10) == 143);       // 3 + 11 | 6 + 11 | 12 + 33 | 33 + 110
    CHECK(adj_hit_words(3) == 28 && adj_ext_words(0) == 2 && adj_ext_words(1) == 2 && adj_ext_words(3) == 6 && adj_lk_entries(3) == 16);
    CHECK(adj_lane_words(3, false) == 34 && adj_lane_words(3, true) == 82 && adj_lane_words(1, true) == 38 && adj_lane_words(0, false) == 6);     // 28 + 6 (+ 48) | 12 + 2 + 24 | 4 + 2
    CHECK(adj_mat_row(false) == 16 && adj_mat_row(true) == 28);
    CHECK(kAdjMisc == 32 && kAdjCam == 0 && kAdjEnvScale == 12 && kAdjEnvXf == 16 && kAdjEnvUv == 28);      // camera 0..11 | scale 12 | from_world 16..26 | uv transform 28..31
    CHECK(kAdjBlock == 256 && kSecAdjLaneWords == 12 && kSecAdjScratch == 12 * 256 + 16);
    CHECK(kAdjLdsCap == 163840 && kAdjLdsTwoWg == 81920 && kAdjMinHot == 64 && kAdjEnvLdsMax == 32768);
}

static void check_plans() {
    // (a) class 1, the Cornell box at depth 3 under the sweep: 24 KB of blob + traversal rows, 5 BSDFs, 1 emitter, 36 hot triangles
    //     records 45 x 256 = 11520 floats; misc 32, materials 5 x 16 = 80, colours 15, emitters 3 -> 130 floats of fixed accumulators
    //     24576 + 4 (11520 + 130 + 1408) = 76808 <= 81920: two workgroups fit WITH the records -> they stay in LDS, budget 80 KB
    //     room (81920 - 24576 - 46600) / 88 = 122 rows >= 36: all of the scene's hot rows
    AdjPlanIn a;
    a.smem_base = 24576; a.depth = 3; a.form = kAdjSweep; a.n_bsdfs = 5; a.n_emitters = 1; a.n_hot = 36;
    AdjPlan p = adj_plan(a);
    CHECK(p.error == nullptr && p.lane_words == 45 && p.rec_in_lds && p.env_lds == 0 && p.mat_row == 16 && p.n_hot_used == 36 && p.budget == 81920);
    CHECK(offsets(p.L, 0, 11520, 11552, 11632, 11632 + 792, 12424 + 15, 12439 + 3, 12442));
    CHECK(p.smem == 24576 + 4 * 12442);

    // (b) class 2, a BVH scene with 40 KB of traversal rows at depth 3 under the sweep: 3 BSDFs, 2 emitters, 720 hot triangles
    //     fixed accumulators 32 + 48 + 9 + 6 = 95 floats = 380 bytes; with the records 40960 + 46080 + 380 + 5632 = 93052 > 81920, without 46972 <= 81920:
    //     the records are what keeps the second workgroup off -> global; budget 80 KB; room (81920 - 40960 - 380) / 88 = 461 rows
    AdjPlanIn b;
    b.smem_base = 40960; b.depth = 3; b.form = kAdjSweep; b.n_bsdfs = 3; b.n_emitters = 2; b.n_hot = 720;
    p = adj_plan(b);
    CHECK(p.error == nullptr && p.lane_words == 45 && !p.rec_in_lds && p.n_hot_used == 461 && p.budget == 81920);
    CHECK(offsets(p.L, 0, 0, 32, 80, 80 + 10142, 10222 + 9, 10231 + 6, 10237));
    CHECK(p.smem == 40960 + 4 * 10237 && p.smem <= 81920);
    //     ... with the measurement knob the records stay: 40960 + 46080 + 380 = 87420 fixed, one workgroup, room (163840 - 87420) / 88 = 868 >= 720
    b.rec_lds_knob = true;
    p = adj_plan(b);
    CHECK(p.error == nullptr && p.rec_in_lds && p.n_hot_used == 720 && p.budget == 163840);
    CHECK(offsets(p.L, 0, 11520, 11552, 11600, 11600 + 15840, 27440 + 9, 27449 + 6, 27455));

    // (c) class 0, a bitmap scene in the probe form: 4 KB of traversal rows, 2 BSDFs, 1 emitter, 100 hot triangles
    //     depth 1: 38 words = 9728 floats of records; accumulators 32 + 32 + 6 + 3 = 73 floats; 4096 + 4 (9728 + 73 + 1408) = 48932 <= 81920 -> records in LDS
    AdjPlanIn c;
    c.smem_base = 4096; c.depth = 1; c.with_lookups = true; c.form = kAdjProbe; c.n_bsdfs = 2; c.n_emitters = 1; c.n_hot = 100;
    p = adj_plan(c);
    CHECK(p.error == nullptr && p.lane_words == 38 && p.rec_in_lds && p.mat_row == 16 && p.n_hot_used == 100 && p.budget == 81920);
    CHECK(offsets(p.L, 0, 9728, 9760, 9760 + 32, 9792 + 2200, 11992 + 6, 11998 + 3, 12001));
    //     ... with g_uv_xf: 28 words per BSDF, every later section 2 x 12 = 24 floats further
    c.want_uv_xf = true;
    p = adj_plan(c);
    CHECK(p.error == nullptr && p.rec_in_lds && p.mat_row == 28 && p.n_hot_used == 100);
    CHECK(offsets(p.L, 0, 9728, 9760, 9760 + 56, 9816 + 2200, 12016 + 6, 12022 + 3, 12025));
    CHECK(p.smem == 4096 + 4 * 12025);
    //     depth 3: 82 words = 83968 bytes of records; with them 4096 + 83968 + 292 + 5632 = 93988 > 81920, without 10020 -> global; every section from 0
    c.depth = 3; c.want_uv_xf = false;
    p = adj_plan(c);
    CHECK(p.error == nullptr && p.lane_words == 82 && !p.rec_in_lds && p.n_hot_used == 100);
    CHECK(offsets(p.L, 0, 0, 32, 64, 2264, 2270, 2273, 2273) && p.smem == 4096 + 4 * 2273);
    c.want_uv_xf = true;
    p = adj_plan(c);
    CHECK(offsets(p.L, 0, 0, 32, 88, 2288, 2294, 2297, 2297) && p.smem == 4096 + 4 * 2297);
    //     a scene without lookups carries no lookup record: 34 words
    c.with_lookups = false;
    CHECK(adj_plan(c).lane_words == 34);

    // (d) a 64 x 32 environment map under a sweep (class 2, 40 KB of rows, depth 3, 1 BSDF, the map as the only emitter, 200 hot triangles, g_env wanted):
    //     2048 texels x 3 = 6144 floats = 24576 bytes <= 32 KB -> in LDS; accumulators 32 + 16 + 3 + 3 + 6144 = 6198 floats = 24792 bytes
    //     without the records 40960 + 24792 + 5632 = 71384 <= 81920 (with: 117464) -> global records, budget 80 KB, room (81920 - 65752) / 88 = 183 rows
    AdjPlanIn d;
    d.smem_base = 40960; d.depth = 3; d.form = kAdjSweep; d.n_bsdfs = 1; d.n_emitters = 1; d.n_hot = 200; d.env_texels = 64 * 32; d.want_env = true;
    p = adj_plan(d);
    CHECK(p.error == nullptr && p.env_lds == 6144 && !p.rec_in_lds && p.n_hot_used == 183);
    CHECK(offsets(p.L, 0, 0, 32, 48, 48 + 4026, 4074 + 3, 4077 + 3, 4080 + 6144) && p.smem == 40960 + 4 * 10224);
    //     the same map under the material sweep too; not in the probe form, and not when g_env is not asked for
    d.form = kAdjSweepMat; CHECK(adj_plan(d).env_lds == 6144);
    d.form = kAdjProbe; CHECK(adj_plan(d).env_lds == 0);
    d.form = kAdjSweep; d.want_env = false; CHECK(adj_plan(d).env_lds == 0);
    d.want_env = true;
    //     the bound is 32 KB = 2730 texels: 64 x 42 = 2688 texels (32256 bytes) go to LDS, one texel row more (64 x 43 = 2752 texels, 33024 bytes) does not
    d.env_texels = 64 * 42; CHECK(adj_plan(d).env_lds == 8064);
    d.env_texels = 64 * 43;
    p = adj_plan(d);
    CHECK(p.error == nullptr && p.env_lds == 0 && p.L.total == p.L.env);
    d.env_texels = 64 * 33; CHECK(adj_plan(d).env_lds == 6336);         // (one row more than 64 x 32 still fits)

    // (e) the depth at which the records no longer fit 160 KB beside the accumulators: 80 KB in front (no second workgroup either way), the sweep, 1 BSDF, 1 emitter
    //     accumulators 32 + 16 + 3 + 3 = 54 floats = 216 bytes.  Depth 5: 73 words = 74752 bytes, 81920 + 74752 + 216 + 5632 = 162520 <= 163840 -> LDS,
    //     room (163840 - 156888) / 88 = 79 rows.  Depth 6: 87 words = 89088 bytes, 176856 > 163840 -> global, room (163840 - 82136) / 88 = 928 rows
    AdjPlanIn e;
    e.smem_base = 81920; e.depth = 5; e.form = kAdjSweep; e.n_bsdfs = 1; e.n_emitters = 1; e.n_hot = 720;
    p = adj_plan(e);
    CHECK(p.error == nullptr && p.lane_words == 73 && p.rec_in_lds && p.budget == 163840 && p.n_hot_used == 79 && p.smem == 81920 + 4 * (18688 + 54 + 79 * 22));
    e.depth = 6;
    p = adj_plan(e);
    CHECK(p.error == nullptr && p.lane_words == 87 && !p.rec_in_lds && p.budget == 163840 && p.n_hot_used == 720 && p.smem == 81920 + 4 * (54 + 720 * 22));
    e.n_hot = 1000;
    CHECK(adj_plan(e).n_hot_used == 928);

    // (f) a fixed part over 160 KB: 64 KB in front, 1000 BSDFs with g_uv_xf -> 32 + 28000 + 3000 floats = 124128 bytes, 65536 + 124128 = 189664 > 163840
    AdjPlanIn f;
    f.smem_base = 65536; f.depth = 3; f.form = kAdjSweepMat; f.n_bsdfs = 1000; f.n_emitters = 0; f.n_hot = 10; f.want_uv_xf = true;
    p = adj_plan(f);
    CHECK(p.error != nullptr && std::strcmp(p.error, "scene too large for the adjoint kernel's LDS accumulators") == 0);
    f.want_uv_xf = false;         // 32 + 16000 + 3000 floats = 76128 bytes, 141664 <= 163840: fits, one workgroup, room (163840 - 141664) / 88 = 252 rows
    p = adj_plan(f);
    CHECK(p.error == nullptr && !p.rec_in_lds && p.budget == 163840 && p.n_hot_used == 10);
    f.n_bsdfs = 1 << 30;          // (counts whose sizes do not fit an int)
    CHECK(adj_plan(f).error != nullptr);
}

static void check_edges() {
    // secondary edges: 12 x 256 = 3072 floats of records | 16 camera | the tables.  100 edges, 36 triangles: 600 + 792 = 1392 floats = 5568 bytes <= 48 KB -> both in LDS
    SecAdjPlan s = sec_adj_plan(100, 36, 36, true, 256);
    CHECK(s.lds_acc == 1 && s.n_hot == 0 && s.L.rec == 0 && s.L.cam == 3072 && s.L.acc == 3088 && s.L.sec == 3088 && s.L.tri == 3688 && s.L.total == 4480 && s.bytes == 17920);
    // 948 edges, 300 triangles: 5688 + 6600 = 12288 floats = 48 KB exactly -> still in LDS; one edge more -> not
    s = sec_adj_plan(948, 300, 720, true, 256);
    CHECK(s.lds_acc == 1 && s.L.total == 3088 + 12288);
    // ... then the closed form keeps 9 floats of min(n_hot, 256) hot triangles: 720 -> 256 rows = 2304 floats; 100 -> 900 floats; the probe form keeps none
    s = sec_adj_plan(949, 300, 720, true, 256);
    CHECK(s.lds_acc == 0 && s.n_hot == 256 && s.L.acc == 3088 && s.L.tri == 3088 && s.L.total == 3088 + 2304 && s.bytes == 4 * 5392);
    s = sec_adj_plan(949, 300, 100, true, 256);
    CHECK(s.lds_acc == 0 && s.n_hot == 100 && s.L.total == 3088 + 900);
    s = sec_adj_plan(949, 300, 720, false, 256);
    CHECK(s.lds_acc == 0 && s.n_hot == 0 && s.L.total == 3088);
    s = sec_adj_plan(10, 100000000, 720, true, 256);       // (22 x 10^8 floats does not fit an int: decided in size_t)
    CHECK(s.lds_acc == 0 && s.n_hot == 256 && s.L.total == 3088 + 2304);
    CHECK(sec_adj_lds_layout(true, 100, 36, 0).total == 4480 && sec_adj_lds_layout(false, 100, 36, 7).total == 3088 + 63);
    // primary edges: 4 floats per edge up to 2048 edges
    CHECK(prim_adj_lds_floats(42) == 168 && prim_adj_lds_floats(2048) == 8192 && prim_adj_lds_floats(2049) == 0 && adj_lds_bytes(168) == 672);
}

static void check_invariants() {
    long long cases = 0;
    const size_t bases[3] = {4 * 1024, 40 * 1024, 64 * 1024};
    for (int depth = 0; depth <= 12; ++depth)
    for (int n_bsdfs = 0; n_bsdfs <= 40; ++n_bsdfs)
    for (int n_hot = 0; n_hot <= 720; ++n_hot)
    for (int uv = 0; uv < 2; ++uv)
    for (int form = 0; form < 3; ++form)
    for (int ib = 0; ib < 3; ++ib) {
        AdjPlanIn in;
        in.smem_base = bases[ib]; in.depth = depth; in.form = form; in.n_bsdfs = n_bsdfs; in.n_hot = n_hot; in.want_uv_xf = uv != 0;
        in.with_lookups = (n_bsdfs & 1) != 0; in.n_emitters = 1 + n_hot % 3; in.rec_lds_knob = (n_hot & 4) != 0;
        in.env_texels = (n_bsdfs % 4 == 3) ? 64 * 32 : 0; in.want_env = in.env_texels > 0 && (n_hot & 1);
        const AdjPlan p = adj_plan(in);
        const AdjLdsLayout &L = p.L;
        ++cases;
        bool ok = p.error == nullptr;
        ok = ok && L.rec == 0 && L.misc - L.rec == (p.rec_in_lds ? p.lane_words * 256 : 0) && L.mat - L.misc == 32 && L.hot - L.mat == n_bsdfs * (uv ? 28 : 16) &&
             L.bsdf - L.hot == p.n_hot_used * 22 && L.emit - L.bsdf == n_bsdfs * 3 && L.env - L.emit == in.n_emitters * 3 && L.total - L.env == p.env_lds;     // disjoint, in order
        ok = ok && p.mat_row == (uv ? 28 : 16) && L.mat_row == p.mat_row;
        ok = ok && p.smem == in.smem_base + 4 * (size_t) L.total;
        ok = ok && p.smem <= p.budget && p.budget <= 160 * 1024 && (p.budget == 80 * 1024 || p.budget == 160 * 1024);
        ok = ok && p.n_hot_used >= 0 && p.n_hot_used <= n_hot;
        ok = ok && p.rec_in_lds == (L.misc > L.rec);
        ok = ok && (p.env_lds == 0 || (form != kAdjProbe && in.want_env && p.env_lds == 6144));
        if (!ok) { if (failures < 20) std::printf("FAILED invariants: depth %d n_bsdfs %d n_hot %d uv %d form %d base %zu\n", depth, n_bsdfs, n_hot, uv, form, in.smem_base); ++failures; }
    }
    CHECK(cases == 13ll * 41 * 721 * 2 * 3 * 3);
}

int main() {
    check_words_and_slots();
    check_plans();
    check_edges();
    check_invariants();
    if (failures == 0) std::printf("OK\n");
    return failures == 0 ? 0 : 1;
}
