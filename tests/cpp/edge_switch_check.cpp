// Stand-alone check of the primary-edge term's side switch (psdr_jit_amd/csrc/hip/edge_switch.h; host code only, g++ alone - tests/test_edge_switch_cpu.py).
//
// Plays the loop of paths.h::run_paths (MODE 1) for ONE lane and one edge sample in both schedules - the late switch (the counted kernels: the second path's first
// vertex is built by a make_its of its own at the bottom of the loop) and the early switch (the decision of edge_switch.h ahead of the loop's one make_its) - with a
// stub for the shading that records, per path of the sample,
//   the first-vertex builds (which hit, from which origin), the sampler draws (the stream position of each), the skip_levels arguments, and the radiance handed on
// for max_depth 0 ... 4 and every way each of the two paths can end: the camera ray misses; an invalid BSDF sample or a miss at each depth; a last hit on a non-emitter
// and on an emitter; with and without emitters at the camera hit and at the hits in between.  Asserts
//   same record      both schedules draw, skip, build and hand on the same
//   one build        a path's first vertex is built exactly once (never for a camera ray that missed), and in the early schedule no vertex is built that nobody reads
//   pending          the early schedule takes the one-iteration detour exactly where needs_itx is set
//   ends             every lane leaves the loop, after the late schedule's iterations plus one per detour
#include "psdr_jit_amd/csrc/hip/edge_switch.h"

#include <cstdio>
#include <vector>

using namespace psdr;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++fails <= 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

constexpr int kCamOrigin = 1000;          // the sensor's position (every other origin is the slot of the vertex a ray leaves)
constexpr int kDrawsPerLevel = 5;

struct Hit { int slot = -1; bool emitter = false; };

// one path of the sample: its camera ray, then `n_ext` extension rays that hit, then how it ends
enum End { kRunsOut = 0, kBsdfInvalid = 1, kMiss = 2 };
struct PathSpec { bool cam_hit, cam_emitter; int n_ext; End end; bool mid_emitter, last_emitter; };

struct Scene {
    int max_depth;
    PathSpec path[2];
    Hit camera(int side) const {
        Hit h;
        if (path[side].cam_hit) { h.slot = side * 100; h.emitter = path[side].cam_emitter; }
        return h;
    }
    // the extension ray of vertex `depth`: is the BSDF sample valid, and what does its ray hit
    bool extension(int side, int depth, Hit &h) const {
        const PathSpec &p = path[side];
        h = Hit();
        if (depth < p.n_ext) { h.slot = side * 100 + depth + 1; h.emitter = depth + 1 >= max_depth ? p.last_emitter : p.mid_emitter; return true; }
        return p.end != kBsdfInvalid;
    }
};

static double Le(const Hit &h) { return h.slot >= 0 && h.emitter ? 1.0 + 0.5 * h.slot : 0.0; }

struct Record {
    struct Build { int slot, origin; };
    std::vector<Build> first_builds[2];       // first vertices built from a hit
    std::vector<long long> draws[2];          // the stream position of every draw
    std::vector<int> skips[2];                // skip_levels(nd, k) as nd * 100 + k
    double handed[2] = {-1.0, -1.0};          // Ln as parked, Lp as accumulated
    int handed_n[2] = {0, 0};
    int iterations = 0, pending = 0, builds = 0, builds_unread = 0;
    bool ended = false;
};

template <bool EARLY> static Record play(const Scene &sc) {
    Record rec;
    const int max_depth = sc.max_depth;
    // the lane's state (paths.h::run_paths); side 2 = switched, the parked hit not handed to make_its yet
    bool busy = true, trace_p = true;
    int depth = -1, side = 0, origin = kCamOrigin;
    long long rng = 0;
    double thr = 1.0, res = 0.0;
    Hit its, parked;
    auto draw = [&](int path) { rec.draws[path].push_back(rng); return (double) (rng++ % 97) * 0.001; };
    auto skip_levels = [&](int path, int nd, int k) { rec.skips[path].push_back(nd * 100 + k); rng += (long long) nd * k; };
    auto hand_on = [&](int path, double v) { rec.handed[path] = v; rec.handed_n[path]++; };

    for (int it = 0; busy; ++it) {
        if (it > 4 * (max_depth + 4)) break;
        rec.iterations++;
        const int path = side == 0 ? 0 : 1;
        // [A] next-event estimation, [B] the extension ray
        const bool at_vertex = depth >= 0;
        bool bs_valid = true;
        Hit hx;
        if (at_vertex) {
            const double sx = draw(path), sy = draw(path);
            if (!its.emitter) res += thr * (sx + 2.0 * sy);
            draw(path); draw(path); draw(path);
            bs_valid = sc.extension(side, depth, hx);
            origin = its.slot;
            if (!bs_valid) hx = Hit();
        } else if (side != 2) {
            hx = sc.camera(side);
        }
        if (trace_p) { parked = sc.camera(1); trace_p = false; }

        if (EARLY) {
            bool switch_now = false;
            if (side == 2) switch_now = true;
            else if (side == 0) {
                const bool hit = hx.slot >= 0;
                const bool emitter = es_last_hit(depth, max_depth, bs_valid, hit) && hx.emitter;
                const EdgeSwitch es = es_path_end(depth, max_depth, bs_valid, hit, emitter);
                if (es.ends && !es.needs_itx) {
                    hand_on(0, res);
                    const int d_end = es_end_depth(depth);
                    if (d_end < max_depth) skip_levels(0, kDrawsPerLevel, max_depth - d_end);
                    thr = 1.0; res = 0.0; depth = -1;
                    switch_now = true;
                }
            }
            if (switch_now) { side = 1; origin = kCamOrigin; hx = parked; }
        }

        // the loop's one make_its, and the vertex block
        bool finished = false;
        const int built_for = side == 0 ? 0 : 1;
        const Hit itx = hx;
        if (itx.slot >= 0) rec.builds++;
        if (depth < 0) {
            if (itx.slot >= 0) rec.first_builds[built_for].push_back({itx.slot, origin});
            its = itx;
            res = Le(itx);
            depth = 0;
            finished = itx.slot < 0 || max_depth == 0;
        } else if (bs_valid && itx.slot >= 0) {
            thr *= 0.5 + 0.01 * itx.slot;
            res += Le(itx) * thr * 0.75;
            // (a last hit off the emitters: the vertex is built and nothing of it is read)
            if (depth + 1 >= max_depth && !itx.emitter) rec.builds_unread++;
            its = itx;
            depth += 1;
            finished = depth >= max_depth;
        } else {
            depth += 1;
            finished = true;
        }

        if (finished) {
            bool sample_done = side == 1;
            if (side == 0) {
                hand_on(0, res);
                if (depth < max_depth) skip_levels(0, kDrawsPerLevel, max_depth - depth);
                thr = 1.0; res = 0.0; depth = -1;
                if (EARLY) { side = 2; rec.pending++; }
                else {
                    side = 1; origin = kCamOrigin;
                    const Hit itp = parked;
                    if (itp.slot >= 0) { rec.builds++; rec.first_builds[1].push_back({itp.slot, origin}); }
                    its = itp;
                    res = Le(itp);
                    depth = 0;
                    sample_done = itp.slot < 0 || max_depth == 0;
                }
            }
            if (sample_done) { hand_on(1, res); busy = false; }
        }
    }
    rec.ended = !busy;
    return rec;
}

static std::vector<PathSpec> all_paths(int max_depth) {
    std::vector<PathSpec> out;
    out.push_back({false, false, 0, kRunsOut, false, false});                        // the camera ray misses
    for (int cam_e = 0; cam_e < 2; ++cam_e) {
        if (max_depth == 0) { out.push_back({true, cam_e != 0, 0, kRunsOut, false, false}); continue; }
        for (int mid_e = 0; mid_e < 2; ++mid_e) {
            for (int k = 0; k < max_depth; ++k) {                                    // ends at vertex k
                out.push_back({true, cam_e != 0, k, kBsdfInvalid, mid_e != 0, false});
                out.push_back({true, cam_e != 0, k, kMiss, mid_e != 0, false});
            }
            out.push_back({true, cam_e != 0, max_depth, kRunsOut, mid_e != 0, false});     // a last hit off the emitters
            out.push_back({true, cam_e != 0, max_depth, kRunsOut, mid_e != 0, true});      // ... and on one
        }
    }
    return out;
}

int main() {
    // the decision itself, exhaustively against its definition
    for (int max_depth = 0; max_depth <= 4; ++max_depth)
        for (int depth = -1; depth < (max_depth > 0 ? max_depth : 1); ++depth)
            for (int m = 0; m < 8; ++m) {
                const bool bs_valid = m & 1, hit = m & 2, emitter = m & 4;
                const EdgeSwitch es = es_path_end(depth, max_depth, bs_valid, hit, emitter);
                bool ends, needs;
                if (depth < 0) { ends = !(bs_valid && hit) || max_depth == 0; needs = bs_valid && hit && max_depth == 0; }
                else { ends = !(bs_valid && hit) || depth + 1 >= max_depth; needs = bs_valid && hit && depth + 1 >= max_depth && emitter; }
                CHECK(es.ends == ends && es.needs_itx == needs, "es_path_end(%d, %d, %d, %d, %d) = %d, %d", depth, max_depth, bs_valid, hit, emitter, es.ends, es.needs_itx);
                CHECK(!es.needs_itx || es.ends, "needs_itx without ends");
                CHECK(es_end_depth(depth) == (depth < 0 ? 0 : depth + 1), "es_end_depth(%d)", depth);
            }

    long long cases = 0, detours = 0;
    for (int max_depth = 0; max_depth <= 4; ++max_depth) {
        const std::vector<PathSpec> paths = all_paths(max_depth);
        for (size_t a = 0; a < paths.size(); ++a)
            for (size_t b = 0; b < paths.size(); ++b) {
                Scene sc;
                sc.max_depth = max_depth; sc.path[0] = paths[a]; sc.path[1] = paths[b];
                const Record late = play<false>(sc), early = play<true>(sc);
                ++cases;
#define WHERE "max_depth %d, paths %zu / %zu"
#define AT max_depth, a, b
                CHECK(late.ended && early.ended, "a lane did not end: " WHERE, AT);
                for (int p = 0; p < 2; ++p) {
                    CHECK(late.draws[p] == early.draws[p], "draws of path %d differ: " WHERE, p, AT);
                    CHECK(late.skips[p] == early.skips[p], "skip_levels of path %d differ: " WHERE, p, AT);
                    CHECK(late.handed_n[p] == 1 && early.handed_n[p] == 1, "path %d handed on %d / %d times: " WHERE, p, late.handed_n[p], early.handed_n[p], AT);
                    CHECK(late.handed[p] == early.handed[p], "radiance of path %d: %.17g / %.17g: " WHERE, p, late.handed[p], early.handed[p], AT);
                    const size_t want = sc.path[p].cam_hit ? 1 : 0;
                    CHECK(late.first_builds[p].size() == want && early.first_builds[p].size() == want, "first-vertex builds of path %d: %zu / %zu: " WHERE, p,
                          late.first_builds[p].size(), early.first_builds[p].size(), AT);
                    if (late.first_builds[p].size() == want && early.first_builds[p].size() == want && want == 1) {
                        CHECK(late.first_builds[p][0].slot == p * 100 && late.first_builds[p][0].origin == kCamOrigin, "late first vertex of path %d: " WHERE, p, AT);
                        CHECK(early.first_builds[p][0].slot == p * 100 && early.first_builds[p][0].origin == kCamOrigin, "early first vertex of path %d: " WHERE, p, AT);
                    }
                    // every level's draws are taken or skipped: the stream ends at 2 paths x 5 x max_depth whatever the paths did
                    long long used = (long long) late.draws[p].size();
                    for (int s : late.skips[p]) used += (long long) (s / 100) * (s % 100);
                    if (p == 0) CHECK(used == (long long) kDrawsPerLevel * max_depth, "path 0 leaves the stream at %lld: " WHERE, used, AT);
                }
                // the detour: exactly where the first path's last vertex is read
                const PathSpec &p0 = sc.path[0];
                const bool needs = p0.cam_hit && (max_depth == 0 || (p0.end == kRunsOut && p0.last_emitter));
                CHECK(early.pending == (needs ? 1 : 0), "pending %d, wanted %d: " WHERE, early.pending, (int) needs, AT);
                CHECK(late.pending == 0, "late schedule pending");
                CHECK(early.iterations == late.iterations + early.pending, "iterations %d / %d: " WHERE, late.iterations, early.iterations, AT);
                // the early schedule builds no vertex of the first path that nobody reads, and never more vertices than the late one
                const bool p0_unread = p0.cam_hit && max_depth > 0 && p0.end == kRunsOut && !p0.last_emitter;
                const bool p1_unread = sc.path[1].cam_hit && max_depth > 0 && sc.path[1].end == kRunsOut && !sc.path[1].last_emitter;
                CHECK(late.builds_unread == (int) p0_unread + (int) p1_unread, "late unread builds %d: " WHERE, late.builds_unread, AT);
                CHECK(early.builds_unread == (int) p1_unread, "early unread builds %d: " WHERE, early.builds_unread, AT);
                CHECK(early.builds == late.builds - (int) p0_unread, "builds %d / %d: " WHERE, late.builds, early.builds, AT);
                detours += early.pending;
            }
    }
    if (fails) { std::printf("%d check(s) failed\n", fails); return 1; }
    std::printf("OK %lld samples in both schedules, %lld detours\n", cases, detours);
    return 0;
}
