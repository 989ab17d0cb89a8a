// Stand-alone check of the interior term's start bookkeeping (psdr_jit_amd/csrc/hip/group_start.h; host code only, g++ alone - tests/test_group_start_cpu.py).
//
// Plays the loop of paths.h::run_paths (MODE 0, live-pixel hand-out) for the waves of a launch on the host - 64 lanes each, one shared queue counter, random path
// lengths (0 = the camera ray misses: the lane is idle again at once), random live masks - with the decision and the queue arithmetic the kernel calls:
//   once, in order    every live position is handed to exactly one lane, no dead one to any; a wave's positions go out in increasing order, lower lanes first
//   fills             a grouped start (G > 1) leaves an idle lane empty only when the launch's queue is exhausted
//   ends              every wave leaves its loop, within the iterations its positions and path lengths allow; nobody waits on a start that cannot come
//   G = 1             the schedule of the lane-by-lane form: at most three windows per start, no fetch inside a start
// for every threshold of the sweep, queues of 0 ... 1 000 positions (as they are and padded with dead positions to the fetch batch) and live fractions 0 ... 1.
#include "psdr_jit_amd/csrc/hip/group_start.h"

#include <cstdio>
#include <random>
#include <vector>

using namespace psdr;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++fails <= 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

constexpr int kBatch = 256;

struct Launch {
    std::vector<unsigned char> live;      // per queue position
    std::vector<int> handed;              // how often a position was handed out
    long long n_local = 0;
    unsigned long long counter = 0;       // the launch's queue head
};

struct Wave {
    long long q_next = 0, q_end = 0;
    bool exhausted = false, done = false;
    bool busy[64] = {};
    int left[64] = {};                    // loop bodies the lane's path still takes
    long long last = -1;                  // the last position this wave handed out
    long long iters = 0, bodies = 0, starts = 0, started = 0;
};

static void fetch(Launch &L, Wave &w) {
    const unsigned long long base = L.counter;
    L.counter += kBatch;
    gs_fetched(base, L.n_local, kBatch, w.q_next, w.q_end, w.exhausted);
}

// paths.h::take_live_items_fill for the 64 lanes of a wave: item[l] = the position lane l takes, -1 = none
static void take(Launch &L, Wave &w, bool fill, long long item[64], int &windows, int &fetches) {
    for (int l = 0; l < 64; ++l) item[l] = -1;
    windows = 0; fetches = 0;
    for (int win = 0; fill || win < 3; ++win) {
        unsigned long long want = 0ull;
        for (int l = 0; l < 64; ++l) if (!w.busy[l] && item[l] < 0) want |= 1ull << l;
        if (want == 0ull) break;
        if (w.q_next >= w.q_end) {
            if (fill && !w.exhausted) { fetch(L, w); ++fetches; }
            if (w.q_next >= w.q_end) break;
        }
        const int wlen = gs_window_len(w.q_next, w.q_end);
        CHECK(wlen >= 1 && wlen <= 64, "window of %d positions", wlen);
        unsigned long long lv = 0ull;
        for (int l = 0; l < wlen; ++l) if (L.live[(size_t) (w.q_next + l)]) lv |= 1ull << l;
        for (int l = 0; l < 64; ++l)
            if ((want >> l) & 1ull) { const int p = gs_lane_pick(lv, want, (1ull << l) - 1ull); if (p >= 0) item[l] = w.q_next + p; }
        const int used = gs_window_used(lv, gs_popc(want), wlen);
        CHECK(used >= 1 && used <= wlen, "a window of %d positions uses up %d", wlen, used);
        // nothing live is left behind the queue's head
        for (int l = 0; l < used; ++l)
            if ((lv >> l) & 1ull) { bool taken = false; for (int k = 0; k < 64; ++k) taken |= item[k] == w.q_next + l; CHECK(taken, "live position %lld skipped", w.q_next + l); }
        w.q_next += used;
        ++windows;
    }
}

// one iteration of run_paths' loop
static void step(Launch &L, Wave &w, int G, std::mt19937 &rng, const int len_weights[4]) {
    ++w.iters;
    if (w.q_next >= w.q_end && !w.exhausted) fetch(L, w);
    int n_idle = 0;
    for (int l = 0; l < 64; ++l) n_idle += !w.busy[l];
    if (gs_start_now(n_idle, 64 - n_idle, G, w.q_next < w.q_end)) {
        ++w.starts;
        long long item[64];
        int windows, fetches;
        take(L, w, G > 1, item, windows, fetches);
        if (G == 1) CHECK(windows <= 3 && fetches == 0, "lane-by-lane start with %d windows, %d fetches", windows, fetches);
        std::discrete_distribution<int> len(len_weights, len_weights + 4);
        int n_got = 0;
        for (int l = 0; l < 64; ++l) {
            if (item[l] < 0) continue;
            CHECK(!w.busy[l], "a busy lane took position %lld", item[l]);
            CHECK(item[l] > w.last, "position %lld after %lld", item[l], w.last);
            w.last = item[l];
            CHECK(item[l] < L.n_local && L.live[(size_t) item[l]], "dead position %lld handed out", item[l]);
            if (item[l] < L.n_local) L.handed[(size_t) item[l]]++;
            w.left[l] = len(rng);
            w.busy[l] = w.left[l] > 0;
            ++n_got; ++w.started;
        }
        if (G > 1 && n_got < n_idle) CHECK(w.exhausted && w.q_next >= w.q_end, "a grouped start filled %d of %d idle lanes with work left", n_got, n_idle);
    }
    int n_busy = 0;
    for (int l = 0; l < 64; ++l) n_busy += w.busy[l];
    if (n_busy == 0) { if (w.exhausted && w.q_next >= w.q_end) w.done = true; return; }
    ++w.bodies;
    for (int l = 0; l < 64; ++l) if (w.busy[l] && --w.left[l] == 0) w.busy[l] = false;
}

static void play(int G, long long n, bool pad, double live_frac, int n_waves, unsigned seed, const int len_weights[4]) {
    std::mt19937 rng(seed);
    Launch L;
    L.n_local = pad ? (n + kBatch - 1) / kBatch * kBatch : n;
    L.live.assign((size_t) L.n_local, 0);
    L.handed.assign((size_t) L.n_local, 0);
    long long n_live = 0;
    std::uniform_real_distribution<double> U(0.0, 1.0);
    for (long long i = 0; i < n; ++i) { L.live[(size_t) i] = live_frac >= 1.0 || U(rng) < live_frac; n_live += L.live[(size_t) i]; }
    std::vector<Wave> waves((size_t) n_waves);
    // every iteration of a wave that is not its last either consumes a position, runs a body (at most 3 per started sample) or fetches: a generous bound
    const long long bound = 16 + 8 * L.n_local + 4 * n_waves;
    long long total = 0;
    for (bool any = true; any && total <= bound;) {
        any = false;
        for (auto &w : waves) {
            if (w.done) continue;
            // (waves advance in a random interleaving: the hand-out may not depend on who fetches first)
            const int burst = 1 + (int) (rng() % 3u);
            for (int b = 0; b < burst && !w.done; ++b) { step(L, w, G, rng, len_weights); ++total; }
            any = true;
        }
    }
    bool all_done = true;
    for (auto &w : waves) all_done &= w.done;
    CHECK(all_done, "G %d, %lld positions, live %.3f, %d waves: the loop did not end within %lld iterations", G, n, live_frac, n_waves, bound);
    long long once = 0;
    for (long long i = 0; i < L.n_local; ++i) {
        CHECK(L.handed[(size_t) i] == (L.live[(size_t) i] ? 1 : 0), "G %d, %lld positions, live %.3f: position %lld handed out %d times (live %d)", G, n, live_frac, i,
              L.handed[(size_t) i], (int) L.live[(size_t) i]);
        once += L.handed[(size_t) i];
    }
    CHECK(once == n_live, "%lld of %lld live positions handed out", once, n_live);
    for (auto &w : waves)
        for (int l = 0; l < 64; ++l) CHECK(!w.busy[l], "a lane is left busy");
}

int main() {
    // the bit arithmetic
    std::mt19937_64 r64(5);
    for (int i = 0; i < 20000; ++i) {
        const unsigned long long m = i < 64 ? 1ull << i : (i == 64 ? ~0ull : r64() & r64());
        int seen = 0;
        for (int b = 0; b < 64; ++b)
            if ((m >> b) & 1ull) { CHECK(gs_nth_set_bit(m, seen) == b, "nth_set_bit(%llx, %d)", m, seen); ++seen; }
        CHECK(gs_popc(m) == seen, "popc(%llx)", m);
    }
    // the decision
    for (int G : {1, 16, 32, 48, 64})
        for (int idle = 0; idle <= 64; ++idle) {
            CHECK(!gs_start_now(idle, 64 - idle, G, false), "a start without positions in hand");
            CHECK(gs_start_now(idle, 64 - idle, G, true) == (idle > 0 && (idle >= G || idle == 64)), "start_now(%d idle, G %d)", idle, G);
        }
    // the loop
    const int lens[3][4] = {{1, 2, 3, 10}, {10, 1, 1, 1}, {0, 0, 0, 1}};      // weights of path lengths 0 .. 3: the box, mostly misses, every path full length
    unsigned seed = 1;
    for (int G : {1, 16, 32, 48, 64})
        for (long long n : {0ll, 1ll, 63ll, 64ll, 65ll, 255ll, 256ll, 257ll, 1000ll})
            for (double f : {0.0, 1.0 / 64.0, 0.36, 1.0})
                for (int pad = 0; pad < 2; ++pad)
                    for (int n_waves : {1, 3})
                        for (int k = 0; k < 3; ++k) play(G, n, pad != 0, f, n_waves, seed++, lens[k]);
    // a long queue with few live positions: starts that need many windows and cross batches
    for (int G : {1, 16, 64}) play(G, 20000, true, 1.0 / 200.0, 2, seed++, lens[0]);
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("OK\n");
    return 0;
}
