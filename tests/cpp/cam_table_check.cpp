// Stand-alone check of the camera-ray table's builder (psdr_jit_amd/csrc/hip/cam_table.h; host code only, g++ alone - tests/test_cam_table_cpu.py).
//
// Random triangles in front of a pinhole camera, frames of odd sizes:
//   conservative   a point of the frame that lies inside a triangle's image (tested in double, on a 5 x 5 grid per pixel that includes the pixel's corners and edge
//                  midpoints) finds that triangle's slot in its pixel's cell
//   tight          a cell lists no triangle whose image stays more than a pixel away from it
//   cells          the cell-by-cell form the device runs (covers_cell) gives the bits of the row walk the host runs (cover_rows); the table of g x g tiles is the
//                  union of the pixel table's cells
//   no table       a triangle across the camera plane; triangles behind the camera are left out
//   sizes          the cell grows until the table fits 4 MB: 512^2 -> 1, 1024^2 -> 2, 2048^2 -> 4
#include "psdr_jit_amd/csrc/hip/cam_table.h"

#include <cstdio>
#include <random>

using namespace psdr;

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++fails <= 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// world_to_sample of a camera at the origin looking down +z with a 90 degree field of view: x_s = 0.5 - 0.5 x / z, y_s = 0.5 - 0.5 y / z
static const float kW2S[16] = {-0.5f, 0.f, 0.5f, 0.f, 0.f, -0.5f, 0.5f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f};

static double edge_fn(double ax, double ay, double bx, double by, double px, double py) { return (bx - ax) * (py - ay) - (by - ay) * (px - ax); }

static void check_frame(int W, int H, int n, unsigned seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> U(-1.f, 1.f);
    std::vector<float> p0(3 * n), e1(3 * n), e2(3 * n);
    std::vector<int32_t> slot(n);
    for (int t = 0; t < n; ++t) {
        const float z = 2.f + 3.f * (U(rng) + 1.f), s = 0.2f + 1.5f * (U(rng) + 1.f);
        p0[3 * t] = 1.3f * z * U(rng); p0[3 * t + 1] = 1.3f * z * U(rng); p0[3 * t + 2] = z;
        for (int c = 0; c < 3; ++c) { e1[3 * t + c] = (c == 2 ? 0.3f : 1.f) * s * U(rng); e2[3 * t + c] = (c == 2 ? 0.3f : 1.f) * s * U(rng); }      // (|e.z| < 1: in front of the camera)
        slot[t] = (t * 7 + 3) % n;             // a permutation (n and 7 coprime)
    }
    ScreenTris st;
    CHECK(project_tris(p0.data(), e1.data(), e2.data(), n, kW2S, W, H, st), "project_tris refused triangles in front of the camera");
    CHECK((int) st.tri.size() == n, "%d of %d triangles projected", (int) st.tri.size(), n);
    // the host's walk (triangle by triangle, row by row: what fills the live-pixel mask) ...
    std::vector<uint64_t> tab((size_t) W * H, 0ull);
    cover_rows(st, W, H, [&](int i, int row, int c0, int c1) { for (int c = c0; c <= c1; ++c) tab[(size_t) row * W + c] |= 1ull << slot[st.tri[(size_t) i]]; });
    // ... and the device's (cell by cell: what fills the camera-ray table) agree bit for bit
    std::vector<uint64_t> by_cell((size_t) W * H, 0ull);
    for (size_t i = 0; i < st.tri.size(); ++i)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                if (covers_cell(&st.X[3 * i], &st.Y[3 * i], W, H, x, x, y, y)) by_cell[(size_t) y * W + x] |= 1ull << slot[st.tri[i]];
    CHECK(tab == by_cell, "the cell-by-cell table differs from the row walk (%d x %d)", W, H);
    long long listed = 0;
    for (size_t i = 0; i < st.tri.size(); ++i) {
        const double *X = &st.X[3 * i], *Y = &st.Y[3 * i];
        const uint64_t bit = 1ull << slot[st.tri[i]];
        const double area = edge_fn(X[0], Y[0], X[1], Y[1], X[2], Y[2]);
        const double xmin = std::min(X[0], std::min(X[1], X[2])), xmax = std::max(X[0], std::max(X[1], X[2]));
        const double ymin = std::min(Y[0], std::min(Y[1], Y[2])), ymax = std::max(Y[0], std::max(Y[1], Y[2]));
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const bool has = (tab[(size_t) y * W + x] & bit) != 0;
                listed += has;
                if (has) CHECK(x + 1 >= xmin - 1 && x <= xmax + 1 && y + 1 >= ymin - 1 && y <= ymax + 1, "pixel (%d, %d) lists triangle %d, whose image is further than a pixel away", x, y, st.tri[i]);
                if (has || area == 0.0) continue;
                for (int a = 0; a <= 4; ++a)
                    for (int b = 0; b <= 4; ++b) {
                        const double px = x + 0.25 * a, py = y + 0.25 * b;
                        const double w0 = edge_fn(X[1], Y[1], X[2], Y[2], px, py) / area, w1 = edge_fn(X[2], Y[2], X[0], Y[0], px, py) / area, w2 = edge_fn(X[0], Y[0], X[1], Y[1], px, py) / area;
                        CHECK(!(w0 >= 0 && w1 >= 0 && w2 >= 0), "point (%g, %g) lies in the image of triangle %d, which pixel (%d, %d) does not list", px, py, st.tri[i], x, y);
                    }
            }
    }
    CHECK(listed > 0 && listed < (long long) W * H * n, "%lld bits set of %lld", listed, (long long) W * H * n);
    // g x g tiles: the union of their pixels
    for (int shift = 1; shift <= 2; ++shift) {
        const int g = 1 << shift, cw = (W + g - 1) >> shift, ch = (H + g - 1) >> shift;
        std::vector<uint64_t> coarse((size_t) cw * ch, 0ull), want((size_t) cw * ch, 0ull);
        for (size_t i = 0; i < st.tri.size(); ++i)
            for (int cy = 0; cy < ch; ++cy)
                for (int cx = 0; cx < cw; ++cx)
                    if (covers_cell(&st.X[3 * i], &st.Y[3 * i], W, H, cx << shift, std::min(W - 1, (cx << shift) + g - 1), cy << shift, std::min(H - 1, (cy << shift) + g - 1)))
                        coarse[(size_t) cy * cw + cx] |= 1ull << slot[st.tri[i]];
        for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) want[(size_t) (y >> shift) * cw + (x >> shift)] |= tab[(size_t) y * W + x];
        CHECK(coarse == want, "the table of %d x %d tiles is not the union of its pixels (%d x %d)", g, g, W, H);
    }
}

int main() {
    check_frame(37, 29, 23, 1u);
    check_frame(64, 48, 36, 2u);
    check_frame(5, 91, 64, 3u);
    // across the camera plane / behind it
    {
        const float p0[6] = {0.f, 0.f, 2.f, 0.f, 0.f, -3.f}, e1[6] = {1.f, 0.f, 0.f, 1.f, 0.f, 0.f}, e2[6] = {0.f, 1.f, -4.f, 0.f, 1.f, 0.f};
        ScreenTris st;
        CHECK(!project_tris(p0, e1, e2, 1, kW2S, 16, 16, st), "a triangle across the camera plane was projected");
        CHECK(project_tris(p0 + 3, e1 + 3, e2 + 3, 1, kW2S, 16, 16, st) && st.tri.empty(), "a triangle behind the camera was kept");
        const float nan_p[3] = {0.f, std::nanf(""), 2.f};
        CHECK(!project_tris(nan_p, e1, e2, 1, kW2S, 16, 16, st), "a NaN vertex was projected");
    }
    CHECK(cam_table_shift(512, 512) == 0 && cam_table_shift(724, 724) == 0 && cam_table_shift(1024, 1024) == 1 && cam_table_shift(2048, 2048) == 2 && cam_table_shift(96, 80) == 0,
          "cell sizes: %d %d %d", cam_table_shift(512, 512), cam_table_shift(1024, 1024), cam_table_shift(2048, 2048));
    if (fails) { std::printf("%d check(s) failed\n", fails); return 1; }
    std::printf("OK\n");
    return 0;
}
