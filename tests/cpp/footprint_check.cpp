// env::bitmap_footprint and env::bitmap_footprint_env (psdr_jit_amd/csrc/common/envmath.h: the four texels and weights that the reverse-mode kernels scatter a lookup's adjoint
// into) as the transposes of env::bitmap_eval_tex and env::bitmap_eval_fn (what the forward kernels evaluate): for a one-hot map, the weight the footprint puts on the hot texel equals
// the evaluated value to within 2 ulp of 1, and every index lies inside the map.  Host only; prints "OK <lookups>" or the first failures.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <vector>

#include "psdr_jit_amd/csrc/common/envmath.h"

using namespace psdr::env;

static long g_checked = 0;
static int g_failed = 0;

static void fail(const char *what, int W, int H, float u, float v, bool flip, bool with_xf, int t, double got, double want) {
    if (++g_failed <= 20)
        std::printf("FAIL %s %d x %d u = %.9g v = %.9g flip_v = %d xf = %d texel %d: footprint %.9g, eval %.9g\n", what, W, H, u, v, (int) flip, (int) with_xf, t, got, want);
}

static std::vector<float> grid() {
    const float below_one = 1.0f - ldexpf(1.0f, -24);
    std::vector<float> g = {0.0f, 1.0f, below_one, -0.0f, 0.5f, 0.25f, 0.75f, 1.0f / 3.0f, 0.999f, 1e-7f, ldexpf(1.0f, -24), -1e-9f, -0.3f, -1.0f, -2.75f, 1.2f, 2.0f, 3.6f, 17.125f};
    for (int i = 1; i < 16; ++i) g.push_back((float) i / 16.0f + 0.013f);
    return g;
}

static bool inside(const int idx[4], int n) {
    for (int k = 0; k < 4; ++k)
        if (idx[k] < 0 || idx[k] >= n) return false;
    return true;
}

static double weight_on(const int idx[4], const float w[4], int t) {
    double s = 0.0;
    for (int k = 0; k < 4; ++k)
        if (idx[k] == t) s += (double) w[k];
    return s;
}

int main() {
    const int sizes[5][2] = {{2, 2}, {2, 5}, {5, 2}, {3, 7}, {16, 8}};
    const std::vector<float> g = grid();
    const double tol = 2.0 * (double) FLT_EPSILON;
    const UvXf<float> plain, turned(0.4f, 1.7f, 0.13f, -0.21f);
    for (const auto &sz : sizes) {
        const int W = sz[0], H = sz[1], n = W * H;
        for (int with_xf = 0; with_xf < 2; ++with_xf) {
            const UvXf<float> &xf = with_xf ? turned : plain;
            for (float u : g)
                for (float v : g) {
                    int idx[4];
                    float w[4];
                    for (int flip = 0; flip < 2; ++flip) {
                        bitmap_footprint(W, H, u, v, flip != 0, idx, w, xf);
                        if (!inside(idx, n)) { fail("texture: index outside the map", W, H, u, v, flip != 0, with_xf != 0, idx[0], idx[3], n); continue; }
                        for (int t = 0; t < n; ++t) {
                            float out3[3], out1[1];
                            bitmap_eval_tex<float, 3>([&](int i, int c) { return (i == t && c == 1) ? 1.0f : 0.0f; }, W, H, u, v, flip != 0, out3, xf);
                            bitmap_eval_tex<float, 1>([&](int i, int) { return i == t ? 1.0f : 0.0f; }, W, H, u, v, flip != 0, out1, xf);
                            const double got = weight_on(idx, w, t);
                            if (!(std::fabs(got - (double) out3[1]) <= tol) || out3[0] != 0.0f || out3[2] != 0.0f) fail("texture, 3 channels", W, H, u, v, flip != 0, with_xf != 0, t, got, out3[1]);
                            if (!(std::fabs(got - (double) out1[0]) <= tol)) fail("texture, 1 channel", W, H, u, v, flip != 0, with_xf != 0, t, got, out1[0]);
                        }
                        ++g_checked;
                    }
                    bitmap_footprint_env(W, H, u, v, idx, w, xf);
                    if (!inside(idx, n)) { fail("environment: index outside the map", W, H, u, v, false, with_xf != 0, idx[0], idx[3], n); continue; }
                    for (int t = 0; t < n; ++t) {
                        float out[3];
                        bitmap_eval_fn<float>([&](int i, int c) { return (i == t && c == 2) ? 1.0f : 0.0f; }, W, H, u, v, out, xf);
                        const double got = weight_on(idx, w, t);
                        if (!(std::fabs(got - (double) out[2]) <= tol) || out[0] != 0.0f || out[1] != 0.0f) fail("environment", W, H, u, v, false, with_xf != 0, t, got, out[2]);
                    }
                    ++g_checked;
                }
        }
    }
    if (g_failed) {
        std::printf("%d failures in %ld lookups\n", g_failed, g_checked);
        return 1;
    }
    std::printf("OK %ld\n", g_checked);
    return 0;
}
