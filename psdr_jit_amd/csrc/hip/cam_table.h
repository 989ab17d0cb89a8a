// cam_table.h — conservative screen-space coverage of the scene for one sensor (scene_build.hip: host and device; tests/cpp/cam_table_check.cpp: g++ alone).
//
// Which triangles a ray through a given pixel can hit depends only on the triangles and the sensor: world_to_sample is a projective map, so the image of a
// triangle in front of the camera is the triangle of its projected vertices, and a ray through a pixel's square can only reach the triangles whose image comes
// within a quarter of a pixel of that square (the pad covers the float roundings of the ray's direction and of tri_test).  Two tables come out of the same
// arithmetic (project_vertex, tri_rows, row_extent - double precision, the same operations in the same order on both sides):
//   the live-pixel mask    bit (y * width + x) = some triangle covers the pixel (SensorDev::live: the interior term skips the samples of the other pixels);
//                          filled on the host, triangle by triangle and row by row (cover_rows)
//   the camera-ray table   one 64-bit word per cell, bit k = the triangle in traversal slot k covers a pixel of the cell (SensorDev::cam_tab: a camera ray is
//                          tested against these triangles only, paths.h).  A cell is one pixel, or a g x g tile of them (g a power of two) on large frames;
//                          filled on the device, cell by cell, from the triangle rows that are already there (scene_build.hip::k_cam_table) - nothing is uploaded
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define PSDR_CT_HD __host__ __device__ inline
#else
#define PSDR_CT_HD inline
#endif

namespace psdr {

constexpr double kCoverPad = 0.25;                      // pixels
constexpr size_t kCamTableMaxBytes = 4u << 20;          // the table of one sensor: cells grow until it fits

// vertex p through world_to_sample, in pixel units.  false: not in front of the camera
PSDR_CT_HD bool project_vertex(const float *w2s, const double p[3], int W, int H, double &X, double &Y) {
    const double x = w2s[0] * p[0] + w2s[1] * p[1] + w2s[2] * p[2] + w2s[3], y = w2s[4] * p[0] + w2s[5] * p[1] + w2s[6] * p[2] + w2s[7];
    const double w = w2s[12] * p[0] + w2s[13] * p[1] + w2s[14] * p[2] + w2s[15];
    if (!(w > 1e-9)) return false;
    X = x / w * W; Y = y / w * H;
    return true;
}

// the three vertices of triangle (p0, e1, e2) -> X[3], Y[3]; the number of vertices that are not in front of the camera (0: projected; 3: behind it - no forward
// ray reaches the triangle; 1, 2: it crosses the camera plane and its image is not a triangle)
PSDR_CT_HD int project_triangle(const float *w2s, const float p0[3], const float e1[3], const float e2[3], int W, int H, double X[3], double Y[3]) {
    int behind = 0;
    for (int v = 0; v < 3; ++v) {
        double p[3];
        for (int c = 0; c < 3; ++c) p[c] = (double) p0[c] + (v == 1 ? (double) e1[c] : (v == 2 ? (double) e2[c] : 0.0));
        if (!project_vertex(w2s, p, W, H, X[v], Y[v])) ++behind;
    }
    return behind;
}

// the pixel rows r0..r1 of the frame a projected triangle comes within the pad of (r0 > r1: none)
PSDR_CT_HD void tri_rows(const double Y[3], int H, int &r0, int &r1) {
    const double ymin = fmin(Y[0], fmin(Y[1], Y[2])) - kCoverPad, ymax = fmax(Y[0], fmax(Y[1], Y[2])) + kCoverPad;
    r0 = 0; r1 = -1;
    if (!(ymax >= 0.0 && ymin < (double) H)) return;
    r0 = (int) fmax(0.0, floor(ymin)); r1 = (int) fmin((double) (H - 1), floor(ymax));
}

// the columns c0..c1 of pixel row `row` the triangle covers: its x-extent inside the (padded) row slab, padded.  false: none
PSDR_CT_HD bool row_extent(const double X[3], const double Y[3], int row, int W, int &c0, int &c1) {
    const double lo = row - kCoverPad, hi = row + 1 + kCoverPad;
    double xmin = 1e300, xmax = -1e300;
    for (int v = 0; v < 3; ++v) {
        if (Y[v] >= lo && Y[v] <= hi) { xmin = fmin(xmin, X[v]); xmax = fmax(xmax, X[v]); }
        const int u = (v + 1) % 3;
        const double dy = Y[u] - Y[v];
        if (dy != 0.0)
            for (int side = 0; side < 2; ++side) {
                const double s = ((side ? hi : lo) - Y[v]) / dy;
                if (s >= 0.0 && s <= 1.0) { const double xc = X[v] + s * (X[u] - X[v]); xmin = fmin(xmin, xc); xmax = fmax(xmax, xc); }
            }
    }
    if (xmin > xmax) return false;
    xmin -= kCoverPad; xmax += kCoverPad;
    if (!(xmax >= 0.0 && xmin < (double) W)) return false;
    c0 = (int) fmax(0.0, floor(xmin)); c1 = (int) fmin((double) (W - 1), floor(xmax));
    return true;
}

// does the projected triangle cover a pixel of the cell (columns x0..x1, rows y0..y1 of the frame)?  The row walk of cover_rows, asked cell by cell
PSDR_CT_HD bool covers_cell(const double X[3], const double Y[3], int W, int H, int x0, int x1, int y0, int y1) {
    int r0, r1;
    tri_rows(Y, H, r0, r1);
    for (int row = r0 > y0 ? r0 : y0; row <= (r1 < y1 ? r1 : y1); ++row) {
        int c0, c1;
        if (row_extent(X, Y, row, W, c0, c1) && c0 <= x1 && c1 >= x0) return true;
    }
    return false;
}

// the triangles in front of the camera, projected to pixel units.  false: a triangle crosses the camera plane or has a vertex that is not finite - no table can be made
struct ScreenTris {
    std::vector<int> tri;             // index into the caller's triangle arrays
    std::vector<double> X, Y;         // [3 * tri.size()]
};
inline bool project_tris(const float *p0, const float *e1, const float *e2, int n, const float *w2s, int W, int H, ScreenTris &out) {
    out.tri.clear(); out.X.clear(); out.Y.clear();
    for (int t = 0; t < n; ++t) {
        for (int c = 0; c < 3; ++c)
            if (!(std::isfinite(p0[3 * t + c]) && std::isfinite(e1[3 * t + c]) && std::isfinite(e2[3 * t + c]))) return false;
        double X[3], Y[3];
        const int behind = project_triangle(w2s, p0 + 3 * t, e1 + 3 * t, e2 + 3 * t, W, H, X, Y);
        if (behind == 3) continue;
        if (behind != 0) return false;
        out.tri.push_back(t);
        for (int v = 0; v < 3; ++v) { out.X.push_back(X[v]); out.Y.push_back(Y[v]); }
    }
    return true;
}

// emit(i, row, c0, c1) for every projected triangle i (an index into st.tri) and every pixel row it comes within the pad of: the columns c0..c1 it covers there
template <typename Emit>
inline void cover_rows(const ScreenTris &st, int W, int H, Emit emit) {
    for (size_t i = 0; i < st.tri.size(); ++i) {
        int r0, r1;
        tri_rows(&st.Y[3 * i], H, r0, r1);
        for (int row = r0; row <= r1; ++row) {
            int c0, c1;
            if (row_extent(&st.X[3 * i], &st.Y[3 * i], row, W, c0, c1)) emit((int) i, row, c0, c1);
        }
    }
}

// log2 of the cell size g: the smallest power of two that keeps ceil(W / g) * ceil(H / g) words within kCamTableMaxBytes
inline int cam_table_shift(int W, int H) {
    int s = 0;
    while ((size_t) ((W + (1 << s) - 1) >> s) * (size_t) ((H + (1 << s) - 1) >> s) * sizeof(uint64_t) > kCamTableMaxBytes) ++s;
    return s;
}

} // namespace psdr
