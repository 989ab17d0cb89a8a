// The shared keep test and primary-edge row (psdr_jit_amd/csrc/host/edge_select.h: one definition for the host loop and the device kernels) on hand-made edges,
// against values written here.  Host compile only: g++ -O2 -std=c++17 -I<repo> tests/cpp/edge_select_check.cpp
#include <cmath>
#include <cstdio>

#include "psdr_jit_amd/csrc/host/edge_select.h"

using namespace psdr_host;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)
static bool near(float a, float b, float tol = 1e-6f) { return std::fabs(a - b) <= tol; }

int main() {
    // camera on the +z axis, looking at an edge along y through the origin.  A face is given by its first vertex and unit normal.
    const float cam[3] = {0.f, 0.f, 10.f};
    const float s = 0.70710678f;
    const float front_l[6] = {0.f, 0.f, 0.f, -s, 0.f, s};      // faces the camera (n.z > 0), tilted left
    const float front_r[6] = {0.f, 0.f, 0.f, s, 0.f, s};       // faces the camera, tilted right
    const float back_r[6] = {0.f, 0.f, 0.f, s, 0.f, -s};       // faces away
    const float back_l[6] = {0.f, 0.f, 0.f, -s, 0.f, -s};
    const float flat_a[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 1.f}, flat_b[6] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f};     // coplanar pair

    // ---- smooth meshes: kept = boundary, or exactly one of the two faces looks at the camera
    CHECK(edge_keep(cam, front_l, back_r, false, false, false));         // silhouette
    CHECK(edge_keep(cam, back_l, front_r, false, false, false));         // silhouette, the other way round
    CHECK(!edge_keep(cam, front_l, front_r, false, false, false));       // crease seen from the front: both look at the camera
    CHECK(!edge_keep(cam, back_l, back_r, false, false, false));         // both look away
    CHECK(!edge_keep(cam, flat_a, flat_b, false, false, false));         // coplanar
    CHECK(edge_keep(cam, front_l, nullptr, false, false, false));        // boundary (f1 = -1)
    CHECK(edge_keep(cam, back_l, nullptr, false, false, false));
    // ---- use_face_normal meshes: dropped = both faces look away, or the faces are coplanar
    CHECK(edge_keep(cam, front_l, back_r, true, false, false));          // silhouette
    CHECK(edge_keep(cam, front_l, front_r, true, false, false));         // crease: kept, unlike on a smooth mesh
    CHECK(!edge_keep(cam, back_l, back_r, true, false, false));          // both look away
    CHECK(!edge_keep(cam, flat_a, flat_b, true, false, false));          // coplanar: n0 . n1 = 1 > 1 - Epsilon
    CHECK(edge_keep(cam, back_l, nullptr, true, false, false));          // boundary
    // ---- uv seam: adds edges on meshes with uv coordinates, never removes one
    CHECK(edge_keep(cam, front_l, front_r, false, true, true));
    CHECK(!edge_keep(cam, front_l, front_r, false, true, false));
    CHECK(!edge_keep(cam, front_l, front_r, false, false, true));        // (no uv coordinates: the mask is not consulted)
    CHECK(edge_keep(cam, flat_a, flat_b, true, true, true));
    CHECK(edge_keep(cam, front_l, back_r, false, true, false));
    // a grazing face: |e . n| below Epsilon counts as not looking at the camera
    const float graze[6] = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f};
    CHECK(edge_keep(cam, graze, front_r, false, false, false));
    CHECK(!edge_keep(cam, graze, back_r, false, false, false));

    // ---- the uv-seam mask: the two faces share exactly two uv indices or it is a seam
    const int f0[3] = {0, 1, 2}, shares2[3] = {2, 1, 3}, shares0[3] = {4, 5, 6}, shares1[3] = {2, 7, 8}, shares3[3] = {1, 2, 0};
    CHECK(!edge_uv_seam(f0, shares2));
    CHECK(edge_uv_seam(f0, shares0));
    CHECK(edge_uv_seam(f0, shares1));
    CHECK(edge_uv_seam(f0, shares3));
    CHECK(edge_uv_seam(f0, nullptr));                                    // boundary: the masked gather reads (0, 0, 0), one index matches
    const int g0[3] = {5, 6, 7};
    CHECK(edge_uv_seam(g0, nullptr));                                    // ... or none

    // ---- the row: world_to_sample = (x, y) -> (x / 2 + 1 / 2, y / 2 + 1 / 2), with a tangent that shifts x by 1 per unit of the parameter
    DM4 w2s = DM4::identity();
    w2s.m[0][0] = DF(0.5f); w2s.m[0][3] = DF(0.5f, 1.f); w2s.m[1][1] = DF(0.5f); w2s.m[1][3] = DF(0.5f);
    const D3 v0{DF(0.f, 2.f), DF(0.f), DF(1.f)}, v1{DF(0.6f), DF(0.8f, -1.f), DF(1.f)};
    const PrimEdgeRow r = edge_row(w2s, v0, v1);
    CHECK(near(r.p0[0], 0.5f) && near(r.p0[1], 0.5f) && near(r.p1[0], 0.8f) && near(r.p1[1], 0.9f));
    CHECK(near(r.d_p0[0], 2.f) && near(r.d_p0[1], 0.f) && near(r.d_p1[0], 1.f) && near(r.d_p1[1], -0.5f));       // 0.5 * 2 + 1, 0, 1, 0.5 * -1
    CHECK(near(r.length, 0.5f));
    CHECK(near(r.normal[0], -0.8f) && near(r.normal[1], 0.6f));                                                  // (-ey, ex) / length
    // a projective map: w = z
    DM4 persp = DM4::identity();
    persp.m[3][2] = DF(1.f); persp.m[3][3] = DF(0.f);
    const PrimEdgeRow q = edge_row(persp, D3{DF(2.f), DF(0.f), DF(2.f)}, D3{DF(2.f), DF(4.f), DF(4.f, 4.f)});
    CHECK(near(q.p0[0], 1.f) && near(q.p0[1], 0.f) && near(q.p1[0], 0.5f) && near(q.p1[1], 1.f));
    CHECK(near(q.d_p1[0], -0.5f) && near(q.d_p1[1], -1.f));              // d(x / w) = -x dw / w^2 = -2 * 4 / 16, d(y / w) = -4 * 4 / 16
    CHECK(near(q.length, std::sqrt(1.25f)));

    // ---- the secondary-edge length
    const float a[3] = {1.f, 2.f, 3.f}, b[3] = {3.f, 5.f, 9.f};
    CHECK(edge_length3(a, b) == 7.f);

    if (failures == 0) std::printf("OK\n");
    return failures == 0 ? 0 : 1;
}
