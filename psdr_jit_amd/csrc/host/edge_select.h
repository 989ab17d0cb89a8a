// edge_select.h — which mesh edges a perspective / orthographic sensor keeps as primary edges, and the sample-space row of a kept edge.
//
// The two loop bodies of PerspectiveCamera::configure (reference src/sensor/perspective.cpp:52-151: the silhouette test on device arrays and the rows compressD
// gathers), written ONCE and compiled for both sides like hnum.h: the host loop (scene_host.cpp) and the kernels that select a sensor's primary edges on the
// device (csrc/hip/scene_build.hip, k_pe_*) call these functions, so both write the same bits.
#pragma once
#include "hnum.h"

namespace psdr_host {

constexpr float kEdgeSelectEpsilon = 1e-5f;      // reference include/psdr/constants.h:12 (Epsilon)

// uv seam (perspective.cpp:95-110): the two faces of the edge do not share exactly two uv indices.  uv_f0 / uv_f1: the three uv indices of the faces; uv_f1 = nullptr
// for a boundary edge (a masked gather: zeros).  A function of the topology alone - computed once per topology version, one byte per edge.
PSDR_HNUM_HD inline bool edge_uv_seam(const int *uv_f0, const int *uv_f1) {
    int b[3] = {0, 0, 0}, cut = 0;
    if (uv_f1) for (int k = 0; k < 3; ++k) b[k] = uv_f1[k];
    for (int k = 0; k < 3; ++k) { const int a = uv_f0[k]; if (a == b[0] || a == b[1] || a == b[2]) ++cut; }
    return cut != 2;
}

// the keep test.  cam: camera position; t0 / t1: first vertex [0..2] and unit normal [3..5] of the edge's faces, t1 = nullptr for a boundary edge (f1 = -1);
// flat: the mesh uses face normals; has_uv / seam: the mesh has uv coordinates / edge_uv_seam of this edge
PSDR_HNUM_HD inline bool edge_keep(const float *cam, const float *t0, const float *t1, bool flat, bool has_uv, bool seam) {
    const bool valid = t1 != nullptr;
    const D3 cpos = {DF(cam[0]), DF(cam[1]), DF(cam[2])};
    const D3 e0 = dnormalize(cpos - D3{DF(t0[0]), DF(t0[1]), DF(t0[2])}), n0 = {DF(t0[3]), DF(t0[4]), DF(t0[5])};
    D3 e1 = dnormalize(cpos), n1 = {DF(0.f), DF(0.f), DF(0.f)};        // masked gathers return zeros
    if (valid) { e1 = dnormalize(cpos - D3{DF(t1[0]), DF(t1[1]), DF(t1[2])}); n1 = {DF(t1[3]), DF(t1[4]), DF(t1[5])}; }
    const float eps = kEdgeSelectEpsilon;
    bool keep;
    if (flat) keep = !(valid && ((ddot(e0, n0).v < eps && ddot(e1, n1).v < eps) || ddot(n0, n1).v > 1.f - eps));
    else keep = !valid || ((ddot(e0, n0).v > eps) != (ddot(e1, n1).v > eps));
    if (has_uv) keep = keep || seam;
    return keep;
}

// PrimaryEdgeInfo of one kept edge (edge.h:27-40): end points and their tangents in sample space, the unit normal of the projected edge, its length
struct PrimEdgeRow { float p0[2], p1[2], d_p0[2], d_p1[2], normal[2], length; };

// v0 / v1: world-space end points (value, tangent); w2s: the sensor's world_to_sample (value, tangent)
PSDR_HNUM_HD inline PrimEdgeRow edge_row(const DM4 &w2s, const D3 &v0, const D3 &v1) {
    const D3 q0 = xform_pos(w2s, v0), q1 = xform_pos(w2s, v1);
    float ex = q1.x.v - q0.x.v, ey = q1.y.v - q0.y.v;
    const float len = std::sqrt(std::fmaf(ey, ey, ex * ex));
    ex /= len; ey /= len;
    PrimEdgeRow r;
    r.p0[0] = q0.x.v; r.p0[1] = q0.y.v; r.p1[0] = q1.x.v; r.p1[1] = q1.y.v;
    r.d_p0[0] = q0.x.d; r.d_p0[1] = q0.y.d; r.d_p1[0] = q1.x.d; r.d_p1[1] = q1.y.d;
    r.normal[0] = -ey; r.normal[1] = ex;
    r.length = len;
    return r;
}

// length of a secondary edge (scene.cpp:559-563: the PMF entry of Scene::m_sec_edge_distrb) from its world-space end points
PSDR_HNUM_HD inline float edge_length3(const float *a, const float *b) {
    float e1[3];
    for (int k = 0; k < 3; ++k) e1[k] = b[k] - a[k];
    return std::sqrt(std::fmaf(e1[2], e1[2], std::fmaf(e1[1], e1[1], e1[0] * e1[0])));
}

} // namespace psdr_host
