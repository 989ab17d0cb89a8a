// blob_rows.h — the words of one item of the scene blob as the HOST path writes them from a snapshot (include/psdr_hip.h): one definition for scene_build.hip's
// writers (on the pinned copy) and for the check aids psdr_hip_scene_check_rows / _check_edges (on a local array, against the device's words).  The device kernels
// k_geo_rows, k_geo_sec and k_pe_rows spell the same rows out on their own: that independence is what the check aids test.  Host only, no HIP include
// (tests/cpp/blob_layout_check.cpp compiles it with g++).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../../include/psdr_hip.h"

namespace psdr {

static inline void put4(float *b, size_t word, float x, float y, float z, float w) { float *q = b + 4 * word; q[0] = x; q[1] = y; q[2] = z; q[3] = w; }
static inline float ibits(int32_t v) { float f; std::memcpy(&f, &v, 4); return f; }
static inline size_t words_for_floats(size_t n) { return (n + 3) / 4; }

constexpr int kTravWords = 3, kShadeWords = 6, kTanWords = 6, kSecWords = 6, kPeWords = 3;      // float4 words per item

// triangle o: traversal row  {p0.xyz, e1.x} {e1.yz, e2.xy} {e2.z, bits(o), 0, 0}                                     -> trav[12]
//             shading row    {n0.xyz, area} {n1.xyz, bits(mesh)} {n2.xyz, bits(flat)} {fn.xyz, bits(o)} {uv0, uv1} {uv2, 0, 0}   -> shade[24] (tr.uv NULL: zeros)
static inline void pack_tri_rows(const psdr_triangles &tr, size_t o, float *trav, float *shade) {
    const float *p0 = tr.p0 + 3 * o, *e1 = tr.e1 + 3 * o, *e2 = tr.e2 + 3 * o;
    put4(trav, 0, p0[0], p0[1], p0[2], e1[0]);
    put4(trav, 1, e1[1], e1[2], e2[0], e2[1]);
    put4(trav, 2, e2[2], ibits((int32_t) o), 0.f, 0.f);
    const float *n0 = tr.n0 + 3 * o, *n1 = tr.n1 + 3 * o, *n2 = tr.n2 + 3 * o, *fn = tr.face_normal + 3 * o;
    put4(shade, 0, n0[0], n0[1], n0[2], tr.face_area[o]);
    put4(shade, 1, n1[0], n1[1], n1[2], ibits(tr.mesh_id[o]));
    put4(shade, 2, n2[0], n2[1], n2[2], ibits(tr.use_face_normal && tr.use_face_normal[o] ? 1 : 0));
    put4(shade, 3, fn[0], fn[1], fn[2], ibits((int32_t) o));
    if (tr.uv) {
        const float *uv = tr.uv + 6 * o;
        put4(shade, 4, uv[0], uv[1], uv[2], uv[3]);
        put4(shade, 5, uv[4], uv[5], 0.f, 0.f);
    } else { put4(shade, 4, 0.f, 0.f, 0.f, 0.f); put4(shade, 5, 0.f, 0.f, 0.f, 0.f); }
}

// triangle o (tr.d_p0 != NULL): {d_p0.xyz, d_e1.x} {d_e1.yz, d_e2.xy} {d_e2.z, d_n0.xyz} {d_n1.xyz, d_n2.x} {d_n2.yz, d_fn.xy} {d_fn.z, d_area, 0, 0}   -> tan[24]
static inline void pack_tan_row(const psdr_triangles &tr, size_t o, float *tan) {
    const float *a = tr.d_p0 + 3 * o, *b = tr.d_e1 + 3 * o, *c = tr.d_e2 + 3 * o, *d0 = tr.d_n0 + 3 * o, *d1 = tr.d_n1 + 3 * o, *d2 = tr.d_n2 + 3 * o, *df = tr.d_face_normal + 3 * o;
    put4(tan, 0, a[0], a[1], a[2], b[0]);
    put4(tan, 1, b[1], b[2], c[0], c[1]);
    put4(tan, 2, c[2], d0[0], d0[1], d0[2]);
    put4(tan, 3, d1[0], d1[1], d1[2], d2[0]);
    put4(tan, 4, d2[1], d2[2], df[0], df[1]);
    put4(tan, 5, df[2], tr.d_face_area[o], 0.f, 0.f);
}

// secondary edge i: {p0.xyz, e1.x} {e1.yz, n0.xy} {n0.z, n1.xyz} {p2.xyz, bits(is_boundary)} {d_p0.xyz, d_e1.x} {d_e1.yz, 0, 0}   -> row[24] (d_p0 / d_e1 NULL: zeros)
static inline void pack_sec_row(const psdr_sec_edges &se, size_t i, float *row) {
    const float z3[3] = {0.f, 0.f, 0.f};
    const float *p0 = se.p0 + 3 * i, *e1 = se.e1 + 3 * i, *n0 = se.n0 + 3 * i, *n1 = se.n1 + 3 * i, *p2 = se.p2 + 3 * i;
    const float *dp0 = se.d_p0 ? se.d_p0 + 3 * i : z3, *de1 = se.d_e1 ? se.d_e1 + 3 * i : z3;
    put4(row, 0, p0[0], p0[1], p0[2], e1[0]);
    put4(row, 1, e1[1], e1[2], n0[0], n0[1]);
    put4(row, 2, n0[2], n1[0], n1[1], n1[2]);
    put4(row, 3, p2[0], p2[1], p2[2], ibits(se.is_boundary[i] ? 1 : 0));
    put4(row, 4, dp0[0], dp0[1], dp0[2], de1[0]);
    put4(row, 5, de1[1], de1[2], 0.f, 0.f);
}

// primary edge i of a sensor: {p0.xy, p1.xy} {d_p0.xy, d_p1.xy} {normal.xy, length, 0}   -> row[12] (d_edge_p0 / d_edge_p1 NULL: zeros)
static inline void pack_pe_row(const psdr_sensor_rec &r, size_t i, float *row) {
    put4(row, 0, r.edge_p0[2 * i], r.edge_p0[2 * i + 1], r.edge_p1[2 * i], r.edge_p1[2 * i + 1]);
    put4(row, 1, r.d_edge_p0 ? r.d_edge_p0[2 * i] : 0.f, r.d_edge_p0 ? r.d_edge_p0[2 * i + 1] : 0.f, r.d_edge_p1 ? r.d_edge_p1[2 * i] : 0.f, r.d_edge_p1 ? r.d_edge_p1[2 * i + 1] : 0.f);
    put4(row, 2, r.edge_normal[2 * i], r.edge_normal[2 * i + 1], r.edge_length[i], 0.f);
}

// entry i of a distribution of n entries at float `cdf` of the blob: pmf at [i], cmf behind all of them at [n + i]
static inline void pack_distrb(float *cdf, size_t n, size_t i, float pmf, float cmf) { cdf[i] = pmf; cdf[n + i] = cmf; }

} // namespace psdr
