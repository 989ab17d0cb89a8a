// The layout of the scene blob (psdr_jit_amd/csrc/hip/blob_layout.h) and the host's row packers (blob_rows.h) against numbers written here: offsets counted by hand from
// the per-item sizes of DESIGN.md section 3, every word of every packer against the word order of include/psdr_hip.h / scene_dev.h.
// Host compile only: g++ -O2 -std=c++17 -I<repo> tests/cpp/blob_layout_check.cpp
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "psdr_jit_amd/csrc/hip/blob_layout.h"

using namespace psdr;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static uint32_t F(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }
static uint32_t I(int32_t x) { return (uint32_t) x; }
// every word of `got` is the word of `want`, bit for bit (integers travel in float fields)
static bool words(const float *got, const std::vector<uint32_t> &want) {
    for (size_t i = 0; i < want.size(); ++i) {
        uint32_t u; std::memcpy(&u, got + i, 4);
        if (u != want[i]) { std::printf("  word %zu: got %08x want %08x\n", i, u, want[i]); return false; }
    }
    return true;
}

// stand-ins for SceneTables / SecEdgeTables (scene_dev.h needs the HIP headers): the members the layout code touches
struct Tables { int nodes_off, trav_off, shade_off, tan_off, map_off, filt_off, mesh_off, bsdf_off, emit_off, ecdf_off, fcdf_off, blob_words, has_tangent; };
struct SecTables { int off, cdf_off, n; };

static void check_layout() {
    // (a) 1 triangle in 1 node, no tangent, 1 filter primitive, 1 mesh, no BSDF, no emitter, no face distribution, no edges, one sensor: every max(1, .) floor
    BlobCounts a;
    a.n_tris = 1; a.n_nodes = 1; a.n_filt = 1; a.n_meshes = 1; a.sensor_edges = {0};
    BlobLayout L;
    CHECK(blob_layout(a, L));
    CHECK(L.nodes == 0 && L.trav == 4 && L.shade == 7 && L.tan == 13 && L.map == 13 && L.filt == 14);          // 4 | 3 | 6 | none | ceil(1/4) = 1 | 6
    CHECK(L.small_begin == 20 && L.mesh == 20 && L.bsdf == 22 && L.emit == 24 && L.ecdf == 26 && L.fcdf == 27 && L.small_end == 28);      // 2 | 2 x max(1, 0) | 2 x max(1, 0) | ceil(2/4) | ceil(2/4)
    CHECK(L.sec == 28 && L.sec_cdf == 28 && L.sec_end == 29 && L.n_sec == 0);                                   // no rows | ceil(2 max(1, 0) / 4) = 1
    CHECK(L.pe.size() == 1 && L.pe[0].first == 29 && L.pe[0].second == 29 && L.words == 30);                    // no rows | 1

    // (b) 36 triangles in 5 nodes with tangents, 20 filter primitives, 8 meshes, 5 BSDFs, 1 emitter, 2 face-distribution entries, 40 secondary edges, sensors with 7 and 12 edges
    BlobCounts b;
    b.n_tris = 36; b.n_nodes = 5; b.has_tan = true; b.n_filt = 20; b.n_meshes = 8; b.n_bsdfs = 5; b.n_emitters = 1; b.n_face_distrb = 2; b.n_sec_edges = 40; b.sensor_edges = {7, 12};
    CHECK(blob_layout(b, L));
    CHECK(L.nodes == 0 && L.trav == 20 && L.shade == 128 && L.tan == 344 && L.map == 560 && L.filt == 569);    // 20 | 108 | 216 | 216 | 9 | 120
    CHECK(L.small_begin == 689 && L.mesh == 689 && L.bsdf == 705 && L.emit == 715 && L.ecdf == 717 && L.fcdf == 718 && L.small_end == 719);   // 16 | 10 | 2 | ceil(2/4) | ceil(4/4)
    CHECK(L.sec == 719 && L.sec_cdf == 959 && L.sec_end == 979 && L.n_sec == 40);                               // 240 | ceil(80/4) = 20
    CHECK(L.pe.size() == 2 && L.pe[0].first == 979 && L.pe[0].second == 1000);                                  // 21 | ceil(14/4) = 4
    CHECK(L.pe[1].first == 1004 && L.pe[1].second == 1040 && L.words == 1046);                                  // 36 | ceil(24/4) = 6
    // ... the same without tangents: everything behind the shading rows moves up by 216
    BlobCounts b0 = b; b0.has_tan = false;
    BlobLayout L0;
    CHECK(blob_layout(b0, L0));
    CHECK(L0.tan == 344 && L0.map == 344 && L0.sec == 719 - 216 && L0.words == 1046 - 216);
    // an 8-wide tree: 8 words per node
    BlobCounts b8 = b; b8.node_words = 8;
    CHECK(blob_layout(b8, L0) && L0.trav == 40 && L0.words == 1066);

    // (c) room for 50 edges per sensor: both sensors get it, and each CDF starts behind the room
    BlobCounts c = b; c.pe_cap = 50;
    CHECK(blob_layout(c, L));
    CHECK(L.sec_end == 979 && L.pe[0].first == 979 && L.pe[0].second == 1129);                                  // 150 | ceil(100/4) = 25
    CHECK(L.pe[1].first == 1154 && L.pe[1].second == 1304 && L.words == 1329);
    // a capped layout of a scene whose meshes have no edges: no room, whatever the sensors' records say
    BlobCounts c0 = b; c0.capped = true;
    CHECK(blob_layout(c0, L) && L.pe[0].first == 979 && L.pe[0].second == 979 && L.pe[1].first == 980 && L.pe[1].second == 980 && L.words == 981);

    // (d) 40 million triangles with tangents: 600 million words of rows alone, beyond 0x7fffffff / 4 = 536 870 911 -> refused; 30 million without tangents fit
    BlobCounts d;
    d.n_tris = 40000000; d.n_nodes = 1; d.has_tan = true; d.n_meshes = 1; d.sensor_edges = {0};
    CHECK(!blob_layout(d, L));
    d.n_tris = 30000000; d.has_tan = false;
    CHECK(blob_layout(d, L) && L.words == 4 + 9ull * 30000000 + 7500000 + 2 + 2 + 2 + 1 + 1 + 1 + 1);

    // the offsets reach the tables in one place
    CHECK(blob_layout(b, L));
    Tables T{}; SecTables E{};
    assign_offsets(L, T, E);
    CHECK(T.nodes_off == 0 && T.trav_off == 20 && T.shade_off == 128 && T.tan_off == 344 && T.map_off == 560 && T.filt_off == 569 && T.mesh_off == 689 && T.bsdf_off == 705 &&
          T.emit_off == 715 && T.ecdf_off == 717 && T.fcdf_off == 718 && T.blob_words == 1046 && E.off == 719 && E.cdf_off == 959 && E.n == 40);

    // layout_kept: true for the tables this layout was assigned to, false when any one compared member differs
    T.has_tangent = 1;
    CHECK(layout_kept(L, T, E, true));
    CHECK(!layout_kept(L, T, E, false));                       // (the snapshot lost its tangent arrays)
    { Tables X = T; X.trav_off++; CHECK(!layout_kept(L, X, E, true)); }
    { Tables X = T; X.shade_off++; CHECK(!layout_kept(L, X, E, true)); }
    { Tables X = T; X.tan_off++; CHECK(!layout_kept(L, X, E, true)); }
    { Tables X = T; X.map_off++; CHECK(!layout_kept(L, X, E, true)); }
    { Tables X = T; X.has_tangent = 0; CHECK(!layout_kept(L, X, E, true)); }
    { SecTables X = E; X.off++; CHECK(!layout_kept(L, T, X, true) && !sec_section_kept(L, X)); }
    { SecTables X = E; X.cdf_off++; CHECK(!layout_kept(L, T, X, true) && !sec_section_kept(L, X)); }
    { SecTables X = E; X.n++; CHECK(!layout_kept(L, T, X, true) && !sec_section_kept(L, X)); }
    { Tables X = T; X.filt_off++; X.mesh_off++; X.blob_words++; CHECK(layout_kept(L, X, E, true)); }      // (sections the device never writes are not part of it)
    CHECK(sec_section_kept(L, E));
}

static void check_packers() {
    // two triangles, every field its own value: field f, triangle t, component k -> 100 f + 3 t + k (tangents: + 0.5)
    float p0[6], e1[6], e2[6], n0[6], n1[6], n2[6], fn[6], area[2] = {801.f, 802.f}, uv[12], d[7][6], d_area[2] = {1801.5f, 1802.5f};
    float *val[7] = {p0, e1, e2, n0, n1, n2, fn};
    for (int f = 0; f < 7; ++f) for (int i = 0; i < 6; ++i) { val[f][i] = 100.f * (f + 1) + i; d[f][i] = 1000.5f + 100.f * (f + 1) + i; }
    for (int i = 0; i < 12; ++i) uv[i] = 900.f + i;
    const int32_t mesh_id[2] = {3, 5};
    const uint8_t flat[2] = {0, 1};
    psdr_triangles tr{};
    tr.n_triangles = 2;
    tr.p0 = p0; tr.e1 = e1; tr.e2 = e2; tr.n0 = n0; tr.n1 = n1; tr.n2 = n2; tr.face_normal = fn; tr.face_area = area; tr.uv = uv; tr.mesh_id = mesh_id; tr.use_face_normal = flat;
    tr.d_p0 = d[0]; tr.d_e1 = d[1]; tr.d_e2 = d[2]; tr.d_n0 = d[3]; tr.d_n1 = d[4]; tr.d_n2 = d[5]; tr.d_face_normal = d[6]; tr.d_face_area = d_area;
    float trav[12], shade[24], tan[24];
    pack_tri_rows(tr, 1, trav, shade);
    // traversal {p0.xyz, e1.x} {e1.yz, e2.xy} {e2.z, bits(id), 0, 0}
    CHECK(words(trav, {F(103), F(104), F(105), F(203), F(204), F(205), F(303), F(304), F(305), I(1), F(0), F(0)}));
    // shading {n0.xyz, area} {n1.xyz, bits(mesh)} {n2.xyz, bits(flat)} {fn.xyz, bits(id)} {uv0, uv1} {uv2, 0, 0}
    CHECK(words(shade, {F(403), F(404), F(405), F(802), F(503), F(504), F(505), I(5), F(603), F(604), F(605), I(1), F(703), F(704), F(705), I(1),
                        F(906), F(907), F(908), F(909), F(910), F(911), F(0), F(0)}));
    pack_tri_rows(tr, 0, trav, shade);
    CHECK(words(trav, {F(100), F(101), F(102), F(200), F(201), F(202), F(300), F(301), F(302), I(0), F(0), F(0)}));
    CHECK(words(shade, {F(400), F(401), F(402), F(801), F(500), F(501), F(502), I(3), F(600), F(601), F(602), I(0), F(700), F(701), F(702), I(0),
                        F(900), F(901), F(902), F(903), F(904), F(905), F(0), F(0)}));
    // no uv, no flat-shading flags: zeros
    tr.uv = nullptr; tr.use_face_normal = nullptr;
    pack_tri_rows(tr, 1, trav, shade);
    CHECK(words(shade + 8, {F(603), F(604), F(605), I(0)}));
    CHECK(words(shade + 16, {F(0), F(0), F(0), F(0), F(0), F(0), F(0), F(0)}));
    // tangent {d_p0.xyz, d_e1.x} {d_e1.yz, d_e2.xy} {d_e2.z, d_n0.xyz} {d_n1.xyz, d_n2.x} {d_n2.yz, d_fn.xy} {d_fn.z, d_area, 0, 0}
    pack_tan_row(tr, 1, tan);
    CHECK(words(tan, {F(1103.5f), F(1104.5f), F(1105.5f), F(1203.5f), F(1204.5f), F(1205.5f), F(1303.5f), F(1304.5f), F(1305.5f), F(1403.5f), F(1404.5f), F(1405.5f),
                      F(1503.5f), F(1504.5f), F(1505.5f), F(1603.5f), F(1604.5f), F(1605.5f), F(1703.5f), F(1704.5f), F(1705.5f), F(1802.5f), F(0), F(0)}));

    // two secondary edges
    float sp0[6], se1[6], sn0[6], sn1[6], sp2[6], sdp0[6], sde1[6];
    float *sv[7] = {sp0, se1, sn0, sn1, sp2, sdp0, sde1};
    for (int f = 0; f < 7; ++f) for (int i = 0; i < 6; ++i) sv[f][i] = 10.f * (f + 1) + i;
    const uint8_t boundary[2] = {1, 0};
    psdr_sec_edges se{};
    se.n_edges = 2; se.p0 = sp0; se.e1 = se1; se.n0 = sn0; se.n1 = sn1; se.p2 = sp2; se.is_boundary = boundary; se.d_p0 = sdp0; se.d_e1 = sde1;
    float row[24];
    // {p0.xyz, e1.x} {e1.yz, n0.xy} {n0.z, n1.xyz} {p2.xyz, bits(is_boundary)} {d_p0.xyz, d_e1.x} {d_e1.yz, 0, 0}
    pack_sec_row(se, 1, row);
    CHECK(words(row, {F(13), F(14), F(15), F(23), F(24), F(25), F(33), F(34), F(35), F(43), F(44), F(45), F(53), F(54), F(55), I(0), F(63), F(64), F(65), F(73), F(74), F(75), F(0), F(0)}));
    pack_sec_row(se, 0, row);
    CHECK(words(row, {F(10), F(11), F(12), F(20), F(21), F(22), F(30), F(31), F(32), F(40), F(41), F(42), F(50), F(51), F(52), I(1), F(60), F(61), F(62), F(70), F(71), F(72), F(0), F(0)}));
    se.d_p0 = nullptr; se.d_e1 = nullptr;
    pack_sec_row(se, 1, row);
    CHECK(words(row + 12, {F(53), F(54), F(55), I(0), F(0), F(0), F(0), F(0), F(0), F(0), F(0), F(0)}));

    // two primary edges of a sensor: {p0.xy, p1.xy} {d_p0.xy, d_p1.xy} {normal.xy, length, 0}
    const float ep0[4] = {1, 2, 3, 4}, ep1[4] = {5, 6, 7, 8}, dp0[4] = {9, 10, 11, 12}, dp1[4] = {13, 14, 15, 16}, en[4] = {17, 18, 19, 20}, len[2] = {21, 22};
    psdr_sensor_rec r{};
    r.n_edges = 2; r.edge_p0 = ep0; r.edge_p1 = ep1; r.d_edge_p0 = dp0; r.d_edge_p1 = dp1; r.edge_normal = en; r.edge_length = len;
    float pe[12];
    pack_pe_row(r, 1, pe);
    CHECK(words(pe, {F(3), F(4), F(7), F(8), F(11), F(12), F(15), F(16), F(19), F(20), F(22), F(0)}));
    pack_pe_row(r, 0, pe);
    CHECK(words(pe, {F(1), F(2), F(5), F(6), F(9), F(10), F(13), F(14), F(17), F(18), F(21), F(0)}));
    r.d_edge_p0 = nullptr;
    pack_pe_row(r, 1, pe);
    CHECK(words(pe + 4, {F(0), F(0), F(15), F(16)}));
    r.d_edge_p0 = dp0; r.d_edge_p1 = nullptr;
    pack_pe_row(r, 1, pe);
    CHECK(words(pe + 4, {F(11), F(12), F(0), F(0)}));

    // a distribution of 3 entries: pmf at [i], cmf at [3 + i]
    float cdf[6] = {-1, -1, -1, -1, -1, -1};
    pack_distrb(cdf, 3, 0, 0.25f, 0.25f); pack_distrb(cdf, 3, 2, 0.5f, 1.f);
    CHECK(words(cdf, {F(0.25f), F(-1), F(0.5f), F(0.25f), F(-1), F(1.f)}));
    // the small helpers
    float q[8] = {0};
    put4(q, 1, 1.f, 2.f, 3.f, 4.f);
    CHECK(words(q, {F(0), F(0), F(0), F(0), F(1), F(2), F(3), F(4)}));
    CHECK(words_for_floats(0) == 0 && words_for_floats(1) == 1 && words_for_floats(4) == 1 && words_for_floats(5) == 2);
    const float m1 = ibits(-1);
    CHECK(words(&m1, {0xffffffffu}));
}

int main() {
    check_layout();
    check_packers();
    if (failures == 0) std::printf("OK\n");
    return failures == 0 ? 0 : 1;
}
