// blob_layout.h — where every section of the scene blob lies (float4-word offsets), as a function of counts alone; the one place scene_build.hip takes the offsets of
// SceneTables / SecEdgeTables / SensorDev from, and the predicate "the sections an update leaves to the device stayed where they were".  Host only, no HIP include
// (tests/cpp/blob_layout_check.cpp compiles it with g++ and holds the offsets of hand-counted cases).
//
// Sections in order, float4 words per item:
//   nodes 4 (bvh.h: 64 bytes) | traversal 3 | shading 6 | tangent 6 or none | slot map ceil(n / 4) | filter primitives 6
//   | small tables, always rewritten: mesh 2, bsdf 2 x max(1, n), emitter 2 x max(1, n), emitter pmf + cmf ceil(2 max(1, n) / 4), face pmf + cmf ceil(2 max(1, n) / 4)
//   | secondary edges 6, their pmf + cmf ceil(2 max(1, n) / 4)
//   | per sensor: primary edges 3, their pmf + cmf ceil(2 max(1, n) / 4)
#pragma once
#include <algorithm>
#include <cstddef>
#include <utility>
#include <vector>

#include "blob_rows.h"

namespace psdr {

struct BlobCounts {
    int n_tris = 0, n_nodes = 0, node_words = 4;      // node_words: bvh.h::kNodeFloats / 4 (a 4-wide node is 64 bytes)
    bool has_tan = false;
    int n_filt = 0, n_meshes = 0, n_bsdfs = 0, n_emitters = 0, n_face_distrb = 0, n_sec_edges = 0;
    std::vector<int> sensor_edges;       // primary edges every sensor carries
    size_t pe_cap = 0;                   // > 0, or `capped`: every sensor's edge arrays have room for this many edges and the CDF starts behind that room
    bool capped = false;                 // (psdr_hip_scene_update_edges sizes them once: the kept count changes from configure to configure, the sections behind must not move)
};

struct BlobLayout {
    int nodes = 0, trav = 0, shade = 0, tan = 0, map = 0, filt = 0;
    size_t small_begin = 0, small_end = 0;                  // the small tables: mesh, bsdf, emit, ecdf, fcdf
    int mesh = 0, bsdf = 0, emit = 0, ecdf = 0, fcdf = 0;
    int sec = 0, sec_cdf = 0;
    size_t sec_end = 0;
    int n_sec = 0;                                          // (as given: what SecEdgeTables::n holds)
    std::vector<std::pair<int, int>> pe;                    // per sensor (pe_off, pecdf_off)
    size_t words = 0;                                       // blob_words
};

// -> false: the scene is too large for 32-bit byte offsets into the blob
inline bool blob_layout(const BlobCounts &c, BlobLayout &L) {
    const size_t n = (size_t) c.n_tris;
    size_t w = 0;
    L.nodes = (int) w; w += (size_t) c.node_words * (size_t) c.n_nodes;      // nodes of the 4-wide tree (bvh.h: 64 bytes each)
    L.trav = (int) w;  w += kTravWords * n;
    L.shade = (int) w; w += kShadeWords * n;
    L.tan = (int) w;   w += c.has_tan ? kTanWords * n : 0;
    L.map = (int) w;   w += words_for_floats(n);
    L.filt = (int) w;  w += 6 * (size_t) c.n_filt;
    L.small_begin = w;
    L.mesh = (int) w;  w += 2 * (size_t) c.n_meshes;
    L.bsdf = (int) w;  w += 2 * (size_t) std::max(1, c.n_bsdfs);
    L.emit = (int) w;  w += 2 * (size_t) std::max(1, c.n_emitters);
    L.ecdf = (int) w;  w += words_for_floats(2 * (size_t) std::max(1, c.n_emitters));
    L.fcdf = (int) w;  w += words_for_floats(2 * (size_t) std::max(1, c.n_face_distrb));
    L.small_end = w;
    L.n_sec = c.n_sec_edges;
    L.sec = (int) w;     w += kSecWords * (size_t) std::max(0, c.n_sec_edges);
    L.sec_cdf = (int) w; w += words_for_floats(2 * (size_t) std::max(1, c.n_sec_edges));
    L.sec_end = w;
    L.pe.clear();
    for (int edges : c.sensor_edges) {
        const int ne = (c.capped || c.pe_cap > 0) ? (int) c.pe_cap : std::max(0, edges);
        const int o1 = (int) w; w += kPeWords * (size_t) ne;
        const int o2 = (int) w; w += words_for_floats(2 * (size_t) std::max(1, ne));
        L.pe.emplace_back(o1, o2);
    }
    L.words = w;
    return w <= 0x7fffffffull / 4;
}

// the secondary-edge section is where `Eold` (a SecEdgeTables) has it, with as many edges: the device's rows and distribution in it stand
template <typename SecTables> inline bool sec_section_kept(const BlobLayout &now, const SecTables &Eold) {
    return now.sec == Eold.off && now.sec_cdf == Eold.cdf_off && now.n_sec == Eold.n;
}

// every section the device writes for a moved mesh - traversal, shading and tangent rows (found through the slot map), secondary-edge rows - is where `Told` /
// `Eold` (SceneTables / SecEdgeTables) have it: the host's copy of such a section may be behind, so it must not have to be sent
template <typename Tables, typename SecTables> inline bool layout_kept(const BlobLayout &now, const Tables &Told, const SecTables &Eold, bool has_tan) {
    return now.trav == Told.trav_off && now.shade == Told.shade_off && now.tan == Told.tan_off && now.map == Told.map_off && (has_tan ? 1 : 0) == Told.has_tangent &&
           sec_section_kept(now, Eold);
}

// the offsets of SceneTables / SecEdgeTables, assigned from the layout in one place (the sensors' pairs go into SensorDev as each sensor is written)
template <typename Tables, typename SecTables> inline void assign_offsets(const BlobLayout &L, Tables &T, SecTables &E) {
    T.nodes_off = L.nodes; T.trav_off = L.trav; T.shade_off = L.shade; T.tan_off = L.tan; T.map_off = L.map; T.filt_off = L.filt;
    T.mesh_off = L.mesh; T.bsdf_off = L.bsdf; T.emit_off = L.emit; T.ecdf_off = L.ecdf; T.fcdf_off = L.fcdf;
    T.blob_words = (int) L.words;
    E.off = L.sec; E.cdf_off = L.sec_cdf; E.n = L.n_sec;
}

} // namespace psdr
