/* psdr_hip.h — C ABI of libpsdr_hip.so: the MI355X (gfx950) implementation of psdr-jit's
 * PathTracer.renderC / renderD hot path.
 *
 * The reference has no FFI seam for this path (Python -> pybind11 -> C++ virtuals -> drjit/OptiX,
 * reference src/psdr.cpp:100-441); the seam below is the one SURVEY.md §8(b) specifies: a POD
 * "configured-scene snapshot" (= what Scene::configure leaves in Scene's public SoA members,
 * reference include/psdr/scene/scene.h:56-90) plus render entry points that replace
 *   Integrator::renderC / renderD            reference src/integrator/integrator.cpp:12-100
 *   Integrator::__render / __render_batch    reference src/integrator/integrator.cpp:103-176
 *   Integrator::render_primary_edges         reference src/integrator/integrator.cpp:179-198
 *   PathTracer::__Li                         reference src/integrator/path.cpp:35-127
 *   PathTracer::render_secondary_edges       reference src/integrator/path.cpp:171-294
 *   PathTracer::preprocess_secondary_edges   reference src/integrator/path.cpp:130-168
 *   Scene::ray_intersect + Scene_OptiX       reference src/scene/scene.cpp:612-806, scene_optix.cpp:265-410
 *
 * Conventions: every function returns 0 on success, non-zero on error (message via
 * psdr_hip_last_error(), which mirrors psdr_jit::Exception's text, reference include/misc/Exception.h).
 * All pointers inside psdr_scene_snapshot are HOST pointers owned by the caller and are copied
 * during psdr_hip_scene_create.  Image buffers passed to the render calls are DEVICE pointers
 * owned by the caller (e.g. a torch tensor's data_ptr); `stream` is a hipStream_t (NULL = default
 * stream).  No call synchronises the device.  Float data is IEEE float32, indices int32, RNG state uint64.
 * Matrices are row-major float[16].  Tangent ("d_") arrays hold d(value)/d(theta) for ONE scalar scene
 * parameter theta (forward mode; the reference gets the same from drjit.forward_to) and may be NULL.
 */
#ifndef PSDR_HIP_H
#define PSDR_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* (psdr_hip_render_d_fwd_batch / psdr_hip_render_d_bwd_batch, and later psdr_hip_render_c_sq / psdr_hip_render_d_fwd_sq, were ADDED under version 16: no struct changed
 * its layout and no existing entry point its behaviour, so every ABI-16 caller stays valid; a caller that wants the added functions looks the symbols up) */
#define PSDR_HIP_ABI_VERSION 16

/* TriangleInfo SoA, reference include/psdr/types.h:162-175 (+ Scene::m_triangle_uv,
 * m_triangle_face_normals, scene.cpp:528-542).  Arrays of n_triangles rows. */
typedef struct psdr_triangles {
    int32_t n_triangles;
    const float *p0, *e1, *e2, *n0, *n1, *n2, *face_normal;   /* [n*3] each */
    const float *face_area;                                   /* [n]   */
    const float *uv;                                          /* [n*6] uv0 uv1 uv2, zeros if no uv */
    const int32_t *mesh_id;                                   /* [n]   */
    const uint8_t *use_face_normal;                           /* [n]   */
    const int32_t *face_indices;                              /* [n*3] mesh-local vertex ids (TriangleInfo::face_indices, types.h:172); may be NULL
                                                                 unless a MicrofacetPerVertex BSDF is present */
    /* forward tangents (NULL = none) */
    const float *d_p0, *d_e1, *d_e2, *d_n0, *d_n1, *d_n2, *d_face_normal, *d_face_area;
} psdr_triangles;

typedef struct psdr_mesh_rec {       /* what the kernels need of reference Mesh (mesh.h:82-141) */
    int32_t bsdf_id;                 /* -1 = none */
    int32_t emitter_id;              /* -1 = not an emitter */
    int32_t face_offset, n_faces;    /* rows of psdr_triangles */
    float inv_total_area;            /* Mesh::m_inv_total_area */
    /* Mesh::m_face_distrb (DiscreteDistribution over faces ~ area); used when emitter_id >= 0 */
    int32_t distrb_offset;           /* into psdr_scene_snapshot.face_pmf / face_cmf */
    float distrb_sum;
} psdr_mesh_rec;

typedef struct psdr_bsdf_rec {       /* Diffuse, reference src/bsdf/diffuse.cpp */
    int32_t type;                    /* 0 = Diffuse, 1 = Microfacet, 2 = RoughConductor, 3 = RoughDielectric, 4 = MicrofacetPerVertex, 5 = NormalMap */
    int32_t two_sided;
    float reflectance[3], d_reflectance[3];
    /* textured reflectance: Bitmap3fD with a resolution above 1x1 (bitmap.cpp:47-128, looked up at its.uv with flip_v);
     * tex_data != NULL overrides `reflectance`.  Host pointers, copied by psdr_hip_scene_create. */
    int32_t tex_width, tex_height;
    const float *tex_data;           /* [tex_height*tex_width*3] row-major rgb */
    const float *d_tex_data;         /* forward tangent of the texels, may be NULL */
    /* type 1 = Microfacet (src/bsdf/microfacet.cpp, ggx.cpp): `reflectance` is its diffuse reflectance, plus */
    float specular[3], d_specular[3];
    float roughness, d_roughness;
    /* type 2 = RoughConductor (src/bsdf/roughconductor.cpp): `specular` is its specular_reflectance, plus */
    float alpha_u, alpha_v, d_alpha_u, d_alpha_v;
    float eta[3], d_eta[3], k[3], d_k[3];
    /* type 3 = RoughDielectric (src/bsdf/roughdielectric.cpp): alpha_u / alpha_v as above, eta[0] = m_eta = intIOR / extIOR,
     * eta[1] = m_inv_eta = extIOR / intIOR (the reference stores both), d_eta[0..1] their tangents */
    /* Microfacet bitmap parameters with a resolution above 1x1 (microfacet.cpp:38-45, looked up at its.uv like tex_data, which
     * is then the diffuse reflectance map): override `specular` (rgb) / `roughness` (one channel).  Host pointers, copied. */
    int32_t spec_tex_width, spec_tex_height;
    const float *spec_tex_data, *d_spec_tex_data;
    int32_t rough_tex_width, rough_tex_height;
    const float *rough_tex_data, *d_rough_tex_data;
    /* type 4 = MicrofacetPerVertex (src/bsdf/microfacet_pv.cpp): parameters per mesh-local vertex, interpolated over the hit
     * triangle with the barycentrics (its.face_indices, its.bc).  Host pointers, copied. */
    int32_t pv_count;
    const float *pv_specular, *pv_diffuse, *pv_roughness;          /* [n*3], [n*3], [n] */
    const float *d_pv_specular, *d_pv_diffuse, *d_pv_roughness;    /* forward tangents, may be NULL */
    /* type 5 = NormalMap (src/bsdf/normalmap.cpp): `reflectance` / tex_data = the normal map (rgb in [0, 1], looked up at its.uv),
     * nested_bsdf = index in psdr_scene_snapshot.bsdfs of the BSDF it perturbs (any type but NormalMap; the host may append the
     * nested BSDF as an extra entry no mesh refers to) */
    int32_t nested_bsdf;
    /* uv transform of the three bitmap slots above (0 tex_data, 1 spec_tex_data, 2 rough_tex_data): Bitmap::m_rot, m_scale,
     * m_trans.x, m_trans.y (include/psdr/core/bitmap.h:37-39, applied by src/core/bitmap.cpp:64-86; the reference binds them as
     * rotate / scale / translate, src/psdr.cpp:204-206, 217-219) and their forward tangents.  Identity = {0, 1, 0, 0}.
     * Reverse mode: psdr_grads.g_uv_xf (ABI 12; until then four psdr_hip_render_d_fwd launches per bitmap). */
    float tex_xf[3][4], d_tex_xf[3][4];
} psdr_bsdf_rec;

typedef struct psdr_emitter_rec {    /* AreaLight (src/emitter/area.cpp) or EnvironmentMap (src/emitter/envmap.cpp) */
    int32_t mesh_id;                 /* the light's mesh; for the envmap the bounding cube scene.cpp:442-480 adds */
    float sampling_weight;           /* normalised, scene.cpp:511-514 */
    float radiance[3], d_radiance[3];
    int32_t type;                    /* 0 = AreaLight, 1 = EnvironmentMap (psdr_scene_snapshot.envmap) */
} psdr_emitter_rec;

/* EnvironmentMap after configure() (envmap.cpp:17-44): lat-long radiance, transform, the scene box it is carried to
 * (scene.cpp:436-440) and its HyperCubeDistribution2f over (2(W-1)) x (2(H-1)) cells, cell index = cx*reso[1] + cy */
typedef struct psdr_envmap_rec {
    int32_t width, height;
    const float *radiance;           /* [height*width*3] row-major rgb (Bitmap3fD m_radiance) */
    float scale;                     /* m_scale */
    float to_world[16], from_world[16];
    float lower[3], upper[3];
    int32_t reso[2];
    const float *cell_pmf, *cell_cmf; /* unnormalised masses and their running sums, [reso[0]*reso[1]] */
    float cell_sum;
    /* forward tangents of the differentiable members (envmap.h:40-45): texels of m_radiance (host pointer, may be NULL),
     * m_scale, m_to_world / m_from_world */
    const float *d_radiance;
    float d_scale;
    float d_to_world[16], d_from_world[16];
    /* uv transform of m_radiance (as psdr_bsdf_rec.tex_xf: rotate, scale, translate.x, translate.y) and its forward tangent;
     * cell_pmf / cell_cmf are the masses of the transformed map (envmap.cpp:28-31 evaluates m_radiance through Bitmap::eval) */
    float radiance_xf[4], d_radiance_xf[4];
} psdr_envmap_rec;

/* SecondaryEdgeInfo SoA, reference include/psdr/edge/edge.h:49-68 */
typedef struct psdr_sec_edges {
    int32_t n_edges;
    const float *p0, *e1, *n0, *n1, *p2;      /* [n*3] */
    const uint8_t *is_boundary;               /* [n] */
    const float *d_p0, *d_e1;                 /* tangents used by the estimator */
    const float *pmf, *cmf;                   /* Scene::m_sec_edge_distrb, [n] */
    float sum;
} psdr_sec_edges;

/* PerspectiveCamera after configure(), reference src/sensor/perspective.cpp:10-152 */
typedef struct psdr_sensor_rec {
    float sample_to_camera[16];
    float to_world[16], d_to_world[16];
    float world_to_sample[16], d_world_to_sample[16];
    float cam_pos[3], cam_dir[3];
    float inv_area;
    int32_t orthographic;            /* 1: OrthographicCamera (src/sensor/orthographic.cpp): rays start on the near plane along cam_dir */
    /* PrimaryEdgeInfo (edge.h:27-40) + Sensor::m_edge_distrb; n_edges == 0 disables the term */
    int32_t n_edges;
    const float *edge_p0, *edge_p1;           /* [n*2] sample-space end points */
    const float *d_edge_p0, *d_edge_p1;       /* [n*2] tangents */
    const float *edge_normal;                 /* [n*2] */
    const float *edge_length;                 /* [n] */
    const float *edge_pmf, *edge_cmf;         /* [n] */
    float edge_sum;
} psdr_sensor_rec;

/* What ONE mesh's rows of psdr_triangles / psdr_sec_edges are a function of (ABI 16): Mesh::configure + process_mesh, reference src/shape/mesh.cpp:23-62, 317-400, run on
 * drjit device arrays - the reference computes these rows ON THE GPU in every Scene::configure.  With psdr_scene_snapshot.geometry set, psdr_hip_scene_update computes the
 * rows of the meshes flagged `moved` on the device, in the host's own (value, tangent) arithmetic (csrc/host/hnum.h compiled for both sides: the same bits), from the raw vertices
 * and the composed transform: ~1 MB travels instead of the 30 MB of rows the host would write.  The snapshot's row arrays stay valid (they are what psdr_hip_scene_create,
 * a rebuild and the host-side consumers read); under psdr_hip_scene_update the edge distributions and the sensors' primary edges come from the host; psdr_hip_scene_update_edges selects the primary edges and builds both edge distributions on the device as well (only the float `sum`s are added on the host, from lengths read back). */
typedef struct psdr_mesh_geometry {
    int32_t n_vertices, n_faces, n_edges;          /* n_edges: this mesh's rows of psdr_sec_edges (0 when its edges are disabled or sppse == 0) */
    const float *vertices_raw, *d_vertices_raw;    /* [n_vertices*3] Mesh::m_vertex_positions_raw and its forward tangent */
    float to_world[16], d_to_world[16];            /* m_to_world_left * m_to_world_raw * m_to_world_right, row-major, composed in (value, tangent) arithmetic by the host */
    const int32_t *faces;                          /* [n_faces*3] mesh-local vertex ids (Mesh::m_face_indices) */
    const int32_t *vf_begin, *vf_item;             /* [n_vertices+1], [n_faces*3]: per vertex its (face << 2 | corner) incidences in the order the reference's three scatter passes
                                                      visit them (mesh.cpp:34-41), so that the per-vertex normal sums add in that very order */
    const int32_t *edges;                          /* [n_edges*5] v0 v1 f0 f1 opp (Mesh::m_edge_indices; f1 = -1: boundary edge) */
    int32_t mesh_id, use_face_normals;
    uint64_t topology_version;                     /* changes whenever faces / vf lists / edges / the counts do: the device keeps the topology of the version it saw last */
    int32_t moved;                                 /* 1: vertices, transform or their tangents differ from what the previous create / update carried */
} psdr_mesh_geometry;

typedef struct psdr_scene_snapshot {
    int32_t abi_version;                      /* PSDR_HIP_ABI_VERSION */
    int32_t width, height, spp, sppe, sppse;  /* RenderOption, reference include/psdr/types.h:217-228 */
    psdr_triangles tris;
    int32_t n_meshes;   const psdr_mesh_rec *meshes;
    int32_t n_bsdfs;    const psdr_bsdf_rec *bsdfs;
    int32_t n_emitters; const psdr_emitter_rec *emitters;
    const float *emitter_pmf, *emitter_cmf;   /* Scene::m_emitters_distrb, [n_emitters] */
    float emitter_sum;
    int32_t n_face_distrb;                    /* total length of the concatenated face CDFs */
    const float *face_pmf, *face_cmf;
    psdr_sec_edges sec_edges;
    int32_t n_sensors;  const psdr_sensor_rec *sensors;
    const psdr_envmap_rec *envmap;            /* Scene::m_emitter_env, NULL = none */
    const psdr_mesh_geometry *geometry;       /* [n_meshes] or NULL: lets psdr_hip_scene_update compute moved meshes' rows on the device (BVH scenes; see psdr_mesh_geometry) */
    int32_t rows_valid;                       /* psdr_hip_scene_update only.  1: the row arrays of `tris` and `sec_edges` hold this state.  0: the caller has not computed the rows of
                                                 the moved meshes (their sizes, the CDFs and everything else are valid) and relies on `geometry`: the update computes them on the
                                                 device, or returns PSDR_HIP_NEED_ROWS with the scene unchanged - then call again with the rows */
} psdr_scene_snapshot;

/* One of Scene::m_samplers[0..2] in closed form: lane i was seeded with
 * seed_value = seed + (pix_ids ? pix_ids[i / spp] : i) (integrator.cpp:24-28, scene.cpp:330-344)
 * and has already produced `skip` numbers.  The kernels never store per-lane RNG state. */
typedef struct psdr_sampler {
    uint64_t seed;
    uint64_t skip;
} psdr_sampler;

#define PSDR_SHARD_CHUNK 256
#define PSDR_SHARD_INTERLEAVED 0
#define PSDR_SHARD_ROWS 1

#define PSDR_TERM_INTERIOR  1
#define PSDR_TERM_PRIMARY   2
#define PSDR_TERM_SECONDARY 4

typedef struct psdr_hip_scene psdr_hip_scene;      /* device-resident scene + BVH */
typedef struct psdr_hip_guiding psdr_hip_guiding;  /* device-resident HyperCubeDistribution3f */

typedef struct psdr_render_args {
    int32_t sensor_id;
    int32_t max_depth;            /* PathTracer(max_depth) */
    int32_t hide_emitters;        /* PathTracer::m_hide_emitters */
    psdr_sampler samplers[3];     /* interior / primary edge / secondary edge */
    const int32_t *pix_ids;       /* DEVICE pointer, batch_pix (integrator.cpp:139-176); NULL = full frame.  psdr_hip_render_d_fwd / _bwd: interior term only;
                                     psdr_hip_render_d_fwd_batch / _bwd_batch: interior term + the edge terms of the listed pixels */
    int32_t n_pix;
    int32_t terms;                /* PSDR_TERM_* mask (renderD only) */
    int32_t shard_rank, shard_count;  /* multi-GPU: rank r of c evaluates the PSDR_SHARD_CHUNK-lane chunks k of each
                                       * sampler's lane range with k % c == r (interleaved for load balance); c<=1 = all */
    const psdr_hip_guiding *guiding;  /* NULL = unguided secondary edges */
    int32_t zero_output;          /* 1: the call clears out buffers first (hipMemsetAsync on `stream`) */
    int32_t direct_mode;          /* 0: PathTracer(max_depth); 1 + mis: DirectIntegrator(mis), mis = 0/1/2 (reference
                                     src/integrator/direct.cpp:34-132: emitter sample only / BSDF sample only / both with MIS) */
    int32_t field_mode;           /* 0: none; 1 + f: first-hit integrators (no secondary-edge term): FieldExtractionIntegrator (reference
                                     src/integrator/field.cpp) f = 0 silhouette, 1 position, 2 depth, 3 geoNormal, 4 shNormal, 5 uv, 6 bsdf,
                                     7 segmentation; f = 8: CollocatedIntegrator(intensity) (src/integrator/collocated.cpp) */
    int32_t field_object;         /* mesh index the field is restricted to (field.cpp:59-66), -1 = all; only read when field_mode > 0 */
    float intensity, d_intensity; /* CollocatedIntegrator::m_intensity and its forward tangent */
    int32_t skip_static_edges;    /* psdr_hip_render_d_fwd, primary-edge term: 1 = a sample whose edge point has a zero normal velocity under the installed
                                     tangents (an edge of a mesh that does not move, a camera that does not move) is not traced - its contribution to out_drgb is
                                     d(x.n) x (Ln - Lp) / pdf = exactly 0 (integrator.cpp:179-198), so the same numbers are added to the derivative image; 0 = every sample's
                                     two paths are traced, as the reference does */
    int32_t shard_mode;           /* multi-GPU partition of every sampler's lanes over shard_count ranks (ABI 15): PSDR_SHARD_INTERLEAVED (0) = the chunks k % c == r above;
                                     PSDR_SHARD_ROWS (1) = CONTIGUOUS ranges - the interior sampler by whole pixel rows (rank r renders rows [r R, (r + 1) R), R = ceil(H / c):
                                     one block of the image per rank, which an all-gather assembles; batch rendering: by whole pixels of the list), the two edge samplers by
                                     equal runs of whole PSDR_SHARD_CHUNK-lane chunks.  Every lane's random stream is a function of (seed, lane), so both partitions add up to
                                     the same frame; the reference's nearest hook is batch_pix (integrator.cpp:139-176) */
} psdr_render_args;

/* counters of the instrumented build: filled by psdr_hip_render_*_counted */
typedef struct psdr_counters {
    uint64_t rays, nodes_visited, tris_tested, shaded_hits;
} psdr_counters;

/* Threading / streams: every entry point that launches kernels takes the stream to launch on.  Calls on one stream are ordered by
 * the stream.  The launches of ONE scene share device scratch (work-queue ring, traversal-stack overflow, adjoint records), so calls
 * on the same scene from different streams or host threads are serialised by the library: a call first makes its stream wait for
 * the completion event of the scene's previous call (no host synchronisation).  Different scenes run concurrently.
 *
 * THE STREAM CONTRACT (tests/test_gpu_streams.py runs every entry point on a side stream behind a delay):
 *   1. All device work of a call that takes a `stream` - kernels, clears, copies, the scratch it allocates inside the call - is issued to that stream or to streams
 *      the call forks from it and joins into it before it returns (the edge terms of a BVH scene's renderD).  Nothing goes to the NULL stream, with which streams
 *      created non-blocking (torch's pool streams) do not synchronise.
 *   2. The caller's duty: every device input of the call is ready ON THE STREAM THAT IS PASSED (written by work queued on it earlier, or complete before the call),
 *      and the outputs are read on that stream or after it has been waited for.
 *   3. Every psdr_hip_*_create (scene, guiding_build, precond, denoise, vdenoise, subdiv, msloss, ssim, meshreg) returns with the handle usable on ANY stream and with the caller's host and
 *      device arrays free again: it synchronises `stream` (the scene calls: the NULL stream they work on) before it returns.  They are cold paths.
 *   4. What the library serialises: calls on ONE SCENE from different streams (above).  psdr_hip_scene_update waits on the host for the scene's last call before it
 *      rewrites anything, works on the NULL stream and synchronises it before it returns: a render queued before it sees the old state, one issued after it the new.
 *   5. What it does not: a denoise / vdenoise / precond / msloss handle owns work frames and so does an ssim handle, so calls on one such handle must follow each other on one stream or be ordered
 *      by the caller; the same holds for a meshreg handle (it owns the contribution buffers and partial sums of its eval).  subdiv handles are read-only after the create and
 *      may be applied from any number of streams.  The chamfer entry points (psdr_hip_chamfer_nearest, psdr_hip_chamfer_eval) have no handle and no create: their work
 *      arrays (keys, partial) are the caller's, one set per call in flight, and psdr_hip_chamfer_plan touches no device; the grid search beside them is stateless too
 *      (psdr_hip_chamfer_grid_build, psdr_hip_chamfer_grid_nearest: the grid, work, keys, list and stats are the caller's - a built grid is read-only and may be searched
 *      from any number of streams that wait for its build; psdr_hip_chamfer_grid_plan touches no device).  The same holds for the point-to-mesh entry points
 *      (psdr_hip_pointmesh_nearest, psdr_hip_pointmesh_eval: records, keys, corners and partial are the caller's; psdr_hip_pointmesh_plan touches no device) and for the
 *      signed-distance entry points (psdr_hip_sdf_winding, psdr_hip_sdf_grad: records, partial and corners are the caller's), and for the isosurface entry points
 *      (psdr_hip_mtet_count, psdr_hip_mtet_emit, psdr_hip_mtet_vertices, psdr_hip_mtet_vertices_adj: mask, base, the cell arrays, scratch and totals are the caller's and
 *      none of them synchronises - the caller reads totals after waiting for `stream` itself; psdr_hip_mtet_plan touches no device), and for the lattice regularisers
 *      (psdr_hip_latreg_eval: scratch, out, crossings and grad are the caller's; psdr_hip_latreg_plan touches no device).
 * "No call synchronises the device" (above) means hipDeviceSynchronize; the calls that wait for their own stream say so: the creates, psdr_hip_guiding_build,
 * psdr_hip_precond_solve (it reads its residuals), the *_counted renders, and a render that has to grow the scene's scratch (first call, or a larger one). */
const char *psdr_hip_last_error(void);
int psdr_hip_abi_version(void);
int psdr_hip_device_count(void);
int psdr_hip_set_device(int device);

/* replaces Scene_OptiX::configure (GAS build) + the jit uploads of Scene::configure */
int psdr_hip_scene_create(const psdr_scene_snapshot *snapshot, psdr_hip_scene **out);
int psdr_hip_scene_destroy(psdr_hip_scene *scene);
/* Scene::configure() AGAIN on a scene that already has a device copy (the reference's per-step pattern, README.md:87-106: set_transform ->
 * configure -> renderD -> backward; the reference re-uploads every array and rebuilds its OptiX GAS each time, src/scene/scene.cpp:311-599,
 * src/scene/scene_optix.cpp:265-332).  The new snapshot replaces the old one inside the same handle (guiding grids built from the old state
 * are the caller's to rebuild, as PathTracer::preprocess_secondary_edges is in the reference):
 *   - same triangle count: the tree and the triangle order are kept.  Moved triangles -> the 4-wide tree is refitted on the device (bottom-up, the
 *     builder's own box padding and quantisation), and built again only when the refitted tree's SAH cost exceeds 1.4 x the cost it was built with;
 *   - another triangle count: the tree is built again (host threads).
 * `same`: PSDR_SAME_* bits by which the caller vouches that a part of the snapshot holds the values of the previous create / update of this handle -
 * such a part is neither rewritten nor sent.  0 is always correct (everything is rewritten; the tree is still kept and refitted).  The call waits for
 * the scene's pending render calls and returns when the device copy is complete; `info` (may be NULL) says what was done. */
#define PSDR_SAME_TRIANGLES     1u   /* every array of psdr_triangles except the d_ (tangent) arrays */
#define PSDR_SAME_TRI_TANGENTS  2u   /* the d_ arrays of psdr_triangles */
#define PSDR_SAME_SEC_EDGES     4u   /* psdr_sec_edges, tangents included */
#define PSDR_SAME_PRIM_EDGES    8u   /* the primary-edge arrays of every sensor, tangents included */
#define PSDR_SAME_ENV_TEXELS   16u   /* psdr_envmap_rec.radiance, cell_pmf, cell_cmf (not its transform, scale or tangents) */
#define PSDR_SAME_ENV_TANGENT  32u   /* psdr_envmap_rec.d_radiance */
#define PSDR_SAME_BITMAPS      64u   /* the texel / per-vertex arrays of every psdr_bsdf_rec and their tangents (not the constants or uv transforms) */
typedef struct psdr_update_info {
    int32_t tree;                    /* 0 kept as it was, 1 refitted on the device, 2 built */
    int32_t reallocated;             /* device allocations whose size changed */
    int64_t bytes_uploaded;
    double sah_cost, sah_cost_built; /* SAH cost of the tree now / when it was built (sum over child boxes of half-area x triangles-or-1, over the root's half-area) */
    double ms_tree, ms_fill, ms_upload, ms_total;   /* host wall clock: tree build / refit, writing the host copy, copies issued, whole call */
} psdr_update_info;
#define PSDR_HIP_NEED_ROWS 2          /* psdr_hip_scene_update: snapshot->rows_valid == 0 and this update cannot do without the rows (see psdr_scene_snapshot.rows_valid) */
int psdr_hip_scene_update(psdr_hip_scene *scene, const psdr_scene_snapshot *snapshot, uint32_t same, psdr_update_info *info);
/* what the last create / update of this handle did */
int psdr_hip_scene_last_update(const psdr_hip_scene *scene, psdr_update_info *info);
/* test aid (synchronises, downloads the tree): number of places where the device tree is NOT a bounding hierarchy of the device triangles - a child
 * box that does not contain the padded box of a triangle below it, a triangle slot under no or several leaves.  0 for brute-force scenes. */
int psdr_hip_scene_check_tree(const psdr_hip_scene *scene, int64_t *violations);
/* test aid (synchronises, downloads the sections): 32-bit words of the device's triangle rows (traversal, shading, tangent) and secondary-edge rows that differ from the rows
 * the host path would write from `snapshot` - 0 when the kernels that compute a moved mesh's rows on the device (psdr_mesh_geometry) produced the host's bits */
int psdr_hip_scene_check_rows(const psdr_hip_scene *scene, const psdr_scene_snapshot *snapshot, int64_t *mismatches);
/* PRIMARY EDGES ON THE DEVICE.  The reference selects every configured sensor's primary edges on drjit device arrays in each Scene::configure (the silhouette test and compressD,
 * src/sensor/perspective.cpp:52-151).  psdr_hip_scene_update_edges is psdr_hip_scene_update plus that: with the world vertices, face normals and areas of psdr_mesh_geometry resident on
 * the device, the sensors marked PSDR_EDGES_DEVICE get their edges selected there - keep flags, a stable compaction (the order of an in-order walk over meshes and edges), the rows, in
 * the host's own arithmetic (csrc/host/edge_select.h compiled for both sides: the same bits) - and no array proportional to an edge count travels to the device.  The distribution
 * (DiscreteDistribution::init, src/core/pmf.cpp:6-15: a sequential double-precision running sum rounded to float per entry, and a sequential float sum) is completed there too: the
 * cmf by a parallel scan where every partial sum is provably exact in double (exponent range of the lengths + 24 + log2 n bits within 53, checked on the device); the kept lengths and
 * ids come BACK (16 B per kept edge, device to host) and the host adds the float sum - and, where the bound does not hold, runs the sequential form itself and sends that cmf (4 B
 * per entry: the only edge-proportional bytes that can still go up).
 * Memory: under this call every sensor's edge arrays have room for every edge of the meshes with edges (56 B per edge and sensor, in the scene blob and its pinned host copy);
 * psdr_hip_scene_create reserves that room for BVH scenes with `geometry` and sppe > 0 (from psdr_mesh_geometry.n_edges - nothing when sppse == 0: the first such update then moves
 * the blob once), and a scene that has been given the size keeps it under psdr_hip_scene_update.  After an update in which the HOST wrote triangle rows, the next device update recomputes
 * the world vertices of every mesh, not only of the moved ones.
 * Under this call every sensor's edge arrays are sized once, to the number of edges of the meshes with edges: a later call never moves them.
 *   topo [snapshot->n_meshes]: the edge list of every mesh (read when a topology_version, count or flag differs from what the device saw last)
 *   sensor_mode [snapshot->n_sensors]: PSDR_EDGES_HOST - the snapshot's edge arrays of this sensor, as psdr_hip_scene_update; PSDR_EDGES_DEVICE - select them on the device (the
 *     snapshot's edge pointers, n_edges and edge_sum of this sensor are ignored); PSDR_EDGES_KEEP - what an earlier PSDR_EDGES_DEVICE selected still holds (same meshes, same sensor)
 * Returns PSDR_HIP_NEED_ROWS with the scene unchanged when a sensor is not PSDR_EDGES_HOST and the device cannot do it now (a brute-force scene, a tree to build, a blob that moves,
 * snapshot->geometry NULL, world vertices not resident yet, PSDR_HOST_GEOMETRY set): call again with PSDR_EDGES_HOST for every sensor and the edge arrays filled. */
typedef struct psdr_edge_topology {
    int32_t n_edges;                 /* edges of the mesh (Mesh::m_edge_indices) */
    const int32_t *edges;            /* [n_edges*5] v0 v1 f0 f1 opp, mesh-local ids; f1 = -1: boundary edge */
    const uint8_t *uv_seam;          /* [n_edges] 1: the two faces do not share exactly two uv indices (perspective.cpp:95-110); NULL: the mesh has no uv coordinates */
    int32_t enabled;                 /* Mesh::m_enable_edges */
    uint64_t topology_version;       /* changes whenever edges / uv_seam do */
} psdr_edge_topology;
#define PSDR_EDGES_HOST   0
#define PSDR_EDGES_DEVICE 1
#define PSDR_EDGES_KEEP   2
int psdr_hip_scene_update_edges(psdr_hip_scene *scene, const psdr_scene_snapshot *snapshot, uint32_t same, const psdr_edge_topology *topo, const int32_t *sensor_mode,
                                psdr_update_info *info);
/* what a sensor keeps (perspective.cpp:112-151): *count edges, *edge_sum = Sensor::m_edge_distrb.sum(); ids (HOST [cap*3], may be NULL): (Mesh id, v0, v1) of the kept edges in their
 * order - only for a sensor whose edges the device selected */
int psdr_hip_scene_primary_edges(const psdr_hip_scene *scene, int32_t sensor_id, int32_t *count, int32_t *ids, int32_t cap, float *edge_sum);
/* test aid (synchronises, downloads the sections): 32-bit words in which the device's primary-edge arrays and distribution of every sensor and the secondary-edge distribution differ
 * from what the host path would write from `snapshot` (its edge arrays filled) - 0 when the device's selection produced the host's bits in the host's order */
int psdr_hip_scene_check_edges(const psdr_hip_scene *scene, const psdr_scene_snapshot *snapshot, int64_t *mismatches);
/* what the last create / update COMPUTED: *path = 0 no edge array or edge distribution was made on the device in it (they came from the host's arrays, or stood as they were:
 * PSDR_EDGES_KEEP, PSDR_SAME_SEC_EDGES), 1 it selected a sensor's primary edges and / or built the secondary-edge distribution on the device and every cmf came from the parallel scan,
 * 2 as 1 but a cmf needed the sequential form; *edge_bytes = bytes it sent host to device for the sensors' primary edges (rows, distributions, search tables, the edge list) and for the
 * secondary-edge distribution (pmf, cmf, search table; not the secondary-edge rows) */
int psdr_hip_scene_edge_path(const psdr_hip_scene *scene, int32_t *path, int64_t *edge_bytes);
/* BVH statistics for DESIGN/bench: nodes, leaves, max depth, bytes resident in LDS per workgroup */
int psdr_hip_scene_stats(const psdr_hip_scene *scene, int32_t *n_nodes, int32_t *n_leaves, int32_t *max_depth, int32_t *lds_bytes);
/* bytes of the scene's global per-lane records of the interior adjoint: 0 until a psdr_hip_render_d_bwd whose records do not fit LDS (deep paths) has allocated them
 * inside the call, on its stream - what a test reads to know that such a call took that path */
int64_t psdr_hip_scene_adjoint_record_bytes(const psdr_hip_scene *scene);
/* The live-pixel mask of a sensor (HOST bits[(width*height + 31) / 32], bit y*width + x; either pointer may be NULL): a pixel is dead when
 * no ray through its square can reach a triangle - the conservative screen-space coverage of the scene, built at scene creation.  The
 * interior term of every sample of a dead pixel is exactly zero (Integrator::__render, src/integrator/integrator.cpp:103-131: the
 * camera ray misses), and psdr_hip_render_c / _d_fwd skip such samples before seeding them.  All ones: no mask (environment-lit
 * scenes, a triangle across the camera plane, 2^31 lanes or more, less than a quarter of the frame dead, PSDR_NO_LIVE_MASK=1 in the
 * environment). */
int psdr_hip_scene_live_pixels(const psdr_hip_scene *scene, int32_t sensor_id, uint32_t *bits, int64_t *n_live);
/* The camera-ray table of a sensor (ADDED under version 16; every pointer may be NULL): the same screen-space coverage kept apart per triangle - one 64-bit
 * word per cell of *cell x *cell pixels (1, or the smallest power of two that keeps the table within 4 MB), HOST table[*cells_h * *cells_w], cell (y / *cell) *
 * *cells_w + x / *cell, bit k = the triangle in device slot k (psdr_hip_ray_intersect_ad's out_hit) comes within a quarter of a pixel of the cell.  The interior
 * term of psdr_hip_render_c / _d_fwd resolves a sample's camera ray against the triangles of its pixel's cell alone, with the tracer's own test and its
 * (t, id) order, so the hit is the tracer's.  *cell = 0: no table (more than 64 triangles, an environment map, a triangle across the camera plane,
 * an orthographic sensor, PSDR_NO_CAM_TABLE=1 in the environment: every camera ray goes through the tracer, as before the table existed). */
int psdr_hip_scene_camera_table(const psdr_hip_scene *scene, int32_t sensor_id, int32_t *cell, int32_t *cells_w, int32_t *cells_h, uint64_t *table);
/* bytes of one node of the 4-wide BVH this build walks (64: quantised child boxes, csrc/hip/bvh.h) - the unit of the algorithmic
 * bytes bench.py prices a node visit at */
int psdr_hip_bvh_node_bytes(void);

/* Scene::ray_intersect<false> for a batch of rays (reference src/scene/scene.cpp:612-806; bound to Python as
 * Scene.unit_ray_intersect, src/psdr.cpp:404).  Device arrays o[n*3], d[n*3] -> out[n*24]:
 * {valid, mesh id (-1 = miss), t, J, p.xyz, n.xyz (geometric), sh_frame.s.xyz, .t.xyz, .n.xyz, wi.xyz (local), uv.xy} */
#define PSDR_ITS_STRIDE 24
int psdr_hip_ray_intersect(const psdr_hip_scene *scene, int32_t n, const float *o, const float *d, float *out, void *stream);
/* Scene::ray_intersect<true> (reference src/scene/scene.cpp:774-797, ad = true, path_space = false; bound to Python as
 * Scene.unit_ray_intersectAD, src/psdr.cpp:405): the record of the differentiable re-intersection of the hit triangle
 * (ray_intersect_triangle<true>, include/psdr/utils.h:83-93), same layout as above, J = 1.  d_o[n*3], d_d[n*3]: tangents of the
 * rays (NULL = zero); the triangle rows carry the scene's installed tangents.  out_d[n*24]: the record's forward tangent (NULL = not
 * wanted).  out_hit[n]: the hit's slot in the device scene (-1 = miss), an opaque handle for the adjoint below, valid until the
 * scene is updated again. */
int psdr_hip_ray_intersect_ad(const psdr_hip_scene *scene, int32_t n, const float *o, const float *d,
                              const float *d_o, const float *d_d,
                              float *out, float *out_d, int32_t *out_hit, void *stream);
/* The transpose of the record above (reference: drjit's backward through scene.cpp:774-797), from the slots it returned, without a
 * traversal.  g_rec[n*24]: adjoint of the record (the valid / mesh / J words are ignored).  Writes g_o[n*3], g_d[n*3] (each may be
 * NULL; zero for misses and all-zero rows of g_rec) and ADDS the triangle-row adjoints [p0 e1 e2 n0 n1 n2 face_normal] into
 * g_triangles[n_triangles*22] (psdr_grads.g_triangles layout, original triangle order; face_area gets nothing; NULL = not wanted),
 * only for the meshes with mesh_filter[mesh] != 0 (NULL = all).  Non-finite values add nothing. */
int psdr_hip_ray_intersect_adj(const psdr_hip_scene *scene, int32_t n, const float *o, const float *d,
                               const int32_t *hit, const float *g_rec, const uint8_t *mesh_filter,
                               float *g_triangles, float *g_o, float *g_d, void *stream);
/* closest hit for a batch of rays (device arrays o[n*3], d[n*3] -> tri[n], uv[n*2], t[n]); parity aid */
int psdr_hip_trace(const psdr_hip_scene *scene, int32_t n, const float *o, const float *d,
                   int32_t *out_tri, float *out_uv, float *out_t, void *stream);
/* same query, two rays per lane through the two-ray tracer the path kernels use (rays 2i, 2i+1 share a lane) */
int psdr_hip_trace_pairs(const psdr_hip_scene *scene, int32_t n, const float *o, const float *d,
                         int32_t *out_tri, float *out_uv, float *out_t, void *stream);

/* EnvironmentMap::sample_position / sample_position_pdf alone (envmap.cpp:91-166; device arrays; parity aids):
 * ref_p[n*3], s2[n*2] -> p[n*3] on the scene box, its normal n[n*3], pdf[n];  ref_p, p, nrm -> pdf[n] */
int psdr_hip_env_sample(const psdr_hip_scene *scene, int32_t n, const float *ref_p, const float *s2,
                        float *out_p, float *out_n, float *out_pdf, void *stream);
int psdr_hip_env_pdf(const psdr_hip_scene *scene, int32_t n, const float *ref_p, const float *p, const float *nrm,
                     float *out_pdf, void *stream);

/* EnvironmentMap::configure, the cell masses of its HyperCubeDistribution2f (reference src/emitter/envmap.cpp:17-44,
 * src/core/cube_distrb.cpp:22-29: luminance x sin(theta) at the centre of each of the 2(W-1) x 2(H-1) cells, which the
 * reference evaluates on the device in every Scene::configure).  HOST arrays: texels[height*width*3] ->
 * mass[2(width-1) * 2(height-1)], cell index = cx * 2(height-1) + cy.  The prefix sums stay with the caller. */
int psdr_hip_env_cell_masses(const float *texels, int32_t width, int32_t height, float *mass);
/* the same with m_radiance's uv transform uv_xf[4] = rotate, scale, translate.x, translate.y (psdr_envmap_rec.radiance_xf;
 * NULL = identity): envmap.cpp:28-31 looks the cell centres up through Bitmap::eval, bitmap.cpp:64-86 */
int psdr_hip_env_cell_masses_xf(const float *texels, int32_t width, int32_t height, const float *uv_xf, float *mass);

/* Integrator::renderC: out_rgb is [n_pixels*3] float32, pixel-interleaved, pixel = y*W + x */
int psdr_hip_render_c(const psdr_hip_scene *scene, const psdr_render_args *args, float *out_rgb, void *stream);
/* Integrator::renderD + forward derivative: out_rgb = image, out_drgb = d image / d theta */
int psdr_hip_render_d_fwd(const psdr_hip_scene *scene, const psdr_render_args *args,
                          float *out_rgb, float *out_drgb, void *stream);
/* Batch rendering WITH the edge terms (what Integrator::renderD means to do for a pixel list, integrator.cpp:68-90, where it seeds samplers 1 and 2 with the
 * full-frame counts and calls render_primary_edges / render_secondary_edges - and then scatters at the full-frame pixel index into a result of n_pix rows,
 * integrator.cpp:195).  Requires args->pix_ids (n_pix full-frame pixel ids, duplicates allowed, any order).  Row k of out_drgb = the interior derivative of row k,
 * as psdr_hip_render_d_fwd gives it for the same list, PLUS the full-frame primary- and secondary-edge derivative of pixel pix_ids[k]: the edge samplers run over the
 * full-frame lane counts (W*H*sppe, W*H*sppse; args->samplers[1..2], guiding, shard_rank / shard_count / shard_mode exactly as in the full-frame call with the same
 * arguments), and a sample whose pixel is not listed is dropped BEFORE its rays are traced - the primary-edge sample at sampling time, the secondary-edge sample once
 * the hit of its opposite ray has been projected to the sensor.  A pixel listed twice receives its edge share in both rows.  args->terms selects the terms as in
 * psdr_hip_render_d_fwd (0 = all three).  The shards of such a call add up to the unsharded call, as those of the full frame do. */
int psdr_hip_render_d_fwd_batch(const psdr_hip_scene *scene, const psdr_render_args *args,
                                float *out_rgb, float *out_drgb, void *stream);
/* psdr_hip_render_c / psdr_hip_render_d_fwd WITH the per-pixel sums of squared sample contributions (a diagnostic the reference does not have; DESIGN.md, "Sample
 * squares").  out_sq / out_dsq have the layout of out_rgb / out_drgb, and
 *     out_sq[p, c]  = the sum, over the samples of the launched terms, of (what that sample adds to out_rgb[p, c])^2,        out_dsq: the same for out_drgb:
 * interior image (value / spp)^2, interior derivative (tangent / spp)^2, an edge sample (its whole, already / sppe or / sppse and / pdf divided, contribution)^2 - each
 * after the NaN / Inf scrub of the plain call, so a scrubbed or zero contribution adds nothing to either buffer.  For ONE term with n independent samples behind a pixel
 * estimate m - n = spp for the interior term, W*H*sppe and W*H*sppse for the edge terms, whose samples may land on any pixel - the unbiased variance of m is
 * (sq - m*m/n) * n/(n-1).  Independent terms add: with several terms in args->terms, out_dsq is the SUM of their raw second moments, and the exact variance of such a
 * derivative is the sum over single-term calls.  out_rgb / out_drgb and the sampler streams are those of the plain call with the same arguments (other order of the
 * float atomics); args->pix_ids, terms, the shards in both modes, guiding, direct_mode, field_mode, hide_emitters, skip_static_edges and zero_output (which also clears
 * the two new buffers) mean what they mean there - a pixel list has the interior term only; the squares of psdr_hip_render_d_fwd_batch do not exist.  The shards of
 * such a call add up to the unsharded call in all four buffers.  NULL scene, args or output pointers are refused before any device call.
 * Range: the squares are float32 like the sums, so a contribution below ~1e-19 in magnitude adds 0 and one above ~1.8e19 (finite, so it passes the scrub) adds +inf
 * to the square while the image stays finite; such an entry says "one sample dominates", not a variance. */
int psdr_hip_render_c_sq(const psdr_hip_scene *scene, const psdr_render_args *args, float *out_rgb, float *out_sq, void *stream);
int psdr_hip_render_d_fwd_sq(const psdr_hip_scene *scene, const psdr_render_args *args,
                             float *out_rgb, float *out_drgb, float *out_sq, float *out_dsq, void *stream);
/* Reverse mode of renderD (the reference's drjit.backward through Integrator::renderD, README.md:102-106):
 * given d_rgb = d loss / d image ([n_pixels*3], device), accumulate the adjoints of the snapshot quantities
 * the image depends on.  All buffers are DEVICE pointers owned by the caller; rows follow the snapshot order.
 * The host chains them to vertices / transforms / colours / camera pose.  With args->pix_ids (batch rendering) d_rgb is
 * [n_pix*3] and only the interior term exists, as in the forward path (psdr_hip_render_d_bwd_batch has the edge terms too).  g_bsdf / g_mat / psdr_hip_scene_tex_layout rows cover
 * every entry of psdr_scene_snapshot.bsdfs, including the records nested in normal maps. */
typedef struct psdr_grads {
    float *g_triangles;    /* [n_triangles*22] rows [p0 e1 e2 n0 n1 n2 face_normal face_area] */
    float *g_bsdf;         /* [n_bsdfs*3] reflectance */
    float *g_emitter;      /* [n_emitters*3] radiance */
    float *g_sec_edges;    /* [n_sec_edges*6] (p0, e1); required when sppse > 0 and the term is requested */
    float *g_prim_edges;   /* [n_primary_edges(sensor)*4] sample-space (p0.xy, p1.xy); required when sppe > 0 */
    /* optional filter (autograd's requires_grad at the level of the snapshot): the interior adjoint skips what is not wanted */
    const uint8_t *mesh_filter;   /* DEVICE [n_meshes]: 1 = triangle rows of this mesh are wanted; NULL = all meshes */
    int32_t skip_bsdf, skip_emitter;   /* 1 = g_bsdf / g_emitter are not wanted (left untouched by the interior term) */
    /* texel adjoints of the bitmap parameters (drjit.backward into Bitmap3fD / Bitmap1fD data): DEVICE [total] floats laid out
     * as psdr_hip_scene_tex_layout reports, or NULL = not wanted */
    float *g_tex;
    /* adjoint of the sensor's to_world through the camera rays of the interior and secondary-edge terms (DEVICE [16], row major,
     * rows 0-2 filled), or NULL = not wanted.  The camera's share of the primary-edge term arrives through g_prim_edges (sample-space edge
     * endpoints = world_to_sample . vertex: the host chains both). */
    float *g_camera;
    /* adjoints of the environment map: its texels (DEVICE [height*width*3]) and its scale (DEVICE [1]); NULL = not wanted */
    float *g_env, *g_env_scale;
    /* adjoints of the constant parameters of the GGX BSDFs, DEVICE [n_bsdfs*16], one row per BSDF, or NULL = not wanted:
     *   Microfacet      [specular rgb, roughness]
     *   RoughConductor  [alpha_u, alpha_v, eta rgb, k rgb, specular_reflectance rgb]
     *   RoughDielectric [alpha_u, alpha_v, eta (= intIOR / extIOR)]                     (the diffuse colour stays in g_bsdf) */
    float *g_mat;
    /* adjoint of the environment map's from_world (DEVICE [16], row major; the 3x3 block that maps world directions), or NULL */
    float *g_env_from_world;
    /* adjoints of the bitmaps' uv transforms (psdr_bsdf_rec.tex_xf, psdr_emitter_rec's radiance transform): DEVICE
     * [(3*n_bsdfs + 1)*4], row 3*b + k = [rotate, scale, translate.x, translate.y] of bitmap k of BSDF b, last row = the environment
     * map's; or NULL = not wanted.  Every lookup of the interior term adds its share in the same pass that fills g_tex / g_env:
     * give g_tex beside it for the rows of BSDF bitmaps and g_env for the environment map's row (the record-and-probe form visits a
     * lookup only for a buffer that is wanted).  The edge terms do not see the transforms (their values are
     * detached, src/integrator/integrator.cpp:179-198, path.cpp:171-270). */
    float *g_uv_xf;
    /* primary-edge term: DEVICE [n_primary_edges(sensor)], 1 = the row of g_prim_edges is wanted; an edge sample of an unwanted row is not traced (its
     * whole contribution is that row).  NULL = all rows.  (A caller that differentiates one mesh and not the camera wants the rows of that mesh's edges.) */
    const uint8_t *prim_edge_filter;
} psdr_grads;
/* offsets[3*n_bsdfs] (HOST): float offset of the texel block of BSDF b's bitmap k (0 reflectance / diffuse reflectance rgb,
 * 1 specular reflectance rgb, 2 roughness; RoughConductor: eta, k, alpha; NormalMap: the map; MicrofacetPerVertex: the per-vertex
 * diffuse / specular / roughness arrays) inside psdr_grads.g_tex, same row-major layout as the bitmap; -1 = constant.
 * *total = floats to allocate (0 = the scene has no bitmap parameter).  Either pointer may be NULL. */
int psdr_hip_scene_tex_layout(const psdr_hip_scene *scene, int64_t *offsets, int64_t *total);
int psdr_hip_render_d_bwd(const psdr_hip_scene *scene, const psdr_render_args *args, const float *d_rgb,
                          const psdr_grads *grads, void *stream);
/* the transpose of psdr_hip_render_d_fwd_batch (requires args->pix_ids; d_rgb is [n_pix*3]): the adjoint an edge sample on pixel p sees is the sum of d_rgb over the
 * rows k with pix_ids[k] == p; samples on pixels that are not listed are not traced */
int psdr_hip_render_d_bwd_batch(const psdr_hip_scene *scene, const psdr_render_args *args, const float *d_rgb,
                                const psdr_grads *grads, void *stream);
/* same kernels with traversal counters enabled (slower; counters is a HOST struct, call synchronises) */
int psdr_hip_render_c_counted(const psdr_hip_scene *scene, const psdr_render_args *args, float *out_rgb,
                              psdr_counters *counters, void *stream);
int psdr_hip_render_d_fwd_counted(const psdr_hip_scene *scene, const psdr_render_args *args, float *out_rgb,
                                  float *out_drgb, psdr_counters *counters, void *stream);
/* per-lane radiance of the interior term, out [n_lanes*3] (device); parity aid */
int psdr_hip_li_lanes(const psdr_hip_scene *scene, const psdr_render_args *args, int64_t lane_begin, int64_t lane_end,
                      float *out, void *stream);

/* PathTracer::preprocess_secondary_edges: reso = {rx, ry, rz, samples per cell} */
int psdr_hip_guiding_build(const psdr_hip_scene *scene, int32_t sensor_id, int32_t max_depth, const int32_t reso[4],
                           int32_t nrounds, int32_t seed, psdr_hip_guiding **out, void *stream);
int psdr_hip_guiding_mass(const psdr_hip_guiding *g, float *out_host, int32_t cap);   /* returns n_cells via cap check */
int psdr_hip_guiding_num_cells(const psdr_hip_guiding *g);
int psdr_hip_guiding_destroy(psdr_hip_guiding *g);

/* LAPLACIAN VERTEX PRECONDITIONER ("Large Steps in Inverse Rendering", Nicolet et al. 2021; the reference's users get it from the CUDA-only largesteps / cholespy packages).
 * M = I + lambda L, L the combinatorial Laplacian of a mesh: L_ii = number of distinct neighbours of vertex i, L_ij = -1 once per distinct undirected edge.  Only the CSR
 * pattern is given and kept (row_begin[n + 1], col[row_begin[n]], HOST arrays, copied): row i of M x is (1 + lambda deg_i) x_i - lambda sum_j x_j with
 * deg_i = row_begin[i + 1] - row_begin[i].  The create call validates the host arrays BEFORE any device call (n > 0, row_begin[0] == 0, row_begin monotonic, every col in
 * [0, n), no col equal to its row; lambda finite and >= 0) and returns non-zero for a bad list: no bad index reaches a kernel.  x, y, b are DEVICE [n, 3] row-major float32
 * (a contiguous torch [n, 3]); the three columns are independent systems solved at once.  Added under ABI 16 like the batch entry points: nothing existing changed. */
typedef struct psdr_hip_precond psdr_hip_precond;
typedef struct psdr_precond_info {
    int32_t iterations;              /* iterations enqueued (a multiple of the chunk between two looks at the residual, or max_iter) */
    int32_t converged;               /* 1: every column's recomputed residual |b - M x|_2 <= rtol |b|_2 */
    int32_t launches;                /* kernels launched by the call */
    float rel_residual[3];           /* |b - M x|_2 / |b|_2 per column, from r = b - M x recomputed from x (0 for a zero column of b) */
} psdr_precond_info;
int psdr_hip_precond_create(int32_t n, const int32_t *row_begin, const int32_t *col, float lambda, psdr_hip_precond **out, void *stream);
int psdr_hip_precond_destroy(psdr_hip_precond *precond);
/* y = M x (x and y different arrays); no synchronisation */
int psdr_hip_precond_apply(const psdr_hip_precond *precond, const float *x, float *y, void *stream);
/* M x = b by Jacobi-preconditioned conjugate gradients in float32 from x0 = 0, each column with its own scalars: plain launches on `stream` (two per iteration, every scalar
 * in device memory, dot products as per-workgroup partials added in a fixed order by the next launch: no atomics, no grid barrier, the same b gives the same bits).  After every
 * chunk of iterations r = b - M x is recomputed from x, its norms reach the host in one small copy (the call's only synchronisations) and the iteration goes on from that
 * residual; convergence is declared on it alone.  max_iter reached: converged = 0, x as it stands, return 0.  A column with |b| = 0, r.z = 0 or p.q <= 0 is frozen
 * (alpha = beta = 0) for the rest of the solve; a zero column of b gives exactly zero.  The handle holds the work arrays: one solve at a time per handle. */
int psdr_hip_precond_solve(psdr_hip_precond *precond, const float *b, float *x, float rtol, int32_t max_iter, psdr_precond_info *info, void *stream);

/* ADAPTIVE SAMPLING (csrc/hip/adaptive.hip; psdr_jit_amd/adaptive.py): a per-pixel weight map becomes a pixel list that spends an exact sample budget -
 * the list the batch entry points take, duplicates and all - and the rows of that list are folded back into a frame.  Device pointers throughout, plain launches on `stream`,
 * no synchronisation, no float atomics (the same input gives the same bits).  Every call checks its arguments BEFORE any device call and returns non-zero with
 * psdr_hip_last_error text for a NULL pointer or a value out of range.  Added under ABI 16 like the batch entry points: nothing existing changed.
 *
 * counts: w_i = weights[i] if finite and > 0, else 0; wmax = max w_i; q_i = (uint32) floor((double) w_i / (double) wmax * 2^bits), every q_i = 1 if wmax == 0;
 * C = the exclusive prefix sum of q in uint64 (n + 1 positions), S = C_n; B' = budget - n * min_count;
 *     counts[i] = min_count + floor(B' C_{i+1} / S) - floor(B' C_i / S),      offsets[i] = i * min_count + floor(B' C_i / S),  offsets[n] = budget
 * so the counts add up to budget exactly and each is within one of its share min_count + B' q_i / S.  bits = min(20, 62 - ceil_log2(n) - ceil_log2(max(budget, 1)))
 * (the value the bits call returns, -1 for n <= 0 or budget < 0) keeps B' S below 2^62; the call refuses n outside [1, 2^24], budget outside [n * min_count, 2^31 - 1],
 * min_count < 0 and bits < 8.  scratch: a device buffer of at least the scratch_bytes call's size, the call's own between its launches. */
int64_t psdr_hip_adaptive_scratch_bytes(void);
int psdr_hip_adaptive_bits(int32_t n, int64_t budget);
int psdr_hip_adaptive_counts(const float *weights, int32_t n, int64_t budget, int32_t min_count, int32_t *counts, int32_t *offsets, void *scratch, void *stream);
/* pix_ids[k] = the pixel p with offsets[p] <= k < offsets[p + 1], for k in [0, total): the list sorted by pixel.  total = offsets[n] (the budget: the host knows it);
 * total == 0 writes nothing and accepts pix_ids == NULL */
int psdr_hip_adaptive_expand(const int32_t *offsets, int32_t n, int64_t total, int32_t *pix_ids, void *stream);
/* The segment fold.  rows is [total, channels], row k belongs to pixel p(k) and averages rows_n samples; base is an earlier frame [n, channels] that averaged base_n samples
 * per pixel, or NULL with base_n = 0.  With c_p = offsets[p + 1] - offsets[p] and n_tot = base_n + rows_n c_p:
 *     square = 0:  out[p] = (base_n base[p] + rows_n sum_k rows[k]) / n_tot                      the combined mean
 *     square = 1:  out[p] = (base_n / n_tot)^2 base[p] + (rows_n / n_tot)^2 sum_k rows[k]        the same estimator's sum of squared sample contributions
 * and 0 where n_tot = 0.  One wave per pixel adds its segment in a fixed order in float32; the rest of the formula is evaluated in double and rounded once.
 * channels in [1, 4]; rows_n > 0; base_n >= 0. */
int psdr_hip_adaptive_merge(const int32_t *offsets, int32_t n, int64_t total, int32_t channels, const float *rows, float rows_n, const float *base, float base_n,
                            int32_t square, float *out, void *stream);
/* the transpose of the square = 0 fold: d_rows[k] = d_out[p(k)] rows_n / n_tot (a gather, one thread per row), d_base[p] = d_out[p] base_n / n_tot (d_base may be NULL) */
int psdr_hip_adaptive_merge_adj(const int32_t *offsets, int32_t n, int64_t total, int32_t channels, const float *d_out, float rows_n, float base_n, float *d_rows,
                                float *d_base, void *stream);

/* EDGE-AVOIDING A-TROUS DENOISER AND ITS TRANSPOSE (csrc/hip/denoise.hip; psdr_jit_amd/denoise.py).  Device pointers throughout, plain launches on
 * `stream` (one per level), no synchronisation, no atomics (the same input gives the same bits).  Every call checks its arguments BEFORE any device call and returns non-zero
 * with psdr_hip_last_error text for a NULL pointer, W or H < 1, W H > 2^24, L outside [1, 8], C outside [1, 4], G outside [0, 8], in == out.  Added under ABI 16 like the
 * adaptive entry points: nothing existing changed.
 *
 * The operator.  The frame is W x H, pixel p = y W + x (the order renderC returns).  The image x is [W H, C] float32, the guides g are [W H, G] float32 and PRE-SCALED: the
 * kernel knows nothing of what a channel means.  Level l = 0 .. L - 1 has stride s = 2^l and the taps (i, j) in {-2 .. 2}^2 with h = [1, 4, 6, 4, 1] / 16.
 *     the tap q = p + s (i, j) exists only if q lies inside the frame (taps outside are dropped, not clamped)
 *     d2 = sum_k (g_k(p) - g_k(q))^2,    w_l(p, q) = h(i) h(j) exp(-d2) if d2 is finite, otherwise 0;   the centre tap always has weight h(0)^2, whatever the guides hold
 *     N_l(p) = sum_q w_l(p, q) >= 9/64 (no guard is needed),    A_l x (p) = sum_q w_l(p, q) x(q) / N_l(p)
 * A_l is linear in x and row-stochastic; the guides carry no gradient.  The filter is D = A_{L-1} ... A_0.
 * The transpose.  w_l is symmetric in (p, q) (h and d2 are, and p and q are both in-frame), so A_l^T y (q) = sum_p w_l(q, p) (y(p) / N_l(p)): the same gather over the same
 * taps with the source pre-divided and no division at the end; D^T = A_0^T ... A_{L-1}^T.  No scatter.
 * In float32 as written: d2 by G subtractions, squares and additions in channel order (no fused multiply-add), expf, the 25 taps added row by row (j outer, i inner),
 * 1 / N_l by one IEEE division when the handle is made, and one multiplication by it per element (apply: of the sum; transpose: of the source).
 *
 * create copies the guides into planes, computes the L planes of 1 / N_l and allocates two work frames: it waits for `stream`, so the guides are the caller's again when it returns.
 * G == 0 takes guides == NULL and gives the plain B3-spline a-trous smoother.  The handle holds the work frames: one apply or apply_adj at a time per handle. */
typedef struct psdr_hip_denoise psdr_hip_denoise;
int psdr_hip_denoise_create(const float *guides, int32_t G, int32_t W, int32_t H, int32_t L, psdr_hip_denoise **out, void *stream);
/* out = D in; in and out are [W H, C] and may not alias */
int psdr_hip_denoise_apply(psdr_hip_denoise *denoise, const float *in, int32_t C, float *out, void *stream);
/* d_in = D^T d_out; the same shapes, the same rule */
int psdr_hip_denoise_apply_adj(psdr_hip_denoise *denoise, const float *d_out, int32_t C, float *d_in, void *stream);
int psdr_hip_denoise_destroy(psdr_hip_denoise *denoise);

/* VARIANCE-GUIDED A-TROUS DENOISER, ITS FROZEN OPERATOR AND THAT OPERATOR'S TRANSPOSE (csrc/hip/vdenoise.hip; psdr_jit_amd/vdenoise.py).  The denoiser
 * above stops at edges of the guides only; this one also stops where two pixels' luminances differ by more than their variances explain (Dammertz et al.'s colour weight,
 * normalised by variance as in SVGF, Schied et al. 2017), so that an illumination edge without a guide edge survives.  Device pointers throughout except `lum`, plain launches
 * on `stream` (apply: two per level, frozen and frozen_adj: one per level), no synchronisation, no atomics (the same input gives the same bits).  Every call checks its
 * arguments BEFORE any device call and returns non-zero with psdr_hip_last_error text for a NULL pointer, W or H < 1, W H > 2^24, L outside [1, 8], G outside [0, 8], C other
 * than 1 or 3, in == out, var == var_out, k negative or not finite, eps not positive or not finite, a luminance coefficient that is not finite, and a frozen, frozen_adj or
 * record call on a handle that holds no record.  Added under ABI 16 like the adaptive and denoise entry points: nothing existing changed.
 *
 * The operator.  Frame W x H, pixel p = y W + x.  Image x [W H, C] float32, C in {1, 3}; variance v [W H] float32, the variance of the pixel's LUMINANCE estimate; guides g
 * [W H, G] float32, pre-scaled as for psdr_hip_denoise; luminance coefficients a[C] on the host; k = 1 / sigma_l^2 >= 0; eps > 0.  The state is (x_l, v_l), x_0 = x, v_0 = v.
 * Level l = 0 .. L - 1 has stride s = 2^l and the taps (i, j) in {-2 .. 2}^2 with h = [1, 4, 6, 4, 1] / 16, exactly as above:
 *     lum_l(p) = a_0 x_l,0(p) + a_1 x_l,1(p) + a_2 x_l,2(p)          (this order, no contraction; C = 1: a_0 x_l,0(p))
 *     vt_l(p)  = 3 x 3 prefilter of v_l at UNIT stride: coefficients [1, 2, 1] x [1, 2, 1] / 16 over the taps inside the frame, divided by the sum of the coefficients that
 *                were inside
 *     the tap q = p + s (i, j) exists only inside the frame
 *     d2 = sum_k (g_k(p) - g_k(q))^2                                 (as above)
 *     z  = k (lum_l(p) - lum_l(q))^2 / (vt_l(p) + vt_l(q) + eps)
 *     w_l(p, q) = h(i) h(j) exp(-(d2 + z)) if 0 <= d2 + z < inf and vt_l(p) + vt_l(q) + eps is finite, otherwise 0
 *     the centre tap always has weight h(0)^2, whatever the inputs hold
 *     N_l(p) = sum_q w_l(p, q) >= 9/64
 *     x_{l+1}(p) = sum_q w_l(p, q) x_l(q) / N_l(p)
 *     v_{l+1}(p) = sum_q w_l(p, q)^2 v_l(q) / N_l(p)^2
 * A tap whose weight is 0 adds nothing to either sum, whatever x_l(q) and v_l(q) hold.  So a NaN or Inf in x or a guide at q cuts q off - no tap reaches it or leaves it - and
 * q's own centre tap hands its value through; a NaN or Inf in v at q makes vt_l non-finite on q's 3 x 3 unit-stride neighbourhood and cuts those (up to nine) pixels off
 * (the second condition on w_l is there for v = Inf, which would otherwise give z = 0 and let the infinite variance spread).
 * z is the squared difference of two estimates over the variance of that difference, in units of sigma_l^2.  w_l is symmetric in (p, q).  With k = 0 the image part is the
 * operator of psdr_hip_denoise, bit for bit.  v_{l+1} is the exact variance of x_{l+1}'s luminance for ONE level with independent pixels and the weights held fixed; over
 * several levels a level's inputs are correlated and it is SVGF's approximation, not a variance.
 * In float32 as written: lum by C multiplications and C - 1 additions; vt by nine multiply-and-adds row by row with the integer coefficients 1 2 1 / 2 4 2 / 1 2 1 and one
 * division by their sum; d2 as above; z = (k * (dl * dl)) / ((vt(p) + vt(q)) + eps) with dl = lum(p) - lum(q); expf(-(d2 + z)); the 25 taps added row by row; 1 / N_l by one
 * IEEE division, then one multiplication by it per channel, and two for v_{l+1}.
 *
 * The record and the frozen operator.  The weights depend on the image, so the map x -> x_L is not linear.  apply RECORDS what the weights were formed from: three planes per
 * level, lum_l, vt_l and 1 / N_l, beside k and eps.  With these held fixed, D_x = A_{L-1} ... A_0, A_l u (p) = (sum_q w_l(p, q) u(q)) (1 / N_l)(p), is linear; frozen applies
 * it to any image (C need not be the recording's) and frozen_adj applies D_x^T = A_0^T ... A_{L-1}^T, A_l^T y (q) = sum_p w_l(q, p) (y(p) (1 / N_l)(p)): the same gather with
 * the source pre-multiplied, no scatter.  Both form z and w from the record with apply's float32 expression sequence: frozen(x) after apply(x, v) returns apply's bits.
 * D_x^T g is the EXACT TRANSPOSE OF THE FROZEN OPERATOR, which is what a loss that treats the weights as constants (stop-gradient) differentiates; it is NOT the derivative of
 * the nonlinear map x -> x_L, and v receives no gradient.
 *
 * create copies the guides into planes and allocates the record and the work frames: (G + 3 L + 8) W H floats.  The record alone is 12 L W H bytes: 252 MB at 2048 x 2048
 * and L = 5.  G == 0 takes guides == NULL.  The handle holds the work frames: one call at a time per handle.  A new apply replaces the record. */
typedef struct psdr_hip_vdenoise psdr_hip_vdenoise;
int psdr_hip_vdenoise_create(const float *guides, int32_t G, int32_t W, int32_t H, int32_t L, psdr_hip_vdenoise **out, void *stream);
/* out = x_L, var_out = v_L (may be NULL); `lum`: C floats on the HOST; in / out and var / var_out may not alias; records */
int psdr_hip_vdenoise_apply(psdr_hip_vdenoise *vdenoise, const float *in, int32_t C, const float *var, const float *lum, float k, float eps, float *out, float *var_out,
                            void *stream);
/* out = D_x in with the last apply's record */
int psdr_hip_vdenoise_frozen(psdr_hip_vdenoise *vdenoise, const float *in, int32_t C, float *out, void *stream);
/* d_in = D_x^T d_out */
int psdr_hip_vdenoise_frozen_adj(psdr_hip_vdenoise *vdenoise, const float *d_out, int32_t C, float *d_in, void *stream);
/* out [L][3][W H] = the record: lum_l, vt_l, 1 / N_l for l = 0 .. L - 1 (a device-to-device copy; what the tests feed the restatement) */
int psdr_hip_vdenoise_record(psdr_hip_vdenoise *vdenoise, float *out, void *stream);
int psdr_hip_vdenoise_destroy(psdr_hip_vdenoise *vdenoise);

/* MESH SUBDIVISION AS A LINEAR OPERATOR AND ITS TRANSPOSE (csrc/hip/subdiv.hip; psdr_jit_amd/subdiv.py).  One level of Loop or midpoint subdivision
 * takes the n_in coarse vertices to n_out = n_in + (number of edges) fine ones; on any per-vertex array (positions, uv pairs, scalar or RGB values) that is the product with
 * a sparse matrix S (n_out x n_in, rows that sum to 1), and the gradient of a loss on the fine array reaches the coarse one through S^T.  One level is one handle; levels
 * are chained by the caller.  Device pointers in apply / apply_adj, one plain launch on `stream` each, no synchronisation, no copy to the host, no atomics (the same input
 * gives the same bits).  Added under ABI 16 like the denoise entry points: nothing existing changed.
 *
 * The matrices.  create takes S and S^T, BOTH as CSR in HOST arrays (copied; the caller's again when the call returns):
 *     row_begin[n_out + 1], col[nnz] in [0, n_in),  weight[nnz]          row r of S   is the entries k in [row_begin[r], row_begin[r + 1])
 *     t_row_begin[n_in + 1], t_col[nnz] in [0, n_out), t_weight[nnz]     row j of S^T likewise: the inverted index of S, every list in a fixed (ascending) order
 * The topology, the float32 weights (Warren's Loop weights, crease and corner rules, or the midpoint rule) and the transpose are the host's business
 * (psdr_jit_amd/subdiv.py: subdivision_level); the device never forms a transpose and never scatters.  The price is a second copy of the pattern: 16 nnz bytes of
 * indices and weights in all, beside the two row_begin arrays.
 * create validates the host arrays BEFORE any device call and returns non-zero with psdr_hip_last_error text unless: out and both row_begin arrays are not NULL; n_in and
 * n_out are positive and 4 n_out, 4 n_in < 2^31; both row_begin arrays start at 0 and are monotonic; both end at the same nnz (an int32, so < 2^31); col, weight, t_col,
 * t_weight are not NULL when nnz > 0; every col is in [0, n_in) and every t_col in [0, n_out); every weight is finite.  No bad index reaches a kernel.
 * create does NOT check that the second CSR is the transpose of the first: two unrelated matrices of the same nnz are accepted, and apply_adj is then simply the product
 * with the second one.  The Python layer builds both from one list of entries and is what guarantees it.
 *
 * The product.  x, y, d_y, d_x are row-major [rows, C] float32, C in [1, 4]; input and output may not alias.  Both directions are the same kernel over a different CSR: one
 * lane owns one output row r and computes, per channel c and in float32,
 *     acc = 0;   for k = row_begin[r] .. row_begin[r + 1] - 1 in this order:  acc = fmaf(weight[k], x[col[k] C + c], acc);   y[r C + c] = acc
 * (an empty row gives 0).  Rows beyond one pass of the 1024 x 256 grid are taken by a grid-stride loop.  A lane walks its row alone: a launch takes as long as its longest
 * row, which is accepted for meshes (valence is bounded almost everywhere; the transpose row of a vertex of valence d has about 3 d + 1 entries).
 * Other C, a NULL pointer, a NULL handle or x == y return non-zero before anything is launched. */
typedef struct psdr_hip_subdiv psdr_hip_subdiv;
int psdr_hip_subdiv_create(int32_t n_in, int32_t n_out,
        const int32_t *row_begin, const int32_t *col, const float *weight,         /* S   : n_out rows, columns < n_in  */
        const int32_t *t_row_begin, const int32_t *t_col, const float *t_weight,   /* S^T : n_in rows,  columns < n_out */
        psdr_hip_subdiv **out, void *stream);
/* y[n_out, C] = S x, x [n_in, C] */
int psdr_hip_subdiv_apply(const psdr_hip_subdiv *s, const float *x, int32_t C, float *y, void *stream);
/* d_x[n_in, C] = S^T d_y, d_y [n_out, C] */
int psdr_hip_subdiv_apply_adj(const psdr_hip_subdiv *s, const float *d_y, int32_t C, float *d_x, void *stream);
int psdr_hip_subdiv_destroy(psdr_hip_subdiv *s);

/* MULTI-SCALE IMAGE LOSS, VALUE AND GRADIENT IN ONE FUSED PASS (csrc/hip/msloss.hip; psdr_jit_amd/msloss.py).  A sum of per-level losses over an
 * image pyramid of the weighted residual: the coarse levels carry a silhouette's error across the frame where a per-pixel loss has no signal.  Device pointers in eval and
 * level, plain launches on `stream` (three with a gradient, two without), no host synchronisation, no copy to the host, no atomics: the same input gives the same bits.
 * Added under ABI 16 like the subdiv entry points: nothing existing changed.
 *
 * The definition.  Frame W x H, pixel (x, y) at row y W + x.  img, target: float32 [W H, C], C in [1, 4].  weight: absent (weight_channels = 0: 1 everywhere), [W H]
 * (weight_channels = 1) or [W H, C] (weight_channels = C); it gets no gradient.
 *     level 0:      d_0 = weight (img - target)
 *     level l + 1:  W_{l+1} x H_{l+1} = ceil(W_l / 2) x ceil(H_l / 2);  d_{l+1}(i, j) = the mean of those of d_l(2i .. 2i + 1, 2j .. 2j + 1) that exist: 4 pixels, 2 at an odd
 *                   edge, 1 at an odd corner (the divisors are powers of two; in float32 ((a + b) + (c + d)) / count with missing pixels as 0)
 *     levels:       L of them, l = 0 .. L - 1; the full depth ends at the 1 x 1 level, L_full = 1 + ceil(log2(max(W, H)))
 *     level_loss_l = sum rho(d_l) / (C W_l H_l),   rho(x) = |x| with rho'(0) = 0 (PSDR_MSLOSS_L1) or x^2 (PSDR_MSLOSS_L2)
 *     loss         = sum_l lambda_l level_loss_l,  lambda = level_weights (a HOST array of L floats, read during the call; NULL: all 1)
 *     dloss / dimg = weight G_0,   G_l = (lambda_l / (C W_l H_l)) rho'(d_l) + G_{l+1}(parent) / (the number of the parent's children),   G_L = 0
 *     dloss / dtarget is its negative (the caller negates).
 * create(W, H, levels, C) owns the work frames: the residual pyramid (every d_l), per-tile partial sums and the coarse part of the gradient.  It is refused with
 * psdr_hip_last_error text BEFORE any device call unless: out is not NULL; 1 <= W, H <= 16384 and W H <= 2^24; C in [1, 4]; levels in [1, L_full].
 * eval writes out[0] = loss and out[1 .. L] = level_loss_l (device, L + 1 floats) and, if grad is not NULL, dloss / dimg [W H, C].  It is refused before any launch for a
 * NULL handle, img, target or out, an unknown norm, a weight_channels not in {0, 1, C}, a NULL weight with weight_channels != 0, a level weight that is not finite, and a
 * grad that is one of the other arrays.  grad = NULL gives the same loss bits.
 * level(l) copies d_l of the handle's last eval, [W_l H_l, C], to `out` (device) on `stream`; refused for a NULL argument, l outside [0, L) and a handle never evaluated.
 * The sums: a level's sum of rho is added per 32 x 32 tile (a lane's own elements, the wave, the workgroup's four waves, always in the same order), then over the tiles by
 * one workgroup in a fixed order; levels above 5 are reduced by that one workgroup. */
#define PSDR_MSLOSS_L1 0
#define PSDR_MSLOSS_L2 1
typedef struct psdr_hip_msloss psdr_hip_msloss;
int psdr_hip_msloss_create(int32_t W, int32_t H, int32_t levels, int32_t C, psdr_hip_msloss **out, void *stream);
int psdr_hip_msloss_eval(psdr_hip_msloss *m, const float *img, const float *target, const float *weight, int32_t weight_channels, int32_t norm,
                         const float *level_weights, float *out, float *grad, void *stream);
int psdr_hip_msloss_level(psdr_hip_msloss *m, int32_t level, float *out, void *stream);
int psdr_hip_msloss_destroy(psdr_hip_msloss *m);

/* THE SSIM LOSS, 1 - MEAN STRUCTURAL SIMILARITY, VALUE AND IMAGE GRADIENT IN ONE FUSED PASS (csrc/hip/ssim.hip; psdr_jit_amd/ssim.py).  A norm of pixel
 * differences cannot tell structure from brightness; SSIM compares local means, variances and the covariance under a Gaussian window.  Device pointers in eval and map, plain
 * launches on `stream` (three with a gradient, two without), no host synchronisation, no copy to the host, no atomics: the same input gives the same bits.  Added under ABI 16
 * like the msloss entry points: nothing existing changed.
 *
 * The definition.  Frame W x H, pixel (x, y) at row y W + x.  img = x, target = y: float32 [W H, C], C in [1, 4].  mask = m: NULL (1 everywhere) or [W H], finite and
 * non-negative.  Neither target nor mask gets a gradient.
 *     window:   K odd in [3, 11], R = K / 2, taps g_0 .. g_{K-1}: a HOST array read by create.  The float32 taps ARE the definition (psdr.gaussian_window(K, sigma):
 *               exp(-(k - R)^2 / (2 sigma^2)) normalised in double, rounded once); they travel to the kernels as arguments.
 *     G v     = the vertical pass of the horizontal pass of v, each pass sum_k g_k v(. + k - R), in any summation order; pixels outside the frame count as 0 and the
 *               window is not renormalised (F.conv2d(padding = R))
 *     mu_x = G x, mu_y = G y, E_xx = G(x x), E_yy = G(y y), E_xy = G(x y);   s_xx = E_xx - mu_x mu_x, s_yy = E_yy - mu_y mu_y, s_xy = E_xy - mu_x mu_y
 *     a1 = 2 (mu_x mu_y) + c1,  a2 = 2 s_xy + c2,  b1 = (mu_x mu_x + mu_y mu_y) + c1,  b2 = (s_xx + s_yy) + c2;   c1 = (k1 range)^2, c2 = (k2 range)^2 as float32
 *     S = (a1 a2) / (b1 b2): one product each, one division; img == target gives S == 1 exactly
 *     m_eff   = m (PSDR_SSIM_SAME), or m times the indicator of R <= x < W - R and R <= y < H - R (PSDR_SSIM_VALID: the mean over windows that lie wholly inside)
 *     N = C sum_p m_eff(p);  mean = (sum_{p,c} m_eff(p) S(p, c)) / N;  out[0] = loss = 1 - mean, out[1] = mean;  N == 0: out = (0, 0) and the gradient is 0
 *     P = m_eff [2 mu_y (a2 - a1) - 2 mu_x S (b2 - b1)] / (b1 b2),   Q = -m_eff S / b2,   T = m_eff 2 a1 / (b1 b2)
 *     dloss / dimg = -(G P + 2 x G Q + y G T) / N with the same zero-padded G: the window is symmetric, so the gradient is a gather
 * create(W, H, C, window, taps, c1, c2, padding) owns S, P, Q, T ([W H, C] each), the tiles' partial sums and the scale -1 / N.  It is refused with psdr_hip_last_error
 * text BEFORE any device call unless: out and taps are not NULL; 1 <= W, H <= 16384 and W H <= 2^24; C in [1, 4]; window odd in [3, 11]; every tap finite and their sum 1
 * within 1e-5; c1, c2 finite and positive; padding one of the two; W, H >= window under PSDR_SSIM_VALID.
 * eval writes out[0 .. 1] (device) and, if grad is not NULL, dloss / dimg [W H, C].  It is refused before any launch for a NULL handle, img, target or out and a grad that
 * is img or target.  grad = NULL gives the same out bits.
 * map copies the unmasked S of the handle's last eval, [W H, C], to `out` (device) on `stream`; refused for a NULL argument and a handle never evaluated.
 * The sums: m_eff S and m_eff are added per 32 x 16 tile (a lane's own elements, the wave, the workgroup's four waves, always in the same order), then over the tiles by
 * one workgroup in a fixed order. */
#define PSDR_SSIM_SAME 0
#define PSDR_SSIM_VALID 1
typedef struct psdr_hip_ssim psdr_hip_ssim;
int psdr_hip_ssim_create(int32_t W, int32_t H, int32_t C, int32_t window, const float *taps, float c1, float c2, int32_t padding, psdr_hip_ssim **out, void *stream);
int psdr_hip_ssim_eval(psdr_hip_ssim *s, const float *img, const float *target, const float *mask, float *out, float *grad, void *stream);
int psdr_hip_ssim_map(psdr_hip_ssim *s, float *out, void *stream);
int psdr_hip_ssim_destroy(psdr_hip_ssim *s);

/* THE MESH REGULARISERS - UNIFORM LAPLACIAN, NORMAL CONSISTENCY, EDGE LENGTH - VALUE AND VERTEX GRADIENT IN ONE FUSED PASS (csrc/hip/meshreg.hip; psdr_jit_amd/meshreg.py;
 * DESIGN.md section 7j).  The part of a shape-optimisation loss that depends on the mesh, not on the image: it holds the vertices in place where the image is silent.  Device
 * pointers in eval, plain launches on `stream` (three with a gradient, two without), no host synchronisation, no copy to the host, no atomics: the same input gives the same
 * bits.  Added under ABI 16 like the ssim entry points: nothing existing changed.
 *
 * The definition.  V = v: float32 [n, 3].  F: [f, 3] vertex ids, every face with three distinct ids in [0, n); no welding.  The topology is built on the host once per mesh
 * (psdr_jit_amd/meshreg.py: mesh_topology) and travels to create:
 *     E        the distinct undirected edges (a < b) of F in ascending (a, b) order, e of them.  N(i) = the other ends of the edges at i, deg_i = |N(i)| (the CSR of
 *              psdr_jit_amd/precond.py: laplacian_csr)
 *     hinges   the edges with exactly two incident faces, in edge order, h of them, each a row (a, b, c, d): c the vertex opposite the edge in its first incident face (the
 *              lower face index), d the one in the second.  A boundary edge (one face) and a non-manifold edge (three or more) form no hinge; two copies of one face make
 *              a hinge with c == d.
 *     n1 = (b - a) x (c - a),  n2 = (d - a) x (b - a),  u = n / |n|: independent of the faces' winding
 * The terms:
 *     laplacian = (1 / n_L) sum_i |delta_i|^2,   delta_i = v_i - (1 / deg_i) sum_{j in N(i)} v_j;  delta_i = 0 for a vertex no face uses, n_L = the number of vertices with
 *                 deg_i > 0, the value 0 when n_L = 0.   d / dv_k = (2 / n_L) (delta_k - sum_{j in N(k)} delta_j / deg_j): a gather over the same CSR
 *     normal    = (1 / h) sum_hinges 1/2 |u1 - u2|^2:  1 - cos of the dihedral deviation without the cancellation of 1 - u1 . u2;  0 on a flat hinge, 2 on one folded back
 *                 onto itself, smooth at both.  A hinge with |n1|^2 < 2^-100 or |n2|^2 < 2^-100 adds 0 to the value and no gradient; it still counts in h.
 *                 With w = u1 - u2:  d / dn1 = (w - (u1 . w) u1) / |n1|,  d / dn2 = -(w - (u2 . w) u2) / |n2|  (the projections applied to w, which is small where the hinge
 *                 is flat);  d / db = (c - a) x g1 + g2 x (d - a),  d / dc = g1 x (b - a),  d / dd = (b - a) x g2,  d / da = -(their sum)
 *     edge      = (1 / e) sum_edges (|v_a - v_b| - L0)^2,  L0 = target_length >= 0.  At L0 == 0 the summand is |v_a - v_b|^2 and nothing is divided; at L0 > 0 an edge with
 *                 |v_a - v_b|^2 < 2^-100 adds L0^2 and no gradient.
 *     loss      = w_lap laplacian + w_nor normal + w_edge edge, weights[3] = (w_lap, w_nor, w_edge).  A term whose weight is 0 is not evaluated: its reported value is 0, it
 *                 does no work and the gradient is the other terms' bit for bit; a term with e = 0 or h = 0 is 0.  The terms are added in this order, those that are off left out.
 * out[4] (device) = (loss, laplacian, normal, edge); grad (device, [n, 3], or NULL for a value-only call, which gives the same out bits) = d loss / d V.
 *
 * create(n, e, h, edges [e, 2], hinges [h, 4], row_begin [n + 1], col, ev_begin [n + 1], ev_elem, ev_role [2 e], hv_begin [n + 1], hv_elem, hv_role [4 h]): HOST arrays, read by
 * create.  ev_* and hv_* are the inverted indices: per vertex the (element, role) pairs that name it, in ascending (element, role) order - role 0, 1 = a, b of an edge, role
 * 0 .. 3 = a, b, c, d of a hinge - so that the gradient is a gather in a fixed order.  It is refused with psdr_hip_last_error text BEFORE any device call unless: out is not
 * NULL; 1 <= n <= 2^26, 0 <= e, h <= 2^26; no array that has entries is NULL; every edge has 0 <= a < b < n; every hinge's ids lie in [0, n) with a < b and c, d off the
 * edge; row_begin, ev_begin, hv_begin start at 0 and never decrease; every col lies in [0, n) and is not its row; ev_begin ends at 2 e and hv_begin at 4 h; every element
 * lies in [0, e) or [0, h) and every role in [0, 2) or [0, 4); the vertex an entry names is the one that lists it; the entries of a vertex ascend.
 * The handle owns delta and delta / deg ([n] float4 each), one float4 per edge, four per hinge and one partial sum per 256 elements of each kind.
 * eval is refused before any launch for a NULL handle, v, weights or out, a grad that is v, and a weight or target_length that is negative or not finite.
 * The sums: a workgroup of 256 elements of one kind adds its summands in a fixed order (the wave, then its four waves), one workgroup then adds the partial sums of each
 * kind in a fixed order; a vertex adds its contributions in the stored order and scales each term's sum once (2 w_lap / n_L, w_nor / h, w_edge / e, rounded from double). */
typedef struct psdr_hip_meshreg psdr_hip_meshreg;
int psdr_hip_meshreg_create(int32_t n, int32_t e, int32_t h, const int32_t *edges, const int32_t *hinges, const int32_t *row_begin, const int32_t *col,
                            const int32_t *ev_begin, const int32_t *ev_elem, const int32_t *ev_role, const int32_t *hv_begin, const int32_t *hv_elem, const int32_t *hv_role,
                            psdr_hip_meshreg **out, void *stream);
int psdr_hip_meshreg_eval(psdr_hip_meshreg *m, const float *v, const float *weights, float target_length, float *out, float *grad, void *stream);
int psdr_hip_meshreg_destroy(psdr_hip_meshreg *m);

/* THE CHAMFER DISTANCE BETWEEN TWO POINT SETS - EXACT NEAREST NEIGHBOURS BY A BRUTE-FORCE SCAN, VALUE AND BOTH GRADIENTS (csrc/hip/chamfer.hip; psdr_jit_amd/chamfer.py; DESIGN.md
 * section 7k).  The part of a shape-optimisation loop that measures the shape itself: how far a mesh's surface samples are from a scan, a point cloud or another mesh's samples.
 * Stateless entry points: device pointers, work arrays from the caller, plain launches on `stream`, no host synchronisation, no copy to the host, no float atomics: the same
 * input gives the same bits.  Added under ABI 16 like the meshreg entry points: nothing existing changed.
 *
 * The definition.  x: float32 [n, 3], y: float32 [m, 3], 1 <= n, m <= 2^26, all finite.
 *     distance  d2(i, j) = (dx dx + dy dy) + dz dz with dx = x_i0 - y_j0, dy = x_i1 - y_j1, dz = x_i2 - y_j2: every operation one float32 rounding, nothing fused, in this
 *               order.  The difference form on purpose: |x|^2 + |y|^2 - 2 x.y cancels exactly where a neighbour is near; this form does not, and a float32 restatement
 *               reproduces it bit for bit.  d2 >= +0.
 *     nearest   a(i) = the lowest j that minimises d2(i, j), dist2_xy[i] = d2(i, a(i));  b(j) = the lowest i that minimises d2(i, j), dist2_yx[j] = d2(b(j), j).  The
 *               lexicographic minimum over (d2, j) is associative and commutative: the result does not depend on how the scan is split or merged.  With non-finite inputs
 *               the values are unspecified, but every index lies in range.
 *     loss      = w_xy (1 / n) sum_i rho(dist2_xy[i]) + w_yx (1 / m) sum_j rho(dist2_yx[j]), weights[2] = (w_xy, w_yx);  rho(s) = s (squared != 0) or sqrt(s) (squared == 0),
 *               whose derivative at s = 0 is defined as 0.  A term whose weight is 0 is not evaluated: its reported value is 0 and the gradients are the other term's bit for
 *               bit.  The terms are added in this order.
 *     gradient  the indices are constants.  With k(s) = 2 w / count (squared) or (w / count) / sqrt(s), 0 at s = 0 (not squared), w / count and 2 w / count rounded from double:
 *               d loss / d x_i = k_xy(dist2_xy[i]) (x_i - y_a(i))  +  sum over {j : b(j) = i}, in ascending j, of k_yx(dist2_yx[j]) (x_i - y_j)
 *               and y_j receives the mirror image.  Each product is k times the rounded difference; the second sum starts at 0 and is added to the first contribution once.
 *
 * psdr_hip_chamfer_plan(n, m) -> (tile, queries_per_lane, slices, slice_len): how psdr_hip_chamfer_nearest splits its scan, a pure function, callable without a GPU.  A
 * workgroup of 256 lanes holds 256 queries_per_lane queries; slice s holds the candidates [s slice_len, min(m, (s + 1) slice_len)), slice_len a multiple of tile, no slice
 * empty; the grid is ceil(n / (256 queries_per_lane)) x slices.  queries_per_lane = 4 for n > 1024, else 1; slices = the fewest that bring the grid to 2048 workgroups, at
 * most one per tile.  The result of the scan does not depend on the plan.
 * psdr_hip_chamfer_nearest(x, n, y, m, keys, index, dist2): one direction; index int32 [n] = a, dist2 float32 [n]; keys: uint64 [n] work array of the caller (the per-query
 * minimum of (float bits of d2) << 32 | j, merged over the slices by an integer atomic minimum).  For b and dist2_yx call it with the sets swapped.
 * psdr_hip_chamfer_eval(x, n, y, m, index_xy, dist2_xy [n], index_yx, dist2_yx [m], x_begin [n + 1], x_list [m], y_begin [m + 1], y_list [n], weights, squared, partial, out,
 * grad_x, grad_y): out[3] (device) = (loss, mean_i rho(dist2_xy), mean_j rho(dist2_yx)); grad_x [n, 3], grad_y [m, 3] (device; both NULL for a value-only call, which gives the
 * same out bits).  x_begin / x_list: the inverted index of index_yx - x_list holds the j in ascending (index_yx[j], j) order (a stable sort of index_yx), x_begin[i] the
 * position of point i's first entry, x_begin[n] = m; y_begin / y_list the same for index_xy.  They are the caller's duty; the kernel clamps what it reads from them into
 * range.  partial: double work array of ceil(n / 256) + ceil(m / 256) entries (the sums of rho are
 * added in double and each mean is rounded to float32 once).  The arrays of a direction whose weight is 0, and the inverted indices of a value-only call, are
 * not read and may be NULL.  One launch per point set and one that adds the per-workgroup sums in a fixed order.
 * All three are refused with psdr_hip_last_error text before any device call for n or m outside [1, 2^26], a NULL array that would be read or written, a weight that is
 * negative or not finite, one gradient without the other, and a gradient that aliases an input or the other gradient. */
int psdr_hip_chamfer_plan(int32_t n, int32_t m, int32_t *tile, int32_t *queries_per_lane, int32_t *slices, int32_t *slice_len);
int psdr_hip_chamfer_nearest(const float *x, int32_t n, const float *y, int32_t m, uint64_t *keys, int32_t *index, float *dist2, void *stream);
int psdr_hip_chamfer_eval(const float *x, int32_t n, const float *y, int32_t m, const int32_t *index_xy, const float *dist2_xy, const int32_t *index_yx, const float *dist2_yx,
                          const int32_t *x_begin, const int32_t *x_list, const int32_t *y_begin, const int32_t *y_list, const float *weights, int32_t squared,
                          double *partial, float *out, float *grad_x, float *grad_y, void *stream);

/* THE SAME NEAREST NEIGHBOURS THROUGH A UNIFORM GRID OVER THE CANDIDATES (csrc/hip/nn_grid.h, entry points in csrc/hip/chamfer.hip; psdr_jit_amd/pointgrid.py; DESIGN.md
 * section 7q; numpy restatement: tests/pointgrid_ref.py).  Offered beside the scan, which it never replaces.  Stateless like the chamfer entry points above: every array is
 * the caller's, plain launches (and one clear) on `stream`, no host synchronisation, no copy to the host, no float atomics.  Added under ABI 16: nothing existing changed.
 *
 * THE CONTRACT FIXES THE RESULTS, NOT THE SCHEDULE: for finite inputs, index and dist2 of psdr_hip_chamfer_grid_nearest equal psdr_hip_chamfer_nearest's bit for bit - the
 * lowest j that minimises the float32 d2 of the chamfer section, and that d2.  With non-finite inputs the values are unspecified and every index lies in range.
 *     the grid     res cells per axis over the bounding box [lo, hi] of y, res = the largest r in [1, 256] with 2 r^3 <= m: a function of m alone, so that nothing is read
 *                  back to size an array.  Per axis, on the device, once: inv = fl(res / fl(hi - lo)), width = fl(fl(hi - lo) / res); the axis has dim = res cells, or
 *                  dim = 1 when its extent is zero or inv is not a finite positive number.
 *     the cell     c(v) = clamp((int) floor(fl(fl(v - lo) inv)), 0, dim - 1), the clamp done in float (a NaN goes to 0).  Every step is monotone non-decreasing in v,
 *                  so c is.  A query outside the box starts from its clamped cell.  Cell (c0, c1, c2) has the number (c0 res + c1) res + c2.
 *     the build    the box by integer atomic minimum / maximum on order-preserving keys of the floats; every candidate's cell and a histogram by integer atomicAdd; an
 *                  exclusive scan over the cells into cell_begin [res^3 + 1]; a scatter of (x, y, z, index) into cell order.  The order inside a cell is not deterministic
 *                  and nothing depends on it: the lexicographic minimum over (d2, j) does not.
 *     the planes   plane(a, upper, k), 1 <= k < dim: a float b with c(b) < k - then every candidate of a cell >= k along axis a has a coordinate > b, c being monotone.  It is
 *                  searched from fl(lo + fl(k width)) downwards by at most 8 steps, the first fl(2^-22 max(|lo|, |hi|)) long and each twice the one before, and is the
 *                  first b for which c(b) < k was evaluated; when none of them has it, the plane is -infinity: no certificate.
 *                  plane(a, lower, k), 0 <= k < dim - 1: the mirror image, a float b with c(b) > k, from fl(lo + fl((k + 1) width)) upwards, else +infinity.
 *     the walk     a query visits the cells at Chebyshev distance s = 0, 1, ... from its own.  After shell s the unvisited cells lie, along some axis a, at >= c_a + s + 1
 *                  or at <= c_a - s - 1.  A side beyond the grid holds no candidate.  For a side inside it, g = fl(plane - x_a) (upper) or fl(x_a - plane) (lower): when
 *                  g >= 0, every candidate y of that side has |fl(x_a - y_a)| >= g (rounding is monotone), hence fl((x_a - y_a)^2) >= fl(g g), and d2, a rounded sum of
 *                  non-negative terms, is not below it.  The query stops when every such side has g >= 0 and fl(g g) > best - strictly: on equality a lower index may
 *                  wait farther out.  A NaN passes neither comparison, so it never certifies.  No epsilon anywhere.
 *     the fallback a query not certified after max_shells = res / 4 shells, within [4, 16] (far outside the box, in the hollow of a surface cloud, between two clusters) goes onto a compacted
 *                  list whose length stays on the device, and a fixed grid of workgroups (fallback_groups x fallback_slices) strides over that length with the scan's
 *                  inner loop over ALL m candidates in their original order, merging the slices by the integer minimum of the scan's keys.
 * EVERY LOOP of every kernel has an iteration bound that does not depend on the floats in the data: strides over integer counts, shells <= max_shells, the cells of a
 * shell, cell ranges clamped into [0, m], at most 8 steps of a plane search.  That is why non-finite input can neither fault nor hang.
 *
 * psdr_hip_chamfer_grid_plan(n, m) -> res, max_shells and the lengths of every array, a pure function, callable without a GPU (psdr_jit_amd/pointgrid.py: grid_plan states
 * it in Python).  Lengths in 32-bit words.  The grid blob: [0, 16) the header - lo[3], inv[3], width[3] as float32, dim[3] as int32, 4 unused; [planes_at, + 6 res) the
 * planes, plane (a, side, k) at planes_at + (2 a + side) res + k, side 0 = upper; [begin_at, + cells) cell_begin, cells = res^3 + 1; [points_at, + 4 m) the candidates in
 * cell order, (x, y, z, the bits of the original index); begin_at and points_at are multiples of 4, and the blob must be 16-byte aligned; grid_words = points_at + 4 m.
 * The build's work array: work_words = 8 + 2 m + ceil(cells / 2048).  The search's arrays: keys uint64 [n], list int32 [n], stats uint64 [2].  The fallback's fixed grid:
 * fallback_groups x fallback_slices workgroups, slice s holding the candidates [s fallback_slice_len, min(m, (s + 1) fallback_slice_len)).  lanes_per_query: the lanes
 * that share one query's walk, 8 for n <= 65 536 and 1 beyond; the results and the statistics do not depend on it.
 * psdr_hip_chamfer_grid_build(y, m, grid, grid_words, work, work_words): fills the grid blob of the candidates y [m, 3] in eight launches; work is free again once they ran.
 * psdr_hip_chamfer_grid_nearest(x, n, y, m, grid, grid_words, keys, list, index, dist2, stats): index int32 [n], dist2 float32 [n] of the queries x [n, 3] in the grid of
 * y (THE grid built from this y: the caller's duty; the resolution is taken from m, and whatever is read from the blob is clamped into range, so that a foreign blob gives
 * wrong numbers, not a fault).  stats[0] = the queries the fallback finished, stats[1] = the (query, candidate) pairs tested - by the walk every candidate of every visited
 * cell, by the fallback m per listed query.  A clear of stats and three launches: the walk (lanes_per_query lanes per query), the fallback, the unpacking of the keys.
 * All three are refused with psdr_hip_last_error text before any device call for n or m outside [1, 2^26], a NULL array, and grid_words or work_words below the plan's. */
int psdr_hip_chamfer_grid_plan(int32_t n, int32_t m, int32_t *res, int32_t *max_shells, int64_t *cells, int64_t *planes_at, int64_t *begin_at, int64_t *points_at,
                               int64_t *grid_words, int64_t *work_words, int32_t *fallback_groups, int32_t *fallback_slices, int32_t *fallback_slice_len, int32_t *lanes_per_query);
int psdr_hip_chamfer_grid_build(const float *y, int32_t m, uint32_t *grid, int64_t grid_words, int32_t *work, int64_t work_words, void *stream);
int psdr_hip_chamfer_grid_nearest(const float *x, int32_t n, const float *y, int32_t m, const uint32_t *grid, int64_t grid_words, uint64_t *keys, int32_t *list,
                                  int32_t *index, float *dist2, uint64_t *stats, void *stream);

/* THE POINT-TO-MESH DISTANCE - FOR EVERY POINT THE NEAREST FACE, FOR EVERY FACE THE NEAREST POINT, VALUE AND BOTH GRADIENTS (csrc/hip/pointmesh.hip; psdr_jit_amd/pointmesh.py;
 * DESIGN.md section 7l).  What a user fitting a mesh to a scan needs: the distance from the scan's points to the closed triangles themselves, not to a frozen sample of them
 * (pytorch3d's point_mesh_face_distance).  Stateless entry points like the chamfer ones: device pointers, work arrays from the caller, plain launches on `stream`, no host
 * synchronisation, no float atomics: the same input gives the same bits.  Added under ABI 16: nothing existing changed.
 *
 * The definition.  p: float32 [N, 3] points; v: float32 [n, 3] vertices; faces: int32 [F, 3], ids in [0, n), no id repeated in a face; 1 <= N, F, n <= 2^26, all values finite.
 *   The pair function cp(p; a, b, c): the closest point of the closed triangle (a, b, c) to p as barycentrics (1 - s - t, s, t), by the region cascade of Ericson, Real-Time
 *   Collision Detection, section 5.1.5.  With ab = b - a, ac = c - a, ap = p - a, bp = p - b, cp = p - c (componentwise) and x.y = (x0 y0 + x1 y1) + x2 y2:
 *       d1 = ab.ap, d2 = ac.ap, d3 = ab.bp, d4 = ac.bp, d5 = ab.cp, d6 = ac.cp,  vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4
 *   the first test that holds decides:
 *       1. d1 <= 0 && d2 <= 0                              vertex a   s = 0, t = 0
 *       2. d3 >= 0 && d4 <= d3                             vertex b   s = 1, t = 0
 *       3. vc <= 0 && d1 >= 0 && d3 <= 0                   edge ab    s = d1 / (d1 - d3), t = 0
 *       4. d6 >= 0 && d5 <= d6                             vertex c   s = 0, t = 1
 *       5. vb <= 0 && d2 >= 0 && d6 <= 0                   edge ac    s = 0, t = d2 / (d2 - d6)
 *       6. va <= 0 && d4 - d3 >= 0 && d5 - d6 >= 0         edge bc    t = (d4 - d3) / ((d4 - d3) + (d5 - d6)), s = 1 - t
 *       7. otherwise                                       interior   s = vb / ((va + vb) + vc), t = vc / ((va + vb) + vc)
 *   A quotient whose denominator is 0 is 0: a zero-length edge and a zero-area face give a finite point of the triangle, never a NaN.  Then
 *       e = ap - (s ab + t ac)  (componentwise: two products, their sum, one difference),   dist2(p, f) = (e0 e0 + e1 e1) + e2 e2 >= +0
 *   the difference form of the chamfer section: nothing is expanded, nothing cancels where the point is near the face.  Every operation written here is one float32 operation
 *   with one rounding, in this order, nothing contracted; a comparison with a NaN is false.  The barycentrics reported are ((1 - s) - t, s, t).
 *   nearest   D_p[i] = min_f dist2(p_i, f), a(i) = the lowest f among the minima of this float32 dist2;  D_f[f] = min_i dist2(p_i, f), b(f) = the lowest i likewise.  The
 *             lexicographic minimum over (dist2, index) does not depend on how a scan is split or merged.  On a closed mesh a point nearest a shared edge or vertex is equally
 *             near several faces: a(i) is defined by THIS float32 dist2 and need not be the face another precision picks; the closest point itself is unique.  With non-finite
 *             inputs the values are unspecified, but every index lies in range.
 *   loss      = w_pf (1 / N) sum_i rho(D_p[i]) + w_fp (1 / F) sum_f rho(D_f[f]), weights[2] = (w_pf, w_fp);  rho(s) = s (squared != 0) or sqrt(s) (squared == 0), whose
 *             derivative at s = 0 is defined as 0.  A term whose weight is 0 is not evaluated: its reported value is exactly 0 and the gradients are the other term's bit for
 *             bit.  The terms are added in this order.
 *   gradient  the indices and the barycentrics are constants.  For the squared distance this is not a convention but the exact derivative: dist2 is the minimum over the
 *             triangle's points of |p - q|^2, and by the envelope theorem the derivative of a minimum with respect to a parameter is the partial derivative at the minimiser.
 *             For a chosen pair (i, f) with r = p_i - q, q = sum_c bary_c v_faces[f][c] - evaluated as the pair function's e, which is that difference without the
 *             cancellation - p_i receives +k r and v_faces[f][c] receives -k bary_c r, each product k r first, then times bary_c;  k(s) = 2 w / count (squared) or
 *             (w / count) / sqrt(s), 0 at s = 0 (not squared), w / count and 2 w / count rounded from double, s the pair's dist2.  The orders of addition:
 *               p_i       its own pair (i, a(i)), then the sum, started at 0 and added once, over the faces with b(f) = i in ascending f
 *               face f    a [3, 3] corner record: its own pair (b(f), f), then the sum, started at 0 and added once, over the points with a(i) = f in ascending i
 *               vertex    the corner records of the corners that name it, in ascending (face, corner) order (vc_begin / vc_corner below), added from 0
 *
 * psdr_hip_pointmesh_plan(n_queries, n_candidates) -> (tile, queries_per_lane, slices, slice_len): how either scan is split, a pure function, callable without a GPU.  A
 * workgroup of 256 lanes holds 256 queries_per_lane queries; slice s holds the candidates [s slice_len, min(count, (s + 1) slice_len)), slice_len a multiple of tile, no slice
 * empty; the grid is ceil(n_queries / (256 queries_per_lane)) x slices.  tile = 256; queries_per_lane = 2 for n_queries > 1024, else 1; slices = the fewest that bring the grid
 * to 2048 workgroups, at most one per tile.  The result of a scan does not depend on the plan.
 * psdr_hip_pointmesh_nearest(p, N, v, n, faces, F, direction, records, keys, index, bary, dist2): one scan.  direction 0: the points are the queries - index int32 [N] = a, bary
 * float32 [N, 3], dist2 float32 [N] = D_p; direction 1: the faces are - index [F] = b, bary [F, 3], dist2 [F] = D_f.  keys: uint64 work array with one entry per query (the minimum
 * of (float bits of dist2) << 32 | index, merged over the slices by an integer atomic minimum, after a clear to all ones on `stream`).  records: float32 [F, 16] work array,
 * direction 0 only (NULL otherwise): per face (a, ab, ac, b, c, 0), written once per call by a small kernel and staged through LDS by the scan; nothing else is precomputed.
 * The scan carries dist2 only; the barycentrics are those of the winning pair, evaluated once more per query by the same pair function.  Vertex ids read from `faces` are
 * clamped into [0, n).
 * psdr_hip_pointmesh_eval(p, N, v, n, faces, F, face_of_point, bary_p, dist2_p, point_of_face, bary_f, dist2_f, p_begin [N + 1], p_list [F], f_begin [F + 1], f_list [N],
 * vc_begin [n + 1], vc_corner [3 F], weights, squared, partial, corners, out, grad_p, grad_v): out[3] (device) = (loss, mean_i rho(D_p), mean_f rho(D_f)); grad_p [N, 3], grad_v
 * [n, 3] (device; both NULL for a value-only call, which gives the same out bits).  p_begin / p_list: the inverted index of point_of_face - p_list holds the f in ascending
 * (point_of_face[f], f) order (a stable sort), p_begin[i] the position of point i's first entry; f_begin / f_list the same for face_of_point.  vc_begin / vc_corner: per vertex
 * the corners 3 f + c that name it, ascending - the mesh's topology, from the host once per mesh.  All three are the caller's duty; the kernels clamp everything they read
 * from an index into range.  partial: double work array of ceil(N / 256) + ceil(F / 256) entries (the sums of rho are added in double in a fixed order, each mean is rounded to
 * float32 once); corners: float32 [F, 9] work array, the corner records.  The arrays of a direction whose weight is 0, and the inverted indices, vc_* and corners of a
 * value-only call, are not read and may be NULL.  One launch each for the points, the faces and the vertices, and one that adds the per-workgroup sums.
 * All three are refused with psdr_hip_last_error text before any device call for a count outside [1, 2^26], a direction other than 0 or 1, a NULL array that would be read or
 * written, a weight that is negative or not finite, one gradient without the other, and a gradient that aliases an input or the other gradient. */
int psdr_hip_pointmesh_plan(int32_t n_queries, int32_t n_candidates, int32_t *tile, int32_t *queries_per_lane, int32_t *slices, int32_t *slice_len);
int psdr_hip_pointmesh_nearest(const float *p, int32_t n_points, const float *v, int32_t n_vertices, const int32_t *faces, int32_t n_faces, int32_t direction,
                               float *records, uint64_t *keys, int32_t *index, float *bary, float *dist2, void *stream);
int psdr_hip_pointmesh_eval(const float *p, int32_t n_points, const float *v, int32_t n_vertices, const int32_t *faces, int32_t n_faces,
                            const int32_t *face_of_point, const float *bary_p, const float *dist2_p, const int32_t *point_of_face, const float *bary_f, const float *dist2_f,
                            const int32_t *p_begin, const int32_t *p_list, const int32_t *f_begin, const int32_t *f_list, const int32_t *vc_begin, const int32_t *vc_corner,
                            const float *weights, int32_t squared, double *partial, float *corners, float *out, float *grad_p, float *grad_v, void *stream);

/* THE SIGNED DISTANCE - FOR EVERY POINT THE GENERALIZED WINDING NUMBER OF A MESH, THE DISTANCE SIGNED BY IT, AND THE VECTOR-JACOBIAN PRODUCT OF THAT DISTANCE (csrc/hip/sdf.hip;
 * psdr_jit_amd/sdf.py).  What a penetration penalty, a containment or free-space constraint and supervision against signed distance samples need: which
 * side of the surface a point lies on.  The sign is that of the generalized winding number (Jacobson, Kavan, Sorkine-Hornung 2013): the sum of the signed solid angles of all
 * faces, 1 inside and 0 outside a closed mesh, degrading smoothly at holes where a normal-based sign is wrong.  Stateless entry points like the point-to-mesh ones: device
 * pointers, work arrays from the caller, plain launches on `stream`, no host synchronisation, no float atomics: the same input gives the same bits.  Added under ABI 16: nothing
 * existing changed.
 *
 * The definition.  p, v, faces, N, n, F as in the point-to-mesh section.  For a point p and a face with the corners A, B, C in the file's vertex order, with
 * x.y = (x0 y0 + x1 y1) + x2 y2 and x X y = (x1 y2 - x2 y1, x2 y0 - x0 y2, x0 y1 - x1 y0):
 *       a = A - p, b = B - p, c = C - p (componentwise),   la = sqrt(a.a), lb = sqrt(b.b), lc = sqrt(c.c)
 *       Nm = a . (b X c),   Dn = ((la lb) lc + (a.b) lc) + ((b.c) la + (c.a) lb)
 *       theta(p, f) = 0 if Nm == 0, else atan2(Nm, Dn)
 *   theta is half the signed solid angle of the face seen from p (Van Oosterom & Strackee 1983), in (-pi, pi].  The Nm == 0 branch is the principal value: a point in the
 *   face's plane, a point on a vertex and a face of zero area contribute 0, and no pair of finite inputs produces a NaN.  Every operation written here is one float32 operation
 *   with one rounding, in this order, nothing contracted, the square roots correctly rounded; atan2 is the device library's float32 atan2f.
 *   winding   w[i] = (1 / (2 pi)) sum_f theta(p_i, f).  The order of summation: the faces are split into the slices of psdr_hip_pointmesh_plan(N, F) - there is no second plan -
 *             a lane adds the thetas of a slice in ascending f into a double, started at 0, and rounds the slice's sum to float32 (partial[slice][i]); the slices are added in
 *             ascending order from 0 in double, the sum is multiplied by the double nearest 1 / (2 pi) and rounded to float32 once.  So the last bits of w depend on the plan -
 *             the one place where this operator differs from the point-to-mesh distance, whose results do not - and the plan is a pure function of (N, F): the same input gives
 *             the same bits.
 *   sign      inside[i] = (orientation w[i] > 1 / 2), orientation = +1 where the faces wind counter-clockwise seen from outside, -1 for the other winding.
 *   distance  s[i] = -sqrt(D_p[i]) if inside[i], else +sqrt(D_p[i]) (one correctly rounded square root);  D_p, a(i) and the barycentrics are exactly those of
 *             psdr_hip_pointmesh_nearest, direction 0, which the caller runs as it is.
 *   gradient  of s only; indices, barycentrics and the sign are constants.  With r_i the point-to-mesh pair function's e of the pair (i, a(i)) - p_i - q_i without the
 *             cancellation, q_i = bary_i . v[faces[a(i)]] - ds_i / dp_i = r_i / s_i and ds_i / dv[faces[a(i)][c]] = -bary_ic r_i / s_i, both 0 where s_i == 0 (D_p[i] = 0), as
 *             rho' is in the point-to-mesh section.  For an incoming g [N]: k_i = g_i / s_i (one division; 0 where s_i == 0), p_i receives k_i r_i, corner c of a(i) receives
 *             -((k_i r_i) bary_ic).  The orders of addition: a face's [3, 3] corner record is the sum, started at 0, over the points with a(i) = f in ascending i; a vertex adds
 *             the corner records of the corners that name it in ascending (face, corner) order (vc_begin / vc_corner), from 0.
 *             w and inside carry no gradient.  For a closed mesh the winding number is piecewise constant in the point and in the vertices: its analytic vertex gradient cancels
 *             to 1e-17 in float64.  It is the sign, not a differentiable quantity; the differentiable operator is the signed distance.
 *
 * psdr_hip_sdf_winding(p, N, v, n, faces, F, records, partial, dist2_or_null, orientation, w, sdf_or_null): w float32 [N]; with dist2 float32 [N] (D_p) also sdf float32 [N] = s,
 * both given or both NULL.  records: float32 [F, 12] work array, per face (A, B, C, 0, 0, 0), vertex ids clamped into [0, n), written once per call by a small kernel and staged
 * through LDS by the scan, which keeps the plan's queries per lane in registers; its grid is query blocks x slices.  partial: float32 [slices, N] work array, slices from
 * psdr_hip_pointmesh_plan(N, F); every entry is written by one lane, nothing is cleared.  One launch each for the records, the scan and the merge.  Nothing of size N x F exists.
 * psdr_hip_sdf_grad(p, N, v, n, faces, F, face, bary, sdf, g, f_begin [F + 1], f_list [N], vc_begin [n + 1], vc_corner [3 F], corners, grad_p, grad_v): the vector-Jacobian
 * product of s for the incoming g float32 [N]: grad_p [N, 3], grad_v [n, 3].  face int32 [N], bary float32 [N, 3]: a and the barycentrics from psdr_hip_pointmesh_nearest; sdf: s
 * from psdr_hip_sdf_winding.  f_begin / f_list: the inverted index of face (a stable sort); vc_begin / vc_corner: the mesh's vertex-to-corner index, as in
 * psdr_hip_pointmesh_eval; corners: float32 [F, 9] work array.  One launch each for the points, the faces and the vertices; the kernels clamp everything they read from an index
 * into range.
 * Both are refused with psdr_hip_last_error text before any device call for a count outside [1, 2^26], an orientation other than +1 or -1, a NULL array that would be read or
 * written, dist2 without sdf or sdf without dist2, and a gradient that aliases an input or the other gradient. */
int psdr_hip_sdf_winding(const float *p, int32_t n_points, const float *v, int32_t n_vertices, const int32_t *faces, int32_t n_faces, float *records, float *partial,
                         const float *dist2, int32_t orientation, float *w, float *sdf, void *stream);
int psdr_hip_sdf_grad(const float *p, int32_t n_points, const float *v, int32_t n_vertices, const int32_t *faces, int32_t n_faces, const int32_t *face, const float *bary,
                      const float *sdf, const float *g, const int32_t *f_begin, const int32_t *f_list, const int32_t *vc_begin, const int32_t *vc_corner, float *corners,
                      float *grad_p, float *grad_v, void *stream);

/* THE ISOSURFACE - MARCHING TETRAHEDRA: FROM A SIGNED DISTANCE ON A LATTICE TO A TRIANGLE MESH, THE POSITIONS OF ITS VERTICES AND THEIR VECTOR-JACOBIAN PRODUCT (csrc/hip/mtet.hip;
 * psdr_jit_amd/mtet.py).  The way back from the signed-distance section: that one makes a lattice of signed distances from any mesh, this one makes a
 * mesh from any lattice, so that an optimisation can change the topology (DMTet, Shen et al. 2021: optimise the values, extract at every step).  Stateless entry points: device
 * pointers, work arrays from the caller, plain launches on `stream`, no host synchronisation, no float atomics: the same input gives the same bits.  Added under ABI 16: nothing
 * existing changed.
 *
 * The definition.
 *   lattice     shape = (nx, ny, nz) vertices, every extent at least 2; vertex id u = x + nx (y + ny z); Nv = nx ny nz <= 2^24, so that every count and every 3 F offset fits an
 *               int32; cell id cx + (nx - 1) (cy + (ny - 1) cz).  sdf float32 [Nv], pos float32 [Nv, 3]; pos may be deformed (DMTet moves the lattice).
 *   tetrahedra  Kuhn's split, six per cell.  For the axis permutations (a, b, c) in the order xyz, xzy, yxz, yzx, zxy, zyx tet k has the corners q0 = the cell's low corner,
 *               q1 = q0 + e_a, q2 = q1 + e_b, q3 = q2 + e_c; tet id 6 cell + k.  The split is translation invariant: the face diagonals of neighbouring cells agree.
 *   edge slots  every edge of every tet is one of seven classes anchored at its low end, with the offsets d_0..6 = (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1); slot
 *               7 u + c is the edge from u to u + d_c and exists where that end lies in the lattice.
 *   inside      inside(u) = sdf[u] < 0: a zero is outside and so is a NaN.  A slot crosses where its two ends differ.  The mesh's vertices are the crossing slots in ascending
 *               slot order; edges int32 [V, 2] holds (a, b), a the anchor.
 *   position    t = s_a / (s_a - s_b), always from the anchor (the two values have opposite signs or one is zero: nothing cancels), p = p_a + t (p_b - p_a) per component, every
 *               operation one float32 rounding.  s_b = 0 gives t = 1, p = p_b up to the rounding of that formula; several slots may then coincide and faces of zero area
 *               result: defined, not an error.  With an infinite or NaN end the topology is as above and the position is unspecified.
 *   faces       a tet with 0 or 4 inside corners gives none.  One inside corner i - or, the mirror case, one outside corner i - gives the triangle of the slots e_ij, e_ik, e_il
 *               to the other three corners j < k < l in tet-local order.  Two inside corners i < j with the outside corners k < l give the quad e_ik, e_il, e_jl, e_jk, split along
 *               e_ik - e_jl into (e_ik, e_il, e_jl) and (e_ik, e_jl, e_jk).  Each triangle is then wound counter-clockwise seen from the outside (sdf >= 0) corners on a regular
 *               lattice of positive spacing - the signed distance's orientation = +1 - by exchanging its last two slots where needed.  The winding is a function of (k, mask)
 *               alone, a table, never a test on pos: a deformed lattice keeps the topological orientation.  Faces come in ascending tet id, the two of a quad in the order above.
 *   gradient    with the topology held constant.  For the slot (a, b), d = p_b - p_a, den = s_a - s_b, and an incoming g (the slot's row of g [V, 3]):
 *               w = ((g0 d0 + g1 d1) + g2 d2) / (den den);  s_a receives (-s_b) w, s_b receives s_a w, p_a receives (1 - t) g, p_b receives t g (dp/ds_a = -s_b d / den^2, dp/ds_b =
 *               s_a d / den^2, dp/dp_a = 1 - t, dp/dp_b = t).  A lattice vertex adds, from 0, its own seven slots in ascending class and then the seven slots it is the far end of
 *               (anchors u - d_c) in ascending class: fourteen fixed look-ups, no sort, no inverted index, no float atomics.
 *
 * The index of slot 7 u + c among the mesh's vertices is base[u] + popcount(mask[u] & ((1 << c) - 1)): mask uint8 [Nv] holds the seven crossing bits of a lattice vertex and
 * base int32 [Nv] the exclusive scan of their popcounts.  These five bytes per lattice vertex are the whole topology state a later call needs (a slot table would take 28).
 * The scans are reduce / scan of the workgroup sums / scatter in plain launches over tiles of 256 entries - no workgroup waits for another - so Nv <= 256^3 needs at most two
 * passes over workgroup sums.  psdr_hip_mtet_plan(nx, ny, nz) -> (tile = 256, vertex_blocks = ceil(Nv / tile), cell_blocks = ceil(cells / tile), vertex_passes, cell_passes:
 * 1 where the blocks fit one tile, else 2, scratch_ints): a pure function, callable without a GPU.
 * psdr_hip_mtet_count(sdf, nx, ny, nz, mask, base, cell_faces, cell_base, scratch, totals): mask and base as above; cell_faces uint8 [cells] the faces of a cell's six tets
 * (0 .. 12), cell_base int32 [cells] their exclusive scan (one lane emits a cell's tets in ascending k, so one offset per cell serves and nothing of size 6 cells exists);
 * scratch int32 [scratch_ints]; totals int32 [2] (device) = (V, F).  Nothing is cleared, every entry is written by one lane.
 * psdr_hip_mtet_emit(sdf, nx, ny, nz, mask, base, cell_base, num_vertices, num_faces, edges, edge_rows, faces, face_rows): edges int32 [V, 2], faces int32 [F, 3], two launches.
 * num_vertices and num_faces are the totals the caller read, edge_rows and face_rows the rows of the arrays it gives; sdf must be the one the count saw.  The kernels write no
 * row beyond those given.  psdr_hip_mtet_vertices(sdf, pos, nx, ny, nz, edges, num_vertices, v): v float32 [V, 3], one launch; ids read from edges are clamped into [0, Nv).
 * psdr_hip_mtet_vertices_adj(sdf, pos, nx, ny, nz, mask, base, num_vertices, g, grad_sdf, grad_pos): the vector-Jacobian product for g float32 [V, 3]: grad_sdf [Nv], grad_pos
 * [Nv, 3], one launch, every entry written (0 where no slot crosses).
 * All are refused with psdr_hip_last_error text before any device call for a NULL array, an extent below 2, more than 2^24 lattice vertices, num_vertices outside [1, 7 Nv] or
 * num_faces outside [1, 12 cells] (a lattice without a crossing has nothing to emit: the caller skips the call), totals that disagree with the rows given to the emit, and
 * outputs that alias an input or each other. */
int psdr_hip_mtet_plan(int32_t nx, int32_t ny, int32_t nz, int32_t *tile, int32_t *vertex_blocks, int32_t *cell_blocks, int32_t *vertex_passes, int32_t *cell_passes,
                       int32_t *scratch_ints);
int psdr_hip_mtet_count(const float *sdf, int32_t nx, int32_t ny, int32_t nz, uint8_t *mask, int32_t *base, uint8_t *cell_faces, int32_t *cell_base, int32_t *scratch,
                        int32_t *totals, void *stream);
int psdr_hip_mtet_emit(const float *sdf, int32_t nx, int32_t ny, int32_t nz, const uint8_t *mask, const int32_t *base, const int32_t *cell_base, int32_t num_vertices,
                       int32_t num_faces, int32_t *edges, int32_t edge_rows, int32_t *faces, int32_t face_rows, void *stream);
int psdr_hip_mtet_vertices(const float *sdf, const float *pos, int32_t nx, int32_t ny, int32_t nz, const int32_t *edges, int32_t num_vertices, float *v, void *stream);
int psdr_hip_mtet_vertices_adj(const float *sdf, const float *pos, int32_t nx, int32_t ny, int32_t nz, const uint8_t *mask, const int32_t *base, int32_t num_vertices,
                               const float *g, float *grad_sdf, float *grad_pos, void *stream);

/* THE LATTICE REGULARISERS - EIKONAL, LAPLACIAN, SIGN-CHANGE CROSS-ENTROPY OF A SIGNED DISTANCE ON A REGULAR LATTICE - VALUE AND GRADIENT IN ONE FUSED STENCIL (csrc/hip/latreg.hip;
 * psdr_jit_amd/latreg.py).  The term of a DMTet / nvdiffrec-style loop that depends on the lattice alone: marching tetrahedra hands a gradient to the two
 * ends of a crossing edge only, and nothing else keeps the rest of the field a distance, smooth and free of sign changes that no pixel sees.  What the mesh regularisers are to
 * a fixed topology.  Stateless entry points: device pointers, work arrays from the caller, plain launches on `stream`, no host synchronisation, no atomics, every output entry
 * written by one lane in a fixed order: the same input gives the same bits.  Added under ABI 16: nothing existing changed.
 *
 * The definition.
 *   lattice     THE ISOSURFACE's: shape = (nx, ny, nz) vertices, every extent at least 2, vertex id u = x + nx (y + ny z), Nv = nx ny nz <= 2^24, inside(u) = sdf[u] < 0 (a zero
 *               is outside), Nc = (nx - 1) (ny - 1) (nz - 1) cells.  The lattice is regular with the spacing h = (hx, hy, hz) > 0 (float64, host); a deformed lattice is out of
 *               scope.  The divisions by the spacing are multiplications by the float32 roundings of 1 / (4 h_a) and 1 / h_a^2, formed in float64 on the host.
 *   eikonal     = (1 / Nc) sum_cells e_c, e_c = (n - 1)^2, n = sqrt((g_x^2 + g_y^2) + g_z^2), g_x = ((((s100 - s000) + (s110 - s010)) + (s101 - s001)) + (s111 - s011)) / (4 hx)
 *               the mean of the cell's four x-edge differences (s_xyz: the corner at offset (x, y, z) from the cell's low corner), g_y and g_z likewise with the differences
 *               in the order of their low ends 000, 100, 001, 101 for y and 000, 100, 010, 110 for z (x: 000, 010, 001, 011).  A cell with n = 0 adds 1 and no gradient: defined,
 *               not NaN.  d e_c / d s_corner = sum_a (+-) q_a, q_a = (2 (n - 1) (g_a / n)) / (4 h_a), + where the corner is the high end of axis a.
 *   laplacian   = (1 / Nv) sum_u r_u^2, r_u = sum_a ((s_{u - e_a} - s_u) + (s_{u + e_a} - s_u)) / h_a^2 over the axes a, in the order x, y, z, along which u has both
 *               neighbours (the two-difference form: it does not cancel as s_- - 2 s + s_+ does).  An axis of extent 2 contributes nowhere and a vertex on a boundary face
 *               omits the axis normal to it, so a linear field gives exactly 0.  d / d s_u = (2 / Nv) sum_a (-2 r_u [u interior along a] + r_{u - e_a} [u - e_a interior along
 *               a] + r_{u + e_a} [u + e_a interior along a]) / h_a^2.
 *   sign        nvdiffrec's sdf_reg_loss over the lattice edges of the seven classes d in {0, 1}^3 \ {0} - THE ISOSURFACE's slots, the edges of Kuhn's tetrahedra.  For every edge
 *               (a, b) with inside(a) != inside(b) add bce(k s_a, y_b) + bce(k s_b, y_a), y_j = 0 if inside(j) else 1, bce(x, y) = max(x, 0) - x y + log1p(exp(-|x|)), k =
 *               sign_scale; sign = (1 / V) sum, V the number of crossing edges, held constant in the gradient; V = 0 gives 0 and a zero gradient.  Each of the two summands is
 *               softplus(k |s|) of its own end (softplus(t) = t + log1p(exp(-t))), so the sum is the per-vertex form (1 / V) sum_u m_u softplus(k |s_u|), m_u the crossing edges
 *               among u's fourteen - the form the kernels evaluate - with d / d s_u = (+-) (k / V) m_u / (1 + exp(-k |s_u|)), - where u is inside.
 *   loss        = w_eik eikonal + w_lap laplacian + w_sign sign, weights = (w_eik, w_lap, w_sign); a term of weight 0 is not evaluated and reports 0 (crossings too reports 0
 *               where w_sign = 0).  The gradient adds the evaluated terms in that order.
 * sdf is expected to be finite; nothing checks it (a check would synchronise).  Every address is computed from lattice coordinates, never from data: a NaN gives NaNs, not an
 * access out of range.
 *
 * psdr_hip_latreg_plan(nx, ny, nz) -> (tile_x, tile_y, tile_z: the vertices of a workgroup's tile, workgroups = the product of ceil(n_a / tile_a), scratch_floats = 4
 * workgroups): a pure function, callable without a GPU.
 * psdr_hip_latreg_eval(sdf, nx, ny, nz, spacing, weights, sign_scale, scratch, out, crossings, grad): sdf float32 [Nv]; spacing float64 [3] and weights float32 [3] on the host;
 * scratch float32 [scratch_floats] the workgroups' partial sums; out float32 [4] = (loss, eikonal, laplacian, sign); crossings int32 [1] = V, which stays on the device: the
 * gradient pass reads it there; grad float32 [Nv] = d loss / d sdf, or NULL for a value-only call.  Three launches (two without grad): the workgroups' partial sums in a fixed
 * order, one finishing workgroup that adds them in float64, the gradient.  Every work array is the caller's, one set per call in flight; nothing is cleared, every entry is
 * written.  Refused with psdr_hip_last_error text before any device call: a NULL required array, an extent below 2, more than 2^24 lattice vertices, a spacing that is not finite
 * and positive (or whose 1 / (4 h) or 1 / h^2 is no positive float32), a weight or sign_scale that is negative or not finite, and scratch, out, crossings or grad that alias sdf
 * or each other. */
int psdr_hip_latreg_plan(int32_t nx, int32_t ny, int32_t nz, int32_t *tile_x, int32_t *tile_y, int32_t *tile_z, int32_t *workgroups, int32_t *scratch_floats);
int psdr_hip_latreg_eval(const float *sdf, int32_t nx, int32_t ny, int32_t nz, const double *spacing, const float *weights, float sign_scale, float *scratch, float *out,
                         int32_t *crossings, float *grad, void *stream);

/* sampler building blocks (host side, bit-exact with the kernels): known-answer tests */
uint64_t psdr_hip_tea64(uint64_t v0, uint64_t v1);
int psdr_hip_sampler_floats(uint64_t seed_value, uint64_t lane, uint64_t skip, int32_t n, float *out_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PSDR_HIP_H */
