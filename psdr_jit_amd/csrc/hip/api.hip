// api.hip — the host unit of libpsdr_hip.so: the C ABI (include/psdr_hip.h) and the small kernels it launches.
//
// The kernel templates are in render_kernels.h.  The heavy ones are compiled in units of their own (render_units.hip): this file
// declares their instantiations extern, validates a call, fills the kernel parameters and launches.
// There is no host synchronisation inside a render call (the reference syncs before each of its 7+
// OptiX launches, scene_optix.cpp:345).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../../include/psdr_hip.h"
#include "scene_obj.h"
#include "render_kernels.h"

// ------------------------------------------------------------------------------------------------
// error plumbing
// (psdr::api_fail and HIPCHK: scene_obj.h; the message store itself is in the host part of this file)
[[maybe_unused]] static int fail(const std::string &msg) { return psdr::api_fail(msg); }

// the heavy kernels: every instantiation the launch layer below can name is defined in one of the kernel units
PSDR_TU1(extern) PSDR_TU2(extern) PSDR_TU3(extern) PSDR_TU4(extern) PSDR_TU5(extern) PSDR_TU6(extern) PSDR_TU7(extern) PSDR_TU8(extern) PSDR_TU9(extern) PSDR_TU10(extern)

// ------------------------------------------------------------------------------------------------
// the plain kernels of this unit (its small kernel TEMPLATES - k_trace, k_intersect*, k_guiding_round - are in render_kernels.h and are
// instantiated here, where they are launched)
// EnvironmentMap::sample_position / sample_position_pdf alone (parity aids)
__global__ void k_env_sample(const SceneTables T, int n, const float *__restrict__ ref_p, const float *__restrict__ s2,
                             float *__restrict__ out_p, float *__restrict__ out_n, float *__restrict__ out_pdf) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Vec3f p, nn; float pdf;
    env_sample_position(T.env, Vec3f(ref_p[3 * i], ref_p[3 * i + 1], ref_p[3 * i + 2]), s2[2 * i], s2[2 * i + 1], p, nn, pdf);
    out_p[3 * i] = p.x; out_p[3 * i + 1] = p.y; out_p[3 * i + 2] = p.z;
    out_n[3 * i] = nn.x; out_n[3 * i + 1] = nn.y; out_n[3 * i + 2] = nn.z;
    out_pdf[i] = pdf;
}
__global__ void k_env_pdf(const SceneTables T, int n, const float *__restrict__ ref_p, const float *__restrict__ p, const float *__restrict__ nrm,
                          float *__restrict__ out_pdf) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out_pdf[i] = env_position_pdf(T.env, Vec3f(ref_p[3 * i], ref_p[3 * i + 1], ref_p[3 * i + 2]), Vec3f(p[3 * i], p[3 * i + 1], p[3 * i + 2]),
                                  Vec3f(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]));
}

// Batch rendering with edge terms (psdr_hip_render_d_fwd_batch / _bwd_batch).  The edge samples of a renderD are spread over the WHOLE frame; the ones whose pixel is in
// the list are kept.  slot_of[full-frame pixel] = the smallest k with pix_ids[k] == pixel (unsigned atomicMin over a table preset to ~0u = -1: deterministic with
// duplicates), -1 = not listed: SceneTables::slot_of, read by the edge kernels where a sample's pixel becomes known.  Kept samples add into (forward) / read their adjoint
// from (reverse) a buffer of n_pix rows indexed by that representative slot; the two kernels below carry it to and from the caller's rows, duplicates included.
__global__ void k_batch_slots(const int *__restrict__ pix_ids, int n_pix, int n_full, int *__restrict__ slot_of) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_pix) return;
    const int p = pix_ids[k];
    if (p >= 0 && p < n_full) atomicMin(reinterpret_cast<unsigned *>(slot_of) + p, (unsigned) k);
}
// forward: row k += the edge share of pixel pix_ids[k]
__global__ void k_batch_gather(const int *__restrict__ pix_ids, int n_pix, int n_full, const int *__restrict__ slot_of, const float *__restrict__ rows, float *__restrict__ dout) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_pix) return;
    const int p = pix_ids[k];
    if (p < 0 || p >= n_full) return;
    const int s = slot_of[p];
    if (s < 0 || s >= n_pix) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) { const float v = rows[3 * (long long) s + c]; if (v != 0.f) dout[3 * (long long) k + c] += v; }
}
// reverse: the adjoint an edge sample on pixel p sees = the sum of d_rgb over the rows k with pix_ids[k] == p, kept at p's representative slot
__global__ void k_batch_reduce(const int *__restrict__ pix_ids, int n_pix, int n_full, const int *__restrict__ slot_of, const float *__restrict__ d_rgb, float *__restrict__ rows) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_pix) return;
    const int p = pix_ids[k];
    if (p < 0 || p >= n_full) return;
    const int s = slot_of[p];
    if (s < 0 || s >= n_pix) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) { const float v = d_rgb[3 * (long long) k + c]; if (v != 0.f) atomicAdd(&rows[3 * (long long) s + c], v); }
}

__global__ void k_sampler_floats(unsigned long long seed_value, unsigned long long lane, unsigned long long skip, int n, float *out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        LaneRng r; r.seed(seed_value, lane, skip_ahead(skip));        // (the kernels' form of the skip-ahead: sampler.h)
        for (int i = 0; i < n; ++i) out[i] = r.next_1d();
    }
}

// ------------------------------------------------------------------------------------------------
// host side (the scene object, its creation and its updates: scene_obj.h, scene_build.hip)
static thread_local std::string g_err;
namespace psdr { int api_fail(const std::string &msg) { g_err = msg; return 1; } }

struct psdr_hip_guiding {
    GuidingDev G{};
    DevBuf pmf, cmf, guide;
    std::vector<float> mass;
};


extern "C" {

const char *psdr_hip_last_error(void) { return g_err.c_str(); }
int psdr_hip_abi_version(void) { return PSDR_HIP_ABI_VERSION; }
int psdr_hip_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }
int psdr_hip_set_device(int device) { HIPCHK(hipSetDevice(device)); return 0; }

} // extern "C"

// number of 256-lane chunks of [0, n) that belong to shard `rank` of `count` (chunk k -> rank k % count)
static inline long long local_lanes(long long n, int rank, int count) {
    const long long chunks = (n + kBlock - 1) / kBlock;
    const long long mine = chunks > rank ? (chunks - rank + count - 1) / count : 0;
    return mine * kBlock;
}
// psdr_render_args.shard_mode == PSDR_SHARD_ROWS: rank `rank` of `count` owns one CONTIGUOUS run of a sampler's lanes, a whole number of `unit` lanes (a pixel row of the
// interior sampler - the rank's pixels are then one block of the image -, a pixel of a batch list, a 256-lane chunk of an edge sampler); the kernels see it as the lane range
// [begin, end) of a single rank, the form the per-lane entry points use
static inline void shard_run(long long n_lanes, long long unit, int rank, int count, long long &begin, long long &end) {
    const long long n_units = (n_lanes + unit - 1) / unit, per = (n_units + count - 1) / count;
    begin = std::min(n_lanes, (long long) rank * per * unit);
    end = std::min(n_lanes, ((long long) rank + 1) * per * unit);
}
template <typename Params> static inline void set_shard(Params &P, const psdr_render_args *a, long long n_lanes, long long unit, int rank, int count) {
    P.begin = 0; P.end = n_lanes; P.shard_rank = rank; P.shard_count = count;
    if (count > 1 && a->shard_mode == PSDR_SHARD_ROWS) { shard_run(n_lanes, unit, rank, count, P.begin, P.end); P.shard_rank = 0; P.shard_count = 1; }
    P.n_local = local_lanes(P.end - P.begin, P.shard_rank, P.shard_count);
}
static inline int grid_for(const psdr_hip_scene *sc, long long n) {
    long long chunks = (n + kBlock - 1) / kBlock;
    if (chunks < 1) chunks = 1;
    return (int) std::min<long long>(chunks, sc->grid);
}

// ------------------------------------------------------------------------------------------------
// the launch layer
//
// Development builds can leave scene classes out (hipcc -DPSDR_CLS_MASK=4 compiles the class-2 kernels only: a third of the build
// time); bit c = scene class c (scene_dev.h).  A scene of a class that is compiled out fails loudly.
#ifndef PSDR_CLS_MASK
#define PSDR_CLS_MASK 15
#endif
// IF_CLS<c>(x): x where class c is built, nothing where it is not (dropped by the preprocessor: x names kernels that no unit of such a build defines)
#if (PSDR_CLS_MASK) & 1
#define IF_CLS0(...) __VA_ARGS__
#else
#define IF_CLS0(...) (void) 0
#endif
#if (PSDR_CLS_MASK) & 2
#define IF_CLS1(...) __VA_ARGS__
#else
#define IF_CLS1(...) (void) 0
#endif
#if (PSDR_CLS_MASK) & 4
#define IF_CLS2(...) __VA_ARGS__
#else
#define IF_CLS2(...) (void) 0
#endif
#if (PSDR_CLS_MASK) & 8
#define IF_CLS3(...) __VA_ARGS__
#else
#define IF_CLS3(...) (void) 0
#endif
// ON_CLS(c, launch): the launch of a class-c kernel, or the failure of a call that needs a class this build leaves out
#define ON_CLS(c, ...) do { if (!(((PSDR_CLS_MASK) >> c) & 1)) return fail("scene class " #c " is compiled out of this development build"); IF_CLS##c(__VA_ARGS__); } while (0)

// THE CLASS DISPATCH: the one place that knows which instantiations of the heavy kernels exist (the PSDR_TU lists of render_kernels.h).  K names a function-like macro,
// K(C) = the launch of a kernel's class-C instantiation, defined where the kernel is launched.  Only the rungs written here are expanded: a template or a generic lambda
// over the class would make this unit instantiate, for all four classes, kernels that no unit defines.
//   forward mode: classes 0-3.  Class 3 has the uncounted instantiations only (CLS_COUNTED; call_shape gives a counted run of such a scene class 0).
//   reverse mode: classes 0-2.  There are no class-3 adjoint kernels (call_shape gives such a scene class 0).
#define CLS_COUNTED(C, COUNT) ((C) != 3 && (COUNT))
#define LAUNCH_CLS_(cls, K, RUNG3) do { if ((cls) == 1) ON_CLS(1, K(1)); else if ((cls) == 2) ON_CLS(2, K(2)); RUNG3 else ON_CLS(0, K(0)); } while (0)
#define LAUNCH_CLS_FWD(cls, K) LAUNCH_CLS_(cls, K, else if ((cls) == 3) ON_CLS(3, K(3));)
#define LAUNCH_CLS_REV(cls, K) LAUNCH_CLS_(cls, K, )
// THE VARIANT DISPATCH of the forward path kernels (paths.h::Switches): the lean instantiations exist for classes 1 and 2, uncounted (PSDR_TU9 / PSDR_TU10); every
// other rung names the general kernel twice.  `lean_`: this call is one the lean kernels are compiled for (render_impl)
#define PATHS_VAR(C, COUNT) ((((C) == 1 || (C) == 2) && !(COUNT)) ? kLean : kGeneral)
#define LAUNCH_PATHS(C, AD_, COUNT, MODE_, lean_, sc, n_lanes, stream, ...) \
    do { if (lean_) LAUNCH(C, (k_paths<AD_, C, CLS_COUNTED(C, COUNT), MODE_, PATHS_VAR(C, COUNT)>), sc, n_lanes, stream, __VA_ARGS__); \
         else LAUNCH(C, (k_paths<AD_, C, CLS_COUNTED(C, COUNT), MODE_, kGeneral>), sc, n_lanes, stream, __VA_ARGS__); } while (0)

// dynamic LDS of a kernel of scene class `cls` (0 global tables, 1 LDS blob, 2 lean BVH, 3 LDS blob with materials): the traversal stack / cold rows,
// plus the blob only for the classes that stage it - a class-0 kernel launched on a scene that ALSO has an LDS class (reverse mode,
// counted runs, ray batches, field integrators on Microfacet / bitmap boxes) must not reserve the blob's bytes it never fills
static size_t smem_for(const psdr_hip_scene *sc, int cls) {
    const size_t blob = (sc->lds || sc->lds_mat) ? (size_t) sc->T.blob_words * 16 : 0;
#ifdef PSDR_DEV_KNOBS
    // (measurement: PSDR_PAD_LDS=bytes asks for more LDS per workgroup than the kernels use - fewer workgroups per CU, to see what occupancy is worth)
    static const size_t pad = std::getenv("PSDR_PAD_LDS") ? (size_t) std::atoll(std::getenv("PSDR_PAD_LDS")) : 0;
    return ((cls == 1 || cls == 3) ? sc->smem_bytes : sc->smem_bytes - blob) + pad;
#else
    return (cls == 1 || cls == 3) ? sc->smem_bytes : sc->smem_bytes - blob;
#endif
}
// ... of a reverse-mode kernel other than k_paths: the cold path-state rows of brute-force scenes belong to run_paths, the adjoint kernels get tables without them
static int adj_cold_rows(const SceneTables &T) {
#ifdef PSDR_NO_ASYNC
    return kColdRows;
#else
    return T.n_tris > kBruteForceMax ? 0 : kColdRows;
#endif
}
static size_t smem_for_adjoint(const psdr_hip_scene *sc, int cls) { return smem_for(sc, cls) - (size_t) adj_cold_rows(sc->T) * kBlock * sizeof(int); }
// persistent workgroups over `n_lanes` work items with `smem` bytes of dynamic LDS / with the LDS of scene class `cls_`
#define LAUNCH_SM(kernel, sc, n_lanes, smem, stream, ...) \
    hipLaunchKernelGGL(kernel, dim3(grid_for(sc, n_lanes)), dim3(kBlock), smem, (hipStream_t) (stream), __VA_ARGS__)
#define LAUNCH(cls_, kernel, sc, n_lanes, stream, ...) LAUNCH_SM(kernel, sc, n_lanes, smem_for(sc, cls_), stream, __VA_ARGS__)
// ray batches and guiding rounds: the small kernel templates of this unit (in every build, whatever its class mask), on the LDS blob (1) or on global memory (0)
#define LAUNCH_RAYS(K, sc, n_lanes, stream, ...) \
    do { if ((sc)->lds) LAUNCH(1, (K<1>), sc, n_lanes, stream, __VA_ARGS__); else LAUNCH(0, (K<0>), sc, n_lanes, stream, __VA_ARGS__); } while (0)

// What a render call is: validated and derived once, for the forward and the reverse path.
struct CallShape {
    int count, rank;      // the shard of this call (1, 0: the whole frame)
    int cls;              // scene class of the kernels (scene_dev.h)
    int fh_field;         // field of a first-hit integrator, -1: PathTracer
    int depth;            // path depth the kernels trace
    int terms;            // PSDR_TERM_* this call evaluates
};
// `ad`: a renderD (forward or reverse mode); `cls3`: the class-3 instantiations exist for this kind of call (see the class dispatch above);
// `entry`: the full-frame entry point's name, for the message of its batch sibling
static int call_shape(const psdr_hip_scene *sc, const psdr_render_args *a, bool ad, bool cls3, bool batch_edges, const char *entry, CallShape &s) {
    if (!sc || !a) return fail("null argument");
    if (a->sensor_id < 0 || a->sensor_id >= (int) sc->sensors.size()) return fail("Invalid sensor id!");
    if (a->max_depth < 0) return fail("max_depth >= 0");
    if (a->pix_ids && a->n_pix <= 0) return fail("batch rendering needs n_pix > 0");
    // Scene::sample_emitter_position asserts "No Emitter!" (reference scene.cpp:989); the first-hit integrators and
    // PathTracer(0) never sample an emitter, so emitter-less scenes (silhouette / depth rendering) are fine there
    if (sc->T.n_emitters == 0 && a->field_mode == 0 && (a->direct_mode > 0 || a->max_depth > 0)) return fail("No Emitter!");
    if (batch_edges && !a->pix_ids) return fail(std::string(entry) + "_batch needs args->pix_ids (the full frame has its edge terms in " + entry + ")");
    s.count = a->shard_count > 1 ? a->shard_count : 1;
    s.rank = s.count > 1 ? a->shard_rank : 0;
    if (s.rank < 0 || s.rank >= s.count) return fail("bad shard rank");
    if (a->shard_mode != PSDR_SHARD_INTERLEAVED && a->shard_mode != PSDR_SHARD_ROWS) return fail("bad shard mode");
    if (a->field_mode < 0 || a->field_mode > 9) return fail("bad field_mode");
    // the first-hit integrators (field_mode) live in the class-0 instantiations only
    s.cls = a->field_mode != 0 ? 0 : (sc->lds ? 1 : (sc->lean ? 2 : ((sc->lds_mat && cls3) ? 3 : 0)));
    s.fh_field = a->field_mode - 1;
    s.depth = s.fh_field >= 0 ? 0 : (a->direct_mode > 0 ? 1 : a->max_depth);
    s.terms = (ad ? (a->terms ? a->terms : 7) : PSDR_TERM_INTERIOR) & ((a->field_mode > 0 || sc->T.n_emitters == 0) ? ~PSDR_TERM_SECONDARY : ~0);   // first-hit integrators have no secondary-edge term
    return 0;
}

// the kernel parameters (PathParams / AdjointParams) of sampler `sampler`: the fields all samplers share, and this call's shard of the sampler's `n_lanes` lanes
template <typename Params>
static Params sampler_params(const psdr_render_args *a, const CallShape &s, int sampler, long long n_lanes, long long unit) {
    Params P{};
    P.max_depth = s.depth; P.mis = a->direct_mode - 1; P.field = s.fh_field; P.field_object = a->field_object; P.intensity = a->intensity; P.d_intensity = a->d_intensity;
    P.hide_emitters = a->hide_emitters; P.seed = a->samplers[sampler].seed; P.skip = skip_ahead(a->samplers[sampler].skip);
    set_shard(P, a, n_lanes, unit, s.rank, s.count);
    return P;
}

// a zeroed work-queue counter for one launch, from the scene's ring
static int next_queue(const psdr_hip_scene *sc, hipStream_t st, unsigned long long *&q) {
    q = (unsigned long long *) sc->queues.p + (sc->queue_slot++ % kQueueRing);
    HIPCHK(hipMemsetAsync(q, 0, sizeof(unsigned long long), st));
    return 0;
}

// batch rendering with edge terms: builds the pixel -> slot map of this call's list in the scene's scratch (k_batch_slots) and clears the n_pix edge rows
static int batch_edge_scratch(const psdr_hip_scene *sc, const psdr_render_args *a, hipStream_t st, int *&slot_of, float *&rows) {
    const size_t n_full = (size_t) sc->T.width * sc->T.height;
    const size_t map_bytes = sizeof(int) * n_full, row_bytes = sizeof(float) * 3 * (size_t) a->n_pix;
    if (n_full >= (1ull << 31)) return fail("batch rendering with edge terms: frame too large");
    if (sc->batch_map.bytes < map_bytes || sc->batch_rows.bytes < row_bytes) {
        // (every earlier user of the scratch was ordered before this stream by the guard: its completion is this stream's)
        HIPCHK(hipStreamSynchronize(st));
        if (sc->batch_map.bytes < map_bytes && sc->batch_map.ensure(map_bytes)) return 1;
        if (sc->batch_rows.bytes < row_bytes && sc->batch_rows.ensure(row_bytes)) return 1;
    }
    slot_of = (int *) sc->batch_map.p; rows = (float *) sc->batch_rows.p;
    HIPCHK(hipMemsetAsync(slot_of, 0xff, map_bytes, st));
    HIPCHK(hipMemsetAsync(rows, 0, row_bytes, st));
    hipLaunchKernelGGL(k_batch_slots, dim3((a->n_pix + 255) / 256), dim3(256), 0, st, a->pix_ids, a->n_pix, (int) n_full, slot_of);
    return 0;
}

// sq / dsq (psdr_hip_render_c_sq / _d_fwd_sq; NULL = a plain call): the per-pixel sums of squared sample contributions, rows as out / dout
template <bool COUNT>
static int render_impl(const psdr_hip_scene *sc, const psdr_render_args *a, bool ad, float *out, float *dout, float *lanes_out,
                       long long lane_b, long long lane_e, psdr_counters *counters, void *stream, bool batch_edges = false, float *sq = nullptr, float *dsq = nullptr) {
    CallShape s;
    if (call_shape(sc, a, ad, !COUNT, batch_edges, "psdr_hip_render_d_fwd", s)) return 1;
    SCRATCH_GUARD(sc, stream);
    const SceneTables &T = sc->T;
    hipStream_t st = (hipStream_t) stream;
    const long long npx = a->pix_ids ? a->n_pix : (long long) T.width * T.height;
    if (a->zero_output) {
        if (out) HIPCHK(hipMemsetAsync(out, 0, sizeof(float) * 3 * npx, st));
        if (dout) HIPCHK(hipMemsetAsync(dout, 0, sizeof(float) * 3 * npx, st));
        if (sq) HIPCHK(hipMemsetAsync(sq, 0, sizeof(float) * 3 * npx, st));
        if (dsq) HIPCHK(hipMemsetAsync(dsq, 0, sizeof(float) * 3 * npx, st));
    }
    Counters *ctr = (Counters *) sc->counters.p;
    if (COUNT) HIPCHK(hipMemsetAsync(ctr, 0, sizeof(Counters), st));
#if PSDR_DIAG == 13 || PSDR_DIAG == 14
    if (!COUNT) HIPCHK(hipMemsetAsync(ctr, 0, sizeof(Counters), st));
#endif
    const SensorDev &cam = sc->sensors[a->sensor_id];
    const int terms = s.terms, cls = s.cls;

    // The three terms of a renderD are independent launches that add into the same two images: each is a grid of persistent workgroups that drains its own queue,
    // and the last workgroups of one launch leave most of the device idle while they finish.  With the edge terms on two side streams of the scene (forked from the
    // caller's stream after the clears, joined before the call returns) the next term's workgroups take the slots as they free up.
    hipStream_t s_prim = st, s_sec = st;
    // (BVH scenes only: config 5 219.3 -> 217.9 ms; the brute-force classes lose - C3 7.09 -> 7.34 ms - because a second kernel's waves beside a VALU-bound one only take issue slots)
    // (PSDR_NO_FORK: measurement / test knob, read per call - the three terms one after the other on the caller's stream, so that a profiler sees each kernel's own
    //  duration (tools/profile.sh) and a test can compare the forked call with the serial one)
    const bool no_fork = std::getenv("PSDR_NO_FORK") != nullptr;
    const bool fork = !no_fork && ad && !a->pix_ids && !lanes_out && !COUNT && T.n_tris > kBruteForceMax && ((terms & (PSDR_TERM_PRIMARY | PSDR_TERM_SECONDARY)) != 0) && (terms & (terms - 1)) != 0;
    // the lean path kernels: forward mode (this function), PathTracer, perspective sensor, no per-lane output - what they fix at compile time (paths.h::Switches)
    // (PSDR_NO_LEAN: measurement / test knob, read per call - the general kernels, which compute the same samples)
    // (a call with the squares takes the general kernels: the lean ones have no second accumulation)
    const bool lean = std::getenv("PSDR_NO_LEAN") == nullptr && a->direct_mode == 0 && a->field_mode == 0 && !lanes_out && !sq && !dsq && !cam.ortho;
    unsigned long long *q_int = nullptr, *q_prim = nullptr, *q_sec = nullptr;
    // concurrent launches must not share the global tail of the traversal stack (trav4.h indexes it by workgroup and thread only): the edge terms get slices of their own
    SceneTables T_prim = T, T_sec = T;
    if (fork && T.gstack != nullptr) { T_prim.gstack = T.gstack + sc->gstack_slice; T_sec.gstack = T.gstack + 2 * sc->gstack_slice; }
    if (fork) {
        if (sc->make_term_streams()) return fail("term streams: cannot create");
        if (next_queue(sc, st, q_int) || next_queue(sc, st, q_prim) || next_queue(sc, st, q_sec)) return 1;
        HIPCHK(hipEventRecord(sc->ev_fork, st));
        HIPCHK(hipStreamWaitEvent(sc->aux[0], sc->ev_fork, 0));
        HIPCHK(hipStreamWaitEvent(sc->aux[1], sc->ev_fork, 0));
        s_prim = sc->aux[0]; s_sec = sc->aux[1];
    }
    if ((terms & PSDR_TERM_INTERIOR) && T.spp > 0) {
        PathParams P = sampler_params<PathParams>(a, s, 0, npx * T.spp, a->pix_ids ? (long long) T.spp : (long long) T.width * T.spp);
        P.pix_ids = a->pix_ids;
        P.out = out; P.dout = dout; P.lanes_out = lanes_out; P.sq = sq; P.dsq = dsq;
        // the wave's start threshold (paths.h GROUPED STARTS; the kernel itself keeps 1 on the routes that trace the camera ray)
        // (PSDR_GROUP_START: measurement / test knob, read per call - 0 = lane by lane, the schedule before the threshold; n = that threshold for both kernels)
        P.group_start = ad ? kGroupStartAD : kGroupStartC;
        if (const char *e = std::getenv("PSDR_GROUP_START")) P.group_start = std::max(1, std::min(64, std::atoi(e)));
        if (lanes_out) { P.begin = lane_b; P.end = lane_e; P.shard_rank = 0; P.shard_count = 1; P.n_local = local_lanes(P.end - P.begin, 0, 1); }
        if (P.n_local > 0) {
            if (fork) P.counter = q_int; else if (next_queue(sc, st, P.counter)) return 1;
#define K_INTERIOR_AD(C) LAUNCH_PATHS(C, true, COUNT, 0, lean, sc, P.n_local, st, sc->blob.as<float4>(), T, cam, P, ctr)
#define K_INTERIOR_C(C) LAUNCH_PATHS(C, false, COUNT, 0, lean, sc, P.n_local, st, sc->blob.as<float4>(), T, cam, P, ctr)
            if (ad) LAUNCH_CLS_FWD(cls, K_INTERIOR_AD); else LAUNCH_CLS_FWD(cls, K_INTERIOR_C);
#undef K_INTERIOR_AD
#undef K_INTERIOR_C
#if PSDR_DIAG == 13
            if (!COUNT) {      // the census of paths.h: one line per interior launch (development builds; the call waits for the kernel)
                Counters h;
                HIPCHK(hipMemcpyAsync(&h, ctr, sizeof(h), hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
                std::fprintf(stderr, "psdr census: ad %d G %d depth %d starts %llu started %llu bodies %llu busy %llu\n", (int) ad, P.group_start, P.max_depth, h.rays, h.nodes, h.tris, h.hits);
            }
#endif
        }
    }
    if (ad && (!a->pix_ids || batch_edges) && !lanes_out) {
        // the edge samplers run over the FULL frame, with or without a pixel list (integrator.cpp:68-90)
        const long long npx_e = (long long) T.width * T.height;
        const bool want_prim = (terms & PSDR_TERM_PRIMARY) && T.sppe > 0 && cam.n_edges > 0, want_sec = (terms & PSDR_TERM_SECONDARY) && T.sppse > 0 && sc->E.n > 0;
        float *edge_out = dout;
        int *slot_of = nullptr;
        if (batch_edges && (want_prim || want_sec)) {
            if (batch_edge_scratch(sc, a, st, slot_of, edge_out)) return 1;
            T_prim.slot_of = slot_of; T_sec.slot_of = slot_of;
        }
        if (want_prim) {
            PathParams P = sampler_params<PathParams>(a, s, 1, npx_e * T.sppe, kBlock);
            P.dout = edge_out; P.dsq = dsq;
            P.skip_static = a->skip_static_edges;
            if (P.n_local > 0) {
                if (fork) P.counter = q_prim; else if (next_queue(sc, st, P.counter)) return 1;
#define K_PRIMARY(C) LAUNCH_PATHS(C, false, COUNT, 1, lean, sc, P.n_local, s_prim, sc->blob.as<float4>(), T_prim, cam, P, ctr)
                LAUNCH_CLS_FWD(cls, K_PRIMARY);
#undef K_PRIMARY
#if PSDR_DIAG == 14
                if (!COUNT) {      // the census of the side switch (paths.h): one line per primary-edge launch (development builds; the call waits for the kernel)
                    Counters h;
                    HIPCHK(hipMemcpyAsync(&h, ctr, sizeof(h), hipMemcpyDeviceToHost, s_prim));
                    HIPCHK(hipStreamSynchronize(s_prim));
                    std::fprintf(stderr, "psdr census: edge samples %llu early %llu detour %llu bodies %llu depth %d\n", h.rays, h.nodes, h.hits, h.tris, P.max_depth);
                }
#endif
            }
        }
        if (want_sec) {
            // (the term exists with field_mode == 0 only, where `cls` is the scene's own class: LDS blob, lean BVH, LDS blob with materials, global)
            PathParams P = sampler_params<PathParams>(a, s, 2, npx_e * T.sppse, kBlock);
            P.dout = edge_out; P.dsq = dsq;
            const GuidingDev G = a->guiding ? a->guiding->G : GuidingDev{};
            const int use_g = a->guiding ? 1 : 0;
            if (P.n_local > 0) {
                if (fork) P.counter = q_sec; else if (next_queue(sc, st, P.counter)) return 1;
#define K_SECONDARY(C) LAUNCH(C, (k_secondary_edges<C, CLS_COUNTED(C, COUNT), false>), sc, P.n_local, s_sec, sc->blob.as<float4>(), T_sec, sc->E, cam, P, G, use_g, ctr)
#define K_SECONDARY_SQ(C) LAUNCH(C, (k_secondary_edges<C, false, false, true>), sc, P.n_local, s_sec, sc->blob.as<float4>(), T_sec, sc->E, cam, P, G, use_g, ctr)
                if (dsq) LAUNCH_CLS_FWD(cls, K_SECONDARY_SQ); else LAUNCH_CLS_FWD(cls, K_SECONDARY);
#undef K_SECONDARY_SQ
#undef K_SECONDARY
            }
        }
        if (slot_of != nullptr)
            hipLaunchKernelGGL(k_batch_gather, dim3((a->n_pix + 255) / 256), dim3(256), 0, st, a->pix_ids, a->n_pix, (int) npx_e, (const int *) slot_of, (const float *) edge_out, dout);
    }
    if (fork) {
        HIPCHK(hipEventRecord(sc->ev_join[0], sc->aux[0]));
        HIPCHK(hipEventRecord(sc->ev_join[1], sc->aux[1]));
        HIPCHK(hipStreamWaitEvent(st, sc->ev_join[0], 0));
        HIPCHK(hipStreamWaitEvent(st, sc->ev_join[1], 0));
    }
    HIPCHK(hipGetLastError());
    if (COUNT && counters) {
        Counters h;
        HIPCHK(hipMemcpyAsync(&h, ctr, sizeof(h), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        counters->rays = h.rays; counters->nodes_visited = h.nodes; counters->tris_tested = h.tris; counters->shaded_hits = h.hits;
    }
    return 0;
}

extern "C" {

int psdr_hip_render_c(const psdr_hip_scene *sc, const psdr_render_args *a, float *out, void *stream) {
    if (!out) return fail("null output");
    return render_impl<false>(sc, a, false, out, nullptr, nullptr, 0, 0, nullptr, stream);
}
int psdr_hip_render_d_fwd(const psdr_hip_scene *sc, const psdr_render_args *a, float *out, float *dout, void *stream) {
    if (!out || !dout) return fail("null output");
    return render_impl<false>(sc, a, true, out, dout, nullptr, 0, 0, nullptr, stream);
}
int psdr_hip_render_d_fwd_batch(const psdr_hip_scene *sc, const psdr_render_args *a, float *out, float *dout, void *stream) {
    if (!out || !dout) return fail("null output");
    return render_impl<false>(sc, a, true, out, dout, nullptr, 0, 0, nullptr, stream, true);
}
int psdr_hip_render_c_sq(const psdr_hip_scene *sc, const psdr_render_args *a, float *out, float *out_sq, void *stream) {
    if (!sc || !a) return fail("null argument");
    if (!out || !out_sq) return fail("null output");
    return render_impl<false>(sc, a, false, out, nullptr, nullptr, 0, 0, nullptr, stream, false, out_sq, nullptr);
}
int psdr_hip_render_d_fwd_sq(const psdr_hip_scene *sc, const psdr_render_args *a, float *out, float *dout, float *out_sq, float *out_dsq, void *stream) {
    if (!sc || !a) return fail("null argument");
    if (!out || !dout || !out_sq || !out_dsq) return fail("null output");
    return render_impl<false>(sc, a, true, out, dout, nullptr, 0, 0, nullptr, stream, false, out_sq, out_dsq);
}
int psdr_hip_render_c_counted(const psdr_hip_scene *sc, const psdr_render_args *a, float *out, psdr_counters *c, void *stream) {
    if (!out) return fail("null output");
    return render_impl<true>(sc, a, false, out, nullptr, nullptr, 0, 0, c, stream);
}
int psdr_hip_render_d_fwd_counted(const psdr_hip_scene *sc, const psdr_render_args *a, float *out, float *dout, psdr_counters *c, void *stream) {
    if (!out || !dout) return fail("null output");
    return render_impl<true>(sc, a, true, out, dout, nullptr, 0, 0, c, stream);
}
int psdr_hip_li_lanes(const psdr_hip_scene *sc, const psdr_render_args *a, int64_t lane_begin, int64_t lane_end, float *out, void *stream) {
    if (!out || lane_end <= lane_begin) return fail("bad lane range");
    return render_impl<false>(sc, a, false, nullptr, nullptr, out, lane_begin, lane_end, nullptr, stream);
}

int64_t psdr_hip_scene_adjoint_record_bytes(const psdr_hip_scene *sc) {
    if (!sc) return 0;
    std::lock_guard<std::mutex> lk(sc->mu);
    return (int64_t) sc->adj_rec_bytes;
}

int psdr_hip_scene_tex_layout(const psdr_hip_scene *sc, int64_t *offsets, int64_t *total) {
    if (!sc) return fail("null scene");
    if (total) *total = sc->tex_total;
    if (offsets)
        for (int i = 0; i < 3 * sc->T.n_bsdfs; ++i) offsets[i] = (size_t) i < sc->tex_layout.size() ? sc->tex_layout[i] : -1;
    return 0;
}

static int render_bwd_impl(const psdr_hip_scene *sc, const psdr_render_args *a, const float *d_rgb, const psdr_grads *g, void *stream, bool batch_edges) {
    CallShape s;
    if (call_shape(sc, a, true, false, batch_edges, "psdr_hip_render_d_bwd", s)) return 1;
    if (!d_rgb || !g || !g->g_triangles || !g->g_bsdf || !g->g_emitter) return fail("null gradient buffer");
    SCRATCH_GUARD(sc, stream);
    // batch rendering (integrator.cpp:139-176): d_rgb is [n_pix*3]; the edge terms of a pixel list only with batch_edges (as in the forward path)
    const SceneTables &T = sc->T;
    hipStream_t st = (hipStream_t) stream;
    const long long npx_full = (long long) T.width * T.height;
    const long long npx = a->pix_ids ? a->n_pix : npx_full;
    const int terms = s.terms, cls = s.cls;
    SensorDev cam = sc->sensors[a->sensor_id];
    for (int i = 0; i < 16; ++i) { cam.d_to_world.m[i] = 0.f; cam.d_world_to_sample.m[i] = 0.f; }     // probes only
    if (a->zero_output) {
        HIPCHK(hipMemsetAsync(g->g_triangles, 0, sizeof(float) * 22 * (size_t) T.n_tris, st));
        HIPCHK(hipMemsetAsync(g->g_bsdf, 0, sizeof(float) * 3 * (size_t) std::max(1, T.n_bsdfs), st));
        HIPCHK(hipMemsetAsync(g->g_emitter, 0, sizeof(float) * 3 * (size_t) std::max(1, T.n_emitters), st));
        if (g->g_tex && sc->tex_total > 0) HIPCHK(hipMemsetAsync(g->g_tex, 0, sizeof(float) * (size_t) sc->tex_total, st));
        if (g->g_camera) HIPCHK(hipMemsetAsync(g->g_camera, 0, sizeof(float) * 16, st));
        if (g->g_env && T.env_emitter >= 0) HIPCHK(hipMemsetAsync(g->g_env, 0, sizeof(float) * 3 * (size_t) T.env.width * T.env.height, st));
        if (g->g_env_scale) HIPCHK(hipMemsetAsync(g->g_env_scale, 0, sizeof(float), st));
        if (g->g_env_from_world) HIPCHK(hipMemsetAsync(g->g_env_from_world, 0, sizeof(float) * 16, st));
        if (g->g_mat) HIPCHK(hipMemsetAsync(g->g_mat, 0, sizeof(float) * kMatOut * (size_t) std::max(1, T.n_bsdfs), st));
        if (g->g_uv_xf) HIPCHK(hipMemsetAsync(g->g_uv_xf, 0, sizeof(float) * 4 * (3 * (size_t) T.n_bsdfs + 1), st));
        if (g->g_sec_edges && sc->E.n > 0) HIPCHK(hipMemsetAsync(g->g_sec_edges, 0, sizeof(float) * 6 * (size_t) sc->E.n, st));
        if (g->g_prim_edges && cam.n_edges > 0) HIPCHK(hipMemsetAsync(g->g_prim_edges, 0, sizeof(float) * 4 * (size_t) cam.n_edges, st));
    }
    const bool with_lookups = T.tex != nullptr || T.pv != nullptr || T.env_emitter >= 0;
    // PSDR_ADJ_GLOBAL=1: run the interior adjoint of an LDS-class scene from global memory (no blob copy in LDS: more workgroups per CU)
#ifdef PSDR_DEV_KNOBS
    static const bool adj_global = std::getenv("PSDR_ADJ_GLOBAL") != nullptr;
#else
    constexpr bool adj_global = false;
#endif
    const int adj_cls = (cls == 1 && adj_global) ? 2 : cls;
    SceneTables Ta = T;
    Ta.stack_depth -= adj_cold_rows(T);
    const int adj_depth = s.depth;
    // Diffuse BSDFs + area lights / an environment map under PathTracer: the reverse sweep (adjoint.h); everything else: record and probe
    const bool no_sweep = std::getenv("PSDR_ADJ_PROBE") != nullptr;                // measurement / test knob, read per call: force the probe form
    const bool sweep = !no_sweep && adj_cls != 0 && a->field_mode == 0 && T.tex == nullptr && T.pv == nullptr && (T.env_emitter < 0 || adj_cls == 2);
    // GGX scenes (class 0): the material sweep, when every BSDF is Diffuse or a constant-parameter Microfacet
    // ... and the first-hit integrators on such scenes (the sweep's camera-hit block with the integrator's own adjoint; field 0 and 7 are constants)
    // the record-and-probe form fills g_uv_xf only while it visits a bitmap / environment lookup for g_tex / g_env: a caller that wants the uv-transform adjoints
    // without those buffers would get zeros from this form and numbers from the sweeps - refuse instead
    if (g->g_uv_xf && (no_sweep || a->field_mode == 0) && !sweep) {
        const bool sweep_mat_ = !no_sweep && adj_cls == 0 && sc->simple_mats;
        if (!sweep_mat_ && ((sc->tex_total > 0 && !g->g_tex) || (T.env_emitter >= 0 && !g->g_env)))
            return fail("g_uv_xf in the record-and-probe form needs g_tex (BSDF bitmaps) / g_env (environment map) beside it");
    }
    const bool sweep_mat = !no_sweep && !sweep && adj_cls == 0 && sc->simple_mats && (a->field_mode > 0 || T.mat != nullptr || T.tex != nullptr || T.pv != nullptr || sc->has_nmap);
    // the LDS behind the traversal rows - where the per-lane records live, how many hot triangle rows fit, a small environment map's texels: adj_layout.h
    AdjPlanIn pin;
    pin.smem_base = smem_for_adjoint(sc, adj_cls);
    pin.depth = adj_depth; pin.with_lookups = with_lookups; pin.form = sweep ? kAdjSweep : (sweep_mat ? kAdjSweepMat : kAdjProbe);
    pin.n_bsdfs = T.n_bsdfs; pin.n_emitters = T.n_emitters; pin.n_hot = sc->n_hot;
    pin.env_texels = T.env_emitter >= 0 ? (size_t) T.env.width * T.env.height : 0;
    pin.want_env = T.env_emitter >= 0 && g->g_env != nullptr; pin.want_uv_xf = g->g_uv_xf != nullptr; pin.rec_lds_knob = PSDR_ADJ_REC_LDS;
    const AdjPlan plan = adj_plan(pin);
    if (plan.error) return fail(plan.error);
    if (!sc->adj_attr_set) {         // (per scene = per device and context; a process-wide flag would skip the second device)
#define LDS_160K(kernel) HIPCHK(hipFuncSetAttribute((const void *) kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) kAdjLdsCap))
        IF_CLS1(LDS_160K(k_interior_adjoint<1>));
        IF_CLS0(LDS_160K(k_interior_adjoint<0>));
        IF_CLS0(LDS_160K(k_interior_adjoint_mat<0>));
        IF_CLS2(LDS_160K(k_interior_adjoint<2>));
        IF_CLS1(LDS_160K((k_secondary_edges<1, false, true>)));
        IF_CLS0(LDS_160K((k_secondary_edges<0, false, true>)));
        IF_CLS2(LDS_160K((k_secondary_edges<2, false, true>)));
#undef LDS_160K
        sc->adj_attr_set = true;
    }
    if ((terms & PSDR_TERM_INTERIOR) && T.spp > 0) {
        AdjointParams P = sampler_params<AdjointParams>(a, s, 0, npx * T.spp, a->pix_ids ? (long long) T.spp : (long long) T.width * T.spp);
        P.pix_ids = a->pix_ids;
        P.w = d_rgb; P.g_tri = g->g_triangles; P.g_bsdf = g->g_bsdf; P.g_emitter = g->g_emitter; P.hot_map = sc->hot_map.as<int>(); P.hot_inv = sc->hot_inv.as<int>(); P.n_hot = plan.n_hot_used;
        P.mesh_filter = g->mesh_filter; P.skip_bsdf = g->skip_bsdf; P.skip_emitter = g->skip_emitter;
        P.g_tex = sc->tex_total > 0 ? g->g_tex : nullptr;
#ifdef PSDR_SWEEP_DUMP
        P.g_tex = g->g_tex;        // (diagnostic build: the sweep's per-lane dump goes there)
#endif
        P.g_cam = g->g_camera;
        P.g_mat = sc->T.mat != nullptr ? g->g_mat : nullptr;
        P.g_env_xf = sc->T.env_emitter >= 0 ? g->g_env_from_world : nullptr;
        P.g_uv_xf = g->g_uv_xf;
        P.g_env = sc->T.env_emitter >= 0 ? g->g_env : nullptr; P.g_env_scale = sc->T.env_emitter >= 0 ? g->g_env_scale : nullptr;
        if (P.n_local > 0) {
            if (next_queue(sc, st, P.counter)) return 1;
            const int grid = grid_for(sc, P.n_local);
            P.hit_words = adj_hit_words(adj_depth); P.ext_words = adj_ext_words(adj_depth); P.lk_words = with_lookups ? 3 * adj_lk_entries(adj_depth) : 0;
            P.sweep = pin.form;
            if (sweep || sweep_mat) { P.hit_words = plan.lane_words; P.ext_words = 0; P.lk_words = 0; }
            P.env_lds = plan.env_lds;
            P.rec_global = nullptr;
            if (!plan.rec_in_lds) {
                const size_t need = sizeof(float) * (size_t) grid * (size_t) plan.lane_words * kBlock;
                if (need > sc->adj_rec_bytes) {
                    // (every earlier user of the records was ordered before this stream by the guard: its completion is this stream's)
                    if (sc->adj_rec.p) { HIPCHK(hipStreamSynchronize(st)); HIPCHK(hipFree(sc->adj_rec.p)); sc->adj_rec.p = nullptr; sc->adj_rec_bytes = 0; }
                    if (sc->adj_rec.clear_on(need, st)) return 1;          // (on the caller's stream: a clear on the null stream is not ordered before the kernel below)
                    sc->adj_rec_bytes = need;
                }
                P.rec_global = (float *) sc->adj_rec.p;
            }
#define K_ADJOINT(C) LAUNCH_SM((k_interior_adjoint<C>), sc, P.n_local, plan.smem, st, sc->blob.as<float4>(), Ta, cam, P)
            if (sweep_mat) ON_CLS(0, LAUNCH_SM((k_interior_adjoint_mat<0>), sc, P.n_local, plan.smem, st, sc->blob.as<float4>(), Ta, cam, P));       // (class 0 only: adj_cls == 0 here)
            else LAUNCH_CLS_REV(adj_cls, K_ADJOINT);
#undef K_ADJOINT
        }
    }
    const bool want_prim = (!a->pix_ids || batch_edges) && (terms & PSDR_TERM_PRIMARY) && T.sppe > 0 && cam.n_edges > 0;
    const bool want_sec = (!a->pix_ids || batch_edges) && (terms & PSDR_TERM_SECONDARY) && T.sppse > 0 && sc->E.n > 0;
    // a pixel list: the edge samples read their adjoint at the representative slot of their pixel (k_batch_reduce), the others are dropped
    const float *edge_w = d_rgb;
    SceneTables Tp = T;
    if (batch_edges && (want_prim || want_sec)) {
        int *slot_of = nullptr;
        float *rows = nullptr;
        if (batch_edge_scratch(sc, a, st, slot_of, rows)) return 1;
        hipLaunchKernelGGL(k_batch_reduce, dim3((a->n_pix + 255) / 256), dim3(256), 0, st, a->pix_ids, a->n_pix, (int) npx_full, (const int *) slot_of, d_rgb, rows);
        Tp.slot_of = slot_of; Ta.slot_of = slot_of; edge_w = rows;
    }
    if (want_prim) {
        if (!g->g_prim_edges) return fail("g_prim_edges is required when the primary-edge term is requested");
        PathParams P = sampler_params<PathParams>(a, s, 1, npx_full * T.sppe, kBlock);
        P.adj_w = edge_w; P.g_prim = g->g_prim_edges; P.n_prim = cam.n_edges; P.lds_acc = prim_adj_lds_floats(cam.n_edges) > 0 ? 1 : 0;
        P.prim_filter = g->prim_edge_filter;
        if (P.n_local > 0) {
            if (next_queue(sc, st, P.counter)) return 1;
            const size_t sm = smem_for(sc, cls) + adj_lds_bytes(prim_adj_lds_floats(cam.n_edges));
#define K_PRIMARY_ADJ(C) LAUNCH_SM((k_paths<false, C, false, 1, kGeneral>), sc, P.n_local, sm, st, sc->blob.as<float4>(), Tp, cam, P, (Counters *) nullptr)
            LAUNCH_CLS_REV(cls, K_PRIMARY_ADJ);
#undef K_PRIMARY_ADJ
        }
    }
    if (want_sec) {
        if (!g->g_sec_edges) return fail("g_sec_edges is required when the secondary-edge term is requested");
        // (the term exists with field_mode == 0 only, where `cls` is the scene's own class: the lean instantiation on BVH scenes, as the forward pass)
        PathParams P = sampler_params<PathParams>(a, s, 2, npx_full * T.sppse, kBlock);
        P.adj_w = edge_w; P.g_sec = g->g_sec_edges; P.g_tri = g->g_triangles; P.n_sec = sc->E.n;
        P.g_cam = g->g_camera;
        P.sec_closed = no_sweep ? 0 : 1;
        // both tables in LDS, or - too large - the hot triangle rows (closed form only): adj_layout.h
        const SecAdjPlan sp = sec_adj_plan(sc->E.n, T.n_tris, sc->n_hot, P.sec_closed != 0, PSDR_SEC_HOT_MAX);
        P.lds_acc = sp.lds_acc; P.n_hot = sp.n_hot;
        P.hot_map = sc->hot_map.as<int>(); P.hot_inv = sc->hot_inv.as<int>();
        const size_t smem_sec = smem_for_adjoint(sc, sc->lds ? 1 : 0) + sp.bytes;
        const GuidingDev G = a->guiding ? a->guiding->G : GuidingDev{};
        const int use_g = a->guiding ? 1 : 0;
        if (P.n_local > 0) {
            if (next_queue(sc, st, P.counter)) return 1;
#define K_SECONDARY_ADJ(C) LAUNCH_SM((k_secondary_edges<C, false, true>), sc, P.n_local, smem_sec, st, sc->blob.as<float4>(), Ta, sc->E, cam, P, G, use_g, (Counters *) nullptr)
            LAUNCH_CLS_REV(cls, K_SECONDARY_ADJ);
#undef K_SECONDARY_ADJ
        }
    }
    HIPCHK(hipGetLastError());
    return 0;
}

int psdr_hip_render_d_bwd(const psdr_hip_scene *sc, const psdr_render_args *a, const float *d_rgb, const psdr_grads *g, void *stream) {
    return render_bwd_impl(sc, a, d_rgb, g, stream, false);
}
int psdr_hip_render_d_bwd_batch(const psdr_hip_scene *sc, const psdr_render_args *a, const float *d_rgb, const psdr_grads *g, void *stream) {
    return render_bwd_impl(sc, a, d_rgb, g, stream, true);
}

static int trace_impl(const psdr_hip_scene *sc, int32_t n, const float *o, const float *d, int32_t *out_tri, float *out_uv, float *out_t, void *stream, int pairs) {
    if (!sc) return fail("null scene");
    if (n <= 0) return 0;
    SCRATCH_GUARD(sc, stream);
    LAUNCH_RAYS(k_trace, sc, (long long) n, stream, sc->blob.as<float4>(), sc->T, n, o, d, out_tri, out_uv, out_t, pairs);
    HIPCHK(hipGetLastError());
    return 0;
}
int psdr_hip_env_sample(const psdr_hip_scene *sc, int32_t n, const float *ref_p, const float *s2, float *out_p, float *out_n, float *out_pdf, void *stream) {
    if (!sc) return fail("null scene");
    if (sc->T.env_emitter < 0) return fail("the scene has no EnvironmentMap");
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_env_sample, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t) stream, sc->T, n, ref_p, s2, out_p, out_n, out_pdf);
    HIPCHK(hipGetLastError());
    return 0;
}
int psdr_hip_env_pdf(const psdr_hip_scene *sc, int32_t n, const float *ref_p, const float *p, const float *nrm, float *out_pdf, void *stream) {
    if (!sc) return fail("null scene");
    if (sc->T.env_emitter < 0) return fail("the scene has no EnvironmentMap");
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_env_pdf, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t) stream, sc->T, n, ref_p, p, nrm, out_pdf);
    HIPCHK(hipGetLastError());
    return 0;
}
// cell masses of the environment map's sampling distribution: one thread per cell, the same envmath.h::cell_mass the host half's
// test hook evaluates (bit-equal); 2 M cells of a 1024 x 512 map take ~0.1 ms instead of 80 ms on the host cores
__global__ void k_env_cell_mass(const float *__restrict__ texels, int W, int H, int w2, int h2, int n, float *__restrict__ mass, env::UvXf<float> xf) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) mass[i] = env::cell_mass(texels, W, H, w2, h2, i, xf);
}
int psdr_hip_env_cell_masses(const float *texels, int32_t width, int32_t height, float *mass) {
    return psdr_hip_env_cell_masses_xf(texels, width, height, nullptr, mass);
}
int psdr_hip_env_cell_masses_xf(const float *texels, int32_t width, int32_t height, const float *uv_xf, float *mass) {
    if (!texels || !mass) return fail("null texel / mass buffer");
    if (width < 2 || height < 2) return fail("EnvironmentMap: the bitmap needs at least 2 x 2 texels");
    const int w2 = (width - 1) << 1, h2 = (height - 1) << 1;
    const long long n = (long long) w2 * h2;
    if (n > 0x7fffffffll) return fail("EnvironmentMap: too many cells");
    DevBuf tex, out;
    if (tex.upload(texels, sizeof(float) * 3 * (size_t) width * height) || out.upload(nullptr, sizeof(float) * (size_t) n)) return 1;
    hipLaunchKernelGGL(k_env_cell_mass, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, (hipStream_t) nullptr, tex.as<float>(), width, height, w2, h2, (int) n, (float *) out.p, uv_xf ? env::UvXf<float>(uv_xf) : env::UvXf<float>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(mass, out.p, sizeof(float) * (size_t) n, hipMemcpyDeviceToHost));
    return 0;
}
int psdr_hip_ray_intersect(const psdr_hip_scene *sc, int32_t n, const float *o, const float *d, float *out, void *stream) {
    if (!sc) return fail("null scene");
    if (n <= 0) return 0;
    if (!o || !d || !out) return fail("null ray / output buffer");
    SCRATCH_GUARD(sc, stream);
    LAUNCH_RAYS(k_intersect, sc, (long long) n, stream, sc->blob.as<float4>(), sc->T, n, o, d, out);
    HIPCHK(hipGetLastError());
    return 0;
}
// Scene::ray_intersect<true, false> (reference src/scene/scene.cpp:774-797, Scene.unit_ray_intersectAD at src/psdr.cpp:405): isect_ad.h
int psdr_hip_ray_intersect_ad(const psdr_hip_scene *sc, int32_t n, const float *o, const float *d, const float *d_o, const float *d_d,
                              float *out, float *out_d, int32_t *out_hit, void *stream) {
    if (!sc) return fail("null scene");
    if (n <= 0) return 0;
    if (!o || !d || !out || !out_hit) return fail("null ray / output buffer");
    SCRATCH_GUARD(sc, stream);
    LAUNCH_RAYS(k_intersect_ad, sc, (long long) n, stream, sc->blob.as<float4>(), sc->T, n, o, d, d_o, d_d, out, out_d, out_hit);
    HIPCHK(hipGetLastError());
    return 0;
}
// the transpose of psdr_hip_ray_intersect_ad (the reference gets it by drjit::backward through the same re-intersection)
int psdr_hip_ray_intersect_adj(const psdr_hip_scene *sc, int32_t n, const float *o, const float *d, const int32_t *hit, const float *g_rec,
                               const uint8_t *mesh_filter, float *g_triangles, float *g_o, float *g_d, void *stream) {
    if (!sc) return fail("null scene");
    if (n <= 0) return 0;
    if (!o || !d || !hit || !g_rec) return fail("null ray / hit / adjoint buffer");
    SCRATCH_GUARD(sc, stream);
    // measurement knob, read per call: wave reductions per 64 rays before per-lane atomics (0 = per-lane atomics only)
    int rounds = PSDR_ISECT_ADJ_ROUNDS;
    if (const char *e = std::getenv("PSDR_ISECT_ADJ_ROUNDS")) rounds = std::max(0, std::min(64, std::atoi(e)));
    // (no traversal: the blob alone in LDS, no stack rows)
    if (sc->lds) LAUNCH_SM((k_intersect_adj<1>), sc, n, (size_t) sc->T.blob_words * 16, stream, sc->blob.as<float4>(), sc->T, n, o, d, hit, g_rec, mesh_filter, g_triangles, g_o, g_d, rounds);
    else LAUNCH_SM((k_intersect_adj<0>), sc, n, 0, stream, sc->blob.as<float4>(), sc->T, n, o, d, hit, g_rec, mesh_filter, g_triangles, g_o, g_d, rounds);
    HIPCHK(hipGetLastError());
    return 0;
}
int psdr_hip_trace(const psdr_hip_scene *sc, int32_t n, const float *o, const float *d, int32_t *out_tri, float *out_uv, float *out_t, void *stream) {
    return trace_impl(sc, n, o, d, out_tri, out_uv, out_t, stream, 0);
}
int psdr_hip_trace_pairs(const psdr_hip_scene *sc, int32_t n, const float *o, const float *d, int32_t *out_tri, float *out_uv, float *out_t, void *stream) {
    return trace_impl(sc, n, o, d, out_tri, out_uv, out_t, stream, 1);
}

int psdr_hip_guiding_build(const psdr_hip_scene *sc, int32_t sensor_id, int32_t max_depth, const int32_t reso[4], int32_t nrounds, int32_t seed,
                           psdr_hip_guiding **out, void *stream) {
    (void) max_depth;
    if (!sc || !out || !reso) return fail("null argument");
    if (nrounds <= 0) return fail("nrounds > 0");
    if (sensor_id < 0 || sensor_id >= (int) sc->sensors.size()) return fail("Invalid sensor id!");
    if (sc->E.n <= 0) return fail("Scene needs to be configured with sppse > 0!");
    const long long cells = (long long) reso[0] * reso[1] * reso[2];
    if (cells <= 0 || reso[3] <= 0 || cells * reso[3] > 2147483647LL) return fail("bad guiding resolution");
    auto g = std::make_unique<psdr_hip_guiding>();
    GuidingDev &G = g->G;
    for (int k = 0; k < 3; ++k) { G.reso[k] = reso[k]; G.unit[k] = 1.f / (float) reso[k]; }
    G.num_cells = (int) cells;
    SCRATCH_GUARD(sc, stream);
    hipStream_t st = (hipStream_t) stream;
    DevBuf mass;
    if (mass.clear_on(sizeof(float) * cells, st)) return 1;        // (on the caller's stream, as the rounds that add into it)
    const long long nl = cells * reso[3];
    for (int r = 0; r < nrounds; ++r)
        LAUNCH_RAYS(k_guiding_round, sc, nl, st, sc->blob.as<float4>(), sc->T, sc->E, sc->sensors[sensor_id], G, reso[3], seed, r, (float *) mass.p);
    HIPCHK(hipGetLastError());
    g->mass.resize(cells);
    HIPCHK(hipMemcpyAsync(g->mass.data(), mass.p, sizeof(float) * cells, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // DiscreteDistribution::init on the host (double-precision CDF, reference pmf.h:12-38)
    std::vector<float> cmf(cells);
    float sum = 0.f; double acc = 0.0;
    for (long long i = 0; i < cells; ++i) {
        if (nrounds > 1) g->mass[i] /= (float) nrounds;
        sum += g->mass[i]; acc += (double) g->mass[i]; cmf[i] = (float) acc;
    }
    G.sum = sum;
    // the tables go out on the caller's stream; the call returns after they have arrived (cmf and guide are locals), usable on any stream
    if (g->pmf.upload_on(g->mass.data(), sizeof(float) * cells, st) || g->cmf.upload_on(cmf.data(), sizeof(float) * cells, st)) return 1;
    G.pmf = g->pmf.as<float>(); G.cmf = g->cmf.as<float>();
    {
        std::vector<int> guide;
        build_cdf_guide(cmf.data(), (int) cells, sum, guide);
        G.guide = nullptr; G.guide_n = 0;
        if (!guide.empty()) {
            if (g->guide.upload_on(guide.data(), guide.size() * sizeof(int), st)) return 1;
            G.guide = g->guide.as<int>(); G.guide_n = (int) guide.size() - 1;
        }
        HIPCHK(hipStreamSynchronize(st));
    }
    *out = g.release();
    return 0;
}
int psdr_hip_guiding_num_cells(const psdr_hip_guiding *g) { return g ? g->G.num_cells : 0; }
int psdr_hip_guiding_mass(const psdr_hip_guiding *g, float *out_host, int32_t cap) {
    if (!g || !out_host) return fail("null argument");
    if (cap < g->G.num_cells) return fail("buffer too small");
    std::memcpy(out_host, g->mass.data(), sizeof(float) * g->G.num_cells);
    return 0;
}
int psdr_hip_guiding_destroy(psdr_hip_guiding *g) { delete g; return 0; }

uint64_t psdr_hip_tea64(uint64_t v0, uint64_t v1) { return tea64(v0, v1); }
int psdr_hip_sampler_floats(uint64_t seed_value, uint64_t lane, uint64_t skip, int32_t n, float *out_dev, void *stream) {
    hipLaunchKernelGGL(k_sampler_floats, dim3(1), dim3(64), 0, (hipStream_t) stream, seed_value, lane, skip, n, out_dev);
    HIPCHK(hipGetLastError());
    return 0;
}

} // extern "C"
