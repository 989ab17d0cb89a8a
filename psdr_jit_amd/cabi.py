"""ctypes view of the C ABI in include/psdr_hip.h (libpsdr_hip.so), used by bench.py and the
parity tests to call the entry points directly with device pointers."""
import ctypes as C
import os

from . import build as _build

SYMBOLS = [
    "psdr_hip_last_error", "psdr_hip_abi_version", "psdr_hip_device_count", "psdr_hip_set_device",
    "psdr_hip_scene_create", "psdr_hip_scene_update", "psdr_hip_scene_last_update", "psdr_hip_scene_check_tree", "psdr_hip_scene_check_rows", "psdr_hip_scene_update_edges", "psdr_hip_scene_primary_edges", "psdr_hip_scene_check_edges", "psdr_hip_scene_edge_path", "psdr_hip_scene_destroy", "psdr_hip_scene_stats", "psdr_hip_scene_adjoint_record_bytes", "psdr_hip_scene_live_pixels", "psdr_hip_scene_camera_table", "psdr_hip_bvh_node_bytes", "psdr_hip_scene_tex_layout", "psdr_hip_trace", "psdr_hip_trace_pairs", "psdr_hip_ray_intersect", "psdr_hip_ray_intersect_ad", "psdr_hip_ray_intersect_adj", "psdr_hip_env_sample", "psdr_hip_env_pdf", "psdr_hip_env_cell_masses", "psdr_hip_env_cell_masses_xf",
    "psdr_hip_render_c", "psdr_hip_render_d_fwd", "psdr_hip_render_d_bwd", "psdr_hip_render_d_fwd_batch", "psdr_hip_render_d_bwd_batch", "psdr_hip_render_c_counted", "psdr_hip_render_d_fwd_counted", "psdr_hip_render_c_sq", "psdr_hip_render_d_fwd_sq",
    "psdr_hip_li_lanes", "psdr_hip_guiding_build", "psdr_hip_guiding_mass", "psdr_hip_guiding_num_cells",
    "psdr_hip_guiding_destroy", "psdr_hip_tea64", "psdr_hip_sampler_floats",
    "psdr_hip_precond_create", "psdr_hip_precond_destroy", "psdr_hip_precond_apply", "psdr_hip_precond_solve",
    "psdr_hip_adaptive_scratch_bytes", "psdr_hip_adaptive_bits", "psdr_hip_adaptive_counts", "psdr_hip_adaptive_expand", "psdr_hip_adaptive_merge", "psdr_hip_adaptive_merge_adj",
    "psdr_hip_denoise_create", "psdr_hip_denoise_apply", "psdr_hip_denoise_apply_adj", "psdr_hip_denoise_destroy",
    "psdr_hip_vdenoise_create", "psdr_hip_vdenoise_apply", "psdr_hip_vdenoise_frozen", "psdr_hip_vdenoise_frozen_adj", "psdr_hip_vdenoise_record", "psdr_hip_vdenoise_destroy",
    "psdr_hip_subdiv_create", "psdr_hip_subdiv_apply", "psdr_hip_subdiv_apply_adj", "psdr_hip_subdiv_destroy",
    "psdr_hip_msloss_create", "psdr_hip_msloss_eval", "psdr_hip_msloss_level", "psdr_hip_msloss_destroy",
    "psdr_hip_ssim_create", "psdr_hip_ssim_eval", "psdr_hip_ssim_map", "psdr_hip_ssim_destroy",
    "psdr_hip_meshreg_create", "psdr_hip_meshreg_eval", "psdr_hip_meshreg_destroy",
    "psdr_hip_chamfer_plan", "psdr_hip_chamfer_nearest", "psdr_hip_chamfer_eval",
    "psdr_hip_chamfer_grid_plan", "psdr_hip_chamfer_grid_build", "psdr_hip_chamfer_grid_nearest",
    "psdr_hip_pointmesh_plan", "psdr_hip_pointmesh_nearest", "psdr_hip_pointmesh_eval",
    "psdr_hip_sdf_winding", "psdr_hip_sdf_grad",
    "psdr_hip_mtet_plan", "psdr_hip_mtet_count", "psdr_hip_mtet_emit", "psdr_hip_mtet_vertices", "psdr_hip_mtet_vertices_adj",
    "psdr_hip_latreg_plan", "psdr_hip_latreg_eval",
]


class Sampler(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("skip", C.c_uint64)]


class RenderArgs(C.Structure):
    _fields_ = [("sensor_id", C.c_int32), ("max_depth", C.c_int32), ("hide_emitters", C.c_int32),
                ("samplers", Sampler * 3), ("pix_ids", C.c_void_p), ("n_pix", C.c_int32), ("terms", C.c_int32),
                ("shard_rank", C.c_int32), ("shard_count", C.c_int32), ("guiding", C.c_void_p), ("zero_output", C.c_int32), ("direct_mode", C.c_int32),
                ("field_mode", C.c_int32), ("field_object", C.c_int32), ("intensity", C.c_float), ("d_intensity", C.c_float), ("skip_static_edges", C.c_int32), ("shard_mode", C.c_int32)]


class Grads(C.Structure):
    _fields_ = [("g_triangles", C.c_void_p), ("g_bsdf", C.c_void_p), ("g_emitter", C.c_void_p), ("g_sec_edges", C.c_void_p),
                ("g_prim_edges", C.c_void_p), ("mesh_filter", C.c_void_p), ("skip_bsdf", C.c_int32), ("skip_emitter", C.c_int32),
                ("g_tex", C.c_void_p), ("g_camera", C.c_void_p), ("g_env", C.c_void_p), ("g_env_scale", C.c_void_p), ("g_mat", C.c_void_p), ("g_env_from_world", C.c_void_p), ("g_uv_xf", C.c_void_p),
                ("prim_edge_filter", C.c_void_p)]


class Counters(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("nodes_visited", C.c_uint64), ("tris_tested", C.c_uint64), ("shaded_hits", C.c_uint64)]


class UpdateInfo(C.Structure):      # psdr_update_info
    _fields_ = [("tree", C.c_int32), ("reallocated", C.c_int32), ("bytes_uploaded", C.c_int64), ("sah_cost", C.c_double), ("sah_cost_built", C.c_double),
                ("ms_tree", C.c_double), ("ms_fill", C.c_double), ("ms_upload", C.c_double), ("ms_total", C.c_double)]


class PrecondInfo(C.Structure):     # psdr_precond_info
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("launches", C.c_int32), ("rel_residual", C.c_float * 3)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_build.HIP_LIB):
            raise ImportError("libpsdr_hip.so is not built: run python -m psdr_jit_amd.build")
        L = C.CDLL(_build.HIP_LIB)
        L.psdr_hip_last_error.restype = C.c_char_p
        L.psdr_hip_tea64.restype = C.c_uint64
        L.psdr_hip_tea64.argtypes = [C.c_uint64, C.c_uint64]
        L.psdr_hip_sampler_floats.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p]
        L.psdr_hip_trace.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.psdr_hip_trace_pairs.argtypes = L.psdr_hip_trace.argtypes
        L.psdr_hip_ray_intersect_ad.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 8
        L.psdr_hip_ray_intersect_adj.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 9
        L.psdr_hip_env_sample.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 6
        L.psdr_hip_env_pdf.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 5
        L.psdr_hip_render_c.argtypes = [C.c_void_p, C.POINTER(RenderArgs), C.c_void_p, C.c_void_p]
        L.psdr_hip_render_d_fwd.argtypes = [C.c_void_p, C.POINTER(RenderArgs), C.c_void_p, C.c_void_p, C.c_void_p]
        L.psdr_hip_render_d_bwd.argtypes = [C.c_void_p, C.POINTER(RenderArgs), C.c_void_p, C.POINTER(Grads), C.c_void_p]
        L.psdr_hip_render_d_fwd_batch.argtypes = L.psdr_hip_render_d_fwd.argtypes
        L.psdr_hip_render_c_sq.argtypes = [C.c_void_p, C.POINTER(RenderArgs), C.c_void_p, C.c_void_p, C.c_void_p]
        L.psdr_hip_render_d_fwd_sq.argtypes = [C.c_void_p, C.POINTER(RenderArgs)] + [C.c_void_p] * 5
        L.psdr_hip_render_d_bwd_batch.argtypes = L.psdr_hip_render_d_bwd.argtypes
        L.psdr_hip_render_c_counted.argtypes = [C.c_void_p, C.POINTER(RenderArgs), C.c_void_p, C.POINTER(Counters), C.c_void_p]
        L.psdr_hip_render_d_fwd_counted.argtypes = [C.c_void_p, C.POINTER(RenderArgs), C.c_void_p, C.c_void_p, C.POINTER(Counters), C.c_void_p]
        L.psdr_hip_li_lanes.argtypes = [C.c_void_p, C.POINTER(RenderArgs), C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
        L.psdr_hip_scene_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.psdr_hip_scene_adjoint_record_bytes.restype = C.c_int64
        L.psdr_hip_scene_adjoint_record_bytes.argtypes = [C.c_void_p]
        L.psdr_hip_scene_last_update.argtypes = [C.c_void_p, C.POINTER(UpdateInfo)]
        L.psdr_hip_scene_check_tree.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.psdr_hip_scene_live_pixels.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_int64)]
        L.psdr_hip_scene_camera_table.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]
        L.psdr_hip_precond_create.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_float, C.POINTER(C.c_void_p), C.c_void_p]
        L.psdr_hip_precond_destroy.argtypes = [C.c_void_p]
        L.psdr_hip_precond_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.psdr_hip_precond_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int32, C.POINTER(PrecondInfo), C.c_void_p]
        L.psdr_hip_adaptive_scratch_bytes.restype = C.c_int64
        L.psdr_hip_adaptive_scratch_bytes.argtypes = []
        L.psdr_hip_adaptive_bits.argtypes = [C.c_int32, C.c_int64]
        L.psdr_hip_adaptive_counts.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.psdr_hip_adaptive_expand.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]
        L.psdr_hip_adaptive_merge.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_float, C.c_void_p, C.c_float, C.c_int32, C.c_void_p, C.c_void_p]
        L.psdr_hip_adaptive_merge_adj.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        L.psdr_hip_denoise_create.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.c_void_p]
        L.psdr_hip_denoise_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.psdr_hip_denoise_apply_adj.argtypes = L.psdr_hip_denoise_apply.argtypes
        L.psdr_hip_denoise_destroy.argtypes = [C.c_void_p]
        L.psdr_hip_vdenoise_create.argtypes = L.psdr_hip_denoise_create.argtypes
        L.psdr_hip_vdenoise_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_float), C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        L.psdr_hip_vdenoise_frozen.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.psdr_hip_vdenoise_frozen_adj.argtypes = L.psdr_hip_vdenoise_frozen.argtypes
        L.psdr_hip_vdenoise_record.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.psdr_hip_vdenoise_destroy.argtypes = [C.c_void_p]
        L.psdr_hip_subdiv_create.argtypes = [C.c_int32, C.c_int32] + [C.c_void_p] * 6 + [C.POINTER(C.c_void_p), C.c_void_p]
        L.psdr_hip_subdiv_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.psdr_hip_subdiv_apply_adj.argtypes = L.psdr_hip_subdiv_apply.argtypes
        L.psdr_hip_subdiv_destroy.argtypes = [C.c_void_p]
        L.psdr_hip_msloss_create.argtypes = [C.c_int32] * 4 + [C.POINTER(C.c_void_p), C.c_void_p]
        L.psdr_hip_msloss_eval.argtypes = [C.c_void_p] * 4 + [C.c_int32, C.c_int32, C.POINTER(C.c_float), C.c_void_p, C.c_void_p, C.c_void_p]
        L.psdr_hip_msloss_level.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.psdr_hip_msloss_destroy.argtypes = [C.c_void_p]
        L.psdr_hip_ssim_create.argtypes = [C.c_int32] * 4 + [C.POINTER(C.c_float), C.c_float, C.c_float, C.c_int32, C.POINTER(C.c_void_p), C.c_void_p]
        L.psdr_hip_ssim_eval.argtypes = [C.c_void_p] * 7
        L.psdr_hip_ssim_map.argtypes = [C.c_void_p] * 3
        L.psdr_hip_ssim_destroy.argtypes = [C.c_void_p]
        L.psdr_hip_meshreg_create.argtypes = [C.c_int32] * 3 + [C.c_void_p] * 10 + [C.POINTER(C.c_void_p), C.c_void_p]
        L.psdr_hip_meshreg_eval.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
        L.psdr_hip_meshreg_destroy.argtypes = [C.c_void_p]
        L.psdr_hip_chamfer_plan.argtypes = [C.c_int32, C.c_int32] + [C.POINTER(C.c_int32)] * 4
        L.psdr_hip_chamfer_nearest.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 4
        L.psdr_hip_chamfer_eval.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 8 + [C.POINTER(C.c_float), C.c_int32] + [C.c_void_p] * 5
        L.psdr_hip_chamfer_grid_plan.argtypes = [C.c_int32, C.c_int32] + [C.POINTER(C.c_int32)] * 2 + [C.POINTER(C.c_int64)] * 6 + [C.POINTER(C.c_int32)] * 4
        L.psdr_hip_chamfer_grid_build.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
        L.psdr_hip_chamfer_grid_nearest.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64] + [C.c_void_p] * 6
        L.psdr_hip_pointmesh_plan.argtypes = [C.c_int32, C.c_int32] + [C.POINTER(C.c_int32)] * 4
        L.psdr_hip_pointmesh_nearest.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 6
        L.psdr_hip_pointmesh_eval.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 12 + [C.POINTER(C.c_float), C.c_int32] + [C.c_void_p] * 6
        L.psdr_hip_sdf_winding.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 3
        L.psdr_hip_sdf_grad.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 12
        L.psdr_hip_mtet_plan.argtypes = [C.c_int32] * 3 + [C.POINTER(C.c_int32)] * 6
        L.psdr_hip_mtet_count.argtypes = [C.c_void_p] + [C.c_int32] * 3 + [C.c_void_p] * 7
        L.psdr_hip_mtet_emit.argtypes = [C.c_void_p] + [C.c_int32] * 3 + [C.c_void_p] * 3 + [C.c_int32] * 2 + [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
        L.psdr_hip_mtet_vertices.argtypes = [C.c_void_p] * 2 + [C.c_int32] * 3 + [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.psdr_hip_mtet_vertices_adj.argtypes = [C.c_void_p] * 2 + [C.c_int32] * 3 + [C.c_void_p] * 2 + [C.c_int32] + [C.c_void_p] * 4
        L.psdr_hip_latreg_plan.argtypes = [C.c_int32] * 3 + [C.POINTER(C.c_int32)] * 5
        L.psdr_hip_latreg_eval.argtypes = [C.c_void_p] + [C.c_int32] * 3 + [C.POINTER(C.c_double), C.POINTER(C.c_float), C.c_float] + [C.c_void_p] * 5
        _lib = L
    return _lib


def check(rc):
    if rc:
        raise RuntimeError(lib().psdr_hip_last_error().decode())


def make_args(sensor_id=0, max_depth=1, hide_emitters=False, seeds=(0, 0, 0), skips=(0, 0, 0), pix_ids_ptr=0, n_pix=0,
              terms=7, shard_rank=0, shard_count=1, guiding=None, zero_output=True, direct_mis=-1, field=-1, field_object=-1, intensity=1.0, d_intensity=0.0,
              skip_static_edges=False, shard_mode=0):
    a = RenderArgs()
    a.sensor_id, a.max_depth, a.hide_emitters = sensor_id, max_depth, int(hide_emitters)
    for k in range(3):
        a.samplers[k].seed, a.samplers[k].skip = int(seeds[k]), int(skips[k])
    a.pix_ids, a.n_pix, a.terms = pix_ids_ptr or None, n_pix, terms
    a.shard_rank, a.shard_count, a.guiding, a.zero_output = shard_rank, shard_count, guiding, int(zero_output)
    a.direct_mode = int(direct_mis) + 1
    a.field_mode, a.field_object, a.intensity, a.d_intensity = int(field) + 1, int(field_object), float(intensity), float(d_intensity)
    a.skip_static_edges = int(skip_static_edges)
    a.shard_mode = int(shard_mode)          # 0: interleaved 256-lane chunks, 1: contiguous runs (pixel-row tiles), include/psdr_hip.h
    return a
