"""Reverse mode of renderD on the host, in three statements: the LAYOUT of the configured snapshot as psdr_grads sees it (row counts, object -> row maps, the
shape of every adjoint buffer), the PLAN of one backward() (one route per leaf; the buffers, filters, skip flags and terms of the launch follow from the routes) and
the GATHER from the filled buffers to the leaves' gradients.  Nothing here touches the device: _RenderDFn.backward allocates and launches in between."""
import collections
import types

import numpy as _np
import torch as _torch

from . import _psdr_core as _core
from . import chain

GEO_NAMES = ("vertex_positions", "to_world_left", "to_world", "to_world_right")
UV_SUFFIX = "@uv"
# the three bitmap / per-vertex slots of a BSDF (psdr_hip_scene_tex_layout, psdr_grads.g_uv_xf): parameter name -> slot
SLOT = {"reflectance": 0, "diffuseReflectance": 0, "specularReflectance": 1, "roughness": 2, "normal_map": 0,
        "eta": 0, "k": 1, "alpha_u": 2, "alpha_v": 2}
# constant parameters of the GGX BSDFs: (offset, length) inside the BSDF's 16-float row of psdr_grads.g_mat
MAT_ROWS = {"MicrofacetBSDF": {"specularReflectance": (0, 3), "roughness": (3, 1)},
            "RoughConductorBSDF": {"alpha_u": (0, 1), "alpha_v": (1, 1), "eta": (2, 3), "k": (5, 3), "specular_reflectance": (8, 3)},
            "RoughDielectricBSDF": {"alpha_u": (0, 1), "alpha_v": (1, 1), "eta": (2, 1)}}
# the five row buffers share one allocation (one all-reduce, one copy to the host); the others are reduced one by one, in this order
ROW_BUFFERS = ("g_triangles", "g_bsdf", "g_emitter", "g_sec_edges", "g_prim_edges")
EXTRA_BUFFERS = ("g_env", "g_env_scale", "g_mat", "g_env_from_world", "g_uv_xf", "g_camera", "g_tex")
SLICE, GEOMETRY, ENV_POSE, INTENSITY, ZEROS = "slice", "geometry", "env_pose", "intensity", "zeros"
# kind; buffer (psdr_grads field); offset and length in floats (GEOMETRY of a mesh: offset = its row of mesh_filter); fold: the slice is summed to one number
Route = collections.namedtuple("Route", "kind buffer offset length fold")


def uv_row(bsdf_row, slot):
    """row of psdr_grads.g_uv_xf: three per BSDF; the environment map's is the one behind the last BSDF's (bsdf_row = the number of BSDF rows, slot 0)"""
    return 3 * bsdf_row + slot


class Layout:
    """the configured snapshot as reverse mode sees it, through sensor `sensor_id`"""

    def __init__(self, scene, sensor_id=0):
        pm = scene.param_map
        self.scene, self.sensor_id = scene, sensor_id
        self.n_tris, self.n_sec = (int(x) for x in scene._snapshot_counts())
        cam = pm.get("Sensor[%d]" % sensor_id)
        # mesh of every primary edge of the sensor (None: the scene has no such sensor - unit_ray_intersectAD without a camera)
        self.edge_mesh = None if cam is None else _np.asarray(cam._primary_edge_ids(), dtype=_np.int64).reshape(-1, 3)[:, 0]
        self.n_prim = 0 if cam is None else int(self.edge_mesh.shape[0])
        self.n_own = sum(1 for k in pm if k.startswith("BSDF[") and not k.startswith("BSDF[id="))
        self.n_emitters = sum(1 for k in pm if k.startswith("Emitter[") and not k.startswith("Emitter[id="))
        self.n_meshes = int(scene.num_meshes)
        # id(object) -> row.  BSDFs: the scene's own in order, then the ones nested in normal maps (a map without a nested BSDF still owns its hidden row)
        self._alive = []                       # (the ids stay valid while the layout lives)
        self.bsdf_rows, self.emitter_rows, self.mesh_rows = {}, {}, {}
        own = [pm["BSDF[%d]" % k] for k in range(self.n_own)]
        maps = [b for b in own if isinstance(b, _core.NormalMapBSDF)]
        self.n_hidden = len(maps)
        self.n_bsdfs = self.n_own + self.n_hidden
        for rows, objs in ((self.bsdf_rows, own + [b._nested for b in maps]), (self.emitter_rows, [pm.get("Emitter[%d]" % k) for k in range(self.n_emitters)]),
                           (self.mesh_rows, [pm.get("Mesh[%d]" % k) for k in range(self.n_meshes)])):
            for row, obj in enumerate(objs):
                if obj is not None:
                    rows.setdefault(id(obj), row)
                    self._alive.append(obj)

    def bsdf_row(self, obj):
        if id(obj) not in self.bsdf_rows:
            raise RuntimeError("BSDF is not part of the scene")
        return self.bsdf_rows[id(obj)]

    def mesh_row(self, mesh):
        if id(mesh) not in self.mesh_rows:
            raise RuntimeError("mesh is not part of the scene")
        return self.mesh_rows[id(mesh)]

    def shapes(self, tex_total=0, env_texels=0):
        """shape of every float buffer of psdr_grads, by the field names of include/psdr_hip.h (g_tex: `tex_total` floats as psdr_hip_scene_tex_layout reports,
        g_env: the radiance image's `env_texels` floats)"""
        nb = max(1, self.n_bsdfs)
        return {"g_triangles": (self.n_tris, 22), "g_bsdf": (nb, 3), "g_emitter": (max(1, self.n_emitters), 3), "g_sec_edges": (max(1, self.n_sec), 6),
                "g_prim_edges": (max(1, self.n_prim), 4), "g_tex": (max(1, int(tex_total)),), "g_camera": (16,), "g_env": (int(env_texels),), "g_env_scale": (1,),
                "g_mat": (nb, 16), "g_env_from_world": (16,), "g_uv_xf": (uv_row(self.n_bsdfs, 0) + 1, 4)}


def _route(layout, integ, obj, name, t, tex):
    """the route of one leaf; `tex()` -> offsets of the texel layout"""
    fold = lambda buffer, offset, n: Route(SLICE, buffer, offset, n, t.numel() != n)          # a colour given as one number is the sum of its components
    if isinstance(obj, (_core.Mesh, _core.Sensor)):
        if name not in GEO_NAMES:
            return None
        return Route(GEOMETRY, "g_triangles", layout.mesh_row(obj), 0, False) if isinstance(obj, _core.Mesh) else Route(GEOMETRY, "g_camera", 0, 16, False)
    if isinstance(obj, _core.BSDF):
        if name.endswith(UV_SUFFIX):           # [rotate, scale, translate.x, translate.y] of one bitmap
            return Route(SLICE, "g_uv_xf", 4 * uv_row(layout.bsdf_row(obj), SLOT[name[:-len(UV_SUFFIX)]]), 4, False)
        if t.dim() >= 2 or isinstance(obj, _core.MicrofacetBSDFPerVertex):      # the leaf IS the texel / per-vertex array: its block of g_tex
            off = int(tex()[3 * layout.bsdf_row(obj) + SLOT[name]])
            return Route(ZEROS if off < 0 else SLICE, "g_tex", off, t.numel(), False)
        if name in ("reflectance", "diffuseReflectance"):
            return fold("g_bsdf", 3 * layout.bsdf_row(obj), 3)
        if name in MAT_ROWS.get(type(obj).__name__, {}):
            off, n = MAT_ROWS[type(obj).__name__][name]
            return fold("g_mat", 16 * layout.bsdf_row(obj) + off, n)
        return None
    if isinstance(obj, _core.EnvironmentMap):
        if name.endswith(UV_SUFFIX):
            return Route(SLICE, "g_uv_xf", 4 * uv_row(layout.n_bsdfs, 0), 4, False)
        if name in ("radiance", "scale"):
            return Route(SLICE, "g_env" if name == "radiance" else "g_env_scale", 0, t.numel(), False)
        return Route(ENV_POSE, "g_env_from_world", 0, 16, False)      # to_world_left: through the adjoint of from_world = (to_world_left . to_world_raw)^-1
    if isinstance(obj, _core.AreaLight) and name == "radiance" and id(obj) in layout.emitter_rows:
        return fold("g_emitter", 3 * layout.emitter_rows[id(obj)], 3)
    if obj is integ and name == "m_intensity":                         # CollocatedIntegrator.m_intensity: the image is linear in it
        return Route(INTENSITY, None, 0, 1, False)
    return None


def plan(layout, integ, leaves, needs, terms, tex_layout):
    """-> routes: one per leaf, None where no gradient is needed or exists; buffers: the fields of EXTRA_BUFFERS to allocate (tex_total / env_texels: the sizes of
    g_tex / g_env); mesh_filter, prim_edge_filter: host uint8 arrays (the latter None = every row); skip_bsdf, skip_emitter; terms: the terms to launch.
    `tex_layout()` -> (offsets, total) of the scene's texels; called only when a route needs g_tex or a BSDF's uv row"""
    from . import TERM_PRIMARY, _derivative_terms, _moves_edges       # (looked up per call: the package's own names)
    p = types.SimpleNamespace(layout=layout, leaves=leaves, tex=None)

    def tex():
        if p.tex is None:
            p.tex = tex_layout()
        return p.tex[0]
    p.routes = [_route(layout, integ, obj, name, t, tex) if need else None for (obj, name, t), need in zip(leaves, needs)]
    used, p.env_texels = set(), 0
    p.mesh_filter = _np.zeros(max(1, layout.n_meshes), dtype=_np.uint8)
    for (obj, name, t), r in zip(leaves, p.routes):
        if r is None:
            continue
        used.add(r.buffer)
        if r.kind == GEOMETRY and r.buffer == "g_triangles":
            p.mesh_filter[r.offset] = 1
        elif r.buffer == "g_env":
            p.env_texels = t.numel()
        elif r.buffer == "g_uv_xf" and isinstance(obj, _core.BSDF):
            tex()
            used.add("g_tex")                 # a BSDF bitmap's uv row is filled in the pass over its texels
        elif r.buffer in ("g_env_scale", "g_uv_xf"):
            used.add("g_env")                 # the scale adjoint is assembled from the texel probes, the map's uv row is filled beside them
            p.env_texels = p.env_texels or int(_np.prod(obj._get("radiance", False).shape))
    p.buffers = [b for b in EXTRA_BUFFERS if b in used]
    p.tex_total = int(p.tex[1]) if p.tex is not None else 0
    p.skip_bsdf, p.skip_emitter = "g_bsdf" not in used, "g_emitter" not in used
    # the boundary terms' adjoints are rows of edges (g_sec / g_prim): nobody reads them unless a mesh or the camera is differentiated
    p.terms = _derivative_terms(terms, leaves, {id(t) for (_o, _n, t), need in zip(leaves, needs) if need}) & 7
    # ... and the primary-edge samples add to the row of THEIR edge only: with some meshes differentiated and the camera (and the integrator) not, the samples
    # on the other meshes' edges are not traced (psdr_grads.prim_edge_filter)
    p.prim_edge_filter = None
    if (p.terms & TERM_PRIMARY) and layout.n_prim > 0 and not any(need and not isinstance(obj, _core.Mesh) and _moves_edges(obj, name) for (obj, name, t), need in zip(leaves, needs)):
        p.prim_edge_filter = _np.ascontiguousarray(p.mesh_filter[layout.edge_mesh])
    return p


def geometry_grads(layout, wanted, g_tri, g_sec, g_prim, g_camera):
    """wanted: [(index, object, name, leaf tensor)] of mesh / sensor leaves; g_*: float64 / float32 numpy rows -> {index: gradient}.  The per-triangle / per-edge part of
    the chain rule runs in the host core (Scene::chain_geometry through chain.native_geometry_grads: double arithmetic on host threads)"""
    if not wanted:
        return {}
    geo = chain.native_geometry_grads(layout.scene, layout.sensor_id, [(obj, name) for _i, obj, name, _t in wanted], g_tri, g_sec[:6 * layout.n_sec],
                                      g_prim[:4 * layout.n_prim], g_camera)
    return {i: _torch.as_tensor(_np.ascontiguousarray(geo[(id(obj), name)])).reshape(t.shape).to(t.device, t.dtype)
            for i, obj, name, t in wanted if (id(obj), name) in geo}


def gather(p, buffers, g_img, img):
    """buffers: {psdr_grads field: flat tensor} - the row buffers as their float64 host copy, the others as allocated -> the gradient of every leaf, None where no route"""
    grads = [None] * len(p.routes)
    geo = [(i, obj, name, t) for i, ((obj, name, t), r) in enumerate(zip(p.leaves, p.routes)) if r is not None and r.kind == GEOMETRY]
    g_cam = buffers["g_camera"].to("cpu", _torch.float64).numpy().reshape(4, 4) if "g_camera" in buffers else None
    for i, g in geometry_grads(p.layout, geo, *(buffers[b].numpy() for b in ("g_triangles", "g_sec_edges", "g_prim_edges")), g_cam).items():
        grads[i] = g
    for i, ((obj, name, t), r) in enumerate(zip(p.leaves, p.routes)):
        if r is None or r.kind == GEOMETRY:
            continue
        if r.kind == SLICE:
            row = buffers[r.buffer][r.offset:r.offset + r.length].to(_torch.float32)
            g = row.sum().reshape(1) if r.fold else row
        elif r.kind == ZEROS:                  # a slot without texels (psdr_hip_scene_tex_layout: offset -1)
            g = _torch.zeros_like(t)
        elif r.kind == INTENSITY:
            g = (g_img * img).sum() / t.detach().to(g_img.device).reshape(())
        else:                                  # ENV_POSE.  from_world = inverse(to_world_left . to_world_raw): d from = -from . d to . from
            with _torch.enable_grad():
                L = t.detach().to("cpu", _torch.float64).reshape(4, 4).clone().requires_grad_(True)
                raw = _torch.as_tensor(_np.asarray(obj._get("to_world_raw", False), dtype=_np.float64))
                (g,) = _torch.autograd.grad(_torch.linalg.inv(L @ raw), L, buffers[r.buffer].to("cpu", _torch.float64).reshape(4, 4))
        grads[i] = g.reshape(t.shape).to(t.device, t.dtype)
    return tuple(grads)
