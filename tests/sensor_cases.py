"""The three-sensor scenes shared by tests/test_sensors_cpu.py (the preconditions, on the oracle) and tests/test_gpu_sensors.py (the product against the
oracle): one per scene class the renderer treats differently - 'cbox' (36 triangles: brute force, live-pixel masks), 'sphere' (652 triangles: BVH),
'envmap' (the tutorial spheres under an environment map: BVH, lean configure, no masks, a bounding cube that depends on every camera position) and
'ortho' (the unit-scale box seen by an orthographic, a perspective and another orthographic camera)."""
import numpy as np

import scenes

FAMILIES = ("cbox", "sphere", "envmap", "ortho")
SPP = {"cbox": 8, "sphere": 4, "envmap": 4, "ortho": 8}
DEPTH = 2
W = H = 40


def family_spec(family, moving=True):
    """moving=True: the family's usual geometry tangent (a mesh translated along x); False: no tangent at all"""
    n = SPP[family]
    if family == "cbox":
        spec = scenes.cbox_scene(W, H, n, n, n, param="box_x" if moving else None)
    elif family == "sphere":
        spec = scenes.sphere_scene(W, H, n, n, n)
        if not moving:
            for m in spec.meshes:
                m.d_to_world_left = np.zeros((4, 4), np.float32)
    elif family == "envmap":
        spec = scenes.envmap_scene(W, H, n, n, n, param="box_x" if moving else None, balls=True)
    elif family == "ortho":
        spec = scenes.ortho_cbox_scene(W, H, n, n, n, param="box_x" if moving else None)
        if moving:
            # the luminaire moves with the box: through an OrthographicCamera the box alone has an exactly zero secondary-edge term at this size,
            # and the luminaire alone an exactly zero primary-edge term (none of its edges is a silhouette from below)
            spec.meshes[0].d_to_world_left = spec.meshes[1].d_to_world_left.copy()
    else:
        raise ValueError(family)
    return scenes.with_extra_sensors(spec, "ortho" if family == "ortho" else "perspective")


def camera_tangent_spec(family, camera):
    """nothing moves but camera `camera`, along its x: to_world_left = T(100 P, 0, 0) (0.3 P at the orthographic scene's unit scale, as in scenes.ortho_cbox_scene)"""
    spec = family_spec(family, moving=False)
    dT = np.zeros((4, 4), np.float32)
    dT[0, 3] = 0.3 if family == "ortho" else 100.0
    spec.cameras[camera].d_to_world_left = dT
    return spec
