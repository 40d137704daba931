"""Scenes of more than 32 geometries for the tests of the G-buffer and of the scene-size classes (csrc/ff_kernels.hip
scene_size_class: up to 32 records, up to 128, more): the C2 box filled up to an exact record count, with the records on either side
of each class boundary placed where the camera sees them, and the two crowds the rest of the suite renders.  Test infrastructure."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fuzz_parity as fz  # noqa: E402
from gpupathtracer_amd import lib, scenes  # noqa: E402
from gpupathtracer_amd import types as T  # noqa: E402
from gbuffer_ref import surface_colour  # noqa: E402
from oracle_lib import load_oracle  # noqa: E402

W, H = 64, 48
COUNTS = (32, 33, 128, 129)
BOUNDARY = (31, 32, 127, 128)  # the last record of a class and the first of the next; a scene's last record n - 1 joins them
BOX_RECORDS = 8  # scenes.cornell_wahoo_scene: the wahoo, the cube, five walls and the emitter

# The shelf: a row of places 0.9 in front of the camera, below its axis.  Nothing else comes nearer to the camera than z = 1.0.
SHELF_Z, SHELF_Y = 1.5, -0.22
SHELF_X = (-0.42, -0.14, 0.14, 0.42, 0.0)
SHELF_KINDS = ("cube", "sphere", "quad", "quad", "cube")  # by place: record 31, 32, 127, 128, and a last record that is none of them
FILL_Z = (-2.2, 0.9)


def camera(w=W, h=H):
    """The C2 camera, inside the open front of the box."""
    return scenes.posed_camera(w, h, position=(0.0, 0.0, 2.4), yaw=-90.0, pitch=0.0)


def crowd_camera(w=W, h=H):
    """The fixed pose tests/test_gpu_fuzz.py renders its crowds from."""
    return scenes.posed_camera(w, h, position=(0.5, 0.2, 4.5), yaw=-95.0, pitch=-4.0)


def shelf_indices(n):
    """The hand-placed records of counted_scene(n), in shelf order."""
    return sorted({i for i in BOUNDARY + (n - 1,) if BOX_RECORDS <= i < n})


def _material(k, rng):
    """Materials in a cycle of six: three diffuse with albedos of their own, a mirror, a glass and a dim emitter."""
    col = tuple(float(v) for v in rng.uniform(0.25, 0.95, 3))
    k %= 6
    if k in (0, 2, 4):
        return scenes.make_bxdf(T.BXDF_DIFFUSE, albedo=col)
    if k == 1:
        return scenes.make_bxdf(T.BXDF_MIRROR, specular=col)
    if k == 3:
        return scenes.make_bxdf(T.BXDF_GLASS, specular=(1, 1, 1), transmittance=col, ior=float(rng.uniform(1.2, 1.8)))
    return scenes.make_bxdf(T.BXDF_EMITTER, emissive=col, intensity=0.3)


def _add(s, kind, pos, rot, size, bxdf):
    if kind == "cube":
        s.add_mesh(fz.meshes()["cube"], pos, rot, size, bxdf)
    elif kind == "sphere":
        s.add_sphere(0.5, pos, rot, size, bxdf)  # (radius 0.5: `size` is the extent along each object axis, as for the cube)
    else:
        s.add_plane(pos, rot, size, bxdf)


def _counted(n, seed):
    if n < BOX_RECORDS + 1:
        raise ValueError("the box alone has 8 records")
    rng = np.random.default_rng(1000 + seed)
    s = scenes.Scene()
    s.add_mesh(scenes.load_mesh("wahoo"), (0, -2.4, 0), (0, 0, 0), (0.28, 0.28, 0.28), scenes.make_bxdf(T.BXDF_DIFFUSE, albedo=(1, 0, 0)))
    s.add_mesh(fz.meshes()["cube"], (1.5, -2.0, 1.0), (0, 0, 0), (1, 1, 1), scenes.make_bxdf(T.BXDF_DIFFUSE, albedo=(0.75, 0.75, 0.75)))
    scenes._box(s)
    assert len(s) == BOX_RECORDS
    shelf = shelf_indices(n)
    for i in range(BOX_RECORDS, n):
        # (every record draws the same numbers whether it ends up on the shelf or not: a scene of n + 1 records is this one plus one)
        kind = ("cube", "sphere", "quad")[int(rng.integers(0, 3))]
        pos = (float(rng.uniform(-2.1, 2.1)), float(rng.uniform(-2.2, 2.0)), float(rng.uniform(*FILL_Z)))
        rot = tuple(float(v) for v in rng.uniform(-180, 180, 3))
        size = tuple(float(v) for v in rng.uniform(0.18, 0.42, 3))
        bxdf = _material(i, rng)
        if i in shelf:
            place = BOUNDARY.index(i) if i in BOUNDARY else len(BOUNDARY)
            kind = SHELF_KINDS[place]
            pos = (SHELF_X[place], SHELF_Y, SHELF_Z)
            rot = {"cube": (20.0, 30.0, 10.0), "sphere": (0.0, 0.0, 35.0), "quad": (0.0, 15.0, 25.0)}[kind]
            size = {"cube": (0.12, 0.16, 0.1), "sphere": (0.14, 0.2, 0.16), "quad": (0.2, 0.14, 1.0)}[kind]
            # the quads carry a texture in one test, which wants a diffuse surface; the others keep the cycle's material
            if kind == "quad" or bxdf.m_type == T.BXDF_EMITTER:
                bxdf = scenes.make_bxdf(T.BXDF_DIFFUSE, albedo=(0.3 + 0.1 * place, 0.9 - 0.15 * place, 0.5))
        _add(s, kind, pos, rot, size, bxdf)
    return s


def counted_scene(n, seed=0):
    """The C2 box (records 0-7) and n - 8 small cubes, spheres and quads at seeded places inside it, rotated and unevenly scaled,
    their materials in a cycle of diffuse, mirror, glass and a dim emitter.  Records 31, 32, 127, 128 and n - 1, where the scene has
    them, stand on a shelf in front of camera() with nothing before them: a cube, a sphere and two quads, in that order."""
    s = _counted(n, seed).finalize()
    assert len(s) == n
    return s


def moved_scene(n, seed=0, others=20):
    """counted_scene(n, seed) with the shelf records and `others` seeded records of the fill moved, turned and rescaled (the box
    stays): the same geometries in the same order, for update_transforms."""
    s = _counted(n, seed)
    rng = np.random.default_rng(5000 + seed)
    shelf = shelf_indices(n)
    rest = [i for i in range(BOX_RECORDS, n) if i not in shelf]
    picked = sorted(int(i) for i in rng.choice(rest, size=min(others, len(rest)), replace=False))
    for i in shelf + picked:
        kind, pos, rot, scl, payload, bxdf = s._specs[i]
        d = rng.uniform(-0.08, 0.08, 3) if i in shelf else rng.uniform(-0.4, 0.4, 3)
        if i in shelf:
            d[2] = abs(d[2])  # (towards the camera: still nothing before them)
        pos = tuple(float(np.clip(p + v, -2.2, 2.2)) for p, v in zip(pos, d))
        if i not in shelf:
            pos = pos[:2] + (min(pos[2], FILL_Z[1]),)
        rot = tuple(float(r + v) for r, v in zip(rot, rng.uniform(-40, 40, 3)))
        scl = tuple(float(c * v) for c, v in zip(scl, rng.uniform(0.7, 1.4, 3)))
        s._specs[i] = (kind, pos, rot, scl, payload, bxdf)
    s.finalize()
    assert len(s) == n
    return s, shelf, picked


def crowd_scene(crowd):
    """The crowd of `crowd` small things around one or two meshes that tests/test_gpu_fuzz.py and tests/test_gpu_kernel_names.py
    upload (80: records in LDS behind the tree over the geometries; 500: records in global memory)."""
    return fz.rand_scene(np.random.default_rng(3), small=True, crowd=crowd)


SCENES = {"n32": (lambda: counted_scene(32), camera), "n33": (lambda: counted_scene(33), camera), "n128": (lambda: counted_scene(128), camera),
          "n129": (lambda: counted_scene(129), camera), "crowd80": (lambda: crowd_scene(80), crowd_camera),
          "crowd500": (lambda: crowd_scene(500), crowd_camera)}


def oracle_gbuffer_jittered(scene, cam, params, jx, jy):
    """gbuffer_ref.oracle_gbuffer with ff_camera_ray_matrix_jittered(cam, jx, jy) as the ray matrix (the arithmetic of
    tests/test_gpu_jitter.py, for any frame size)."""
    lib_o = load_oracle()
    w, h = params.width, params.height
    mat = (C.c_float * 16)(*lib.camera_ray_matrix_jittered(cam, jx, jy).m[:])
    out = {"depth": np.zeros((h, w), np.float32), "position": np.zeros((h, w, 3), np.float32), "normal": np.zeros((h, w, 3), np.float32),
           "albedo": np.zeros((h, w, 3), np.float32), "ids": np.full((h, w, 3), -1, np.int32)}
    colours = [surface_colour(scene.geometries[i]) for i in range(len(scene))]
    ray, isect = T.FfRay(), T.FfIntersect()
    for y in range(h):
        for x in range(w):
            lib_o.orc_primary_ray(mat, C.byref(cam), x, y, C.byref(ray))
            lib_o.orc_intersect_rays(C.byref(ray), scene.geometries, len(scene), C.byref(isect))
            if not isect.m_hit:
                continue
            out["depth"][y, x] = isect.m_t
            out["position"][y, x] = isect.m_intersectionPoint.tuple()
            out["normal"][y, x] = isect.m_normal.tuple()
            col, kind = colours[isect.geometryIndex]
            out["albedo"][y, x] = col
            out["ids"][y, x] = (isect.geometryIndex, isect.triangleIndex, kind)
    return out


def visible_figures(ids, placed=()):
    """What the conditions on a scene are stated in: the share of pixels that hit, the distinct visible geometry indices, the bxdf
    types in view and the pixel count of each index in `placed`."""
    geom = ids[..., 0]
    seen = np.unique(geom[geom >= 0])
    return {"hit_share": float((geom >= 0).mean()), "visible": [int(v) for v in seen],
            "pixels": {i: int((geom == i).sum()) for i in placed}, "kinds": sorted(int(v) for v in np.unique(ids[..., 2][geom >= 0]))}
