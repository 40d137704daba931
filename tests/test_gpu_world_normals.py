"""Normal tables (csrc/ff_frame_kernels.hip world_normals_kernel; csrc/ff_k_shade.h unit_world_normal; csrc/ff_k_traverse.h
finish_segment<WN>; csrc/ff_kernels.hip trace_bvh_kernel<..., WN>; csrc/ff_scene_api.cpp finalize_layout): the unit world normal of every
triangle and plane is computed once, where the scene changes, by the function the shading pass calls, and the diffuse small-scene
kernels fetch it with the winner's record instead of computing it per hit.  Nothing a frame computes may change: every case compares
radiance bits, rgb8 bytes and the ray counters of three renderings -
  on:    the default (the kernels on the tables);
  off:   FF_NO_WORLD_NORMALS=1, the kernels that compute the normal in the shading pass (same reported name: the tables do not show in it);
  brute: FF_TRACE_BRUTE_FORCE, the reference's loop, which computes every normal where it shades.  It traces every segment, so its
         rays_answered and rays_cut_short are zero by construction (asserted): rays_traced is compared across all three, the other two
         between on and off.
Both diffuse small-scene kernels are covered: the one on start records (the default at 8 spp) and, under FF_NO_START_RECORDS=1, the one
that starts every sample from the pixel's raw stored hit (whose normal is the object-space one: that kernel looks the table up).
Frames are 32 x 24, 4 bounces, 8 spp."""
import numpy as np
import pytest

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T

pytestmark = pytest.mark.gpu

W, H = 32, 24
INSIDE = dict(position=(0.0, 0.0, 2.4), yaw=-90.0, pitch=0.0)
GREY = dict(albedo=(0.75, 0.75, 0.75))


def _frame(t, cam, params, repeat=1):
    for _ in range(repeat):
        rgb8, rad = t.render(cam, params)
    st = t.stats()
    return rgb8.tobytes(), rad.view(np.int32).copy(), int(st.rays_traced), int(st.rays_answered), int(st.rays_cut_short), t.kernel_name()


def _three(tracer, monkeypatch, cam, params, repeat=1):
    """The frame with the switch on, off and from the brute-force loop: equal bits, bytes and counters.  repeat: render it that many
    times in a row and compare the last one (the stored hits are kept from the first to the next)."""
    monkeypatch.delenv("FF_NO_WORLD_NORMALS", raising=False)
    tracer.reload_switches()
    on = _frame(tracer, cam, params, repeat)
    monkeypatch.setenv("FF_NO_WORLD_NORMALS", "1")
    tracer.reload_switches()
    off = _frame(tracer, cam, params, repeat)
    monkeypatch.delenv("FF_NO_WORLD_NORMALS")
    tracer.reload_switches()
    assert on[5] == off[5], (on[5], off[5])
    assert on[2:5] == off[2:5], (on[2:5], off[2:5])
    assert on[0] == off[0] and np.array_equal(on[1], off[1])
    params.trace_mode = T.TRACE_BRUTE_FORCE
    brute = _frame(tracer, cam, params)
    params.trace_mode = T.TRACE_BVH
    assert brute[2] == on[2] and brute[3] == 0 and brute[4] == 0, (on[2:5], brute[2:5])
    assert on[0] == brute[0] and np.array_equal(on[1], brute[1])
    return on, off


def _boxed(*meshes, planes=()):
    """The C2 box around the given meshes (triangles, position, rotation, scale) and extra planes (position, rotation, scale)."""
    s = scenes.Scene()
    for tris, pos, rot, scl in meshes:
        s.add_mesh(tris, pos, rot, scl, scenes.make_bxdf(T.BXDF_DIFFUSE, **GREY))
    scenes._box(s)
    for pos, rot, scl in planes:
        s.add_plane(pos, rot, scl, scenes.make_bxdf(T.BXDF_DIFFUSE, albedo=(0.2, 0.4, 0.9)))
    return s.finalize()


def _cube_with_zero_area_triangle():
    """cube.obj plus one triangle with two equal vertices, in front of the cube's camera-side face."""
    cube = scenes.load_mesh("cube")
    extra = np.zeros((1, 24), dtype=np.float32)
    extra[0, 0:9] = (-0.3, -0.3, 0.7, -0.3, -0.3, 0.7, 0.3, 0.3, 0.7)
    return np.concatenate([cube, extra], axis=0)


def _scene(name):
    cube = scenes.load_mesh("cube")
    if name == "c2":
        return scenes.cornell_wahoo_scene()
    if name == "nonuniform":  # (the inverse-transpose is not the rotation)
        return _boxed((cube, (0.2, -1.2, 0.3), (25, 35, 10), (1.7, 0.4, 1.1)))
    if name == "mirrored":  # (negative determinant)
        return _boxed((cube, (-0.4, -1.4, 0.2), (10, 20, 0), (-1.2, 0.8, 1.0)), (scenes.load_mesh("wahoo"), (0.9, -2.4, 0.0), (0, -30, 0), (0.25, -0.25, 0.25)))
    if name == "zero_area":
        return _boxed((_cube_with_zero_area_triangle(), (0.0, -1.5, 0.0), (0, 30, 0), (1.3, 1.3, 1.3)))
    if name == "oblique_plane":  # (both of its sides are lit and seen: paths reach it from either)
        return _boxed((cube, (1.3, -2.0, 0.6), (0, 15, 0), (1, 1, 1)), planes=[((-0.3, -0.6, -0.2), (35, 20, 15), (2.0, 1.2, 1.0))])
    raise KeyError(name)


@pytest.mark.parametrize("start_records", [True, False])
@pytest.mark.parametrize("name", ["c2", "nonuniform", "mirrored", "zero_area", "oblique_plane"])
def test_frames_with_and_without_the_tables(tracer, monkeypatch, name, start_records):
    if not start_records:
        monkeypatch.setenv("FF_NO_START_RECORDS", "1")
    tracer.upload_scene(_scene(name))
    cam = scenes.posed_camera(W, H, **INSIDE)
    on, off = _three(tracer, monkeypatch, cam, lib.render_params(W, H, 4, 8, 21))
    assert on[5].endswith(", false, 0, false, true>") == start_records, on[5]
    assert on[1].view(np.float32).max() > 0  # (paths reach the emitter)


def test_a_one_sample_frame_on_kept_hits(tracer, monkeypatch):
    """2 bounces, 1 spp, rendered twice: the second frame starts from the hits the first one stored."""
    tracer.upload_scene(scenes.cornell_wahoo_scene())
    cam = scenes.posed_camera(W, H, **INSIDE)
    on, off = _three(tracer, monkeypatch, cam, lib.render_params(W, H, 2, 1, 5), repeat=2)
    assert on[3] >= W * H and off[3] == on[3]  # (both kernels: every pixel's primary segment answered from what was kept)


def test_every_scene_change_rebuilds_the_tables(monkeypatch):
    """A transform update (rotation and a non-uniform scale: every normal of the mesh moves), then a mesh update (sheared vertices:
    the triangles' own normals move).  After each, the frame equals that of a fresh Tracer that uploaded the changed scene, and the
    brute-force frame.  The same sequence with the switch off gives the same frames and counters."""
    wahoo, cube = scenes.load_mesh("wahoo"), scenes.load_mesh("cube")
    sheared = wahoo.copy()
    for v in range(3):
        sheared[:, 3 * v] = (wahoo[:, 3 * v] + np.float32(0.35) * wahoo[:, 3 * v + 1]).astype(np.float32)
        sheared[:, 3 * v + 2] = (wahoo[:, 3 * v + 2] * np.float32(0.6)).astype(np.float32)
    cube_at = (cube, (1.5, -2.0, 1.0), (0, 0, 0), (1, 1, 1))
    first = _boxed((wahoo, (0, -2.4, 0), (0, 0, 0), (0.28, 0.28, 0.28)), cube_at)
    moved_at = ((0.3, -2.4, 0.2), (10, 40, 5), (0.4, 0.22, 0.3))
    moved = _boxed((wahoo, *moved_at), cube_at)
    reshaped = _boxed((sheared, *moved_at), cube_at)
    cam = scenes.posed_camera(W, H, **INSIDE)
    p = lib.render_params(W, H, 4, 8, 9)

    def fresh(scene):
        with lib.Tracer(0) as t:
            t.upload_scene(scene)
            bvh = _frame(t, cam, p)
            p.trace_mode = T.TRACE_BRUTE_FORCE
            brute = _frame(t, cam, p)
            p.trace_mode = T.TRACE_BVH
        assert bvh[0] == brute[0] and np.array_equal(bvh[1], brute[1]) and bvh[2] == brute[2]
        return bvh

    def updated():
        with lib.Tracer(0) as t:
            t.upload_scene(first)
            out = [_frame(t, cam, p)]
            t.update_transforms(moved)
            out.append(_frame(t, cam, p))
            t.update_mesh(0, sheared, T.UPDATE_REFIT)
            out.append(_frame(t, cam, p))
        return out

    monkeypatch.setenv("FF_NO_WORLD_NORMALS", "1")
    frames_off = updated()
    monkeypatch.delenv("FF_NO_WORLD_NORMALS")
    frames = updated()
    for got, got_off, scene in zip(frames, frames_off, (first, moved, reshaped)):
        want = fresh(scene)
        assert got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2:5] == want[2:5]
        assert got[0] == got_off[0] and np.array_equal(got[1], got_off[1]) and got[2:] == got_off[2:]
    assert not np.array_equal(frames[0][1], frames[1][1]) and not np.array_equal(frames[1][1], frames[2][1])
