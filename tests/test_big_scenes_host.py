"""The conditions on the scenes of tests/big_scenes.py, checked with the CPU oracle alone: the GPU tests of the scene-size classes
compare G-buffers bit for bit, which says something only where the camera sees the records on either side of each class boundary."""
import functools

import numpy as np
import pytest

import big_scenes as B
from gpupathtracer_amd import lib
from gpupathtracer_amd import types as T
from gbuffer_ref import oracle_gbuffer


@functools.lru_cache(maxsize=None)
def _figures(name):
    scene_fn, cam_fn = B.SCENES[name]
    scene = scene_fn()
    gb = oracle_gbuffer(scene, cam_fn(), lib.render_params(B.W, B.H))
    f = B.visible_figures(gb["ids"], B.shelf_indices(len(scene)) if name.startswith("n") else ())
    print(f"{name}: {len(scene)} records, hit share {f['hit_share']:.3f}, {len(f['visible'])} visible indices "
          f"({sum(v >= 32 for v in f['visible'])} of 32 and above, {sum(v >= 128 for v in f['visible'])} of 128 and above), "
          f"pixels of the hand-placed {f['pixels']}, bxdf types {f['kinds']}\n  visible: {f['visible']}")
    return len(scene), f


@pytest.mark.parametrize("n", B.COUNTS)
def test_counted_scene_has_its_count_and_shows_its_boundary_records(n):
    count, f = _figures(f"n{n}")
    assert count == n
    assert f["hit_share"] >= 0.5
    want = [i for i in (31, 32, 127, 128, n - 1) if i < n]
    assert sorted(set(want)) == B.shelf_indices(n)
    for i in want:
        assert f["pixels"][i] >= 4, (i, f["pixels"])
    if n >= 128:
        assert sum(v >= 32 for v in f["visible"]) >= 10
    assert {T.BXDF_MIRROR, T.BXDF_GLASS, T.BXDF_DIFFUSE} <= set(f["kinds"])


def test_shelf_records_are_a_cube_a_sphere_and_quads():
    scene = B.counted_scene(129)
    kinds = [scene.geometries[i].m_geometryType for i in B.shelf_indices(129)]
    assert kinds == [T.GEOM_TRIANGLEMESH, T.GEOM_SPHERE, T.GEOM_PLANE, T.GEOM_PLANE]
    assert scene.geometries[128].m_bxdf.contents.m_type == T.BXDF_DIFFUSE  # (an albedo texture binds to diffuse surfaces only)


def test_counted_scenes_are_prefixes_of_each_other_but_for_the_shelf():
    """Record i is the same in every counted scene that has it, unless it is the last record of one of them (then it is on the
    shelf there): what differs between 32 and 33, or 128 and 129, is the count."""
    a, b = B.counted_scene(128), B.counted_scene(129)
    for i in range(127):
        assert bytes(a.geometries[i].m_modelMatrix) == bytes(b.geometries[i].m_modelMatrix), i
    assert bytes(a.geometries[127].m_modelMatrix) == bytes(b.geometries[127].m_modelMatrix)  # (on the shelf in both)


def test_moved_scene_moves_the_shelf_and_twenty_others():
    base = B.counted_scene(129)
    moved, shelf, picked = B.moved_scene(129)
    assert len(moved) == 129 and shelf == [31, 32, 127, 128] and len(picked) == 20 and not set(picked) & set(shelf)
    changed = [i for i in range(129) if bytes(base.geometries[i].m_modelMatrix) != bytes(moved.geometries[i].m_modelMatrix)]
    assert changed == sorted(shelf + picked)
    assert min(picked) >= B.BOX_RECORDS
    for i in range(129):
        assert base.geometries[i].m_geometryType == moved.geometries[i].m_geometryType
    # the moved shelf is still in view, elsewhere
    cam, params = B.camera(), lib.render_params(B.W, B.H)
    before, after = oracle_gbuffer(base, cam, params)["ids"][..., 0], oracle_gbuffer(moved, cam, params)["ids"][..., 0]
    for i in shelf:
        assert (after == i).sum() >= 4 and not np.array_equal(after == i, before == i), i


@pytest.mark.parametrize("crowd", [80, 500])
def test_crowds_show_many_records(crowd):
    count, f = _figures(f"crowd{crowd}")
    assert (32 < count <= 128) if crowd == 80 else count > 128
    assert len(f["visible"]) >= 20
    if crowd == 500:
        assert max(f["visible"]) >= 128
