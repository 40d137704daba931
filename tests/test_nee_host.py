"""FF_SHADE_DIFFUSE_PATH_NEE on the host: the light table (ff_light_table) against numpy, its exclusions, the alias table, the
Philox streams of tests/nee_ref.py against the oracle, and the parameter check.  Needs no GPU."""
import ctypes as C

import numpy as np
import pytest

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
import nee_ref


def model(scene, i):
    return np.array(scene.geometries[i].m_modelMatrix.m, np.float64).reshape(4, 4).T  # column-major storage


def lum_of(scene, i):
    b = scene.geometries[i].m_bxdf.contents
    e = np.array([b.m_emissiveColor.x, b.m_emissiveColor.y, b.m_emissiveColor.z], np.float32) * np.float32(b.m_intensity)
    return float(np.dot([0.2126, 0.7152, 0.0722], e.astype(np.float64)))


def numpy_table(scene):
    """The light table of ff_api.h in float64: list of (geometry, primitive, area, v0, e1, e2, normal, lum)."""
    out = []
    for i in range(len(scene)):
        g = scene.geometries[i]
        b = g.m_bxdf.contents
        if b.m_type != T.BXDF_EMITTER or lum_of(scene, i) <= 0.0:
            continue
        M = model(scene, i)
        if g.m_geometryType == T.GEOM_PLANE:
            nx, ny, nz = g.m_normal.x, g.m_normal.y, g.m_normal.z
            c0 = np.array([-0.5, -0.5, (0.5 * nx + 0.5 * ny) / nz, 1.0])
            a = np.array([1.0, 0.0, -nx / nz, 0.0])
            bb = np.array([0.0, 1.0, -ny / nz, 0.0])
            v0, e1, e2 = (M @ c0)[:3], (M @ a)[:3], (M @ bb)[:3]
            c = np.cross(e1, e2)
            out.append((i, -1, np.linalg.norm(c), v0, e1, e2, c / np.linalg.norm(c), lum_of(scene, i)))
        elif g.m_geometryType == T.GEOM_TRIANGLEMESH:
            tris = T.triangles_to_array(g.m_triangles, g.m_numberOfTriangles).astype(np.float64)
            for k, t in enumerate(tris):
                w = [(M @ np.append(t[3 * j:3 * j + 3], 1.0))[:3] for j in range(3)]
                e1, e2 = w[1] - w[0], w[2] - w[0]
                c = np.cross(e1, e2)
                out.append((i, k, 0.5 * np.linalg.norm(c), w[0], e1, e2, c / np.linalg.norm(c), lum_of(scene, i)))
    return out


def mixed_scene():
    """Every kind the table must handle: a rotated, non-uniformly scaled emitting plane, an emitting cube mesh, an emitting
    sphere (left out), a plane with zero emission (left out) and diffuse geometry (left out)."""
    s = scenes.Scene()
    s.add_plane((0.3, 1.1, -0.7), (35, 20, 70), (2.0, 0.5, 3.0), scenes.make_bxdf(T.BXDF_EMITTER, emissive=(1.0, 0.5, 0.25), intensity=3.0))
    s.add_mesh(scenes.load_mesh("cube"), (1.0, 0.5, 0.0), (10, 40, 5), (0.5, 0.3, 0.8), scenes.make_bxdf(T.BXDF_EMITTER, emissive=(0.2, 0.9, 0.4), intensity=1.5))
    s.add_sphere(0.5, (0, 0, 0), (0, 0, 0), (1, 1, 1), scenes.make_bxdf(T.BXDF_EMITTER, emissive=(1, 1, 1), intensity=5.0))
    s.add_plane((0, -1, 0), (90, 0, 0), (4, 4, 4), scenes.make_bxdf(T.BXDF_EMITTER, emissive=(0, 0, 0), intensity=2.0))
    s.add_plane((0, 0, -2), (0, 0, 0), (4, 4, 4), scenes.make_bxdf(T.BXDF_DIFFUSE, albedo=(0.5, 0.5, 0.5)))
    return s.finalize()


SCENES = {
    "C2": scenes.cornell_wahoo_scene,
    "C3": scenes.blooper_scene,
    "mixed": mixed_scene,
    "triangle_lights": nee_ref.triangle_light_scene,
}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_light_table_matches_numpy(ff, name):
    scene = SCENES[name]()
    entries, pdf = lib.light_table(scene)
    ref = numpy_table(scene)
    assert len(entries["area"]) == len(ref) > 0
    total = sum(a * l for (_, _, a, _, _, _, _, l) in ref)
    for k, (g, p, area, v0, e1, e2, nrm, lum) in enumerate(ref):
        assert entries["geometry"][k] == g and entries["primitive"][k] == p
        np.testing.assert_allclose(entries["area"][k], area, rtol=1e-6)
        np.testing.assert_allclose(entries["probability"][k], area * lum / total, rtol=1e-6)
        for got, want in ((entries["v0"][k], v0), (entries["e1"][k], e1), (entries["e2"][k], e2), (entries["normal"][k], nrm)):
            np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(entries["probability"].astype(np.float64).sum(), 1.0, rtol=1e-6)
    want_pdf = np.zeros(len(scene))
    for (g, _, _, _, _, _, _, lum) in ref:
        want_pdf[g] = lum / total
    np.testing.assert_allclose(pdf, want_pdf, rtol=1e-6)


def test_light_table_exclusions(ff):
    scene = mixed_scene()
    entries, pdf = lib.light_table(scene)
    assert set(entries["geometry"].tolist()) == {0, 1}  # sphere, zero emission and diffuse left out
    assert (entries["primitive"][entries["geometry"] == 0] == -1).all()
    assert sorted(entries["primitive"][entries["geometry"] == 1].tolist()) == list(range(scene.geometries[1].m_numberOfTriangles))
    assert pdf[2] == pdf[3] == pdf[4] == 0.0 and pdf[0] > 0.0 and pdf[1] > 0.0
    # a scene whose only emitter is a sphere has an empty table
    entries, pdf = lib.light_table(nee_ref.sphere_light_scene())
    assert len(entries["area"]) == 0 and not pdf.any()
    # the reference's own scene has no emitter at all
    entries, _ = lib.light_table(scenes.reference_scene(scenes.load_mesh("cube")))
    assert len(entries["area"]) == 0


def test_alias_table_reproduces_the_probabilities(ff):
    entries, _ = lib.light_table(nee_ref.triangle_light_scene())
    n = len(entries["area"])
    got = entries["alias_probability"].astype(np.float64) / n
    np.add.at(got, entries["alias"], (1.0 - entries["alias_probability"].astype(np.float64)) / n)
    np.testing.assert_allclose(got, entries["probability"], rtol=1e-5, atol=1e-7)
    assert ((entries["alias"] >= 0) & (entries["alias"] < n)).all()


def test_light_table_arguments(ff):
    L = lib.load()
    assert L.ff_light_table(None, 1, None, 0, None) == -T.FF_ERR_INVALID_ARG
    scene = scenes.cornell_wahoo_scene()
    assert L.ff_light_table(scene.geometries, len(scene), None, 0, None) == 1  # count only
    assert L.ff_light_table(scene.geometries, len(scene), None, 4, None) == -T.FF_ERR_INVALID_ARG


def test_reference_philox_matches_the_oracle(ff, oracle):
    rng = np.random.default_rng(3)
    c0 = rng.integers(0, 2 ** 32, 64, dtype=np.uint64)
    c1 = rng.integers(0, 2 ** 32, 64, dtype=np.uint64)
    for key in (nee_ref.frame_key(1234), nee_ref.frame_key(1234) ^ nee_ref.KEY_SELECT, nee_ref.frame_key(77) ^ nee_ref.KEY_POINT):
        o0, o1 = nee_ref.philox(c0, c1, key)
        for i in range(len(c0)):
            a, b = C.c_uint32(), C.c_uint32()
            oracle.orc_philox2x32_10(int(c0[i]), int(c1[i]), key, C.byref(a), C.byref(b))
            assert (int(o0[i]), int(o1[i])) == (a.value, b.value)


def test_shade_mode_nee_passes_parameter_validation(ff):
    p = lib.render_params(64, 36, bounces=4, spp=3, shade_mode=T.SHADE_DIFFUSE_PATH_NEE)
    assert T.SHADE_DIFFUSE_PATH_NEE == 3
    assert lib.check_render_params(p) == T.FF_OK
    for bad in (4, 5, -1, 100):
        p.shade_mode = bad
        assert lib.check_render_params(p) == T.FF_ERR_INVALID_ARG
    for mode in (T.SHADE_NORMAL_DEBUG, T.SHADE_DIFFUSE_PATH, T.SHADE_DIFFUSE_PATH_SMOOTH):
        p.shade_mode = mode
        assert lib.check_render_params(p) == T.FF_OK
    p = lib.render_params(64, 36, bounces=0, shade_mode=T.SHADE_DIFFUSE_PATH_NEE)
    assert lib.check_render_params(p) == T.FF_ERR_INVALID_ARG
