"""ff_interpolate on the host side: exports, defaults, every argument check (all before any device work), the host twin
ff_interpolate_host - the kernels' per-pixel functions compiled for the host - bit for bit against the numpy float32 restatement
(tests/interpolate_ref.py) over sizes, t, fill radii and geometry maps, the consequences the header states,
ff_interpolate_geometry_maps against a float64 composition, and one case on real frames from the CPU oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
import interpolate_cases as IC
import interpolate_ref as R

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def twin(c, **params):
    """ff_interpolate_host of a case -> (rgb8, radiance, counts)."""
    return lib.interpolate_host((c["mid"][0], c["mid"][1:]), (c["a"][0], c["a"][1], c["a"][2:]), (c["b"][0], c["b"][1], c["b"][2:]),
                                lib.interpolate_params(**params), c["maps"])


def assert_matches_reference(got, c, **params):
    out, rgb8, counts, state = IC.ref(c, **params)
    assert R.same_bits(got[1], out), np.argwhere((got[1].view(np.uint32) != out.view(np.uint32)).any(-1))[:5]
    assert np.array_equal(got[0], rgb8) and np.array_equal(got[2], counts), (got[2], counts)
    return out, counts, state


def test_new_entry_points_are_exported_and_declared(ff):
    handle = ff.load()
    header = open(os.path.join(ROOT, "include", "firefly", "ff_api.h")).read()
    declared = set(re.findall(r"FF_API\s+[\w\s\*]+?\b(ff_\w+)\s*\(", header))
    for name in ("ff_interpolate_params_init", "ff_interpolate", "ff_interpolate_host", "ff_interpolate_geometry_maps"):
        assert name in ff.EXPORTS and name in declared and hasattr(handle, name), name


def test_interpolate_params_defaults_and_size():
    p = lib.interpolate_params()
    assert (p.t, p.surface_tolerance, p.fill_radius, p.flags, p.reserved) == (0.5, 4.0, 4, 0, 0)
    assert C.sizeof(T.FfInterpolateParams) == T.INTERPOLATE_PARAMS_BYTES == 20
    types_h = open(os.path.join(ROOT, "include", "firefly", "ff_types.h")).read()
    assert "static_assert(sizeof(FfInterpolateParams) == 20" in types_h and "_Static_assert(sizeof(FfInterpolateParams) == 20" in types_h
    assert lib.interpolate_params(t=0.25, fill_radius=8).fill_radius == 8
    with pytest.raises(TypeError):
        lib.interpolate_params(strength=1.0)


def raw_host(c, p, rgb8=None, out=None, w=None, h=None, drop=None, maps=None, n=0, counts=None):
    """ff_interpolate_host with raw pointers; drop names an argument that is passed as NULL."""
    ptr = lambda name, a: None if drop == name or a is None else a.ctypes.data  # noqa: E731
    cam = lambda name, k: None if drop == name else C.byref(k)  # noqa: E731
    (cm, pm, im), (ca, ra, pa, ia), (cb, rb, pb, ib) = c["mid"], c["a"], c["b"]
    hh, ww = im.shape[:2]
    return lib.load().ff_interpolate_host(ww if w is None else w, hh if h is None else h, C.byref(p) if p is not None else None,
                                          cam("camera_mid", cm), ptr("position", pm), ptr("ids", im),
                                          cam("camera_a", ca), ptr("radiance_a", ra), ptr("position_a", pa), ptr("ids_a", ia),
                                          cam("camera_b", cb), ptr("radiance_b", rb), ptr("position_b", pb), ptr("ids_b", ib),
                                          ptr("maps", maps), n, ptr("rgb8", rgb8), ptr("out", out), ptr("counts", counts))


def test_every_refused_argument_names_its_field():
    c = IC.case((33, 9))
    out = np.full((9, 33, 3), 7.0, F)
    last = lambda: lib.load().ff_last_error().decode()  # noqa: E731
    nan, inf = float("nan"), float("inf")
    for field, value in [("t", -0.25), ("t", 1.5), ("t", nan), ("t", inf), ("surface_tolerance", 0.0), ("surface_tolerance", -1.0),
                         ("surface_tolerance", nan), ("surface_tolerance", inf), ("fill_radius", -1), ("fill_radius", 9), ("flags", 1),
                         ("reserved", 1)]:
        assert raw_host(c, lib.interpolate_params(**{field: value}), None, out) == T.FF_ERR_INVALID_ARG, (field, value)
        assert field in last(), (field, value, last())
    for t in (0.0, -0.0, 1.0):  # (both ends are allowed)
        assert raw_host(c, lib.interpolate_params(t=t), None, out) == T.FF_OK
    out[:] = 7.0
    p = lib.interpolate_params()
    assert raw_host(c, None, None, out) == T.FF_ERR_INVALID_ARG and "params" in last()
    for name in ("camera_mid", "position", "ids", "camera_a", "radiance_a", "position_a", "ids_a", "camera_b", "radiance_b", "position_b", "ids_b"):
        assert raw_host(c, p, None, out, drop=name) == T.FF_ERR_INVALID_ARG and re.search(rf"\b{name} is null", last()), (name, last())
    for w, h in [(0, 9), (33, 0), (65536, 1), (1, 65536), (-1, 3)]:
        assert raw_host(c, p, None, out, w=w, h=h) == T.FF_ERR_INVALID_ARG and "size" in last()
    maps = np.tile(np.eye(3, 4, dtype=F), (6, 2, 1, 1))
    for n in (0, -1):
        assert raw_host(c, p, None, out, maps=maps, n=n) == T.FF_ERR_INVALID_ARG and "num_geometries" in last()
    # an output on an input, on a part of one, and on the other output
    for name, arr in [("position", c["mid"][1]), ("radiance_a", c["a"][1]), ("position_a", c["a"][2]), ("radiance_b", c["b"][1]), ("position_b", c["b"][2])]:
        arr = np.array(arr)
        cc = dict(c, mid=(c["mid"][0], arr, c["mid"][2])) if name == "position" else dict(
            c, **{name[-1]: tuple(arr if i == (1 if name.startswith("radiance") else 2) else v for i, v in enumerate(c[name[-1]]))})
        assert raw_host(cc, p, None, arr) == T.FF_ERR_INVALID_ARG and f"radiance_out overlaps {name}" in last(), (name, last())
        assert raw_host(cc, p, arr.view(np.uint8), out) == T.FF_ERR_INVALID_ARG and f"rgb8 overlaps {name}" in last(), (name, last())
        assert raw_host(cc, p, None, arr.reshape(-1)[3:]) == T.FF_ERR_INVALID_ARG and f"radiance_out overlaps {name}" in last()
    ids = np.array(c["b"][3])
    cc = dict(c, b=c["b"][:3] + (ids,))
    assert raw_host(cc, p, ids.view(np.uint8), out) == T.FF_ERR_INVALID_ARG and "rgb8 overlaps ids_b" in last()
    assert raw_host(c, p, out.view(np.uint8), out) == T.FF_ERR_INVALID_ARG and "rgb8 overlaps radiance_out" in last()
    assert (out == 7.0).all()  # (no refused call wrote anything)
    # the device entry point refuses a NULL state, and the same arguments, before it touches a device
    (cm, pm, im), (ca, ra, pa, ia), (cb, rb, pb, ib) = c["mid"], c["a"], c["b"]
    d = lambda a: a.ctypes.data  # noqa: E731
    call = lambda state, q: lib.load().ff_interpolate(state, 33, 9, C.byref(q), C.byref(cm), d(pm), d(im), C.byref(ca), d(ra), d(pa), d(ia), C.byref(cb),  # noqa: E731
                                                      d(rb), d(pb), d(ib), None, 0, 0, None, 0, d(out), 0, None)
    assert call(None, p) == T.FF_ERR_INVALID_ARG and "state" in last()


@pytest.mark.parametrize("size", IC.SIZES + [IC.MAIN], ids=lambda s: f"{s[0]}x{s[1]}")
def test_twin_matches_the_restatement_over_t_radii_and_maps(size):
    for moving in (False, True):
        c = IC.case(size, moving)
        for t in IC.TS:
            assert_matches_reference(twin(c, t=t), c, t=t)
        for r in IC.RADII:
            assert_matches_reference(twin(c, t=0.25, fill_radius=r), c, t=0.25, fill_radius=r)
        for tol in (0.5, 16.0):
            assert_matches_reference(twin(c, surface_tolerance=tol), c, surface_tolerance=tol)


def test_main_case_populates_all_five_counts_and_they_sum_to_the_image():
    for moving in (False, True):
        counts = IC.ref(IC.case(IC.MAIN, moving))[2]
        assert (counts > 0).all() and counts.sum() == IC.MAIN[0] * IC.MAIN[1], counts
    for size in IC.SIZES:
        for r in (0, 4):
            assert twin(IC.case(size), fill_radius=r)[2].sum() == size[0] * size[1]
    assert twin(IC.case(IC.MAIN), fill_radius=0)[2][R.FILLED] == 0  # (no fill: every hole falls back)


def test_geometry_index_beyond_the_table_fails_the_lookup():
    c = IC.case(IC.MAIN, True)
    short = dict(c, maps=c["maps"][:2])  # geometries 2 .. 5 are not known
    out, counts, state = assert_matches_reference(twin(short), short)
    unknown = c["mid"][2][..., 0] >= 2
    assert unknown.any() and (state[unknown] >= R.FILLED).all()


def test_equal_cameras_and_equal_sources_return_the_source():
    cm, pm, im = IC.case(IC.MAIN)["mid"]
    rad = IC.radiance(pm, im, 3)
    rad[5, 7, 1] = -0.0
    c = {"mid": (cm, pm, im), "a": (cm, rad, pm, im), "b": (cm, rad, pm, im), "maps": None}
    for t in IC.TS:
        rgb8, out, counts = twin(c, t=t)
        assert R.same_bits(out, rad) and counts[R.BOTH] == rad.shape[0] * rad.shape[1]
    identities = dict(c, maps=np.tile(np.eye(3, 4, dtype=F), (6, 2, 1, 1)))
    assert R.same_bits(twin(identities, t=0.25)[1], rad)


def test_t_zero_and_one_return_the_valid_source_colour():
    c = IC.case(IC.MAIN)
    ra = np.array(c["a"][1])
    ra[ra[..., 0] > 0.5, 2] = -0.0  # (signed zeros among A's colours)
    c = IC.with_radiance(c, ra)
    half = IC.ref(c, t=0.5)
    state = half[3]
    # c_A and c_B themselves: what a call with the other source made invalid (all NaN) returns where the source alone is valid
    only_a = twin(IC.with_radiance(c, None, np.full_like(ra, np.nan)))[1]
    only_b = twin(IC.with_radiance(c, np.full_like(ra, np.nan), None))[1]
    a_valid, b_valid = np.isin(state, (R.BOTH, R.A_ONLY)), np.isin(state, (R.BOTH, R.B_ONLY))
    assert (a_valid & (ra[..., 2] == 0)).any()
    assert R.same_bits(twin(c, t=0.0)[1][a_valid], only_a[a_valid])
    assert R.same_bits(twin(c, t=1.0)[1][b_valid], only_b[b_valid])


def test_constant_colour_comes_back_everywhere():
    for moving in (False, True):
        c = IC.case(IC.MAIN, moving)
        const = np.broadcast_to(np.array([0.3, 1.7, 0.1], F), c["a"][1].shape).copy()
        cc = IC.with_radiance(c, const, const)
        for t in (0.0, 0.3, 1.0):
            for r in (0, 4):
                rgb8, out, counts = twin(cc, t=t, fill_radius=r)
                assert R.same_bits(out, const) and (counts > 0).sum() >= 4


def test_non_finite_source_pixels_never_count_as_taps():
    c = IC.planted_nonfinite(IC.case(IC.MAIN))
    out, counts, state = assert_matches_reference(twin(c), c)
    assert not np.isfinite(c["a"][1]).all() and not np.isfinite(c["b"][1]).all()
    assert np.isfinite(out[state != R.FALLBACK]).all()
    moving = IC.planted_nonfinite(IC.case(IC.MAIN, True), seed=9)
    assert_matches_reference(twin(moving, t=0.25), moving, t=0.25)


def test_seam_holes_are_filled_across_the_tile_seams():
    c, hole = IC.seam_holes()
    for r in IC.RADII:
        out, counts, state = assert_matches_reference(twin(c, fill_radius=r), c, fill_radius=r)
        assert np.array_equal(state >= R.FILLED, hole)
        if r == 0:
            assert (state[hole] == R.FALLBACK).all() and not np.isfinite(out[hole]).all()
        else:
            assert np.isfinite(out[state == R.FILLED]).all() and (state == R.FILLED).sum() >= 12
    # the inside of a block wider than the radius has no donor
    assert (IC.ref(c, fill_radius=1)[3][11:13, 42:50] == R.FALLBACK).all()


def test_geometry_maps_against_a_float64_composition():
    rng = np.random.default_rng(4)
    mid = scenes.Scene()
    a = scenes.Scene()
    b = scenes.Scene()
    grey = scenes.make_bxdf(T.BXDF_DIFFUSE, albedo=(0.5, 0.5, 0.5))
    for g in range(5):
        pose = lambda: (tuple(rng.uniform(-3, 3, 3)), tuple(rng.uniform(-180, 180, 3)), tuple(rng.uniform(0.5, 2, 3)))  # noqa: E731
        pm = pose()
        pa = pm if g in (1, 3) else pose()
        pb = pm if g in (3, 4) else pose()
        for s, p in ((mid, pm), (a, pa), (b, pb)):
            s.add_plane(*p, grey)
    mid.finalize(), a.finalize(), b.finalize()
    maps, flags = lib.interpolate_geometry_maps(mid.geometries, a.geometries, b.geometries)
    assert maps.shape == (5, 2, 3, 4) and flags.tolist() == [[0, 0], [1, 0], [0, 0], [1, 1], [0, 1]]
    model = lambda s, g: np.array(s.geometries[g].m_modelMatrix.m[:], F).astype(np.float64).reshape(4, 4).T  # noqa: E731
    for g in range(5):
        for S, s in enumerate((a, b)):
            if flags[g, S]:
                assert maps[g, S].tobytes() == np.eye(3, 4, dtype=F).tobytes()
                continue
            want = (model(s, g) @ np.linalg.inv(model(mid, g)))[:3]
            # float32 rounding of entries of magnitude up to |want|, plus the float64 inverse's error
            assert np.abs(maps[g, S] - want).max() <= 2.0 ** -23 * max(1.0, np.abs(want).max())
    # the same from plain matrices
    mats = lambda s: np.array([s.geometries[g].m_modelMatrix.m[:] for g in range(5)], F)  # noqa: E731
    maps2, flags2 = lib.interpolate_geometry_maps(mats(mid), mats(a), mats(b))
    assert maps2.tobytes() == maps.tobytes() and np.array_equal(flags, flags2)
    h = lib.load()
    assert h.ff_interpolate_geometry_maps(None, a.geometries, b.geometries, 5, maps.ctypes.data, None) == T.FF_ERR_INVALID_ARG
    assert h.ff_interpolate_geometry_maps(mid.geometries, a.geometries, b.geometries, 0, maps.ctypes.data, None) == T.FF_ERR_INVALID_ARG
    singular = np.array(mats(mid))
    singular[0] = 0.0
    with pytest.raises(Exception, match="singular"):
        lib.interpolate_geometry_maps(singular, mats(a), mats(b))


ORACLE_POSES = [(-0.35, 0.0, 2.4), (0.0, 0.0, 2.4), (0.35, 0.0, 2.4)]  # A, mid, B: about 5 pixels of parallax at the cube, 64 x 36


@pytest.fixture(scope="module")
def oracle_frames():
    """Three poses of the Cornell box with spheres at 64 x 36 (the size smoke() uses) in FF_SHADE_NORMAL_DEBUG, noise-free, and
    their G-buffers, all from the CPU oracle."""
    from gbuffer_ref import oracle_gbuffer
    from oracle_lib import oracle_render
    scene = scenes.cornell_spheres_scene()
    params = lib.render_params(64, 36, bounces=1, spp=1, shade_mode=T.SHADE_NORMAL_DEBUG)
    frames = []
    for pos in ORACLE_POSES:
        cam = scenes.posed_camera(64, 36, position=pos, yaw=-90.0, pitch=0.0)
        gb = oracle_gbuffer(scene, cam, params)
        frames.append((cam, oracle_render(scene, cam, params, threads=8)[1], gb["position"], gb["ids"]))
    return frames


def oracle_mse_ratio(frames, **params):
    (ca, ra, pa, ia), (cm, rm, pm, im), (cb, rb, pb, ib) = frames
    out = lib.interpolate_host((cm, (pm, im)), (ca, ra, (pa, ia)), (cb, rb, (pb, ib)), lib.interpolate_params(**params))[1]
    truth = rm.astype(np.float64)
    mse = ((out - truth) ** 2).mean()
    blend = (((ra.astype(np.float64) + rb) / 2 - truth) ** 2).mean()
    return mse, blend


def test_interpolated_oracle_frame_beats_the_blend(oracle_frames):
    """Measured: MSE 0.000546 against the blend's 0.0149 (ratio 0.0365) with the defaults; DESIGN.md section 8 row 21 has the sweep
    of surface_tolerance."""
    (ca, ra, pa, ia), (cm, rm, pm, im), (cb, rb, pb, ib) = oracle_frames
    assert np.abs(ra.astype(np.float64) - rm).max() > 0.5  # (the poses differ visibly)
    mse, blend = oracle_mse_ratio(oracle_frames)
    print(f"interpolated MSE {mse:.6g}, blend MSE {blend:.6g}, ratio {mse / blend:.4f}")
    assert mse < blend
    c = {"mid": (cm, pm, im), "a": (ca, ra, pa, ia), "b": (cb, rb, pb, ib), "maps": None}
    assert_matches_reference(twin(c), c)
