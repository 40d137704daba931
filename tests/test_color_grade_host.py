"""ff_color_grade_host (no GPU): the twin against the numpy float32 restatement (tests/color_grade_ref.py) bit for bit over the stage
combinations, both interpolations and both knot axes; the identities the header promises; the tetrahedron a tie takes; both
interpolations against float64 within bounds counted from the formulas' roundings; .cube files; every argument check."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from gpupathtracer_amd import lib
from gpupathtracer_amd import types as T
import color_grade_ref as R
from color_grade_cases import (AXES, FLAG_SETTINGS, PRIMARY_FIELDS, assert_same, flags_id, inputs, log_axis, make_lut, params, planted_non_finite)

F = np.float32
U24 = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ff_grade_params_init", "ff_grade_lut_create", "ff_grade_lut_destroy", "ff_color_grade", "ff_color_grade_host", "ff_load_cube", "ff_free_cube",
         "ff_save_cube"]


def last_error():
    return lib.load().ff_last_error().decode()


def test_exports_layout_and_defaults():
    handle = lib.load()
    header = open(os.path.join(ROOT, "include", "firefly", "ff_api.h")).read()
    declared = set(re.findall(r"FF_API\s+[\w\s\*]+?\b(ff_\w+)\s*\(", header))
    for name in NAMES:
        assert name in lib.EXPORTS and name in declared and hasattr(handle, name), name
    assert (C.sizeof(T.FfGradeParams), C.sizeof(T.FfGradeLut), C.sizeof(T.FfCubeFile)) == (64, 64, 192)
    assert T.FfGradeLut.curves.offset == 48 and T.FfCubeFile.lut.offset == 128
    p = lib.grade_params()
    assert (p.flags, p.saturation, p.lut_id, p.reserved) == (0, 1.0, -1, 0)
    assert list(p.matrix) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and list(p.offset) == [0, 0, 0]
    assert (T.GRADE_PRIMARY, T.GRADE_CURVES, T.GRADE_LUT3D, T.GRADE_TRILINEAR) == (R.PRIMARY, R.CURVES, R.LUT3D, R.TRILINEAR)
    assert T.GRADE_LDS_MAX_SIZE ** 3 * 12 <= T.GRADE_LDS_BYTES < (T.GRADE_LDS_MAX_SIZE + 1) ** 3 * 12


@pytest.mark.parametrize("N", (2, 3, 5))
@pytest.mark.parametrize("K", (2, 3, 129))
def test_twin_equals_restatement_bit_for_bit(N, K):
    for axis in AXES:
        lut = make_lut(N, K, axis)
        rad = planted_non_finite(inputs(41, 29, lut), (0, 3, 4, 700))
        for flags in FLAG_SETTINGS:
            p = params(flags)
            got = lib.color_grade_host(rad, p, lut)
            assert_same(got, R.color_grade(rad, p, lut))
            assert np.array_equal(R.bits(got[1].reshape(-1, 3)[[0, 3, 4, 700]]), R.bits(rad.reshape(-1, 3)[[0, 3, 4, 700]])), flags_id(flags)


def test_flags_0_is_a_copy_and_outputs_are_optional():
    lut = make_lut(3, 3, R.AXIS_LINEAR)
    rad = planted_non_finite(inputs(33, 9, lut), (1, 2, 100))
    for use in (None, lut):
        rgb8, out = lib.color_grade_host(rad, params(0), use)
        assert np.array_equal(R.bits(out), R.bits(rad)) and np.array_equal(rgb8, R.to_u8(rad))
    p = params(7)
    want = R.color_grade(rad, p, lut)
    got = lib.color_grade_host(rad, p, lut, want_out=False)
    assert got[1] is None and np.array_equal(got[0], want[0])
    got = lib.color_grade_host(rad, p, lut, want_rgb8=False)
    assert got[0] is None and np.array_equal(R.bits(got[1]), R.bits(want[1]))
    assert lib.color_grade_host(rad, p, lut, want_rgb8=False, want_out=False) == (None, None)
    assert_same(lib.color_grade_host(rad, p, lut, in_place=True), want)


def test_constant_lattice_and_curves_return_their_value():
    for value in (0.3, -2.75, 1.0e30, 0.0):
        for axis in AXES:
            lut = make_lut(5, 129, axis, constant=value)
            rad = inputs(41, 29, lut)
            for flags in (R.CURVES, R.LUT3D, R.LUT3D | R.TRILINEAR, R.PRIMARY | R.CURVES | R.LUT3D):
                out = lib.color_grade_host(rad, params(flags), lut)[1]
                assert (R.bits(out) == R.bits(F(value))).all(), (value, flags_id(flags))


def test_lattice_points_return_lattice_values_exactly():
    for N, dmin, dmax in ((5, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), (3, (-1.0, 0.0, 2.0), (1.0, 4.0, 3.0)), (17, (0.0, 0.0, 0.0), (2.0, 2.0, 2.0))):
        # (domains whose lattice points are floats and whose p is an integer exactly: N - 1 a power of two)
        rng = np.random.default_rng(N)
        table = rng.uniform(-1.0, 2.0, (N, N, N, 3)).astype(F)
        lut = lib.grade_lut(table=table, domain_min=dmin, domain_max=dmax)
        k, j, i = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
        pts = np.stack([dmin[c] + (dmax[c] - dmin[c]) * (ix / (N - 1)) for c, ix in enumerate((i, j, k))], axis=-1).astype(F).reshape(1, -1, 3)
        for flags in (R.LUT3D, R.LUT3D | R.TRILINEAR):
            out = lib.color_grade_host(pts, lib.grade_params(flags=flags), lut)[1].reshape(N, N, N, 3)
            # (every fraction is 0 below the top ends; at a top end f = 1 and A + 1 (B - A) is B only within a rounding)
            assert np.array_equal(R.bits(out[:-1, :-1, :-1]), R.bits(table[:-1, :-1, :-1]))
            assert np.abs(out - table).max() <= 4 * 3 * U24 * np.abs(table).max()
    # ... and knots return knot values
    for axis in AXES:
        lut = make_lut(0, 129, axis)
        d = lut.desc
        if axis == R.AXIS_LOG:
            x = (int(F(d.curve_lo).view(np.uint32)) + (np.arange(129, dtype=np.int64) << d.curve_shift)).astype(np.uint32).view(F)
        else:
            lut = lib.grade_lut(curves=lut.curves, curve_lo=-1.0, curve_hi=3.0)   # (knot positions that are floats: 128 cells of 1 / 32)
            x = (-1.0 + np.arange(129) / 32.0).astype(F)
        out = lib.color_grade_host(np.stack([x, x, x], -1)[None], lib.grade_params(flags=R.CURVES), lut)[1]
        assert np.array_equal(R.bits(out[0].T[:, :-1]), R.bits(lut.curves[:, :-1]))


def test_tie_pixels_take_the_branch_the_stable_sort_names():
    """On a face two tetrahedra share, their formulas agree in exact arithmetic and differ in float32 rounding, through P1 or P2.
    On the unit cube at N = 2 (the fractions are the pixel itself) with eight unrelated texels, every tie pixel must carry the bits
    of the order the stable sort names, r before g before b - and the other orders its fractions allow must give other bits on many
    of them, or the lattice would not tell the branches apart."""
    rng = np.random.default_rng(11)
    table = rng.uniform(-3.0, 5.0, (2, 2, 2, 3)).astype(F)
    lut = lib.grade_lut(table=table)
    flat = table.reshape(8, 3)
    step = (1, 2, 4)

    def along(order, f):
        a, b, c = (F(f[x]) for x in order)
        p0, p1, p2, p3 = flat[0], flat[step[order[0]]], flat[step[order[0]] + step[order[1]]], flat[7]
        out = p0 + a * (p1 - p0)
        out = out + b * (p2 - p1)
        return (out + c * (p3 - p2)).astype(F)

    v = rng.uniform(0.05, 0.95, (300, 2)).astype(F)
    ties = np.concatenate([np.stack([v[:, 0], v[:, 0], v[:, 1]], -1), np.stack([v[:, 0], v[:, 1], v[:, 0]], -1), np.stack([v[:, 1], v[:, 0], v[:, 0]], -1),
                           np.stack([v[:, 0], v[:, 0], v[:, 0]], -1)])
    out = lib.color_grade_host(ties[None], lib.grade_params(flags=R.LUT3D), lut)[1][0]
    assert np.array_equal(R.bits(out), R.bits(R.lattice(ties[None], lut, False)[0]))
    told_apart = 0
    for f, got in zip(ties, out):
        named = tuple(sorted(range(3), key=lambda ax: -f[ax]))          # (Python's sort is stable)
        assert np.array_equal(R.bits(got), R.bits(along(named, f))), (f, named)
        allowed = [o for o in itertools.permutations(range(3)) if f[o[0]] >= f[o[1]] >= f[o[2]] and o != named]
        assert allowed
        told_apart += any(not np.array_equal(R.bits(along(o, f)), R.bits(got)) for o in allowed)
    print(f"{told_apart} of {len(ties)} tie pixels have other bits under another allowed order")
    assert told_apart > len(ties) // 4


def affine_lattice(N, A, b, dmin, dmax):
    """V = A c + b at the lattice points, in float64."""
    k, j, i = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
    c = np.stack([dmin[n] + (dmax[n] - dmin[n]) * (ix / (N - 1)) for n, ix in enumerate((i, j, k))], axis=-1)
    return c @ A.T + b


def test_affine_lattice_reproduces_the_affine_map():
    """V = A c + b sampled in float64 and rounded to float32; pixels inside the domain; the result against A x + b in float64.
    With u = 2^-24, M the largest lattice magnitude and, per output channel o, T_o = sum_c |A_oc| (dmax_c - dmin_c), to first order:
      texels   each is rounded once, and both forms are convex combinations of them:                                   1 u M
      p        dmax - dmin, x' - dmin, the quotient and the product with N - 1 are four roundings, p (1 + 4u); f = p - i is
               exact.  An error of 4 u p_c <= 4 u (N - 1) cells on axis c moves the result by the slope per cell,
               |A_oc| (dmax_c - dmin_c) / (N - 1), whichever cell the rounded p falls in (an affine lattice interpolates exactly
               in each):                                                                                               4 u T_o
      formula  tetrahedral: three differences (each |d| <= 2M: 2 u M), three products with a fraction <= 1 (2 u M each), three
               sums whose exact values are convex combinations of texels (u M each): 3 (2 + 2 + 1) = 15 u M.  Trilinear: three
               levels of lerps, each one difference, one product and one sum (5 u M), a level passing the errors of the one
               before with weights that sum to 1: 15 u M again.
    Together 16 u M + 4 u T_o <= 20 u L with L = max(M, T_o), the largest magnitude involved; the bound asserted is 21 u L, the last
    u L covering the second-order terms."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for N, dmin, dmax, scale in ((2, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 1.0), (5, (-0.5, 0.0, 0.125), (1.5, 1.0, 2.0), 3.0), (17, (-1.0, -1.0, -1.0), (7.0, 2.0, 3.0), 40.0)):
        A = rng.uniform(-1.0, 1.0, (3, 3)) * scale
        b = rng.uniform(-1.0, 1.0, 3) * scale
        V = affine_lattice(N, A, b, dmin, dmax)
        lut = lib.grade_lut(table=V, domain_min=dmin, domain_max=dmax)
        lo, hi = np.array(dmin, F), np.array(dmax, F)
        x = (lo + (hi - lo) * rng.random((1, 4000, 3))).astype(F)
        x = np.clip(x, lo, hi)
        want = x.astype(np.float64) @ A.T + b
        span = (np.abs(A) * (hi.astype(np.float64) - lo.astype(np.float64))[None, :]).sum(axis=1)
        L = max(np.abs(V).max(), span.max())
        for flags in (R.LUT3D, R.LUT3D | R.TRILINEAR):
            out = lib.color_grade_host(x, lib.grade_params(flags=flags), lut)[1]
            err = np.abs(out.astype(np.float64) - want).max()
            print(f"N = {N} {flags_id(flags)}: max error {err:.3e} = {err / (21 * U24 * L):.3f} of the bound 21 * 2^-24 * {L:.4g}")
            worst = max(worst, err / (21 * U24 * L))
            assert err <= 21 * U24 * L
    assert worst > 0.0


def test_a_lattice_that_is_not_affine_tells_the_interpolations_apart():
    """Each form against its own formula in float64 on the float32 cells, fractions and texels: only the formula's roundings
    remain, 15 u M to first order (see test_affine_lattice_reproduces_the_affine_map); asserted 16 u M."""
    lut = make_lut(5, 0, R.AXIS_LINEAR)
    rad = inputs(61, 37, lut)
    M = float(np.abs(lut.table).max())
    tet = lib.color_grade_host(rad, lib.grade_params(flags=R.LUT3D), lut)[1]
    tri = lib.color_grade_host(rad, lib.grade_params(flags=R.LUT3D | R.TRILINEAR), lut)[1]
    assert (np.abs(tet - tri) > 1.0e-3).any()
    for out, trilinear in ((tet, False), (tri, True)):
        err = np.abs(out.astype(np.float64) - R.lattice(rad, lut, trilinear, np.float64)).max()
        print(f"{'trilinear' if trilinear else 'tetrahedral'}: max error {err:.3e} = {err / (16 * U24 * M):.3f} of the bound 16 * 2^-24 * {M:.4g}")
        assert 0.0 < err <= 16 * U24 * M
    # each is nearer its own float64 form than the other's
    assert np.abs(tet.astype(np.float64) - R.lattice(rad, lut, True, np.float64)).max() > 16 * U24 * M


def test_non_finite_pixels_are_copied_and_nothing_else_moves():
    lut = make_lut(5, 129, R.AXIS_LOG)
    clean = inputs(65, 3, lut)
    places = (0, 3, 4, 63, 64, 127, 128, 194)
    bad = planted_non_finite(clean, places)
    for flags in FLAG_SETTINGS:
        p = params(flags)
        rgb8, out = lib.color_grade_host(bad, p, lut)
        ref8, ref = lib.color_grade_host(clean, p, lut)
        mask = np.zeros(65 * 3, bool)
        mask[list(places)] = True
        mask = mask.reshape(3, 65)
        assert np.array_equal(R.bits(out[mask]), R.bits(bad[mask])) and np.array_equal(rgb8[mask], R.to_u8(bad[mask]))
        assert np.array_equal(R.bits(out[~mask]), R.bits(ref[~mask])) and np.array_equal(rgb8[~mask], ref8[~mask])


def test_primary_alone_matches_float64_and_an_overflow_is_stored_as_it_comes():
    rad = inputs(41, 29)
    out = lib.color_grade_host(rad, params(R.PRIMARY))[1]
    m, o, s = np.array(PRIMARY_FIELDS["matrix"], F).astype(np.float64).reshape(3, 3), np.array(PRIMARY_FIELDS["offset"], F).astype(np.float64), float(F(0.7))
    c = rad.astype(np.float64) @ m.T + o
    lum = c @ np.array([F(0.2126), F(0.7152), F(0.0722)], np.float64)
    want = lum[..., None] + s * (c - lum[..., None])
    assert np.abs(out - want).max() <= 16 * U24 * np.abs(c).max() * 1.3   # (a sanity bound: 16 roundings of values up to 1.3 max|c'|)
    big = np.full((1, 4, 3), 3.0e38, F)
    got = lib.color_grade_host(big, lib.grade_params(flags=R.PRIMARY, matrix=(2, 0, 0, 0, 2, 0, 0, 0, 2)))
    assert np.isnan(got[1]).all() and not got[0].any()            # (Inf, and Inf - Inf in the saturation; a NaN's byte is 0)
    got = lib.color_grade_host(big, lib.grade_params(flags=R.PRIMARY, matrix=(2, 0, 0, 0, 2, 0, 0, 0, 2), saturation=0.0))
    assert np.isnan(got[1]).all()                                 # (0 * NaN)


# ---- .cube ----------------------------------------------------------------------------------------------------------------------

def test_cube_round_trip_bit_for_bit(tmp_path):
    lut3 = make_lut(5, 0, R.AXIS_LINEAR)
    path = str(tmp_path / "look.cube")
    lib.save_cube(path, lut3, title="a look")
    back, title = lib.load_cube(path)
    assert title == "a look" and back.desc.size == 5 and back.desc.curve_size == 0 and back.curves is None
    assert np.array_equal(R.bits(back.table), R.bits(lut3.table))
    assert list(back.desc.domain_min) == list(lut3.desc.domain_min) and list(back.desc.domain_max) == list(lut3.desc.domain_max)
    lut1 = make_lut(0, 129, R.AXIS_LINEAR)
    lib.save_cube(path, lut1)
    back, title = lib.load_cube(path)
    assert title == "" and back.desc.curve_size == 129 and back.desc.size == 0 and back.desc.curve_axis == R.AXIS_LINEAR
    assert np.array_equal(R.bits(back.curves), R.bits(lut1.curves))
    assert (F(back.desc.curve_lo), F(back.desc.curve_hi)) == (F(lut1.desc.curve_lo), F(lut1.desc.curve_hi))
    # awkward values survive %.9g
    odd = np.array([1.0e-45, -1.1754944e-38, 0.1, 1.0 / 3.0, 16777217.0, 1.0e38, -0.0, 3.4028235e38 / 4], F)
    table = np.resize(odd, 2 * 2 * 2 * 3).astype(F).reshape(2, 2, 2, 3)
    lib.save_cube(path, lib.grade_lut(table=table, domain_min=(-0.1, 0.0, 1.0e-3), domain_max=(0.1, 1.0 / 3.0, 7.0)))
    back, _ = lib.load_cube(path)
    assert np.array_equal(R.bits(back.table), R.bits(table))
    assert np.array_equal(R.bits(np.array(list(back.desc.domain_max), F)), R.bits(np.array([0.1, 1.0 / 3.0, 7.0], F)))
    # what a file cannot hold
    with pytest.raises(lib.FireflyError, match="not both"):
        lib.save_cube(path, make_lut(3, 3, R.AXIS_LINEAR))
    with pytest.raises(lib.FireflyError, match="FF_GRADE_AXIS_LINEAR"):
        lib.save_cube(path, make_lut(0, 3, R.AXIS_LOG))
    with pytest.raises(lib.FireflyError, match="title"):
        lib.save_cube(path, lut3, title='a "look"')
    with pytest.raises(lib.FireflyError) as e:
        lib.save_cube(str(tmp_path / "none" / "look.cube"), lut3)
    assert e.value.status == T.FF_ERR_IO


def test_hand_written_cube_files(tmp_path):
    path = str(tmp_path / "hand.cube")
    text3 = ('# a comment\r\nTITLE "hand made"\r\n\r\nLUT_3D_SIZE 2\r\nDOMAIN_MIN 0 0 0\r\nDOMAIN_MAX 1 2.0 4e0\r\n# red fastest\r\n'
             "0 0 0\r\n1 0 0\r\n0 1 0\r\n1 1 0\r\n  0 0 1  \r\n1 0 1\r\n0 1 1\r\n\t1 1 1\r\n\r\n# the end\r\n")
    open(path, "wb").write(text3.encode())
    lut, title = lib.load_cube(path)
    assert title == "hand made" and lut.desc.size == 2 and list(lut.desc.domain_max) == [1.0, 2.0, 4.0]
    k, j, i = np.meshgrid(np.arange(2), np.arange(2), np.arange(2), indexing="ij")
    assert np.array_equal(lut.table, np.stack([i, j, k], -1).astype(F))     # (an identity lattice: red fastest)
    px = np.array([[[0.25, 1.0, 3.0]]], F)
    assert np.array_equal(lib.color_grade_host(px, lib.grade_params(flags=R.LUT3D), lut)[1], np.array([[[0.25, 0.5, 0.75]]], F))
    text1 = "LUT_1D_SIZE 3\n# no title, the default domain, no line end after the last line\n0 0.5 1\n0.25 0.5 0.5\n1 0.5 0"
    open(path, "wb").write(text1.encode())
    lut, title = lib.load_cube(path)
    assert title == "" and lut.desc.curve_size == 3 and (lut.desc.curve_lo, lut.desc.curve_hi) == (0.0, 1.0)
    assert np.array_equal(lut.curves, np.array([[0, 0.25, 1], [0.5, 0.5, 0.5], [1, 0.5, 0]], F))   # (channel-major)
    px = np.array([[[0.25, 0.9, 0.75]]], F)
    assert np.array_equal(lib.color_grade_host(px, lib.grade_params(flags=R.CURVES), lut)[1], np.array([[[0.125, 0.5, 0.25]]], F))
    open(path, "wb").write(b'TITLE "shaped"\nDOMAIN_MIN -1 -1 -1\nDOMAIN_MAX 3 3 3\nLUT_1D_SIZE 2\n0 0 0\n1 1 1\n')
    lut, title = lib.load_cube(path)
    assert title == "shaped" and (lut.desc.curve_lo, lut.desc.curve_hi) == (-1.0, 3.0)


HEAD3 = "LUT_3D_SIZE 2\n"
ROWS8 = "0 0 0\n" * 8
MALFORMED = [
    ("", T.FF_ERR_INVALID_ARG, "neither LUT_1D_SIZE nor LUT_3D_SIZE"),
    (HEAD3 + "0 0 0\n" * 7, T.FF_ERR_IO, "ends after 7 of 8"),
    (HEAD3 + "0 0 0\n" * 9, T.FF_ERR_INVALID_ARG, "line 10: more than the 8"),
    (HEAD3 + "0 0\n" + ROWS8, T.FF_ERR_INVALID_ARG, "line 2: a data line wants three numbers"),
    (HEAD3 + "0 0 0 0\n" + ROWS8, T.FF_ERR_INVALID_ARG, "line 2: a data line wants three numbers"),
    (HEAD3 + "0 x 0\n" + ROWS8, T.FF_ERR_INVALID_ARG, "line 2: a data line wants three numbers"),
    (HEAD3 + "0 nan 0\n" + ROWS8, T.FF_ERR_INVALID_ARG, "line 2: a value that is not finite"),
    (HEAD3 + "inf 0 0\n" + ROWS8, T.FF_ERR_INVALID_ARG, "line 2: a value that is not finite"),
    (HEAD3 + "0 0 1e39\n" + ROWS8, T.FF_ERR_INVALID_ARG, "line 2: a value that is not finite"),
    (HEAD3 + "0 0 3e38\n" + "0 0 0\n" * 7, T.FF_ERR_INVALID_ARG, "FLT_MAX / 2"),
    ("0 0 0\n" + HEAD3 + ROWS8, T.FF_ERR_INVALID_ARG, "line 1: a data line before"),
    ("LUT_3D_SIZE 1\n0 0 0\n", T.FF_ERR_INVALID_ARG, "LUT_3D_SIZE 1 is outside 2 .. 65"),
    ("LUT_3D_SIZE 66\n", T.FF_ERR_INVALID_ARG, "LUT_3D_SIZE 66 is outside 2 .. 65"),
    ("LUT_1D_SIZE 4097\n", T.FF_ERR_INVALID_ARG, "LUT_1D_SIZE 4097 is outside 2 .. 4096"),
    ("LUT_3D_SIZE two\n", T.FF_ERR_INVALID_ARG, "LUT_3D_SIZE wants one integer"),
    ("LUT_3D_SIZE 2 2\n", T.FF_ERR_INVALID_ARG, "LUT_3D_SIZE wants one integer"),
    (HEAD3 + "LUT_1D_SIZE 2\n" + ROWS8, T.FF_ERR_INVALID_ARG, "line 2: a second size"),
    (HEAD3 + "0 0 0\nDOMAIN_MIN 0 0 0\n" + "0 0 0\n" * 7, T.FF_ERR_INVALID_ARG, "line 3: DOMAIN_MIN after the first data line"),
    ("DOMAIN_MIN 0 0\n" + HEAD3 + ROWS8, T.FF_ERR_INVALID_ARG, "line 1: DOMAIN_MIN wants three numbers"),
    ("DOMAIN_MAX 1 inf 1\n" + HEAD3 + ROWS8, T.FF_ERR_INVALID_ARG, "line 1: DOMAIN_MAX holds a value that is not finite"),
    ("DOMAIN_MIN 0 1 0\n" + HEAD3 + ROWS8, T.FF_ERR_INVALID_ARG, "DOMAIN_MIN 1 is not below DOMAIN_MAX 1"),
    ("DOMAIN_MIN 0 0.5 0\nLUT_1D_SIZE 2\n0 0 0\n1 1 1\n", T.FF_ERR_INVALID_ARG, "the same for r, g and b"),
    ("LUT_3D_INPUT_RANGE 0 1\n" + HEAD3 + ROWS8, T.FF_ERR_INVALID_ARG, "line 1: unknown keyword 'LUT_3D_INPUT_RANGE'"),
    ("TITLE look\n" + HEAD3 + ROWS8, T.FF_ERR_INVALID_ARG, "line 1: TITLE wants one"),
    ('TITLE "' + "x" * 128 + '"\n' + HEAD3 + ROWS8, T.FF_ERR_INVALID_ARG, "line 1: TITLE is longer than 127"),
]


@pytest.mark.parametrize("text,status,words", MALFORMED, ids=[m[2][:40] for m in MALFORMED])
def test_malformed_cube_files_name_what_is_wrong(tmp_path, text, status, words):
    path = str(tmp_path / "bad.cube")
    open(path, "wb").write(text.encode())
    f = T.FfCubeFile()
    assert lib.load().ff_load_cube(os.fsencode(path), C.byref(f)) == status
    assert words in last_error(), last_error()
    assert not f.lut.curves and not f.lut.table and f.lut.size == 0 and f.lut.curve_size == 0
    lib.load().ff_free_cube(C.byref(f))   # (an empty one is fine)


def test_cube_files_that_are_not_there():
    f = T.FfCubeFile()
    handle = lib.load()
    assert handle.ff_load_cube(b"/nonexistent/look.cube", C.byref(f)) == T.FF_ERR_IO and "cannot open" in last_error()
    assert handle.ff_load_cube(None, C.byref(f)) == T.FF_ERR_INVALID_ARG and handle.ff_load_cube(b"x.cube", None) == T.FF_ERR_INVALID_ARG
    assert handle.ff_save_cube(None, C.byref(f)) == T.FF_ERR_INVALID_ARG and handle.ff_save_cube(b"x.cube", None) == T.FF_ERR_INVALID_ARG
    handle.ff_free_cube(None)


# ---- argument checks ------------------------------------------------------------------------------------------------------------

def host_status(p, lut, rad, w=None, h=None, rgb8=None, out=None, rad_ptr=True):
    hh, ww = rad.shape[:2]
    return lib.load().ff_color_grade_host(C.byref(p) if p is not None else None, C.byref(lut.desc) if lut is not None else None, ww if w is None else w,
                                          hh if h is None else h, rad.ctypes.data if rad_ptr else None, rgb8, out)


def test_every_argument_check_of_the_call():
    lut = make_lut(3, 3, R.AXIS_LINEAR)
    rad = np.array(inputs(17, 15, lut))
    out = np.full((15, 17, 3), 7.0, F)
    o = out.ctypes.data
    bad_fields = [("flags", 16, "flags"), ("flags", 0x80000001, "flags"), ("reserved", 1, "reserved"), ("saturation", -0.5, "saturation"),
                  ("saturation", float("nan"), "saturation"), ("saturation", float("inf"), "saturation"),
                  ("matrix", (1, 0, 0, 0, float("inf"), 0, 0, 0, 1), "matrix[4]"), ("matrix", (1, 0, 0, 0, 1, 0, 0, 0, float("nan")), "matrix[8]"),
                  ("offset", (0, float("-inf"), 0), "offset[1]")]
    for field, value, word in bad_fields:
        for flags in (0, 7):   # (whether or not the stage runs)
            fields = dict(flags=flags)
            fields[field] = value
            assert host_status(lib.grade_params(**fields), lut, rad, out=o) == T.FF_ERR_INVALID_ARG and word in last_error(), (field, last_error())
    p = params(7)
    assert host_status(None, lut, rad, out=o) == T.FF_ERR_INVALID_ARG and "params" in last_error()
    assert host_status(p, lut, rad, out=o, rad_ptr=False) == T.FF_ERR_INVALID_ARG and "radiance_in" in last_error()
    for w, h in ((0, 15), (17, 0), (65536, 1), (-1, 15)):
        assert host_status(p, lut, rad, w=w, h=h, out=o) == T.FF_ERR_INVALID_ARG and "image size" in last_error()
    # a stage without its half
    for flags, use, word in ((R.CURVES, None, "lut is null"), (R.LUT3D, None, "lut is null"), (R.CURVES, make_lut(3, 0, 0), "no curves"),
                             (R.LUT3D, make_lut(0, 3, 0), "no lattice"), (R.PRIMARY | R.LUT3D | R.TRILINEAR, make_lut(0, 3, 0), "no lattice")):
        assert host_status(params(flags), use, rad, out=o) == T.FF_ERR_INVALID_ARG and word in last_error(), last_error()
    assert host_status(params(R.PRIMARY), None, rad, out=o) == T.FF_OK       # (no stage needs one)
    assert host_status(params(R.PRIMARY | R.TRILINEAR), None, rad, out=o) == T.FF_OK
    out[:] = 7.0
    # overlap: in place is fine, anything else is refused with nothing written
    n = rad.size
    src = rad.ctypes.data
    big8 = np.full(n + 64, 7, np.uint8)
    for rgb8, dst, word in ((None, src + 4, "radiance_out overlaps radiance_in"), (None, src - 4, "radiance_out overlaps radiance_in"),
                            (src + 4 * n - 1, None, "rgb8 overlaps radiance_in"), (src, src, "rgb8 overlaps radiance_in"),
                            (o + 8, o, "rgb8 overlaps radiance_out"), (o + 4 * n - 1, o, "rgb8 overlaps radiance_out")):
        before = rad.copy()
        assert host_status(p, lut, rad, rgb8=rgb8, out=dst) == T.FF_ERR_INVALID_ARG and word in last_error(), last_error()
        assert np.array_equal(R.bits(rad), R.bits(before)) and (out == 7.0).all()
    assert host_status(p, lut, rad, rgb8=big8.ctypes.data, out=src) == T.FF_OK
    assert_same((big8[:n].reshape(15, 17, 3), rad), R.color_grade(inputs(17, 15, lut), p, lut))
    assert (big8[n:] == 7).all()


def lut_status(**changes):
    base = make_lut(3, 3, R.AXIS_LINEAR)
    d = T.FfGradeLut()
    C.memmove(C.byref(d), C.byref(base.desc), C.sizeof(d))
    for k, v in changes.items():
        setattr(d, k, (C.c_float * 3)(*v) if k.startswith("domain") else v)
    rad = inputs(4, 4, base)
    p = lib.grade_params()
    return lib.load().ff_color_grade_host(C.byref(p), C.byref(d), 4, 4, rad.ctypes.data, None, None)


def test_every_check_of_the_lut_descriptor():
    lo, hi, shift = log_axis(3)
    cases = [(dict(curve_size=1), "curve_size 1 is outside 2 .. 4096"), (dict(curve_size=4097), "curve_size 4097"), (dict(curve_size=0), "curve_size 0 is outside"),
             (dict(curves=None), "curve_size 3 without curves"), (dict(curve_axis=2), "unknown curve_axis 2"), (dict(curve_lo=1.5), "curve_lo"),
             (dict(curve_lo=float("nan")), "curve_lo"), (dict(curve_hi=float("inf")), "curve_hi"), (dict(curve_lo=-3.0e38, curve_hi=3.0e38), "finite difference"),
             (dict(curve_shift=8), "curve_shift 8 must be 0"), (dict(size=1), "size 1 is outside 2 .. 65"), (dict(size=66), "size 66"),
             (dict(size=0), "size 0 is outside"), (dict(table=None), "size 3 without table"), (dict(domain_min=(0.0, 1.25, 0.0)), "domain_min[1]"),
             (dict(domain_max=(1.0, 1.0, float("nan"))), "domain_max[2]"), (dict(domain_min=(-3.0e38, 0, 0), domain_max=(3.0e38, 1, 1)), "domain_min[0]"),
             (dict(curve_axis=1, curve_lo=0.0, curve_hi=hi, curve_shift=shift), "curve_lo 0 must be > 0"),
             (dict(curve_axis=1, curve_lo=-0.25, curve_hi=hi, curve_shift=shift), "must be > 0"),
             (dict(curve_axis=1, curve_lo=lo, curve_hi=hi, curve_shift=7), "curve_shift 7 is outside 8 .. 23"),
             (dict(curve_axis=1, curve_lo=lo, curve_hi=hi, curve_shift=24), "curve_shift 24 is outside 8 .. 23"),
             (dict(curve_axis=1, curve_lo=0.3, curve_hi=hi, curve_shift=shift), "bits of curve_lo"),
             (dict(curve_axis=1, curve_lo=lo, curve_hi=0.75, curve_shift=shift), "bits of curve_lo"),
             (dict(curve_axis=1, curve_lo=lo, curve_hi=2.0, curve_shift=shift), "curve_size 3 is not the 4 knots"),
             (dict(curve_size=0, curves=None, size=0, table=None), "neither curves")]
    for changes, words in cases:
        assert lut_status(**changes) == T.FF_ERR_INVALID_ARG and words in last_error(), (changes, last_error())
    assert lut_status(curve_axis=1, curve_lo=lo, curve_hi=hi, curve_shift=shift) == T.FF_OK
    assert lut_status() == T.FF_OK
    # values
    for half, bad, words in (("curves", float("nan"), "knot 1 of channel 2"), ("curves", 2.0e38, "knot 1 of channel 2"), ("table", float("-inf"), "texel 13 channel 1"),
                             ("table", -2.0e38, "texel 13 channel 1")):
        base = make_lut(3, 3, R.AXIS_LINEAR)
        cv, tb = np.array(base.curves), np.array(base.table)
        if half == "curves":
            cv[2, 1] = bad
        else:
            tb.reshape(-1, 3)[13, 1] = bad
        lut = lib.grade_lut(curves=cv, curve_lo=0.0, curve_hi=1.0, table=tb)
        with pytest.raises(lib.FireflyError, match=words) as e:
            lib.color_grade_host(inputs(4, 4, base), lib.grade_params(), lut)
        assert e.value.status == T.FF_ERR_INVALID_ARG
