"""ff_gbuffer / ff_denoise on the host side: exports, defaults, argument checks (all before any device work) and the numpy
reference of the filter that the GPU tests compare against."""
import ctypes as C

import numpy as np
import pytest

from gpupathtracer_amd import lib
from gpupathtracer_amd import types as T
from gbuffer_ref import denoise_ref, filterable


def test_new_entry_points_are_exported(ff):
    handle = ff.load()
    for name in ("ff_gbuffer", "ff_denoise_params_init", "ff_denoise"):
        assert name in ff.EXPORTS
        assert hasattr(handle, name), name


def test_denoise_params_defaults():
    dn = lib.denoise_params()
    assert dn.iterations == 5
    assert dn.flags == T.DENOISE_SAME_GEOMETRY | T.DENOISE_DEMODULATE_ALBEDO
    assert dn.sigma_color > 0 and dn.sigma_normal > 0 and dn.sigma_plane > 0
    assert C.sizeof(T.FfDenoiseParams) == 20
    assert lib.denoise_params(iterations=2, sigma_color=0.5).iterations == 2
    with pytest.raises(TypeError):
        lib.denoise_params(sigma=1.0)


def _buf(n, dtype=np.float32):
    return np.zeros(n, dtype=dtype)


def test_invalid_arguments_are_refused_before_any_device_work(ff):
    handle = ff.load()
    state = C.c_void_p(0x1)  # never dereferenced: every check below fails before the state is used
    W, H = 8, 4
    rad, pos, nrm, alb = (_buf(W * H * 3) for _ in range(4))
    ids = _buf(W * H * 3, np.int32)
    out = _buf(W * H * 3)

    def denoise(st=state, w=W, h=H, dn=None, r=rad, p=pos, n=nrm, a=alb, i=ids):
        dn = lib.denoise_params() if dn is None else dn
        ptr = lambda x: x.ctypes.data if x is not None else None  # noqa: E731
        return handle.ff_denoise(st, w, h, C.byref(dn), ptr(r), ptr(p), ptr(n), ptr(a), ptr(i), 0, None, 0, out.ctypes.data, 0)

    assert denoise(st=None) == T.FF_ERR_INVALID_ARG
    assert denoise(w=0) == T.FF_ERR_INVALID_ARG
    assert denoise(h=-3) == T.FF_ERR_INVALID_ARG
    assert denoise(dn=lib.denoise_params(iterations=-1)) == T.FF_ERR_INVALID_ARG
    assert denoise(dn=lib.denoise_params(iterations=11)) == T.FF_ERR_INVALID_ARG
    assert denoise(dn=lib.denoise_params(sigma_color=0.0)) == T.FF_ERR_INVALID_ARG
    assert denoise(dn=lib.denoise_params(sigma_plane=float("nan"))) == T.FF_ERR_INVALID_ARG
    assert denoise(dn=lib.denoise_params(flags=8)) == T.FF_ERR_INVALID_ARG
    for missing in ("r", "p", "n", "i", "a"):
        assert denoise(**{missing: None}) == T.FF_ERR_INVALID_ARG, missing
    assert handle.ff_denoise(state, W, H, None, rad.ctypes.data, pos.ctypes.data, nrm.ctypes.data, alb.ctypes.data, ids.ctypes.data, 0,
                             None, 0, out.ctypes.data, 0) == T.FF_ERR_INVALID_ARG
    assert "ff_denoise" in handle.ff_last_error().decode()

    cam = T.FfCamera()
    handle.ff_camera_init_default(C.byref(cam), W, H)
    depth = _buf(W * H)

    def gbuffer(st=state, p=None, c=cam):
        p = lib.render_params(W, H) if p is None else p
        return handle.ff_gbuffer(st, C.byref(c) if c is not None else None, C.byref(p), depth.ctypes.data, pos.ctypes.data, nrm.ctypes.data,
                                 alb.ctypes.data, ids.ctypes.data, 0)

    assert gbuffer(st=None) == T.FF_ERR_INVALID_ARG
    assert gbuffer(c=None) == T.FF_ERR_INVALID_ARG
    assert gbuffer(p=lib.render_params(0, H)) == T.FF_ERR_INVALID_ARG
    assert gbuffer(p=lib.render_params(W, -1)) == T.FF_ERR_INVALID_ARG
    assert handle.ff_gbuffer(state, C.byref(cam), None, None, None, None, None, None, 0) == T.FF_ERR_INVALID_ARG


def _random_gbuffer(rng, H, W, geoms=3):
    """A G-buffer of a few tilted planes with some misses, emitters and mirrors among them."""
    ids = np.full((H, W, 3), -1, np.int32)
    g = rng.integers(0, geoms, size=(H, W))
    ids[..., 0] = g
    ids[..., 1] = -1
    ids[..., 2] = T.BXDF_DIFFUSE
    ids[rng.random((H, W)) < 0.05] = -1
    ids[(rng.random((H, W)) < 0.05) & (ids[..., 0] >= 0), 2] = T.BXDF_MIRROR
    ids[(rng.random((H, W)) < 0.03) & (ids[..., 0] >= 0), 2] = T.BXDF_EMITTER
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    normals = np.array([[0, 0, 1], [0, 1, 0.2], [1, 0, 0]], dtype=np.float64)
    pos = np.stack([xx * 0.01, yy * 0.01, 0.02 * g], -1)
    nrm = normals[g] * 1.7  # (not unit length: the filter normalises)
    alb = rng.uniform(0.0, 1.0, size=(H, W, 3))
    alb[..., 1] = np.where(rng.random((H, W)) < 0.1, 0.0, alb[..., 1])  # channels with albedo 0 stay undivided
    return {"ids": ids, "position": pos.astype(np.float32), "normal": nrm.astype(np.float32), "albedo": alb.astype(np.float32)}


@pytest.mark.parametrize("flags", [0, T.DENOISE_SAME_GEOMETRY, T.DENOISE_DEMODULATE_ALBEDO, T.DENOISE_SAME_GEOMETRY | T.DENOISE_DEMODULATE_ALBEDO])
def test_numpy_reference_scales_and_passes_through(flags):
    rng = np.random.default_rng(11)
    H, W = 24, 40
    gb = _random_gbuffer(rng, H, W)
    rad = rng.exponential(0.5, size=(H, W, 3)) * (rng.random((H, W, 3)) < 0.7)
    out = denoise_ref(rad, gb, 4, 0.8, 0.2, 0.3, flags)
    # scaling the radiance by k scales the output by k
    out4 = denoise_ref(4.0 * rad, gb, 4, 0.8, 0.2, 0.3, flags)
    assert np.allclose(out4, 4.0 * out, rtol=1e-12, atol=0)
    # pixels that are not filterable are copied through exactly
    keep = ~filterable(gb["ids"])
    assert keep.any() and np.array_equal(out[keep], rad[keep])
    # iterations = 0 is the identity; filtering changes the filterable pixels
    assert np.array_equal(denoise_ref(rad, gb, 0, 0.8, 0.2, 0.3, flags), rad)
    assert not np.allclose(out[~keep], rad[~keep])
    # a constant (demodulated) colour per geometry comes back
    const = np.array([[0.3, 0.2, 0.1], [1.0, 2.0, 3.0], [0.5, 0.5, 0.5]])[np.maximum(gb["ids"][..., 0], 0)]
    if flags & T.DENOISE_DEMODULATE_ALBEDO:
        a = gb["albedo"].astype(np.float64)
        const = np.where(a > 0, const * a, const)
    same = denoise_ref(const, gb, 4, 0.8, 0.2, 0.3, flags | T.DENOISE_SAME_GEOMETRY)
    assert np.allclose(same, const, rtol=1e-12, atol=0)
