"""ff_taa_upscale without a GPU: the parameter defaults and the exported symbols, and the reconstruction property of the float64
reference (tests/taa_upscale_ref.py) that the GPU tests then hold the kernel to: at rest, a cycle of jittered low-resolution
frames hands every high pixel the low sample whose ray is its own."""
import ctypes as C

import numpy as np

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
from taa_upscale_ref import BLEND, FIRST, HOLD, SPATIAL, TaaUpscaleRef

IDENTITY = (np.eye(4), np.eye(4))


def test_defaults_and_exports():
    names = ["ff_taa_upscale_params_init", "ff_taa_upscale", "ff_taa_upscale_reset", "ff_taa_upscale_history"]
    handle = lib.load()
    for name in names:
        assert name in lib.EXPORTS and hasattr(handle, name), name
    assert C.sizeof(T.FfTaaUpscaleParams) == T.TAA_UPSCALE_PARAMS_BYTES == 24
    p = T.FfTaaUpscaleParams(alpha_min=9.0, gamma=9.0, lo_jitter=(C.c_float * 2)(0.5, 0.5), flags=7, reserved=7)
    handle.ff_taa_upscale_params_init(C.byref(p))
    assert (p.alpha_min, p.gamma, tuple(p.lo_jitter), p.flags, p.reserved) == (np.float32(0.1), 1.0, (0.0, 0.0), 0, 0)
    q, t = lib.taa_upscale_params(), lib.taa_params()
    assert (q.alpha_min, q.gamma, q.flags) == (t.alpha_min, t.gamma, t.flags)  # (ff_taa's)
    q = lib.taa_upscale_params(lo_jitter=(0.25, 0.5), flags=T.TAA_NO_CLAMP)
    assert tuple(q.lo_jitter) == (0.25, 0.5) and q.flags == T.TAA_NO_CLAMP
    try:
        lib.taa_upscale_params(sigma=1.0)
    except TypeError:
        pass
    else:
        raise AssertionError("an unknown field must be refused")


def _target(W, H, seed):
    """A seeded image in [0.5, 1) (float32) and seeded ids: four geometries, one of them a miss, two bxdf types."""
    rng = np.random.default_rng(seed)
    target = rng.uniform(0.5, 1.0, size=(H, W, 3)).astype(np.float32)
    geom = rng.integers(-1, 3, size=(H, W))
    ids = np.stack([geom, np.zeros_like(geom), np.where(geom < 0, -1, geom % 2)], -1).astype(np.int32)
    return target, {"ids": ids, "position": rng.uniform(-1, 1, size=(H, W, 3)).astype(np.float32)}


def test_the_reference_rebuilds_the_target_from_a_cycle_of_jittered_low_frames():
    """Factor 2: low frame (a, b) is target[b::2, a::2] under jitter (a/2, b/2): its pixel i went through high pixel 2 i + a.  u, dx and
    k are exact, so after the four frames the image is the target bit for bit with every length 1 (NO_CLAMP), and after call t the
    parity classes visited so far are.  (From the second call on a pixel's first sample meets the spatial estimate the first call
    stored with length 0: alpha = 1 and o = h + (c - h), which is c whenever c - h is exact.)  Factor 3 (63 x 36, nine frames under jitters (a/3, b/3)): 1/3 is not a float32, so k is 1
    up to ~1e-6 on the pixel's own sample and up to ~3e-6 (half an ulp of u = 20.33, times the factor) instead of 0 on the two
    neighbours a third of a low pixel away; the target lies in [0.5, 1), so a neighbour's sample differs from the pixel's own by at
    most the pixel's own value, and the weighted mean is the target to well within rtol 1e-5."""
    W, H = 64, 36
    target, gb = _target(W, H, 11)
    cam = scenes.posed_camera(W, H, position=(0.0, 0.0, 2.4), yaw=-90.0, pitch=0.0)
    ref = TaaUpscaleRef()
    done = np.zeros((H, W), bool)
    for cycle in range(2):
        for b in range(2):
            for a in range(2):
                p = lib.taa_upscale_params(lo_jitter=(a / 2, b / 2), flags=T.TAA_NO_CLAMP)
                r = ref.step(target[b::2, a::2], gb["ids"][b::2, a::2], gb, cam, [IDENTITY] * 3, p)
                own = np.zeros((H, W), bool)
                own[b::2, a::2] = True
                assert np.array_equal(r["k"], own.astype(np.float32))
                if cycle == 0 and (a, b) == (0, 0):
                    assert (r["case"][own] == FIRST).all() and (r["case"][~own] == SPATIAL).all()
                else:
                    assert (r["case"][own] == BLEND).all()
                    assert (r["case"][~own & done] == HOLD).all() and (r["case"][~own & ~done] == SPATIAL).all()
                done |= own
                assert np.array_equal(r["out"][done], target.astype(np.float64)[done])
                assert not r["tainted"].any() and not r["motion"].any()
        assert done.all() and np.array_equal(r["out"], target.astype(np.float64))
        assert (r["length"] == cycle + 1).all()
    # factor 3
    W, H = 63, 36
    target, gb = _target(W, H, 12)
    cam = scenes.posed_camera(W, H, position=(0.0, 0.0, 2.4), yaw=-90.0, pitch=0.0)
    ref = TaaUpscaleRef()
    for b in range(3):
        for a in range(3):
            p = lib.taa_upscale_params(lo_jitter=(a / 3, b / 3), flags=T.TAA_NO_CLAMP)
            r = ref.step(target[b::3, a::3], gb["ids"][b::3, a::3], gb, cam, [IDENTITY] * 3, p)
    err = np.abs(r["out"] - target) / target
    print(f"factor 3: largest relative error {err.max():.3g}, lengths {r['length'].min():.7f} .. {r['length'].max():.7f}")
    assert np.allclose(r["out"], target, rtol=1e-5, atol=0)
    assert np.allclose(r["length"], 1.0, rtol=1e-5, atol=0)


def test_the_reference_rebuilds_the_target_from_sixteen_quarter_resolution_frames():
    """Factor 4, 68 x 36 from 17 x 9 (tiles cut on both edges): low frame (a, b) is target[b::4, a::4] under jitter (a/4, b/4).
    u = (X * 17) / 68 - a/4 is exactly X/4 - a/4 in float32, so k is 1 on the pixel's own sample and 0 on every other (|dx| >= 1/4:
    the tent, one high pixel wide, is 0 there), and the argument of the factor-2 cycle holds phase by phase: after the sixteen
    frames the image is the target bit for bit with every length 1, and a second cycle brings every length to 2."""
    W, H, F = 68, 36, 4
    target, gb = _target(W, H, 13)
    cam = scenes.posed_camera(W, H, position=(0.0, 0.0, 2.4), yaw=-90.0, pitch=0.0)
    ref = TaaUpscaleRef()
    done = np.zeros((H, W), bool)
    for cycle in range(2):
        for b in range(F):
            for a in range(F):
                p = lib.taa_upscale_params(lo_jitter=(a / F, b / F), flags=T.TAA_NO_CLAMP)
                r = ref.step(target[b::F, a::F], gb["ids"][b::F, a::F], gb, cam, [IDENTITY] * 3, p)
                own = np.zeros((H, W), bool)
                own[b::F, a::F] = True
                assert np.array_equal(r["k"], own.astype(np.float32))
                if cycle == 0 and (a, b) == (0, 0):
                    assert (r["case"][own] == FIRST).all() and (r["case"][~own] == SPATIAL).all()
                else:
                    assert (r["case"][own] == BLEND).all()
                    assert (r["case"][~own & done] == HOLD).all() and (r["case"][~own & ~done] == SPATIAL).all()
                done |= own
                assert np.array_equal(r["out"][done], target.astype(np.float64)[done])
                assert not r["tainted"].any() and not r["motion"].any()
        assert done.all() and np.array_equal(r["out"], target.astype(np.float64))
        assert (r["length"] == cycle + 1).all()
