"""The part of the binding that needs no GPU and no ff_create: file readers and writers, the host tables and samplers the kernels'
tests compare against, the *_params builders, the host-only twin (*_host) of every image filter, and the private helpers these
share with tracer.Tracer - the input validators (_*_images) and the one output convention of the image calls (_image_outputs).
"""
import ctypes as C
import os

import numpy as np

from . import types as T
from ._abi import check, load


def load_obj(path):
    """LoadMesh (utilities.h:781-840) -> float32 [n, 24] triangles."""
    lib = load()
    ptr = C.POINTER(T.FfTriangle)()
    n = C.c_int(0)
    check(lib.ff_load_obj(os.fsencode(path), C.byref(ptr), C.byref(n)))
    try:
        return T.triangles_to_array(ptr, n.value)
    finally:
        lib.ff_free_triangles(ptr)


def save_ppm(path, rgb8):
    """saveToPPM (utilities.h:842-856) for an [H, W, 3] uint8 frame."""
    a = np.ascontiguousarray(rgb8, dtype=np.uint8)
    check(load().ff_save_ppm(os.fsencode(path), a.ctypes.data, a.shape[1], a.shape[0]))


class SceneFile:
    """A scene description file (ff_scene_file_load): exposes `.geometries` / `len()` like scenes.Scene."""

    def __init__(self, path):
        self._lib = load()
        self._handle = C.c_void_p()
        check(self._lib.ff_scene_file_load(os.fsencode(path), C.byref(self._handle)))
        n = C.c_int(0)
        self.geometries = self._lib.ff_scene_file_geometries(self._handle, C.byref(n))
        self._count = n.value

    def __len__(self):
        return self._count

    @property
    def triangle_count(self):
        return int(sum(self.geometries[i].m_numberOfTriangles for i in range(self._count)
                       if self.geometries[i].m_geometryType == T.GEOM_TRIANGLEMESH))

    def environment(self):
        """The file's environment statement as (resolved .hdr path, intensity, rotation in degrees), or None."""
        path, inten, rot = C.c_char_p(), C.c_float(0.0), C.c_float(0.0)
        if self._lib.ff_scene_file_environment(self._handle, C.byref(path), C.byref(inten), C.byref(rot)) == 0:
            return None
        return os.fsdecode(path.value), float(inten.value), float(rot.value)

    def textures(self):
        """The file's texture statements, in file order: a list of (name, resolved path, flags) with flags the T.TEX_* bits and
        T.SCENE_TEX_SRGB for `srgb`."""
        out = []
        for i in range(self._lib.ff_scene_file_texture_count(self._handle)):
            name, path, flags = C.c_char_p(), C.c_char_p(), C.c_int(0)
            check(self._lib.ff_scene_file_texture(self._handle, i, C.byref(name), C.byref(path), C.byref(flags)))
            out.append((name.value.decode(), os.fsdecode(path.value), int(flags.value)))
        return out

    def albedo_map(self, geometry_index):
        """Geometry `geometry_index`'s albedo_map as (index of its texture statement, (scale u, v), (offset u, v)), or None."""
        tex = C.c_int(-1)
        scale, offset = (C.c_float * 2)(), (C.c_float * 2)()
        if self._lib.ff_scene_file_albedo_map(self._handle, geometry_index, C.byref(tex), scale, offset) == 0:
            return None
        return int(tex.value), (float(scale[0]), float(scale[1])), (float(offset[0]), float(offset[1]))

    def roughness(self, geometry_index):
        """The `roughness` of geometry `geometry_index`'s mirror bxdf (ff_scene_file_roughness), or None."""
        r = C.c_float(0.0)
        if self._lib.ff_scene_file_roughness(self._handle, geometry_index, C.byref(r)) == 0:
            return None
        return float(r.value)

    def camera_sampling(self):
        """The camera statement's aperture / focus / filter keys as a T.FfCameraSampling (ff_scene_file_camera_sampling), or None
        if the file gives none of them.  Tracer.set_camera_sampling applies it."""
        cs = T.FfCameraSampling()
        if self._lib.ff_scene_file_camera_sampling(self._handle, C.byref(cs)) == 0:
            return None
        return cs

    def camera(self, width, height):
        cam = T.FfCamera()
        check(self._lib.ff_scene_file_camera(self._handle, width, height, C.byref(cam)))
        return cam

    def close(self):
        if self._handle:
            self._lib.ff_scene_file_free(self._handle)
            self._handle = C.c_void_p()
            self.geometries = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def scene_info(scene):
    """Host-only dry run of the scene compiler (sizes, BVH shape, structural self-check)."""
    info = T.FfSceneInfo()
    check(load().ff_scene_info(scene.geometries, len(scene), C.byref(info)))
    return info


def light_table(scene):
    """The light table FF_SHADE_DIFFUSE_PATH_NEE samples (host-only, ff_light_table): (entries, pdf_area) with entries a dict of
    numpy arrays - geometry, primitive, area, probability, v0, e1, e2, normal [n, 3], alias_probability, alias - and pdf_area the
    pdf per unit area of a light sample on each caller geometry (0 outside the table)."""
    lib = load()
    n = len(scene)
    count = lib.ff_light_table(scene.geometries, n, None, 0, None)
    if count < 0:
        check(-count)
    buf = (T.FfLightEntry * max(count, 1))()
    pdf = np.zeros(max(n, 1), dtype=np.float32)
    got = lib.ff_light_table(scene.geometries, n, buf, count, pdf.ctypes.data_as(C.POINTER(C.c_float)))
    if got < 0:
        check(-got)
    rows = list(buf)[:count]
    vec = lambda name: np.array([[getattr(r, name).x, getattr(r, name).y, getattr(r, name).z] for r in rows], dtype=np.float32).reshape(count, 3)
    entries = {name: np.array([getattr(r, name) for r in rows], dtype=np.int32) for name in ("geometry", "primitive", "alias")}
    entries.update({name: np.array([getattr(r, name) for r in rows], dtype=np.float32) for name in ("area", "probability", "alias_probability")})
    entries.update({name: vec(name) for name in ("v0", "e1", "e2", "normal")})
    return entries, pdf[:n]


def _env_map(rgb):
    a = np.ascontiguousarray(rgb, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"an environment map is an [H, W, 3] array (got shape {a.shape})")
    return a


def environment_table(rgb):
    """The sampling table ff_set_environment builds for an [H, W, 3] map (host-only, ff_environment_table): a dict of [H, W] arrays -
    probability (float32), alias_probability (float32), alias (int32, flat texel index r * W + c) and pdf (float32, per steradian)."""
    a = _env_map(rgb)
    h, w = a.shape[:2]
    out = {"probability": np.zeros((h, w), np.float32), "alias_probability": np.zeros((h, w), np.float32),
           "alias": np.zeros((h, w), np.int32), "pdf": np.zeros((h, w), np.float32)}
    check(load().ff_environment_table(a.ctypes.data, w, h, out["probability"].ctypes.data, out["alias_probability"].ctypes.data,
                                      out["alias"].ctypes.data, out["pdf"].ctypes.data))
    return out


def load_hdr(path):
    """A Radiance RGBE .hdr file (ff_load_hdr) -> float32 [H, W, 3], row 0 the top."""
    lib = load()
    ptr = C.POINTER(C.c_float)()
    w, h = C.c_int(0), C.c_int(0)
    check(lib.ff_load_hdr(os.fsencode(path), C.byref(ptr), C.byref(w), C.byref(h)))
    try:
        return np.ctypeslib.as_array(ptr, shape=(h.value * w.value * 3,)).reshape(h.value, w.value, 3).copy()
    finally:
        lib.ff_free_hdr(ptr)


def save_hdr(path, rgb):
    """float32 [H, W, 3] (finite, >= 0) -> a Radiance RGBE .hdr file with flat scanlines (ff_save_hdr), row 0 the top."""
    a = np.ascontiguousarray(rgb, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("an image is [H, W, 3]")
    check(load().ff_save_hdr(os.fsencode(path), a.ctypes.data, a.shape[1], a.shape[0]))


def _texture_image(rgb):
    a = np.ascontiguousarray(rgb, dtype=np.float32)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"a texture is an [H, W, 3] array (got shape {a.shape})")
    return a


def texture_sample(rgb, uv, flags=0):
    """The texel lookup of the kernels on the host (ff_texture_sample): [H, W, 3] texels (row 0 the top), lookup coordinates
    [..., 2], flags T.TEX_* -> float32 [..., 3]."""
    a = _texture_image(rgb)
    c = np.ascontiguousarray(uv, dtype=np.float32)
    if c.shape[-1:] != (2,):
        raise ValueError("coordinates are [..., 2]")
    out = np.zeros(c.shape[:-1] + (3,), dtype=np.float32)
    check(load().ff_texture_sample(a.ctypes.data, a.shape[1], a.shape[0], int(flags), c.ctypes.data, c.size // 2, out.ctypes.data))
    return out


def surface_uv(scene, geometry_index, world_points, triangle_indices=None):
    """The surface coordinate (before scale and offset) the kernels compute for world points [..., 3] on one geometry of a host
    scene (ff_surface_uv) -> float32 [..., 2].  triangle_indices [...]: each point's triangle, for a mesh."""
    p = np.ascontiguousarray(world_points, dtype=np.float32)
    if p.shape[-1:] != (3,):
        raise ValueError("points are [..., 3]")
    n = p.size // 3
    tri = None
    if triangle_indices is not None:
        tri = np.ascontiguousarray(triangle_indices, dtype=np.int32)
        if tri.size != n:
            raise ValueError("one triangle index per point")
    out = np.zeros(p.shape[:-1] + (2,), dtype=np.float32)
    check(load().ff_surface_uv(scene.geometries, len(scene), int(geometry_index), tri.ctypes.data if tri is not None else None,
                               p.ctypes.data, n, out.ctypes.data))
    return out


def _directions(a, name):
    d = np.ascontiguousarray(a, dtype=np.float32)
    if d.shape[-1:] != (3,):
        raise ValueError(f"{name} is [..., 3]")
    return d


def glossy_eval(alpha, f0, wo, wi):
    """The rough-specular lobe of the kernels on the host (ff_glossy_eval): unit local-frame directions wo, wi [..., 3] (z the normal)
    -> (f float32 [..., 3], the BRDF not times cosine; pdf float32 [...], the solid-angle pdf of wi under the sampler)."""
    o, i = _directions(wo, "wo"), _directions(wi, "wi")
    if o.shape != i.shape:
        raise ValueError("wo and wi have the same shape")
    f0 = np.ascontiguousarray(f0, dtype=np.float32).reshape(3)
    f = np.zeros(o.shape, dtype=np.float32)
    pdf = np.zeros(o.shape[:-1], dtype=np.float32)
    check(load().ff_glossy_eval(float(alpha), f0.ctypes.data, o.ctypes.data, i.ctypes.data, o.size // 3, f.ctypes.data, pdf.ctypes.data))
    return f, pdf


def glossy_sample(alpha, f0, wo, u):
    """The lobe's sampler on the host (ff_glossy_sample): wo [..., 3], u [..., 2] in [0, 1)^2 -> (wi float32 [..., 3], weight float32
    [..., 3] = F G2 / G1, pdf float32 [...]); weight and pdf are 0 for a wi at or below the horizon."""
    o = _directions(wo, "wo")
    uu = np.ascontiguousarray(u, dtype=np.float32)
    if uu.shape != o.shape[:-1] + (2,):
        raise ValueError("u is [..., 2], one pair per direction")
    f0 = np.ascontiguousarray(f0, dtype=np.float32).reshape(3)
    wi = np.zeros(o.shape, dtype=np.float32)
    weight = np.zeros(o.shape, dtype=np.float32)
    pdf = np.zeros(o.shape[:-1], dtype=np.float32)
    check(load().ff_glossy_sample(float(alpha), f0.ctypes.data, o.ctypes.data, uu.ctypes.data, o.size // 3, wi.ctypes.data, weight.ctypes.data,
                                  pdf.ctypes.data))
    return wi, weight, pdf


def camera_sampling(pixel_filter=T.PIXEL_CORNER, lens_radius=0.0, focus_distance=1.0):
    """A T.FfCameraSampling: ff_camera_sampling_init's defaults (today's camera) with the given fields replaced."""
    cs = T.FfCameraSampling()
    load().ff_camera_sampling_init(C.byref(cs))
    cs.pixel_filter, cs.lens_radius, cs.focus_distance = int(pixel_filter), float(lens_radius), float(focus_distance)
    return cs


def camera_sample_rays(camera, sampling, width, seed, xs, ys, samples, jitter=(0.0, 0.0)):
    """The kernel's per-sample camera rays on the host (ff_camera_sample_rays): sample samples[i] of pixel (xs[i], ys[i]) of an image
    `width` pixels wide under `seed` -> (origins float32 [n, 3], directions float32 [n, 3]).  sampling None: the defaults."""
    x = np.ascontiguousarray(xs, dtype=np.int32).reshape(-1)
    y = np.ascontiguousarray(ys, dtype=np.int32).reshape(-1)
    s = np.ascontiguousarray(samples, dtype=np.int32).reshape(-1)
    if not (x.shape == y.shape == s.shape):
        raise ValueError("xs, ys and samples have the same length")
    o = np.zeros((x.size, 3), dtype=np.float32)
    d = np.zeros((x.size, 3), dtype=np.float32)
    check(load().ff_camera_sample_rays(C.byref(camera), None if sampling is None else C.byref(sampling), float(jitter[0]), float(jitter[1]), int(width),
                                       int(seed), x.ctypes.data, y.ctypes.data, s.ctypes.data, x.size, o.ctypes.data, d.ctypes.data))
    return o, d


def load_ppm(path):
    """An 8-bit P3 or P6 PPM (ff_load_ppm) -> uint8 [H, W, 3], top row first."""
    lib = load()
    ptr = C.POINTER(C.c_ubyte)()
    w, h = C.c_int(0), C.c_int(0)
    check(lib.ff_load_ppm(os.fsencode(path), C.byref(ptr), C.byref(w), C.byref(h)))
    try:
        return np.ctypeslib.as_array(ptr, shape=(h.value * w.value * 3,)).reshape(h.value, w.value, 3).copy()
    finally:
        lib.ff_free_ppm(ptr)


def rgb8_to_linear(rgb8, srgb=True):
    """Bytes of any shape -> float32 texels (ff_rgb8_to_linear): the sRGB EOTF of ff_display, or b / 255 with srgb=False."""
    a = np.ascontiguousarray(rgb8, dtype=np.uint8)
    out = np.zeros(a.shape, dtype=np.float32)
    check(load().ff_rgb8_to_linear(a.ctypes.data, a.size, 1 if srgb else 0, out.ctypes.data))
    return out


def check_render_params(params):
    """ff_check_render_params: the status every render entry point's parameter check gives `params` (host-only)."""
    return load().ff_check_render_params(C.byref(params))


def render_params(width, height, bounces=1, spp=1, seed=1234, trace_mode=T.TRACE_BVH, shade_mode=T.SHADE_DIFFUSE_PATH,
                  grid_mode=T.GRID_FULL, spp_per_launch=0):
    return T.FfRenderParams(width, height, bounces, spp, seed, trace_mode, shade_mode, grid_mode, spp_per_launch)


def _params(struct, init, overrides, arrays=None, fixed=()):
    """What every *_params(**overrides) returns: a `struct` with the defaults of the library's `init` function and the given fields
    replaced.  arrays: field -> ctypes array type, for the fields given as a sequence; fixed: fields that may not be set."""
    p = struct()
    getattr(load(), init)(C.byref(p))
    fields = dict(struct._fields_)
    for name, value in overrides.items():
        if name not in fields or name in fixed:
            raise TypeError(f"{struct.__name__} has no {'settable ' if fixed else ''}field {name!r}")
        setattr(p, name, arrays[name](*value) if arrays and name in arrays else value)
    return p


def _or_default(p, builder):
    """The parameter struct `p`, or the defaults of its *_params `builder` where the caller gave none."""
    return p if p is not None else builder()


def _vp(q):
    """A raw pointer (an int; 0 or None: none) as ctypes passes it."""
    return C.c_void_p(q) if q else None


def _tail(on_device, rgb8_ptr, out_ptr):
    """The five arguments an image filter's C call ends in from the input's flag on: on_device, rgb8, on_device, out, on_device
    (on_device 0: host pointers, 1: device pointers).  tail[1:] is what a call without an input image, a render call, ends in."""
    return on_device, _vp(rgb8_ptr), on_device, _vp(out_ptr), on_device


def _image_outputs(h, w, want_rgb8=True, want_out=True, device=None, out=None):
    """The two optional outputs of an image call for an h x w image -> ((rgb8 [h,w,3] uint8, out [h,w,3] float32), their _tail):
    numpy arrays, or torch tensors on `device`; None for an output that is not wanted.  out: the array or tensor to use as the
    float output where one is wanted (an in-place call's).  A *_device method, whose caller owns the buffers, calls _tail itself."""
    if device is None:
        new, ptr = (lambda dtype: np.zeros((h, w, 3), dtype=dtype)), (lambda a: a.ctypes.data)
    else:
        import torch
        new, ptr = (lambda dtype: torch.zeros((h, w, 3), dtype=getattr(torch, dtype), device=device)), (lambda a: a.data_ptr())
    rgb8 = new("uint8") if want_rgb8 else None
    out = (out if out is not None else new("float32")) if want_out else None
    return (rgb8, out), _tail(0 if device is None else 1, ptr(rgb8) if want_rgb8 else None, ptr(out) if want_out else None)


def _host_outputs(h, w, want_rgb8=True, want_out=True, out=None):
    """_image_outputs for a *_host twin -> ((rgb8, out), (rgb8 pointer, out pointer)): its C call takes no on_device flags."""
    ret, tail = _image_outputs(h, w, want_rgb8, want_out, out=out)
    return ret, tail[1::2]


def _in_place(rad, in_place, want_out):
    """(source, out) of a filter call on the host array `rad`: an in-place call (radiance_out == radiance_in) writes over a copy
    of the input, and the copy is the source only when the float output is wanted."""
    if in_place and want_out:
        rad = rad.copy()
        return rad, rad
    return rad, None


def denoise_params(**overrides):
    """ff_denoise_params_init's defaults with the given fields replaced (iterations, sigma_color, sigma_normal, sigma_plane, flags)."""
    return _params(T.FfDenoiseParams, "ff_denoise_params_init", overrides)


def temporal_params(**overrides):
    """ff_temporal_params_init's defaults with the given fields replaced (any FfTemporalParams field)."""
    return _params(T.FfTemporalParams, "ff_temporal_params_init", overrides)


def taa_params(**overrides):
    """ff_taa_params_init's defaults with the given fields replaced (any FfTaaParams field)."""
    return _params(T.FfTaaParams, "ff_taa_params_init", overrides)


def upscale_params(**overrides):
    """ff_upscale_params_init's defaults with the given fields replaced (any FfUpscaleParams field; a jitter as a pair)."""
    return _params(T.FfUpscaleParams, "ff_upscale_params_init", overrides, arrays={"lo_jitter": C.c_float * 2, "hi_jitter": C.c_float * 2})


def taa_upscale_params(**overrides):
    """ff_taa_upscale_params_init's defaults with the given fields replaced (any FfTaaUpscaleParams field; lo_jitter as a pair)."""
    return _params(T.FfTaaUpscaleParams, "ff_taa_upscale_params_init", overrides, arrays={"lo_jitter": C.c_float * 2})


_GUIDE_PLANES = ("position", "normal", "albedo", "ids")


def _guides(gbuffer, names=_GUIDE_PLANES):
    """The named planes of a gbuffer() dict as contiguous arrays: ids int32, the others float32."""
    return {k: np.ascontiguousarray(gbuffer[k], dtype=np.int32 if k == "ids" else np.float32) for k in names}


def _upscale_images(radiance_lo, gbuffer_lo, gbuffer_hi, who):
    """The nine input images of ff_upscale as contiguous arrays, and (h, w), (H, W)."""
    rad = np.ascontiguousarray(radiance_lo, dtype=np.float32)
    lo, hi = _guides(gbuffer_lo), _guides(gbuffer_hi)
    h, w = rad.shape[:2]
    H, W = hi["ids"].shape[:2]
    if rad.shape != (h, w, 3) or any(a.shape != (h, w, 3) for a in lo.values()) or any(a.shape != (H, W, 3) for a in hi.values()):
        raise ValueError(f"{who}: radiance_lo and gbuffer_lo must be [h,w,3] and gbuffer_hi [H,W,3]")
    return rad, lo, hi, (h, w), (H, W)


def upscale_host(radiance_lo, gbuffer_lo, gbuffer_hi, p=None):
    """ff_upscale_host (no GPU): host radiance [h,w,3] with its gbuffer dict and the [H,W] gbuffer dict of the same view
    -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32)."""
    rad, lo, hi, (h, w), (H, W) = _upscale_images(radiance_lo, gbuffer_lo, gbuffer_hi, "upscale_host")
    p = _or_default(p, upscale_params)
    ret, outs = _host_outputs(H, W)
    check(load().ff_upscale_host(C.byref(p), w, h, rad.ctypes.data, *(lo[k].ctypes.data for k in _GUIDE_PLANES),
                                 W, H, *(hi[k].ctypes.data for k in _GUIDE_PLANES), *outs))
    return ret


def motion_blur_params(**overrides):
    """ff_motion_blur_params_init's defaults with the given fields replaced (any FfMotionBlurParams field)."""
    return _params(T.FfMotionBlurParams, "ff_motion_blur_params_init", overrides)


def _motion_blur_images(radiance, motion, depth, who):
    """The three input images of ff_motion_blur as contiguous float32 arrays, and (h, w)."""
    rad = np.ascontiguousarray(radiance, dtype=np.float32)
    mot = np.ascontiguousarray(motion, dtype=np.float32)
    dep = np.ascontiguousarray(depth, dtype=np.float32)
    h, w = rad.shape[:2]
    if rad.shape != (h, w, 3) or mot.shape != (h, w, 2) or dep.shape != (h, w):
        raise ValueError(f"{who}: radiance must be [H,W,3], motion [H,W,2] and depth [H,W]")
    return rad, mot, dep, (h, w)


def motion_blur_host(radiance, motion, depth, p=None, want_rgb8=True, want_out=True):
    """ff_motion_blur_host (no GPU): host radiance [H,W,3], motion [H,W,2] (a *_history call's) and depth [H,W] (gbuffer()'s)
    -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32)."""
    rad, mot, dep, (h, w) = _motion_blur_images(radiance, motion, depth, "motion_blur_host")
    p = _or_default(p, motion_blur_params)
    ret, outs = _host_outputs(h, w, want_rgb8, want_out)
    check(load().ff_motion_blur_host(w, h, C.byref(p), rad.ctypes.data, mot.ctypes.data, dep.ctypes.data, *outs))
    return ret


def dof_params(**overrides):
    """ff_dof_params_init's defaults with the given fields replaced (any FfDofParams field; reserved: a pair)."""
    return _params(T.FfDofParams, "ff_dof_params_init", overrides, arrays={"reserved": C.c_int32 * 2})


def dof_params_from_camera(camera, cs, **overrides):
    """dof_params(**overrides) with the focus_distance and coc_scale of the thin lens `cs` (lib.camera_sampling(...)) under
    `camera` (ff_dof_params_from_camera)."""
    p = dof_params(**overrides)
    check(load().ff_dof_params_from_camera(C.byref(camera), C.byref(cs), C.byref(p)))
    return p


def _dof_images(radiance, gbuffer_or_planes, who):
    """The three input images of ff_depth_of_field as contiguous float32 arrays, and (h, w).  gbuffer_or_planes: a gbuffer() dict
    or the pair (position [H,W,3], depth [H,W])."""
    position, depth = (gbuffer_or_planes["position"], gbuffer_or_planes["depth"]) if isinstance(gbuffer_or_planes, dict) else gbuffer_or_planes
    rad = np.ascontiguousarray(radiance, dtype=np.float32)
    pos = np.ascontiguousarray(position, dtype=np.float32)
    dep = np.ascontiguousarray(depth, dtype=np.float32)
    h, w = rad.shape[:2]
    if rad.shape != (h, w, 3) or pos.shape != (h, w, 3) or dep.shape != (h, w):
        raise ValueError(f"{who}: radiance and position must be [H,W,3] and depth [H,W]")
    return rad, pos, dep, (h, w)


def depth_of_field_host(radiance, gbuffer_or_planes, camera, p=None, want_rgb8=True, want_out=True):
    """ff_depth_of_field_host (no GPU): host radiance [H,W,3] and a gbuffer() dict of `camera` (or its (position, depth) planes)
    -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32)."""
    rad, pos, dep, (h, w) = _dof_images(radiance, gbuffer_or_planes, "depth_of_field_host")
    p = _or_default(p, dof_params)
    ret, outs = _host_outputs(h, w, want_rgb8, want_out)
    check(load().ff_depth_of_field_host(C.byref(camera), w, h, C.byref(p), rad.ctypes.data, pos.ctypes.data, dep.ctypes.data, *outs))
    return ret


def despeckle_params(**overrides):
    """ff_despeckle_params_init's defaults with the given fields replaced (any FfDespeckleParams field)."""
    return _params(T.FfDespeckleParams, "ff_despeckle_params_init", overrides)


def _despeckle_planes(gbuffer_or_planes):
    """(albedo, ids) of a gbuffer() dict or of the pair itself; albedo may be None (a frame judged without demodulation)."""
    if isinstance(gbuffer_or_planes, dict):
        return gbuffer_or_planes.get("albedo"), gbuffer_or_planes["ids"]
    return gbuffer_or_planes


def _despeckle_images(radiance, gbuffer_or_planes, who):
    """The three input images of ff_despeckle as contiguous arrays (albedo: None where none was given), and (h, w)."""
    albedo, ids = _despeckle_planes(gbuffer_or_planes)
    rad = np.ascontiguousarray(radiance, dtype=np.float32)
    alb = None if albedo is None else np.ascontiguousarray(albedo, dtype=np.float32)
    idp = np.ascontiguousarray(ids, dtype=np.int32)
    h, w = rad.shape[:2]
    if rad.shape != (h, w, 3) or idp.shape != (h, w, 3) or (alb is not None and alb.shape != (h, w, 3)):
        raise ValueError(f"{who}: radiance, albedo and ids must be [H,W,3]")
    return rad, alb, idp, (h, w)


def despeckle_host(radiance, gbuffer_or_planes, p=None, want_rgb8=True, want_out=True):
    """ff_despeckle_host (no GPU): host radiance [H,W,3] and a gbuffer() dict (or its (albedo, ids) planes; albedo None without
    FF_DESPECKLE_DEMODULATE_ALBEDO) -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32, the number of clamped pixels)."""
    rad, alb, ids, (h, w) = _despeckle_images(radiance, gbuffer_or_planes, "despeckle_host")
    p = _or_default(p, despeckle_params)
    ret, outs = _host_outputs(h, w, want_rgb8, want_out)
    clamped = C.c_uint32(0)
    check(load().ff_despeckle_host(w, h, C.byref(p), rad.ctypes.data, alb.ctypes.data if alb is not None else None, ids.ctypes.data,
                                   *outs, C.byref(clamped)))
    return (*ret, int(clamped.value))


def sharpen_params(**overrides):
    """ff_sharpen_params_init's defaults with the given fields replaced (any FfSharpenParams field)."""
    return _params(T.FfSharpenParams, "ff_sharpen_params_init", overrides)


def _float3_image(radiance, who):
    """An [H,W,3] input image (ff_sharpen's, ff_local_tonemap's, ff_encode_yuv's, ff_resize's, ff_color_grade's,
    ff_display's) as a contiguous float32
    array, and (h, w)."""
    rad = np.ascontiguousarray(radiance, dtype=np.float32)
    if rad.ndim != 3 or rad.shape[2] != 3:
        raise ValueError(f"{who}: radiance must be [H,W,3]")
    return rad, rad.shape[:2]


def sharpen_host(radiance, p=None, want_rgb8=True, want_out=True):
    """ff_sharpen_host (no GPU): host radiance [H,W,3] -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32)."""
    rad, (h, w) = _float3_image(radiance, "sharpen_host")
    p = _or_default(p, sharpen_params)
    ret, outs = _host_outputs(h, w, want_rgb8, want_out)
    check(load().ff_sharpen_host(w, h, C.byref(p), rad.ctypes.data, *outs))
    return ret


def local_tonemap_params(**overrides):
    """ff_local_tonemap_params_init's defaults with the given fields replaced (any FfLocalTonemapParams field but reserved)."""
    return _params(T.FfLocalTonemapParams, "ff_local_tonemap_params_init", overrides, fixed=("reserved",))


def local_tonemap_host(radiance, p=None, want_rgb8=True, want_out=True, in_place=False):
    """ff_local_tonemap_host (no GPU): host radiance [H,W,3] -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32).  in_place: the
    radiance output is written over a copy of the input (radiance_out == radiance_in in the call)."""
    rad, (h, w) = _float3_image(radiance, "local_tonemap_host")
    p = _or_default(p, local_tonemap_params)
    src, out = _in_place(rad, in_place, want_out)
    ret, outs = _host_outputs(h, w, want_rgb8, want_out, out)
    check(load().ff_local_tonemap_host(w, h, C.byref(p), src.ctypes.data, *outs))
    return ret


def local_tonemap_grid_host(radiance, p=None):
    """ff_local_tonemap_grid_host (no GPU): step 2's grid of host radiance [H,W,3] -> (n, S), each [gh, gw, 40] int32."""
    rad, (h, w) = _float3_image(radiance, "local_tonemap_grid_host")
    p = _or_default(p, local_tonemap_params)
    s = int(p.cell) if int(p.cell) > 0 else 1
    shape = ((h + s - 1) // s, (w + s - 1) // s, T.LOCAL_TONEMAP_BINS)
    n = np.zeros(shape, dtype=np.int32)
    S = np.zeros(shape, dtype=np.int32)
    check(load().ff_local_tonemap_grid_host(w, h, C.byref(p), rad.ctypes.data, n.ctypes.data, S.ctypes.data))
    return n, S


def yuv_params(**overrides):
    """ff_yuv_params_init's defaults with the given fields replaced (any FfYuvParams field)."""
    return _params(T.FfYuvParams, "ff_yuv_params_init", overrides)


def yuv_plane_bytes(width, height, p=None):
    """ff_yuv_plane_bytes -> (luma bytes, chroma bytes) of a width x height image under p."""
    p = _or_default(p, yuv_params)
    luma, chroma = C.c_uint64(0), C.c_uint64(0)
    check(load().ff_yuv_plane_bytes(width, height, C.byref(p), C.byref(luma), C.byref(chroma)))
    return int(luma.value), int(chroma.value)


def yuv_knots(transfer):
    """ff_yuv_knots -> K_0 .. K_4096 of a transfer, float32 [4097]."""
    out = np.zeros(T.YUV_KNOTS, dtype=np.float32)
    check(load().ff_yuv_knots(transfer, out.ctypes.data))
    return out


def _yuv_planes(h, w, p):
    """Empty host planes of ff_encode_yuv: luma [H,W] and chroma [ceil(H/2),ceil(W/2),2], uint8 at depth 8 and uint16 otherwise (a
    depth the library refuses gets uint16 planes: the call names it)."""
    dtype = np.uint8 if int(p.depth) == 8 else np.uint16
    return np.zeros((h, w), dtype=dtype), np.zeros(((h + 1) // 2, (w + 1) // 2, 2), dtype=dtype)


def encode_yuv_host(linear, p=None):
    """ff_encode_yuv_host (no GPU): host display-linear [H,W,3] -> (luma [H,W], chroma [ceil(H/2),ceil(W/2),2] of Cb Cr pairs);
    uint8 codes at depth 8 (NV12), uint16 codes << 6 at depth 10 (P010)."""
    img, (h, w) = _float3_image(linear, "encode_yuv_host")
    p = _or_default(p, yuv_params)
    luma, chroma = _yuv_planes(h, w, p)
    check(load().ff_encode_yuv_host(w, h, C.byref(p), img.ctypes.data, luma.ctypes.data, chroma.ctypes.data))
    return luma, chroma


def save_y4m(path, luma, chroma, p=None, append=False):
    """ff_save_y4m: one YUV4MPEG2 frame of encode_yuv's host planes; append=False writes the stream header first."""
    p = _or_default(p, yuv_params)
    dtype = np.uint8 if int(p.depth) == 8 else np.uint16
    lum = np.ascontiguousarray(luma, dtype=dtype)
    chr_ = np.ascontiguousarray(chroma, dtype=dtype)
    h, w = lum.shape[:2]
    if lum.ndim != 2 or chr_.shape != ((h + 1) // 2, (w + 1) // 2, 2):
        raise ValueError("save_y4m: luma must be [H,W] and chroma [ceil(H/2),ceil(W/2),2]")
    check(load().ff_save_y4m(os.fsencode(path), 1 if append else 0, w, h, C.byref(p), lum.ctypes.data, chr_.ctypes.data))


def resize_params(**overrides):
    """ff_resize_params_init's defaults with the given fields replaced (any FfResizeParams field)."""
    return _params(T.FfResizeParams, "ff_resize_params_init", overrides)


def resize_taps(in_size, out_size, filter):
    """ff_resize_taps -> T of an axis of in_size input and out_size output samples under filter."""
    taps = C.c_int(0)
    check(load().ff_resize_taps(in_size, out_size, filter, C.byref(taps)))
    return int(taps.value)


def resize_weights(in_size, out_size, filter):
    """ff_resize_weights -> (first int32 [out_size], weights float32 [out_size, T]) of one axis."""
    taps = resize_taps(in_size, out_size, filter)
    first = np.zeros(out_size, dtype=np.int32)
    weights = np.zeros((out_size, taps), dtype=np.float32)
    check(load().ff_resize_weights(in_size, out_size, filter, first.ctypes.data, weights.ctypes.data))
    return first, weights


def _resize_shape(out_width, out_height):
    """(rows, columns) of ff_resize's output arrays (a size the library refuses still gets arrays: the call names it)."""
    return max(int(out_height), 0), max(int(out_width), 0)


def resize_host(radiance, out_width, out_height, p=None, want_rgb8=True, want_out=True):
    """ff_resize_host (no GPU): host radiance [H,W,3] -> (rgb8 [H',W',3] uint8, radiance [H',W',3] float32)."""
    rad, (h, w) = _float3_image(radiance, "resize_host")
    p = _or_default(p, resize_params)
    ret, outs = _host_outputs(*_resize_shape(out_width, out_height), want_rgb8, want_out)
    check(load().ff_resize_host(C.byref(p), w, h, rad.ctypes.data, out_width, out_height, *outs))
    return ret


def grade_params(**overrides):
    """ff_grade_params_init's defaults with the given fields replaced (any FfGradeParams field; matrix a sequence of 9 row-major,
    offset of 3)."""
    return _params(T.FfGradeParams, "ff_grade_params_init", overrides, arrays={"matrix": C.c_float * 9, "offset": C.c_float * 3})


class GradeLut:
    """An FfGradeLut descriptor with the arrays it points to: .desc is what the library takes; .curves [3, K] and .table
    [N, N, N, 3] (indexed [b, g, r]: red fastest) are the float32 arrays, None for a half that is absent."""

    def __init__(self, desc, curves, table):
        self.desc, self.curves, self.table = desc, curves, table


def grade_lut(curves=None, curve_lo=0.0, curve_hi=1.0, curve_axis=T.GRADE_AXIS_LINEAR, curve_shift=0, table=None,
              domain_min=(0.0, 0.0, 0.0), domain_max=(1.0, 1.0, 1.0)):
    """A LUT descriptor (GradeLut) from curves [3, K] and / or a lattice table [N, N, N, 3] (or [N^3, 3], red fastest).  The sizes
    come from the arrays; nothing is checked here: the library names what it refuses."""
    d = T.FfGradeLut()
    cv = tb = None
    if curves is not None:
        cv = np.ascontiguousarray(curves, dtype=np.float32)
        if cv.ndim != 2 or cv.shape[0] != 3:
            raise ValueError("grade_lut: curves must be [3, K]")
        d.curve_size, d.curve_axis, d.curve_shift = cv.shape[1], curve_axis, curve_shift
        d.curve_lo, d.curve_hi = curve_lo, curve_hi
        d.curves = cv.ctypes.data
    if table is not None:
        tb = np.ascontiguousarray(table, dtype=np.float32)
        if tb.ndim == 2 and tb.shape[1] == 3:
            n = round(tb.shape[0] ** (1.0 / 3.0))
            if n ** 3 != tb.shape[0]:
                raise ValueError("grade_lut: a [M, 3] table must have M = N^3 rows")
            tb = tb.reshape(n, n, n, 3)
        if tb.ndim != 4 or tb.shape[3] != 3 or not (tb.shape[0] == tb.shape[1] == tb.shape[2]):
            raise ValueError("grade_lut: table must be [N, N, N, 3] or [N^3, 3]")
        d.size = tb.shape[0]
        d.domain_min = (C.c_float * 3)(*domain_min)
        d.domain_max = (C.c_float * 3)(*domain_max)
        d.table = tb.ctypes.data
    return GradeLut(d, cv, tb)


def _lut_ref(lut):
    return C.byref(lut.desc) if lut is not None else None


def color_grade_host(radiance, p=None, lut=None, want_rgb8=True, want_out=True, in_place=False):
    """ff_color_grade_host (no GPU): host radiance [H,W,3], a GradeLut or None -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32).
    in_place: the radiance output is written over a copy of the input (radiance_out == radiance_in in the call)."""
    rad, (h, w) = _float3_image(radiance, "color_grade_host")
    p = _or_default(p, grade_params)
    src, out = _in_place(rad, in_place, want_out)
    ret, outs = _host_outputs(h, w, want_rgb8, want_out, out)
    check(load().ff_color_grade_host(C.byref(p), _lut_ref(lut), w, h, src.ctypes.data, *outs))
    return ret


def load_cube(path):
    """ff_load_cube -> (GradeLut, title): a 1D .cube file as curves on the linear axis, a 3D one as the lattice."""
    lib = load()
    f = T.FfCubeFile()
    check(lib.ff_load_cube(os.fsencode(path), C.byref(f)))
    try:
        d = f.lut
        title = f.title.decode("utf-8", "replace")
        if d.curve_size:
            cv = np.ctypeslib.as_array(C.cast(d.curves, C.POINTER(C.c_float)), shape=(3, d.curve_size)).copy()
            return grade_lut(curves=cv, curve_lo=d.curve_lo, curve_hi=d.curve_hi), title
        n = d.size
        tb = np.ctypeslib.as_array(C.cast(d.table, C.POINTER(C.c_float)), shape=(n, n, n, 3)).copy()
        return grade_lut(table=tb, domain_min=tuple(d.domain_min), domain_max=tuple(d.domain_max)), title
    finally:
        lib.ff_free_cube(C.byref(f))


def save_cube(path, lut, title=""):
    """ff_save_cube: a GradeLut with exactly one half (curves on the linear axis, or the lattice) as a .cube file."""
    f = T.FfCubeFile()
    f.title = title.encode("utf-8")
    f.lut = lut.desc
    check(load().ff_save_cube(os.fsencode(path), C.byref(f)))


def lens_params(**overrides):
    """ff_lens_params_init's defaults (the identity) with the given fields replaced (any FfLensParams field)."""
    return _params(T.FfLensParams, "ff_lens_params_init", overrides)


def lens_host(radiance, p=None, want_rgb8=True, want_out=True):
    """ff_lens_host (no GPU): host radiance [H,W,3] -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32)."""
    rad, (h, w) = _float3_image(radiance, "lens_host")
    p = _or_default(p, lens_params)
    ret, outs = _host_outputs(h, w, want_rgb8, want_out)
    check(load().ff_lens_host(w, h, C.byref(p), rad.ctypes.data, *outs))
    return ret


def lens_tables(width, height, p=None):
    """ff_lens_tables -> (e float32 [LENS_KNOTS + 1], gain float32 [LENS_KNOTS + 1], r2_max) as the kernel gets them."""
    p = _or_default(p, lens_params)
    e = np.zeros(T.LENS_KNOTS + 1, dtype=np.float32)
    gain = np.zeros(T.LENS_KNOTS + 1, dtype=np.float32)
    r2_max = C.c_double(0.0)
    check(load().ff_lens_tables(C.byref(p), width, height, e.ctypes.data, gain.ctypes.data, C.byref(r2_max)))
    return e, gain, float(r2_max.value)


def lens_map(width, height, xy_out, p=None, channel=1):
    """ff_lens_map_host: output positions [n,2] (x y in pixels, a pixel's centre at + 0.5) -> the source positions float32 [n,2] of
    `channel` (0 red, 1 green, 2 blue)."""
    p = _or_default(p, lens_params)
    xy = np.ascontiguousarray(xy_out, dtype=np.float32)
    if xy.ndim != 2 or xy.shape[1] != 2:
        raise ValueError("lens_map: xy_out must be [n,2]")
    src = np.zeros_like(xy)
    check(load().ff_lens_map_host(C.byref(p), width, height, channel, xy.ctypes.data, xy.shape[0], src.ctypes.data))
    return src


def lens_fit_zoom(width, height, p=None, mode=T.LENS_FIT_FILL):
    """ff_lens_fit_zoom -> the zoom that fills the frame (LENS_FIT_FILL) or keeps the whole source in view (LENS_FIT_ALL)."""
    p = _or_default(p, lens_params)
    zoom = C.c_float(0.0)
    check(load().ff_lens_fit_zoom(C.byref(p), width, height, mode, C.byref(zoom)))
    return float(zoom.value)


def interpolate_params(**overrides):
    """ff_interpolate_params_init's defaults with the given fields replaced (any FfInterpolateParams field)."""
    return _params(T.FfInterpolateParams, "ff_interpolate_params_init", overrides)


def _interpolate_planes(gbuffer_or_planes):
    """(position, ids) of a gbuffer() dict or of the pair itself."""
    if isinstance(gbuffer_or_planes, dict):
        return gbuffer_or_planes["position"], gbuffer_or_planes["ids"]
    return gbuffer_or_planes


def _interpolate_images(mid, a, b, who):
    """The inputs of ff_interpolate: mid = (camera, gbuffer), a and b = (camera, radiance, gbuffer), a gbuffer being a gbuffer() dict
    or the pair (position, ids) -> the three cameras, the eight images as contiguous host arrays in the C call's order, and (h, w)."""
    cams = (mid[0], a[0], b[0])
    pos, ids = _interpolate_planes(mid[1])
    images = [np.ascontiguousarray(pos, dtype=np.float32), np.ascontiguousarray(ids, dtype=np.int32)]
    for src in (a, b):
        pos, ids = _interpolate_planes(src[2])
        images += [np.ascontiguousarray(src[1], dtype=np.float32), np.ascontiguousarray(pos, dtype=np.float32), np.ascontiguousarray(ids, dtype=np.int32)]
    shape = images[0].shape
    if len(shape) != 3 or shape[2] != 3 or any(im.shape != shape for im in images):
        raise ValueError(f"{who}: every image must be [H,W,3] and of one size")
    return cams, images, shape[:2]


def _interpolate_maps(geom_maps, who):
    """geom_maps as a contiguous float32 [n,2,3,4] array (None stays None) and n."""
    if geom_maps is None:
        return None, 0
    maps = np.ascontiguousarray(geom_maps, dtype=np.float32)
    if maps.ndim != 4 or maps.shape[1:] != (2, 3, 4):
        raise ValueError(f"{who}: geom_maps must be [n,2,3,4]")
    return maps, maps.shape[0]


def interpolate_host(mid, a, b, p=None, geom_maps=None, want_rgb8=True, want_out=True):
    """ff_interpolate_host (no GPU): mid = (camera, gbuffer), a and b = (camera, radiance [H,W,3], gbuffer), a gbuffer being a gbuffer()
    dict or the pair (position, ids); geom_maps [n,2,3,4] or None
    -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32, counts [5] uint32: both, A only, B only, filled, fallback)."""
    cams, im, (h, w) = _interpolate_images(mid, a, b, "interpolate_host")
    maps, n = _interpolate_maps(geom_maps, "interpolate_host")
    p = _or_default(p, interpolate_params)
    ret, outs = _host_outputs(h, w, want_rgb8, want_out)
    counts = np.zeros(5, dtype=np.uint32)
    d = [x.ctypes.data for x in im]
    check(load().ff_interpolate_host(w, h, C.byref(p), C.byref(cams[0]), d[0], d[1], C.byref(cams[1]), d[2], d[3], d[4], C.byref(cams[2]), d[5], d[6], d[7],
                                     maps.ctypes.data if maps is not None else None, n, *outs, counts.ctypes.data))
    return (*ret, counts)


def interpolate_geometry_maps(mid, a, b):
    """ff_interpolate_geometry_maps (no GPU): the model matrices of a scene's n geometries at the three poses - each either a ctypes
    array of FfGeometry or an [n,16] array of column-major matrices (FfGeometry.m_modelMatrix) -> (geom_maps [n,2,3,4] float32,
    identity flags [n,2] int32)."""
    def geometries(x):
        if isinstance(x, C.Array) and x._type_ is T.FfGeometry:
            return x
        m = np.ascontiguousarray(x, dtype=np.float32)
        if m.ndim != 2 or m.shape[1] != 16:
            raise ValueError("interpolate_geometry_maps: model matrices must be [n,16]")
        g = (T.FfGeometry * max(m.shape[0], 1))()
        for i in range(m.shape[0]):
            g[i].m_modelMatrix.m[:] = [float(v) for v in m[i]]
        return g if m.shape[0] else None
    gm, ga, gb = geometries(mid), geometries(a), geometries(b)
    n = len(gm) if gm is not None else 0
    if any(len(x) != n for x in (ga, gb) if x is not None):
        raise ValueError("interpolate_geometry_maps: the three poses must have as many geometries")
    maps = np.zeros((max(n, 1), 2, 3, 4), dtype=np.float32)
    flags = np.zeros((max(n, 1), 2), dtype=np.int32)
    check(load().ff_interpolate_geometry_maps(gm, ga, gb, n, maps.ctypes.data, flags.ctypes.data))
    return maps[:n], flags[:n]


def adaptive_params(**overrides):
    """ff_adaptive_params_init's defaults with the given fields replaced (any FfAdaptiveParams field)."""
    return _params(T.FfAdaptiveParams, "ff_adaptive_params_init", overrides)


def _adaptive_sums(sum_all, sum_even, who):
    """The two sum planes of the tile error as contiguous float32 [H,W,3] arrays, and (h, w)."""
    a = np.ascontiguousarray(sum_all, dtype=np.float32)
    b = np.ascontiguousarray(sum_even, dtype=np.float32)
    h, w = a.shape[:2]
    if a.shape != (h, w, 3) or b.shape != (h, w, 3):
        raise ValueError(f"{who}: sum and sum_even must be [H,W,3]")
    return a, b, (h, w)


def adaptive_tile_grid(width, height, tile):
    """(tiles_y, tiles_x) of ff_render_adaptive's tile grid."""
    return (height + tile - 1) // tile, (width + tile - 1) // tile


def adaptive_tile_error_host(sum_all, sum_even, tile, n):
    """ff_adaptive_tile_error_host (no GPU): the running sums [H,W,3] after n passes -> E_t per tile, float32 [tiles_y, tiles_x]."""
    a, b, (h, w) = _adaptive_sums(sum_all, sum_even, "adaptive_tile_error_host")
    out = np.zeros(adaptive_tile_grid(w, h, tile) if tile > 0 else (1, 1), dtype=np.float32)
    check(load().ff_adaptive_tile_error_host(w, h, tile, n, a.ctypes.data, b.ctypes.data, out.ctypes.data))
    return out


def adaptive_plan_host(active, max_rects=None):
    """ff_adaptive_plan_host: a [tiles_y, tiles_x] array of flags -> the driver's rectangles, int32 [n, 4] of {tx0, ty0, tx1, ty1} in
    tiles (half open).  max_rects: the room offered (default: one per tile); a list that does not fit raises."""
    flags = np.ascontiguousarray(np.asarray(active) != 0, dtype=np.uint8)
    ty, tx = flags.shape
    room = flags.size if max_rects is None else max_rects
    out = np.zeros((max(room, 1), 4), dtype=np.int32)
    n = load().ff_adaptive_plan_host(tx, ty, flags.ctypes.data, out.ctypes.data, room)
    if n < 0:
        check(T.FF_ERR_INVALID_ARG)
    return out[:n].copy()


def display_params(**overrides):
    """ff_display_params_init's defaults with the given fields replaced (any FfDisplayParams field)."""
    return _params(T.FfDisplayParams, "ff_display_params_init", overrides)


def srgb_thresholds():
    """ff_srgb_thresholds: T_1 .. T_255 of FF_ENCODE_SRGB, float32 [255]."""
    out = np.zeros(255, dtype=np.float32)
    check(load().ff_srgb_thresholds(out.ctypes.data))
    return out


def display_curve(p, exposed):
    """ff_display_curve: tone curve and encoding of p for exposed values of any shape -> (y float32, bytes uint8), same shape."""
    e = np.ascontiguousarray(exposed, dtype=np.float32)
    y = np.zeros(e.shape, dtype=np.float32)
    b = np.zeros(e.shape, dtype=np.uint8)
    check(load().ff_display_curve(C.byref(p), e.ctypes.data, e.size, y.ctypes.data, b.ctypes.data))
    return y, b


def display_exposure(p, histogram, previous_exposure=0.0):
    """ff_display_exposure: (target, exposure) of a 256-bin histogram; previous_exposure <= 0: there is none."""
    h = np.ascontiguousarray(histogram, dtype=np.uint32)
    if h.shape != (T.DISPLAY_BINS,):
        raise ValueError("the histogram has 256 bins")
    target, exposure = C.c_float(), C.c_float()
    check(load().ff_display_exposure(C.byref(p), h.ctypes.data, previous_exposure, C.byref(target), C.byref(exposure)))
    return target.value, exposure.value


def jitter_sequence(index, period=16):
    """ff_jitter_sequence: the (jx, jy) of frame `index` of a Halton(2, 3) cycle of `period` jitters."""
    jx, jy = C.c_float(), C.c_float()
    check(load().ff_jitter_sequence(index, period, C.byref(jx), C.byref(jy)))
    return jx.value, jy.value


def camera_ray_matrix_jittered(camera, jx, jy):
    """ff_camera_ray_matrix_jittered -> T.FfMat4."""
    m = T.FfMat4()
    load().ff_camera_ray_matrix_jittered(C.byref(camera), jx, jy, C.byref(m))
    return m
