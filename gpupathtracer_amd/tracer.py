"""The part of the binding that needs a GPU: ``Tracer`` (one FfState on one HIP device: upload once, render per frame, then the
image pipeline), ``MultiTracer`` (several GPUs, one process) and the ff_dist_* helpers.  An image filter's method is its validation
plus one C call; what the calls share - the host-array / device-tensor dispatch and the output convention - is in _filter,
_run_filter and host._image_outputs.
"""
import ctypes as C

import numpy as np

from . import types as T
from ._abi import check, load
from .host import (_adaptive_sums, _despeckle_images, _despeckle_planes, _dof_images, _env_map, _float3_image, _guides, _image_outputs, _in_place,
                   _interpolate_images, _interpolate_maps, _motion_blur_images, _or_default, _resize_shape, _tail, _texture_image, _upscale_images,
                   _vp, _yuv_planes, adaptive_params, adaptive_tile_grid, denoise_params, despeckle_params, display_params, dof_params,
                   grade_params, interpolate_params, lens_params, local_tonemap_params, motion_blur_params, resize_params, sharpen_params,
                   taa_params, taa_upscale_params, temporal_params, upscale_params, yuv_params, yuv_plane_bytes)

DIST_ID_BYTES = 128

GBUFFER_CHANNELS = (("depth", np.float32, ()), ("position", np.float32, (3,)), ("normal", np.float32, (3,)), ("albedo", np.float32, (3,)),
                    ("ids", np.int32, (3,)))


# the eight values of ff_debug_layout, in order
LAYOUT_FIELDS = ("scene_block_threads", "stack_entries", "stack_lds_levels", "lds_cap", "setup_threshold", "leaf_threshold", "max_depth4", "top_depth")


def _device_image(t, dtype, what, spelled, hw=None):
    """(h, w) of the device tensor `t`, which must be contiguous, on the device, of the torch `dtype` and [H,W,3] (of the size hw,
    where one is given); what and spelled: the tensor and its type as the error names them."""
    h, w = hw if hw is not None else t.shape[:2]
    if not t.is_cuda or t.dtype != dtype or tuple(t.shape) != (h, w, 3) or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous [H,W,3] {spelled} tensor on the device")
    return h, w


def _run_filter(call, images, size, out_size, want_rgb8, want_out, device=None, out=None):
    """One image-filter call on checked inputs -> (rgb8, out) as _image_outputs makes them for out_size.  images: the input images
    of `size`, host arrays (device None) or tensors on `device` (None: an image that is absent); call(w, h, *their pointers, tail)
    makes the C call and returns its status.  Work queued on `device` is waited for first: the library runs on its own stream."""
    ret, tail = _image_outputs(*out_size, want_rgb8, want_out, device, out)
    if device is None:
        ptrs = [a.ctypes.data if a is not None else None for a in images]
    else:
        import torch
        torch.cuda.synchronize(device)
        ptrs = [_vp(t.data_ptr()) if t is not None else None for t in images]
    check(call(size[1], size[0], *ptrs, tail))
    return ret


def _filter(who, radiance, call, want_rgb8, want_out, in_place=False, out_size=None):
    """A single-image filter (`who` names it in errors) of radiance [H,W,3]: a host array gives host arrays, a contiguous float32
    device tensor (torch) gives device tensors -> (rgb8, out).  call(w, h, radiance pointer, tail): see _run_filter.  in_place:
    radiance_out is radiance_in in the call - a device tensor is overwritten and returned, a host array is copied first.
    out_size: (rows, columns) of the outputs where they differ from the input's."""
    if hasattr(radiance, "data_ptr"):
        import torch
        size = _device_image(radiance, torch.float32, f"{who}: radiance", "float32")
        src, out, device = radiance, (radiance if in_place else None), radiance.device
    else:
        rad, size = _float3_image(radiance, who)
        (src, out), device = _in_place(rad, in_place, want_out), None
    return _run_filter(call, (src,), size, out_size or size, want_rgb8, want_out, device, out)


class Tracer:
    """Owner of one FfState (one HIP device). Mirrors the call sequence of the reference's main():
    upload once (kernel.cu:268-298), then render per frame (kernel.cu:335-344)."""

    def __init__(self, device_id=0):
        self._lib = load()
        self._state = C.c_void_p()
        check(self._lib.ff_create(C.byref(self._state), device_id))
        self._scene_keepalive = None
        # (h, w) of the last call of each filter that keeps a history (what its *_history call returns)
        self._temporal_size = self._taa_size = self._taa_upscale_size = (0, 0)

    def close(self):
        if self._state:
            self._lib.ff_destroy(self._state)
            self._state = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream_ptr):
        check(self._lib.ff_set_stream(self._state, C.c_void_p(hip_stream_ptr)))

    def upload_scene(self, scene):
        """scene: gpupathtracer_amd.scenes.Scene"""
        check(self._lib.ff_upload_scene(self._state, scene.geometries, len(scene)))

    def set_environment(self, rgb, intensity=1.0, rotation_deg=0.0):
        """Light the scene with an [H, W, 3] environment map (row 0 the top, +Y), `intensity` times its texels, turned by
        `rotation_deg` about +Y (ff_set_environment).  It stays until clear_environment(), across scene uploads."""
        a = _env_map(rgb)
        check(self._lib.ff_set_environment(self._state, a.ctypes.data, a.shape[1], a.shape[0], float(intensity), float(rotation_deg)))

    def clear_environment(self):
        check(self._lib.ff_set_environment(self._state, None, 0, 0, 0.0, 0.0))

    def create_texture(self, rgb, flags=0):
        """Copy an [H, W, 3] float32 texture (linear RGB, row 0 the top) to the device (ff_texture_create) -> its id.  flags:
        T.TEX_REPEAT or T.TEX_CLAMP, T.TEX_BILINEAR or T.TEX_NEAREST.  It stays until destroy_texture(), across scene uploads."""
        a = _texture_image(rgb)
        tid = C.c_int(-1)
        check(self._lib.ff_texture_create(self._state, a.ctypes.data, a.shape[1], a.shape[0], int(flags), C.byref(tid)))
        return tid.value

    def destroy_texture(self, texture_id):
        """ff_texture_destroy: frees the texture and unbinds it wherever it is bound."""
        check(self._lib.ff_texture_destroy(self._state, int(texture_id)))

    def set_albedo_texture(self, geometry_index, texture_id, scale=(1.0, 1.0), offset=(0.0, 0.0)):
        """Bind a texture to a diffuse geometry's albedo (ff_set_albedo_texture): albedo = m_albedo * texel(uv * scale + offset);
        texture_id -1 (or None) unbinds.  Bindings last until the next upload_scene."""
        check(self._lib.ff_set_albedo_texture(self._state, int(geometry_index), -1 if texture_id is None else int(texture_id),
                                              float(scale[0]), float(scale[1]), float(offset[0]), float(offset[1])))

    def set_roughness(self, geometry_index, roughness):
        """Make a mirror geometry a rough (GGX) conductor of this roughness in [0, 1], F0 = its m_specularColor (ff_set_roughness);
        0 (or None) unbinds.  Bindings last until the next upload_scene."""
        check(self._lib.ff_set_roughness(self._state, int(geometry_index), 0.0 if roughness is None else float(roughness)))

    def set_camera_sampling(self, sampling=None):
        """ff_set_camera_sampling: a T.FfCameraSampling (lib.camera_sampling(...)) for the following render* calls - T.PIXEL_BOX draws
        a point of the pixel per sample, lens_radius > 0 a point of a thin lens focused at focus_distance; None: the defaults (today's
        camera).  The setting stays through upload_scene and the update calls."""
        check(self._lib.ff_set_camera_sampling(self._state, None if sampling is None else C.byref(sampling)))

    def apply_scene_file_materials(self, scene_file):
        """After upload_scene(scene_file): bind every `roughness` of the file's mirror bxdfs (the file's albedo_maps need their images
        loaded and created first: textures(), albedo_map(), create_texture(), set_albedo_texture())."""
        for g in range(len(scene_file)):
            r = scene_file.roughness(g)
            if r is not None:
                self.set_roughness(g, r)

    def set_builder(self, builder):
        """T.BUILD_HOST_SAH (default) or T.BUILD_GPU_LBVH for the following upload_scene calls."""
        check(self._lib.ff_set_builder(self._state, builder))

    def update_transforms(self, scene):
        """Same geometries as uploaded, new transforms / materials: rewrites the per-geometry records only."""
        check(self._lib.ff_update_transforms(self._state, scene.geometries, len(scene)))

    def update_mesh(self, geometry_index, triangles, mode=T.UPDATE_REFIT):
        """New vertices (float32 [n, 24], as load_obj returns) for one uploaded mesh: refit or rebuild its tree on the device."""
        buf = T.triangles_from_array(triangles)
        check(self._lib.ff_update_mesh(self._state, geometry_index, buf, len(buf), mode))

    def build_stats(self):
        st = T.FfBuildStats()
        check(self._lib.ff_build_stats(self._state, C.byref(st)))
        return st

    def download_bvh(self, num_geometries):
        """(nodes, triangle records, mesh table) of the compiled scene (tests).  mesh table: int32 [num_geometries, 5] =
        bvh_root, node_count, tri_first, tri_count, depth per uploaded geometry."""
        nn, nt = C.c_int(0), C.c_int(0)
        check(self._lib.ff_debug_download_bvh(self._state, None, 0, C.byref(nn), None, 0, C.byref(nt), None, 0))
        nodes = np.zeros(max(nn.value, 1), dtype=T.BVH_NODE_DTYPE)
        tris = np.zeros(max(nt.value, 1), dtype=T.TRI_RECORD_DTYPE)
        table = np.full((num_geometries, 5), -1, dtype=np.int32)
        check(self._lib.ff_debug_download_bvh(self._state, nodes.ctypes.data, nn.value, C.byref(nn), tris.ctypes.data, nt.value, C.byref(nt),
                                              table.ctypes.data_as(C.POINTER(C.c_int)), num_geometries))
        return nodes[:nn.value], tris[:nt.value], table

    def download_bvh4(self, num_geometries):
        """(4-wide nodes [capacity] with fields mn[3][4], mx[3][4], link[4]; table int32 [num_geometries, 6] = first node, node
        count, depth, first LDS slot, nodes in LDS, LDS node slots)."""
        cap = C.c_int(0)
        check(self._lib.ff_debug_download_bvh4(self._state, None, 0, C.byref(cap), None, 0))
        nodes = np.zeros(max(cap.value, 1), dtype=T.BVH4_NODE_DTYPE)
        table = np.full((num_geometries, 6), -1, dtype=np.int32)
        check(self._lib.ff_debug_download_bvh4(self._state, nodes.ctypes.data, cap.value, C.byref(cap),
                                               table.ctypes.data_as(C.POINTER(C.c_int)), num_geometries))
        return nodes[:cap.value], table

    def set_collect_stats(self, on):
        check(self._lib.ff_set_collect_stats(self._state, 1 if on else 0))

    def stats(self):
        st = T.FfStats()
        check(self._lib.ff_stats(self._state, C.byref(st)))
        return st

    def kernel_name(self):
        """Trace-kernel instantiation of the last frame, as rocprofv3 names it."""
        return self._lib.ff_debug_kernel_name(self._state).decode()

    def debug_layout(self):
        """ff_debug_layout: what the next BVH launch on the uploaded scene will use -> dict of ints (LAYOUT_FIELDS)."""
        buf = (C.c_int * 8)()
        check(self._lib.ff_debug_layout(self._state, buf))
        return dict(zip(LAYOUT_FIELDS, (int(v) for v in buf)))

    def reset_stack_spill(self):
        """ff_debug_stack_spill(reset): fill the traversal stacks' global spill area, if there is one, with the sentinel word."""
        n = C.c_ulonglong(0)
        check(self._lib.ff_debug_stack_spill(self._state, 1, C.byref(n)))

    def stack_spill_words(self):
        """ff_debug_stack_spill: words of the spill area that differ from the sentinel (0 where there is no area)."""
        n = C.c_ulonglong(0)
        check(self._lib.ff_debug_stack_spill(self._state, 0, C.byref(n)))
        return int(n.value)

    def check_ieee(self):
        """(reciprocal mismatches, square-root mismatches) of the kernels' lean IEEE sequences over all 2^32 floats."""
        buf = (C.c_ulonglong * 2)()
        check(self._lib.ff_debug_check_ieee(self._state, buf))
        return int(buf[0]), int(buf[1])

    def reload_switches(self):
        """Re-read the FF_* experiment switches from the environment (they are read once, at ff_create)."""
        check(self._lib.ff_debug_reload_switches(self._state))

    def debug_counters(self):
        buf = (C.c_ulonglong * 32)()
        check(self._lib.ff_debug_counters(self._state, buf))
        return list(buf)

    def debug_timeline(self):
        """(bucket_us, counts[1024]): rays completed per wall-clock bucket of the last instrumented launch (FF_DEBUG_TIMELINE_US)."""
        buf = (C.c_uint * 1024)()
        us = C.c_int(0)
        check(self._lib.ff_debug_timeline(self._state, buf, C.byref(us)))
        return int(us.value), np.frombuffer(buf, dtype=np.uint32).copy()

    def render(self, camera, params, want_rgb8=True, want_radiance=True):
        """Headless frame to host numpy arrays: (rgb8 [H,W,3] uint8, radiance [H,W,3] float32)."""
        ret, tail = _image_outputs(params.height, params.width, want_rgb8, want_radiance)
        check(self._lib.ff_render(self._state, C.byref(camera), C.byref(params), *tail[1:]))
        return ret

    def render_progressive(self, camera, params, frame_index):
        """Frame `frame_index` of a progressive sequence -> (rgb8, radiance) of the mean over frames 0..frame_index."""
        ret, tail = _image_outputs(params.height, params.width)
        check(self._lib.ff_render_progressive(self._state, C.byref(camera), C.byref(params), frame_index, *tail[1:]))
        return ret

    def render_tile(self, camera, params, x0, y0, w, h):
        """Tile [x0, x0+w) x [y0, y0+h) of the frame -> (rgb8 [h,w,3], radiance [h,w,3])."""
        ret, tail = _image_outputs(h, w)
        check(self._lib.ff_render_tile(self._state, C.byref(camera), C.byref(params), x0, y0, w, h, *tail[1:]))
        return ret

    def render_adaptive(self, camera, params, ap=None):
        """ff_render_adaptive: passes of params.spp samples (seed, seed + 1, ...) until every tile's error estimate is below
        ap.threshold -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32, passes [H,W] uint16, FfAdaptiveInfo)."""
        ap = _or_default(ap, adaptive_params)
        ret, tail = _image_outputs(params.height, params.width)
        passes = np.zeros((params.height, params.width), dtype=np.uint16)
        info = T.FfAdaptiveInfo()
        check(self._lib.ff_render_adaptive(self._state, C.byref(camera), C.byref(params), C.byref(ap), *tail[1:], passes.ctypes.data, 0, C.byref(info)))
        return (*ret, passes, info)

    def render_adaptive_device(self, camera, params, ap=None, rgb8_ptr=None, radiance_ptr=None, passes_ptr=None):
        """ff_render_adaptive into caller-owned DEVICE buffers (raw pointers; each may be None) -> FfAdaptiveInfo."""
        ap = _or_default(ap, adaptive_params)
        info = T.FfAdaptiveInfo()
        check(self._lib.ff_render_adaptive(self._state, C.byref(camera), C.byref(params), C.byref(ap), *_tail(1, rgb8_ptr, radiance_ptr)[1:],
                                           _vp(passes_ptr), 1, C.byref(info)))
        return info

    def adaptive_state(self, width, height, tile):
        """ff_adaptive_state of the last render_adaptive call (its size and tile edge are the caller's to give) -> dict of numpy
        arrays: sum / sum_even [H,W,3] float32, tile_passes [tiles_y,tiles_x] uint16, tile_error [tiles_y,tiles_x] float32."""
        grid = adaptive_tile_grid(width, height, tile)
        out = {"sum": np.zeros((height, width, 3), dtype=np.float32), "sum_even": np.zeros((height, width, 3), dtype=np.float32),
               "tile_passes": np.zeros(grid, dtype=np.uint16), "tile_error": np.zeros(grid, dtype=np.float32)}
        check(self._lib.ff_adaptive_state(self._state, out["sum"].ctypes.data, out["sum_even"].ctypes.data, out["tile_passes"].ctypes.data,
                                          out["tile_error"].ctypes.data, 0))
        return out

    def adaptive_tile_error(self, sum_all, sum_even, tile, n):
        """ff_adaptive_tile_error (the device kernel on planted sums): host sums [H,W,3] after n passes -> E_t per tile, float32
        [tiles_y, tiles_x]."""
        a, b, (h, w) = _adaptive_sums(sum_all, sum_even, "adaptive_tile_error")
        out = np.zeros(adaptive_tile_grid(w, h, tile) if tile > 0 else (1, 1), dtype=np.float32)
        check(self._lib.ff_adaptive_tile_error(self._state, w, h, tile, n, a.ctypes.data, b.ctypes.data, 0, out.ctypes.data))
        return out

    def render_device(self, camera, params, rgb8_ptr=None, radiance_ptr=None):
        """Headless frame into caller-owned DEVICE buffers (raw pointers, e.g. torch tensor.data_ptr())."""
        check(self._lib.ff_render(self._state, C.byref(camera), C.byref(params), *_tail(1, rgb8_ptr, radiance_ptr)[1:]))

    def gbuffer(self, camera, params):
        """What every pixel's primary ray hits (ff_gbuffer) -> dict of numpy arrays: depth [H,W] float32, position / normal / albedo
        [H,W,3] float32, ids [H,W,3] int32 (geometry, triangle, bxdf type; -1 on a miss)."""
        h, w = params.height, params.width
        out = {name: np.zeros((h, w) + shape, dtype=dt) for name, dt, shape in GBUFFER_CHANNELS}
        check(self._lib.ff_gbuffer(self._state, C.byref(camera), C.byref(params), *(out[name].ctypes.data for name, _, _ in GBUFFER_CHANNELS), 0))
        return out

    def gbuffer_device(self, camera, params, depth_ptr=None, position_ptr=None, normal_ptr=None, albedo_ptr=None, ids_ptr=None):
        """ff_gbuffer into caller-owned DEVICE buffers (raw pointers; any may be None)."""
        check(self._lib.ff_gbuffer(self._state, C.byref(camera), C.byref(params), _vp(depth_ptr), _vp(position_ptr), _vp(normal_ptr), _vp(albedo_ptr),
                                   _vp(ids_ptr), 1))

    def denoise(self, radiance, gbuffer, dn=None):
        """ff_denoise of host radiance [H,W,3] guided by a gbuffer() dict -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32)."""
        rad = np.ascontiguousarray(radiance, dtype=np.float32)
        h, w = rad.shape[:2]
        dn = _or_default(dn, denoise_params)
        g = _guides(gbuffer)
        ret, tail = _image_outputs(h, w)
        check(self._lib.ff_denoise(self._state, w, h, C.byref(dn), rad.ctypes.data, g["position"].ctypes.data, g["normal"].ctypes.data,
                                   g["albedo"].ctypes.data, g["ids"].ctypes.data, *tail))
        return ret

    def denoise_device(self, width, height, radiance_ptr, position_ptr, normal_ptr, albedo_ptr, ids_ptr, dn=None, rgb8_ptr=None, radiance_out_ptr=None):
        """ff_denoise on DEVICE buffers (raw pointers); radiance_out_ptr may equal radiance_ptr."""
        dn = _or_default(dn, denoise_params)
        check(self._lib.ff_denoise(self._state, width, height, C.byref(dn), _vp(radiance_ptr), _vp(position_ptr), _vp(normal_ptr), _vp(albedo_ptr),
                                   _vp(ids_ptr), *_tail(1, rgb8_ptr, radiance_out_ptr)))

    def denoise_temporal(self, radiance, gbuffer, camera, tp=None):
        """ff_denoise_temporal of this frame's host radiance [H,W,3] guided by gbuffer() of `camera`; the history stays in the state
        -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32)."""
        rad = np.ascontiguousarray(radiance, dtype=np.float32)
        h, w = rad.shape[:2]
        if rad.shape != (h, w, 3) or any(np.shape(gbuffer[k])[:2] != (h, w) for k in ("position", "normal", "albedo", "ids")):
            raise ValueError("denoise_temporal: radiance must be [H,W,3] and the G-buffer of the same size")
        tp = _or_default(tp, temporal_params)
        g = _guides(gbuffer)
        ret, tail = _image_outputs(h, w)
        check(self._lib.ff_denoise_temporal(self._state, C.byref(camera), w, h, C.byref(tp), rad.ctypes.data, g["position"].ctypes.data,
                                            g["normal"].ctypes.data, g["albedo"].ctypes.data, g["ids"].ctypes.data, *tail))
        self._temporal_size = (h, w)
        return ret

    def denoise_temporal_device(self, camera, width, height, radiance_ptr, position_ptr, normal_ptr, albedo_ptr, ids_ptr, tp=None, rgb8_ptr=None,
                                radiance_out_ptr=None):
        """ff_denoise_temporal on DEVICE buffers (raw pointers); radiance_out_ptr may equal radiance_ptr."""
        tp = _or_default(tp, temporal_params)
        check(self._lib.ff_denoise_temporal(self._state, C.byref(camera), width, height, C.byref(tp), _vp(radiance_ptr), _vp(position_ptr),
                                            _vp(normal_ptr), _vp(albedo_ptr), _vp(ids_ptr), *_tail(1, rgb8_ptr, radiance_out_ptr)))
        self._temporal_size = (height, width)

    def temporal_reset(self):
        """Drop the temporal history (ff_temporal_reset)."""
        check(self._lib.ff_temporal_reset(self._state))

    def _history(self, fn, size):
        """What the three *_history calls return: (motion [H,W,2] float32, history length [H,W] float32) of the filter's last call,
        whose (H, W) is `size`; fn: the filter's ff_*_history."""
        h, w = size
        motion = np.zeros((h, w, 2), dtype=np.float32)
        length = np.zeros((h, w), dtype=np.float32)
        check(fn(self._state, motion.ctypes.data if h * w else None, length.ctypes.data if h * w else None, 0))
        return motion, length

    def temporal_history(self):
        """The last denoise_temporal call's (motion [H,W,2] float32, history length [H,W] float32)."""
        return self._history(self._lib.ff_temporal_history, self._temporal_size)

    def set_pixel_jitter(self, jx, jy):
        """ff_set_pixel_jitter: the following render* and gbuffer calls trace pixel (x, y) through (x + jx, y + jy)."""
        check(self._lib.ff_set_pixel_jitter(self._state, jx, jy))

    def taa(self, radiance, gbuffer, camera, p=None):
        """ff_taa of this frame's host radiance [H,W,3] with gbuffer() of `camera` (same jitter); the history stays in the state
        -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32)."""
        rad = np.ascontiguousarray(radiance, dtype=np.float32)
        h, w = rad.shape[:2]
        if rad.shape != (h, w, 3) or any(np.shape(gbuffer[k])[:2] != (h, w) for k in ("position", "ids")):
            raise ValueError("taa: radiance must be [H,W,3] and the G-buffer of the same size")
        p = _or_default(p, taa_params)
        g = _guides(gbuffer, ("position", "ids"))
        ret, tail = _image_outputs(h, w)
        check(self._lib.ff_taa(self._state, C.byref(camera), w, h, C.byref(p), rad.ctypes.data, g["position"].ctypes.data, g["ids"].ctypes.data, *tail))
        self._taa_size = (h, w)
        return ret

    def taa_device(self, camera, width, height, radiance_ptr, position_ptr, ids_ptr, p=None, rgb8_ptr=None, radiance_out_ptr=None):
        """ff_taa on DEVICE buffers (raw pointers); radiance_out_ptr may equal radiance_ptr."""
        p = _or_default(p, taa_params)
        check(self._lib.ff_taa(self._state, C.byref(camera), width, height, C.byref(p), _vp(radiance_ptr), _vp(position_ptr), _vp(ids_ptr),
                               *_tail(1, rgb8_ptr, radiance_out_ptr)))
        self._taa_size = (height, width)

    def taa_reset(self):
        """Drop the TAA history (ff_taa_reset)."""
        check(self._lib.ff_taa_reset(self._state))

    def taa_history(self):
        """The last taa call's (motion [H,W,2] float32, history length [H,W] float32)."""
        return self._history(self._lib.ff_taa_history, self._taa_size)

    def upscale(self, radiance_lo, gbuffer_lo, gbuffer_hi, p=None):
        """ff_upscale of host radiance [h,w,3] with its gbuffer() dict, guided by the [H,W] gbuffer() dict of the same view (p: the
        jitters both were made with) -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32)."""
        rad, lo, hi, (h, w), (H, W) = _upscale_images(radiance_lo, gbuffer_lo, gbuffer_hi, "upscale")
        p = _or_default(p, upscale_params)
        ret, tail = _image_outputs(H, W)
        check(self._lib.ff_upscale(self._state, C.byref(p), w, h, rad.ctypes.data, lo["position"].ctypes.data, lo["normal"].ctypes.data,
                                   lo["albedo"].ctypes.data, lo["ids"].ctypes.data, W, H, hi["position"].ctypes.data, hi["normal"].ctypes.data,
                                   hi["albedo"].ctypes.data, hi["ids"].ctypes.data, *tail))
        return ret

    def upscale_device(self, lo_width, lo_height, radiance_lo_ptr, position_lo_ptr, normal_lo_ptr, albedo_lo_ptr, ids_lo_ptr, width, height, position_ptr,
                       normal_ptr, albedo_ptr, ids_ptr, p=None, rgb8_ptr=None, radiance_out_ptr=None):
        """ff_upscale on DEVICE buffers (raw pointers); the outputs must not overlap an input."""
        p = _or_default(p, upscale_params)
        check(self._lib.ff_upscale(self._state, C.byref(p), lo_width, lo_height, _vp(radiance_lo_ptr), _vp(position_lo_ptr), _vp(normal_lo_ptr),
                                   _vp(albedo_lo_ptr), _vp(ids_lo_ptr), width, height, _vp(position_ptr), _vp(normal_ptr), _vp(albedo_ptr), _vp(ids_ptr),
                                   *_tail(1, rgb8_ptr, radiance_out_ptr)))

    def taa_upscale(self, radiance_lo, gbuffer_lo, gbuffer_hi, camera, p=None):
        """ff_taa_upscale of this frame's host radiance [h,w,3], rendered under p.lo_jitter, with the ids of its gbuffer() (same
        jitter) and the position and ids of the unjittered [H,W] gbuffer() of `camera` (the W x H pose); the history stays in the
        state -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32)."""
        rad = np.ascontiguousarray(radiance_lo, dtype=np.float32)
        ids_lo = np.ascontiguousarray(gbuffer_lo["ids"], dtype=np.int32)
        pos = np.ascontiguousarray(gbuffer_hi["position"], dtype=np.float32)
        ids = np.ascontiguousarray(gbuffer_hi["ids"], dtype=np.int32)
        h, w = rad.shape[:2]
        H, W = ids.shape[:2]
        if rad.shape != (h, w, 3) or ids_lo.shape != (h, w, 3) or pos.shape != (H, W, 3) or ids.shape != (H, W, 3):
            raise ValueError("taa_upscale: radiance_lo and gbuffer_lo must be [h,w,3] and gbuffer_hi [H,W,3]")
        p = _or_default(p, taa_upscale_params)
        ret, tail = _image_outputs(H, W)
        check(self._lib.ff_taa_upscale(self._state, C.byref(camera), C.byref(p), w, h, rad.ctypes.data, ids_lo.ctypes.data, W, H, pos.ctypes.data,
                                       ids.ctypes.data, *tail))
        self._taa_upscale_size = (H, W)
        return ret

    def taa_upscale_device(self, camera, lo_width, lo_height, radiance_lo_ptr, ids_lo_ptr, width, height, position_ptr, ids_ptr, p=None, rgb8_ptr=None,
                           radiance_out_ptr=None):
        """ff_taa_upscale on DEVICE buffers (raw pointers); the outputs must not overlap an input."""
        p = _or_default(p, taa_upscale_params)
        check(self._lib.ff_taa_upscale(self._state, C.byref(camera), C.byref(p), lo_width, lo_height, _vp(radiance_lo_ptr), _vp(ids_lo_ptr), width, height,
                                       _vp(position_ptr), _vp(ids_ptr), *_tail(1, rgb8_ptr, radiance_out_ptr)))
        self._taa_upscale_size = (height, width)

    def taa_upscale_reset(self):
        """Drop the temporal upsampler's history (ff_taa_upscale_reset)."""
        check(self._lib.ff_taa_upscale_reset(self._state))

    def taa_upscale_history(self):
        """The last taa_upscale call's (motion [H,W,2] float32, history length [H,W] float32)."""
        return self._history(self._lib.ff_taa_upscale_history, self._taa_upscale_size)

    def motion_blur(self, radiance, motion, depth, p=None, want_rgb8=True, want_out=True):
        """ff_motion_blur of host radiance [H,W,3] with the motion [H,W,2] of a *_history call and gbuffer()'s depth [H,W]
        -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32)."""
        rad, mot, dep, (h, w) = _motion_blur_images(radiance, motion, depth, "motion_blur")
        p = _or_default(p, motion_blur_params)
        ret, tail = _image_outputs(h, w, want_rgb8, want_out)
        check(self._lib.ff_motion_blur(self._state, w, h, C.byref(p), rad.ctypes.data, mot.ctypes.data, dep.ctypes.data, *tail))
        return ret

    def motion_blur_device(self, width, height, radiance_ptr, motion_ptr, depth_ptr, p=None, rgb8_ptr=None, radiance_out_ptr=None):
        """ff_motion_blur on DEVICE buffers (raw pointers); the outputs must not overlap an input."""
        p = _or_default(p, motion_blur_params)
        check(self._lib.ff_motion_blur(self._state, width, height, C.byref(p), _vp(radiance_ptr), _vp(motion_ptr), _vp(depth_ptr),
                                       *_tail(1, rgb8_ptr, radiance_out_ptr)))

    def depth_of_field(self, radiance, gbuffer_or_planes, camera, p=None, want_rgb8=True, want_out=True):
        """ff_depth_of_field of host radiance [H,W,3] with a gbuffer() dict of `camera` (or its (position [H,W,3], depth [H,W])
        planes) -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32)."""
        rad, pos, dep, (h, w) = _dof_images(radiance, gbuffer_or_planes, "depth_of_field")
        p = _or_default(p, dof_params)
        ret, tail = _image_outputs(h, w, want_rgb8, want_out)
        check(self._lib.ff_depth_of_field(self._state, C.byref(camera), w, h, C.byref(p), rad.ctypes.data, pos.ctypes.data, dep.ctypes.data, *tail))
        return ret

    def depth_of_field_device(self, camera, width, height, radiance_ptr, position_ptr, depth_ptr, p=None, rgb8_ptr=None, radiance_out_ptr=None):
        """ff_depth_of_field on DEVICE buffers (raw pointers); the outputs must not overlap an input."""
        p = _or_default(p, dof_params)
        check(self._lib.ff_depth_of_field(self._state, C.byref(camera), width, height, C.byref(p), _vp(radiance_ptr), _vp(position_ptr), _vp(depth_ptr),
                                          *_tail(1, rgb8_ptr, radiance_out_ptr)))

    def despeckle(self, radiance, gbuffer_or_planes, p=None, want_rgb8=True, want_out=True):
        """ff_despeckle of radiance [H,W,3] with a gbuffer() dict (or its (albedo, ids) planes; albedo None without
        FF_DESPECKLE_DEMODULATE_ALBEDO) -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32, the number of clamped pixels).  Host
        arrays give host arrays; contiguous device tensors (torch, float32 / int32) give device tensors."""
        p = _or_default(p, despeckle_params)
        if hasattr(radiance, "data_ptr"):
            import torch
            images, device = (radiance, *_despeckle_planes(gbuffer_or_planes)), radiance.device
            h, w = radiance.shape[:2]
            for name, t, dtype in zip(("radiance", "albedo", "ids"), images, (torch.float32, torch.float32, torch.int32)):
                if t is not None:
                    _device_image(t, dtype, f"despeckle: {name}", dtype, (h, w))
        else:
            *images, (h, w) = _despeckle_images(radiance, gbuffer_or_planes, "despeckle")
            device = None
        clamped = C.c_uint32(0)
        ret = _run_filter(lambda w, h, rad, alb, ids, tail: self._lib.ff_despeckle(self._state, w, h, C.byref(p), rad, alb, ids, *tail, C.byref(clamped)),
                          images, (h, w), (h, w), want_rgb8, want_out, device)
        return (*ret, int(clamped.value))

    def despeckle_device(self, width, height, radiance_ptr, albedo_ptr, ids_ptr, p=None, rgb8_ptr=None, radiance_out_ptr=None, want_count=True):
        """ff_despeckle on DEVICE buffers (raw pointers); the outputs must not overlap an input -> the number of clamped pixels
        (None with want_count=False: out_clamped is passed as NULL)."""
        p = _or_default(p, despeckle_params)
        clamped = C.c_uint32(0)
        check(self._lib.ff_despeckle(self._state, width, height, C.byref(p), _vp(radiance_ptr), _vp(albedo_ptr), _vp(ids_ptr),
                                     *_tail(1, rgb8_ptr, radiance_out_ptr), C.byref(clamped) if want_count else None))
        return int(clamped.value) if want_count else None

    def sharpen(self, radiance, p=None, want_rgb8=True, want_out=True):
        """ff_sharpen of radiance [H,W,3] -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32).  A host array gives host arrays; a
        contiguous float32 device tensor (torch) gives device tensors."""
        p = _or_default(p, sharpen_params)
        return _filter("sharpen", radiance, lambda w, h, rad, tail: self._lib.ff_sharpen(self._state, w, h, C.byref(p), rad, *tail), want_rgb8, want_out)

    def sharpen_device(self, width, height, radiance_ptr, p=None, rgb8_ptr=None, radiance_out_ptr=None):
        """ff_sharpen on DEVICE buffers (raw pointers); the outputs must not overlap the input."""
        p = _or_default(p, sharpen_params)
        check(self._lib.ff_sharpen(self._state, width, height, C.byref(p), _vp(radiance_ptr), *_tail(1, rgb8_ptr, radiance_out_ptr)))

    def local_tonemap(self, radiance, p=None, want_rgb8=True, want_out=True, in_place=False):
        """ff_local_tonemap of radiance [H,W,3] -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32).  A host array gives host arrays; a
        contiguous float32 device tensor (torch) gives device tensors.  in_place: radiance_out is radiance_in in the call (a device
        tensor is overwritten and returned; a host array is copied first)."""
        p = _or_default(p, local_tonemap_params)
        return _filter("local_tonemap", radiance, lambda w, h, rad, tail: self._lib.ff_local_tonemap(self._state, w, h, C.byref(p), rad, *tail),
                       want_rgb8, want_out, in_place)

    def local_tonemap_device(self, width, height, radiance_ptr, p=None, rgb8_ptr=None, radiance_out_ptr=None):
        """ff_local_tonemap on DEVICE buffers (raw pointers); radiance_out_ptr may be radiance_ptr."""
        p = _or_default(p, local_tonemap_params)
        check(self._lib.ff_local_tonemap(self._state, width, height, C.byref(p), _vp(radiance_ptr), *_tail(1, rgb8_ptr, radiance_out_ptr)))

    def encode_yuv(self, linear, p=None):
        """ff_encode_yuv of host display-linear [H,W,3] -> (luma [H,W], chroma [ceil(H/2),ceil(W/2),2] of Cb Cr pairs), host arrays:
        uint8 codes at depth 8 (NV12), uint16 codes << 6 at depth 10 (P010)."""
        img, (h, w) = _float3_image(linear, "encode_yuv")
        p = _or_default(p, yuv_params)
        luma, chroma = _yuv_planes(h, w, p)
        check(self._lib.ff_encode_yuv(self._state, w, h, C.byref(p), img.ctypes.data, 0, luma.ctypes.data, chroma.ctypes.data, 0))
        return luma, chroma

    def encode_yuv_device(self, linear, p=None, luma=None, chroma=None):
        """ff_encode_yuv on DEVICE tensors (torch): linear a contiguous [H,W,3] float32 tensor -> (luma, chroma) tensors laid out as
        encode_yuv's arrays (uint8 at depth 8, int16 holding the uint16 bit patterns otherwise).  luma / chroma: contiguous tensors
        of at least the planes' bytes to write into (any dtype and shape; returned as given); they must not overlap the input or
        each other."""
        import torch
        p = _or_default(p, yuv_params)
        h, w = _device_image(linear, torch.float32, "encode_yuv_device: linear", "float32")
        need = yuv_plane_bytes(w, h, p)
        dtype = torch.uint8 if int(p.depth) == 8 else torch.int16
        if luma is None:
            luma = torch.zeros((h, w), dtype=dtype, device=linear.device)
        if chroma is None:
            chroma = torch.zeros(((h + 1) // 2, (w + 1) // 2, 2), dtype=dtype, device=linear.device)
        for name, t, n in (("luma", luma, need[0]), ("chroma", chroma, need[1])):
            if not t.is_cuda or not t.is_contiguous() or t.numel() * t.element_size() < n:
                raise ValueError(f"encode_yuv_device: {name} must be a contiguous device tensor of at least {n} bytes")
        torch.cuda.synchronize(linear.device)
        check(self._lib.ff_encode_yuv(self._state, w, h, C.byref(p), _vp(linear.data_ptr()), 1, _vp(luma.data_ptr()), _vp(chroma.data_ptr()), 1))
        return luma, chroma

    def resize(self, radiance, out_width, out_height, p=None, want_rgb8=True, want_out=True):
        """ff_resize of radiance [H,W,3] -> (rgb8 [H',W',3] uint8, radiance [H',W',3] float32).  A host array gives host arrays; a
        contiguous float32 device tensor (torch) gives device tensors."""
        p = _or_default(p, resize_params)
        return _filter("resize", radiance,
                       lambda w, h, rad, tail: self._lib.ff_resize(self._state, C.byref(p), w, h, rad, tail[0], out_width, out_height, *tail[1:]),
                       want_rgb8, want_out, out_size=_resize_shape(out_width, out_height))

    def resize_device(self, in_width, in_height, radiance_ptr, out_width, out_height, p=None, rgb8_ptr=None, radiance_out_ptr=None):
        """ff_resize on DEVICE buffers (raw pointers); the outputs must not overlap the input or each other."""
        p = _or_default(p, resize_params)
        check(self._lib.ff_resize(self._state, C.byref(p), in_width, in_height, _vp(radiance_ptr), 1, out_width, out_height,
                                  *_tail(1, rgb8_ptr, radiance_out_ptr)[1:]))

    def grade_lut_create(self, lut):
        """ff_grade_lut_create of a GradeLut (lib.grade_lut, lib.load_cube) -> the LUT's id, for FfGradeParams.lut_id."""
        out = C.c_int(-1)
        check(self._lib.ff_grade_lut_create(self._state, C.byref(lut.desc), C.byref(out)))
        return int(out.value)

    def grade_lut_destroy(self, lut_id):
        check(self._lib.ff_grade_lut_destroy(self._state, lut_id))

    def color_grade(self, radiance, p=None, want_rgb8=True, want_out=True, in_place=False):
        """ff_color_grade of radiance [H,W,3] -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32).  A host array gives host arrays; a
        contiguous float32 device tensor (torch) gives device tensors.  in_place: radiance_out is radiance_in in the call (a device
        tensor is overwritten and returned; a host array is copied first)."""
        p = _or_default(p, grade_params)
        return _filter("color_grade", radiance, lambda w, h, rad, tail: self._lib.ff_color_grade(self._state, C.byref(p), w, h, rad, *tail),
                       want_rgb8, want_out, in_place)

    def color_grade_device(self, width, height, radiance_ptr, p=None, rgb8_ptr=None, radiance_out_ptr=None):
        """ff_color_grade on DEVICE buffers (raw pointers); radiance_out_ptr may be radiance_ptr."""
        p = _or_default(p, grade_params)
        check(self._lib.ff_color_grade(self._state, C.byref(p), width, height, _vp(radiance_ptr), *_tail(1, rgb8_ptr, radiance_out_ptr)))

    def lens(self, radiance, p=None, want_rgb8=True, want_out=True):
        """ff_lens of radiance [H,W,3] -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32).  A host array gives host arrays; a
        contiguous float32 device tensor (torch) gives device tensors."""
        p = _or_default(p, lens_params)
        return _filter("lens", radiance, lambda w, h, rad, tail: self._lib.ff_lens(self._state, w, h, C.byref(p), rad, *tail), want_rgb8, want_out)

    def lens_device(self, width, height, radiance_ptr, p=None, rgb8_ptr=None, radiance_out_ptr=None):
        """ff_lens on DEVICE buffers (raw pointers); the outputs must not overlap the input."""
        p = _or_default(p, lens_params)
        check(self._lib.ff_lens(self._state, width, height, C.byref(p), _vp(radiance_ptr), *_tail(1, rgb8_ptr, radiance_out_ptr)))

    def lens_table_builds(self):
        """ff_debug_lens_table_builds: how often this tracer has built and uploaded ff_lens's table."""
        n = C.c_uint64(0)
        check(self._lib.ff_debug_lens_table_builds(self._state, C.byref(n)))
        return int(n.value)

    def interpolate(self, mid, a, b, p=None, geom_maps=None, want_rgb8=True, want_out=True):
        """ff_interpolate of host arrays: mid = (camera, gbuffer), a and b = (camera, radiance [H,W,3], gbuffer), a gbuffer being a
        gbuffer() dict or the pair (position, ids); geom_maps [n,2,3,4] or None
        -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32, counts [5] uint32: both, A only, B only, filled, fallback)."""
        cams, im, (h, w) = _interpolate_images(mid, a, b, "interpolate")
        maps, n = _interpolate_maps(geom_maps, "interpolate")
        p = _or_default(p, interpolate_params)
        ret, tail = _image_outputs(h, w, want_rgb8, want_out)
        counts = np.zeros(5, dtype=np.uint32)
        d = [x.ctypes.data for x in im]
        check(self._lib.ff_interpolate(self._state, w, h, C.byref(p), C.byref(cams[0]), d[0], d[1], C.byref(cams[1]), d[2], d[3], d[4], C.byref(cams[2]),
                                       d[5], d[6], d[7], maps.ctypes.data if maps is not None else None, n, *tail, counts.ctypes.data))
        return (*ret, counts)

    def interpolate_device(self, width, height, cameras, image_ptrs, p=None, geom_maps=None, rgb8_ptr=None, radiance_out_ptr=None, want_counts=True):
        """ff_interpolate on DEVICE buffers (raw pointers): cameras = (mid, a, b); image_ptrs = the eight images in the C call's order
        (position, ids, radiance_a, position_a, ids_a, radiance_b, position_b, ids_b); geom_maps a HOST [n,2,3,4] array or None; the
        outputs must not overlap an input -> counts [5] uint32 (None without want_counts)."""
        maps, n = _interpolate_maps(geom_maps, "interpolate_device")
        p = _or_default(p, interpolate_params)
        d = [_vp(q) for q in image_ptrs]
        if len(d) != 8:
            raise ValueError("interpolate_device: image_ptrs must name eight images")
        counts = np.zeros(5, dtype=np.uint32)
        check(self._lib.ff_interpolate(self._state, width, height, C.byref(p), C.byref(cameras[0]), d[0], d[1], C.byref(cameras[1]), d[2], d[3], d[4],
                                       C.byref(cameras[2]), d[5], d[6], d[7], maps.ctypes.data if maps is not None else None, n,
                                       *_tail(1, rgb8_ptr, radiance_out_ptr), counts.ctypes.data if want_counts else None))
        return counts if want_counts else None

    def display(self, radiance, p=None, want_rgb8=True, want_out=True):
        """ff_display of host radiance [H,W,3] -> (rgb8 [H,W,3] uint8, display_out [H,W,3] float32: the curve's output in [0, 1]);
        the adapted exposure stays in the state."""
        rad, (h, w) = _float3_image(radiance, "display")
        p = _or_default(p, display_params)
        ret, tail = _image_outputs(h, w, want_rgb8, want_out)
        check(self._lib.ff_display(self._state, w, h, C.byref(p), rad.ctypes.data, *tail))
        return ret

    def display_device(self, width, height, radiance_ptr, p=None, rgb8_ptr=None, display_out_ptr=None):
        """ff_display on DEVICE buffers (raw pointers); display_out_ptr may equal radiance_ptr."""
        p = _or_default(p, display_params)
        check(self._lib.ff_display(self._state, width, height, C.byref(p), _vp(radiance_ptr), *_tail(1, rgb8_ptr, display_out_ptr)))

    def display_to_pbo(self, radiance, p=None):
        """ff_display_to_pbo of host radiance [H,W,3] into the buffer registered with ff_register_gl_pbo."""
        rad = np.ascontiguousarray(radiance, dtype=np.float32)
        p = _or_default(p, display_params)
        check(self._lib.ff_display_to_pbo(self._state, rad.shape[1], rad.shape[0], C.byref(p), rad.ctypes.data, 0))

    def display_reset(self):
        """Forget the adapted exposure (ff_display_reset)."""
        check(self._lib.ff_display_reset(self._state))

    def display_state(self):
        """The last display call's (exposure, target, histogram uint32 [256])."""
        e, t = C.c_float(), C.c_float()
        hist = np.zeros(T.DISPLAY_BINS, dtype=np.uint32)
        check(self._lib.ff_display_state(self._state, C.byref(e), C.byref(t), hist.ctypes.data))
        return e.value, t.value, hist

    def strips_local_rows(self, height, strip_rows, part, num_parts):
        return self._lib.ff_strips_local_rows(height, strip_rows, part, num_parts)

    def render_strips(self, camera, params, strip_rows, part, num_parts, want_rgb8=True, want_radiance=True):
        rows = self._lib.ff_strips_local_rows(params.height, strip_rows, part, num_parts)
        ret, tail = _image_outputs(rows, params.width, want_rgb8, want_radiance)
        if not rows:  # (a part without rows gets empty arrays, and the call no pointer to them)
            tail = _tail(0, None, None)
        n = C.c_int(0)
        check(self._lib.ff_render_strips(self._state, C.byref(camera), C.byref(params), strip_rows, part, num_parts, *tail[1:], C.byref(n)))
        assert n.value == rows
        return ret

    def render_strips_device(self, camera, params, strip_rows, part, num_parts, rgb8_ptr=None, radiance_ptr=None):
        n = C.c_int(0)
        check(self._lib.ff_render_strips(self._state, C.byref(camera), C.byref(params), strip_rows, part, num_parts,
                                         *_tail(1, rgb8_ptr, radiance_ptr)[1:], C.byref(n)))
        return n.value

    def deinterleave_strips(self, src_ptr, dst_ptr, width, height, strip_rows, num_parts, elem_bytes):
        check(self._lib.ff_deinterleave_strips(self._state, C.c_void_p(src_ptr), C.c_void_p(dst_ptr), width, height,
                                               strip_rows, num_parts, elem_bytes))

    def intersect_rays(self, origins, directions, trace_mode=T.TRACE_BVH):
        """intersectRays (kernel.cu:127-176) for arrays of world-space rays -> structured result arrays."""
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
        n = o.shape[0]
        rays = np.concatenate([o, d], axis=1).astype(np.float32)
        rbuf = (T.FfRay * n)()
        C.memmove(rbuf, rays.ctypes.data, rays.nbytes)
        out = (T.FfIntersect * n)()
        check(self._lib.ff_intersect_rays(self._state, rbuf, n, out, trace_mode))
        return intersect_array(out, n)

    # ---- multi-GPU, one process per GPU (ff_dist_*) ----

    def dist_init(self, rank, world_size, unique_id):
        """Join the job's RCCL communicator.  `unique_id`: the 128 bytes dist_unique_id() returned on rank 0."""
        buf = (C.c_char * DIST_ID_BYTES).from_buffer_copy(bytes(unique_id))
        check(self._lib.ff_dist_init(self._state, rank, world_size, buf, DIST_ID_BYTES))

    def dist_shutdown(self):
        check(self._lib.ff_dist_shutdown(self._state))

    def debug_dist_fail_rank(self, rank):
        """Tests: rank `rank` reports an injected local failure from the next distributed frame on (-1: off)."""
        check(self._lib.ff_debug_dist_fail_rank(self._state, rank))

    def render_distributed(self, camera, params, strip_rows=0, rank=0, want_rgb8=True, want_radiance=True):
        """One frame over all ranks; returns (rgb8, radiance) host arrays on rank 0, (None, None) elsewhere."""
        root = rank == 0
        ret, tail = _image_outputs(params.height, params.width, want_rgb8 and root, want_radiance and root)
        check(self._lib.ff_render_distributed(self._state, C.byref(camera), C.byref(params), strip_rows, *tail[1:]))
        return ret

    def render_distributed_device(self, camera, params, strip_rows=0, rgb8_ptr=None, radiance_ptr=None):
        """The same into caller-owned device buffers on rank 0 (raw pointers; ignored on other ranks)."""
        check(self._lib.ff_render_distributed(self._state, C.byref(camera), C.byref(params), strip_rows, *_tail(1, rgb8_ptr, radiance_ptr)[1:]))


def dist_unique_id():
    """128-byte RCCL id for Tracer.dist_init (call on rank 0, hand to the other ranks)."""
    buf = (C.c_char * DIST_ID_BYTES)()
    check(load().ff_dist_unique_id(buf, DIST_ID_BYTES))
    return bytes(buf)


def dist_available():
    """True if this process can load RCCL (what dist_unique_id / Tracer.dist_init need)."""
    return load().ff_dist_available() == T.FF_OK


def dist_strip_rows(world_size, height=1080):
    return load().ff_dist_strip_rows_for(height, world_size)


class MultiTracer:
    """Several GPUs driven by ONE process (ff_multi_*): what a single-process viewer calls.  device_ids[0] gathers."""

    def __init__(self, device_ids):
        self._lib = load()
        self._handle = C.c_void_p()
        ids = (C.c_int * len(device_ids))(*device_ids)
        check(self._lib.ff_multi_create(C.byref(self._handle), ids, len(device_ids)))

    def close(self):
        if self._handle:
            self._lib.ff_multi_destroy(self._handle)
            self._handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __len__(self):
        return self._lib.ff_multi_count(self._handle)

    @property
    def uses_rccl(self):
        return bool(self._lib.ff_multi_uses_rccl(self._handle))

    def upload_scene(self, scene):
        check(self._lib.ff_multi_upload_scene(self._handle, scene.geometries, len(scene)))

    def render(self, camera, params, strip_rows=0, want_rgb8=True, want_radiance=True):
        ret, tail = _image_outputs(params.height, params.width, want_rgb8, want_radiance)
        check(self._lib.ff_multi_render(self._handle, C.byref(camera), C.byref(params), strip_rows, *tail[1:]))
        return ret

    def render_device(self, camera, params, strip_rows=0, rgb8_ptr=None, radiance_ptr=None):
        check(self._lib.ff_multi_render(self._handle, C.byref(camera), C.byref(params), strip_rows, *_tail(1, rgb8_ptr, radiance_ptr)[1:]))

    def set_pixel_jitter(self, jx, jy):
        check(self._lib.ff_multi_set_pixel_jitter(self._handle, jx, jy))

    def stats(self):
        st = T.FfStats()
        check(self._lib.ff_multi_stats(self._handle, C.byref(st)))
        return st


INTERSECT_DTYPE = np.dtype([("point", np.float32, 3), ("normal", np.float32, 3), ("t", np.float32), ("hit", np.uint8),
                            ("_pad", np.uint8, 3), ("geom", np.int32), ("tri", np.int32)])
assert INTERSECT_DTYPE.itemsize == 40


def intersect_array(buf, n):
    return np.frombuffer(bytes(buf), dtype=INTERSECT_DTYPE, count=n).copy()
