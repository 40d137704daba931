"""The C ABI of include/firefly/ff_api.h as ctypes sees it: where libfirefly_hip.so is, the one handle every module of the binding
shares, the prototype of every exported function (PROTOTYPES, which tests/test_host_api.py holds against the header) and the
status check.

There is no CPU fallback: if the HIP library is missing, ``load()`` raises.
"""
import ctypes as C
import os

from . import types as T

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FF_LIB_PATH") or os.path.join(_HERE, "libfirefly_hip.so")  # FF_LIB_PATH: another build of the same library (A/B runs)

vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
P = C.POINTER
cam = P(T.FfCamera)
rp = P(T.FfRenderParams)

# every exported symbol declared in include/firefly/ff_api.h: name -> argtypes, or (argtypes, restype) where it does not return int
PROTOTYPES = {
    "ff_create": [P(vp), i32],
    "ff_destroy": [vp],
    "ff_last_error": ([], C.c_char_p),
    "ff_version": [],
    "ff_set_stream": [vp, vp],
    "ff_geometry_init": ([P(T.FfGeometry), i32, T.FfVec3, T.FfVec3, T.FfVec3, P(T.FfTriangle), i32, f32], None),
    "ff_bxdf_init": ([P(T.FfBXDF)], None),
    "ff_camera_init_default": ([cam, i32, i32], None),
    "ff_camera_update_basis": ([cam], None),
    "ff_camera_ray_matrix": ([cam, P(T.FfMat4)], None),
    # scene upload and the builders' debug views
    "ff_upload_scene": [vp, P(T.FfGeometry), i32],
    "ff_set_builder": [vp, i32],
    "ff_update_transforms": [vp, P(T.FfGeometry), i32],
    "ff_update_mesh": [vp, i32, P(T.FfTriangle), i32, i32],
    "ff_build_stats": [vp, P(T.FfBuildStats)],
    "ff_debug_download_bvh": [vp, vp, i32, P(i32), vp, i32, P(i32), P(i32), i32],
    "ff_debug_download_bvh4": [vp, vp, i32, P(i32), P(i32), i32],
    "ff_scene_info": [P(T.FfGeometry), i32, P(T.FfSceneInfo)],
    "ff_debug_wall_table": [P(T.FfGeometry), i32, P(C.c_float), i32],
    "ff_debug_wall_entries": [P(T.FfGeometry), i32],
    # render calls
    "ff_render": [vp, cam, rp, vp, i32, vp, i32],
    "ff_render_tile": [vp, cam, rp, i32, i32, i32, i32, vp, i32, vp, i32],
    "ff_render_strips": [vp, cam, rp, i32, i32, i32, vp, i32, vp, i32, P(i32)],
    "ff_strips_local_rows": [i32, i32, i32, i32],
    "ff_deinterleave_strips": [vp, vp, vp, i32, i32, i32, i32, i32],
    "ff_intersect_rays": [vp, P(T.FfRay), i32, P(T.FfIntersect), i32],
    "ff_register_gl_pbo": [vp, C.c_uint, i32, i32],
    "ff_unregister_gl_pbo": [vp],
    "ff_render_to_pbo": [vp, cam, rp],
    "ff_render_progressive": [vp, cam, rp, i32, vp, i32, vp, i32],
    "ff_render_to_pbo_progressive": [vp, cam, rp, i32],
    "ff_save_ppm": [C.c_char_p, vp, i32, i32],
    # statistics and debug views
    "ff_set_collect_stats": [vp, i32],
    "ff_stats": [vp, P(T.FfStats)],
    "ff_debug_counters": [vp, P(C.c_ulonglong)],
    "ff_debug_timeline": [vp, P(C.c_uint), P(C.c_int)],
    "ff_debug_kernel_name": ([vp], C.c_char_p),
    "ff_debug_layout": [vp, P(i32)],
    "ff_debug_stack_spill": [vp, i32, P(C.c_ulonglong)],
    "ff_debug_check_ieee": [vp, P(C.c_ulonglong)],
    "ff_debug_reload_switches": [vp],
    # mesh and scene files
    "ff_load_obj": [C.c_char_p, P(P(T.FfTriangle)), P(i32)],
    "ff_free_triangles": ([P(T.FfTriangle)], None),
    "ff_scene_file_load": [C.c_char_p, P(vp)],
    "ff_scene_file_geometries": ([vp, P(i32)], P(T.FfGeometry)),
    "ff_scene_file_camera": [vp, i32, i32, cam],
    "ff_scene_file_free": ([vp], None),
    # multi-GPU: one process per GPU (ff_dist_*), one process for several (ff_multi_*)
    "ff_dist_unique_id": [vp, i32],
    "ff_dist_init": [vp, i32, i32, vp, i32],
    "ff_dist_shutdown": [vp],
    "ff_debug_dist_fail_rank": [vp, i32],
    "ff_dist_available": [],
    "ff_dist_strip_rows": [i32],
    "ff_dist_strip_rows_for": [i32, i32],
    "ff_dist_part_bytes": ([i32, i32, i32, i32, i32, P(C.c_longlong)], C.c_longlong),
    "ff_render_distributed": [vp, cam, rp, i32, vp, i32, vp, i32],
    "ff_multi_create": [P(vp), P(i32), i32],
    "ff_multi_destroy": [vp],
    "ff_multi_count": [vp],
    "ff_multi_state": ([vp, i32], vp),
    "ff_multi_uses_rccl": [vp],
    "ff_multi_upload_scene": [vp, P(T.FfGeometry), i32],
    "ff_multi_render": [vp, cam, rp, i32, vp, i32, vp, i32],
    "ff_multi_render_to_pbo": [vp, cam, rp, i32],
    "ff_multi_stats": [vp, P(T.FfStats)],
    # G-buffer, denoisers, jitter and TAA
    "ff_gbuffer": [vp, cam, rp, vp, vp, vp, vp, vp, i32],
    "ff_denoise_params_init": ([P(T.FfDenoiseParams)], None),
    "ff_denoise": [vp, i32, i32, P(T.FfDenoiseParams), vp, vp, vp, vp, vp, i32, vp, i32, vp, i32],
    "ff_temporal_params_init": ([P(T.FfTemporalParams)], None),
    "ff_denoise_temporal": [vp, cam, i32, i32, P(T.FfTemporalParams), vp, vp, vp, vp, vp, i32, vp, i32, vp, i32],
    "ff_temporal_reset": [vp],
    "ff_temporal_history": [vp, vp, vp, i32],
    "ff_camera_ray_matrix_jittered": ([cam, f32, f32, P(T.FfMat4)], None),
    "ff_set_pixel_jitter": [vp, f32, f32],
    "ff_multi_set_pixel_jitter": [vp, f32, f32],
    "ff_jitter_sequence": [i32, i32, P(f32), P(f32)],
    "ff_taa_params_init": ([P(T.FfTaaParams)], None),
    "ff_taa": [vp, cam, i32, i32, P(T.FfTaaParams), vp, vp, vp, i32, vp, i32, vp, i32],
    "ff_taa_reset": [vp],
    "ff_taa_history": [vp, vp, vp, i32],
    # lights and the environment
    "ff_light_table": [P(T.FfGeometry), i32, P(T.FfLightEntry), i32, P(f32)],
    "ff_check_render_params": [rp],
    "ff_set_environment": [vp, vp, i32, i32, f32, f32],
    "ff_environment_table": [vp, i32, i32, vp, vp, vp, vp],
    "ff_load_hdr": [C.c_char_p, P(P(f32)), P(i32), P(i32)],
    "ff_free_hdr": ([P(f32)], None),
    "ff_scene_file_environment": [vp, P(C.c_char_p), P(f32), P(f32)],
    # display transform
    "ff_display_params_init": ([P(T.FfDisplayParams)], None),
    "ff_display": [vp, i32, i32, P(T.FfDisplayParams), vp, i32, vp, i32, vp, i32],
    "ff_display_to_pbo": [vp, i32, i32, P(T.FfDisplayParams), vp, i32],
    "ff_display_reset": [vp],
    "ff_display_state": [vp, P(f32), P(f32), vp],
    "ff_srgb_thresholds": [vp],
    "ff_display_curve": [P(T.FfDisplayParams), vp, i32, vp, vp],
    "ff_display_exposure": [P(T.FfDisplayParams), vp, f32, P(f32), P(f32)],
    "ff_save_hdr": [C.c_char_p, vp, i32, i32],
    # albedo textures
    "ff_texture_create": [vp, vp, i32, i32, i32, P(i32)],
    "ff_texture_destroy": [vp, i32],
    "ff_set_albedo_texture": [vp, i32, i32, f32, f32, f32, f32],
    "ff_texture_sample": [vp, i32, i32, i32, vp, i32, vp],
    "ff_surface_uv": [P(T.FfGeometry), i32, i32, vp, vp, i32, vp],
    "ff_load_ppm": [C.c_char_p, P(P(C.c_ubyte)), P(i32), P(i32)],
    "ff_free_ppm": ([P(C.c_ubyte)], None),
    "ff_rgb8_to_linear": [vp, i32, i32, vp],
    "ff_scene_file_texture_count": [vp],
    "ff_scene_file_texture": [vp, i32, P(C.c_char_p), P(C.c_char_p), P(i32)],
    "ff_scene_file_albedo_map": [vp, i32, P(i32), P(f32), P(f32)],
    # rough-specular mirrors
    "ff_set_roughness": [vp, i32, f32],
    "ff_glossy_eval": [f32, vp, vp, vp, i32, vp, vp],
    "ff_glossy_sample": [f32, vp, vp, vp, i32, vp, vp, vp],
    "ff_scene_file_roughness": [vp, i32, P(f32)],
    # per-sample camera rays
    "ff_camera_sampling_init": ([P(T.FfCameraSampling)], None),
    "ff_set_camera_sampling": [vp, P(T.FfCameraSampling)],
    "ff_camera_sample_rays": [cam, P(T.FfCameraSampling), f32, f32, i32, C.c_uint64, vp, vp, vp, i32, vp, vp],
    "ff_scene_file_camera_sampling": [vp, P(T.FfCameraSampling)],
    # guided and temporal upsampling
    "ff_upscale_params_init": ([P(T.FfUpscaleParams)], None),
    "ff_upscale": [vp, P(T.FfUpscaleParams), i32, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, i32, vp, i32, vp, i32],
    "ff_upscale_host": [P(T.FfUpscaleParams), i32, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp],
    "ff_taa_upscale_params_init": ([P(T.FfTaaUpscaleParams)], None),
    "ff_taa_upscale": [vp, cam, P(T.FfTaaUpscaleParams), i32, i32, vp, vp, i32, i32, vp, vp, i32, vp, i32, vp, i32],
    "ff_taa_upscale_reset": [vp],
    "ff_taa_upscale_history": [vp, vp, vp, i32],
    # the image filters: each with its parameter defaults, the device call and a host-only twin
    "ff_motion_blur_params_init": ([P(T.FfMotionBlurParams)], None),
    "ff_motion_blur": [vp, i32, i32, P(T.FfMotionBlurParams), vp, vp, vp, i32, vp, i32, vp, i32],
    "ff_motion_blur_host": [i32, i32, P(T.FfMotionBlurParams), vp, vp, vp, vp, vp],
    "ff_dof_params_init": ([P(T.FfDofParams)], None),
    "ff_dof_params_from_camera": [cam, P(T.FfCameraSampling), P(T.FfDofParams)],
    "ff_depth_of_field": [vp, cam, i32, i32, P(T.FfDofParams), vp, vp, vp, i32, vp, i32, vp, i32],
    "ff_depth_of_field_host": [cam, i32, i32, P(T.FfDofParams), vp, vp, vp, vp, vp],
    "ff_despeckle_params_init": ([P(T.FfDespeckleParams)], None),
    "ff_despeckle": [vp, i32, i32, P(T.FfDespeckleParams), vp, vp, vp, i32, vp, i32, vp, i32, P(C.c_uint32)],
    "ff_despeckle_host": [i32, i32, P(T.FfDespeckleParams), vp, vp, vp, vp, vp, P(C.c_uint32)],
    "ff_sharpen_params_init": ([P(T.FfSharpenParams)], None),
    "ff_sharpen": [vp, i32, i32, P(T.FfSharpenParams), vp, i32, vp, i32, vp, i32],
    "ff_sharpen_host": [i32, i32, P(T.FfSharpenParams), vp, vp, vp],
    "ff_local_tonemap_params_init": ([P(T.FfLocalTonemapParams)], None),
    "ff_local_tonemap": [vp, i32, i32, P(T.FfLocalTonemapParams), vp, i32, vp, i32, vp, i32],
    "ff_local_tonemap_host": [i32, i32, P(T.FfLocalTonemapParams), vp, vp, vp],
    "ff_local_tonemap_grid_host": [i32, i32, P(T.FfLocalTonemapParams), vp, vp, vp],
    "ff_interpolate_params_init": ([P(T.FfInterpolateParams)], None),
    "ff_interpolate": [vp, i32, i32, P(T.FfInterpolateParams), cam, vp, vp, cam, vp, vp, vp, cam, vp, vp, vp, vp, i32, i32,
                       vp, i32, vp, i32, vp],
    "ff_interpolate_host": [i32, i32, P(T.FfInterpolateParams), cam, vp, vp, cam, vp, vp, vp, cam, vp, vp, vp, vp, i32, vp, vp, vp],
    "ff_interpolate_geometry_maps": [P(T.FfGeometry), P(T.FfGeometry), P(T.FfGeometry), i32, vp, vp],
    "ff_adaptive_params_init": ([P(T.FfAdaptiveParams)], None),
    "ff_render_adaptive": [vp, cam, rp, P(T.FfAdaptiveParams), vp, i32, vp, i32, vp, i32, P(T.FfAdaptiveInfo)],
    "ff_adaptive_state": [vp, vp, vp, vp, vp, i32],
    "ff_adaptive_tile_error": [vp, i32, i32, i32, i32, vp, vp, i32, vp],
    "ff_adaptive_tile_error_host": [i32, i32, i32, i32, vp, vp, vp],
    "ff_adaptive_plan_host": [i32, i32, vp, vp, i32],
    "ff_yuv_params_init": ([P(T.FfYuvParams)], None),
    "ff_yuv_plane_bytes": [i32, i32, P(T.FfYuvParams), P(C.c_uint64), P(C.c_uint64)],
    "ff_yuv_knots": [i32, vp],
    "ff_encode_yuv": [vp, i32, i32, P(T.FfYuvParams), vp, i32, vp, vp, i32],
    "ff_encode_yuv_host": [i32, i32, P(T.FfYuvParams), vp, vp, vp],
    "ff_save_y4m": [C.c_char_p, i32, i32, i32, P(T.FfYuvParams), vp, vp],
    "ff_resize_params_init": ([P(T.FfResizeParams)], None),
    "ff_resize_taps": [i32, i32, i32, P(i32)],
    "ff_resize_weights": [i32, i32, i32, vp, vp],
    "ff_resize": [vp, P(T.FfResizeParams), i32, i32, vp, i32, i32, i32, vp, i32, vp, i32],
    "ff_resize_host": [P(T.FfResizeParams), i32, i32, vp, i32, i32, vp, vp],
    "ff_grade_params_init": ([P(T.FfGradeParams)], None),
    "ff_grade_lut_create": [vp, P(T.FfGradeLut), P(i32)],
    "ff_grade_lut_destroy": [vp, i32],
    "ff_color_grade": [vp, P(T.FfGradeParams), i32, i32, vp, i32, vp, i32, vp, i32],
    "ff_color_grade_host": [P(T.FfGradeParams), P(T.FfGradeLut), i32, i32, vp, vp, vp],
    "ff_load_cube": [C.c_char_p, P(T.FfCubeFile)],
    "ff_free_cube": ([P(T.FfCubeFile)], None),
    "ff_save_cube": [C.c_char_p, P(T.FfCubeFile)],
    "ff_lens_params_init": ([P(T.FfLensParams)], None),
    "ff_lens": [vp, i32, i32, P(T.FfLensParams), vp, i32, vp, i32, vp, i32],
    "ff_lens_host": [i32, i32, P(T.FfLensParams), vp, vp, vp],
    "ff_lens_tables": [P(T.FfLensParams), i32, i32, vp, vp, P(C.c_double)],
    "ff_lens_map_host": [P(T.FfLensParams), i32, i32, i32, vp, i32, vp],
    "ff_lens_fit_zoom": [P(T.FfLensParams), i32, i32, i32, P(f32)],
    "ff_debug_lens_table_builds": [vp, P(C.c_uint64)],
}
PROTOTYPES = {name: proto if isinstance(proto, tuple) else (proto, C.c_int) for name, proto in PROTOTYPES.items()}
EXPORTS = list(PROTOTYPES)

_lib = None


class FireflyError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"firefly status {status}: {message}")
        self.status = status
        self.message = message


def load():
    """Load libfirefly_hip.so (once) and declare prototypes. Raises if the library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP extension has not been built (run __graft_entry__.build()); "
            "there is no CPU fallback for the trace path")
    lib = C.CDLL(LIB_PATH)
    # (an older build loaded through FF_LIB_PATH for an A/B run may lack the newest entry points: skip their prototypes)
    tolerant = bool(os.environ.get("FF_LIB_PATH"))
    for name, (argtypes, restype) in PROTOTYPES.items():
        if tolerant and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = argtypes, restype
    _lib = lib
    return lib


def check(status):
    if status != T.FF_OK:
        raise FireflyError(status, load().ff_last_error().decode("utf-8", "replace"))
