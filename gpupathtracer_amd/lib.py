"""ctypes binding of the C ABI in include/firefly/ff_api.h (libfirefly_hip.so, built in-tree by
``python -c 'import __graft_entry__ as g; g.build()'`` or ``make -C gpupathtracer_amd/csrc``).

There is no CPU fallback: if the HIP library is missing, importing this module's ``load()`` raises.
"""
import ctypes as C
import os

import numpy as np

from . import types as T

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FF_LIB_PATH") or os.path.join(_HERE, "libfirefly_hip.so")  # FF_LIB_PATH: another build of the same library (A/B runs)

# every exported symbol declared in include/firefly/ff_api.h
EXPORTS = [
    "ff_create", "ff_destroy", "ff_last_error", "ff_version", "ff_set_stream",
    "ff_geometry_init", "ff_bxdf_init", "ff_camera_init_default", "ff_camera_update_basis", "ff_camera_ray_matrix",
    "ff_render_tile", "ff_upload_scene", "ff_set_builder", "ff_update_transforms", "ff_update_mesh", "ff_build_stats", "ff_debug_download_bvh", "ff_debug_download_bvh4",
    "ff_scene_info", "ff_debug_wall_table", "ff_debug_wall_entries", "ff_render", "ff_render_strips", "ff_strips_local_rows", "ff_deinterleave_strips",
    "ff_intersect_rays", "ff_register_gl_pbo", "ff_unregister_gl_pbo", "ff_render_to_pbo",
    "ff_render_progressive", "ff_render_to_pbo_progressive", "ff_save_ppm",
    "ff_set_collect_stats", "ff_stats", "ff_debug_kernel_name", "ff_debug_layout", "ff_debug_stack_spill", "ff_debug_counters", "ff_debug_timeline", "ff_debug_check_ieee", "ff_debug_reload_switches", "ff_load_obj", "ff_free_triangles",
    "ff_scene_file_load", "ff_scene_file_geometries", "ff_scene_file_camera", "ff_scene_file_free",
    "ff_dist_unique_id", "ff_dist_init", "ff_dist_available", "ff_dist_shutdown", "ff_dist_strip_rows", "ff_dist_strip_rows_for", "ff_dist_part_bytes", "ff_render_distributed", "ff_debug_dist_fail_rank",
    "ff_multi_create", "ff_multi_destroy", "ff_multi_count", "ff_multi_state", "ff_multi_uses_rccl", "ff_multi_upload_scene",
    "ff_multi_render", "ff_multi_render_to_pbo", "ff_multi_stats",
    "ff_gbuffer", "ff_denoise_params_init", "ff_denoise",
    "ff_temporal_params_init", "ff_denoise_temporal", "ff_temporal_reset", "ff_temporal_history",
    "ff_camera_ray_matrix_jittered", "ff_set_pixel_jitter", "ff_multi_set_pixel_jitter", "ff_jitter_sequence",
    "ff_taa_params_init", "ff_taa", "ff_taa_reset", "ff_taa_history",
    "ff_light_table", "ff_check_render_params",
    "ff_set_environment", "ff_environment_table", "ff_load_hdr", "ff_free_hdr", "ff_scene_file_environment",
    "ff_display_params_init", "ff_display", "ff_display_to_pbo", "ff_display_reset", "ff_display_state",
    "ff_srgb_thresholds", "ff_display_curve", "ff_display_exposure", "ff_save_hdr",
    "ff_texture_create", "ff_texture_destroy", "ff_set_albedo_texture", "ff_texture_sample", "ff_surface_uv",
    "ff_load_ppm", "ff_free_ppm", "ff_rgb8_to_linear", "ff_scene_file_texture_count", "ff_scene_file_texture", "ff_scene_file_albedo_map",
    "ff_set_roughness", "ff_glossy_eval", "ff_glossy_sample", "ff_scene_file_roughness",
    "ff_camera_sampling_init", "ff_set_camera_sampling", "ff_camera_sample_rays", "ff_scene_file_camera_sampling",
    "ff_upscale_params_init", "ff_upscale", "ff_upscale_host",
    "ff_taa_upscale_params_init", "ff_taa_upscale", "ff_taa_upscale_reset", "ff_taa_upscale_history",
    "ff_motion_blur_params_init", "ff_motion_blur", "ff_motion_blur_host",
    "ff_dof_params_init", "ff_dof_params_from_camera", "ff_depth_of_field", "ff_depth_of_field_host",
    "ff_despeckle_params_init", "ff_despeckle", "ff_despeckle_host",
    "ff_sharpen_params_init", "ff_sharpen", "ff_sharpen_host",
    "ff_local_tonemap_params_init", "ff_local_tonemap", "ff_local_tonemap_host", "ff_local_tonemap_grid_host",
    "ff_interpolate_params_init", "ff_interpolate", "ff_interpolate_host", "ff_interpolate_geometry_maps",
    "ff_adaptive_params_init", "ff_render_adaptive", "ff_adaptive_state", "ff_adaptive_tile_error", "ff_adaptive_tile_error_host", "ff_adaptive_plan_host",
    "ff_yuv_params_init", "ff_yuv_plane_bytes", "ff_yuv_knots", "ff_encode_yuv", "ff_encode_yuv_host", "ff_save_y4m",
    "ff_resize_params_init", "ff_resize_taps", "ff_resize_weights", "ff_resize", "ff_resize_host",
    "ff_grade_params_init", "ff_grade_lut_create", "ff_grade_lut_destroy", "ff_color_grade", "ff_color_grade_host",
    "ff_load_cube", "ff_free_cube", "ff_save_cube",
    "ff_lens_params_init", "ff_lens", "ff_lens_host", "ff_lens_tables", "ff_lens_map_host", "ff_lens_fit_zoom", "ff_debug_lens_table_builds",
]
DIST_ID_BYTES = 128

_lib = None


class FireflyError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"firefly status {status}: {message}")
        self.status = status
        self.message = message


class _Tolerant:
    """Prototype declarations against a library that may lack some symbols."""

    class _Missing:
        argtypes = restype = None

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        try:
            return getattr(self._lib, name)
        except AttributeError:
            return _Tolerant._Missing()


def load():
    """Load libfirefly_hip.so (once) and declare prototypes. Raises if the library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP extension has not been built (run __graft_entry__.build()); "
            "there is no CPU fallback for the trace path")
    real = C.CDLL(LIB_PATH)
    # (an older build loaded through FF_LIB_PATH for an A/B run may lack the newest entry points: skip their prototypes)
    lib = _Tolerant(real) if os.environ.get("FF_LIB_PATH") else real
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    P = C.POINTER
    lib.ff_create.argtypes = [P(vp), i32]
    lib.ff_destroy.argtypes = [vp]
    lib.ff_last_error.restype = C.c_char_p
    lib.ff_version.restype = i32
    lib.ff_set_stream.argtypes = [vp, vp]
    lib.ff_geometry_init.argtypes = [P(T.FfGeometry), i32, T.FfVec3, T.FfVec3, T.FfVec3, P(T.FfTriangle), i32, f32]
    lib.ff_geometry_init.restype = None
    lib.ff_bxdf_init.argtypes = [P(T.FfBXDF)]
    lib.ff_bxdf_init.restype = None
    lib.ff_camera_init_default.argtypes = [P(T.FfCamera), i32, i32]
    lib.ff_camera_init_default.restype = None
    lib.ff_camera_update_basis.argtypes = [P(T.FfCamera)]
    lib.ff_camera_update_basis.restype = None
    lib.ff_camera_ray_matrix.argtypes = [P(T.FfCamera), P(T.FfMat4)]
    lib.ff_camera_ray_matrix.restype = None
    lib.ff_upload_scene.argtypes = [vp, P(T.FfGeometry), i32]
    lib.ff_set_builder.argtypes = [vp, i32]
    lib.ff_update_transforms.argtypes = [vp, P(T.FfGeometry), i32]
    lib.ff_update_mesh.argtypes = [vp, i32, P(T.FfTriangle), i32, i32]
    lib.ff_build_stats.argtypes = [vp, P(T.FfBuildStats)]
    lib.ff_debug_download_bvh.argtypes = [vp, vp, i32, P(i32), vp, i32, P(i32), P(i32), i32]
    lib.ff_debug_download_bvh4.argtypes = [vp, vp, i32, P(i32), P(i32), i32]
    lib.ff_scene_info.argtypes = [P(T.FfGeometry), i32, P(T.FfSceneInfo)]
    lib.ff_debug_wall_table.argtypes = [P(T.FfGeometry), i32, P(C.c_float), i32]
    lib.ff_debug_wall_entries.argtypes = [P(T.FfGeometry), i32]
    lib.ff_render.argtypes = [vp, P(T.FfCamera), P(T.FfRenderParams), vp, i32, vp, i32]
    lib.ff_render_tile.argtypes = [vp, P(T.FfCamera), P(T.FfRenderParams), i32, i32, i32, i32, vp, i32, vp, i32]
    lib.ff_render_strips.argtypes = [vp, P(T.FfCamera), P(T.FfRenderParams), i32, i32, i32, vp, i32, vp, i32, P(i32)]
    lib.ff_strips_local_rows.argtypes = [i32, i32, i32, i32]
    lib.ff_deinterleave_strips.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32]
    lib.ff_intersect_rays.argtypes = [vp, P(T.FfRay), i32, P(T.FfIntersect), i32]
    lib.ff_register_gl_pbo.argtypes = [vp, C.c_uint, i32, i32]
    lib.ff_unregister_gl_pbo.argtypes = [vp]
    lib.ff_render_to_pbo.argtypes = [vp, P(T.FfCamera), P(T.FfRenderParams)]
    lib.ff_render_progressive.argtypes = [vp, P(T.FfCamera), P(T.FfRenderParams), i32, vp, i32, vp, i32]
    lib.ff_render_to_pbo_progressive.argtypes = [vp, P(T.FfCamera), P(T.FfRenderParams), i32]
    lib.ff_save_ppm.argtypes = [C.c_char_p, vp, i32, i32]
    lib.ff_set_collect_stats.argtypes = [vp, i32]
    lib.ff_stats.argtypes = [vp, P(T.FfStats)]
    lib.ff_debug_counters.argtypes = [vp, P(C.c_ulonglong)]
    lib.ff_debug_timeline.argtypes = [vp, P(C.c_uint), P(C.c_int)]
    lib.ff_debug_kernel_name.argtypes = [vp]
    lib.ff_debug_kernel_name.restype = C.c_char_p
    lib.ff_debug_layout.argtypes = [vp, P(i32)]
    lib.ff_debug_stack_spill.argtypes = [vp, i32, P(C.c_ulonglong)]
    lib.ff_debug_check_ieee.argtypes = [vp, P(C.c_ulonglong)]
    lib.ff_debug_reload_switches.argtypes = [vp]
    lib.ff_load_obj.argtypes = [C.c_char_p, P(P(T.FfTriangle)), P(i32)]
    lib.ff_free_triangles.argtypes = [P(T.FfTriangle)]
    lib.ff_free_triangles.restype = None
    lib.ff_scene_file_load.argtypes = [C.c_char_p, P(vp)]
    lib.ff_scene_file_geometries.argtypes = [vp, P(i32)]
    lib.ff_scene_file_geometries.restype = P(T.FfGeometry)
    lib.ff_scene_file_camera.argtypes = [vp, i32, i32, P(T.FfCamera)]
    lib.ff_scene_file_free.argtypes = [vp]
    lib.ff_scene_file_free.restype = None
    lib.ff_dist_unique_id.argtypes = [vp, i32]
    lib.ff_dist_init.argtypes = [vp, i32, i32, vp, i32]
    lib.ff_dist_shutdown.argtypes = [vp]
    lib.ff_debug_dist_fail_rank.argtypes = [vp, C.c_int]
    lib.ff_dist_available.argtypes = []
    lib.ff_dist_strip_rows.argtypes = [i32]
    lib.ff_dist_strip_rows_for.argtypes = [i32, i32]
    lib.ff_dist_part_bytes.argtypes = [i32, i32, i32, i32, i32, P(C.c_longlong)]
    lib.ff_dist_part_bytes.restype = C.c_longlong
    lib.ff_render_distributed.argtypes = [vp, P(T.FfCamera), P(T.FfRenderParams), i32, vp, i32, vp, i32]
    lib.ff_multi_create.argtypes = [P(vp), P(i32), i32]
    lib.ff_multi_destroy.argtypes = [vp]
    lib.ff_multi_count.argtypes = [vp]
    lib.ff_multi_state.argtypes = [vp, i32]
    lib.ff_multi_state.restype = vp
    lib.ff_multi_uses_rccl.argtypes = [vp]
    lib.ff_multi_upload_scene.argtypes = [vp, P(T.FfGeometry), i32]
    lib.ff_multi_render.argtypes = [vp, P(T.FfCamera), P(T.FfRenderParams), i32, vp, i32, vp, i32]
    lib.ff_multi_render_to_pbo.argtypes = [vp, P(T.FfCamera), P(T.FfRenderParams), i32]
    lib.ff_multi_stats.argtypes = [vp, P(T.FfStats)]
    lib.ff_gbuffer.argtypes = [vp, P(T.FfCamera), P(T.FfRenderParams), vp, vp, vp, vp, vp, i32]
    lib.ff_denoise_params_init.argtypes = [P(T.FfDenoiseParams)]
    lib.ff_denoise_params_init.restype = None
    lib.ff_denoise.argtypes = [vp, i32, i32, P(T.FfDenoiseParams), vp, vp, vp, vp, vp, i32, vp, i32, vp, i32]
    lib.ff_temporal_params_init.argtypes = [P(T.FfTemporalParams)]
    lib.ff_temporal_params_init.restype = None
    lib.ff_denoise_temporal.argtypes = [vp, P(T.FfCamera), i32, i32, P(T.FfTemporalParams), vp, vp, vp, vp, vp, i32, vp, i32, vp, i32]
    lib.ff_temporal_reset.argtypes = [vp]
    lib.ff_temporal_history.argtypes = [vp, vp, vp, i32]
    lib.ff_camera_ray_matrix_jittered.argtypes = [P(T.FfCamera), C.c_float, C.c_float, P(T.FfMat4)]
    lib.ff_camera_ray_matrix_jittered.restype = None
    lib.ff_set_pixel_jitter.argtypes = [vp, C.c_float, C.c_float]
    lib.ff_multi_set_pixel_jitter.argtypes = [vp, C.c_float, C.c_float]
    lib.ff_jitter_sequence.argtypes = [i32, i32, P(C.c_float), P(C.c_float)]
    lib.ff_light_table.argtypes = [P(T.FfGeometry), i32, P(T.FfLightEntry), i32, P(C.c_float)]
    lib.ff_check_render_params.argtypes = [P(T.FfRenderParams)]
    lib.ff_set_environment.argtypes = [vp, vp, i32, i32, f32, f32]
    lib.ff_environment_table.argtypes = [vp, i32, i32, vp, vp, vp, vp]
    lib.ff_load_hdr.argtypes = [C.c_char_p, P(P(C.c_float)), P(i32), P(i32)]
    lib.ff_free_hdr.argtypes = [P(C.c_float)]
    lib.ff_free_hdr.restype = None
    lib.ff_scene_file_environment.argtypes = [vp, P(C.c_char_p), P(C.c_float), P(C.c_float)]
    lib.ff_taa_params_init.argtypes = [P(T.FfTaaParams)]
    lib.ff_taa_params_init.restype = None
    lib.ff_taa.argtypes = [vp, P(T.FfCamera), i32, i32, P(T.FfTaaParams), vp, vp, vp, i32, vp, i32, vp, i32]
    lib.ff_taa_reset.argtypes = [vp]
    lib.ff_taa_history.argtypes = [vp, vp, vp, i32]
    # display transform
    lib.ff_display_params_init.argtypes = [P(T.FfDisplayParams)]
    lib.ff_display_params_init.restype = None
    lib.ff_display.argtypes = [vp, i32, i32, P(T.FfDisplayParams), vp, i32, vp, i32, vp, i32]
    lib.ff_display_to_pbo.argtypes = [vp, i32, i32, P(T.FfDisplayParams), vp, i32]
    lib.ff_display_reset.argtypes = [vp]
    lib.ff_display_state.argtypes = [vp, P(f32), P(f32), vp]
    lib.ff_srgb_thresholds.argtypes = [vp]
    lib.ff_display_curve.argtypes = [P(T.FfDisplayParams), vp, i32, vp, vp]
    lib.ff_display_exposure.argtypes = [P(T.FfDisplayParams), vp, f32, P(f32), P(f32)]
    lib.ff_save_hdr.argtypes = [C.c_char_p, vp, i32, i32]
    # albedo textures
    lib.ff_texture_create.argtypes = [vp, vp, i32, i32, i32, P(i32)]
    lib.ff_texture_destroy.argtypes = [vp, i32]
    lib.ff_set_albedo_texture.argtypes = [vp, i32, i32, f32, f32, f32, f32]
    lib.ff_texture_sample.argtypes = [vp, i32, i32, i32, vp, i32, vp]
    lib.ff_surface_uv.argtypes = [P(T.FfGeometry), i32, i32, vp, vp, i32, vp]
    lib.ff_load_ppm.argtypes = [C.c_char_p, P(P(C.c_ubyte)), P(i32), P(i32)]
    lib.ff_free_ppm.argtypes = [P(C.c_ubyte)]
    lib.ff_free_ppm.restype = None
    lib.ff_rgb8_to_linear.argtypes = [vp, i32, i32, vp]
    lib.ff_scene_file_texture_count.argtypes = [vp]
    lib.ff_scene_file_texture.argtypes = [vp, i32, P(C.c_char_p), P(C.c_char_p), P(i32)]
    lib.ff_scene_file_albedo_map.argtypes = [vp, i32, P(i32), P(f32), P(f32)]
    # rough-specular mirrors
    lib.ff_set_roughness.argtypes = [vp, i32, f32]
    lib.ff_glossy_eval.argtypes = [f32, vp, vp, vp, i32, vp, vp]
    lib.ff_glossy_sample.argtypes = [f32, vp, vp, vp, i32, vp, vp, vp]
    lib.ff_scene_file_roughness.argtypes = [vp, i32, P(f32)]
    lib.ff_camera_sampling_init.argtypes = [P(T.FfCameraSampling)]
    lib.ff_camera_sampling_init.restype = None
    lib.ff_set_camera_sampling.argtypes = [vp, P(T.FfCameraSampling)]
    lib.ff_camera_sample_rays.argtypes = [P(T.FfCamera), P(T.FfCameraSampling), f32, f32, i32, C.c_uint64, vp, vp, vp, i32, vp, vp]
    lib.ff_scene_file_camera_sampling.argtypes = [vp, P(T.FfCameraSampling)]
    # guided upsampling
    lib.ff_upscale_params_init.argtypes = [P(T.FfUpscaleParams)]
    lib.ff_upscale_params_init.restype = None
    lib.ff_upscale.argtypes = [vp, P(T.FfUpscaleParams), i32, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, i32, vp, i32, vp, i32]
    lib.ff_upscale_host.argtypes = [P(T.FfUpscaleParams), i32, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.ff_motion_blur_params_init.argtypes = [P(T.FfMotionBlurParams)]
    lib.ff_motion_blur_params_init.restype = None
    lib.ff_motion_blur.argtypes = [vp, i32, i32, P(T.FfMotionBlurParams), vp, vp, vp, i32, vp, i32, vp, i32]
    lib.ff_motion_blur_host.argtypes = [i32, i32, P(T.FfMotionBlurParams), vp, vp, vp, vp, vp]
    lib.ff_dof_params_init.argtypes = [P(T.FfDofParams)]
    lib.ff_dof_params_init.restype = None
    lib.ff_dof_params_from_camera.argtypes = [P(T.FfCamera), P(T.FfCameraSampling), P(T.FfDofParams)]
    lib.ff_depth_of_field.argtypes = [vp, P(T.FfCamera), i32, i32, P(T.FfDofParams), vp, vp, vp, i32, vp, i32, vp, i32]
    lib.ff_depth_of_field_host.argtypes = [P(T.FfCamera), i32, i32, P(T.FfDofParams), vp, vp, vp, vp, vp]
    lib.ff_despeckle_params_init.argtypes = [P(T.FfDespeckleParams)]
    lib.ff_despeckle_params_init.restype = None
    lib.ff_despeckle.argtypes = [vp, i32, i32, P(T.FfDespeckleParams), vp, vp, vp, i32, vp, i32, vp, i32, P(C.c_uint32)]
    lib.ff_despeckle_host.argtypes = [i32, i32, P(T.FfDespeckleParams), vp, vp, vp, vp, vp, P(C.c_uint32)]
    lib.ff_sharpen_params_init.argtypes = [P(T.FfSharpenParams)]
    lib.ff_sharpen_params_init.restype = None
    lib.ff_sharpen.argtypes = [vp, i32, i32, P(T.FfSharpenParams), vp, i32, vp, i32, vp, i32]
    lib.ff_sharpen_host.argtypes = [i32, i32, P(T.FfSharpenParams), vp, vp, vp]
    lib.ff_local_tonemap_params_init.argtypes = [P(T.FfLocalTonemapParams)]
    lib.ff_local_tonemap_params_init.restype = None
    lib.ff_local_tonemap.argtypes = [vp, i32, i32, P(T.FfLocalTonemapParams), vp, i32, vp, i32, vp, i32]
    lib.ff_local_tonemap_host.argtypes = [i32, i32, P(T.FfLocalTonemapParams), vp, vp, vp]
    lib.ff_local_tonemap_grid_host.argtypes = [i32, i32, P(T.FfLocalTonemapParams), vp, vp, vp]
    lib.ff_interpolate_params_init.argtypes = [P(T.FfInterpolateParams)]
    lib.ff_interpolate_params_init.restype = None
    cam = P(T.FfCamera)
    lib.ff_interpolate.argtypes = [vp, i32, i32, P(T.FfInterpolateParams), cam, vp, vp, cam, vp, vp, vp, cam, vp, vp, vp, vp, i32, i32,
                                   vp, i32, vp, i32, vp]
    lib.ff_interpolate_host.argtypes = [i32, i32, P(T.FfInterpolateParams), cam, vp, vp, cam, vp, vp, vp, cam, vp, vp, vp, vp, i32, vp, vp, vp]
    lib.ff_interpolate_geometry_maps.argtypes = [P(T.FfGeometry), P(T.FfGeometry), P(T.FfGeometry), i32, vp, vp]
    lib.ff_adaptive_params_init.argtypes = [P(T.FfAdaptiveParams)]
    lib.ff_adaptive_params_init.restype = None
    lib.ff_render_adaptive.argtypes = [vp, P(T.FfCamera), P(T.FfRenderParams), P(T.FfAdaptiveParams), vp, i32, vp, i32, vp, i32, P(T.FfAdaptiveInfo)]
    lib.ff_adaptive_state.argtypes = [vp, vp, vp, vp, vp, i32]
    lib.ff_adaptive_tile_error.argtypes = [vp, i32, i32, i32, i32, vp, vp, i32, vp]
    lib.ff_adaptive_tile_error_host.argtypes = [i32, i32, i32, i32, vp, vp, vp]
    lib.ff_adaptive_plan_host.argtypes = [i32, i32, vp, vp, i32]
    lib.ff_yuv_params_init.argtypes = [P(T.FfYuvParams)]
    lib.ff_yuv_params_init.restype = None
    lib.ff_yuv_plane_bytes.argtypes = [i32, i32, P(T.FfYuvParams), P(C.c_uint64), P(C.c_uint64)]
    lib.ff_yuv_knots.argtypes = [i32, vp]
    lib.ff_encode_yuv.argtypes = [vp, i32, i32, P(T.FfYuvParams), vp, i32, vp, vp, i32]
    lib.ff_encode_yuv_host.argtypes = [i32, i32, P(T.FfYuvParams), vp, vp, vp]
    lib.ff_save_y4m.argtypes = [C.c_char_p, i32, i32, i32, P(T.FfYuvParams), vp, vp]
    lib.ff_resize_params_init.argtypes = [P(T.FfResizeParams)]
    lib.ff_resize_params_init.restype = None
    lib.ff_resize_taps.argtypes = [i32, i32, i32, P(i32)]
    lib.ff_resize_weights.argtypes = [i32, i32, i32, vp, vp]
    lib.ff_resize.argtypes = [vp, P(T.FfResizeParams), i32, i32, vp, i32, i32, i32, vp, i32, vp, i32]
    lib.ff_resize_host.argtypes = [P(T.FfResizeParams), i32, i32, vp, i32, i32, vp, vp]
    lib.ff_grade_params_init.argtypes = [P(T.FfGradeParams)]
    lib.ff_grade_params_init.restype = None
    lib.ff_grade_lut_create.argtypes = [vp, P(T.FfGradeLut), P(i32)]
    lib.ff_grade_lut_destroy.argtypes = [vp, i32]
    lib.ff_color_grade.argtypes = [vp, P(T.FfGradeParams), i32, i32, vp, i32, vp, i32, vp, i32]
    lib.ff_color_grade_host.argtypes = [P(T.FfGradeParams), P(T.FfGradeLut), i32, i32, vp, vp, vp]
    lib.ff_load_cube.argtypes = [C.c_char_p, P(T.FfCubeFile)]
    lib.ff_free_cube.argtypes = [P(T.FfCubeFile)]
    lib.ff_free_cube.restype = None
    lib.ff_save_cube.argtypes = [C.c_char_p, P(T.FfCubeFile)]
    lib.ff_lens_params_init.argtypes = [P(T.FfLensParams)]
    lib.ff_lens_params_init.restype = None
    lib.ff_lens.argtypes = [vp, i32, i32, P(T.FfLensParams), vp, i32, vp, i32, vp, i32]
    lib.ff_lens_host.argtypes = [i32, i32, P(T.FfLensParams), vp, vp, vp]
    lib.ff_lens_tables.argtypes = [P(T.FfLensParams), i32, i32, vp, vp, P(C.c_double)]
    lib.ff_lens_map_host.argtypes = [P(T.FfLensParams), i32, i32, i32, vp, i32, vp]
    lib.ff_lens_fit_zoom.argtypes = [P(T.FfLensParams), i32, i32, i32, P(f32)]
    lib.ff_debug_lens_table_builds.argtypes = [vp, P(C.c_uint64)]
    lib.ff_taa_upscale_params_init.argtypes = [P(T.FfTaaUpscaleParams)]
    lib.ff_taa_upscale_params_init.restype = None
    lib.ff_taa_upscale.argtypes = [vp, P(T.FfCamera), P(T.FfTaaUpscaleParams), i32, i32, vp, vp, i32, i32, vp, vp, i32, vp, i32, vp, i32]
    lib.ff_taa_upscale_reset.argtypes = [vp]
    lib.ff_taa_upscale_history.argtypes = [vp, vp, vp, i32]
    _lib = real
    return real


def check(status):
    if status != T.FF_OK:
        raise FireflyError(status, load().ff_last_error().decode("utf-8", "replace"))


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


def _vp(q):
    """A raw device pointer (an int; 0 or None: none) as ctypes passes it."""
    return C.c_void_p(q) if q else None


def _image_outputs(h, w, want_rgb8=True, want_out=True, device=None, out=None):
    """The two optional outputs of an image filter for an h x w image: (rgb8 [h,w,3] uint8, out [h,w,3] float32, and the pointer to
    pass for each) - numpy arrays, or torch tensors on `device`; None for an output that is not wanted.  out: the array or tensor
    to use as the float output where one is wanted (an in-place call's)."""
    if device is None:
        new, ptr = (lambda dtype: np.zeros((h, w, 3), dtype=dtype)), (lambda a: a.ctypes.data)
    else:
        import torch
        new, ptr = (lambda dtype: torch.zeros((h, w, 3), dtype=getattr(torch, dtype), device=device)), (lambda a: a.data_ptr())
    rgb8 = new("uint8") if want_rgb8 else None
    out = (out if out is not None else new("float32")) if want_out else None
    return rgb8, out, ptr(rgb8) if want_rgb8 else None, ptr(out) if want_out else None


def _device_image(t, dtype, what, spelled, hw=None):
    """(h, w) of the device tensor `t`, which must be contiguous, on the device, of the torch `dtype` and [H,W,3] (of the size hw,
    where one is given); what and spelled: the tensor and its type as the error names them."""
    h, w = hw if hw is not None else t.shape[:2]
    if not t.is_cuda or t.dtype != dtype or tuple(t.shape) != (h, w, 3) or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous [H,W,3] {spelled} tensor on the device")
    return h, w


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


def _upscale_images(radiance_lo, gbuffer_lo, gbuffer_hi, who):
    """The nine input images of ff_upscale as contiguous arrays, and (h, w), (H, W)."""
    rad = np.ascontiguousarray(radiance_lo, dtype=np.float32)
    names = ("position", "normal", "albedo", "ids")
    lo = {k: np.ascontiguousarray(gbuffer_lo[k], dtype=np.int32 if k == "ids" else np.float32) for k in names}
    hi = {k: np.ascontiguousarray(gbuffer_hi[k], dtype=np.int32 if k == "ids" else np.float32) for k in names}
    h, w = rad.shape[:2]
    H, W = hi["ids"].shape[:2]
    if rad.shape != (h, w, 3) or any(lo[k].shape != (h, w, 3) for k in names) or any(hi[k].shape != (H, W, 3) for k in names):
        raise ValueError(f"{who}: radiance_lo and gbuffer_lo must be [h,w,3] and gbuffer_hi [H,W,3]")
    return rad, lo, hi, (h, w), (H, W)


def upscale_host(radiance_lo, gbuffer_lo, gbuffer_hi, p=None):
    """ff_upscale_host (no GPU): host radiance [h,w,3] with its gbuffer dict and the [H,W] gbuffer dict of the same view
    -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32)."""
    rad, lo, hi, (h, w), (H, W) = _upscale_images(radiance_lo, gbuffer_lo, gbuffer_hi, "upscale_host")
    p = p if p is not None else upscale_params()
    rgb8, out, rgb8_ptr, out_ptr = _image_outputs(H, W)
    check(load().ff_upscale_host(C.byref(p), w, h, rad.ctypes.data, lo["position"].ctypes.data, lo["normal"].ctypes.data, lo["albedo"].ctypes.data,
                                 lo["ids"].ctypes.data, W, H, hi["position"].ctypes.data, hi["normal"].ctypes.data, hi["albedo"].ctypes.data,
                                 hi["ids"].ctypes.data, rgb8_ptr, out_ptr))
    return rgb8, out


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
    p = p if p is not None else motion_blur_params()
    rgb8, out, rgb8_ptr, out_ptr = _image_outputs(h, w, want_rgb8, want_out)
    check(load().ff_motion_blur_host(w, h, C.byref(p), rad.ctypes.data, mot.ctypes.data, dep.ctypes.data, rgb8_ptr, out_ptr))
    return rgb8, out


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
    p = p if p is not None else dof_params()
    rgb8, out, rgb8_ptr, out_ptr = _image_outputs(h, w, want_rgb8, want_out)
    check(load().ff_depth_of_field_host(C.byref(camera), w, h, C.byref(p), rad.ctypes.data, pos.ctypes.data, dep.ctypes.data,
                                        rgb8_ptr, out_ptr))
    return rgb8, out


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
    p = p if p is not None else despeckle_params()
    rgb8, out, rgb8_ptr, out_ptr = _image_outputs(h, w, want_rgb8, want_out)
    clamped = C.c_uint32(0)
    check(load().ff_despeckle_host(w, h, C.byref(p), rad.ctypes.data, alb.ctypes.data if alb is not None else None, ids.ctypes.data,
                                   rgb8_ptr, out_ptr, C.byref(clamped)))
    return rgb8, out, int(clamped.value)


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
    p = p if p is not None else sharpen_params()
    rgb8, out, rgb8_ptr, out_ptr = _image_outputs(h, w, want_rgb8, want_out)
    check(load().ff_sharpen_host(w, h, C.byref(p), rad.ctypes.data, rgb8_ptr, out_ptr))
    return rgb8, out


def local_tonemap_params(**overrides):
    """ff_local_tonemap_params_init's defaults with the given fields replaced (any FfLocalTonemapParams field but reserved)."""
    return _params(T.FfLocalTonemapParams, "ff_local_tonemap_params_init", overrides, fixed=("reserved",))


def local_tonemap_host(radiance, p=None, want_rgb8=True, want_out=True, in_place=False):
    """ff_local_tonemap_host (no GPU): host radiance [H,W,3] -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32).  in_place: the
    radiance output is written over a copy of the input (radiance_out == radiance_in in the call)."""
    rad, (h, w) = _float3_image(radiance, "local_tonemap_host")
    p = p if p is not None else local_tonemap_params()
    rgb8, out, rgb8_ptr, out_ptr = _image_outputs(h, w, want_rgb8, want_out, out=rad.copy() if in_place else None)
    src = out if (in_place and want_out) else rad
    check(load().ff_local_tonemap_host(w, h, C.byref(p), src.ctypes.data, rgb8_ptr, out_ptr))
    return rgb8, out


def local_tonemap_grid_host(radiance, p=None):
    """ff_local_tonemap_grid_host (no GPU): step 2's grid of host radiance [H,W,3] -> (n, S), each [gh, gw, 40] int32."""
    rad, (h, w) = _float3_image(radiance, "local_tonemap_grid_host")
    p = p if p is not None else local_tonemap_params()
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
    p = p if p is not None else yuv_params()
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
    p = p if p is not None else yuv_params()
    luma, chroma = _yuv_planes(h, w, p)
    check(load().ff_encode_yuv_host(w, h, C.byref(p), img.ctypes.data, luma.ctypes.data, chroma.ctypes.data))
    return luma, chroma


def save_y4m(path, luma, chroma, p=None, append=False):
    """ff_save_y4m: one YUV4MPEG2 frame of encode_yuv's host planes; append=False writes the stream header first."""
    p = p if p is not None else yuv_params()
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


def resize_host(radiance, out_width, out_height, p=None, want_rgb8=True, want_out=True):
    """ff_resize_host (no GPU): host radiance [H,W,3] -> (rgb8 [H',W',3] uint8, radiance [H',W',3] float32)."""
    rad, (h, w) = _float3_image(radiance, "resize_host")
    p = p if p is not None else resize_params()
    # (a size the library refuses still gets arrays: the call names it)
    rgb8, out, rgb8_ptr, out_ptr = _image_outputs(max(int(out_height), 0), max(int(out_width), 0), want_rgb8, want_out)
    check(load().ff_resize_host(C.byref(p), w, h, rad.ctypes.data, out_width, out_height, rgb8_ptr, out_ptr))
    return rgb8, out


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
    p = p if p is not None else grade_params()
    rgb8, out, rgb8_ptr, out_ptr = _image_outputs(h, w, want_rgb8, want_out, out=rad.copy() if in_place else None)
    src = out if (in_place and want_out) else rad
    check(load().ff_color_grade_host(C.byref(p), _lut_ref(lut), w, h, src.ctypes.data, rgb8_ptr, out_ptr))
    return rgb8, out


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
    p = p if p is not None else lens_params()
    rgb8, out, rgb8_ptr, out_ptr = _image_outputs(h, w, want_rgb8, want_out)
    check(load().ff_lens_host(w, h, C.byref(p), rad.ctypes.data, rgb8_ptr, out_ptr))
    return rgb8, out


def lens_tables(width, height, p=None):
    """ff_lens_tables -> (e float32 [LENS_KNOTS + 1], gain float32 [LENS_KNOTS + 1], r2_max) as the kernel gets them."""
    p = p if p is not None else lens_params()
    e = np.zeros(T.LENS_KNOTS + 1, dtype=np.float32)
    gain = np.zeros(T.LENS_KNOTS + 1, dtype=np.float32)
    r2_max = C.c_double(0.0)
    check(load().ff_lens_tables(C.byref(p), width, height, e.ctypes.data, gain.ctypes.data, C.byref(r2_max)))
    return e, gain, float(r2_max.value)


def lens_map(width, height, xy_out, p=None, channel=1):
    """ff_lens_map_host: output positions [n,2] (x y in pixels, a pixel's centre at + 0.5) -> the source positions float32 [n,2] of
    `channel` (0 red, 1 green, 2 blue)."""
    p = p if p is not None else lens_params()
    xy = np.ascontiguousarray(xy_out, dtype=np.float32)
    if xy.ndim != 2 or xy.shape[1] != 2:
        raise ValueError("lens_map: xy_out must be [n,2]")
    src = np.zeros_like(xy)
    check(load().ff_lens_map_host(C.byref(p), width, height, channel, xy.ctypes.data, xy.shape[0], src.ctypes.data))
    return src


def lens_fit_zoom(width, height, p=None, mode=T.LENS_FIT_FILL):
    """ff_lens_fit_zoom -> the zoom that fills the frame (LENS_FIT_FILL) or keeps the whole source in view (LENS_FIT_ALL)."""
    p = p if p is not None else lens_params()
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
    p = p if p is not None else interpolate_params()
    rgb8, out, rgb8_ptr, out_ptr = _image_outputs(h, w, want_rgb8, want_out)
    counts = np.zeros(5, dtype=np.uint32)
    d = [x.ctypes.data for x in im]
    check(load().ff_interpolate_host(w, h, C.byref(p), C.byref(cams[0]), d[0], d[1], C.byref(cams[1]), d[2], d[3], d[4], C.byref(cams[2]), d[5], d[6], d[7],
                                     maps.ctypes.data if maps is not None else None, n, rgb8_ptr, out_ptr,
                                     counts.ctypes.data))
    return rgb8, out, counts


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


GBUFFER_CHANNELS = (("depth", np.float32, ()), ("position", np.float32, (3,)), ("normal", np.float32, (3,)), ("albedo", np.float32, (3,)),
                    ("ids", np.int32, (3,)))


# the eight values of ff_debug_layout, in order
LAYOUT_FIELDS = ("scene_block_threads", "stack_entries", "stack_lds_levels", "lds_cap", "setup_threshold", "leaf_threshold", "max_depth4", "top_depth")


class Tracer:
    """Owner of one FfState (one HIP device). Mirrors the call sequence of the reference's main():
    upload once (kernel.cu:268-298), then render per frame (kernel.cu:335-344)."""

    def __init__(self, device_id=0):
        self._lib = load()
        self._state = C.c_void_p()
        check(self._lib.ff_create(C.byref(self._state), device_id))
        self._scene_keepalive = None

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
        h, w = params.height, params.width
        rgb8 = np.zeros((h, w, 3), dtype=np.uint8) if want_rgb8 else None
        rad = np.zeros((h, w, 3), dtype=np.float32) if want_radiance else None
        check(self._lib.ff_render(self._state, C.byref(camera), C.byref(params),
                                  rgb8.ctypes.data if want_rgb8 else None, 0,
                                  rad.ctypes.data if want_radiance else None, 0))
        return rgb8, rad

    def render_progressive(self, camera, params, frame_index):
        """Frame `frame_index` of a progressive sequence -> (rgb8, radiance) of the mean over frames 0..frame_index."""
        h, w = params.height, params.width
        rgb8 = np.zeros((h, w, 3), dtype=np.uint8)
        rad = np.zeros((h, w, 3), dtype=np.float32)
        check(self._lib.ff_render_progressive(self._state, C.byref(camera), C.byref(params), frame_index, rgb8.ctypes.data, 0, rad.ctypes.data, 0))
        return rgb8, rad

    def render_tile(self, camera, params, x0, y0, w, h):
        """Tile [x0, x0+w) x [y0, y0+h) of the frame -> (rgb8 [h,w,3], radiance [h,w,3])."""
        rgb8 = np.zeros((h, w, 3), dtype=np.uint8)
        rad = np.zeros((h, w, 3), dtype=np.float32)
        check(self._lib.ff_render_tile(self._state, C.byref(camera), C.byref(params), x0, y0, w, h, rgb8.ctypes.data, 0, rad.ctypes.data, 0))
        return rgb8, rad

    def render_adaptive(self, camera, params, ap=None):
        """ff_render_adaptive: passes of params.spp samples (seed, seed + 1, ...) until every tile's error estimate is below
        ap.threshold -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32, passes [H,W] uint16, FfAdaptiveInfo)."""
        ap = ap if ap is not None else adaptive_params()
        h, w = params.height, params.width
        rgb8 = np.zeros((h, w, 3), dtype=np.uint8)
        rad = np.zeros((h, w, 3), dtype=np.float32)
        passes = np.zeros((h, w), dtype=np.uint16)
        info = T.FfAdaptiveInfo()
        check(self._lib.ff_render_adaptive(self._state, C.byref(camera), C.byref(params), C.byref(ap), rgb8.ctypes.data, 0, rad.ctypes.data, 0,
                                           passes.ctypes.data, 0, C.byref(info)))
        return rgb8, rad, passes, info

    def render_adaptive_device(self, camera, params, ap=None, rgb8_ptr=None, radiance_ptr=None, passes_ptr=None):
        """ff_render_adaptive into caller-owned DEVICE buffers (raw pointers; each may be None) -> FfAdaptiveInfo."""
        ap = ap if ap is not None else adaptive_params()
        info = T.FfAdaptiveInfo()
        check(self._lib.ff_render_adaptive(self._state, C.byref(camera), C.byref(params), C.byref(ap), _vp(rgb8_ptr), 1, _vp(radiance_ptr), 1, _vp(passes_ptr), 1,
                                           C.byref(info)))
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
        check(self._lib.ff_render(self._state, C.byref(camera), C.byref(params),
                                  C.c_void_p(rgb8_ptr) if rgb8_ptr else None, 1,
                                  C.c_void_p(radiance_ptr) if radiance_ptr else None, 1))

    def gbuffer(self, camera, params):
        """What every pixel's primary ray hits (ff_gbuffer) -> dict of numpy arrays: depth [H,W] float32, position / normal / albedo
        [H,W,3] float32, ids [H,W,3] int32 (geometry, triangle, bxdf type; -1 on a miss)."""
        h, w = params.height, params.width
        out = {name: np.zeros((h, w) + shape, dtype=dt) for name, dt, shape in GBUFFER_CHANNELS}
        check(self._lib.ff_gbuffer(self._state, C.byref(camera), C.byref(params), *(out[name].ctypes.data for name, _, _ in GBUFFER_CHANNELS), 0))
        return out

    def gbuffer_device(self, camera, params, depth_ptr=None, position_ptr=None, normal_ptr=None, albedo_ptr=None, ids_ptr=None):
        """ff_gbuffer into caller-owned DEVICE buffers (raw pointers; any may be None)."""
        ptrs = [C.c_void_p(p) if p else None for p in (depth_ptr, position_ptr, normal_ptr, albedo_ptr, ids_ptr)]
        check(self._lib.ff_gbuffer(self._state, C.byref(camera), C.byref(params), *ptrs, 1))

    def denoise(self, radiance, gbuffer, dn=None):
        """ff_denoise of host radiance [H,W,3] guided by a gbuffer() dict -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32)."""
        rad = np.ascontiguousarray(radiance, dtype=np.float32)
        h, w = rad.shape[:2]
        dn = dn if dn is not None else denoise_params()
        g = {k: np.ascontiguousarray(gbuffer[k], dtype=np.int32 if k == "ids" else np.float32) for k in ("position", "normal", "albedo", "ids")}
        rgb8, out, rgb8_ptr, out_ptr = _image_outputs(h, w)
        check(self._lib.ff_denoise(self._state, w, h, C.byref(dn), rad.ctypes.data, g["position"].ctypes.data, g["normal"].ctypes.data,
                                   g["albedo"].ctypes.data, g["ids"].ctypes.data, 0, rgb8_ptr, 0, out_ptr, 0))
        return rgb8, out

    def denoise_device(self, width, height, radiance_ptr, position_ptr, normal_ptr, albedo_ptr, ids_ptr, dn=None, rgb8_ptr=None, radiance_out_ptr=None):
        """ff_denoise on DEVICE buffers (raw pointers); radiance_out_ptr may equal radiance_ptr."""
        dn = dn if dn is not None else denoise_params()
        check(self._lib.ff_denoise(self._state, width, height, C.byref(dn), _vp(radiance_ptr), _vp(position_ptr), _vp(normal_ptr), _vp(albedo_ptr),
                                   _vp(ids_ptr), 1, _vp(rgb8_ptr), 1, _vp(radiance_out_ptr), 1))

    def denoise_temporal(self, radiance, gbuffer, camera, tp=None):
        """ff_denoise_temporal of this frame's host radiance [H,W,3] guided by gbuffer() of `camera`; the history stays in the state
        -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32)."""
        rad = np.ascontiguousarray(radiance, dtype=np.float32)
        h, w = rad.shape[:2]
        if rad.shape != (h, w, 3) or any(np.shape(gbuffer[k])[:2] != (h, w) for k in ("position", "normal", "albedo", "ids")):
            raise ValueError("denoise_temporal: radiance must be [H,W,3] and the G-buffer of the same size")
        tp = tp if tp is not None else temporal_params()
        g = {k: np.ascontiguousarray(gbuffer[k], dtype=np.int32 if k == "ids" else np.float32) for k in ("position", "normal", "albedo", "ids")}
        rgb8, out, rgb8_ptr, out_ptr = _image_outputs(h, w)
        check(self._lib.ff_denoise_temporal(self._state, C.byref(camera), w, h, C.byref(tp), rad.ctypes.data, g["position"].ctypes.data,
                                            g["normal"].ctypes.data, g["albedo"].ctypes.data, g["ids"].ctypes.data, 0, rgb8_ptr, 0, out_ptr, 0))
        self._temporal_size = (h, w)
        return rgb8, out

    def denoise_temporal_device(self, camera, width, height, radiance_ptr, position_ptr, normal_ptr, albedo_ptr, ids_ptr, tp=None, rgb8_ptr=None,
                                radiance_out_ptr=None):
        """ff_denoise_temporal on DEVICE buffers (raw pointers); radiance_out_ptr may equal radiance_ptr."""
        tp = tp if tp is not None else temporal_params()
        check(self._lib.ff_denoise_temporal(self._state, C.byref(camera), width, height, C.byref(tp), _vp(radiance_ptr), _vp(position_ptr),
                                            _vp(normal_ptr), _vp(albedo_ptr), _vp(ids_ptr), 1, _vp(rgb8_ptr), 1, _vp(radiance_out_ptr), 1))
        self._temporal_size = (height, width)

    def temporal_reset(self):
        """Drop the temporal history (ff_temporal_reset)."""
        check(self._lib.ff_temporal_reset(self._state))

    def temporal_history(self):
        """The last denoise_temporal call's (motion [H,W,2] float32, history length [H,W] float32)."""
        h, w = getattr(self, "_temporal_size", (0, 0))
        motion = np.zeros((h, w, 2), dtype=np.float32)
        length = np.zeros((h, w), dtype=np.float32)
        check(self._lib.ff_temporal_history(self._state, motion.ctypes.data if h * w else None, length.ctypes.data if h * w else None, 0))
        return motion, length

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
        p = p if p is not None else taa_params()
        pos = np.ascontiguousarray(gbuffer["position"], dtype=np.float32)
        ids = np.ascontiguousarray(gbuffer["ids"], dtype=np.int32)
        rgb8, out, rgb8_ptr, out_ptr = _image_outputs(h, w)
        check(self._lib.ff_taa(self._state, C.byref(camera), w, h, C.byref(p), rad.ctypes.data, pos.ctypes.data, ids.ctypes.data, 0,
                               rgb8_ptr, 0, out_ptr, 0))
        self._taa_size = (h, w)
        return rgb8, out

    def taa_device(self, camera, width, height, radiance_ptr, position_ptr, ids_ptr, p=None, rgb8_ptr=None, radiance_out_ptr=None):
        """ff_taa on DEVICE buffers (raw pointers); radiance_out_ptr may equal radiance_ptr."""
        p = p if p is not None else taa_params()
        check(self._lib.ff_taa(self._state, C.byref(camera), width, height, C.byref(p), _vp(radiance_ptr), _vp(position_ptr), _vp(ids_ptr), 1,
                               _vp(rgb8_ptr), 1, _vp(radiance_out_ptr), 1))
        self._taa_size = (height, width)

    def taa_reset(self):
        """Drop the TAA history (ff_taa_reset)."""
        check(self._lib.ff_taa_reset(self._state))

    def taa_history(self):
        """The last taa call's (motion [H,W,2] float32, history length [H,W] float32)."""
        h, w = getattr(self, "_taa_size", (0, 0))
        motion = np.zeros((h, w, 2), dtype=np.float32)
        length = np.zeros((h, w), dtype=np.float32)
        check(self._lib.ff_taa_history(self._state, motion.ctypes.data if h * w else None, length.ctypes.data if h * w else None, 0))
        return motion, length

    def upscale(self, radiance_lo, gbuffer_lo, gbuffer_hi, p=None):
        """ff_upscale of host radiance [h,w,3] with its gbuffer() dict, guided by the [H,W] gbuffer() dict of the same view (p: the
        jitters both were made with) -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32)."""
        rad, lo, hi, (h, w), (H, W) = _upscale_images(radiance_lo, gbuffer_lo, gbuffer_hi, "upscale")
        p = p if p is not None else upscale_params()
        rgb8, out, rgb8_ptr, out_ptr = _image_outputs(H, W)
        check(self._lib.ff_upscale(self._state, C.byref(p), w, h, rad.ctypes.data, lo["position"].ctypes.data, lo["normal"].ctypes.data,
                                   lo["albedo"].ctypes.data, lo["ids"].ctypes.data, W, H, hi["position"].ctypes.data, hi["normal"].ctypes.data,
                                   hi["albedo"].ctypes.data, hi["ids"].ctypes.data, 0, rgb8_ptr, 0, out_ptr, 0))
        return rgb8, out

    def upscale_device(self, lo_width, lo_height, radiance_lo_ptr, position_lo_ptr, normal_lo_ptr, albedo_lo_ptr, ids_lo_ptr, width, height, position_ptr,
                       normal_ptr, albedo_ptr, ids_ptr, p=None, rgb8_ptr=None, radiance_out_ptr=None):
        """ff_upscale on DEVICE buffers (raw pointers); the outputs must not overlap an input."""
        p = p if p is not None else upscale_params()
        check(self._lib.ff_upscale(self._state, C.byref(p), lo_width, lo_height, _vp(radiance_lo_ptr), _vp(position_lo_ptr), _vp(normal_lo_ptr),
                                   _vp(albedo_lo_ptr), _vp(ids_lo_ptr), width, height, _vp(position_ptr), _vp(normal_ptr), _vp(albedo_ptr), _vp(ids_ptr), 1,
                                   _vp(rgb8_ptr), 1, _vp(radiance_out_ptr), 1))

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
        p = p if p is not None else taa_upscale_params()
        rgb8, out, rgb8_ptr, out_ptr = _image_outputs(H, W)
        check(self._lib.ff_taa_upscale(self._state, C.byref(camera), C.byref(p), w, h, rad.ctypes.data, ids_lo.ctypes.data, W, H, pos.ctypes.data,
                                       ids.ctypes.data, 0, rgb8_ptr, 0, out_ptr, 0))
        self._taa_upscale_size = (H, W)
        return rgb8, out

    def taa_upscale_device(self, camera, lo_width, lo_height, radiance_lo_ptr, ids_lo_ptr, width, height, position_ptr, ids_ptr, p=None, rgb8_ptr=None,
                           radiance_out_ptr=None):
        """ff_taa_upscale on DEVICE buffers (raw pointers); the outputs must not overlap an input."""
        p = p if p is not None else taa_upscale_params()
        check(self._lib.ff_taa_upscale(self._state, C.byref(camera), C.byref(p), lo_width, lo_height, _vp(radiance_lo_ptr), _vp(ids_lo_ptr), width, height,
                                       _vp(position_ptr), _vp(ids_ptr), 1, _vp(rgb8_ptr), 1, _vp(radiance_out_ptr), 1))
        self._taa_upscale_size = (height, width)

    def taa_upscale_reset(self):
        """Drop the temporal upsampler's history (ff_taa_upscale_reset)."""
        check(self._lib.ff_taa_upscale_reset(self._state))

    def taa_upscale_history(self):
        """The last taa_upscale call's (motion [H,W,2] float32, history length [H,W] float32)."""
        h, w = getattr(self, "_taa_upscale_size", (0, 0))
        motion = np.zeros((h, w, 2), dtype=np.float32)
        length = np.zeros((h, w), dtype=np.float32)
        check(self._lib.ff_taa_upscale_history(self._state, motion.ctypes.data if h * w else None, length.ctypes.data if h * w else None, 0))
        return motion, length

    def motion_blur(self, radiance, motion, depth, p=None, want_rgb8=True, want_out=True):
        """ff_motion_blur of host radiance [H,W,3] with the motion [H,W,2] of a *_history call and gbuffer()'s depth [H,W]
        -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32)."""
        rad, mot, dep, (h, w) = _motion_blur_images(radiance, motion, depth, "motion_blur")
        p = p if p is not None else motion_blur_params()
        rgb8, out, rgb8_ptr, out_ptr = _image_outputs(h, w, want_rgb8, want_out)
        check(self._lib.ff_motion_blur(self._state, w, h, C.byref(p), rad.ctypes.data, mot.ctypes.data, dep.ctypes.data, 0,
                                       rgb8_ptr, 0, out_ptr, 0))
        return rgb8, out

    def motion_blur_device(self, width, height, radiance_ptr, motion_ptr, depth_ptr, p=None, rgb8_ptr=None, radiance_out_ptr=None):
        """ff_motion_blur on DEVICE buffers (raw pointers); the outputs must not overlap an input."""
        p = p if p is not None else motion_blur_params()
        check(self._lib.ff_motion_blur(self._state, width, height, C.byref(p), _vp(radiance_ptr), _vp(motion_ptr), _vp(depth_ptr), 1, _vp(rgb8_ptr), 1,
                                       _vp(radiance_out_ptr), 1))

    def depth_of_field(self, radiance, gbuffer_or_planes, camera, p=None, want_rgb8=True, want_out=True):
        """ff_depth_of_field of host radiance [H,W,3] with a gbuffer() dict of `camera` (or its (position [H,W,3], depth [H,W])
        planes) -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32)."""
        rad, pos, dep, (h, w) = _dof_images(radiance, gbuffer_or_planes, "depth_of_field")
        p = p if p is not None else dof_params()
        rgb8, out, rgb8_ptr, out_ptr = _image_outputs(h, w, want_rgb8, want_out)
        check(self._lib.ff_depth_of_field(self._state, C.byref(camera), w, h, C.byref(p), rad.ctypes.data, pos.ctypes.data, dep.ctypes.data, 0,
                                          rgb8_ptr, 0, out_ptr, 0))
        return rgb8, out

    def depth_of_field_device(self, camera, width, height, radiance_ptr, position_ptr, depth_ptr, p=None, rgb8_ptr=None, radiance_out_ptr=None):
        """ff_depth_of_field on DEVICE buffers (raw pointers); the outputs must not overlap an input."""
        p = p if p is not None else dof_params()
        check(self._lib.ff_depth_of_field(self._state, C.byref(camera), width, height, C.byref(p), _vp(radiance_ptr), _vp(position_ptr), _vp(depth_ptr), 1,
                                          _vp(rgb8_ptr), 1, _vp(radiance_out_ptr), 1))

    def despeckle(self, radiance, gbuffer_or_planes, p=None, want_rgb8=True, want_out=True):
        """ff_despeckle of radiance [H,W,3] with a gbuffer() dict (or its (albedo, ids) planes; albedo None without
        FF_DESPECKLE_DEMODULATE_ALBEDO) -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32, the number of clamped pixels).  Host
        arrays give host arrays; contiguous device tensors (torch, float32 / int32) give device tensors."""
        p = p if p is not None else despeckle_params()
        if hasattr(radiance, "data_ptr"):
            import torch
            albedo, ids = _despeckle_planes(gbuffer_or_planes)
            h, w = radiance.shape[:2]
            for name, t, dtype in (("radiance", radiance, torch.float32), ("albedo", albedo, torch.float32), ("ids", ids, torch.int32)):
                if t is not None:
                    _device_image(t, dtype, f"despeckle: {name}", dtype, (h, w))
            rgb8, out, rgb8_ptr, out_ptr = _image_outputs(h, w, want_rgb8, want_out, radiance.device)
            torch.cuda.synchronize(radiance.device)
            clamped = self.despeckle_device(w, h, radiance.data_ptr(), albedo.data_ptr() if albedo is not None else None, ids.data_ptr(), p, rgb8_ptr,
                                            out_ptr)
            return rgb8, out, clamped
        rad, alb, idp, (h, w) = _despeckle_images(radiance, gbuffer_or_planes, "despeckle")
        rgb8, out, rgb8_ptr, out_ptr = _image_outputs(h, w, want_rgb8, want_out)
        clamped = C.c_uint32(0)
        check(self._lib.ff_despeckle(self._state, w, h, C.byref(p), rad.ctypes.data, alb.ctypes.data if alb is not None else None, idp.ctypes.data, 0,
                                     rgb8_ptr, 0, out_ptr, 0, C.byref(clamped)))
        return rgb8, out, int(clamped.value)

    def despeckle_device(self, width, height, radiance_ptr, albedo_ptr, ids_ptr, p=None, rgb8_ptr=None, radiance_out_ptr=None, want_count=True):
        """ff_despeckle on DEVICE buffers (raw pointers); the outputs must not overlap an input -> the number of clamped pixels
        (None with want_count=False: out_clamped is passed as NULL)."""
        p = p if p is not None else despeckle_params()
        clamped = C.c_uint32(0)
        check(self._lib.ff_despeckle(self._state, width, height, C.byref(p), _vp(radiance_ptr), _vp(albedo_ptr), _vp(ids_ptr), 1, _vp(rgb8_ptr), 1,
                                     _vp(radiance_out_ptr), 1, C.byref(clamped) if want_count else None))
        return int(clamped.value) if want_count else None

    def sharpen(self, radiance, p=None, want_rgb8=True, want_out=True):
        """ff_sharpen of radiance [H,W,3] -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32).  A host array gives host arrays; a
        contiguous float32 device tensor (torch) gives device tensors."""
        p = p if p is not None else sharpen_params()
        if hasattr(radiance, "data_ptr"):
            import torch
            h, w = _device_image(radiance, torch.float32, "sharpen: radiance", "float32")
            rgb8, out, rgb8_ptr, out_ptr = _image_outputs(h, w, want_rgb8, want_out, radiance.device)
            torch.cuda.synchronize(radiance.device)
            self.sharpen_device(w, h, radiance.data_ptr(), p, rgb8_ptr, out_ptr)
            return rgb8, out
        rad, (h, w) = _float3_image(radiance, "sharpen")
        rgb8, out, rgb8_ptr, out_ptr = _image_outputs(h, w, want_rgb8, want_out)
        check(self._lib.ff_sharpen(self._state, w, h, C.byref(p), rad.ctypes.data, 0, rgb8_ptr, 0, out_ptr, 0))
        return rgb8, out

    def sharpen_device(self, width, height, radiance_ptr, p=None, rgb8_ptr=None, radiance_out_ptr=None):
        """ff_sharpen on DEVICE buffers (raw pointers); the outputs must not overlap the input."""
        p = p if p is not None else sharpen_params()
        check(self._lib.ff_sharpen(self._state, width, height, C.byref(p), _vp(radiance_ptr), 1, _vp(rgb8_ptr), 1, _vp(radiance_out_ptr), 1))

    def local_tonemap(self, radiance, p=None, want_rgb8=True, want_out=True, in_place=False):
        """ff_local_tonemap of radiance [H,W,3] -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32).  A host array gives host arrays; a
        contiguous float32 device tensor (torch) gives device tensors.  in_place: radiance_out is radiance_in in the call (a device
        tensor is overwritten and returned; a host array is copied first)."""
        p = p if p is not None else local_tonemap_params()
        if hasattr(radiance, "data_ptr"):
            import torch
            h, w = _device_image(radiance, torch.float32, "local_tonemap: radiance", "float32")
            rgb8, out, rgb8_ptr, out_ptr = _image_outputs(h, w, want_rgb8, want_out, radiance.device, out=radiance if in_place else None)
            torch.cuda.synchronize(radiance.device)
            self.local_tonemap_device(w, h, radiance.data_ptr(), p, rgb8_ptr, out_ptr)
            return rgb8, out
        rad, (h, w) = _float3_image(radiance, "local_tonemap")
        rgb8, out, rgb8_ptr, out_ptr = _image_outputs(h, w, want_rgb8, want_out, out=rad.copy() if in_place else None)
        src = out if (in_place and want_out) else rad
        check(self._lib.ff_local_tonemap(self._state, w, h, C.byref(p), src.ctypes.data, 0, rgb8_ptr, 0, out_ptr, 0))
        return rgb8, out

    def local_tonemap_device(self, width, height, radiance_ptr, p=None, rgb8_ptr=None, radiance_out_ptr=None):
        """ff_local_tonemap on DEVICE buffers (raw pointers); radiance_out_ptr may be radiance_ptr."""
        p = p if p is not None else local_tonemap_params()
        check(self._lib.ff_local_tonemap(self._state, width, height, C.byref(p), _vp(radiance_ptr), 1, _vp(rgb8_ptr), 1, _vp(radiance_out_ptr), 1))

    def encode_yuv(self, linear, p=None):
        """ff_encode_yuv of host display-linear [H,W,3] -> (luma [H,W], chroma [ceil(H/2),ceil(W/2),2] of Cb Cr pairs), host arrays:
        uint8 codes at depth 8 (NV12), uint16 codes << 6 at depth 10 (P010)."""
        img, (h, w) = _float3_image(linear, "encode_yuv")
        p = p if p is not None else yuv_params()
        luma, chroma = _yuv_planes(h, w, p)
        check(self._lib.ff_encode_yuv(self._state, w, h, C.byref(p), img.ctypes.data, 0, luma.ctypes.data, chroma.ctypes.data, 0))
        return luma, chroma

    def encode_yuv_device(self, linear, p=None, luma=None, chroma=None):
        """ff_encode_yuv on DEVICE tensors (torch): linear a contiguous [H,W,3] float32 tensor -> (luma, chroma) tensors laid out as
        encode_yuv's arrays (uint8 at depth 8, int16 holding the uint16 bit patterns otherwise).  luma / chroma: contiguous tensors
        of at least the planes' bytes to write into (any dtype and shape; returned as given); they must not overlap the input or
        each other."""
        import torch
        p = p if p is not None else yuv_params()
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
        check(self._lib.ff_encode_yuv(self._state, w, h, C.byref(p), C.c_void_p(linear.data_ptr()), 1, C.c_void_p(luma.data_ptr()),
                                      C.c_void_p(chroma.data_ptr()), 1))
        return luma, chroma

    def resize(self, radiance, out_width, out_height, p=None, want_rgb8=True, want_out=True):
        """ff_resize of radiance [H,W,3] -> (rgb8 [H',W',3] uint8, radiance [H',W',3] float32).  A host array gives host arrays; a
        contiguous float32 device tensor (torch) gives device tensors."""
        p = p if p is not None else resize_params()
        oh, ow = max(int(out_height), 0), max(int(out_width), 0)
        if hasattr(radiance, "data_ptr"):
            import torch
            h, w = _device_image(radiance, torch.float32, "resize: radiance", "float32")
            rgb8, out, rgb8_ptr, out_ptr = _image_outputs(oh, ow, want_rgb8, want_out, radiance.device)
            torch.cuda.synchronize(radiance.device)
            self.resize_device(w, h, radiance.data_ptr(), out_width, out_height, p, rgb8_ptr, out_ptr)
            return rgb8, out
        rad, (h, w) = _float3_image(radiance, "resize")
        rgb8, out, rgb8_ptr, out_ptr = _image_outputs(oh, ow, want_rgb8, want_out)
        check(self._lib.ff_resize(self._state, C.byref(p), w, h, rad.ctypes.data, 0, out_width, out_height, rgb8_ptr, 0, out_ptr, 0))
        return rgb8, out

    def resize_device(self, in_width, in_height, radiance_ptr, out_width, out_height, p=None, rgb8_ptr=None, radiance_out_ptr=None):
        """ff_resize on DEVICE buffers (raw pointers); the outputs must not overlap the input or each other."""
        p = p if p is not None else resize_params()
        check(self._lib.ff_resize(self._state, C.byref(p), in_width, in_height, _vp(radiance_ptr), 1, out_width, out_height, _vp(rgb8_ptr), 1,
                                  _vp(radiance_out_ptr), 1))

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
        p = p if p is not None else grade_params()
        if hasattr(radiance, "data_ptr"):
            import torch
            h, w = _device_image(radiance, torch.float32, "color_grade: radiance", "float32")
            rgb8, out, rgb8_ptr, out_ptr = _image_outputs(h, w, want_rgb8, want_out, radiance.device, out=radiance if in_place else None)
            torch.cuda.synchronize(radiance.device)
            self.color_grade_device(w, h, radiance.data_ptr(), p, rgb8_ptr, out_ptr)
            return rgb8, out
        rad, (h, w) = _float3_image(radiance, "color_grade")
        rgb8, out, rgb8_ptr, out_ptr = _image_outputs(h, w, want_rgb8, want_out, out=rad.copy() if in_place else None)
        src = out if (in_place and want_out) else rad
        check(self._lib.ff_color_grade(self._state, C.byref(p), w, h, src.ctypes.data, 0, rgb8_ptr, 0, out_ptr, 0))
        return rgb8, out

    def color_grade_device(self, width, height, radiance_ptr, p=None, rgb8_ptr=None, radiance_out_ptr=None):
        """ff_color_grade on DEVICE buffers (raw pointers); radiance_out_ptr may be radiance_ptr."""
        p = p if p is not None else grade_params()
        check(self._lib.ff_color_grade(self._state, C.byref(p), width, height, _vp(radiance_ptr), 1, _vp(rgb8_ptr), 1, _vp(radiance_out_ptr), 1))

    def lens(self, radiance, p=None, want_rgb8=True, want_out=True):
        """ff_lens of radiance [H,W,3] -> (rgb8 [H,W,3] uint8, radiance [H,W,3] float32).  A host array gives host arrays; a
        contiguous float32 device tensor (torch) gives device tensors."""
        p = p if p is not None else lens_params()
        if hasattr(radiance, "data_ptr"):
            import torch
            h, w = _device_image(radiance, torch.float32, "lens: radiance", "float32")
            rgb8, out, rgb8_ptr, out_ptr = _image_outputs(h, w, want_rgb8, want_out, radiance.device)
            torch.cuda.synchronize(radiance.device)
            self.lens_device(w, h, radiance.data_ptr(), p, rgb8_ptr, out_ptr)
            return rgb8, out
        rad, (h, w) = _float3_image(radiance, "lens")
        rgb8, out, rgb8_ptr, out_ptr = _image_outputs(h, w, want_rgb8, want_out)
        check(self._lib.ff_lens(self._state, w, h, C.byref(p), rad.ctypes.data, 0, rgb8_ptr, 0, out_ptr, 0))
        return rgb8, out

    def lens_device(self, width, height, radiance_ptr, p=None, rgb8_ptr=None, radiance_out_ptr=None):
        """ff_lens on DEVICE buffers (raw pointers); the outputs must not overlap the input."""
        p = p if p is not None else lens_params()
        check(self._lib.ff_lens(self._state, width, height, C.byref(p), _vp(radiance_ptr), 1, _vp(rgb8_ptr), 1, _vp(radiance_out_ptr), 1))

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
        p = p if p is not None else interpolate_params()
        rgb8, out, rgb8_ptr, out_ptr = _image_outputs(h, w, want_rgb8, want_out)
        counts = np.zeros(5, dtype=np.uint32)
        d = [x.ctypes.data for x in im]
        check(self._lib.ff_interpolate(self._state, w, h, C.byref(p), C.byref(cams[0]), d[0], d[1], C.byref(cams[1]), d[2], d[3], d[4], C.byref(cams[2]),
                                       d[5], d[6], d[7], maps.ctypes.data if maps is not None else None, n, 0, rgb8_ptr, 0, out_ptr,
                                       0, counts.ctypes.data))
        return rgb8, out, counts

    def interpolate_device(self, width, height, cameras, image_ptrs, p=None, geom_maps=None, rgb8_ptr=None, radiance_out_ptr=None, want_counts=True):
        """ff_interpolate on DEVICE buffers (raw pointers): cameras = (mid, a, b); image_ptrs = the eight images in the C call's order
        (position, ids, radiance_a, position_a, ids_a, radiance_b, position_b, ids_b); geom_maps a HOST [n,2,3,4] array or None; the
        outputs must not overlap an input -> counts [5] uint32 (None without want_counts)."""
        maps, n = _interpolate_maps(geom_maps, "interpolate_device")
        p = p if p is not None else interpolate_params()
        d = [_vp(q) for q in image_ptrs]
        if len(d) != 8:
            raise ValueError("interpolate_device: image_ptrs must name eight images")
        counts = np.zeros(5, dtype=np.uint32)
        check(self._lib.ff_interpolate(self._state, width, height, C.byref(p), C.byref(cameras[0]), d[0], d[1], C.byref(cameras[1]), d[2], d[3], d[4],
                                       C.byref(cameras[2]), d[5], d[6], d[7], maps.ctypes.data if maps is not None else None, n, 1, _vp(rgb8_ptr), 1,
                                       _vp(radiance_out_ptr), 1, counts.ctypes.data if want_counts else None))
        return counts if want_counts else None

    def display(self, radiance, p=None, want_rgb8=True, want_out=True):
        """ff_display of host radiance [H,W,3] -> (rgb8 [H,W,3] uint8, display_out [H,W,3] float32: the curve's output in [0, 1]);
        the adapted exposure stays in the state."""
        rad, (h, w) = _float3_image(radiance, "display")
        p = p if p is not None else display_params()
        rgb8, out, rgb8_ptr, out_ptr = _image_outputs(h, w, want_rgb8, want_out)
        check(self._lib.ff_display(self._state, w, h, C.byref(p), rad.ctypes.data, 0, rgb8_ptr, 0, out_ptr, 0))
        return rgb8, out

    def display_device(self, width, height, radiance_ptr, p=None, rgb8_ptr=None, display_out_ptr=None):
        """ff_display on DEVICE buffers (raw pointers); display_out_ptr may equal radiance_ptr."""
        p = p if p is not None else display_params()
        check(self._lib.ff_display(self._state, width, height, C.byref(p), _vp(radiance_ptr), 1, _vp(rgb8_ptr), 1, _vp(display_out_ptr), 1))

    def display_to_pbo(self, radiance, p=None):
        """ff_display_to_pbo of host radiance [H,W,3] into the buffer registered with ff_register_gl_pbo."""
        rad = np.ascontiguousarray(radiance, dtype=np.float32)
        p = p if p is not None else display_params()
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
        w = params.width
        rgb8 = np.zeros((rows, w, 3), dtype=np.uint8) if want_rgb8 else None
        rad = np.zeros((rows, w, 3), dtype=np.float32) if want_radiance else None
        n = C.c_int(0)
        check(self._lib.ff_render_strips(self._state, C.byref(camera), C.byref(params), strip_rows, part, num_parts,
                                         rgb8.ctypes.data if want_rgb8 and rows else None, 0,
                                         rad.ctypes.data if want_radiance and rows else None, 0, C.byref(n)))
        assert n.value == rows
        return rgb8, rad

    def render_strips_device(self, camera, params, strip_rows, part, num_parts, rgb8_ptr=None, radiance_ptr=None):
        n = C.c_int(0)
        check(self._lib.ff_render_strips(self._state, C.byref(camera), C.byref(params), strip_rows, part, num_parts,
                                         C.c_void_p(rgb8_ptr) if rgb8_ptr else None, 1,
                                         C.c_void_p(radiance_ptr) if radiance_ptr else None, 1, C.byref(n)))
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
        h, w = params.height, params.width
        root = rank == 0
        rgb8 = np.zeros((h, w, 3), dtype=np.uint8) if want_rgb8 and root else None
        rad = np.zeros((h, w, 3), dtype=np.float32) if want_radiance and root else None
        check(self._lib.ff_render_distributed(self._state, C.byref(camera), C.byref(params), strip_rows,
                                              rgb8.ctypes.data if rgb8 is not None else None, 0,
                                              rad.ctypes.data if rad is not None else None, 0))
        return rgb8, rad

    def render_distributed_device(self, camera, params, strip_rows=0, rgb8_ptr=None, radiance_ptr=None):
        """The same into caller-owned device buffers on rank 0 (raw pointers; ignored on other ranks)."""
        check(self._lib.ff_render_distributed(self._state, C.byref(camera), C.byref(params), strip_rows,
                                              C.c_void_p(rgb8_ptr) if rgb8_ptr else None, 1,
                                              C.c_void_p(radiance_ptr) if radiance_ptr else None, 1))


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
        h, w = params.height, params.width
        rgb8 = np.zeros((h, w, 3), dtype=np.uint8) if want_rgb8 else None
        rad = np.zeros((h, w, 3), dtype=np.float32) if want_radiance else None
        check(self._lib.ff_multi_render(self._handle, C.byref(camera), C.byref(params), strip_rows,
                                        rgb8.ctypes.data if want_rgb8 else None, 0, rad.ctypes.data if want_radiance else None, 0))
        return rgb8, rad

    def render_device(self, camera, params, strip_rows=0, rgb8_ptr=None, radiance_ptr=None):
        check(self._lib.ff_multi_render(self._handle, C.byref(camera), C.byref(params), strip_rows,
                                        C.c_void_p(rgb8_ptr) if rgb8_ptr else None, 1, C.c_void_p(radiance_ptr) if radiance_ptr else None, 1))

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
