"""ctypes mirrors of include/firefly/ff_types.h (layout-compatible with the reference's structs,
PathTracer/FireflyEngine/utilities.h:57-66,77-88,148-171,219-233,257-267,269-291)."""
import ctypes as C

import numpy as np


class FfVec2(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float)]


class FfVec3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]

    def __init__(self, x=0.0, y=0.0, z=0.0):
        super().__init__(float(x), float(y), float(z))

    def tuple(self):
        return (self.x, self.y, self.z)


class FfMat4(C.Structure):
    _fields_ = [("m", C.c_float * 16)]

    def numpy(self):
        """4x4 array indexed [col][row] (glm storage order)."""
        return np.frombuffer(bytes(self), dtype=np.float32).reshape(4, 4).copy()


class FfBXDF(C.Structure):
    _fields_ = [
        ("m_type", C.c_int32),
        ("m_albedo", FfVec3),
        ("m_specularColor", FfVec3),
        ("m_refractiveIndex", C.c_float),
        ("m_emissiveColor", FfVec3),
        ("m_intensity", C.c_float),
        ("m_transmittanceColor", FfVec3),
    ]


class FfTriangle(C.Structure):
    _fields_ = [
        ("m_v0", FfVec3), ("m_v1", FfVec3), ("m_v2", FfVec3),
        ("m_uv0", FfVec2), ("m_uv1", FfVec2), ("m_uv2", FfVec2),
        ("m_n0", FfVec3), ("m_n1", FfVec3), ("m_n2", FfVec3),
    ]


class FfGeometry(C.Structure):
    _fields_ = [
        ("m_geometryType", C.c_int32),
        ("m_position", FfVec3),
        ("m_rotation", FfVec3),
        ("m_scale", FfVec3),
        ("m_modelMatrix", FfMat4),
        ("m_inverseModelMatrix", FfMat4),
        ("m_sphereRadius", C.c_float),
        ("m_normal", FfVec3),
        ("m_triangles", C.POINTER(FfTriangle)),
        ("m_numberOfTriangles", C.c_int32),
        ("m_bxdf", C.POINTER(FfBXDF)),
    ]


class FfRay(C.Structure):
    _fields_ = [("m_origin", FfVec3), ("m_direction", FfVec3)]


class FfIntersect(C.Structure):
    _fields_ = [
        ("m_intersectionPoint", FfVec3),
        ("m_normal", FfVec3),
        ("m_t", C.c_float),
        ("m_hit", C.c_uint8),
        ("_pad", C.c_uint8 * 3),
        ("geometryIndex", C.c_int32),
        ("triangleIndex", C.c_int32),
    ]


class FfCamera(C.Structure):
    _fields_ = [
        ("m_position", FfVec3), ("m_up", FfVec3), ("m_right", FfVec3), ("m_forward", FfVec3), ("m_worldUp", FfVec3),
        ("m_yaw", C.c_float), ("m_pitch", C.c_float),
        ("m_screenWidth", C.c_float), ("m_screenHeight", C.c_float),
        ("m_fov", C.c_float), ("m_nearClip", C.c_float), ("m_farClip", C.c_float),
        ("m_cameraMovementSpeed", C.c_float), ("m_cameraMouseSensitivity", C.c_float),
        ("m_cameraFirstMouseInput", C.c_uint8), ("_pad", C.c_uint8 * 3),
        ("m_xDelta", C.c_float), ("m_yDelta", C.c_float),
    ]


class FfRenderParams(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32), ("bounces", C.c_int32), ("spp", C.c_int32),
        ("seed", C.c_uint64),
        ("trace_mode", C.c_int32), ("shade_mode", C.c_int32), ("grid_mode", C.c_int32), ("spp_per_launch", C.c_int32),
    ]


FF_STATS_TAIL_ITEMS = 1
FF_STATS_TAIL_SKIPPED_TOO_LARGE = 2


class FfStats(C.Structure):
    _fields_ = [
        ("rays_traced", C.c_uint64), ("nodes_visited", C.c_uint64), ("tris_tested", C.c_uint64), ("planes_tested", C.c_uint64),
        ("kernel_ms", C.c_double), ("total_ms", C.c_double),
        ("kernel_launches", C.c_uint32), ("flags", C.c_uint32),
        ("scene_bytes_nodes", C.c_uint64), ("scene_bytes_tris", C.c_uint64), ("rays_answered", C.c_uint64), ("rays_cut_short", C.c_uint64),
    ]


class FfBuildStats(C.Structure):
    _fields_ = [
        ("builder", C.c_int32), ("bvh_nodes", C.c_int32), ("bvh_max_depth", C.c_int32), ("last_operation", C.c_int32),
        ("num_triangles", C.c_uint64), ("total_ms", C.c_double), ("copy_ms", C.c_double), ("build_ms", C.c_double),
    ]


class FfDenoiseParams(C.Structure):
    _fields_ = [
        ("iterations", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float), ("sigma_plane", C.c_float), ("flags", C.c_int32),
    ]


DENOISE_SAME_GEOMETRY, DENOISE_DEMODULATE_ALBEDO = 1, 2


class FfTemporalParams(C.Structure):
    _fields_ = [
        ("iterations", C.c_int32), ("sigma_luminance", C.c_float), ("sigma_normal", C.c_float), ("sigma_plane", C.c_float), ("flags", C.c_int32),
        ("max_history", C.c_int32), ("variance_history", C.c_int32), ("feedback_pass", C.c_int32), ("reuse_normal", C.c_float),
        ("reuse_plane", C.c_float),
    ]


TEMPORAL_PARAMS_BYTES = 40


class FfTaaParams(C.Structure):
    _fields_ = [("alpha_min", C.c_float), ("gamma", C.c_float), ("flags", C.c_int32), ("reserved", C.c_int32)]


TAA_PARAMS_BYTES = 16
TAA_BILINEAR, TAA_NO_CLAMP = 1, 2


class FfUpscaleParams(C.Structure):
    _fields_ = [("sigma_normal", C.c_float), ("sigma_plane", C.c_float), ("flags", C.c_uint32), ("lo_jitter", C.c_float * 2),
                ("hi_jitter", C.c_float * 2), ("reserved", C.c_uint32)]


UPSCALE_PARAMS_BYTES = 32


class FfTaaUpscaleParams(C.Structure):
    _fields_ = [("alpha_min", C.c_float), ("gamma", C.c_float), ("lo_jitter", C.c_float * 2), ("flags", C.c_int32), ("reserved", C.c_int32)]


TAA_UPSCALE_PARAMS_BYTES = 24


class FfDisplayParams(C.Structure):
    _fields_ = [
        ("curve", C.c_int32), ("encoding", C.c_int32), ("flags", C.c_int32), ("exposure", C.c_float), ("white", C.c_float), ("key", C.c_float),
        ("low_percentile", C.c_float), ("high_percentile", C.c_float), ("min_exposure", C.c_float), ("max_exposure", C.c_float),
        ("adapt_darken", C.c_float), ("adapt_brighten", C.c_float), ("dt", C.c_float), ("bloom_threshold", C.c_float),
        ("bloom_strength", C.c_float), ("bloom_levels", C.c_int32),
    ]


DISPLAY_PARAMS_BYTES = 64
CURVE_CLAMP, CURVE_REINHARD, CURVE_ACES = 0, 1, 2
ENCODE_LINEAR, ENCODE_SRGB = 0, 1
DISPLAY_AUTO_EXPOSURE, DISPLAY_BLOOM = 1, 2
DISPLAY_BINS = 256  # ff_display's luminance histogram: 8 bins per stop from 2^-16 up


class FfMotionBlurParams(C.Structure):
    _fields_ = [("shutter", C.c_float), ("max_radius", C.c_int32), ("samples", C.c_int32), ("depth_extent", C.c_float), ("flags", C.c_int32),
                ("reserved", C.c_int32)]


MOTION_BLUR_PARAMS_BYTES = 24


class FfDofParams(C.Structure):
    _fields_ = [("focus_distance", C.c_float), ("coc_scale", C.c_float), ("max_radius", C.c_int32), ("grid", C.c_int32), ("depth_extent", C.c_float),
                ("flags", C.c_int32), ("reserved", C.c_int32 * 2)]


DOF_PARAMS_BYTES = 32


class FfDespeckleParams(C.Structure):
    _fields_ = [("radius", C.c_int32), ("rank", C.c_int32), ("min_neighbours", C.c_int32), ("threshold", C.c_float), ("floor", C.c_float),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


DESPECKLE_PARAMS_BYTES = 28
DESPECKLE_DEMODULATE_ALBEDO = 1


class FfSharpenParams(C.Structure):
    _fields_ = [("strength", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


SHARPEN_PARAMS_BYTES = 12
SHARPEN_NOISE_AWARE = 1


class FfLocalTonemapParams(C.Structure):
    _fields_ = [("compression", C.c_float), ("detail", C.c_float), ("pivot", C.c_float), ("cell", C.c_int32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]


LOCAL_TONEMAP_PARAMS_BYTES = 32
LOCAL_TONEMAP_CELLS = (8, 16, 32, 64)
LOCAL_TONEMAP_BINS = 40
assert C.sizeof(FfLocalTonemapParams) == LOCAL_TONEMAP_PARAMS_BYTES


class FfInterpolateParams(C.Structure):
    _fields_ = [("t", C.c_float), ("surface_tolerance", C.c_float), ("fill_radius", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


INTERPOLATE_PARAMS_BYTES = 20
INTERPOLATE_MAX_FILL_RADIUS = 8
INTERPOLATE_COUNTS = ("both", "a_only", "b_only", "filled", "fallback")


class FfAdaptiveParams(C.Structure):
    _fields_ = [("tile", C.c_int32), ("min_passes", C.c_int32), ("max_passes", C.c_int32), ("threshold", C.c_float), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


class FfAdaptiveInfo(C.Structure):
    _fields_ = [("passes_run", C.c_int32), ("tiles", C.c_int32), ("tiles_stopped_early", C.c_int32), ("rectangles", C.c_int32),
                ("samples", C.c_uint64), ("max_tile_error", C.c_float)]


ADAPTIVE_PARAMS_BYTES, ADAPTIVE_INFO_BYTES = 24, 32
ADAPTIVE_GUARD_NEIGHBOURS = 1
ADAPTIVE_TILES = (16, 32, 64, 128)
ADAPTIVE_MAX_PASSES = 65534
assert C.sizeof(FfAdaptiveParams) == ADAPTIVE_PARAMS_BYTES and C.sizeof(FfAdaptiveInfo) == ADAPTIVE_INFO_BYTES


class FfYuvParams(C.Structure):
    _fields_ = [("transfer", C.c_int32), ("matrix", C.c_int32), ("range", C.c_int32), ("depth", C.c_int32), ("siting", C.c_int32),
                ("reference_white_nits", C.c_float)]


YUV_PARAMS_BYTES = 24
YUV_TRANSFER_BT709, YUV_TRANSFER_SRGB, YUV_TRANSFER_PQ = 0, 1, 2
YUV_MATRIX_BT709, YUV_MATRIX_BT2020 = 0, 1
YUV_RANGE_LIMITED, YUV_RANGE_FULL = 0, 1
YUV_SITING_CENTER, YUV_SITING_LEFT = 0, 1
YUV_KNOTS = 4097
assert C.sizeof(FfYuvParams) == YUV_PARAMS_BYTES


class FfResizeParams(C.Structure):
    _fields_ = [("filter", C.c_int32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


RESIZE_PARAMS_BYTES = 12
RESIZE_BOX, RESIZE_TRIANGLE, RESIZE_MITCHELL, RESIZE_LANCZOS3 = 0, 1, 2, 3
RESIZE_ANTI_RING = 1
RESIZE_MAX_RATIO, RESIZE_MAX_TAPS = 16, 96
assert C.sizeof(FfResizeParams) == RESIZE_PARAMS_BYTES


class FfGradeParams(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("matrix", C.c_float * 9), ("offset", C.c_float * 3), ("saturation", C.c_float), ("lut_id", C.c_int32),
                ("reserved", C.c_uint32)]


class FfGradeLut(C.Structure):
    _fields_ = [("curve_size", C.c_int32), ("curve_axis", C.c_int32), ("curve_shift", C.c_int32), ("curve_lo", C.c_float), ("curve_hi", C.c_float),
                ("size", C.c_int32), ("domain_min", C.c_float * 3), ("domain_max", C.c_float * 3), ("curves", C.c_void_p), ("table", C.c_void_p)]


class FfCubeFile(C.Structure):
    _fields_ = [("title", C.c_char * 128), ("lut", FfGradeLut)]


GRADE_PARAMS_BYTES, GRADE_LUT_BYTES, CUBE_FILE_BYTES = 64, 64, 192
GRADE_PRIMARY, GRADE_CURVES, GRADE_LUT3D, GRADE_TRILINEAR = 1, 2, 4, 8
GRADE_AXIS_LINEAR, GRADE_AXIS_LOG = 0, 1
GRADE_MAX_LUTS, GRADE_MAX_CURVE, GRADE_MAX_SIZE = 16, 4096, 65
# the kernels' launch (csrc/ff_grade.h): the largest lattice kept in LDS and the LDS bytes a workgroup may take; a fixed grid of at
# most GRADE_MAX_BLOCKS workgroups of GRADE_THREADS lanes, a lane on GRADE_PIXELS_PER_LANE consecutive pixels per pass
GRADE_LDS_MAX_SIZE, GRADE_LDS_BYTES = 17, 65536
GRADE_THREADS, GRADE_PIXELS_PER_LANE, GRADE_MAX_BLOCKS = 256, 4, 512
assert (C.sizeof(FfGradeParams), C.sizeof(FfGradeLut), C.sizeof(FfCubeFile)) == (GRADE_PARAMS_BYTES, GRADE_LUT_BYTES, CUBE_FILE_BYTES)


class FfLensParams(C.Structure):
    _fields_ = [("k1", C.c_float), ("k2", C.c_float), ("k3", C.c_float), ("center_x", C.c_float), ("center_y", C.c_float), ("zoom", C.c_float),
                ("ca_red", C.c_float), ("ca_blue", C.c_float), ("vignette", C.c_float), ("vignette_falloff", C.c_float),
                ("direction", C.c_int32), ("filter", C.c_int32), ("border", C.c_int32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


LENS_PARAMS_BYTES = 60
LENS_KNOTS = 1024
LENS_UNDISTORT, LENS_DISTORT = 0, 1
LENS_BILINEAR, LENS_CATMULL_ROM = 0, 1
LENS_BORDER_BLACK, LENS_BORDER_CLAMP = 0, 1
LENS_FIT_FILL, LENS_FIT_ALL = 0, 1
LENS_ANTI_RING = 1
assert C.sizeof(FfLensParams) == LENS_PARAMS_BYTES

BUILD_HOST_SAH, BUILD_GPU_LBVH, BUILD_GPU_PLOC = 0, 1, 2
UPDATE_REFIT, UPDATE_REBUILD = 0, 1

# device records as ff_debug_download_bvh returns them (gpupathtracer_amd/csrc/ff_internal.h)
import numpy as _np
BVH_NODE_DTYPE = _np.dtype([("lmin", _np.float32, 3), ("left", _np.int32), ("lmax", _np.float32, 3), ("right", _np.int32),
                            ("rmin", _np.float32, 3), ("pad0", _np.int32), ("rmax", _np.float32, 3), ("pad1", _np.int32)])
TRI_RECORD_DTYPE = _np.dtype([("v0", _np.float32, 3), ("orig_index", _np.int32), ("e1", _np.float32, 3), ("cull_margin", _np.float32),
                              ("e2", _np.float32, 3), ("pad1", _np.int32)])
assert BVH_NODE_DTYPE.itemsize == 64 and TRI_RECORD_DTYPE.itemsize == 48
# 4-wide traversal node (csrc/ff_internal.h Bvh4Node): box planes [axis][slot] and links (>= 0: node relative to the mesh's root, < 0: leaf)
BVH4_NODE_DTYPE = _np.dtype([("mn", _np.float32, (3, 4)), ("mx", _np.float32, (3, 4)), ("link", _np.int32, 4)])
assert BVH4_NODE_DTYPE.itemsize == 112
BVH4_EMPTY_LINK = 0x7fffffff


class FfSceneInfo(C.Structure):
    _fields_ = [
        ("num_geometries", C.c_int32), ("num_meshes", C.c_int32), ("num_planes", C.c_int32),
        ("bvh_nodes", C.c_int32), ("bvh_max_depth", C.c_int32), ("bvh_max_leaf", C.c_int32),
        ("lds_nodes", C.c_int32), ("lds_bytes", C.c_int32),
        ("num_triangles", C.c_uint64), ("device_bytes", C.c_uint64),
        ("valid", C.c_int32), ("bvh_child_area", C.c_float),
    ]


class FfLightEntry(C.Structure):
    _fields_ = [
        ("geometry", C.c_int32), ("primitive", C.c_int32), ("area", C.c_float), ("probability", C.c_float),
        ("v0", FfVec3), ("e1", FfVec3), ("e2", FfVec3), ("normal", FfVec3),
        ("alias_probability", C.c_float), ("alias", C.c_int32),
    ]


class FfCameraSampling(C.Structure):
    """ff_set_camera_sampling: the pixel filter and the thin lens of the per-sample camera rays (ff_types.h)."""
    _fields_ = [("pixel_filter", C.c_int32), ("lens_radius", C.c_float), ("focus_distance", C.c_float), ("reserved", C.c_int32)]


assert C.sizeof(FfCameraSampling) == 16
assert C.sizeof(FfLightEntry) == 72
assert C.sizeof(FfBXDF) == 60
assert C.sizeof(FfTriangle) == 96
assert C.sizeof(FfGeometry) == 208
assert C.sizeof(FfRay) == 24
assert C.sizeof(FfIntersect) == 40
assert C.sizeof(FfCamera) == 108

# enums (ff_types.h)
BXDF_EMITTER, BXDF_DIFFUSE, BXDF_MIRROR, BXDF_GLASS, BXDF_COUNT = range(5)
GEOM_SPHERE, GEOM_PLANE, GEOM_TRIANGLEMESH = range(3)
TRACE_BRUTE_FORCE, TRACE_BVH = 0, 1
SHADE_NORMAL_DEBUG, SHADE_DIFFUSE_PATH, SHADE_DIFFUSE_PATH_SMOOTH, SHADE_DIFFUSE_PATH_NEE = 0, 1, 2, 3
GRID_FULL, GRID_REFERENCE_FLOOR = 0, 1
ENV_MAX_TEXELS = 1 << 26  # largest environment map ff_set_environment takes (width x height)
TEX_REPEAT, TEX_CLAMP, TEX_BILINEAR, TEX_NEAREST = 0, 1, 0, 2  # ff_texture_create flags (FF_TEX_*)
TEX_MAX_TEXELS = 1 << 26  # largest texture ff_texture_create takes (width x height)
SCENE_TEX_SRGB = 256  # ff_scene_file_texture: the statement says `srgb`
PIXEL_CORNER, PIXEL_BOX = 0, 1  # FfCameraSampling.pixel_filter (FF_PIXEL_*)
GLOSSY_MIN_ALPHA = 1.0e-3  # ff_set_roughness: a binding whose alpha = roughness^2 is below it shades as the perfect mirror

# status codes (ff_api.h)
FF_OK, FF_ERR_INVALID_ARG, FF_ERR_NO_DEVICE, FF_ERR_HIP, FF_ERR_NO_SCENE, FF_ERR_UNSUPPORTED, FF_ERR_GL_UNAVAILABLE, FF_ERR_IO, FF_ERR_OOM, FF_ERR_COMM = range(10)

TRIANGLE_DTYPE = np.dtype((np.float32, (24,)))


def triangles_from_array(arr):
    """float32 [n, 24] (FfTriangle field order) -> ctypes array of FfTriangle sharing a private copy."""
    a = np.ascontiguousarray(arr, dtype=np.float32).reshape(-1, 24)
    buf = (FfTriangle * a.shape[0])()
    C.memmove(buf, a.ctypes.data, a.nbytes)
    return buf


def triangles_to_array(ptr, count):
    out = np.empty((count, 24), dtype=np.float32)
    C.memmove(out.ctypes.data, ptr, out.nbytes)
    return out
