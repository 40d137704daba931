/*
 * firefly/ff_types.h — plain-C data model shared by the host application and the MI355X
 * path-tracing core.
 *
 * Every struct here is layout-compatible (same field order, same sizeof/offsets on x86-64 LP64)
 * with the reference's host<->device structs so that the reference's viewer code can hand its own
 * arrays to this library by pointer cast, without a glm dependency in the ABI:
 *
 *   FfTriangle   <-> struct Triangle   PathTracer/FireflyEngine/utilities.h:148-171   (96 B)
 *   FfGeometry   <-> struct Geometry   PathTracer/FireflyEngine/utilities.h:173-234   (208 B)
 *   FfBXDF       <-> struct BXDF       PathTracer/FireflyEngine/utilities.h:77-139    (60 B)
 *   FfCamera     <-> struct Camera     PathTracer/FireflyEngine/utilities.h:269-291   (108 B)
 *   FfRay        <-> struct Ray        PathTracer/FireflyEngine/utilities.h:257-267   (24 B)
 *   FfIntersect  <-> struct Intersect  PathTracer/FireflyEngine/utilities.h:57-66     (40 B)
 *   FfScene      <-> struct Scene      PathTracer/FireflyEngine/utilities.h:236-255   (16 B, dead in the reference)
 *
 * glm::vec3 == float[3], glm::vec2 == float[2], glm::mat4 == float[16] column-major
 * (m[col][row] at index col*4+row), exactly glm's default storage.
 */
#ifndef FIREFLY_FF_TYPES_H
#define FIREFLY_FF_TYPES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct FfVec2 { float x, y; } FfVec2;
typedef struct FfVec3 { float x, y, z; } FfVec3;
typedef struct FfMat4 { float m[16]; } FfMat4; /* column-major: element (col c, row r) = m[c*4+r] */

/* utilities.h:68-75 */
typedef enum FfBXDFType {
    FF_BXDF_EMITTER = 0,
    FF_BXDF_DIFFUSE = 1,
    FF_BXDF_MIRROR  = 2,
    FF_BXDF_GLASS   = 3,
    FF_BXDF_COUNT   = 4
} FfBXDFType;

/* utilities.h:141-146 */
typedef enum FfGeometryType {
    FF_GEOM_SPHERE       = 0,
    FF_GEOM_PLANE        = 1,
    FF_GEOM_TRIANGLEMESH = 2
} FfGeometryType;

/* utilities.h:77-88 (data members only; bsdf()/pdf() live in the kernel) */
typedef struct FfBXDF {
    int32_t m_type;               /* FfBXDFType; reference default COUNT */
    FfVec3  m_albedo;
    FfVec3  m_specularColor;
    float   m_refractiveIndex;
    FfVec3  m_emissiveColor;
    float   m_intensity;
    FfVec3  m_transmittanceColor;
} FfBXDF;

/* utilities.h:148-171 — only m_v0/m_v1/m_v2 are read on the hot path (kernel.cu:39-41) */
typedef struct FfTriangle {
    FfVec3 m_v0, m_v1, m_v2;
    FfVec2 m_uv0, m_uv1, m_uv2;
    FfVec3 m_n0, m_n1, m_n2;
} FfTriangle;

/* utilities.h:219-233 */
typedef struct FfGeometry {
    int32_t     m_geometryType;       /* FfGeometryType */
    FfVec3      m_position;
    FfVec3      m_rotation;           /* degrees, per axis (utilities.h:182-184) */
    FfVec3      m_scale;
    FfMat4      m_modelMatrix;        /* T * Rx * Ry * Rz * S (utilities.h:187) */
    FfMat4      m_inverseModelMatrix; /* glm::inverse(m_modelMatrix) (utilities.h:189) */
    float       m_sphereRadius;
    FfVec3      m_normal;             /* object-space plane normal, default (0,0,1) (utilities.h:229) */
    FfTriangle* m_triangles;          /* host pointer, owned by the caller */
    int32_t     m_numberOfTriangles;
    FfBXDF*     m_bxdf;               /* host pointer, owned by the caller */
} FfGeometry;

/* utilities.h:236-255 */
typedef struct FfScene {
    FfGeometry* m_geometries;
    int32_t     m_geometrySize;
} FfScene;

/* utilities.h:257-267 */
typedef struct FfRay {
    FfVec3 m_origin;
    FfVec3 m_direction;
} FfRay;

/* utilities.h:57-66 */
typedef struct FfIntersect {
    FfVec3  m_intersectionPoint;
    FfVec3  m_normal;
    float   m_t;
    uint8_t m_hit;                /* C++ bool */
    uint8_t _pad[3];
    int32_t geometryIndex;
    int32_t triangleIndex;
} FfIntersect;

/* utilities.h:269-291 (data members only) */
typedef struct FfCamera {
    FfVec3  m_position;
    FfVec3  m_up;
    FfVec3  m_right;
    FfVec3  m_forward;
    FfVec3  m_worldUp;
    float   m_yaw;
    float   m_pitch;
    float   m_screenWidth;
    float   m_screenHeight;
    float   m_fov;                /* degrees */
    float   m_nearClip;
    float   m_farClip;
    float   m_cameraMovementSpeed;
    float   m_cameraMouseSensitivity;
    uint8_t m_cameraFirstMouseInput; /* C++ bool */
    uint8_t _pad[3];
    float   m_xDelta;
    float   m_yDelta;
} FfCamera;

/* ---- build-defined parameter blocks (the reference hard-codes these in main(), kernel.cu:261-266,306-309) ---- */

/* How the closest hit is searched.  Both produce bit-identical hits; see DESIGN.md. */
typedef enum FfTraceMode {
    FF_TRACE_BRUTE_FORCE = 0, /* reference loop order kernel.cu:133-155, triangle batches staged in LDS */
    FF_TRACE_BVH         = 1  /* per-mesh object-space BVH, top levels resident in LDS */
} FfTraceMode;

typedef enum FfShadeMode {
    FF_SHADE_NORMAL_DEBUG = 0, /* kernel.cu:178-184: colour = abs(world normal); bounces/spp forced to 1 */
    FF_SHADE_DIFFUSE_PATH = 1, /* N-bounce integrator with the dormant BXDF semantics, utilities.h:90-138 */
    FF_SHADE_DIFFUSE_PATH_SMOOTH = 2, /* the same, shading triangles with the interpolated vertex normals Triangle carries
                                       * (utilities.h:163-170) through the barycentrics of kernel.cu:80-81 */
    FF_SHADE_DIFFUSE_PATH_NEE = 3 /* FF_SHADE_DIFFUSE_PATH's expectation with next-event estimation and multiple importance
                                   * sampling at diffuse vertices (lower variance); the estimator is in ff_api.h */
} FfShadeMode;

typedef enum FfGridMode {
    FF_GRID_FULL            = 0, /* every pixel of the W x H image is traced */
    FF_GRID_REFERENCE_FLOOR = 1  /* reproduce kernel.cu:308-309: only floor(W/16)*16 x floor(H/16)*16 pixels traced */
} FfGridMode;

typedef struct FfRenderParams {
    int32_t  width;       /* image width  W in pixels (row stride) */
    int32_t  height;      /* image height H in pixels */
    int32_t  bounces;     /* max path segments per sample, >= 1 (1 == the reference's primary-only behaviour) */
    int32_t  spp;         /* samples per pixel, >= 1 */
    uint64_t seed;        /* RNG seed (reference literal 1234, utilities.h:118) */
    int32_t  trace_mode;  /* FfTraceMode */
    int32_t  shade_mode;  /* FfShadeMode */
    int32_t  grid_mode;   /* FfGridMode */
    int32_t  spp_per_launch; /* 0 = all samples in one kernel launch; otherwise a frame is rendered in several launches of about
                                this many samples (rounded up to whole 64-sample blocks); the result does not depend on it */
} FfRenderParams;

/* Filled by ff_stats() after a render call. Counts are for the LAST ff_render* call on this state. */
typedef struct FfStats {
    uint64_t rays_traced;        /* closest-hit queries = path segments of the frame, counted on the device (wave-reduced counter) */
    uint64_t nodes_visited;      /* visits of 4-wide BVH nodes (112 B each); only when stats collection is on */
    uint64_t tris_tested;        /* ray/triangle tests (48 B each); only when stats collection is on */
    uint64_t planes_tested;      /* ray/plane tests */
    double   kernel_ms;          /* sum of trace-kernel durations, HIP events on the launch stream */
    double   total_ms;           /* host wall clock of the whole call */
    uint32_t kernel_launches;    /* number of trace-kernel launches in the call */
    uint32_t flags;              /* FF_STATS_* bits about how the frame was scheduled */
    uint64_t scene_bytes_nodes;  /* device bytes of BVH nodes */
    uint64_t scene_bytes_tris;   /* device bytes of triangle records */
    uint64_t rays_answered;      /* ... of rays_traced: path segments answered without a traversal - the primary segments of a frame of more than
                                    one sample per pixel (every sample of a pixel starts with the same ray, kernel.cu:200-205: a pre-pass traces
                                    it once per pixel, its rays are not counted) incl. those of pixels whose view of the scene box is empty
                                    (camera outside the scene); 0 in brute-force mode */
    uint64_t rays_cut_short;     /* ... of rays_traced: last segments of paths (bounce index bounces - 1) whose query ended after the planes and
                                    spheres because no emitter was among the candidates - only an emitter can still add radiance there and
                                    every emitter of the scene is a plane or a sphere; 0 in brute-force mode */
} FfStats;
#define FF_STATS_TAIL_ITEMS 1u             /* the frame's last sample block was handed out as fine-grained items (multi-part frames) */
#define FF_STATS_TAIL_SKIPPED_TOO_LARGE 2u /* ... was wanted, but its per-sample buffer would pass 16 GiB: rendered with whole-block items */

/* Which builder produces the BVH (ff_set_builder). */
typedef enum FfBuilder {
    FF_BUILD_HOST_SAH = 0, /* binned SAH on the host: best trees, for scenes uploaded once (the reference's case, kernel.cu:268-298) */
    FF_BUILD_GPU_LBVH = 1, /* Morton-code LBVH built on the device: for geometry that changes between frames */
    FF_BUILD_GPU_PLOC = 2  /* agglomerative clustering (PLOC) on the device: a few times the LBVH's build time, trees close to SAH quality */
} FfBuilder;

/* ff_update_mesh modes. */
typedef enum FfMeshUpdate {
    FF_UPDATE_REFIT   = 0, /* keep the tree, recompute its boxes from the moved vertices */
    FF_UPDATE_REBUILD = 1  /* rebuild the mesh's tree on the device (scene must have been uploaded with a device builder) */
} FfMeshUpdate;

/* Filled by ff_build_stats(): the last ff_upload_scene / ff_update_mesh / ff_update_transforms call. */
typedef struct FfBuildStats {
    int32_t  builder;          /* FfBuilder that produced the current trees */
    int32_t  bvh_nodes;        /* 64-byte binary nodes in use over all meshes (the builders' trees; the kernels traverse the 4-wide trees derived from them) */
    int32_t  bvh_max_depth;    /* deepest root-to-leaf path, in inner nodes */
    int32_t  last_operation;   /* 0 upload, 1 refit, 2 rebuild, 3 transforms */
    uint64_t num_triangles;
    double   total_ms;         /* host wall clock of the whole call */
    double   copy_ms;          /* of which: host-to-device copies of the caller's triangles */
    double   build_ms;         /* of which: tree construction / refit (host builder: on the CPU; device builder: kernels, synchronised) */
} FfBuildStats;

/* One entry of the light table FF_SHADE_DIFFUSE_PATH_NEE samples (ff_light_table): an emitting plane (the world image of its unit
 * quad) or one triangle of an emitting mesh, in world space.  A point of the entry is v0 + u e1 + v e2 with (u, v) in the unit square
 * (plane) or the triangle u, v >= 0, u + v <= 1. */
typedef struct FfLightEntry {
    int32_t geometry;          /* the caller's geometry index */
    int32_t primitive;         /* triangle index of a mesh, -1 for a plane */
    float   area;              /* world area */
    float   probability;       /* selection probability: area * luminance / sum over all entries */
    FfVec3  v0, e1, e2;        /* corner / first vertex and the two edges from it */
    FfVec3  normal;            /* unit normal, e1 x e2 / |e1 x e2| */
    float   alias_probability; /* Vose alias table: entry k = floor(u0 * n) is kept if u1 < alias_probability, else `alias` is taken */
    int32_t alias;
} FfLightEntry;                /* 72 bytes */

/* Filled by ff_scene_info(): what ff_upload_scene would build for a host scene (no GPU needed). */
typedef struct FfSceneInfo {
    int32_t  num_geometries;
    int32_t  num_meshes;
    int32_t  num_planes;
    int32_t  bvh_nodes;        /* 64-byte inner nodes over all meshes */
    int32_t  bvh_max_depth;    /* deepest root-to-leaf path, in inner nodes */
    int32_t  bvh_max_leaf;     /* largest leaf, in triangles */
    int32_t  lds_nodes;        /* nodes that stay resident in LDS for this scene */
    int32_t  lds_bytes;        /* LDS bytes per workgroup (nodes + traversal stacks) */
    uint64_t num_triangles;
    uint64_t device_bytes;     /* total device bytes of the compiled scene */
    int32_t  valid;            /* 1 if the structural self-check passed (every triangle in exactly one leaf, boxes enclose) */
    float    bvh_child_area;   /* summed half surface area of every child box of the binary trees (object space, padded): what the
                                  SAH build and the insertion-based optimisation pass reduce */
} FfSceneInfo;

/* ff_denoise: edge-avoiding à-trous filter guided by the G-buffer of ff_gbuffer (Dammertz et al. 2010, with albedo
 * demodulation).  ff_denoise_params_init gives the defaults; the formulas are in ff_api.h. */
#define FF_DENOISE_SAME_GEOMETRY      1 /* taps on another geometry weigh 0 */
#define FF_DENOISE_DEMODULATE_ALBEDO  2 /* filter radiance / albedo and multiply back after the last pass */
typedef struct FfDenoiseParams {
    int32_t iterations;    /* à-trous passes, step 2^i for pass i; 0 = copy through; at most 10 */
    float   sigma_color;   /* colour edge-stop, relative to the pixel's own magnitude; halved every pass (> 0) */
    float   sigma_normal;  /* normal edge-stop (> 0) */
    float   sigma_plane;   /* distance of a tap from the pixel's tangent plane, relative to the tap's distance (> 0) */
    int32_t flags;         /* FF_DENOISE_* bits */
} FfDenoiseParams;

/* ff_denoise_temporal: spatiotemporal variance-guided filtering (SVGF, Schied et al. 2017) of 1-spp frames across camera and
 * rigid object motion.  ff_temporal_params_init gives the defaults; the formulas are in ff_api.h. */
typedef struct FfTemporalParams {
    int32_t iterations;       /* variance-guided à-trous passes after the temporal step, step 2^i for pass i; 0..10 */
    float   sigma_luminance;  /* luminance edge-stop in units of the local standard deviation (SVGF sigma_l, > 0) */
    float   sigma_normal;     /* normal edge-stop, as FfDenoiseParams (> 0) */
    float   sigma_plane;      /* plane-distance edge-stop, as FfDenoiseParams (> 0) */
    int32_t flags;            /* FF_DENOISE_SAME_GEOMETRY | FF_DENOISE_DEMODULATE_ALBEDO, meaning as in ff_denoise */
    int32_t max_history;      /* >= 1: the blend factor is 1 / min(len, max_history) */
    int32_t variance_history; /* >= 1: pixels with len < this use the spatial variance estimate */
    int32_t feedback_pass;    /* which pass's output becomes the colour history: -1 = the unfiltered accumulation, else 0..iterations-1 */
    float   reuse_normal;     /* a history tap needs dot(moved normal, tap normal) >= this */
    float   reuse_plane;      /* ... and |n^ . (x_q - x^)| <= this * |x^ - previous eye| */
} FfTemporalParams;           /* 40 bytes */

/* ff_taa: temporal anti-aliasing resolve of jittered frames (Karis 2014, Salvi 2016).  ff_taa_params_init gives the defaults;
 * the formulas are in ff_api.h. */
#define FF_TAA_BILINEAR  1 /* the history is sampled with 2x2 bilinear taps instead of 4x4 Catmull-Rom */
#define FF_TAA_NO_CLAMP  2 /* the history is not clamped to the current frame's neighbourhood */
typedef struct FfTaaParams {
    float   alpha_min;  /* least weight of the current frame, in (0, 1] */
    float   gamma;      /* half-width of the clamp box in standard deviations (> 0) */
    int32_t flags;      /* FF_TAA_* bits */
    int32_t reserved;   /* 0 */
} FfTaaParams;          /* 16 bytes */

/* ff_upscale: G-buffer-guided upsampling of a low-resolution frame (joint bilateral upsampling, Kopf et al. 2007, with ff_denoise's
 * edge-stopping functions).  ff_upscale_params_init gives the defaults; the operator is in ff_api.h. */
typedef struct FfUpscaleParams {
    float    sigma_normal;  /* normal edge-stop, as FfDenoiseParams (> 0) */
    float    sigma_plane;   /* plane-distance edge-stop, as FfDenoiseParams (> 0) */
    uint32_t flags;         /* FF_DENOISE_SAME_GEOMETRY | FF_DENOISE_DEMODULATE_ALBEDO */
    float    lo_jitter[2];  /* the pixel jitter (ff_set_pixel_jitter) the low G-buffer and frame were made with, each in [0, 1) */
    float    hi_jitter[2];  /* ... and the high G-buffer's */
    uint32_t reserved;      /* 0 */
} FfUpscaleParams;          /* 32 bytes */

/* ff_taa_upscale: temporal upsampling, ff_taa writing a W x H image from jittered w x h frames.  ff_taa_upscale_params_init gives
 * the defaults; the operator is in ff_api.h. */
typedef struct FfTaaUpscaleParams {
    float   alpha_min;     /* least weight of a full-confidence sample, in (0, 1] (ff_taa's) */
    float   gamma;         /* half-width of the clamp box in standard deviations, > 0 (ff_taa's) */
    float   lo_jitter[2];  /* the pixel jitter (ff_set_pixel_jitter) the LOW frame and ids_lo were made under, each in [0, 1) */
    int32_t flags;         /* FF_TAA_BILINEAR | FF_TAA_NO_CLAMP, as in ff_taa */
    int32_t reserved;      /* 0 */
} FfTaaUpscaleParams;      /* 24 bytes */

/* ff_display: the display transform, W x H float3 radiance -> 8-bit RGB (exposure, bloom, tone curve, encoding).
 * ff_display_params_init gives the defaults; the formulas are in ff_api.h. */
#define FF_CURVE_CLAMP     0   /* y = x */
#define FF_CURVE_REINHARD  1   /* y = x (1 + x / white^2) / (1 + x) */
#define FF_CURVE_ACES      2   /* y = x (2.51 x + 0.03) / (x (2.43 x + 0.59) + 0.14)   (Narkowicz 2015) */
#define FF_ENCODE_LINEAR   0   /* byte = trunc(clamp(y) * 255): ff_render's quantisation, bit for bit */
#define FF_ENCODE_SRGB     1   /* byte = #{ b in 1..255 : T_b <= y } (ff_srgb_thresholds) */
#define FF_DISPLAY_AUTO_EXPOSURE 1
#define FF_DISPLAY_BLOOM         2
typedef struct FfDisplayParams {
    int32_t curve, encoding, flags; /* FF_CURVE_*, FF_ENCODE_*, FF_DISPLAY_* bits */
    float   exposure;          /* > 0.  Without AUTO_EXPOSURE the multiplier itself; with it, a compensation factor on the target */
    float   white;             /* > 0, REINHARD's white point */
    float   key;               /* > 0, auto: the luminance the scene's average is mapped to */
    float   low_percentile, high_percentile; /* 0 <= low < high <= 1: the share of the histogram's mass that is averaged */
    float   min_exposure, max_exposure;      /* 0 < min <= max: clamp of the automatic target (before compensation) */
    float   adapt_darken, adapt_brighten;    /* >= 0, per second: speed when the exposure has to fall / to rise */
    float   dt;                /* seconds since the previous call; <= 0: no adaptation, the target is taken at once */
    float   bloom_threshold;   /* >= 0, on exposed luminance */
    float   bloom_strength;    /* >= 0 */
    int32_t bloom_levels;      /* 1..8 */
} FfDisplayParams;             /* 64 bytes; every float must be finite */

/* ff_motion_blur: a motion-blur reconstruction filter on stored screen motion (McGuire et al., I3D 2012).
 * ff_motion_blur_params_init gives the defaults; the operator is in ff_api.h. */
typedef struct FfMotionBlurParams {
    float   shutter;       /* fraction of the frame interval the shutter is open, 0 .. 4 */
    int32_t max_radius;    /* k: longest half-spread in pixels = tile edge, 1 .. 64 */
    int32_t samples;       /* S: taps along the dominant velocity, 1 .. 64 */
    float   depth_extent;  /* world distance over which "in front" fades, > 0 */
    int32_t flags;         /* none defined yet: 0 */
    int32_t reserved;      /* 0 */
} FfMotionBlurParams;      /* 24 bytes; every float must be finite */

/* ff_depth_of_field: a gather depth-of-field filter on the G-buffer's position and depth planes.  ff_dof_params_init gives the
 * defaults, ff_dof_params_from_camera the focus and scale of a thin lens (ff_set_camera_sampling); the operator is in ff_api.h. */
typedef struct FfDofParams {
    float   focus_distance; /* distance of the plane of focus along m_forward, > 0 (and 1 / focus_distance finite) */
    float   coc_scale;      /* radius of the circle of confusion in pixels per unit of |1/focus_distance - 1/z|, >= 0 */
    int32_t max_radius;     /* k: largest radius in pixels = tile edge, 1 .. 64 */
    int32_t grid;           /* g: the taps are the points of a (2g+1)^2 grid inside the disk, 1 .. 8 */
    float   depth_extent;   /* world distance over which "in front" fades, > 0 */
    int32_t flags;          /* none defined yet: 0 */
    int32_t reserved[2];    /* 0 */
} FfDofParams;              /* 32 bytes; every float must be finite */

/* ff_despeckle: a G-buffer-guided firefly clamp on the raw frame, ahead of the denoisers.  ff_despeckle_params_init gives the
 * defaults; the operator is in ff_api.h. */
#define FF_DESPECKLE_DEMODULATE_ALBEDO 1   /* judge radiance / albedo (ff_denoise's division), not radiance */
typedef struct FfDespeckleParams {
    int32_t  radius;          /* r: the window is (2r+1)^2 pixels; 1 .. 3 */
    int32_t  rank;            /* the rank-th largest neighbour is the yardstick; 1 .. 4 */
    int32_t  min_neighbours;  /* fewer counting neighbours: the pixel is not judged; rank .. (2r+1)^2 - 1 */
    float    threshold;       /* limit = threshold * yardstick; finite, >= 1 */
    float    floor;           /* a limit below this becomes this; finite, >= 0 */
    uint32_t flags;           /* FF_DESPECKLE_DEMODULATE_ALBEDO */
    uint32_t reserved;        /* 0 */
} FfDespeckleParams;          /* 28 bytes; every float must be finite */

/* ff_sharpen: contrast-adaptive sharpening after the temporal resolve.  ff_sharpen_params_init gives the defaults; the operator is
 * in ff_api.h. */
#define FF_SHARPEN_NOISE_AWARE 1      /* a lone outlier is sharpened half as much as an edge (step 4) */
typedef struct FfSharpenParams {
    float    strength;   /* 0 .. 1; finite */
    uint32_t flags;      /* FF_SHARPEN_NOISE_AWARE */
    uint32_t reserved;   /* 0 */
} FfSharpenParams;       /* 12 bytes */

/* ff_local_tonemap: bilateral-grid local tone mapping directly before ff_display.  ff_local_tonemap_params_init gives the
 * defaults; the operator is in ff_api.h. */
typedef struct FfLocalTonemapParams {
    float    compression; /* what is left of the base layer's log-luminance range about the pivot: 0 .. 1, 1 = untouched */
    float    detail;      /* the factor on the detail layer (log-luminance minus base): 0 .. 4, 1 = untouched */
    float    pivot;       /* the luminance the compression leaves where it is; finite, in [2^-16, 2^24) */
    int32_t  cell;        /* the grid cell's edge in pixels: 8, 16, 32 or 64 */
    uint32_t flags;       /* none defined yet: 0 */
    uint32_t reserved[3]; /* 0 */
} FfLocalTonemapParams;   /* 32 bytes */

/* ff_interpolate: an in-between frame from two rendered neighbours, gathered through the in-between pose's own G-buffer.
 * ff_interpolate_params_init gives the defaults; the operator is in ff_api.h. */
typedef struct FfInterpolateParams {
    float   t;                  /* the in-between frame's place between A (0) and B (1); 0 .. 1 */
    float   surface_tolerance;  /* how far, in pixels of the source, a tap's surface point may lie from the pixel's; > 0, finite */
    int32_t fill_radius;        /* r: a hole is filled from its (2r+1)^2 window; 0 .. 8, 0 = no fill */
    int32_t flags;              /* none defined yet: 0 */
    int32_t reserved;           /* 0 */
} FfInterpolateParams;          /* 20 bytes */

/* ff_render_adaptive: render in passes until every tile's error estimate is below a threshold.  ff_adaptive_params_init gives the
 * defaults; the estimator and the driver are in ff_api.h. */
#define FF_ADAPTIVE_GUARD_NEIGHBOURS 1     /* a tile stops only when its up to 8 neighbours are below the threshold too */
typedef struct FfAdaptiveParams {
    int32_t  tile;            /* the tile edge in pixels: 16, 32, 64 or 128 */
    int32_t  min_passes;      /* no tile is judged before this many passes; even, >= 2 */
    int32_t  max_passes;      /* no tile gets more; even, min_passes .. 65534 */
    float    threshold;       /* a tile stops when its error is below this; finite or +inf (NaN is refused) */
    uint32_t flags;           /* FF_ADAPTIVE_GUARD_NEIGHBOURS */
    uint32_t reserved;        /* 0 */
} FfAdaptiveParams;           /* 24 bytes */

/* What a call of ff_render_adaptive did. */
typedef struct FfAdaptiveInfo {
    int32_t  passes_run;           /* passes the most persistent tile got: the largest n_t */
    int32_t  tiles;                /* tiles of the grid */
    int32_t  tiles_stopped_early;  /* tiles with fewer than max_passes passes */
    int32_t  rectangles;           /* rectangles rendered, over all passes */
    uint64_t samples;              /* camera samples traced: the sum over the rectangles of pixels * spp */
    float    max_tile_error;       /* the largest of the tiles' last error estimates (NaN ones aside) */
} FfAdaptiveInfo;                  /* 32 bytes (4 of padding at the end) */

/* ff_encode_yuv: display-linear float3 into the Y'CbCr 4:2:0 planes of a video encoder (NV12, P010).  ff_yuv_params_init gives the
 * defaults; the operator is in ff_api.h. */
#define FF_YUV_TRANSFER_BT709 0   /* the BT.709 OETF: SDR video */
#define FF_YUV_TRANSFER_SRGB  1   /* ff_display's sRGB curve */
#define FF_YUV_TRANSFER_PQ    2   /* SMPTE ST 2084, 10 000 nits = 1: HDR10 */
#define FF_YUV_MATRIX_BT709   0
#define FF_YUV_MATRIX_BT2020  1   /* non-constant luminance; the input's BT.709 primaries are converted first */
#define FF_YUV_RANGE_LIMITED  0   /* 16 .. 235 / 16 .. 240 (times 4 at depth 10) */
#define FF_YUV_RANGE_FULL     1   /* 0 .. 2^depth - 1 */
#define FF_YUV_SITING_CENTER  0   /* a chroma sample in the middle of its 2 x 2 luma block (JPEG, MPEG-1) */
#define FF_YUV_SITING_LEFT    1   /* co-sited with the even luma column, midway between the rows (MPEG-2, H.264, HEVC) */
typedef struct FfYuvParams {
    int32_t transfer;              /* FF_YUV_TRANSFER_* */
    int32_t matrix;                /* FF_YUV_MATRIX_* */
    int32_t range;                 /* FF_YUV_RANGE_* */
    int32_t depth;                 /* 8 (NV12) or 10 (P010) */
    int32_t siting;                /* FF_YUV_SITING_* */
    float   reference_white_nits;  /* PQ: the luminance of input 1.0; finite, within (0, 10000] */
} FfYuvParams;                     /* 24 bytes */

/* ff_resize: separable polyphase resampling of a float3 image to any size within a factor of 16.  ff_resize_params_init gives the
 * defaults; the operator is in ff_api.h. */
enum { FF_RESIZE_BOX = 0, FF_RESIZE_TRIANGLE = 1, FF_RESIZE_MITCHELL = 2, FF_RESIZE_LANCZOS3 = 3 };
#define FF_RESIZE_ANTI_RING 1u        /* an output sample is clamped to the range of the samples its taps read (step 4) */
typedef struct FfResizeParams {
    int32_t  filter;     /* FF_RESIZE_* */
    uint32_t flags;      /* FF_RESIZE_ANTI_RING */
    uint32_t reserved;   /* 0 */
} FfResizeParams;        /* 12 bytes */

/* ff_color_grade: a primary grade, per-channel curves and a 3D lattice per pixel.  ff_grade_params_init gives the defaults; the
 * operator is in ff_api.h. */
#define FF_GRADE_PRIMARY   1u         /* stage 1: matrix, offset, saturation */
#define FF_GRADE_CURVES    2u         /* stage 2: the LUT object's three curves */
#define FF_GRADE_LUT3D     4u         /* stage 3: the LUT object's lattice, read tetrahedrally ... */
#define FF_GRADE_TRILINEAR 8u         /* ... or, with this bit, trilinearly */
#define FF_GRADE_AXIS_LINEAR 0        /* knots evenly spaced over curve_lo .. curve_hi */
#define FF_GRADE_AXIS_LOG    1        /* knots evenly spaced over the float bit patterns of curve_lo .. curve_hi */
typedef struct FfGradeParams {
    uint32_t flags;      /* FF_GRADE_* stage bits and FF_GRADE_TRILINEAR */
    float    matrix[9];  /* row-major */
    float    offset[3];
    float    saturation; /* >= 0; 1 leaves the colour alone, 0 is the luminance */
    int32_t  lut_id;     /* ff_grade_lut_create's; -1: none */
    uint32_t reserved;   /* 0 */
} FfGradeParams;         /* 64 bytes */
/* What a LUT object is made from (ff_grade_lut_create) and what the host twin reads: host pointers.  Either half may be absent. */
typedef struct FfGradeLut {
    int32_t curve_size;          /* K, 2 .. 4096; 0: no curves */
    int32_t curve_axis;          /* FF_GRADE_AXIS_* */
    int32_t curve_shift;         /* FF_GRADE_AXIS_LOG: 8 .. 23; else 0 */
    float   curve_lo, curve_hi;
    int32_t size;                /* N, 2 .. 65; 0: no lattice */
    float   domain_min[3], domain_max[3];
    const float* curves;         /* 3 K floats, channel-major: r's knots, g's, b's */
    const float* table;          /* 3 N^3 floats: texel i + N (j + N k) holds the r g b of lattice point (r i, g j, b k) */
} FfGradeLut;                    /* 64 bytes */
/* A .cube file in memory (ff_load_cube / ff_save_cube): its title and the half of a LUT it holds.  ff_load_cube allocates curves
 * or table; ff_free_cube frees them. */
typedef struct FfCubeFile {
    char title[128];             /* TITLE without its quotes, NUL-terminated; "" when the file has none */
    FfGradeLut lut;              /* a 1D file: the curves on FF_GRADE_AXIS_LINEAR; a 3D file: the lattice */
} FfCubeFile;                    /* 192 bytes */

/* ff_lens: radial lens distortion, lateral chromatic aberration and vignetting as one gather.  ff_lens_params_init gives the
 * defaults (the identity); the operator is in ff_api.h. */
#define FF_LENS_KNOTS 1024            /* cells of the two radial tables: FF_LENS_KNOTS + 1 knots over r^2 = 0 .. r2_max */
enum { FF_LENS_UNDISTORT = 0, FF_LENS_DISTORT = 1 };          /* direction */
enum { FF_LENS_BILINEAR = 0, FF_LENS_CATMULL_ROM = 1 };       /* filter */
enum { FF_LENS_BORDER_BLACK = 0, FF_LENS_BORDER_CLAMP = 1 };  /* border */
enum { FF_LENS_FIT_FILL = 0, FF_LENS_FIT_ALL = 1 };           /* ff_lens_fit_zoom's mode */
#define FF_LENS_ANTI_RING 1u          /* a Catmull-Rom result is clamped to the range of its inner 2 x 2 taps */
typedef struct FfLensParams {
    float    k1, k2, k3;        /* Brown-Conrady: d(r^2) = 1 + k1 r^2 + k2 r^4 + k3 r^6; each finite, -10 .. 10 */
    float    center_x, center_y; /* the optical centre's offset from the image centre in pixels; |center_x| <= W/2, |center_y| <= H/2 */
    float    zoom;              /* a uniform magnification of the output about the optical centre; 1/16 .. 16 */
    float    ca_red, ca_blue;   /* relative magnification of red and of blue against green; -0.25 .. 0.25 */
    float    vignette;          /* the strength of the natural vignette; 0 .. 1 */
    float    vignette_falloff;  /* F of v = 1 / (1 + (F r)^2)^2; 0 .. 8 */
    int32_t  direction;         /* FF_LENS_UNDISTORT or FF_LENS_DISTORT */
    int32_t  filter;            /* FF_LENS_BILINEAR or FF_LENS_CATMULL_ROM */
    int32_t  border;            /* FF_LENS_BORDER_BLACK or FF_LENS_BORDER_CLAMP */
    uint32_t flags;             /* FF_LENS_ANTI_RING */
    uint32_t reserved;          /* 0 */
} FfLensParams;                 /* 60 bytes; every float must be finite */

/* ff_texture_create: how a texture is addressed and filtered (the formulas are in ff_api.h).  0 = repeat, bilinear. */
#define FF_TEX_REPEAT    0   /* coordinates wrap: c - floor(c) */
#define FF_TEX_CLAMP     1   /* coordinates clamp to [0, 1] */
#define FF_TEX_BILINEAR  0   /* the four nearest texels, interpolated */
#define FF_TEX_NEAREST   2   /* the texel the coordinate falls in */

/* ff_set_camera_sampling: where in its pixel, and from where on the lens, every sample's camera ray starts (ff_api.h). */
typedef enum FfPixelFilter {
    FF_PIXEL_CORNER = 0, /* every sample through the pixel's corner (plus the state's jitter): the reference's ray */
    FF_PIXEL_BOX = 1     /* a uniform point of the pixel per sample: the frame converges to the box-filtered image */
} FfPixelFilter;
typedef struct FfCameraSampling {
    int32_t pixel_filter;   /* FfPixelFilter */
    float   lens_radius;    /* world units, >= 0; 0 = pinhole */
    float   focus_distance; /* distance of the plane of focus along m_forward, > 0 when lens_radius > 0 */
    int32_t reserved;       /* 0 */
} FfCameraSampling;

#ifdef __cplusplus
} /* extern "C" */
#endif

#if defined(__cplusplus)
static_assert(sizeof(FfBXDF) == 60, "BXDF layout must match utilities.h:77-88");
static_assert(sizeof(FfTriangle) == 96, "Triangle layout must match utilities.h:148-171");
static_assert(sizeof(FfGeometry) == 208, "Geometry layout must match utilities.h:219-233");
static_assert(sizeof(FfRay) == 24, "Ray layout must match utilities.h:257-267");
static_assert(sizeof(FfIntersect) == 40, "Intersect layout must match utilities.h:57-66");
static_assert(sizeof(FfCamera) == 108, "Camera layout must match utilities.h:269-291");
static_assert(sizeof(FfDisplayParams) == 64, "FfDisplayParams is 64 bytes");
static_assert(sizeof(FfCameraSampling) == 16, "FfCameraSampling is 16 bytes");
static_assert(sizeof(FfMotionBlurParams) == 24, "FfMotionBlurParams is 24 bytes");
static_assert(sizeof(FfDofParams) == 32, "FfDofParams is 32 bytes");
static_assert(sizeof(FfDespeckleParams) == 28, "FfDespeckleParams is 28 bytes");
static_assert(sizeof(FfSharpenParams) == 12, "FfSharpenParams is 12 bytes");
static_assert(sizeof(FfLocalTonemapParams) == 32, "FfLocalTonemapParams is 32 bytes");
static_assert(sizeof(FfInterpolateParams) == 20, "FfInterpolateParams is 20 bytes");
static_assert(sizeof(FfAdaptiveParams) == 24, "FfAdaptiveParams is 24 bytes");
static_assert(sizeof(FfAdaptiveInfo) == 32, "FfAdaptiveInfo is 32 bytes");
static_assert(sizeof(FfYuvParams) == 24, "FfYuvParams is 24 bytes");
static_assert(sizeof(FfResizeParams) == 12, "FfResizeParams is 12 bytes");
static_assert(sizeof(FfGradeParams) == 64, "FfGradeParams is 64 bytes");
static_assert(sizeof(FfGradeLut) == 64, "FfGradeLut is 64 bytes");
static_assert(sizeof(FfCubeFile) == 192, "FfCubeFile is 192 bytes");
static_assert(sizeof(FfLensParams) == 60, "FfLensParams is 60 bytes");
#else
_Static_assert(sizeof(FfBXDF) == 60, "BXDF layout");
_Static_assert(sizeof(FfTriangle) == 96, "Triangle layout");
_Static_assert(sizeof(FfGeometry) == 208, "Geometry layout");
_Static_assert(sizeof(FfRay) == 24, "Ray layout");
_Static_assert(sizeof(FfIntersect) == 40, "Intersect layout");
_Static_assert(sizeof(FfCamera) == 108, "Camera layout");
_Static_assert(sizeof(FfDisplayParams) == 64, "FfDisplayParams layout");
_Static_assert(sizeof(FfCameraSampling) == 16, "FfCameraSampling layout");
_Static_assert(sizeof(FfMotionBlurParams) == 24, "FfMotionBlurParams layout");
_Static_assert(sizeof(FfDofParams) == 32, "FfDofParams layout");
_Static_assert(sizeof(FfDespeckleParams) == 28, "FfDespeckleParams layout");
_Static_assert(sizeof(FfSharpenParams) == 12, "FfSharpenParams layout");
_Static_assert(sizeof(FfLocalTonemapParams) == 32, "FfLocalTonemapParams layout");
_Static_assert(sizeof(FfInterpolateParams) == 20, "FfInterpolateParams layout");
_Static_assert(sizeof(FfAdaptiveParams) == 24, "FfAdaptiveParams layout");
_Static_assert(sizeof(FfAdaptiveInfo) == 32, "FfAdaptiveInfo layout");
_Static_assert(sizeof(FfYuvParams) == 24, "FfYuvParams layout");
_Static_assert(sizeof(FfResizeParams) == 12, "FfResizeParams layout");
_Static_assert(sizeof(FfGradeParams) == 64, "FfGradeParams layout");
_Static_assert(sizeof(FfGradeLut) == 64, "FfGradeLut layout");
_Static_assert(sizeof(FfCubeFile) == 192, "FfCubeFile layout");
_Static_assert(sizeof(FfLensParams) == 60, "FfLensParams layout");
#endif

#endif /* FIREFLY_FF_TYPES_H */
