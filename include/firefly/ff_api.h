/*
 * firefly/ff_api.h — C ABI of the MI355X path-tracing core (libfirefly_hip.so).
 *
 * The reference has no library seam: host and device code share one translation unit
 * (PathTracer/FireflyEngine/kernel.cu).  This ABI is cut exactly at the two places where the
 * reference's main() talks to the GPU:
 *
 *   scene upload   kernel.cu:268-298   -> ff_upload_scene
 *   per-frame      kernel.cu:335-344   -> ff_render_to_pbo (GL viewer) / ff_render (headless twin)
 *   PBO register   utilities.h:605-618 -> ff_register_gl_pbo,  utilities.h:516 -> ff_unregister_gl_pbo
 *   kernel         kernel.cu:218-221   -> the trace kernels behind ff_render*
 *
 * Conventions: plain pointers and sizes only; every function returns an FfStatus (0 = ok) and never
 * calls exit() (the reference's cudaCheckErrors macro does, utilities.h:27-37); the message for the
 * last failure on the calling thread is available from ff_last_error().  All ff_render* calls are
 * synchronous on return, which is the implicit contract the viewer relies on before glTexSubImage2D
 * (kernel.cu:344-351).  The caller owns the host scene and all GL objects; the library owns all
 * device memory it allocates.
 */
#ifndef FIREFLY_FF_API_H
#define FIREFLY_FF_API_H

#include "ff_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#if defined(_WIN32)
#define FF_API __declspec(dllexport)
#else
#define FF_API __attribute__((visibility("default")))
#endif

typedef enum FfStatus {
    FF_OK                 = 0,
    FF_ERR_INVALID_ARG    = 1,
    FF_ERR_NO_DEVICE      = 2,  /* no HIP device / HIP runtime failure at create */
    FF_ERR_HIP            = 3,  /* a HIP call failed; see ff_last_error() */
    FF_ERR_NO_SCENE       = 4,  /* render called before ff_upload_scene */
    FF_ERR_UNSUPPORTED    = 5,  /* e.g. a non-affine model matrix, an unknown geometry type (kernel.cu:170-173) */
    FF_ERR_GL_UNAVAILABLE = 6,  /* HIP-GL interop not usable (headless box) */
    FF_ERR_IO             = 7,  /* file could not be read / parsed */
    FF_ERR_OOM            = 8,
    FF_ERR_COMM           = 9   /* RCCL unavailable or a collective call failed (multi-GPU entry points) */
} FfStatus;

typedef struct FfState FfState; /* opaque; replaces PathTracerState (kernel.h:12-20) */

/* ---- lifetime --------------------------------------------------------------------------------- */

/* Create a tracer bound to HIP device `device_id`. */
FF_API int ff_create(FfState** out_state, int device_id);
FF_API int ff_destroy(FfState* state);

/* Message of the last failure on this thread ("" if none). Never NULL. */
FF_API const char* ff_last_error(void);

/* Library/ABI version: major*10000 + minor*100 + patch. */
FF_API int ff_version(void);

/* Launch stream for all subsequent work of this state (a hipStream_t; NULL = default stream,
 * which is what the reference uses, kernel.cu:342). */
FF_API int ff_set_stream(FfState* state, void* hip_stream);

/* ---- host-side helpers restating the reference's host code (bit-exact glm operation order) ---- */

/* Geometry::Geometry(type, position, rotation, scale, triangles, radius)  utilities.h:176-213.
 * Builds m_modelMatrix = T*Rx*Ry*Rz*S and its inverse.  `triangles` is borrowed, not copied. */
FF_API void ff_geometry_init(FfGeometry* g, int geometry_type, FfVec3 position, FfVec3 rotation_deg,
                             FfVec3 scale, FfTriangle* triangles, int number_of_triangles, float radius);

/* BXDF default member initialisers utilities.h:81-88. */
FF_API void ff_bxdf_init(FfBXDF* b);

/* Camera default member initialisers utilities.h:287-291 plus the literals of kernel.cu:312-322
 * (position (0,0,15), worldUp (0,1,0), fov 70, near .1, far 1000, yaw -90, pitch 0) for a W x H image,
 * followed by UpdateBasisAxis. Width/height are assigned un-swapped (see SURVEY hazard 2). */
FF_API void ff_camera_init_default(FfCamera* c, int width, int height);

/* Camera::UpdateBasisAxis  utilities.h:407-418. */
FF_API void ff_camera_update_basis(FfCamera* c);

/* invView * invProj of kernel.cu:203 (lookAtRH, perspectiveFovRH_NO, two inverses, one mat*mat),
 * hoisted out of the per-pixel path.  Exposed for tests. */
FF_API void ff_camera_ray_matrix(const FfCamera* c, FfMat4* out_inv_view_times_inv_proj);

/* ff_camera_ray_matrix with a sub-pixel jitter (jx, jy) composed in: the primary ray of pixel (x, y) goes through (x + jx, y + jy)
 * instead of the pixel corner.  The kernel forms v = (Px f, Py f, f, f) (f = m_farClip) and multiplies it by the matrix, so adding
 * (dPx f, dPy f, 0, 0) to v is the same as replacing column 2: c2' = c2 + dPx c0 + dPy c1, dPx = 2 jx / m_screenWidth,
 * dPy = -2 jy / m_screenHeight, composed in double and rounded to float.  Columns 0, 1 and 3 are ff_camera_ray_matrix's;
 * jx = jy = 0 gives ff_camera_ray_matrix's matrix bit for bit. */
FF_API void ff_camera_ray_matrix_jittered(const FfCamera* c, float jx, float jy, FfMat4* out);

/* Sub-pixel jitter of the state's primary rays: the following ff_render* and ff_gbuffer calls trace pixel (x, y) through
 * (x + jx, y + jy), i.e. Px = (x + jx) / screen_w * 2 - 1, Py = 1 - (y + jy) / screen_h * 2 (ff_camera_ray_matrix_jittered).
 * jx, jy finite and in [0, 1); the default 0 0 is the reference's ray bit for bit.  Every sample of one call shares the jitter
 * (the stored primary hits are keyed by the jittered matrix, so a new jitter re-traces them).  ff_denoise_temporal does not
 * see the jitter: it reprojects in unjittered pixel coordinates, and ff_taa cancels the jitter through the G-buffer. */
FF_API int ff_set_pixel_jitter(FfState* state, float jx, float jy);

/* Halton(2), Halton(3) of (index mod period) + 1 (the modulus taken into 0..period-1): (1/2, 1/3), (1/4, 2/3), (3/4, 1/9), ...
 * period >= 1.  A viewer at rest that cycles through `period` jitters converges to the pixel's box-filtered image. */
FF_API int ff_jitter_sequence(int index, int period, float* jx, float* jy);

/* ---- scene upload (kernel.cu:268-298) ---------------------------------------------------------- */

/* Deep-copies `n` geometries (and the triangles / BXDFs they point to) to the device, flattened to
 * 48-byte triangle records, per-geometry transform records and one object-space BVH per mesh.
 * The host arrays are only read and may be freed after the call.  A second call replaces the scene
 * and frees the previous one (the reference leaks it, kernel.cu:364-368).
 * SPHERE geometries (declared by the reference, utilities.h:193-195, but only printf'ed by its kernel, kernel.cu:166-169)
 * are intersected analytically in object space: radius m_sphereRadius about the origin, two-sided. */
FF_API int ff_upload_scene(FfState* state, const FfGeometry* host_geometries, int n);

/* ---- dynamic scenes (no counterpart in the reference, whose upload is one-off) ------- */

/* Selects the BVH builder used by the following ff_upload_scene calls (default FF_BUILD_HOST_SAH).  Rendered results do
 * not depend on the builder: every hit is decided by the reference arithmetic, the tree only prunes. */
FF_API int ff_set_builder(FfState* state, int builder);

/* The same geometries as the last upload (same count, types and triangle counts) with new transforms / materials:
 * rewrites the per-geometry records only.  Trees live in object space, so moving, rotating or scaling a mesh costs no
 * rebuild. */
FF_API int ff_update_transforms(FfState* state, const FfGeometry* host_geometries, int n);

/* New vertex positions for mesh `geometry_index` (index in the uploaded Geometry array; `count` must equal the uploaded
 * triangle count).  FF_UPDATE_REFIT keeps the tree and recomputes its boxes on the device; FF_UPDATE_REBUILD builds a
 * new tree on the device in the mesh's slot. */
FF_API int ff_update_mesh(FfState* state, int geometry_index, const FfTriangle* triangles, int count, int mode);

FF_API int ff_build_stats(FfState* state, FfBuildStats* out_stats);

/* Copies the compiled scene back for inspection (tests): up to `max_nodes` 64-byte binary nodes and `max_tris` 48-byte triangle
 * records; the counts in use are returned through out_nodes / out_tris.  mesh_table (optional) receives, for each of the
 * first `max_geometries` uploaded geometries in the caller's order, {bvh_root, node_count, tri_first, tri_count, depth}
 * (bvh_root = -1 for planes and empty meshes).  Buffers may be null to query the counts. */
FF_API int ff_debug_download_bvh(FfState* state, void* nodes, int max_nodes, int* out_nodes, void* tris, int max_tris, int* out_tris,
                                 int* mesh_table, int max_geometries);

/* The 4-wide trees the trace kernels traverse (derived on the device from the binary trees above): up to `max_nodes`
 * 112-byte nodes of the whole array (*out_capacity = its length; mesh i's nodes start at its binary root's index and link
 * to each other relative to it); mesh_table (optional) receives per uploaded geometry {first node, node count, depth,
 * first LDS slot, nodes cached in LDS, LDS node slots of the scene}. */
FF_API int ff_debug_download_bvh4(FfState* state, void* nodes4, int max_nodes, int* out_capacity, int* mesh_table, int max_geometries);

/* Host-only dry run of the scene compiler: sizes, BVH shape and a structural self-check.  Needs no GPU. */
FF_API int ff_scene_info(const FfGeometry* host_geometries, int n, FfSceneInfo* out_info);

/* Host-only: the planes the trace kernels screen in WORLD space - those whose model matrix maps the unit quad (kernel.cu:18) onto a
 * rectangle parallel to two world axes (rotations by multiples of 90 degrees, any translation, scales within 1 : 16): every wall
 * of a box scene.  Per wall 7 floats {caller's geometry index, normal axis 0/1/2, plane coordinate, centre and half extent along
 * the next axis, centre and half extent along the one after}; walls sorted by axis.  Returns the number of walls (at most 16 of a
 * scene's first 32 planes) or minus an FfStatus.  Results never depend on the table: a plane it leaves out, and every hit inside
 * its margins, goes through the exact reference test.  Needs no GPU. */
FF_API int ff_debug_wall_table(const FfGeometry* host_geometries, int n, float* out_walls7, int max_walls);
/* ... and the number of ENTRIES of that table: two walls normal to the same axis with the same rectangle (floor and ceiling of a box)
 * share one, so this is at most the count above.  Needs no GPU. */
FF_API int ff_debug_wall_entries(const FfGeometry* host_geometries, int n);

/* ---- rendering (kernel.cu:335-344 + launchPathTrace kernel.cu:218-221) -------------------------- */

/* Headless twin of the per-frame block.  Outputs (either may be NULL):
 *   rgb8      W*H*3 bytes, row-major, top row first, exactly the PBO contents the viewer uploads
 *             (kernel.cu:214; miss pixels stay 0 like the cudaMemset at kernel.cu:340)
 *   radiance  W*H*3 floats, mean radiance per pixel before 8-bit quantisation
 * `*_on_device` != 0 means the pointer is device memory of this state's device; otherwise it is host
 * memory and the library copies back (PCIe-inclusive). */
FF_API int ff_render(FfState* state, const FfCamera* camera, const FfRenderParams* params,
                     void* rgb8, int rgb8_on_device, float* radiance, int radiance_on_device);

/* Multi-GPU slice of the same frame: the image is cut into strips of `strip_rows` rows; this call
 * renders the strips s with s % num_parts == part and writes them compacted, in increasing s, into
 * rgb8/radiance (device or host as above), each local row W pixels wide.  part=0,num_parts=1 is
 * ff_render.  The RNG is keyed on the GLOBAL pixel index, so the union over parts is bit-identical to
 * the single-GPU image.  *out_local_rows receives the number of rows written (may be NULL). */
FF_API int ff_render_strips(FfState* state, const FfCamera* camera, const FfRenderParams* params,
                            int strip_rows, int part, int num_parts,
                            void* rgb8, int rgb8_on_device, float* radiance, int radiance_on_device,
                            int* out_local_rows);

/* One rectangular tile [x0, x0 + w) x [y0, y0 + h) of the frame into compact w x h buffers (row stride w): the other way
 * to partition a frame (SURVEY.md section 8b's ff_render_tile).  Pixels are identical to the same pixels of ff_render:
 * the random numbers are keyed on the global pixel index. */
FF_API int ff_render_tile(FfState* state, const FfCamera* camera, const FfRenderParams* params, int x0, int y0, int w, int h, void* rgb8,
                          int rgb8_on_device, float* radiance, int radiance_on_device);

/* Number of rows ff_render_strips writes for (height, strip_rows, part, num_parts). */
FF_API int ff_strips_local_rows(int height, int strip_rows, int part, int num_parts);

/* Scatter gathered per-part compact buffers back to image order on the device:
 * src holds, for part p = 0..num_parts-1 in order, that part's compact rows; elem_bytes is the size of
 * one pixel (3 for rgb8, 12 for float3 radiance). */
FF_API int ff_deinterleave_strips(FfState* state, const void* src_dev, void* dst_dev, int width, int height,
                                  int strip_rows, int num_parts, int elem_bytes);

/* ---- multi-GPU frames (no counterpart in the reference: its only trace of more than one GPU is the dead
 *      `const bool multi_gpu` of utilities.h:484-487; BASELINE north star: image tiles over the GPUs of a node, RCCL
 *      gather of the framebuffer over xGMI) ---------------------------------------------------------------------- */

/* Shape 1 — one process per GPU.  Rank 0 obtains an id (128 bytes) and hands it to the other ranks by any means it has
 * (a file, a socket, MPI, torch.distributed); every rank then joins with its own state.  One RCCL communicator per state. */
#define FF_DIST_ID_BYTES 128
FF_API int ff_dist_unique_id(void* out_id, int bytes);
FF_API int ff_dist_init(FfState* state, int rank, int world_size, const void* id, int bytes);
/* FF_OK if the RCCL library can be loaded in this process (what ff_dist_unique_id / ff_dist_init need).  Lets the ranks of a
 * job agree that all of them can join BEFORE any of them enters ff_dist_init, which blocks until every rank has. */
FF_API int ff_dist_available(void);
FF_API int ff_dist_shutdown(FfState* state);

/* Strip height the distributed renderers use when given strip_rows <= 0: of 1 .. 16 rows the height whose largest part has the
 * fewest rows (the slowest rank sets the frame time), the thinnest such of at least two rows: for 1080 rows 2-row strips over 2 or 4 GPUs, 3-row strips over 8
 * (equal shares: 135 rows each there).  ff_dist_strip_rows(world) is ff_dist_strip_rows_for(1080, world). */
FF_API int ff_dist_strip_rows_for(int height, int world_size);
FF_API int ff_dist_strip_rows(int world_size);

/* The gather's wire layout: bytes of the ONE message part `part` sends to rank 0 (its rows as float3 radiance, then as rgb8,
 * each section padded to 16 bytes; 0 for a part that owns no rows: then no message is posted on either side) and, through
 * out_offset (may be null), where it lands in rank 0's gather buffer.  -1 for invalid arguments. */
FF_API long long ff_dist_part_bytes(int width, int height, int strip_rows, int part, int num_parts, long long* out_offset);

/* One frame over all ranks; every rank calls it with the same camera and params.  Each rank renders the strips
 * s % world == rank (ff_render_strips' partition) into one packed buffer and sends it to rank 0 in a single message;
 * rank 0 receives every peer's message into its gather buffer (one grouped RCCL call) and scatters all strips to image
 * order.  On rank 0, rgb8 / radiance receive the full frame, bit-identical to ff_render's (device or host pointers, as
 * there); on other ranks they are ignored.  Synchronous on return on every rank; ff_stats reports this rank's share.
 *
 * Errors.  No rank is left waiting for a message that cannot come: every rank first does what can fail locally (argument
 * checks, buffers, the launches of its strips), then the ranks agree on a status (a 4-byte all-reduce), and only a frame that
 * is well on every rank is gathered.  A local failure returns its own status on the rank it happened on and FF_ERR_COMM on
 * every other rank; the communicator stays usable.  Waits on other ranks have a deadline (FF_DIST_TIMEOUT_S in the
 * environment at ff_dist_init, default 300 seconds) and watch ncclCommGetAsyncError: a missing or dead peer ends the call with
 * FF_ERR_COMM, the communicator is aborted (ncclCommAbort), and every later call returns FF_ERR_COMM until ff_dist_init has
 * made a new one.  After such an error the process should exit; a fresh process is the retry. */
FF_API int ff_render_distributed(FfState* state, const FfCamera* camera, const FfRenderParams* params, int strip_rows,
                                 void* rgb8, int rgb8_on_device, float* radiance, int radiance_on_device);
/* Tests: from the next frame on, rank `rank` of the job reports an injected local failure (FF_ERR_OOM) before its strips are
 * enqueued; -1 switches it off.  FF_DEBUG_DIST_FAIL_RANK in the environment at ff_dist_init sets the initial value. */
FF_API int ff_debug_dist_fail_rank(FfState* state, int rank);

/* Shape 2 — one process, several GPUs: what a single-process viewer (the reference's main(), kernel.cu:223-368) calls.
 * ff_multi_create makes one state per entry of device_ids, each with its own stream; device_ids[0] is the gathering device
 * (the one whose GL context owns the pixel buffer).  Transport: RCCL (ncclCommInitAll + grouped send/recv); peer copies
 * (hipMemcpyPeerAsync) when a device id repeats — RCCL refuses that, and it is how a one-GPU box rehearses the path — or
 * when FF_MULTI_TRANSPORT=peer. */
typedef struct FfMulti FfMulti;
FF_API int ff_multi_create(FfMulti** out_multi, const int* device_ids, int n);
FF_API int ff_multi_destroy(FfMulti* multi);
FF_API int ff_multi_count(const FfMulti* multi);
FF_API FfState* ff_multi_state(FfMulti* multi, int index);       /* per-device calls: ff_register_gl_pbo on index 0, ff_set_builder, ... */
FF_API int ff_multi_uses_rccl(const FfMulti* multi);
FF_API int ff_multi_upload_scene(FfMulti* multi, const FfGeometry* host_geometries, int n); /* replicated on every device */
/* The frame: all devices render their strips at once, device 0 gathers.  Outputs as in ff_render, on / from device 0. */
FF_API int ff_multi_render(FfMulti* multi, const FfCamera* camera, const FfRenderParams* params, int strip_rows,
                           void* rgb8, int rgb8_on_device, float* radiance, int radiance_on_device);
/* kernel.cu:335-344 with all GPUs behind it: the pixel buffer registered on ff_multi_state(multi, 0). */
FF_API int ff_multi_render_to_pbo(FfMulti* multi, const FfCamera* camera, const FfRenderParams* params, int strip_rows);
/* Sums over the devices of the last frame (kernel_ms: the slowest device). */
FF_API int ff_multi_stats(FfMulti* multi, FfStats* out);
/* ff_set_pixel_jitter on every device's state. */
FF_API int ff_multi_set_pixel_jitter(FfMulti* multi, float jx, float jy);

/* Batch closest-hit query = intersectRays (kernel.cu:127-176) for `n` arbitrary world-space rays.
 * rays/out are host arrays. trace_mode is an FfTraceMode. */
FF_API int ff_intersect_rays(FfState* state, const FfRay* rays, int n, FfIntersect* out, int trace_mode);

/* ---- OpenGL pixel-buffer interop (utilities.h:605-618, kernel.cu:335-344) ----------------------- */

/* cudaGraphicsGLRegisterBuffer(&res, pbo, WriteDiscard) twin via hipGraphicsGLRegisterBuffer.
 * The GL context that owns `pbo` must be current on the calling thread.  The buffer must hold
 * width*height*3 bytes. */
FF_API int ff_register_gl_pbo(FfState* state, unsigned int pbo, int width, int height);
FF_API int ff_unregister_gl_pbo(FfState* state);

/* map -> clear -> trace -> unmap  (kernel.cu:337-344).  params->width/height must match the registration. */
FF_API int ff_render_to_pbo(FfState* state, const FfCamera* camera, const FfRenderParams* params);

/* ---- progressive accumulation (the reference's README sketches it) ------------------- */

/* Frame `frame_index` (0, 1, 2, ... while the camera is still) of a progressive sequence: an ordinary frame rendered with
 * seed + frame_index, added in fp32 to a running per-pixel sum kept in the state; the outputs are sum * (1 / frames) and
 * its 8-bit quantisation.  frame_index 0 restarts the sequence (call it when the camera or the scene changed); other
 * indices must continue it.  Buffers as in ff_render. */
FF_API int ff_render_progressive(FfState* state, const FfCamera* camera, const FfRenderParams* params, int frame_index, void* rgb8, int rgb8_on_device,
                                 float* radiance, int radiance_on_device);

/* The same into the registered pixel buffer (the per-frame block of kernel.cu:335-344). */
FF_API int ff_render_to_pbo_progressive(FfState* state, const FfCamera* camera, const FfRenderParams* params, int frame_index);

/* ---- next-event estimation (FF_SHADE_DIFFUSE_PATH_NEE; no counterpart in the reference) ---- */

/* FF_SHADE_DIFFUSE_PATH_NEE has FF_SHADE_DIFFUSE_PATH's expectation for the same scene, camera, jitter and bounces, with lower
 * variance.  Per sample, with beta the throughput and L the sample's radiance (L = 0 at the camera):
 *   BSDF side: camera rays, scatter directions, throughput updates, mirror, glass, the 1e-4 n^ origin offset and the accumulation
 *     (blocks of 64 samples summed in order, blocks added in order, times 1/spp) are FF_SHADE_DIFFUSE_PATH's, with its random
 *     numbers: Philox2x32-10, counter (gpix, s << 8 | b), key = seed ^ (seed >> 32) (gpix = y * width + x, s sample, b segment).
 *   Light table (ff_light_table): one entry per emitting plane (the world image of its unit quad) and per triangle of an emitting
 *     mesh; spheres and emitters of zero luminance are left out.  lum = 0.2126 r + 0.7152 g + 0.0722 b of m_emissiveColor * m_intensity;
 *     entry k is chosen with probability A_k lum_k / S, S = sum_k A_k lum_k, so pdf_A(g) = lum_g / S per unit area on geometry g
 *     (0 for geometries not in the table).
 *   Light sample, at a diffuse hit x of segment b < bounces - 1 (beta already holds this hit's albedo; n^ = the unit geometric
 *     normal flipped against the incoming ray, as scatter uses it):
 *       (r0, r1) = Philox(gpix, s << 8 | b, key ^ 0x6A09E667):  k = floor(r0 * n / 2^32); if !((r1 >> 8) / 2^24 < alias_probability_k)
 *                                                                k = alias_k
 *       (q0, q1) = Philox(gpix, s << 8 | b, key ^ 0xBB67AE85):  u = (q0 >> 8) / 2^24, v = (q1 >> 8) / 2^24
 *       y = v0 + u e1 + v e2 (plane);  y = v0 + sqrt(u)(1 - v) e1 + sqrt(u) v e2 (triangle)
 *       w = unit(y - x), d2 = |y - x|^2, cos_x = n^ . w, cos_y = |n_y . w|
 *       if cos_x > 0 and cos_y > 0: a shadow ray from x + 1e-4 n^ along w; the sample is visible iff the ray's closest hit is the
 *       sampled primitive (same geometry; same triangle for meshes).  Then
 *         pdf_l = pdf_A(g) d2 / cos_y,  pdf_b = cos_x / pi,  w_l = pdf_l^2 / (pdf_l^2 + pdf_b^2)
 *         L += beta Le (cos_x / pi) w_l / pdf_l
 *   BSDF-sampled emitter hits: L += beta Le after the camera ray or a mirror / glass bounce; after a diffuse bounce
 *     L += beta Le w_b, w_b = pdf_b^2 / (pdf_b^2 + pdf_l^2), pdf_b = cos / pi of the sampled direction at the previous vertex,
 *     pdf_l = pdf_A(hit geometry) t^2 / |n . w| (t the hit distance); pdf_A = 0 (weight 1) for geometries not in the table.
 *   No light sample on the last segment, so the mode's expectation is FF_SHADE_DIFFUSE_PATH's at the same bounces.  With an empty
 *   table every sample is FF_SHADE_DIFFUSE_PATH's bit for bit.  Results do not depend on the lane, spp_per_launch, tile or strip.
 * Geometric normals only (smooth-normal NEE is not offered).  ff_render, ff_render_tile, ff_render_strips, ff_render_progressive
 * and the pixel-buffer twins render it; ff_render_distributed and ff_multi_render* return FF_ERR_UNSUPPORTED, and so does a state
 * whose scene came from ff_multi_upload_scene.  FfStats: rays_traced counts extension and shadow rays, kernel_ms / kernel_launches
 * cover the NEE kernel launches and the combine pass, rays_answered and rays_cut_short are 0. */

/* Host-only: the light table FF_SHADE_DIFFUSE_PATH_NEE samples for a host scene, as ff_upload_scene builds it (in double, stored as
 * float).  Writes up to max_entries entries (may be 0 with out_entries NULL) and, if out_pdf_area is not NULL, n floats: pdf_A per
 * caller geometry (0 outside the table).  Returns the number of entries, or minus an FfStatus.  Needs no GPU. */
FF_API int ff_light_table(const FfGeometry* host_geometries, int n, FfLightEntry* out_entries, int max_entries, float* out_pdf_area);

/* Host-only: FF_OK if every render entry point would accept `params` (sizes, bounces, spp, modes), else FF_ERR_INVALID_ARG. */
FF_API int ff_check_render_params(const FfRenderParams* params);

/* ---- environment light (no counterpart in the reference) ----------------------------------------- */

/* A map of W x H linear RGB texels (row 0 the top, +Y) around the scene: what a ray that leaves the scene sees, times `intensity`.
 *   Mapping of a unit direction d: phi = atan2(d.x, -d.z) - rotation, wrapped to [0, 2 pi); theta = acos(clamp(d.y, -1, 1));
 *     column c = min(floor(phi / 2 pi * W), W - 1), row r = min(floor(theta / pi * H), H - 1); nearest texel, so the radiance
 *     Le = intensity * texel (in float) is constant over texel (r, c), which covers the solid angle
 *     Omega_rc = (2 pi / W)(cos(pi r / H) - cos(pi (r + 1) / H)).
 *   Table (ff_environment_table; built in double): w_rc = lum_rc Omega_rc (lum = 0.2126 r + 0.7152 g + 0.0722 b of the texel),
 *     p_rc = w_rc / sum, a Vose alias table over the W H texels (index k = r W + c), pdf_env = p_rc / Omega_rc per steradian.
 *     A map of zero total luminance has an empty table: it is never sampled, and pdf_env = 0.
 *   With an environment set, FF_SHADE_DIFFUSE_PATH and FF_SHADE_DIFFUSE_PATH_NEE add, on every segment including the last, for a
 *   ray that hits nothing:  L += beta Le(w) w_b, where w_b = 1 after the camera ray or a mirror / glass bounce and always in
 *   FF_SHADE_DIFFUSE_PATH, and w_b = pdf_b^2 / (pdf_b^2 + (p_env pdf_env(w))^2) after a diffuse bounce in FF_SHADE_DIFFUSE_PATH_NEE.
 *   FF_SHADE_DIFFUSE_PATH_NEE's light sample (the block above) then chooses between the environment and the light table:
 *       p_env = 1/2 with a non-empty light table, 1 without one, 0 if the environment's table is empty;
 *       if 0 < p_env < 1: (c0, c1) = Philox(gpix, s << 8 | b, key ^ 0x3C6EF372), the environment iff (c0 >> 8) / 2^24 < p_env.
 *     The light table's branch is the one above with pdf_l = (1 - p_env) pdf_A(g) d2 / cos_y, and so is the weight of a
 *     BSDF-sampled emitter hit.  The environment's branch, with the same (r0, r1) and (q0, q1):
 *       k = floor(r0 * W H / 2^32); if !((r1 >> 8) / 2^24 < alias_probability_k) k = alias_k; r = k / W, c = k % W
 *       z = z_r + u (z_{r+1} - z_r), z_r = cos(pi r / H) (stored as float);  phi = (c + v) 2 pi / W + rotation
 *       w = (sqrt(1 - z^2) sin phi, z, -sqrt(1 - z^2) cos phi),  cos_x = n^ . w
 *       if cos_x > 0 and pdf_env_k > 0: a shadow ray from x + 1e-4 n^ along w, visible iff it hits nothing.  Then
 *         pdf_l = p_env pdf_env_k,  pdf_b = cos_x / pi,  w_l = pdf_l^2 / (pdf_l^2 + pdf_b^2),  L += beta Le_k (cos_x / pi) w_l / pdf_l
 *   Without an environment no frame changes, and no random number is drawn for it.  With an all-zero map every frame is the frame
 *   without an environment bit for bit.  Results do not depend on the lane, spp_per_launch, tile or strip.
 * FF_SHADE_NORMAL_DEBUG ignores the environment; FF_SHADE_DIFFUSE_PATH_SMOOTH returns FF_ERR_UNSUPPORTED while one is set, and so do
 * ff_render_distributed, ff_multi_render*, and a state whose scene came from ff_multi_upload_scene, for FF_SHADE_DIFFUSE_PATH and
 * FF_SHADE_DIFFUSE_PATH_NEE frames.  ff_gbuffer does not see it (a miss stays a miss).  FfStats.rays_traced counts the shadow rays.
 * The environment belongs to the state: it stays through ff_upload_scene and the update calls, until it is replaced, cleared or
 * the state is destroyed. */

/* Sets the state's environment (copied to the device): `rgb` is height rows of width RGB floats; rgb == NULL clears it.
 * FF_ERR_INVALID_ARG for a size below 1x1 or above 2^26 texels, a negative or non-finite texel, a negative or non-finite
 * intensity, a non-finite rotation.  rotation_deg turns the map about world +Y (see the mapping above). */
FF_API int ff_set_environment(FfState* state, const float* rgb, int width, int height, float intensity, float rotation_deg);

/* Host-only: the table ff_set_environment builds for the map, W H entries each (any output may be NULL): probability p_rc,
 * alias_probability, alias, pdf_env.  An all-zero map gives p = 0, alias_probability = 1, alias = itself and pdf = 0.
 * FF_ERR_INVALID_ARG as ff_set_environment. */
FF_API int ff_environment_table(const float* rgb, int width, int height, float* out_probability, float* out_alias_probability, int* out_alias,
                                float* out_pdf);

/* Reads a Radiance RGBE (.hdr) file: a "#?" signature, header lines up to an empty line (FORMAT=32-bit_rle_rgbe or none), the
 * resolution line "-Y h +X w" (other orientations are not supported), then h scanlines, each flat (w RGBE quadruples) or
 * new-style run-length encoded (2 2 w>>8 w&255, then the four channels as runs).  Texel = (R, G, B) * 2^(E - 136) (0 if E = 0),
 * row 0 the top.  *out_rgb is malloc'ed (h rows of w RGB floats); release with ff_free_hdr.  FF_ERR_IO for a file that cannot be
 * opened or ends early, FF_ERR_INVALID_ARG for a malformed or unsupported one. */
FF_API int ff_load_hdr(const char* path, float** out_rgb, int* out_width, int* out_height);
FF_API void ff_free_hdr(float* rgb);

/* ---- albedo textures (no counterpart in the reference) ----------------------------------------- */

/* A texture is W x H linear RGB texels, row 0 the top of the image, bound to the albedo of a FF_BXDF_DIFFUSE geometry: at a hit x
 * of that geometry the surface's albedo is m_albedo * texel(c) per channel, in FF_SHADE_DIFFUSE_PATH, FF_SHADE_DIFFUSE_PATH_NEE
 * and ff_gbuffer's albedo plane.  All arithmetic is float32, evaluated as parenthesised, no fused multiply-add;
 * dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z.
 *   Surface coordinate uv of the WORLD hit point x (the G-buffer's position; never a function of the ray, so the integrator and
 *   ff_gbuffer compute the same bits for the same hit):
 *     object point  p_k = (I0_k x.x + I1_k x.y) + (I2_k x.z + I3_k), I0 .. I3 the columns of m_inverseModelMatrix
 *     triangle      e1 = v1 - v0, e2 = v2 - v0, d = p - v0;  d00 = dot(e1, e1), d01 = dot(e1, e2), d11 = dot(e2, e2),
 *                   d20 = dot(d, e1), d21 = dot(d, e2);  den = d00 d11 - d01 d01;  u = (d11 d20 - d01 d21) / den,
 *                   v = (d00 d21 - d01 d20) / den;  uv = (uv0 + u (uv1 - uv0)) + v (uv2 - uv0) with the triangle's m_uv0 .. m_uv2
 *     plane         uv = (p.x + 0.5, p.y + 0.5) of the unit quad
 *     sphere        u = atan2f(p.x, -p.z) / 2 pi, plus 1 if negative;  v = 1 - acosf(clamp(p.y / |p|, -1, 1)) / pi
 *                   (the environment map's orientation, +Y at the top row; host and device may differ by an ulp here)
 *   Lookup coordinate  c = uv * scale + offset per component (ff_set_albedo_texture).
 *   Sanitising    a coordinate that is NaN or +-Inf reads as 0.  FF_TEX_REPEAT then takes c - floor(c), in [0, 1] (exact for
 *                 c >= 0: the lookup is periodic bit for bit), FF_TEX_CLAMP takes min(max(c, 0), 1).  Every texel index is therefore
 *                 in range for any bit pattern of the coordinate.
 *   Addressing    image row 0 is v = 1 (the OBJ convention).  FF_TEX_BILINEAR: s = c.u W - 0.5, t = (1 - c.v) H - 0.5,
 *                 x0 = floor(s), fx = s - x0, y0 = floor(t), fy = t - y0; taps x0, x0 + 1 and y0, y0 + 1, under REPEAT moved by
 *                 W (H) back into the image, under CLAMP clamped into it;  a = T(x0, y0), b = T(x0 + 1, y0), c = T(x0, y0 + 1),
 *                 d = T(x0 + 1, y0 + 1):  top = a + fx (b - a), bot = c + fx (d - c), texel = top + fy (bot - top), so a texture of
 *                 one constant value returns that value exactly.  FF_TEX_NEAREST: x = floor(c.u W), y = floor((1 - c.v) H); an index
 *                 W (H) becomes 0 under REPEAT and W - 1 (H - 1) under CLAMP.
 * Textures belong to the state: they stay through ff_upload_scene until ff_texture_destroy or ff_destroy.  Bindings belong to the
 * scene: ff_upload_scene drops them; ff_update_transforms and ff_update_mesh keep them (after ff_update_mesh the new triangles' UVs
 * are the ones sampled, in both modes and with every builder).  A binding whose geometry ff_update_transforms makes non-diffuse stays
 * but is not applied.  While a binding exists, FF_SHADE_DIFFUSE_PATH and FF_SHADE_DIFFUSE_PATH_NEE frames run the NEE kernel (the plain
 * path mode with no light sample: its estimator and random numbers are unchanged); a texture whose texels are all 1 leaves every
 * frame and the G-buffer bit for bit as they are without it.  FF_SHADE_NORMAL_DEBUG ignores textures.  FF_SHADE_DIFFUSE_PATH_SMOOTH,
 * ff_render_distributed, ff_multi_render* and a state whose scene came from ff_multi_upload_scene return FF_ERR_UNSUPPORTED while a
 * binding exists (the environment light's precedent).  Emission, specular and normal maps and mip-mapping are not offered. */

/* Copies a texture to the device: `rgb` is height rows of width RGB floats.  flags: FF_TEX_REPEAT or FF_TEX_CLAMP, FF_TEX_BILINEAR or
 * FF_TEX_NEAREST.  *out_id receives its id (>= 0; ids of destroyed textures are reused).  FF_ERR_INVALID_ARG for a size below 1x1
 * or above 2^26 texels, a negative or non-finite texel, an unknown flag (ff_set_environment's rules). */
FF_API int ff_texture_create(FfState* state, const float* rgb, int width, int height, int flags, int* out_id);

/* Frees texture `id` and unbinds it wherever it is bound. */
FF_API int ff_texture_destroy(FfState* state, int id);

/* Binds texture `texture_id` to the albedo of geometry `geometry_index` (the caller's index in the uploaded array) with the lookup
 * coordinate uv * scale + offset; texture_id = -1 unbinds.  FF_ERR_NO_SCENE without a scene; FF_ERR_INVALID_ARG for an unknown
 * geometry or texture or a non-finite scale or offset; FF_ERR_UNSUPPORTED for a geometry that is not FF_BXDF_DIFFUSE. */
FF_API int ff_set_albedo_texture(FfState* state, int geometry_index, int texture_id, float scale_u, float scale_v, float offset_u,
                                 float offset_v);

/* Host-only twins (no GPU, no state), compiled from the same inline functions the kernels use. */
/* The texel lookup for n coordinates `uv` (n pairs, taken as the lookup coordinate c) into out_rgb (n triples).
 * FF_ERR_INVALID_ARG as ff_texture_create. */
FF_API int ff_texture_sample(const float* rgb, int width, int height, int flags, const float* uv, int n, float* out_rgb);
/* The surface coordinate uv of `count` world points (count triples) on geometry `geometry_index` of a host scene, before scale and
 * offset; triangle_indices (count entries, the caller's triangle index of each point) is read for meshes only and may be NULL
 * otherwise.  FF_ERR_INVALID_ARG for an unknown geometry or triangle index. */
FF_API int ff_surface_uv(const FfGeometry* host_geometries, int n, int geometry_index, const int* triangle_indices,
                         const float* world_points, int count, float* out_uv);

/* ---- rough-specular mirrors (no counterpart in the reference) ----------------------------------- */

/* A roughness bound to a FF_BXDF_MIRROR geometry turns the perfect mirror into a microfacet conductor: GGX normal distribution,
 * height-correlated Smith masking, Schlick Fresnel with F0 = m_specularColor.  alpha = roughness * roughness (float).  A binding with
 * alpha < 1e-3 shades as the perfect mirror (the delta branch, no light sample, pdf_b = 0).  FF_SHADE_DIFFUSE_PATH and
 * FF_SHADE_DIFFUSE_PATH_NEE render it.  All arithmetic is float32, evaluated as parenthesised, no fused multiply-add; a quotient is
 * a * (1 / b) with a correctly rounded reciprocal, roots are correctly rounded; dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z.
 *   Frame      the Duff basis (t, s, n^) scatter builds about the unit geometric normal n^ flipped against the incoming ray; a world
 *              direction w has the local components (dot(t, w), dot(s, w), dot(n^, w)).  wo = minus the ray direction, wo.z clamped
 *              to >= 1e-6; wi = the direction towards the light.  Every w.z in a quotient is clamped to >= 1e-6.
 *   Lobe       h = unit(wo + wi);  D(h) = alpha^2 / (pi q^2), q = alpha^2 h.z^2 + (h.x^2 + h.y^2)
 *              Lambda(w) = (sqrt(1 + alpha^2 (w.x^2 + w.y^2) / w.z^2) - 1) / 2;  G1(w) = 1 / (1 + Lambda(w));
 *              G2(wo, wi) = 1 / (1 + Lambda(wo) + Lambda(wi));  F(c) = F0 + (1 - F0) m^5 per channel, m = 1 - c, c = max(dot(wo, h), 0),
 *              m^5 = (m2 m2) m with m2 = m m
 *              f(wo, wi) = F D G2 / (4 wo.z wi.z) (0 for wi.z <= 0);  pdf_b(wi) = G1(wo) D(h) / (4 wo.z)
 *              weight = f wi.z / pdf_b = F G2 / G1 = F (1 + Lambda(wo)) / ((1 + Lambda(wo)) + Lambda(wi)), computed in that form
 *   Sampling   visible normals by spherical caps (Dupuy and Benyoub 2023), from the numbers the diffuse scatter would have drawn at
 *              this vertex: (r0, r1) = Philox(gpix, s << 8 | b, key), k = r0 >> 8, u1 = k / 2^24, u2 = (r1 >> 8) / 2^24
 *              v = unit(alpha wo.x, alpha wo.y, wo.z);  z = (1 - u2)(1 + v.z) - v.z;  r = sqrt(max(0, 1 - z^2))
 *              c = (r cos(2 pi u1), r sin(2 pi u1), z) (sine and cosine: the diffuse bounce's fixed-order polynomials on the octant
 *              taken exactly off k);  h' = c + v;  h = unit(alpha h'.x, alpha h'.y, max(h'.z, 0));  wi = 2 dot(wo, h) h - wo
 *              The sample's weight and pdf_b are the lobe's expressions at (wo, wi), h recomputed from them.
 *   At a glossy hit x of segment b (a mirror with an applied binding and alpha >= 1e-3; beta is NOT multiplied at the hit):
 *     if b < bounces - 1, in FF_SHADE_DIFFUSE_PATH_NEE, with a non-empty light table or a sampled environment: one light sample, with
 *       the streams, the choice between environment and table, the point, w, pdf_l, the shadow ray and the visibility rule of the
 *       blocks above.  With wi = w in the local frame and cos_x = wi.z = dot(n^, w): if cos_x > 0 (and cos_y > 0 for the table)
 *         pb = pdf_b(wi),  w_l = pdf_l^2 / (pdf_l^2 + pb^2),  L += beta Le f(wo, wi) cos_x w_l / pdf_l
 *     then the scatter: wi by the sampler.  wi.z <= 0: the sample ends at this vertex (after its shadow ray, if one is pending); its
 *       radiance so far joins the sum, as for a last segment.  Else beta *= F G2 / G1, the new ray starts at x + 1e-4 n^ along wi,
 *       and pdf_b(wi) is the pdf a BSDF-sampled emitter hit or environment miss of the next segment is weighted with, exactly as
 *       after a diffuse bounce: w_b = pdf_b^2 / (pdf_b^2 + pdf_l^2).
 *     In FF_SHADE_DIFFUSE_PATH, and on the last segment, there is no light sample and w_b = 1.
 * ff_set_roughness binds; roughness = 0 unbinds.  Bindings belong to the scene: ff_upload_scene drops them; ff_update_transforms
 * and ff_update_mesh keep them.  A binding whose geometry ff_update_transforms makes non-mirror stays but is not applied.  While an
 * applied binding exists, FF_SHADE_DIFFUSE_PATH and FF_SHADE_DIFFUSE_PATH_NEE frames run the NEE kernel (the plain path mode with no
 * light sample: its random numbers at non-glossy vertices are unchanged); without one, every frame launches exactly the kernels it
 * launched before.  Results do not depend on the lane, spp_per_launch, tile, strip or trace mode.  FF_SHADE_NORMAL_DEBUG ignores
 * bindings.  FF_SHADE_DIFFUSE_PATH_SMOOTH, ff_render_distributed, ff_multi_render* and a state whose scene came from
 * ff_multi_upload_scene return FF_ERR_UNSUPPORTED while an applied binding exists (the environment's and the textures' precedent).
 * ff_gbuffer is unchanged (its albedo plane holds m_specularColor for mirrors) and the denoisers go on treating the pixel as not
 * filterable.  Not offered: rough glass, anisotropy, multiple-scattering energy compensation, roughness textures, a glossy coat over
 * diffuse, smooth-normal shading of the lobe, glossy frames on the multi-GPU entry points (there is no ff_multi_set_roughness). */

/* Binds `roughness` in [0, 1] to geometry `geometry_index` (the caller's index in the uploaded array); 0 unbinds.  FF_ERR_NO_SCENE
 * without a scene; FF_ERR_INVALID_ARG for an unknown geometry or a roughness that is not finite or outside [0, 1];
 * FF_ERR_UNSUPPORTED for a geometry whose bxdf is not FF_BXDF_MIRROR. */
FF_API int ff_set_roughness(FfState* state, int geometry_index, float roughness);

/* Host-only twins (no GPU, no state), compiled from the same inline functions the kernel uses.  alpha in (0, 1]; directions are
 * unit vectors in the local frame (z the normal; wo.z is clamped to >= 1e-6 as in the kernel). */
/* The lobe for n pairs (wo, wi): out_f_rgb (n triples) = f(wo, wi), the BRDF not times cosine; out_pdf (n) = pdf_b(wi) per steradian.
 * Both 0 for wi.z <= 0. */
FF_API int ff_glossy_eval(float alpha, const float* f0_rgb, const float* wo, const float* wi, int n, float* out_f_rgb, float* out_pdf);
/* The sampler for n directions wo and n pairs u = (u1, u2) in [0, 1)^2 (u1 is used as floor(u1 2^24), the kernel's integer):
 * out_wi (n triples), out_weight_rgb (n triples) = F G2 / G1, out_pdf (n) = pdf_b(wi).  For a wi at or below the horizon the
 * weight and the pdf are 0. */
FF_API int ff_glossy_sample(float alpha, const float* f0_rgb, const float* wo, const float* u, int n, float* out_wi, float* out_weight_rgb,
                            float* out_pdf);

/* ---- per-sample camera rays: box pixel filter and thin lens (no counterpart in the reference) ---- */

/* Without a setting every sample of a pixel starts with the same ray: primary_ray's, through the pixel's corner moved by the state's
 * jitter (ff_set_pixel_jitter).  An ACTIVE setting - pixel_filter == FF_PIXEL_BOX or lens_radius > 0 - draws a camera ray per sample:
 * a uniform point of the pixel (the frame converges to the box-filtered image within one call) and / or a uniform point of a thin
 * lens of radius lens_radius about m_position in the plane of m_right and m_up, focused on the plane at focus_distance along
 * m_forward (depth of field).  FF_SHADE_DIFFUSE_PATH and FF_SHADE_DIFFUSE_PATH_NEE render it.  All arithmetic is float32, evaluated
 * as parenthesised, no fused multiply-add; a quotient by a computed value is a * rcp(b) with a correctly rounded reciprocal, roots
 * are correctly rounded; dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z.
 * For sample s of global pixel (x, y): gpix = y * width + x, key = seed ^ (seed >> 32) (the frame key), u24(r) = (r >> 8) / 2^24.
 *   Pixel point  FF_PIXEL_CORNER: fx = fy = 0 and M = the state's jittered ray matrix (ff_camera_ray_matrix_jittered), as ever.
 *                FF_PIXEL_BOX: (a0, a1) = Philox2x32-10(gpix, s << 8, key ^ 0xA54FF53A), fx = u24(a0), fy = u24(a1), and M = the
 *                UNJITTERED ff_camera_ray_matrix: the state's jitter is not applied to such frames (ff_gbuffer goes on using it).
 *                Px = (((float)x + fx) / screen_w) * 2 - 1,  Py = 1 - (((float)y + fy) / screen_h) * 2
 *   Pinhole      v = (Px far, Py far, far, far);  w_k = (M0_k v.x + M1_k v.y) + (M2_k v.z + M3_k v.w), M0 .. M3 the columns of M;
 *                dd = w - o, o = m_position;  d = dd * rcp(sqrt(dot(dd, dd))): kernel.cu:197-205 operation for operation, and with
 *                fx = fy = 0 the ray every frame without a setting traces, bit for bit.
 *   Lens         (lens_radius > 0)  f^, r^, u^ = m_forward, m_right, m_up as the caller's floats, not renormalised.
 *                c = dot(d, f^).  If !(c > 1e-6) the pinhole ray is kept.  Else t = focus_distance * rcp(c), F = o + d t per
 *                component;  (l0, l1) = Philox(gpix, s << 8, key ^ 0x510E527F);  (sn, cs) = the sine and cosine of 2 pi (l0 >> 8) / 2^24
 *                by the glossy sampler's fixed-order polynomials on the exactly reduced octant;  rho = lens_radius * sqrt(u24(l1)),
 *                a = rho cs, b = rho sn;  o' = o + (a r^ + b u^) per component;  dd' = F - o',
 *                d' = dd' * rcp(sqrt(dot(dd', dd'))).  The sample's ray is (o', d').
 *   Weight       1 (an ideal thin lens, no vignetting): the throughput starts at 1 as ever.  The path, its random numbers at every
 *                vertex, the light samples, the accumulation (blocks of 64 samples in order) and every other stream are unchanged.
 * The setting belongs to the state, like the jitter and the environment: it stays through ff_upload_scene and the update calls
 * until it is replaced or the state is destroyed.  While it is active, FF_SHADE_DIFFUSE_PATH and FF_SHADE_DIFFUSE_PATH_NEE frames run
 * the NEE kernel (the plain path mode with no light sample); without it, every frame launches exactly the kernels it launched before
 * and produces the same bits.  Results do not depend on the lane, spp_per_launch, tile, strip or trace mode.  ff_render,
 * ff_render_tile, ff_render_strips, ff_render_progressive and the pixel-buffer twins render it.  FF_SHADE_NORMAL_DEBUG ignores the
 * setting.  FF_SHADE_DIFFUSE_PATH_SMOOTH, ff_render_distributed, ff_multi_render* and a state whose scene came from
 * ff_multi_upload_scene return FF_ERR_UNSUPPORTED while it is active (the environment's, the textures' and the mirrors' precedent).
 * ff_gbuffer, ff_intersect_rays and the image filters are unchanged: the G-buffer stays the PINHOLE's first hit (with the state's
 * jitter), which is the usual guide for denoising a defocused frame.  Not offered: other pixel filters, polygonal apertures,
 * vignetting, motion blur, a defocus-aware G-buffer, the setting on the multi-GPU entry points. */

/* FF_PIXEL_CORNER, lens_radius 0, focus_distance 1, reserved 0: today's camera. */
FF_API void ff_camera_sampling_init(FfCameraSampling* cs);

/* Replaces the state's setting; NULL = the defaults.  FF_ERR_INVALID_ARG, naming the field, for an unknown pixel_filter, a negative
 * or non-finite lens_radius, a non-finite focus_distance or one <= 0 while lens_radius > 0, a non-zero reserved. */
FF_API int ff_set_camera_sampling(FfState* state, const FfCameraSampling* cs);

/* Host-only twin (no GPU, no state), compiled from the same inline functions the kernel uses: the rays of n samples - sample
 * samples[i] of pixel (xs[i], ys[i]) of an image `width` pixels wide under `seed` - into out_origins3 and out_directions3 (n triples
 * each).  cs = NULL: the defaults.  jitter_x / jitter_y: the state's pixel jitter, applied under FF_PIXEL_CORNER only, as in a frame.
 * FF_ERR_INVALID_ARG for a NULL pointer, n < 0, width < 1, a negative coordinate or sample, a jitter outside [0, 1), and the
 * setting's own checks. */
FF_API int ff_camera_sample_rays(const FfCamera* camera, const FfCameraSampling* cs, float jitter_x, float jitter_y, int width, uint64_t seed,
                                 const int* xs, const int* ys, const int* samples, int n, float* out_origins3, float* out_directions3);

/* ---- G-buffer and denoiser (no counterpart in the reference) ----------------------------- */

/* What every pixel's primary ray (kernel.cu:197-205) hits: I = intersectRays (kernel.cu:127-176) for that ray, the FfIntersect
 * of ff_intersect_rays bit for bit.  Buffers are row-major, top row first; any may be NULL; on_device as ff_render's flags.
 *   depth     W*H   floats  I.m_t (world distance)                                   miss: 0
 *   position  W*H*3 floats  I.m_intersectionPoint                                    miss: 0
 *   normal    W*H*3 floats  I.m_normal: the signed world normal NORMAL_DEBUG shades, in every shade mode (not the interpolated
 *                           normal of SMOOTH mode); not renormalised after the inverse-transpose      miss: 0
 *   albedo    W*H*3 floats  emitter m_emissiveColor * m_intensity, mirror m_specularColor, glass m_transmittanceColor,
 *                           anything else m_albedo, times the texel of a bound albedo texture (diffuse only)   miss: 0
 *   ids       W*H*3 int32   {I.geometryIndex (caller's order), I.triangleIndex (-1 for planes and spheres), bxdf type}
 *                                                                                    miss: {-1, -1, -1}
 * Only the camera, the scene, width, height and grid_mode matter (FF_GRID_REFERENCE_FLOOR: untraced pixels read as misses);
 * spp, bounces, seed, trace_mode, shade_mode and spp_per_launch do not change a bit.  When the state still holds the last
 * frame's primary hits for this camera and pixel mapping (a camera at rest), they are resolved without a traversal; otherwise
 * the call traces the primary rays into a buffer of its own.  It leaves the state's stored hits, "camera at rest" test and
 * FfStats as they were: it is not a frame.  FF_ERR_UNSUPPORTED for a tree too deep for BVH rendering. */
FF_API int ff_gbuffer(FfState* state, const FfCamera* camera, const FfRenderParams* params,
                      float* depth, float* position, float* normal, float* albedo, int32_t* ids, int on_device);

/* Defaults (DESIGN.md section 10 measured them): 5 passes, sigma_color 4, sigma_normal 0.1, sigma_plane 0.1, both flags. */
FF_API void ff_denoise_params_init(FfDenoiseParams* p);

/* Edge-avoiding à-trous filter (Dammertz et al. 2010) of W x H float3 radiance (e.g. ff_render's or ff_render_progressive's mean),
 * guided by a G-buffer of ff_gbuffer (position, normal, ids; albedo with FF_DENOISE_DEMODULATE_ALBEDO, else it may be NULL).
 * A pure image operation: the scene is not read.
 *   filterable pixel: a hit whose bxdf is not emitter, mirror or glass.  Every other pixel is copied through bit for bit and
 *                     weighs 0 as a tap.
 *   c               = radiance / albedo per channel (DEMODULATE_ALBEDO; channels with albedo <= 0 undivided), else radiance
 *   pass i          : c'_p = sum_q w c_q / sum_q w over the 5x5 taps q = p + 2^i (dx, dy), dx, dy in -2..2,
 *                     w = h(dx) h(dy) w_c w_n w_x,  h = (1/16, 1/4, 3/8, 1/4, 1/16);  the centre tap weighs h(0)^2
 *                     w_c = exp(-|c_p - c_q|^2 / (sigma_i^2 (|c_p|^2 + 1e-30))),  sigma_i = sigma_color 2^-i
 *                     w_n = exp(-(1 - n_p . n_q) / sigma_normal)          (n: the G-buffer normal made unit length)
 *                     w_x = exp(-(n_p . (x_q - x_p))^2 / (sigma_plane^2 |x_q - x_p|^2 + 1e-30))
 *                     taps outside the image, not filterable, (FF_DENOISE_SAME_GEOMETRY) on another geometry or with
 *                     w_c w_n w_x < e^-30 weigh 0
 *   output          = c * albedo after the last pass (where it was divided); rgb8 = trunc(clamp(v * 255)) as ff_render's.
 * iterations = 0 copies every pixel through.  Scaling all radiance by k scales the output by k.
 * Non-finite input (the rule of all three image filters): a NaN or +-Inf radiance value may make its own pixel's output
 * non-finite in that call; every other output of the call stays finite.  Here every other pixel's output is bit for bit what
 * it is when the non-finite pixel's ids mark a miss: its neighbours skip it, as its exponent is not <= 30.  rgb8 (W*H*3 bytes) and
 * radiance_out (W*H*3 floats) may each be NULL; radiance_out may alias radiance_in.  Synchronous; FfStats keeps describing
 * the last frame. */
FF_API int ff_denoise(FfState* state, int width, int height, const FfDenoiseParams* dn,
                      const float* radiance_in, const float* position, const float* normal,
                      const float* albedo, const int32_t* ids, int inputs_on_device,
                      void* rgb8, int rgb8_on_device, float* radiance_out, int radiance_out_on_device);

/* ---- temporal denoiser (SVGF: Schied et al., HPG 2017) ---------------------------------------- */

/* Defaults: 5 passes, sigma_luminance 4, sigma_normal 0.1, sigma_plane 0.1, both flags, max_history 16, variance_history 4,
 * feedback after pass 0, reuse_normal 0.9, reuse_plane 0.01 (DESIGN.md section 8 row 6 records what was measured). */
FF_API void ff_temporal_params_init(FfTemporalParams* p);

/* Spatiotemporal variance-guided filter of a moving camera's 1-spp frames.  radiance_in is THIS frame's own samples (ff_render's
 * radiance, not a progressive mean); position, normal, albedo and ids are ff_gbuffer's for `camera` (albedo may be NULL without
 * FF_DENOISE_DEMODULATE_ALBEDO).  The state keeps the history from call to call: the previous camera, guides, colour, moments,
 * history length and per-geometry model matrices.  Filterable pixels and the demodulated colour c are as in ff_denoise; every
 * other pixel is copied through bit for bit and has length 0.  Per filterable pixel p at (x, y) of geometry g:
 *   x^, n^    x^ = Mprev_g inverse(Mcur_g) x_p, n^ = unit(inverse-transpose of that map n_p) (composed in double on the host;
 *             a geometry whose model matrix is bitwise unchanged keeps x^ = x_p, n^ = n_p exactly)
 *   project   q = inverse(ff_camera_ray_matrix(previous camera)) (x^, 1); fx = (q.x/q.w + 1)/2 * screen_w,
 *             fy = (1 - q.y/q.w)/2 * screen_h (the previous camera's m_screenWidth / m_screenHeight; the inverse of the
 *             primary ray's Px = x/screen_w*2-1, Py = 1-y/screen_h*2).  q.w <= 0: no history.  Camera bitwise the previous
 *             call's and g not moved: fx = x, fy = y exactly (the one tap is p itself, weight 1)
 *   taps      (floor(fx) + {0,1}, floor(fy) + {0,1}) with bilinear weights w_q; a tap counts when it lies in the previous image,
 *             has p's class there (same geometry, filterable), dot(n^, n_q) >= reuse_normal, |n^.(x_q - x^)| <= reuse_plane *
 *             |x^ - previous eye|, g's mesh was not replaced by ff_update_mesh since the previous call, w_q > 0 and its stored
 *             colour and moments are all finite
 *   history   W = sum w_q over the taps that count.  W >= 1e-3: h = sum w_q h_q / W for the colour history, both moments and the
 *             length; len = len_h + 1, alpha = 1 / min(len, max_history), acc = h + alpha (cur - h) for colour c and moments
 *             (l, l^2), l = 0.2126 r + 0.7152 g + 0.0722 b of c.  Otherwise len = 1, acc = cur.
 *   variance  len >= variance_history: var = max(0, mu2 - mu1^2) of the accumulated moments.  Otherwise the 7x7 average of the
 *             accumulated moments with weight w_n w_x [same class] (ff_denoise's w_n, w_x; exponent > 30 weighs 0), then
 *             var = max(0, mu2 - mu1^2) * 4 / len
 *   pass i    c'_p = sum w c_q / sum w, var'_p = sum w^2 var_q / (sum w)^2 over the 5x5 taps 2^i apart, w = h(dx) h(dy) w_l w_n w_x
 *             (h, w_n, w_x and the tap exclusions of ff_denoise, including the e^-30 cut-off on the product w_l w_n w_x),
 *             w_l = exp(-|l_p - l_q| / (sigma_luminance sqrt(g_p) + 1e-30)), g_p = sum k var_q / sum k over the 3x3
 *             neighbours that are taps of the pass (k = (1 2 1) x (1 2 1)), the centre always
 *   feedback  the next call's colour history is c after pass feedback_pass (-1: the accumulation before any pass); the
 *             moments history is always the unfiltered accumulation
 *   output    remodulated c after the last pass (the accumulation for iterations 0); rgb8 = trunc(clamp(v * 255)).
 * History is dropped by ff_temporal_reset, the first call, a change of width or height and ff_upload_scene; ff_update_mesh(g)
 * drops geometry g's only; ff_update_transforms moves it with its geometry.  The call leaves FfStats, the stored primary hits
 * and their key, the cull mask, ff_denoise's buffers and the progressive sum as they were.  Buffers as in ff_denoise
 * (radiance_out may alias radiance_in).  FF_ERR_NO_SCENE without a scene.  Synchronous.  Non-finite radiance: ff_denoise's rule
 * (its own pixel only); such a pixel's history is not reused, so the next call starts it afresh.
 * The pixel jitter (ff_set_pixel_jitter) is not seen here: the previous camera's matrix is the unjittered ff_camera_ray_matrix
 * and "at rest" means FfCamera bitwise equal, so a jittered sequence at rest accumulates each pixel's jittered samples like a
 * progressive mean. */
FF_API int ff_denoise_temporal(FfState* state, const FfCamera* camera, int width, int height, const FfTemporalParams* tp,
                               const float* radiance_in, const float* position, const float* normal, const float* albedo,
                               const int32_t* ids, int inputs_on_device,
                               void* rgb8, int rgb8_on_device, float* radiance_out, int radiance_out_on_device);

/* Drops the temporal history: the next ff_denoise_temporal call starts afresh. */
FF_API int ff_temporal_reset(FfState* state);

/* The last ff_denoise_temporal call's per-pixel motion (W*H*2 floats: fx - x, fy - y for every hit pixel whose point the
 * previous camera sees; 0 for misses and on the first call after a reset) and history length (W*H floats; 0 for pixels that
 * are not filterable).  Either may be NULL.  FF_ERR_INVALID_ARG when no call was made since the last reset. */
FF_API int ff_temporal_history(FfState* state, float* motion, float* length, int on_device);

/* ---- temporal anti-aliasing (TAA: Karis, SIGGRAPH 2014; Salvi, GDC 2016) ----------------------- */

/* Defaults: alpha_min 0.1, gamma 1, Catmull-Rom history with the clamp (flags 0). */
FF_API void ff_taa_params_init(FfTaaParams* p);

/* Temporal anti-aliasing resolve of frames rendered with a sub-pixel jitter (ff_set_pixel_jitter, ff_jitter_sequence).
 * radiance_in is this frame's image (raw, ff_denoise's or ff_denoise_temporal's output); position and ids are ff_gbuffer's for
 * `camera` and the same jitter.  The state keeps its own history (colour and length per pixel, the previous camera and the
 * per-geometry model matrices), separate from ff_denoise_temporal's.  P(M, X) is ff_denoise_temporal's projection:
 * q = inverse(M) (X, 1), P = ((q.x/q.w + 1)/2 * screen_w, (1 - q.y/q.w)/2 * screen_h) with that camera's m_screenWidth and
 * m_screenHeight.  M_cur, M_prev: the UNJITTERED ff_camera_ray_matrix of this call's camera and of the previous call's.
 * Per pixel p = (x, y):
 *   motion    hit of geometry g: x^ = Mprev_g inverse(Mcur_g) x_p (ff_denoise_temporal's rows, composed in double on the host),
 *             m = P(M_prev, x^) - P(M_cur, x_p), which cancels the jitter (P(M_cur, x_p) ~ (x + jx, y + jy)).  Miss: X = the
 *             kernel.cu:203 far point of the pixel's unjittered ray under M_cur, m = P(M_prev, X) - (x, y).  Camera bitwise
 *             the previous call's and g not moved (a miss: the camera alone): m = 0 exactly, nothing is projected
 *   history   looked up at h = (x, y) + m.  Valid when there is history, q.w > 0 (of P(M_prev, .)), 0 <= h.x <= W-1,
 *             0 <= h.y <= H-1 and g's mesh was not replaced by ff_update_mesh since the previous call.  Colour: the 4x4
 *             Catmull-Rom sum around floor(h), taps clamped into the image, t = h - floor(h) per axis, weights
 *             ((-t^3 + 2t^2 - t)/2, (3t^3 - 5t^2 + 2)/2, (-3t^3 + 4t^2 + t)/2, (t^3 - t^2)/2) for floor(h) - 1 .. floor(h) + 2,
 *             not renormalised (FF_TAA_BILINEAR: the 2x2 taps floor(h) + {0, 1} with weights (1 - t, t)).  A resampled colour
 *             that is not finite (a zero weight times a stored NaN included) is no history: invalid.  len_h: the
 *             history length at the nearest tap floor(h + 0.5).  m = 0 gives t = 0: exactly the pixel's own history
 *   clamp     (not with FF_TAA_NO_CLAMP) in YCoCg, Y = r/4 + g/2 + b/4, Co = r/2 - b/2, Cg = -r/4 + g/2 - b/4: over the 3x3
 *             neighbourhood of radiance_in (coordinates clamped at the borders) the mean mu, sigma = sqrt(max(0, E[c^2] - mu^2))
 *             and min / max per channel, over the samples whose r, g, b are all finite; the history is clamped per channel to [max(min, mu - gamma sigma),
 *             min(max, mu + gamma sigma)] and converted back (r = Y + Co - Cg, g = Y + Cg, b = Y - Co - Cg)
 *   blend     valid history: len = min(len_h + 1, 4096), alpha = max(alpha_min, 1 / len), o = h + alpha (c - h) in RGB.
 *             Otherwise len = 1 and o = c
 *   stored    o and len are the next call's history; rgb8 = trunc(clamp(o * 255)).
 * History is dropped by ff_taa_reset, the first call, a change of width or height and ff_upload_scene; ff_update_mesh(g)
 * drops geometry g's only; ff_update_transforms moves it with its geometry.  The call leaves FfStats, the stored primary hits
 * and their key, the cull mask, ff_denoise's buffers, the temporal denoiser's history and the progressive sum as they were.
 * Buffers as in ff_denoise (radiance_out may alias radiance_in).  FF_ERR_NO_SCENE without a scene; FF_ERR_INVALID_ARG for
 * alpha_min outside (0, 1], gamma <= 0 or NaN, unknown flags or a nonzero `reserved`.  Synchronous.  Non-finite radiance:
 * ff_denoise's rule (its own pixel only; the next call finds no valid history wherever the resampling reads it). */
FF_API int ff_taa(FfState* state, const FfCamera* camera, int width, int height, const FfTaaParams* p, const float* radiance_in,
                  const float* position, const int32_t* ids, int inputs_on_device, void* rgb8, int rgb8_on_device, float* radiance_out,
                  int radiance_out_on_device);

/* Drops the TAA history: the next ff_taa call starts afresh. */
FF_API int ff_taa_reset(FfState* state);

/* The last ff_taa call's per-pixel motion m (W*H*2 floats; 0 on the first call after a reset and where q.w <= 0) and history
 * length (W*H floats).  Either may be NULL.  FF_ERR_INVALID_ARG when no call was made since the last reset. */
FF_API int ff_taa_history(FfState* state, float* motion, float* length, int on_device);

/* ---- guided upsampling (joint bilateral upsampling: Kopf et al., SIGGRAPH 2007) ---------------- */

/* Defaults: sigma_normal 0.1, sigma_plane 0.1 (ff_denoise's), both FF_DENOISE_* flags, no jitter. */
FF_API void ff_upscale_params_init(FfUpscaleParams* p);

/* Turns a w x h float3 radiance image (lo_width x lo_height: raw, ff_denoise's or ff_denoise_temporal's output) plus its w x h
 * G-buffer plus a W x H G-buffer of the same view (width x height) into a W x H image: trace fewer pixels than are shown, and take
 * geometry edges and albedo textures from the cheap full-resolution G-buffer.  A pure image operation like ff_denoise: no scene is
 * read and none is needed.  Both G-buffers are ff_gbuffer's for the same camera pose with m_screenWidth x m_screenHeight = w x h and
 * W x H, under the pixel jitters lo_jitter = (jx, jy) and hi_jitter = (Jx, Jy) (ff_set_pixel_jitter).  The caller is responsible
 * for w/h = W/H and for the pose; only the sizes are checked.  Primary rays go through Px = (x + jx) / screen_w * 2 - 1, so high
 * pixel X looks along low image coordinate ((X + Jx) w) / W - jx; for an integer factor s and no jitter, low pixel i is high
 * pixel s i.  All arithmetic is float32, evaluated as written with the parentheses shown, no fused multiply-add; a dot product is
 * (x + y) + z.  Filterable is ff_denoise's: a hit whose bxdf is not emitter, mirror or glass.  Per high pixel P = (X, Y) with
 * guides x_P, n_P, a_P, ids_P, over low taps q with x_q, n_q, a_q, ids_q and radiance r_q (n: the G-buffer normal times
 * 1 / sqrt(n.n), 0 for a zero normal):
 *   1 taps    u = (((float)X + Jx) * (float)w) / (float)W - jx,  i0 = floor(u),  fu = u - i0;  v, j0, fv likewise from Y, Jy, h, H, jy.
 *             The 2x2 taps are (i0 + {0, 1}, j0 + {0, 1}) and the 4x4 taps (i0 - 1 .. i0 + 2, j0 - 1 .. j0 + 2), row by row, each
 *             coordinate clamped into the low image (a clamped tap keeps its weight, and counts as often as it is named).
 *             b_q = (1 - fu | fu) * (1 - fv | fv), the bilinear weight of a 2x2 tap
 *   mean      over the taps that count, c_0 the first of them: c = c_0 + (sum w_q (c_q - c_0)) / sum w_q, and c = c_0 for a single
 *             tap.  This is sum w c_q / sum w, and returns one tap, or a colour all taps share, bit for bit
 *   2 P filterable.  A tap counts when it is filterable, (FF_DENOISE_SAME_GEOMETRY) its geometry index is P's, r_q is finite
 *             in all three channels, (FF_DENOISE_DEMODULATE_ALBEDO) every channel with a_P > 0 has a_q > 0, b_q > 0, and
 *             e_q = a_n + a_x <= 30 (ff_denoise's cut-off),  a_n = (1 - n_P . n_q) / sigma_normal,
 *             a_x = (d * d) / ((sigma_plane * sigma_plane) * |x_q - x_P|^2 + 1e-30),  d = n_P . (x_q - x_P).
 *             w_q = b_q * exp(-e_q)  (= b_q w_n w_x of ff_denoise).  c_q = r_q / a_q in the channels with a_P > 0
 *             (DEMODULATE_ALBEDO), r_q elsewhere.  If a 2x2 tap counts: the mean over them.  Otherwise the mean over the 4x4 taps
 *             under the same rule without b_q (w_q = exp(-e_q)).  Otherwise step 4.  Output = c * a_P in the divided channels
 *   3 P not filterable (a miss, an emitter, a mirror, glass: there is no high-resolution radiance to copy through).  A tap counts
 *             when its geometry index and bxdf type equal P's (a miss matches a miss), r_q is finite and b_q > 0;  w_q = b_q,
 *             c_q = r_q.  If none counts: the 4x4 taps with w_q = 1.  Otherwise step 4
 *   4 fallback  r of the low pixel (floor(u + 0.5), floor(v + 0.5)), clamped into the image, as it is.
 * rgb8 = trunc(clamp(v * 255)) as ff_render's.  Equal sizes, no jitter and no DEMODULATE_ALBEDO return a finite input image bit
 * for bit.  Non-finite input: a NaN or +-Inf in radiance_lo never counts as a tap, so it reaches high pixels through step 4 only;
 * every other output stays finite.  rgb8 (W*H*3 bytes) and radiance_out (W*H*3 floats) may each be NULL and must not overlap an
 * input.  inputs_on_device covers all nine input images.  Host buffers are staged through the state's image staging buffer; the
 * call keeps nothing else in the state and leaves FfStats, the stored primary hits and their key, every filter's history and the
 * progressive sum as they were.  Synchronous, on the state's stream.  FF_ERR_INVALID_ARG, naming the field, before any device
 * work for: a NULL state, params, radiance_lo, position, normal or ids of either grid; a NULL albedo of either grid with
 * DEMODULATE_ALBEDO (without it albedo is not read); sizes outside 1 <= lo <= hi <= 8 lo per axis or hi > 65535; a sigma that is
 * not positive and finite; a jitter outside [0, 1); unknown flags; a nonzero `reserved`.
 * Not offered: upscaling ff_denoise_temporal's history, non-uniform or foveated sampling, a multi-GPU twin.  (The temporal
 * upsampler is ff_taa_upscale.) */
FF_API int ff_upscale(FfState* state, const FfUpscaleParams* p,
                      int lo_width, int lo_height, const float* radiance_lo, const float* position_lo, const float* normal_lo,
                      const float* albedo_lo, const int32_t* ids_lo,
                      int width, int height, const float* position, const float* normal, const float* albedo, const int32_t* ids,
                      int inputs_on_device, void* rgb8, int rgb8_on_device, float* radiance_out, int radiance_out_on_device);

/* Host-only twin (no GPU, no state, host pointers), compiled from the same inline per-pixel function the kernel uses: the same
 * image arguments, the same checks.  It differs from ff_upscale in the last bits of exp alone. */
FF_API int ff_upscale_host(const FfUpscaleParams* p,
                           int lo_width, int lo_height, const float* radiance_lo, const float* position_lo, const float* normal_lo,
                           const float* albedo_lo, const int32_t* ids_lo,
                           int width, int height, const float* position, const float* normal, const float* albedo, const int32_t* ids,
                           unsigned char* rgb8, float* radiance_out);

/* ---- temporal upsampling (ff_taa writing a larger image than it reads) --------------------------- */

/* Defaults: alpha_min 0.1, gamma 1 (ff_taa's), lo_jitter 0 0, Catmull-Rom history with the clamp (flags 0). */
FF_API void ff_taa_upscale_params_init(FfTaaUpscaleParams* p);

/* Accumulates jittered w x h frames (lo_width x lo_height) into a W x H image (width x height): a viewer at rest that cycles
 * ff_jitter_sequence over low-resolution frames ends up with the full-resolution picture - shadow edges, reflections and every
 * texture included - where ff_upscale alone can only sharpen one low frame along the G-buffer's edges.  `camera` is the pose
 * with m_screenWidth x m_screenHeight = W x H.  position and ids are ff_gbuffer's at W x H under jitter 0 0.  radiance_lo
 * (w x h float3) is a frame of the same pose with the screen set to w x h, rendered under ff_set_pixel_jitter(lo_jitter); it
 * must be an FF_PIXEL_CORNER frame, because FF_PIXEL_BOX frames ignore the state's jitter.  ids_lo is ff_gbuffer's at w x h under
 * that jitter.  The caller is responsible for the pose; only the sizes are checked.  The state keeps a history of its own (colour
 * and length per high pixel, the previous camera and the per-geometry model matrices), separate from ff_taa's and
 * ff_denoise_temporal's.  All arithmetic is float32, evaluated as parenthesised, no fused multiply-add.  P(M, X), M_cur, M_prev
 * as in ff_taa.  Per high pixel P = (X, Y) with (g_P, k_P) = its geometry index and bxdf type, (jx, jy) = lo_jitter:
 *   1 motion  hit of geometry g: x^ = Mprev_g inverse(Mcur_g) x_p (ff_denoise_temporal's rows, composed in double on the host),
 *             m = P(M_prev, x^) - P(M_cur, x_p).  Miss: X = the kernel.cu:203 far point of the pixel's unjittered ray under M_cur,
 *             m = P(M_prev, X) - (x, y).  Camera bitwise the previous call's and g not moved (a miss: the camera alone): m = 0
 *             exactly, nothing is projected
 *     history looked up at h = (X, Y) + m in the W x H history.  Valid when there is history, q.w > 0 (of P(M_prev, .)),
 *             0 <= h.x <= W-1, 0 <= h.y <= H-1 and g's mesh was not replaced by ff_update_mesh since the previous call.  Colour: the
 *             4x4 Catmull-Rom sum around floor(h), taps clamped into the image, t = h - floor(h) per axis, weights
 *             ((-t^3 + 2t^2 - t)/2, (3t^3 - 5t^2 + 2)/2, (-3t^3 + 4t^2 + t)/2, (t^3 - t^2)/2) for floor(h) - 1 .. floor(h) + 2,
 *             not renormalised (FF_TAA_BILINEAR: the 2x2 taps floor(h) + {0, 1} with weights (1 - t, t)).  A resampled colour
 *             that is not finite (a zero weight times a stored NaN included) is no history: invalid.  len_h: the history
 *             length at the nearest tap floor(h + 0.5).  m = 0 gives t = 0: exactly the pixel's own history
 *   2 look    u = ((float)X * (float)w) / (float)W - jx, v likewise from Y, h, H, jy: where P's ray crosses the low frame.  The
 *             nearest low sample q* = (i*, j*), i* = clamp(floor(u + 0.5), 0, w-1), j* likewise; dx = u - (float)i*, dy likewise
 *   3 confidence  k = max(0, 1 - |dx| * sx) * max(0, 1 - |dy| * sy), sx = (float)W / (float)w, sy = (float)H / (float)h, each
 *             formed once: a tent one high pixel wide about the point the low ray went through.  k = 0 when (geometry, bxdf) of
 *             ids_lo[q*] differ from (g_P, k_P) (a miss matches a miss), and when radiance_lo[q*] is not finite in all three
 *             channels.  The current sample is c = radiance_lo[q*]
 *   4 spatial estimate c_up (used only in step 6's last case): ff_upscale's step 3 applied to every P, then its step 4.  The mean
 *             (ff_upscale's "mean") over the 2x2 taps about (floor u, floor v) whose bilinear weight is > 0, whose (geometry,
 *             bxdf) equal P's and whose radiance is finite, weights b_q; else over the 4x4 taps under the same rule with weight 1;
 *             else radiance_lo[q*] as it is
 *   5 clamp   (not with FF_TAA_NO_CLAMP, not without valid history, not when k = 0) ff_taa's YCoCg box (mean +- gamma sigma, cut by
 *             min / max, over the finite samples only) over the 3x3 low pixels about q*, coordinates clamped into the low image.
 *             With no finite sample nothing is clamped
 *   6 blend   with valid history, wsum = min(len_h + k, 4096).
 *             wsum > 0 and k > 0: alpha = max(alpha_min * k, k / wsum), o = h' + alpha (c - h') with h' the clamped history,
 *                                 len = wsum
 *             wsum > 0 and k = 0: o = h exactly (the unclamped history, no arithmetic on c), len = len_h
 *             no valid history and k > 0: o = c, len = k
 *             every other case:   o = c_up, len = 0
 *   stored    {o, len} is the next call's history, m the motion; rgb8 = trunc(clamp(o * 255)).
 * Consequences.  Equal sizes and lo_jitter 0 0 give k = 1 on finite input, and the call is ff_taa's, bit for bit.  With a
 * factor 2 and jitters in {0, 1/2}^2, u, dx and k are exact and k is 0 or 1: at rest, a cycle of the four jitters hands every high
 * pixel, exactly once, the low sample whose ray is its own; under FF_TAA_NO_CLAMP the accumulated image is then the
 * full-resolution image's samples, bit for bit, with every length 1, and a second cycle of the same frames leaves the bits alone
 * and makes every length 2.  (From the second frame on, a pixel's first sample c meets the c_up the frame before stored with
 * length 0, at alpha = 1: o = h + (c - h), which is c whenever c - h is exact, as it is for h / 2 <= c <= 2 h.)  A non-finite low
 * pixel never enters a history as c: it can reach an output only through c_up's last fallback.
 * History is dropped by ff_taa_upscale_reset, the first call, a change of either size and ff_upload_scene; ff_update_mesh(g)
 * drops geometry g's only; ff_update_transforms moves it with its geometry.  The call leaves FfStats, the stored primary hits
 * and their key, the other histories and the progressive sum as they were.  rgb8 (W*H*3 bytes) and radiance_out (W*H*3 floats)
 * may each be NULL and must not overlap an input.  inputs_on_device covers all four input images.  Synchronous, on the state's
 * stream.  FF_ERR_NO_SCENE without a scene.  FF_ERR_INVALID_ARG, naming the field, before any device work and with the history
 * untouched, for: a NULL state, params, camera or input; sizes outside 1 <= lo <= hi <= 8 lo per axis or hi > 65535; alpha_min
 * outside (0, 1]; gamma <= 0 or not finite; a jitter outside [0, 1) or not finite; unknown flags; a nonzero `reserved`; a singular
 * ray matrix.
 * Not offered: guides other than ids (normals, albedo demodulation), ff_denoise_temporal's moments at high resolution, a jittered
 * high G-buffer, a multi-GPU twin. */
FF_API int ff_taa_upscale(FfState* state, const FfCamera* camera, const FfTaaUpscaleParams* p,
                          int lo_width, int lo_height, const float* radiance_lo, const int32_t* ids_lo,
                          int width, int height, const float* position, const int32_t* ids, int inputs_on_device,
                          void* rgb8, int rgb8_on_device, float* radiance_out, int radiance_out_on_device);

/* Drops the temporal upsampler's history: the next ff_taa_upscale call starts afresh. */
FF_API int ff_taa_upscale_reset(FfState* state);

/* The last ff_taa_upscale call's per-pixel motion m (W*H*2 floats; 0 on the first call after a reset and where q.w <= 0) and
 * history length (W*H floats: the confidence accumulated so far).  Either may be NULL.  FF_ERR_INVALID_ARG when no call was made
 * since the last reset. */
FF_API int ff_taa_upscale_history(FfState* state, float* motion, float* length, int on_device);

/* ---- motion blur (a reconstruction filter on stored motion: McGuire et al., I3D 2012) ----------- */

/* Defaults: shutter 0.5, max_radius 16, samples 15, depth_extent 0.1, flags 0. */
FF_API void ff_motion_blur_params_init(FfMotionBlurParams* p);

/* Blurs a W x H float3 radiance image along the per-pixel screen motion: a 1-spp frame is an instant, this spreads it over the time
 * the shutter is open.  It sits after ff_taa / ff_taa_upscale and before ff_display.  A pure image operation like ff_denoise and
 * ff_display: no scene is read, none is needed, and no history is kept.  motion is W*H*2 floats exactly as ff_taa_history,
 * ff_temporal_history and ff_taa_upscale_history write it (previous position minus current position, in pixels); depth is W*H
 * floats, ff_gbuffer's depth plane (m_t; a miss is 0).  All arithmetic is float32, evaluated as written with the parentheses shown,
 * no fused multiply-add, IEEE sqrt and division; exp and pow appear nowhere, so ff_motion_blur, ff_motion_blur_host and a float32
 * restatement agree bit for bit.  clamp(v) = 0 for v < 0, 1 for v > 1, else v.  With k = max_radius, S = samples:
 *   1 half-spread  per pixel, hs = 0.5f * shutter (formed once), v = (m.x * hs, m.y * hs).  If either component of v is not finite,
 *                v = (0, 0).  l = sqrt(v.x * v.x + v.y * v.y).  If l > (float)k: s = (float)k / l, v = (v.x * s, v.y * s) and
 *                l = sqrt(v.x * v.x + v.y * v.y) again, from the scaled components.  z = depth if it is finite and > 0, else
 *                FLT_MAX (a miss is behind everything).  The pixel keeps {v.x, v.y, l, z}
 *   2 tile max   tiles are k x k pixels from the top-left corner, partial at the right and bottom edges.  T(tile) = the kept {v, l}
 *                of the tile's pixel with the largest v.x * v.x + v.y * v.y (of the kept v); among equals the first in row-major order
 *   3 neighbour max  N(tile) = the T with the largest v.x * v.x + v.y * v.y over the 3x3 tiles around it that exist; among equals the
 *                first in row-major order of the tiles
 *   4 gather     pixel X = (x, y) with (vn, ln) = N(tile (x / k, y / k)) and its own kept lX, zX and colour cX.  If ln <= 0.5, or cX
 *                is not finite in all three channels, the output is cX bit for bit.  Otherwise, in uint32 arithmetic,
 *                h = (x * 0x9E3779B1) ^ (y * 0x85EBCA77);  h ^= h >> 15;  h *= 0x2C1B3C6D;  h ^= h >> 12;
 *                j = (float)(h >> 8) * 2^-24 - 0.5.  For i = 0 .. S-1 in order:
 *                  t = ((((float)i + j) + 1) / (float)(S + 1)) * 2 - 1,
 *                  dx = (int)floor(vn.x * t + 0.5), dy = (int)floor(vn.y * t + 0.5), Y = X + (dx, dy).
 *                The tap is skipped when dx = dy = 0, when Y is outside the image and when cY is not finite in all three channels.
 *                Otherwise, with Y's kept lY, zY:  d = sqrt((float)(dx * dx + dy * dy)),
 *                  soft(a, b) = clamp(1 - (a - b) / depth_extent);  f = soft(zY, zX) (1 when Y is nearer),  b = soft(zX, zY),
 *                  cone(d, l) = clamp(1 - d / l) for l > 0, else 0,
 *                  cyl(d, l)  = 1 - ((u * u) * (3 - (2 * u))),  u = clamp((d - 0.95f * l) / (1.05f * l - 0.95f * l)), for l > 0, else 0,
 *                  a = (f * cone(d, lY) + b * cone(d, lX)) + (cyl(d, lY) * cyl(d, lX)) * 2,
 *                  s_c = s_c + a * (cY_c - cX_c) per channel c,  A = A + a   (s_c and A start at 0).
 *                After the taps  w0 = 1 / max(lX, 0.5)  and per channel  out_c = cX_c + s_c / (w0 + A)  where s_c != 0, and
 *                out_c = cX_c itself where s_c = 0 (so a -0 stays -0): ff_upscale's "mean" form of (w0 cX + sum a cY) / (w0 + sum a).
 *                When every tap has the centre's colour, or none counts, cX comes back bit for bit
 *   5 rgb8 = trunc(clamp(out * 255)), the rule of every rgb8 output here.
 * Consequences.  Motion 0 everywhere, or shutter 0, returns the input bit for bit, NaN and Inf pixels included; so does every pixel
 * whose 3x3 tile neighbourhood holds no motion with l > 0.5.  Non-finite radiance follows the project's rule: such a pixel may spoil
 * only itself - it is copied through and never counts as a tap; non-finite motion is no motion and non-finite depth is a miss.
 * rgb8 (W*H*3 bytes) and radiance_out (W*H*3 floats) may each be NULL.  Neither may overlap an input (the gather reads neighbours;
 * radiance_out == radiance_in is refused), and the two outputs may not overlap each other.  inputs_on_device covers all three
 * input images.  Width and height are 1 .. 65535.
 * Synchronous, on the state's stream; host buffers are staged.  The call leaves FfStats, the stored primary hits and their key, every
 * filter's history, the display exposure and the progressive sum as they were; its own state is a work buffer (allocated on first
 * use, regrown for a larger size, freed by ff_destroy).  FF_ERR_INVALID_ARG, naming the field, before any device work for: a NULL
 * state, params, radiance_in, motion or depth; a bad size; shutter outside 0 .. 4, max_radius or samples outside 1 .. 64,
 * depth_extent not positive (every float must be finite); nonzero flags or reserved; an output that overlaps an input or
 * the other output.
 * Not offered: time-sampled blur inside the path kernels, motion of deforming meshes (the stored motion is rigid), McGuire's
 * diagonal-tile rule, per-tile sample counts, a multi-GPU twin, blurring ff_denoise_temporal's moments. */
FF_API int ff_motion_blur(FfState* state, int width, int height, const FfMotionBlurParams* p,
                          const float* radiance_in, const float* motion, const float* depth, int inputs_on_device,
                          void* rgb8, int rgb8_on_device, float* radiance_out, int radiance_out_on_device);

/* Host-only twin (no GPU, no state, host pointers), compiled from the same inline per-pixel functions the kernels use: the same
 * image arguments, the same checks, the same bits. */
FF_API int ff_motion_blur_host(int width, int height, const FfMotionBlurParams* p, const float* radiance_in, const float* motion,
                               const float* depth, unsigned char* rgb8, float* radiance_out);

/* ---- depth of field (a gather filter on the G-buffer: the thin lens as a post filter) ------------- */

/* Defaults: focus_distance 1, coc_scale 0 (no blur), max_radius 16, grid 4, depth_extent 0.1, flags 0. */
FF_API void ff_dof_params_init(FfDofParams* p);

/* Makes the filter agree with the in-path thin lens of ff_set_camera_sampling: sets p->focus_distance = cs->focus_distance and
 * p->coc_scale = (float)(lens_radius * 0.5 * m_screenHeight / tan(radians(m_fov) / 2)), evaluated in double and rounded once, and
 * leaves the other fields alone.  m_fov is the vertical field of view and pixels are square, so a lens of radius R focused at z_f
 * spreads a point at axial depth z over a circle of R (H / 2) / tan(fov / 2) |1 / z_f - 1 / z| pixels' radius.  A setting with
 * lens_radius 0 gives coc_scale 0: the filter copies.  FF_ERR_INVALID_ARG for a NULL pointer, for each of ff_set_camera_sampling's
 * own checks, and for an m_fov outside (0, 180) or an m_screenHeight that is not positive (every float must be finite). */
FF_API int ff_dof_params_from_camera(const FfCamera* camera, const FfCameraSampling* cs, FfDofParams* p);

/* Spreads every pixel of a W x H float3 radiance image over its circle of confusion: defocus as a post filter on a PINHOLE frame, so
 * that a 1-spp frame can be denoised, resolved and upsampled against the pinhole G-buffer first.  It sits where ff_motion_blur sits:
 * after ff_taa / ff_taa_upscale, before or after ff_motion_blur, before ff_display.  A pure image operation like ff_denoise and
 * ff_display: no scene is read, none is needed, and no history is kept.  position is W*H*3 floats and depth W*H floats, ff_gbuffer's
 * planes of the same pose (a miss: depth 0).  Of camera only m_position and m_forward are read, as the caller's floats, not
 * renormalised (the thin lens's precedent).  All arithmetic is float32, evaluated as written with the parentheses shown, no fused
 * multiply-add, IEEE sqrt and division; exp, pow and trigonometry appear nowhere, so ff_depth_of_field, ff_depth_of_field_host and a
 * float32 restatement agree bit for bit.  clamp(v) = 0 for v < 0, 1 for v > 1, else v.  With k = max_radius, g = grid, f^ = m_forward:
 *   1 radius     per pixel, e = position - m_position per component, z = (e.x * f^.x + e.y * f^.y) + e.z * f^.z.  The pixel is a HIT
 *                when depth is finite and > 0 and z is finite and > 1e-6f.  iz = 1 / z for a hit, else 0 (a miss lies at infinity).
 *                fi = 1 / focus_distance (formed once).  l = coc_scale * fabs(fi - iz), and l > (float)k becomes (float)k.  The
 *                pixel keeps {l, zk}, zk = z for a hit and FLT_MAX otherwise.  (l is finite and >= 0.)
 *   2 tile max   tiles are k x k pixels from the top-left corner, partial at the right and bottom edges.  T(tile) = the largest kept l
 *                in the tile
 *   3 neighbour max  N(tile) = the largest T over the 3x3 tiles around it that exist (a maximum of finite numbers >= 0: no order,
 *                no tie rule)
 *   4 gather     pixel X = (x, y) with n = N(tile (x / k, y / k)) and its own kept lX, zX and colour cX.  If n <= 0.5, or cX is not
 *                finite in all three channels, the output is cX bit for bit.  Otherwise, in uint32 arithmetic (ff_motion_blur's hash),
 *                h = (x * 0x9E3779B1) ^ (y * 0x85EBCA77);  h ^= h >> 15;  h *= 0x2C1B3C6D;  h ^= h >> 12;
 *                jx = (float)(h >> 8) * 2^-24 - 0.5,  jy = (float)((h * 0x9E3779B1) >> 8) * 2^-24 - 0.5.
 *                For b = -g .. g (outer) and a = -g .. g (inner), in that order, over the points with a * a + b * b <= g * g (integers):
 *                  dx = (int)floor(n * (((float)a + jx) / (float)g) + 0.5),  dy = (int)floor(n * (((float)b + jy) / (float)g) + 0.5),
 *                  Y = X + (dx, dy).
 *                The tap is skipped when dx = dy = 0, when Y is outside the image and when cY is not finite in all three channels.
 *                Otherwise, with Y's kept lY, zY:  d = sqrt((float)(dx * dx + dy * dy)),
 *                  f = clamp(1 - (zY - zX) / depth_extent)      (1 when Y is nearer or level, 0 when it is farther by depth_extent),
 *                  cov(d, l) = clamp((l - d) + 0.5),  m = lY < lX ? lY : lX,
 *                  inten(l) = 1 / (q * q),  q = l > 0.5 ? l : 0.5,
 *                  w = (f * cov(d, lY) + (1 - f) * cov(d, m)) * inten(lY),
 *                  s_c = s_c + w * (cY_c - cX_c) per channel c,  A = A + w   (s_c and A start at 0).
 *                A tap in front spreads as far as its own circle; a tap behind reaches X only as far as X itself is blurred, so a
 *                sharp foreground keeps its edge against a blurred background; every tap carries energy inversely to its circle's
 *                area.  After the taps  w0 = inten(lX)  and per channel  out_c = cX_c + s_c / (w0 + A)  where s_c != 0, and
 *                out_c = cX_c itself where s_c = 0 (so a -0 stays -0): ff_motion_blur's mean form.  When every tap has the centre's
 *                colour, or none counts, cX comes back bit for bit
 *   5 rgb8 = trunc(clamp(out * 255)), the rule of every rgb8 output here.
 * Consequences.  coc_scale 0 returns the input bit for bit, NaN and Inf pixels included; so does every pixel whose 3x3 tile
 * neighbourhood holds no l > 0.5 (everything in focus: the whole image).  Non-finite radiance follows the project's rule: such a
 * pixel may spoil only itself - it is copied through and never counts as a tap; non-finite position or depth is a miss.
 * focus_distance must be so large that 1 / focus_distance is finite (above about 2.94e-39): otherwise step 1 would form 0 * Inf
 * under coc_scale 0.
 * rgb8 (W*H*3 bytes) and radiance_out (W*H*3 floats) may each be NULL.  Neither may overlap an input (the gather reads neighbours;
 * radiance_out == radiance_in is refused), and the two outputs may not overlap each other.  inputs_on_device covers all three
 * input images.  Width and height are 1 .. 65535.
 * Synchronous, on the state's stream; host buffers are staged.  The call leaves FfStats, the stored primary hits and their key, every
 * filter's history, the display exposure and the progressive sum as they were; its own state is a work buffer (allocated on first
 * use, regrown for a larger size, freed by ff_destroy).  FF_ERR_INVALID_ARG, naming the field, before any device work for: a NULL
 * state, camera, params, radiance_in, position or depth; a bad size; focus_distance not > 0, coc_scale < 0, max_radius outside
 * 1 .. 64, grid outside 1 .. 8, depth_extent not > 0 (every float must be finite); nonzero flags or reserved; a non-finite
 * m_position or m_forward; an output that overlaps an input or the other output.
 * Not offered: a separate near-field layer with background reconstruction behind a blurred foreground, polygonal or anamorphic
 * apertures, bokeh highlights, an autofocus call, a multi-GPU twin, filtering ff_denoise_temporal's moments. */
FF_API int ff_depth_of_field(FfState* state, const FfCamera* camera, int width, int height, const FfDofParams* p,
                             const float* radiance_in, const float* position, const float* depth, int inputs_on_device,
                             void* rgb8, int rgb8_on_device, float* radiance_out, int radiance_out_on_device);

/* Host-only twin (no GPU, no state, host pointers), compiled from the same inline per-pixel functions the kernels use: the same
 * image arguments, the same checks, the same bits. */
FF_API int ff_depth_of_field_host(const FfCamera* camera, int width, int height, const FfDofParams* p,
                                  const float* radiance_in, const float* position, const float* depth,
                                  unsigned char* rgb8, float* radiance_out);

/* ---- firefly clamp (a G-buffer-guided outlier clamp on the raw frame) ----------------------------- */

/* Defaults: radius 1, rank 2, min_neighbours 3, threshold 2, floor 0, FF_DESPECKLE_DEMODULATE_ALBEDO. */
FF_API void ff_despeckle_params_init(FfDespeckleParams* p);

/* Pulls the fireflies of a W x H float3 radiance image down: every pixel whose illumination is far above that of its neighbours on
 * the same surface is scaled to a multiple of their rank-th largest.  A 1-spp frame with next-event estimation carries isolated
 * pixels orders of magnitude brighter than their surroundings (an emitter hit through a glossy lobe, a sun texel on a low-pdf
 * path), and every filter downstream is linear in radiance or weighs its taps by colour distance: this call sits after ff_render /
 * ff_gbuffer and BEFORE ff_denoise, ff_denoise_temporal, ff_taa or ff_taa_upscale.  A pure image operation like ff_denoise and
 * ff_display: no scene is read, none is needed, and no history is kept.  albedo is W*H*3 floats and ids W*H*3 int32, ff_gbuffer's
 * planes of the frame's pose ({geometry, triangle, bxdf} per pixel; a miss has geometry -1).  All arithmetic is float32, evaluated
 * as written with the parentheses shown, no fused multiply-add, IEEE division; exp, pow and sqrt appear nowhere, and the filter is a
 * selection, not a sum, so ff_despeckle, ff_despeckle_host and a float32 restatement agree bit for bit whatever the order.  With
 * r = radius:
 *   1 measure    per pixel, g = ids[3p] and b = ids[3p+2].  With FF_DESPECKLE_DEMODULATE_ALBEDO, per channel k, c_k = radiance_k /
 *                albedo_k where albedo_k > 0 and c_k = radiance_k otherwise (ff_denoise's division); without the flag c = radiance
 *                and albedo is not read (it may be NULL).  l = (0.2126f * c.r + 0.7152f * c.g) + 0.0722f * c.b.  The pixel COUNTS
 *                when g >= 0, b != FF_BXDF_EMITTER, its three radiance channels are finite, l is finite and, under the flag, none
 *                of its three albedo channels is NaN
 *   2 yardstick  for a counting pixel X the neighbours are the pixels Y != X of the (2r+1)^2 window around X that lie in the image,
 *                count, and have g_Y == g_X.  n = their number, m = the rank-th largest of their l (a value: ties need no rule)
 *   3 clamp      limit = threshold * m, and a limit that is not above floor becomes floor (a limit below floor, and a zero of
 *                either sign under floor 0).  X is clamped when it counts, n >= min_neighbours, l_X > 0 and l_X > limit.  For a
 *                clamped X: s = limit / l_X and out_k = radiance_k * s per channel - the same factor scales the raw and the
 *                demodulated colour, so nothing is multiplied back.  The quotient, the products and a measure of them are each
 *                rounded and may each round up, so the result is measured: l' = step 1's l of out under X's albedo, and while
 *                l' > limit and s > 0, s becomes the float32 next below it (its bit pattern minus 1) and out and l' are formed
 *                again; a 65th such step sets s = 0 instead.  (One or two steps in practice.  More than 64 need radiance of
 *                mixed sign whose channels cancel in l.)  Every other pixel's output is its input bit for bit: misses, emitters,
 *                non-finite pixels, pixels with too few neighbours, pixels at or below their limit
 *   4 rgb8 = trunc(clamp(out * 255)), the rule of every rgb8 output here; *out_clamped = the number of clamped pixels.
 * Consequences.  A constant image (and, under the flag, a constant albedo) returns the input bit for bit (threshold >= 1).  A threshold so large that limit overflows returns
 * the input bit for bit (nothing is above +Inf).  With floor 0, scaling all radiance by a power of two scales the output by it
 * exactly and leaves the count as it is (short of overflow and subnormals).  A clamped pixel, measured again as step 1 measures, is
 * at or below its limit, in float32 and without allowance; no pixel's l grows (s < 1) and no channel changes its sign; a -0 channel of an unclamped pixel stays -0.  Non-finite input follows the project's rule for every image filter: such a
 * pixel may spoil only itself - it is copied through and is nobody's neighbour, as if its ids marked a miss.
 * Bias.  The filter REMOVES energy and puts it nowhere else: the mean of the output is below the mean of the input, and the
 * expectation of a despeckled frame is not the converged image.  It is meant for frames with next-event estimation, whose
 * fireflies are rare events on top of a well-sampled direct term.  The plain path mode at 1 spp carries nearly all of its energy in
 * isolated pixels (the paths that happened to reach an emitter): there the clamp removes the image.  floor is the caller's guard:
 * no pixel is pulled below it.  tools/despeckle_bench.py reports the share of energy removed beside the error (DESIGN.md section 8
 * row 18).
 * rgb8 (W*H*3 bytes) and radiance_out (W*H*3 floats) may each be NULL.  Neither may overlap an input (the window reads neighbours;
 * radiance_out == radiance_in is refused), and the two outputs may not overlap each other.  inputs_on_device covers all three input
 * images.  out_clamped is a host pointer and may be NULL.  Width and height are 1 .. 65535.
 * Synchronous, on the state's stream; host buffers are staged.  The call leaves FfStats, the stored primary hits and their key, every
 * filter's history, the display exposure and the progressive sum as they were; its own state is a work buffer (allocated on first
 * use, regrown for a larger size, freed by ff_destroy).  FF_ERR_INVALID_ARG, naming the field, before any device work for: a NULL
 * state, params, radiance_in or ids; a NULL albedo under the flag; a bad size; radius outside 1 .. 3, rank outside 1 .. 4,
 * min_neighbours outside rank .. (2r+1)^2 - 1 (so min_neighbours < rank is refused), threshold < 1, floor < 0 (every float must be
 * finite); unknown flags or a nonzero reserved; an output that overlaps an input or the other output.
 * Not offered: a temporal test against ff_denoise_temporal's moments, redistribution of the removed energy, a multi-GPU twin. */
FF_API int ff_despeckle(FfState* state, int width, int height, const FfDespeckleParams* p,
                        const float* radiance_in, const float* albedo, const int32_t* ids, int inputs_on_device,
                        void* rgb8, int rgb8_on_device, float* radiance_out, int radiance_out_on_device,
                        uint32_t* out_clamped);

/* Host-only twin (no GPU, no state, host pointers), compiled from the same inline per-pixel functions the kernel uses: the same
 * image arguments, the same checks, the same bits and the same count. */
FF_API int ff_despeckle_host(int width, int height, const FfDespeckleParams* p, const float* radiance_in, const float* albedo,
                             const int32_t* ids, unsigned char* rgb8, float* radiance_out, uint32_t* out_clamped);

/* ---- sharpening (contrast-adaptive, after the temporal resolve) ------------------------------------ */

/* Defaults: strength 0.5, FF_SHARPEN_NOISE_AWARE. */
FF_API void ff_sharpen_params_init(FfSharpenParams* p);

/* Sharpens a W x H float3 radiance image: a 5-tap contrast-adaptive filter (the cross B above, D left, F right, H below the pixel
 * E) whose negative lobe is limited per pixel so that the result stays within what the taps span - it cannot ring - and which is
 * evaluated in the range-compressed domain c / (1 + max c), so that an HDR highlight throws no dark halo.  ff_taa resamples and
 * blends its history, ff_taa_upscale spreads one low sample over several pixels and ff_denoise low-passes what its edge-stopping
 * lets through: this call sits directly after ff_taa / ff_taa_upscale (after ff_denoise in a purely spatial pipeline) and BEFORE
 * ff_motion_blur, ff_depth_of_field and ff_display (after AMD FidelityFX CAS and the limited "robust" sharpening of FSR, by
 * T. Lottes).  A pure image operation like ff_display: no scene, no G-buffer, no history.  All arithmetic is float32, evaluated as
 * written with the parentheses shown, no fused multiply-add, IEEE division; exp, pow and sqrt appear nowhere, so ff_sharpen,
 * ff_sharpen_host and a float32 restatement agree bit for bit.  min(a, b) is b < a ? b : a and max(a, b) is a < b ? b : a, nested
 * left to right in the order written.  LIMIT = 0.1875f, CAP = 0.99999988f (1 - 2^-23), MAXC = 8388608.0f (2^23).
 *   1 compress   a pixel is USABLE when its three channels are finite and >= 0 (a -0 passes) and m = max(max(c_r, c_g), c_b) <=
 *                MAXC.  For a usable pixel t_k = (c_k / (1.0f + m)) + 0.0f per channel: the + 0.0f turns -0 into +0, so no min or
 *                max below ever chooses between zeros of different sign (and 1.0f + m is 1 whichever zero m is); m <= 2^23 keeps
 *                1 + m exact and every t_k <= CAP.  L = (0.2126f * t_r + 0.7152f * t_g) + 0.0722f * t_b
 *   2 taps       for E at (x, y): B = (x, y-1), D = (x-1, y), F = (x+1, y), H = (x, y+1); a tap outside the image is E itself.
 *                If E or any tap inside the image is not usable, the output pixel is the input pixel bit for bit.  If all four
 *                taps (after that substitution) have E's three t exactly, the output is the input bit for bit as well: a constant
 *                neighbourhood, the 1 x 1 image.  It is the COMPRESSED values that are compared
 *   3 lobe       per channel k, of the taps' t_k: mn = min(min(b, d), min(f, h)), mx = max(max(b, d), max(f, h)).  lobe_k = -LIMIT
 *                where mx == 0 (a channel that is black all round limits nothing); otherwise
 *                lobe_k = max(-(mn / (4.0f * mx)), (1.0f - mx) / ((4.0f * mn) - 4.0f)).  (mn <= mx <= CAP: the divisors are never
 *                0, both terms are <= -0, and the second is below 0.)  Then
 *                lobe = max(-LIMIT, min(max(max(lobe_r, lobe_g), lobe_b), 0.0f)) * strength.  A channel with mn = 0 < mx gives
 *                lobe_k = -0 and, being the largest, lobe = -0: a tap that is black in a channel in which another is not leaves
 *                no room below it, and step 5 copies the pixel through
 *   4 noise      (only under FF_SHARPEN_NOISE_AWARE, on step 3's lobe, strength included)
 *                n = (0.25f * (((L_B + L_D) + L_F) + L_H)) - L_E; range = max - min of the five L, each nested in the order E, B,
 *                D, F, H.  Where range > 0: a = min(fabs(n) / range, 1.0f) and lobe = lobe * (1.0f - 0.5f * a).  A lone outlier
 *                (a = 1) is sharpened half as much as an edge
 *   5 apply      where lobe == 0 (of either sign), the output is the input bit for bit.  Otherwise per channel
 *                o_k = ((lobe * (((b_k + d_k) + f_k) + h_k)) + e_k) / ((4.0f * lobe) + 1.0f)   (the divisor is >= 0.25), then
 *                o_k = min(max(o_k, 0.0f), CAP), then M = max(max(o_r, o_g), o_b) and out_k = o_k / (1.0f - M).  (The quotient is
 *                never -0: its dividend is a sum whose exact zero is +0, and dividing by at most 1 does not underflow.)
 *   6 rgb8 = trunc(clamp(out * 255)), the rule of every rgb8 output here.
 * Consequences.  strength 0 returns the input bit for bit, NaN, Inf and -0 included; so does a constant image, a 1 x 1 image and
 * every pixel with an unusable pixel in its cross.  A sharpened pixel is finite and >= 0, and at most CAP * 2^23.  A non-finite or
 * negative pixel (or one above MAXC) spoils itself and at most its four cross neighbours, all of which are copied through.
 * rgb8 (W*H*3 bytes) and radiance_out (W*H*3 floats) may each be NULL.  Neither may overlap the input (the taps read neighbours;
 * radiance_out == radiance_in is refused), and the two outputs may not overlap each other.  Width and height are 1 .. 65535.
 * Synchronous, on the state's stream; host buffers are staged.  The call leaves FfStats, the stored primary hits and their key, every
 * filter's history, the display exposure and the progressive and adaptive sums as they were; its own state is a work buffer
 * (allocated on first use, regrown for a larger size, freed by ff_destroy).  FF_ERR_INVALID_ARG, naming the field, before any
 * device work for: a NULL state, params or radiance_in; a bad size; a strength outside 0 .. 1 or not finite; unknown flags or a
 * nonzero reserved; an output that overlaps the input or the other output.
 * Not offered: the 3 x 3 (9-tap) form, sharpening inside ff_taa_upscale's kernel, a G-buffer-guided form, a multi-GPU twin. */
FF_API int ff_sharpen(FfState* state, int width, int height, const FfSharpenParams* p,
                      const float* radiance_in, int input_on_device,
                      void* rgb8, int rgb8_on_device, float* radiance_out, int radiance_out_on_device);

/* Host-only twin (no GPU, no state, host pointers), compiled from the same inline per-pixel functions the kernel uses: the same
 * image arguments, the same checks, the same bits. */
FF_API int ff_sharpen_host(int width, int height, const FfSharpenParams* p, const float* radiance_in,
                           unsigned char* rgb8, float* radiance_out);

/* ---- local tone mapping (bilateral grid, directly before ff_display) ------------------------------ */

/* Defaults: compression 0.5, detail 1, pivot 0.18, cell 32, no flags. */
FF_API void ff_local_tonemap_params_init(FfLocalTonemapParams* p);

/* Local tone mapping of a W x H float3 scene-referred radiance image, radiance out: the large-scale (base) log-luminance of the
 * image is compressed about a pivot, the detail on top of it is kept or boosted, and every pixel's three channels are scaled by
 * one ratio, which keeps hue and saturation.  The base comes from an edge-aware filter, a bilateral grid (J. Chen, S. Paris,
 * F. Durand, "Real-time edge-aware image processing with the bilateral grid", SIGGRAPH 2007; the decomposition after F. Durand,
 * J. Dorsey 2002): a strong luminance edge throws no halo.  ff_display handles dynamic range with one exposure and one curve for
 * the frame; this call sits directly BEFORE it, after ff_sharpen / ff_motion_blur / ff_depth_of_field, and ff_display then applies
 * exposure, curve and encoding as before.  A pure image operation like ff_sharpen: no scene, no G-buffer, no history.  All
 * arithmetic is float32 + - * / and floor and integer operations on a float's bit pattern, evaluated as written with the
 * parentheses shown, no fused multiply-add; log, exp and pow appear nowhere, and the grid is summed in integers, so
 * ff_local_tonemap, ff_local_tonemap_host and a float32 restatement agree bit for bit.  s = cell; ">>" on a negative integer is
 * the arithmetic shift (floor); gw = ceil(W / s), gh = ceil(H / s).
 *   1 pseudo-log l = (0.2126f * r + 0.7152f * g) + 0.0722f * b.  A pixel is MAPPED when its three channels are finite and >= 0 (a
 *                -0 passes) and l is finite and l >= 2^-16 (the floor of ff_display's histogram).  Every other pixel is copied
 *                through bit for bit and contributes nothing.  With e = (bits(l) >> 23) - 127 and m = bits(l) & 0x7FFFFF:
 *                q16 = e * 65536 + (m >> 7), the piecewise-linear log2 in 16.16 fixed point - exact, monotone in l - clamped
 *                to [-16 * 65536, 24 * 65536 - 1].  q10 = q16 >> 6.  Lf = float(q16) * 2^-16 (exact)
 *   2 splat      the grid has gw x gh columns of 40 cells of one stop; cell (cx, cy, z) is index (cy * gw + cx) * 40 + z.  A mapped
 *                pixel (x, y) goes to cell (x / s, y / s, (q10 >> 10) + 16) (integer divisions).  A cell holds two int32: the count
 *                n of its pixels and the sum S of their q10 (|q10| < 2^15 and at most 4 096 pixels: no overflow).  Integer adds:
 *                the grid does not depend on their order
 *   3 blur       n and S converted to float (round to nearest even: S can exceed 2^24), then per axis, x first, then y, then z, and
 *                for n and S alike: v'(i) = ((v(i-1) + (2.0f * v(i))) + v(i+1)) * 0.25f, each pass on the whole result of the one
 *                before; a tap outside the grid is 0.0f (dropped: n and S lose the same weight, so S / n is not biased)
 *   4 slice      per mapped pixel fx = (((float)x + 0.5f) / s) - 0.5f and fy alike (the division is exact), fz = (Lf + 16.0f) -
 *                0.5f.  Per axis with last = gw - 1, gh - 1, 39: f = f < 0 ? 0 : (f > last ? last : f); i0 = floor(f);
 *                i1 = min(i0 + 1, last); t = f - i0 (exact).  lerp(a, b, t) = (a * (1.0f - t)) + (b * t).  For n and S alike, of the
 *                eight taps v(x, y, z): along x first - v00 = lerp(v(x0,y0,z0), v(x1,y0,z0), tx), v10 = the same at (y1, z0), v01 at
 *                (y0, z1), v11 at (y1, z1) - then along y - v0 = lerp(v00, v10, ty), v1 = lerp(v01, v11, ty) - then
 *                v' = lerp(v0, v1, tz).  base = (S' / n') * 2^-10 where n' > 0, else base = Lf
 *   5 gain       P = step 1's Lf of `pivot` (as if l = pivot).  g = ((compression - 1.0f) * (base - P)) + ((detail - 1.0f) * (Lf -
 *                base)), then g = g < -32 ? -32 : (g > 32 ? 32 : g).  Where g == 0 (of either sign) the pixel is copied through
 *                bit for bit.  Otherwise k = floor(g), f = g - k (exact), ratio = (1.0f + f) * 2^k, the power of two being the
 *                float with bits (k + 127) << 23 (the inverse piecewise-linear exp2), and out_c = c * ratio per channel
 *   6 rgb8 = trunc(clamp(out * 255)), the rule of every rgb8 output here.
 * The piecewise-linear log2 and exp2 are within 0.086 stops and 6 % of the true ones; both are continuous and monotone.  This is accepted; tools/local_tonemap_bench.py reports the deviation
 * from a float64 restatement with true log2 / exp2.
 * Consequences.  compression 1 with detail 1 returns the input bit for bit (NaN, Inf and -0 included) and builds no grid.  A
 * non-finite, negative or too dark pixel is copied and changes no other pixel: it is as if it were black.  Multiplying the image
 * and the pivot by 2^k multiplies the output by 2^k (up to the clamps of steps 1 and 5).  A mapped pixel's output is >= 0; it
 * can overflow to +Inf only for a channel above 2^94.
 * rgb8 (W*H*3 bytes) and radiance_out (W*H*3 floats) may each be NULL.  radiance_out may be radiance_in itself (the grid is
 * complete before any pixel is written and every pixel is read before it is written); any other overlap of an output with the
 * input, and of the two outputs with each other, is refused.  Width and height are 1 .. 65535.  Synchronous, on the state's
 * stream; host buffers are staged.  The call leaves FfStats, the stored primary hits and their key, every filter's history, the
 * display exposure and the progressive and adaptive sums as they were; its own state is a work buffer (two grids and the staging;
 * allocated on first use, regrown for a larger size, freed by ff_destroy).  FF_ERR_INVALID_ARG, naming the field, before any
 * device work for: a NULL state, params or radiance_in; a bad size; a compression outside 0 .. 1, a detail outside 0 .. 4, a
 * pivot outside [2^-16, 2^24) or any of them not finite; a cell other than 8, 16, 32, 64; nonzero flags or reserved; a refused
 * overlap.
 * Not offered: a multi-GPU twin, the call folded into ff_display, a bin other than one stop, temporal smoothing of the grid. */
FF_API int ff_local_tonemap(FfState* state, int width, int height, const FfLocalTonemapParams* p,
                            const float* radiance_in, int input_on_device,
                            void* rgb8, int rgb8_on_device, float* radiance_out, int radiance_out_on_device);

/* Host-only twin (no GPU, no state, host pointers), compiled from the same inline functions the kernels use: the same image
 * arguments, the same checks, the same bits. */
FF_API int ff_local_tonemap_host(int width, int height, const FfLocalTonemapParams* p, const float* radiance_in,
                                 unsigned char* rgb8, float* radiance_out);

/* Step 2's grid alone (host only): out_n and out_S take gw * gh * 40 int32 each, in step 2's cell order.  The parameter block is
 * checked as above (compression, detail and pivot too, though only `cell` is used); built even for compression 1 with detail 1. */
FF_API int ff_local_tonemap_grid_host(int width, int height, const FfLocalTonemapParams* p, const float* radiance_in,
                                      int32_t* out_n, int32_t* out_S);

/* ---- frame interpolation (an in-between frame from two rendered neighbours) ----------------------- */

/* Defaults: t 0.5, surface_tolerance 4 pixels, fill_radius 4, no flags. */
FF_API void ff_interpolate_params_init(FfInterpolateParams* p);

/* Makes the W x H frame of a pose between two rendered frames A and B: frames traced for frames shown, beside ff_upscale (pixels
 * traced for pixels shown) and the temporal filters (samples for history).  ff_gbuffer gives the exact first hit of ANY pose for a
 * fraction of a frame's cost, so the in-between ("mid") frame does not guess its geometry from motion vectors: each of its pixels
 * knows its surface point, projects it through the camera of A and of B, and fetches its colour there - a backward gather, no
 * scatter.  A pure image operation like ff_upscale: no scene is read and none is needed, no history is kept.  All images are W x H,
 * row-major, top row first.  position and ids are ff_gbuffer's at camera_mid; radiance_S (at any stage of the pipeline),
 * position_S and ids_S belong to the source S in {A, B} rendered at camera_S.  geom_maps (a HOST pointer, or NULL for a static
 * scene) holds per geometry g and source S, at geom_maps + 12 (2 g + S), the row-major 3 x 4 affine map a_S,g that carries a
 * world point of g at the mid pose to its place at S's pose (ff_interpolate_geometry_maps builds them); a map whose 12 floats are
 * bitwise those of the identity (1 0 0 0, 0 1 0 0, 0 0 1 0) IS an identity: x^ = x exactly, nothing is multiplied.  All arithmetic
 * is float32, evaluated as written with the parentheses shown, no fused multiply-add, IEEE division, floor and comparisons; exp and
 * sqrt appear nowhere (distances are compared as squares), so ff_interpolate, ff_interpolate_host and a float32 restatement agree
 * bit for bit.  P(M, X) is ff_taa's projection with that camera's m_screenWidth / m_screenHeight; M_mid, M_S: the UNJITTERED
 * ff_camera_ray_matrix of each camera, inverted in double on the host (Gauss-Jordan elimination with partial pivoting) and rounded.  Per pixel p = (x, y) with x_p = position[p],
 * g = ids[3p] (-1: a miss) and k = ids[3p + 2] (the bxdf type):
 *   1 lookup     per source S.  A hit with maps given and g >= num_geometries: the lookup fails (ff_taa's "not known").  A hit:
 *                x^ = x_p under an identity (or without maps), otherwise per row r
 *                x^_r = (a_r.x * x_p.x + a_r.y * x_p.y) + (a_r.z * x_p.z + a_r.w).  If camera_S is bitwise camera_mid and the map is
 *                an identity (a miss: the camera alone), h_S = (x, y) exactly and nothing is projected.  Otherwise
 *                h_S = (x, y) + (P(M_S, X) - base), per axis (float)x + (f - base):  a hit has X = x^ and base = P(M_mid, x_p), which
 *                cancels a pixel jitter in the mid G-buffer as ff_taa's motion does; a miss has X = the kernel.cu:203 far point of
 *                the pixel's unjittered ray under M_mid (ff_taa's) and base = (x, y).  The lookup fails when either projection has
 *                q.w <= 0 (or NaN) or unless 0 <= h_S.x <= W - 1 and 0 <= h_S.y <= H - 1
 *   2 taps       i0 = floor(h_S.x), tx = h_S.x - i0; j0, ty likewise.  The taps are (i0 + {0, 1}, j0 + {0, 1}), row by row, each
 *                coordinate clamped into the image, b_q = (1 - tx | tx) * (1 - ty | ty).  A tap counts when b_q > 0; ids_S there has
 *                p's geometry index and bxdf type (a miss matches a miss); radiance_S there is finite in all three channels; and, for
 *                a hit, it shows the same surface point: with d = position_S[q] - x^ and e = x^ - camera_S.m_position,
 *                (d.x*d.x + d.y*d.y) + d.z*d.z <= (tol * tol) * (((e.x*e.x + e.y*e.y) + e.z*e.z) * (pix_S * pix_S)),  tol =
 *                surface_tolerance, pix_S = 2 tan(m_fov / 2) / m_screenHeight of camera_S (the world size of a pixel at unit distance;
 *                double on the host, rounded to float).  A NaN on either side does not count.  c_S = ff_upscale's "mean" over the
 *                counting taps with w_q = b_q: c_0 + (sum w (c_q - c_0)) / sum w, c_0 the first of them, and c_0 itself for a single
 *                tap - one tap, or a colour all taps share, comes back bit for bit.  S is VALID when a tap counts
 *   3 combine    both valid: o = blend(c_A, c_B) per channel, where blend(a, b) = a if t == 0 or a == b, b if t == 1, and
 *                (1.0f - t) * a + t * b otherwise.  (The two exceptions close what the formula leaves open: at t = 0 it would turn
 *                a -0 of c_A into +0 and an overflowed c_B into NaN, and a colour both sources share would come back rounded.)
 *                One valid: that source's c, bit for bit.  Neither: p is a HOLE
 *   4 fill       (a second pass over step 3's output and validity)  a hole takes the mean, in the same form, over the pixels
 *                q = (x + dx, y + dy), dy = -r .. r outer, dx = -r .. r inner, r = fill_radius, that lie in the image, are no holes
 *                and whose ids geometry index and bxdf type in the MID G-buffer equal p's, with w = 1.0f / (float)(dx*dx + dy*dy):
 *                o_0 + (sum w (o_q - o_0)) / sum w.  This is sum w o_q / sum w; such a pixel counts as "filled".  Without such a
 *                pixel (always for fill_radius 0): o = blend(radiance_A[p], radiance_B[p]), the screen-space blend, counted as
 *                "fallback"; a non-finite blend is written as it is - the rule of the other filters, its own pixel only
 *   5 rgb8 = trunc(clamp(o * 255)), the rule of every rgb8 output here.
 * counts (a HOST pointer to five uint32, may be NULL) receives the number of pixels resolved as {both, A only, B only, filled,
 * fallback}; they sum to W * H.
 * Consequences.  Three bitwise-equal cameras, no maps (or identities), the three G-buffers equal and A == B finite return A bit
 * for bit (every pixel is its own single tap, and blend(a, a) = a).  t = 0 returns c_A wherever A is valid - bit for bit, a -0
 * included - and t = 1 returns c_B wherever B is valid.  A constant finite colour in A and B returns that colour everywhere: the
 * mean of equal colours and blend(a, a) are exact, in steps 2, 3 and 4 alike.  A non-finite source pixel never counts as a tap, so it
 * reaches the output through step 4's fallback only; every other output pixel is finite as long as the means do not overflow.
 * rgb8 (W*H*3 bytes) and radiance_out (W*H*3 floats) may each be NULL and must not overlap an input or each other.
 * inputs_on_device covers the eight input images.  Host buffers are staged through the state's image staging buffer; the call keeps
 * nothing else in the state and leaves FfStats, the stored primary hits and their key, every filter's history, the display
 * exposure and the progressive and adaptive sums as they were; its own state is a work buffer (allocated on first use, regrown for
 * a larger size, freed by ff_destroy).  Synchronous, on the state's stream.  FF_ERR_INVALID_ARG, naming the field, before any
 * device work for: a NULL state, params, camera, position, ids or radiance; a width or height outside 1 .. 65535; t outside
 * [0, 1] or NaN; a surface_tolerance that is not positive and finite; fill_radius outside 0 .. 8; nonzero flags or reserved;
 * geom_maps given with num_geometries <= 0; an output that overlaps an input or the other output; a camera whose ray matrix is
 * singular.
 * Not offered: view-dependent re-shading (mirrors, glass and glossy highlights are fetched at their surface point, so a reflection
 * lags), sources of a different size, extrapolation beyond [0, 1], a multi-GPU twin. */
FF_API int ff_interpolate(FfState* state, int width, int height, const FfInterpolateParams* p,
                          const FfCamera* camera_mid, const float* position, const int32_t* ids,
                          const FfCamera* camera_a, const float* radiance_a, const float* position_a, const int32_t* ids_a,
                          const FfCamera* camera_b, const float* radiance_b, const float* position_b, const int32_t* ids_b,
                          const float* geom_maps, int num_geometries, int inputs_on_device,
                          void* rgb8, int rgb8_on_device, float* radiance_out, int radiance_out_on_device, uint32_t* counts);

/* Host-only twin (no GPU, no state, host pointers), compiled from the same inline per-pixel functions the kernels use: the same
 * image arguments, the same checks, the same bits and the same counts. */
FF_API int ff_interpolate_host(int width, int height, const FfInterpolateParams* p,
                               const FfCamera* camera_mid, const float* position, const int32_t* ids,
                               const FfCamera* camera_a, const float* radiance_a, const float* position_a, const int32_t* ids_a,
                               const FfCamera* camera_b, const float* radiance_b, const float* position_b, const int32_t* ids_b,
                               const float* geom_maps, int num_geometries,
                               unsigned char* rgb8, float* radiance_out, uint32_t* counts);

/* The geom_maps of ff_interpolate from the n geometries of a scene at the three poses (only m_modelMatrix is read): out receives
 * n * 2 * 12 floats, a_S,g = M_S,g inverse(M_mid,g) composed in double and rounded (S = 0: a, 1: b).  A geometry whose model matrix
 * at S is bitwise the one at mid gets the exact identity, which ff_interpolate applies as x^ = x; out_identity_flags (n * 2 int32,
 * may be NULL) says which.  FF_ERR_INVALID_ARG for a NULL array, n <= 0 or a singular model matrix at mid.  No GPU, no state. */
FF_API int ff_interpolate_geometry_maps(const FfGeometry* mid, const FfGeometry* a, const FfGeometry* b, int n, float* out,
                                        int32_t* out_identity_flags);

/* ---- adaptive sampling (render until every tile's noise estimate is below a threshold) ------------- */

/* Defaults: tile 64, min_passes 2, max_passes 64, threshold 0.0002 (the paper's value: a default for users, not a measured optimum
 * for this renderer - tools/adaptive_bench.py sweeps it), no flags. */
FF_API void ff_adaptive_params_init(FfAdaptiveParams* p);

/* Renders a frame in passes and stops sampling the tiles of the image whose error estimate has fallen below ap->threshold: the
 * stopping condition of Dammertz et al., "A Hierarchical Automatic Stopping Condition for Monte Carlo Global Illumination" (2010),
 * on a fixed grid of ap->tile x ap->tile tiles (row-major, narrower and shorter at the right and bottom edges; the paper's block
 * splitting is left out).  Pass k = 0, 1, 2, ... is an ordinary render of params->spp samples with seed params->seed + k -
 * ff_render_progressive's seed sequence - restricted to the tiles that are still active; a rectangle of the frame renders bit for
 * bit as the whole frame would (ff_render_tile).  Per pixel the call keeps two running float32 sums: `sum` over all of the pixel's
 * passes and `sum_even` over its passes of even k (pass 0 writes both, later passes add).  A stopped tile never resumes, so a
 * tile's passes are always 0 .. n_t - 1 and all pixels of a tile share n_t.
 *   The error of a tile after n passes, n even.  float32 throughout, only + - * / sqrt and fabs, evaluated as written with the
 *   parentheses shown, no fused multiply-add.  inv_n = 1.0f / (float)n, inv_h = 1.0f / (float)(n / 2).  Per pixel and channel
 *   I_c = sum_c * inv_n and A_c = sum_even_c * inv_h; d = (I_r + I_g) + I_b; e_p = 0 where !(d > 0), otherwise
 *   e_p = ((|I_r - A_r| + |I_g - A_g|) + |I_b - A_b|) / sqrt(d).  S is the sum of e_p over the tile's N_t pixels in a fixed order:
 *   with the pixels in the tile's row-major order i = 0 .. N_t - 1, lane j of 256 adds e_j, e_(j+256), ... in that order starting
 *   from 0.0f (a lane without a pixel holds 0.0f), then v[j] += v[j + off] for off = 128, 64, ..., 1, and S = v[0].
 *   E_t = S * sqrt((float)N_t / (float)(W * H)) / (float)N_t, left to right.  The order does not depend on the launch shape:
 *   ff_adaptive_tile_error, ff_adaptive_tile_error_host and a float32 restatement agree bit for bit.
 *   A tile stops at a check iff E_t < threshold.  A NaN error is below nothing: such a tile stays active until max_passes.
 *   The driver.  All tiles start active.  Each pass turns the active tiles into rectangles (ff_adaptive_plan_host), renders each
 *   into a compact buffer and adds it to the sums.  After pass k, with n = k + 1: if n is even and n >= min_passes, E_t of the
 *   active tiles is computed on the device and read back, and the tiles below the threshold stop.  Under
 *   FF_ADAPTIVE_GUARD_NEIGHBOURS a tile stops only when it and all of its up to 8 neighbours are below the threshold at this same
 *   check, a neighbour that has already stopped counting as below: no quiet tile stops beside a noisy one, which would leave a
 *   seam.  The call ends when no tile is active or n == max_passes.  Each pixel then is sum * (1.0f / (float)n_t), and rgb8 the
 *   rule of every rgb8 output here of that value.  threshold 0 is ff_render_progressive's frame max_passes - 1 bit for bit;
 *   threshold +inf stops every tile with a finite error at min_passes.
 * rgb8 (W*H*3 bytes), radiance (W*H*3 floats) and passes_out (W*H uint16, each pixel's n_t) follow ff_render's conventions and may
 * each be NULL; out_info is a host pointer and may be NULL.  Because every pass goes through the frame's own code the call honours
 * ff_set_pixel_jitter, ff_set_camera_sampling, textures, roughness and the environment.  Synchronous, on the state's stream.
 * FfStats describes the last rectangle rendered.  The call leaves the progressive sum (a running ff_render_progressive sequence
 * continues after it), every filter's history and the display exposure as they were; the stored primary hits follow the frames'
 * own rule (a rectangle other than the whole frame replaces them).  Its own state is reset per call (buffers allocated on first
 * use, regrown for a larger size, freed by ff_destroy).
 * FF_ERR_INVALID_ARG, naming the field, before any device work, for: a NULL ap; tile not 16, 32, 64 or 128; min_passes odd or
 * below 2; max_passes odd, below min_passes or above 65534; a NaN or -inf threshold; unknown flags; a nonzero reserved; then what
 * ff_render refuses.
 * Not offered: the multi-GPU entry points, a pixel-buffer twin, the paper's hierarchical block splitting. */
FF_API int ff_render_adaptive(FfState* state, const FfCamera* camera, const FfRenderParams* params, const FfAdaptiveParams* ap,
                              void* rgb8, int rgb8_on_device, float* radiance, int radiance_on_device,
                              uint16_t* passes_out, int passes_on_device, FfAdaptiveInfo* out_info);

/* The last ff_render_adaptive call's accumulators and per-tile results, for tests and tools: sum and sum_even (W*H*3 floats each),
 * tile_passes (n_t per tile, uint16, row-major over the ceil(W / tile) x ceil(H / tile) grid) and tile_error (E_t of each tile's
 * last check, float).  Each may be NULL; on_device covers all four.  FF_ERR_INVALID_ARG when no call has completed on this state. */
FF_API int ff_adaptive_state(FfState* state, float* sum, float* sum_even, uint16_t* tile_passes, float* tile_error, int on_device);

/* The device kernel of the error estimate on planted sums: E_t after n passes (even, 2 .. 65534) of every tile of a width x height
 * image (1 .. 65535 each) under the tile edge `tile` (16, 32, 64 or 128), from sum and sum_even (W*H*3 floats each;
 * inputs_on_device covers both) into out_error (a host pointer, one float per tile, row-major).  Leaves the last
 * ff_render_adaptive call's results as they were. */
FF_API int ff_adaptive_tile_error(FfState* state, int width, int height, int tile, int n, const float* sum, const float* sum_even,
                                  int inputs_on_device, float* out_error);

/* Host-only twin (no GPU, no state, host pointers), compiled from the same inline functions the kernel uses: the same checks, the
 * same bits. */
FF_API int ff_adaptive_tile_error_host(int width, int height, int tile, int n, const float* sum, const float* sum_even,
                                       float* out_error);

/* The driver's rectangle list for a tiles_x x tiles_y grid of flags (row-major, nonzero: active): first, per tile row, the maximal
 * runs of active tiles; then runs of consecutive rows with the identical span [tx0, tx1) merge.  A rectangle is four ints
 * {tx0, ty0, tx1, ty1} in tiles, half open, and the list is in the order of the rectangles' first rows, then of tx0.  All tiles
 * active give one rectangle, the whole frame.  Returns the number of rectangles, or -1 with ff_last_error set for a NULL pointer,
 * a grid size below 1 or a max_rects (the room in out_rects4, in rectangles) too small for the list.  ff_render_adaptive calls
 * this very function. */
FF_API int ff_adaptive_plan_host(int tiles_x, int tiles_y, const uint8_t* active, int32_t* out_rects4, int max_rects);

/* ---- display transform (exposure, bloom, tone curve, sRGB) ------------------------------------- */

/* Defaults: ACES, SRGB, flags 0, exposure 1, white 4, key 0.18, percentiles 0.5 / 0.95, min_exposure 2^-10, max_exposure 2^10,
 * adapt_darken 3, adapt_brighten 1, dt 0, bloom_threshold 1, bloom_strength 0.05, bloom_levels 5. */
FF_API void ff_display_params_init(FfDisplayParams* p);

/* The last stage of render -> ff_gbuffer -> ff_denoise_temporal -> ff_taa: turns W x H float3 radiance into the uchar3 buffer a
 * viewer uploads.  A pure image operation like ff_denoise: no scene is read and none is needed.  All per-pixel arithmetic is
 * float32, every formula evaluated left to right as written with the parentheses shown, no fused multiply-add; bits(l) is a
 * float's 32-bit pattern.  In the order it is evaluated:
 *   1 histogram  (only with FF_DISPLAY_AUTO_EXPOSURE; otherwise all 256 counts are 0)  l = (0.2126 r + 0.7152 g) + 0.0722 b of the
 *                input pixel.  A pixel is counted when r, g, b are all finite and l >= 2^-16; its bin is
 *                min((bits(l) >> 20) - 888, 255): 8 bins per stop from 2^-16 up (exponent and three mantissa bits), the top bin
 *                open-ended.  Counts are integers: the histogram does not depend on the order of the adds
 *   2 exposure   (host, double; ff_display_exposure is this step alone)  N = sum n_b.  low_percentile * N of mass is removed from
 *                bin 0 upward and (1 - high_percentile) * N from bin 255 downward, each bin giving min(what it holds, what is
 *                still to remove), the bottom first; with the remaining n'_b: S = sum n'_b and M = (sum n'_b L_b) / S, both sums
 *                from bin 0 upward, L_b = (b + 0.5) / 8 - 16; target = clamp(key / 2^M, min_exposure, max_exposure) * exposure.
 *                N = 0 or S <= 0: target = the previous exposure, or `exposure` if there is none.  No previous exposure (first
 *                call, ff_display_reset) or dt <= 0: E = target.  Otherwise rate = adapt_darken if target < E_prev else
 *                adapt_brighten and E = E_prev * 2^((log2 target - log2 E_prev) * (1 - exp(-dt * rate))).  E and target are
 *                rounded to float once, at the end; E becomes the next call's E_prev.  Without AUTO_EXPOSURE: E = target =
 *                exposure, and the stored previous exposure is left alone
 *   3 exposed    e = c * E per channel.  A pixel with a non-finite channel may spoil only itself: in steps 1 and 4 it counts as
 *                black; in step 5 its channels map NaN -> 0, -Inf -> 0, +Inf -> 1 (its finite channels go the ordinary way)
 *   4 bloom      (only with FF_DISPLAY_BLOOM)  bright pass at full resolution: le = the luminance of e as in step 1,
 *                k = max(le - bloom_threshold, 0) / max(le, 1e-30), B_0 = e * k.  Level j = 1 .. n = bloom_levels has size
 *                (ceil(W_{j-1} / 2), ceil(H_{j-1} / 2)) and D_j(x, y) = ((D_{j-1}(2x, 2y) + D_{j-1}(2x+1, 2y)) + (D_{j-1}(2x, 2y+1)
 *                + D_{j-1}(2x+1, 2y+1))) * 0.25 with coordinates clamped into level j-1 (D_0 = B_0).  Back up: U_n = D_n;
 *                U_j = D_j + up(U_{j+1}) for j = n-1 .. 1, where up(S)(x, y) is the bilinear sample of S at ((x + 0.5) / 2 - 0.5,
 *                (y + 0.5) / 2 - 0.5): taps x0 = (x - 1) >> 1 (arithmetic shift) and x0 + 1, clamped into S, with weights
 *                (wx0, wx1) = (0.25, 0.75) for even x and (0.75, 0.25) for odd x, the same in y, rows combined first:
 *                (S00 wx0 + S10 wx1) wy0 + (S01 wx0 + S11 wx1) wy1.  e' = e + up(U_1) * (bloom_strength / n), the quotient formed
 *                once in float.  Without the flag e' = e
 *   5 curve      x = max(e', 0) (NaN: 0); REINHARD: w2 = white * white, y = (x * (1 + x / w2)) / (1 + x); ACES: y = (x * (2.51 x +
 *                0.03)) / (x * (2.43 x + 0.59) + 0.14); CLAMP: y = x.  A quotient that comes out NaN (Inf / Inf) is 1.  Then
 *                y = min(max(y, 0), 1): this is display_out
 *   6 encoding   LINEAR: byte = trunc(y * 255) (255 for y = 1), the rule of every rgb8 output here.  SRGB: T_b = float(eotf((b -
 *                0.5) / 255)), eotf(s) = s / 12.92 for s <= 0.04045, else ((s + 0.055) / 1.055)^2.4, in double on the host,
 *                b = 1 .. 255 (ff_srgb_thresholds); the byte is the number of thresholds <= y: round(255 oetf(y)), correctly rounded.
 * rgb8 (W*H*3 bytes) and display_out (W*H*3 floats) may each be NULL; display_out may alias radiance_in.  Width and height are
 * 1 .. 65535.  Synchronous; all launches go to the state's stream.  The call leaves FfStats, the stored primary hits and their
 * key, the three filters' histories and the progressive sum as they were; its own state is the adapted exposure, the last
 * histogram and its scratch buffers (allocated on first use, regrown for a larger size, freed by ff_destroy), and
 * ff_upload_scene does not reset it.  FF_ERR_INVALID_ARG, with a message that names the field, for a NULL state / params /
 * input, a bad size, an unknown curve / encoding / flag bit, and every range in FfDisplayParams' comments (every float must be
 * finite), all checked before any device work. */
FF_API int ff_display(FfState* state, int width, int height, const FfDisplayParams* p, const float* radiance_in, int input_on_device,
                      void* rgb8, int rgb8_on_device, float* display_out, int display_out_on_device);

/* ff_display into the buffer registered with ff_register_gl_pbo (map, ff_display with a device rgb8, unmap).
 * FF_ERR_GL_UNAVAILABLE when none is registered, FF_ERR_INVALID_ARG when the size differs from the registration. */
FF_API int ff_display_to_pbo(FfState* state, int width, int height, const FfDisplayParams* p, const float* radiance_in, int input_on_device);

/* Forgets the adapted exposure: the next automatic call takes its target at once. */
FF_API int ff_display_reset(FfState* state);

/* The last ff_display call's E, target and histogram (256 counts); any may be NULL.  FF_ERR_INVALID_ARG before the first call. */
FF_API int ff_display_state(FfState* state, float* out_exposure, float* out_target, uint32_t* out_histogram256);

/* Host-only pieces of the operator (no GPU, no state). */
/* T_1 .. T_255 of step 6. */
FF_API int ff_srgb_thresholds(float* out255);
/* Steps 5 and 6 for n values of e' (p's curve, white and encoding); out_y and out_bytes may each be NULL. */
FF_API int ff_display_curve(const FfDisplayParams* p, const float* exposed, int n, float* out_y, unsigned char* out_bytes);
/* Step 2 for a histogram of 256 counts; previous_exposure <= 0: there is none.  Either output may be NULL. */
FF_API int ff_display_exposure(const FfDisplayParams* p, const uint32_t* histogram256, float previous_exposure, float* out_target,
                               float* out_exposure);

/* The writer twin of ff_load_hdr: flat (not run-length encoded) scanlines, header "#?RADIANCE", "FORMAT=32-bit_rle_rgbe",
 * "-Y h +X w".  Texel, in float: m = max(r, g, b); m < 1e-32: (0, 0, 0, 0); else frexp(m) = (f, e), scale = (f * 256) / m, channel
 * byte = min(trunc(c * scale), 255), exponent byte e + 128.  FF_ERR_INVALID_ARG for a negative or non-finite value or one of
 * 2^127 and more (no exponent byte), FF_ERR_IO when the file cannot be written.  What ff_load_hdr reads back saves to the same
 * bytes again. */
FF_API int ff_save_hdr(const char* path, const float* rgb, int width, int height);

/* saveToPPM (utilities.h:842-856) for the 8-bit framebuffer: P3 text, one "r g b" line per pixel, top row first. */
FF_API int ff_save_ppm(const char* path, const unsigned char* rgb8, int width, int height);

/* The reader twin of ff_save_ppm: a P3 (text) or P6 (binary) PPM with maxval 255, '#' comments in the header.  *out_rgb8 is malloc'ed
 * (height rows of width RGB bytes, top row first); release with ff_free_ppm.  What ff_save_ppm wrote loads back to the same bytes.
 * FF_ERR_IO for a file that cannot be opened or ends early, FF_ERR_INVALID_ARG for a malformed one, another maxval or a size
 * outside 1 .. 2^26 pixels. */
FF_API int ff_load_ppm(const char* path, unsigned char** out_rgb8, int* out_width, int* out_height);
FF_API void ff_free_ppm(unsigned char* rgb8);

/* n bytes to floats for a texture: srgb != 0: out = float(eotf(b / 255)) with ff_display's eotf (s / 12.92 for s <= 0.04045, else
 * ((s + 0.055) / 1.055)^2.4), a 256-entry table computed in double; srgb == 0: out = float(b / 255.0). */
FF_API int ff_rgb8_to_linear(const unsigned char* bytes, int n, int srgb, float* out_floats);

/* ---- video planes (Y'CbCr 4:2:0 for an encoder, after ff_display or ff_local_tonemap) ------------- */

/* Defaults: BT709 transfer, BT709 matrix, LIMITED range, depth 8, LEFT siting, reference_white_nits 203. */
FF_API void ff_yuv_params_init(FfYuvParams* p);

/* The sizes of the two planes ff_encode_yuv writes for a width x height image under p (step 8); either output may be NULL.  The
 * checks are ff_encode_yuv's for the size and the parameters. */
FF_API int ff_yuv_plane_bytes(int width, int height, const FfYuvParams* p, uint64_t* luma_bytes, uint64_t* chroma_bytes);

/* K_0 .. K_4096 of step 4 for FF_YUV_TRANSFER_*: 4097 floats.  FF_ERR_UNSUPPORTED if they do not rise strictly from exactly 0 to
 * exactly 1 on this host (every later step relies on it). */
FF_API int ff_yuv_knots(int transfer, float* out4097);

/* The stage that leaves the pipeline for a video encoder or a stream: turns a W x H image of float3 DISPLAY-LINEAR values into
 * Y'CbCr 4:2:0 planes - NV12 at depth 8, P010 at depth 10.  For SDR the input is ff_display's display_out under FF_ENCODE_LINEAR
 * semantics (1 = peak white; the chain is ff_display(display_out) -> ff_encode_yuv); for PQ it is radiance after exposure, 1.0
 * being reference white (ff_local_tonemap -> ff_encode_yuv with PQ, BT2020, depth 10 is HDR10).  A pure image operation like
 * ff_display: no scene, no G-buffer, no history.  All per-pixel arithmetic is float32 + - * / and floor, every formula evaluated
 * left to right as written with the parentheses shown, no fused multiply-add, IEEE division; pow appears only where the knots are
 * made (double, host), so ff_encode_yuv, ff_encode_yuv_host and a float32 restatement agree bit for bit.  Per pixel and channel:
 *   1 sanitise   NaN and every value that is not > 0 (negative, -Inf, either zero) become +0; then c = min(c, 65536).  All later
 *                steps see finite numbers
 *   2 gamut      (only with FF_YUV_MATRIX_BT2020)  linear BT.709 primaries to BT.2020 (BT.2087, rounded to float):
 *                r' = (0.6274 r + 0.3293 g) + 0.0433 b, g' = (0.0691 r + 0.9195 g) + 0.0114 b, b' = (0.0164 r + 0.0880 g) + 0.8956 b
 *   3 scale      PQ: v = c * (reference_white_nits / 10000), the quotient formed once in float; otherwise v = c.  Then v = min(v, 1)
 *   4 transfer   knots K_j = float(eotf(j / 4096)), j = 0 .. 4096, in double on the host (ff_yuv_knots); K_0 = 0, K_4096 = 1, strictly
 *                increasing.  eotf(s): SRGB s / 12.92 for s <= 0.04045, else ((s + 0.055) / 1.055)^2.4 (ff_display's); BT709
 *                s / 4.5 for s < 0.081, else max(((s + 0.099) / 1.099)^(1 / 0.45), 0.081 / 4.5) (BT.709's OETF steps from 0.081 to
 *                0.08125 at 0.018 and its inverse is level across that gap; without the max K_332 would lie below K_331); PQ (ST 2084, 10 000 nits = 1) p = s^(1 / m2),
 *                (max(p - c1, 0) / (c2 - c3 p))^(1 / m1) with m1 = 2610 / 16384, m2 = 2523 / 4096 * 128, c1 = 3424 / 4096,
 *                c2 = 2413 / 4096 * 32, c3 = 2392 / 4096 * 32.  v >= 1: e = 1.  Otherwise j = the number of K_1 .. K_4095 that are
 *                <= v (twelve halving steps: for step = 2048, 1024 .. 1: if K_{j+step} <= v then j += step) and
 *                e = (float(j) + (v - K_j) / (K_{j+1} - K_j)) * (1 / 4096): the piecewise-linear inverse of the EOTF.  e and the
 *                true OETF value lie in the same cell of 1 / 4096, under a quarter of a 10-bit code apart
 *   5 luma       (Kr, Kg, Kb, Dcb, Dcr) = BT709 (0.2126, 0.7152, 0.0722, 1.8556, 1.5748), BT2020 (0.2627, 0.6780, 0.0593, 1.8814,
 *                1.4746), float constants; with r, g, b step 4's outputs: y = (Kr r + Kg g) + Kb b, cb = (b - y) / Dcb,
 *                cr = (r - y) / Dcr
 *   6 chroma     the chroma planes are ceil(W/2) x ceil(H/2); every tap coordinate is clamped into the image; cb and cr are
 *                filtered unquantised, c(x, y) being either.  CENTER: ((c(2X, 2Y) + c(2X+1, 2Y)) + (c(2X, 2Y+1) + c(2X+1, 2Y+1))) *
 *                0.25.  LEFT: h(row) = (c(2X-1, row) * 0.25 + c(2X, row) * 0.5) + c(2X+1, row) * 0.25, the sample is
 *                (h(2Y) + h(2Y+1)) * 0.5
 *   7 quantise   s = 2^(depth - 8), m = 2^depth - 1.  LIMITED: Y = floor((219 y + 16) * s + 0.5), C = floor((224 c + 128) * s + 0.5)
 *                clamped to [16 s, 240 s].  FULL: Y = floor(y * m + 0.5), C = floor((c * m + 2^(depth-1)) + 0.5) clamped to [0, m]
 *   8 store      depth 8, NV12: luma is W x H bytes; chroma is ceil(H/2) rows of ceil(W/2) interleaved Cb Cr byte pairs.  Depth 10,
 *                P010: the same layout in little-endian uint16 with the code in the high ten bits (code << 6).  Rows are tightly
 *                packed (ff_yuv_plane_bytes gives the sizes).
 * Width and height are 1 .. 65535.  Synchronous, on the state's stream; host buffers are staged (input_on_device covers linear_in,
 * outputs_on_device both planes).  The knots of a transfer are uploaded on its first use and kept in the state; ff_destroy frees
 * them and the staging buffer.  The call leaves FfStats, the stored primary hits and their key, every filter's history, the display
 * exposure and the progressive and adaptive sums as they were.  FF_ERR_INVALID_ARG, naming the field, before any device work for: a
 * NULL state, params, linear_in, luma or chroma; a bad size; an unknown transfer, matrix, range or siting; a depth other than 8 or
 * 10; a reference_white_nits that is not finite or outside (0, 10000]; an output that overlaps the input or the other output.
 * Not offered: 4:4:4 and 4:2:2 output, HLG, dithering, top-left (type 2) siting, row pitches other than tight. */
FF_API int ff_encode_yuv(FfState* state, int width, int height, const FfYuvParams* p, const float* linear_in, int input_on_device,
                         void* luma, void* chroma, int outputs_on_device);

/* Host-only twin (no GPU, no state, host pointers), compiled from the same inline functions the kernel uses: the same image
 * arguments, the same checks, the same bytes. */
FF_API int ff_encode_yuv_host(int width, int height, const FfYuvParams* p, const float* linear_in, void* luma, void* chroma);

/* One YUV4MPEG2 frame of ff_encode_yuv's host planes, to pipe into any encoder.  append == 0 starts the file with the stream header
 * "YUV4MPEG2 W<w> H<h> F30:1 Ip A1:1 <C> XCOLORRANGE=<LIMITED|FULL>", <C> being C420p10 at depth 10, else C420mpeg2 for LEFT and
 * C420jpeg for CENTER; append != 0 adds a frame to an existing file.  A frame is "FRAME\n" and the planar Y, Cb, Cr samples; depth
 * 10 as low-aligned little-endian 16-bit codes (the P010 sample >> 6), as Y4M expects.  The parameter checks are ff_encode_yuv's;
 * FF_ERR_IO when the file cannot be written. */
FF_API int ff_save_y4m(const char* path, int append, int width, int height, const FfYuvParams* p, const void* luma, const void* chroma);

/* ---- resampling (separable polyphase, to any size within a factor of 16) -------------------------- */

/* Defaults: FF_RESIZE_LANCZOS3, FF_RESIZE_ANTI_RING, reserved 0. */
FF_API void ff_resize_params_init(FfResizeParams* p);

/* T, the number of taps every output sample of an axis of in_size input and out_size output samples has under `filter` (below):
 * at most 96.  FF_ERR_INVALID_ARG for a size or a ratio ff_resize refuses, an unknown filter or a NULL out_taps. */
FF_API int ff_resize_taps(int in_size, int out_size, int filter, int* out_taps);

/* The table of one axis as ff_resize and ff_resize_host use it: out_first[X] for X = 0 .. out_size - 1, and out_weights[X * T + j]
 * for tap j = 0 .. T - 1 (T from ff_resize_taps).  The checks are ff_resize_taps'; neither pointer may be NULL. */
FF_API int ff_resize_weights(int in_size, int out_size, int filter, int32_t* out_first, float* out_weights);

/* Resamples a W x H float3 radiance image to W' x H', each size within a factor of 16 of the other, under a reconstruction filter
 * that is stretched when it minifies: what makes an image SMALLER (supersampling - render k times the pixels, filter down -,
 * thumbnails and proxies, the size of the planes ff_encode_yuv writes, host-side mip chains for ff_texture_create) or gives it an
 * arbitrary size, where ff_upscale and ff_taa_upscale only enlarge, need G-buffers and stop at 8 times.  A pure image operation like
 * ff_sharpen: no scene, no G-buffer, no history; it works on linear radiance, so it sits BEFORE ff_local_tonemap and ff_display
 * (or on display_out ahead of ff_encode_yuv).  Two passes, the horizontal one always first, W x H -> W' x H, then the vertical one;
 * neither is skipped, even at equal size, because MITCHELL at equal size is a blur.
 * WEIGHTS.  Per axis, on the host, in double, every formula evaluated left to right as written.  For an axis of n input and N
 * output samples:
 *   1 s = (double)n / (double)N
 *   2 f = max(s, 1): the filter is stretched when minifying
 *   3 the radius R is 0.5 for BOX, 1 for TRIANGLE, 2 for MITCHELL and 3 for LANCZOS3
 *   4 r = R * f
 *   5 T = (int)ceil(2 * r), the same for every output sample of the axis (ff_resize_taps); at the limits it is at most 96
 *   6 for output X: c = ((double)X + 0.5) * s - 0.5; first_X = (int)ceil(c - r); t_j = ((double)(first_X + j) - c) / f for tap
 *     j = 0 .. T-1; k_j = k(t_j); S is the sum of k_j from j = 0 upward; w_j = (float)(k_j / S)
 * k(t) with a = |t|:
 *   BOX        1 for -0.5 <= t < 0.5, else 0
 *   TRIANGLE   1 - a for a < 1, else 0
 *   MITCHELL   (B = C = 1.0 / 3.0)
 *              for a < 1: ((12 - 9B - 6C) a a a + (-18 + 12B + 6C) a a + (6 - 2B)) / 6
 *              for a < 2: ((-B - 6C) a a a + (6B + 30C) a a + (-12B - 48C) a + (8B + 24C)) / 6
 *              else 0
 *   LANCZOS3   0 for a >= 3; 1 for t == 0; 0 for every other t that equals its own floor, so that an equal-size pass has the single
 *              weight 1; else 3 sin(pi t) sin(pi t / 3) / (pi pi t t)
 * No tap outside first_X .. first_X + T - 1 has a nonzero k, S > 0 always, and the rounded weights of an output sample sum to 1
 * within 2^-24.  With n = N, BOX, TRIANGLE and LANCZOS3 each give exactly one weight of 1, at input X.  (BOX, TRIANGLE and MITCHELL
 * use only + - * / and are the same bits wherever they are computed; sin is not correctly rounded, so a LANCZOS3 weight of another
 * libm may differ by a float ulp.  ff_resize and ff_resize_host use this library's, the one ff_resize_weights returns.)
 * PIXELS.  All arithmetic is float32 with no fused multiply-add; min(a, b) is b < a ? b : a and max(a, b) is a < b ? b : a.  In
 * each pass, per output sample and channel:
 *   1 tap j reads input index clamp(first_X + j, 0, n - 1).  A clamped tap keeps its weight and counts as often as it is named
 *   2 a non-finite value reads as +0 in everything below - in the vertical pass too, where the value is an intermediate
 *   3 acc = 0; for j = 0 .. T-1: acc = acc + w_j * v_j
 *   4 with FF_RESIZE_ANTI_RING: lo and hi are the min and max of v_j over the taps with w_j != 0, taken in the order of j, and
 *     out = min(max(acc, lo), hi).  Without the flag out = acc: the negative lobes of MITCHELL and LANCZOS3 may then produce
 *     NEGATIVE radiance beside an edge (and values above the brightest input)
 *   5 rgb8 = trunc(clamp(out * 255)), the rule of every rgb8 output here.
 * Consequences.  An equal-size call under BOX, TRIANGLE or LANCZOS3 returns a finite image value for value (a -0 may come back as
 * +0).  With ANTI_RING a constant image returns bit for bit at every size and filter.  A non-finite input sample affects only the
 * outputs whose taps name it.  No output is non-finite: the absolute weights of an output sample sum to less than 2, so this holds
 * for finite input up to 2^125 in magnitude, which two passes cannot carry past FLT_MAX.
 * rgb8 (W'*H'*3 bytes) and radiance_out (W'*H'*3 floats) may each be NULL.  Neither may overlap the input, and the two may not
 * overlap each other; each span is sized by its own image.  Every size is 1 .. 65535, and on each axis out <= 16 in and
 * in <= 16 out.  Synchronous, on the state's stream; host buffers are staged.  The call leaves FfStats, the stored primary hits and
 * their key, every filter's history, the display exposure and the progressive and adaptive sums as they were, and ff_upload_scene
 * resets nothing of it; its own state is the intermediate image, the staging buffer and, per axis, the table uploaded last with its
 * key (in, out, filter) - rebuilt and uploaded only when the key changes -, all allocated on first use, regrown for a larger size
 * and freed by ff_destroy.  FF_ERR_INVALID_ARG, naming the field, before any device work for: a NULL state, params or radiance_in;
 * a size outside 1 .. 65535; sizes more than a factor of 16 apart on an axis; an unknown filter; unknown flags or a nonzero
 * reserved; an output that overlaps the input or the other output.
 * Not offered: other channel counts, a G-buffer-aware form, gamma-space resampling, a row pitch, a multi-GPU twin, a resize fused
 * into ff_encode_yuv. */
FF_API int ff_resize(FfState* state, const FfResizeParams* p, int in_width, int in_height,
                     const float* radiance_in, int input_on_device, int out_width, int out_height,
                     void* rgb8, int rgb8_on_device, float* radiance_out, int radiance_out_on_device);

/* Host-only twin (no GPU, no state, host pointers), compiled from the same inline per-tap functions the kernels use: the same
 * image arguments, the same checks, the same bits. */
FF_API int ff_resize_host(const FfResizeParams* p, int in_width, int in_height, const float* radiance_in,
                          int out_width, int out_height, unsigned char* rgb8, float* radiance_out);

/* ---- colour grade (primary grade, 1D curves, 3D lattice, .cube files) ---------------------------- */

/* Defaults: flags 0, the identity matrix, offset 0, saturation 1, lut_id -1, reserved 0. */
FF_API void ff_grade_params_init(FfGradeParams* p);

/* A LUT object from a descriptor of host arrays: the three curves, the lattice, or both (a half is absent when its size is 0 and its
 * pointer NULL).  LUTs belong to the state like textures: at most 16 at a time, an id freed by ff_grade_lut_destroy is given out
 * again (the lowest free one first), ff_upload_scene leaves them alone and ff_destroy frees them.  The arrays are copied; the
 * caller's may go.  FF_ERR_INVALID_ARG, naming the field, for: a NULL state, descriptor or out_id; a descriptor with neither
 * half; curve_size outside 2 .. 4096, or not the K its FF_GRADE_AXIS_LOG axis gives; an unknown curve_axis; curve_lo or curve_hi
 * not finite, not curve_lo < curve_hi, or curve_hi - curve_lo not finite; on the LOG axis curve_lo <= 0, curve_shift outside
 * 8 .. 23 or low `curve_shift` bits of either end's bit pattern set; on the LINEAR axis a nonzero curve_shift; size outside
 * 2 .. 65; a domain_min or domain_max that is not finite, not domain_min < domain_max, or whose difference is not finite; a size
 * without its pointer or a pointer without its size; a curve knot or a lattice value that is not finite or exceeds FLT_MAX / 2
 * in magnitude (so that no difference of two overflows); a 17th LUT. */
FF_API int ff_grade_lut_create(FfState* state, const FfGradeLut* lut, int* out_id);
/* Frees LUT `id` (after the stream's work has completed).  FF_ERR_INVALID_ARG for an id that names no LUT. */
FF_API int ff_grade_lut_destroy(FfState* state, int id);

/* The colour grade: the one stage that changes the COLOUR of the picture - white balance, channel gains, a channel mixer, gamut
 * conversion, CDL slope and offset, desaturation (stage 1); a camera-log shaper, contrast curves (stage 2); a "look" from any
 * grading tool, a .cube file (stage 3).  A pure per-pixel operation on a W x H float3 image: no scene, no G-buffer, no history,
 * no neighbours.  It works on whatever it is given - scene-linear radiance ahead of ff_local_tonemap and ff_display, or
 * display_out ahead of ff_encode_yuv.
 * All arithmetic is float32 with no fused multiply-add, every formula evaluated left to right as written; max(a, b) is
 * a > b ? a : b and min(a, b) is a < b ? a : b, so a NaN in first place reads as the bound (only a stage 1 that overflowed makes
 * one); bits(x) is the float's bit pattern as an unsigned integer.  Three stages in this order, each run only when its flag is
 * set; flags = 0 copies the image bit for bit.
 *   1 FF_GRADE_PRIMARY  (matrix[9] row-major m, offset[3] o, saturation s; all finite, s >= 0)
 *       c'_r = ((m[0] r + m[1] g) + m[2] b) + o[0], c'_g and c'_b likewise from rows 1 and 2
 *       l = (0.2126 c'_r + 0.7152 c'_g) + 0.0722 c'_b        (ff_display's weights)
 *       c''_i = l + s (c'_i - l)
 *   2 FF_GRADE_CURVES   (the LUT's K knots C per channel, over curve_lo .. curve_hi = lo .. hi); per channel
 *       x' = min(max(x, lo), hi)
 *       FF_GRADE_AXIS_LINEAR:  p = ((x' - lo) / (hi - lo)) float(K - 1); k = min(int(floor p), K - 2); t = p - float(k)
 *       FF_GRADE_AXIS_LOG:     (for scene-linear HDR ahead of a lattice: the knots are evenly spaced in the float's bit pattern, 2^(23 -
 *                              shift) to a binade, as in ff_display's histogram.  0 < lo < hi, shift in 8 .. 23, the low `shift`
 *                              bits of bits(lo) and bits(hi) zero so that no cell straddles a binade, K = ((bits(hi) - bits(lo)) >>
 *                              shift) + 1)
 *                              d = bits(x') - bits(lo); k = min(d >> shift, K - 2); t = float(d - (k << shift)) / float(1 << shift)
 *                              (exact)
 *       y = C[k] + t (C[k + 1] - C[k])
 *   3 FF_GRADE_LUT3D    (the LUT's N^3 texels V, red fastest - texel i + N (j + N k), the .cube order - over domain_min ..
 *                       domain_max); per channel, with that channel's dmin and dmax:
 *       u = (min(max(x, dmin), dmax) - dmin) / (dmax - dmin); p = u float(N - 1); i = min(int(floor p), N - 2); f = p - float(i)
 *     giving the cell (i, j, k) and the fractions (f_r, f_g, f_b).  Tetrahedral (the default): the three fractions sorted descending
 *     by a stable sort - ties keep r before g before b - are a >= b >= c on the axes A, B, C;
 *       P0 = V(i, j, k); P1 = P0's neighbour one step along A; P2 = P1's one step along B; P3 = V(i + 1, j + 1, k + 1)
 *       out = ((P0 + a (P1 - P0)) + b (P2 - P1)) + c (P3 - P2)       per output channel
 *     FF_GRADE_TRILINEAR: ff_texture's form, each lerp A + f (B - A): four along r (at (j, k), (j + 1, k), (j, k + 1),
 *     (j + 1, k + 1)), two along g (at k and k + 1) of those, one along b.
 * Consequences.  Both forms return a constant lattice's value bit for bit (a lattice of -0 returns +0), and the lattice value
 * exactly where every fraction is 0; constant curves return their value likewise.  A value outside the curve's or the lattice's
 * range reads as the nearest end.  Negative values and -0 go the ordinary way.
 * Special pixels.  A pixel with any channel that is not finite is copied to radiance_out bit for bit, whatever the flags; its bytes
 * follow the rule below.  What the stages produce is stored as it comes: a matrix that overflows gives Inf (and a saturation of
 * Inf - Inf, NaN).
 * rgb8 = trunc(clamp(out * 255)), the rule of every rgb8 output here (NaN -> 0).  rgb8 (W*H*3 bytes) and radiance_out (W*H*3
 * floats) may each be NULL.  radiance_out may be radiance_in itself (a pixel is read before it is written, as in ff_display); any
 * other overlap of an output with the input or the other output is refused.  Every size is 1 .. 65535.  Synchronous, on the
 * state's stream; host buffers are staged.  The call leaves FfStats, the stored primary hits and their key, every filter's
 * history, the display exposure and the progressive and adaptive sums as they were.  FF_ERR_INVALID_ARG, naming the field, before
 * any device work for: a NULL state, params or radiance_in; a size outside 1 .. 65535; unknown flags or a nonzero reserved; a
 * matrix, offset or saturation that is not finite, or a negative saturation (checked whether or not FF_GRADE_PRIMARY is set);
 * FF_GRADE_CURVES or FF_GRADE_LUT3D with a lut_id that names no LUT, or one whose LUT lacks that half; a refused overlap.
 * The kernels keep a lattice of N <= 17 in LDS (FF_GRADE_NO_LDS in the environment at ff_create: never) and larger ones in
 * global memory; the bits are the same.
 * Not offered: other channel counts, a per-channel curve axis, shaper curves stored inside a 3D .cube, lattices that are not cubes,
 * a row pitch, a grade fused into ff_display. */
FF_API int ff_color_grade(FfState* state, const FfGradeParams* p, int width, int height,
                          const float* radiance_in, int input_on_device,
                          void* rgb8, int rgb8_on_device, float* radiance_out, int radiance_out_on_device);

/* Host-only twin (no GPU, no state, host pointers), compiled from the same inline per-pixel functions the kernels use: the
 * descriptor itself in place of lut_id (NULL: none; p->lut_id is not looked at), the same checks - ff_grade_lut_create's on the
 * descriptor -, the same bits. */
FF_API int ff_color_grade_host(const FfGradeParams* p, const FfGradeLut* lut, int width, int height, const float* radiance_in,
                               unsigned char* rgb8, float* radiance_out);

/* .cube files, the text format of Adobe and Resolve: lines of
 *   TITLE "text"  |  DOMAIN_MIN r g b  |  DOMAIN_MAX r g b  |  LUT_1D_SIZE K  |  LUT_3D_SIZE N  |  r g b
 * with '#' comments and blank lines anywhere and LF or CRLF line ends; exactly one of the two sizes, before the first data line;
 * the domain defaults to 0 0 0 .. 1 1 1; K or N^3 data lines, for 3D red fastest.  ff_load_cube fills *out: a 1D file becomes the
 * three curves on FF_GRADE_AXIS_LINEAR over curve_lo .. curve_hi (its DOMAIN_MIN and DOMAIN_MAX must be the same for r, g and b), a
 * 3D file the lattice; out->lut is then what ff_grade_lut_create and ff_color_grade_host take.  The arrays are malloc'ed by the
 * library: release with ff_free_cube (which leaves *file empty; a NULL or empty one is fine).  FF_ERR_IO for a file that cannot be
 * opened or that ends before its last data line; FF_ERR_INVALID_ARG, naming the line, for a NULL argument, an unknown keyword, a
 * malformed line, a missing, repeated or late size, a size outside 2 .. 4096 (1D) or 2 .. 65 (3D), a value that is not finite,
 * a domain that is not min < max, or more data lines than the size says. */
FF_API int ff_load_cube(const char* path, FfCubeFile* out);
FF_API void ff_free_cube(FfCubeFile* file);
/* Writes `file` - exactly one half of file->lut, curves on FF_GRADE_AXIS_LINEAR or the lattice, under ff_grade_lut_create's
 * checks - with every number as %.9g, so that ff_load_cube returns the same bits.  A title may not hold '"' or a line end.
 * FF_ERR_IO when the file cannot be written. */
FF_API int ff_save_cube(const char* path, const FfCubeFile* file);

/* ---- lens (radial distortion, lateral chromatic aberration, vignetting) --------------------------- */

/* Defaults, the identity: k1 = k2 = k3 = 0, center 0 0, zoom 1, ca_red = ca_blue = 0, vignette 0, vignette_falloff 0,
 * FF_LENS_UNDISTORT, FF_LENS_CATMULL_ROM, FF_LENS_BORDER_BLACK, FF_LENS_ANTI_RING, reserved 0. */
FF_API void ff_lens_params_init(FfLensParams* p);

/* The lens: bends a W x H float3 radiance image the way a real lens does (FF_LENS_DISTORT: the render cut against footage, fed
 * to a head-mounted or projector optic) or straightens a plate the way the render is (FF_LENS_UNDISTORT), with the two other lens
 * effects a compositor expects, lateral chromatic aberration and vignetting.  A pure image operation like ff_sharpen: no scene, no
 * G-buffer, no history.  It sits after ff_taa / ff_sharpen / ff_motion_blur / ff_depth_of_field and before ff_color_grade /
 * ff_local_tonemap / ff_display; G-buffer, motion and id planes are not warped, so the stages that need them come first.  It is a
 * gather: every output pixel computes where in the source each of its channels comes from and resamples there.
 * THE TABLES, on the host, in double (ff_lens_tables returns them), every formula evaluated left to right as written.
 *   cx = 0.5f * float(W) + center_x, cy likewise (float; the optical centre c in pixels, pixel (x, y) having its centre at
 *   (x + 0.5, y + 0.5)); D2 = 0.25 (W W + H H), the square of half the diagonal: lengths are normalised by it, so r^2 = 1 at the
 *   corners of a centred image and no square root is taken per pixel.  r2_max = the largest ((dx dx + dy dy) / D2) of the four
 *   corner pixels' centres, (dx, dy) their offsets from c; at least 2^-20.
 *   The radial model is Brown-Conrady: d(t) = 1 + k1 t + k2 t t + k3 t t t, f(s) = s d(s s) the lens's radius of the ideal radius s.
 *   Knot j = 0 .. FF_LENS_KNOTS: r2 = r2_max j / FF_LENS_KNOTS; r = sqrt(r2); rho = r / zoom (zoom magnifies the output about c);
 *     FF_LENS_UNDISTORT  the output is the ideal image, the source the lens's: src = f(rho)
 *     FF_LENS_DISTORT    the output is what the lens with these coefficients records of the rectilinear source: src = the s with
 *                        f(s) = rho (Newton inside a bisection bracket, to the last bit that moves)
 *     e_j = float(src / r - 1), and for j = 0 float(1 / zoom - 1): the source radius over the output radius, less 1
 *     R = rho (DISTORT) or src (UNDISTORT): the radius in the LENS's image, where the vignette lives;
 *     v = 1 / (c c) with c = 1 + (vignette_falloff R) (vignette_falloff R) - cos^4 of the field angle, the natural law;
 *     gain = (1 - vignette) + vignette v;  g_j = float(gain) under DISTORT, which adds the vignette, float(1 / gain) under
 *     UNDISTORT, which removes it.  vignette = 0 gives a table of exact 1.0f; no distortion and zoom 1 give e_j = 0 exactly.
 *   f must rise strictly on the range the image needs - [0, sqrt(r2_max) / zoom] under UNDISTORT, up to where it reaches that under
 *   DISTORT -, or the image would fold over: f'(s) = 1 + 3 k1 t + 5 k2 t t + 7 k3 t t t (t = s s) is tested through its exact
 *   extrema, and such parameters are refused with FF_ERR_INVALID_ARG and a message naming the radius of the fold.
 * PIXELS.  All arithmetic is float32 + - * and floor with no fused multiply-add, every formula evaluated as parenthesised;
 * min(a, b) is b < a ? b : a and max(a, b) is a < b ? b : a; lerp(a, b, t) = a + t * (b - a).  Per output pixel (x, y):
 *   1 radial   px = float(x) + 0.5, py likewise; dx = px - cx, dy = py - cy; r2 = ((dx dx) + (dy dy)) * float(1 / D2);
 *              u = min(r2 * float(FF_LENS_KNOTS / r2_max), FF_LENS_KNOTS); i = min(int(floor(u)), FF_LENS_KNOTS - 1); t = u - float(i);
 *              e = lerp(e_i, e_i+1, t), g = lerp(g_i, g_i+1, t): one floor, one fraction, one linear interpolation each
 *   2 source   per channel, q = ca_red for red, 0 for green, ca_blue for blue (the channel's magnification against green):
 *              ec = (e + q) + (e * q), which is (1 + e)(1 + q) - 1; sx = px + (dx * ec), sy = py + (dy * ec): the displacement form,
 *              so that e = 0 and q = 0 give (px, py) exactly.  When both q are 0 the three channels share one position and one set
 *              of taps
 *   3 border   FF_LENS_BORDER_BLACK: a channel whose (sx, sy) is not inside [0, W] x [0, H] is 0, and step 4 is skipped for it.
 *              Otherwise, and under FF_LENS_BORDER_CLAMP always, sx = sx > 0 ? min-of(sx, W) : 0 and sy likewise - edge replication
 *   4 resample ux = sx - 0.5; ix = floor(ux); fx = ux - ix; uy, iy, fy likewise.  Tap (i, j) reads pixel (clamp(ix + i, 0, W - 1),
 *              clamp(iy + j, 0, H - 1)); a non-finite tap reads as +0, as in ff_resize.
 *              FF_LENS_BILINEAR: i, j in 0 .. 1; v = lerp(lerp(v00, v10, fx), lerp(v01, v11, fx), fy).
 *              FF_LENS_CATMULL_ROM: i, j in -1 .. 2, 4 x 4 taps, the weights ff_taa's history resampling uses, for fraction t:
 *              w_-1 = ((-t3 + 2 t2) - t) 0.5, w_0 = ((3 t3 - 5 t2) + 2) 0.5, w_1 = ((-3 t3 + 4 t2) + t) 0.5, w_2 = (t3 - t2) 0.5
 *              (t2 = t t, t3 = t2 t).  Rows first, taps in the order of i: row_j = (((wx_-1 v_-1j) + (wx_0 v_0j)) + (wx_1 v_1j)) +
 *              (wx_2 v_2j); then v = (((wy_-1 row_-1) + (wy_0 row_0)) + (wy_1 row_1)) + (wy_2 row_2).  With FF_LENS_ANTI_RING lo and
 *              hi are the min and max of the inner taps v_00, v_10, v_01, v_11 taken in this order, and v = min(max(v, lo), hi):
 *              radiance stays >= 0 beside an HDR edge.  Without the flag the negative lobes may produce NEGATIVE radiance.
 *              Under either filter a position on a pixel's centre (fx = 0 and fy = 0) returns that tap v_00 itself
 *   5 gain     out = v * g, per channel; rgb8 = trunc(clamp(out * 255)), the rule of every rgb8 output here.
 * Consequences.  The defaults return a finite image bit for bit, -0 included (a non-finite value comes back as +0).  Under CLAMP
 * with ANTI_RING or BILINEAR a constant finite image comes back bit for bit under any geometry (a constant -0 may return as +0).
 * The green channel does not depend on ca_red and ca_blue.  No geometry and a vignette give the input times g.  Minification is
 * NOT filtered - one set of taps per channel whatever the local scale: for coefficients that compress the corners strongly,
 * render larger and ff_resize afterwards.
 * rgb8 (W*H*3 bytes) and radiance_out (W*H*3 floats) may each be NULL.  Neither may overlap the input - this is a gather - and the
 * two may not overlap each other.  Width and height are 1 .. 65535.  Synchronous, on the state's stream; host buffers are staged.
 * The call leaves FfStats, the stored primary hits and their key, every filter's history, the display exposure and the progressive
 * and adaptive sums as they were, and ff_upload_scene resets nothing of it; its own state is the staging buffer and the device
 * table with its key (k1, k2, k3, center, zoom, vignette, vignette_falloff, direction, W, H) - rebuilt and uploaded only when the
 * key changes -, allocated on first use and freed by ff_destroy.  FF_ERR_INVALID_ARG, naming the field, before any device work,
 * in this order, for: a NULL state or params; a bad size; a k outside -10 .. 10, |center_x| > W/2, |center_y| > H/2, a zoom
 * outside 1/16 .. 16, a ca outside -0.25 .. 0.25, a vignette outside 0 .. 1, a vignette_falloff outside 0 .. 8, or any of them
 * not finite; an unknown direction, filter or border; a nonzero reserved; unknown flags; coefficients that fold the image over;
 * a NULL radiance_in; an output that overlaps the input or the other output.
 * Not offered: tangential (decentering) terms, fisheye and other projections (a host-only addition to the tables), filtered
 * minification, film grain, a `lens` statement in the scene file, warping of G-buffer planes, a multi-GPU twin. */
FF_API int ff_lens(FfState* state, int width, int height, const FfLensParams* p,
                   const float* radiance_in, int input_on_device,
                   void* rgb8, int rgb8_on_device, float* radiance_out, int radiance_out_on_device);

/* Host-only twin (no GPU, no state, host pointers), compiled from the same inline per-pixel functions the kernel uses: the same
 * image arguments, the same checks, the same bits. */
FF_API int ff_lens_host(int width, int height, const FfLensParams* p, const float* radiance_in,
                        unsigned char* rgb8, float* radiance_out);

/* The two tables as the kernel gets them: out_e and out_gain, FF_LENS_KNOTS + 1 floats each, and r2_max; each output may be NULL.
 * The checks are ff_lens's for the size and the parameters. */
FF_API int ff_lens_tables(const FfLensParams* p, int width, int height, float* out_e, float* out_gain, double* out_r2_max);

/* The source positions of n output positions (xy_out, xy_src: n pairs x y, in pixels, a pixel's centre at + 0.5) for `channel`
 * 0 = red, 1 = green, 2 = blue, through steps 1 and 2 as ff_lens runs them, before the border rule: what a viewer needs to pick
 * through a distorted frame.  A position beyond r2_max reads the tables' last knot.  The checks are ff_lens's for the size and
 * the parameters; every xy_out must be finite. */
FF_API int ff_lens_map_host(const FfLensParams* p, int width, int height, int channel, const float* xy_out, int n, float* xy_src);

/* The zoom that fits the frame, for the other parameters as given (p->zoom is not read), computed in double from the model along
 * the image border.  FF_LENS_FIT_FILL: the smallest zoom at which no output pixel's green position leaves the source, so that no
 * border shows, times 1 + 1e-4.  FF_LENS_FIT_ALL: the largest zoom at which the whole source - every point of its edge - stays
 * in view, times 1 - 1e-4.  The margin covers the float arithmetic and the tables of steps 1 and 2.  FF_ERR_INVALID_ARG for
 * ff_lens's parameter checks, an unknown mode, a NULL out_zoom, a fold-over that hides the source's edge (ALL), or a fitting zoom
 * outside 1/16 .. 16. */
FF_API int ff_lens_fit_zoom(const FfLensParams* p, int width, int height, int mode, float* out_zoom);

/* How often this state has built and uploaded ff_lens's table (tests: it is rebuilt only when its key changes). */
FF_API int ff_debug_lens_table_builds(FfState* state, uint64_t* out_builds);

/* ---- measurement -------------------------------------------------------------------------------- */

/* Turn per-launch node/triangle visit counters on (1) or off (0, default).  Ray counting is always on. */
FF_API int ff_set_collect_stats(FfState* state, int on);
FF_API int ff_stats(FfState* state, FfStats* out);

/* Name of the trace-kernel instantiation the last frame launched, spelled as rocprofv3 prints it ("" before the first frame). */
FF_API const char* ff_debug_kernel_name(FfState* state);

/* The layout the next BVH launch on the uploaded scene will use (tests), out8 = workgroup size of the trace kernel (0: the trees are too
 * deep for any), traversal-stack entries per lane, how many of them live in LDS, LDS node slots in use, setup threshold, leaf threshold,
 * depth of the deepest 4-wide mesh tree, depth of the tree over the geometries (0: none).  FF_ERR_NO_SCENE before an upload. */
FF_API int ff_debug_layout(FfState* state, int* out8);

/* The global spill area of the traversal stacks (tests).  reset != 0: fill it, if there is one, with a word that no stack entry can
 * equal.  reset == 0: *words = how many of its words differ from that word now (0 where there is no area).  A launch may reallocate the
 * area when it needs a larger one: reset it after a first launch of the same size, then launch again and count. */
FF_API int ff_debug_stack_spill(FfState* state, int reset, unsigned long long* words);

/* Raw device counters of the last instrumented render (ff_set_collect_stats(1)), 28 values: [0] rays [1] inner-node
 * visits [2] triangle tests [3] plane tests (all summed over lanes) [8] inner-step rounds [9] leaf rounds [10] triangle
 * rounds [11] plane rounds [12] segment rounds (wave-level executions of each phase): lanes / (64 * rounds) is the SIMD
 * occupancy of that phase; [4..7],[13] wave cycles spent in resolve / shade / acquire / begin / traverse; [14] plane-only queries [15] exact plane
 * tests; [16..18] wave cycles in mesh starts / inner-node phases / leaf phases; [19..21] the three parts of the begin phase; [22] the
 * slowest wave's loop cycles; [23..25] 100 MHz wall clock, complemented / complemented / plain: first lane to find the work
 * queue empty, first wave start, last wave end; [28..30] wave cycles of the leaf visits spent waiting for the
 * triangle records / in the triangle tests / in the pop that follows. */
FF_API int ff_debug_counters(FfState* state, unsigned long long* out32);

/* With FF_DEBUG_TIMELINE_US=<bucket> in the environment at ff_create, instrumented renders also count the rays that complete in
 * each bucket of the (first) launch's wall clock: 1 024 buckets from the start of the first wave, the last one open-ended.
 * *bucket_us comes back 0 when the histogram is off. */
FF_API int ff_debug_timeline(FfState* state, unsigned* out1024, int* bucket_us);

/* Self-check of the kernels' arithmetic: their correctly rounded 1/x and sqrt(x) against the compiler's IEEE expansions on
 * every one of the 2^32 float bit patterns; out_mismatches2[0] / [1] must come back 0 (a few milliseconds). */
FF_API int ff_debug_check_ieee(FfState* state, unsigned long long* out_mismatches2);
/* The experiment switches (FF_NO_PRIMARY_REUSE, FF_NO_LAST_BOUNCE_CUT, FF_NO_WALL_TABLE, FF_POOL, ...) are read from the
 * environment once, at ff_create; this re-reads them for `state` (A/B tests that flip a switch between two frames of one state).
 * Layout switches take effect at the next upload or transform update. */
FF_API int ff_debug_reload_switches(FfState* state);

/* ---- mesh loading (next-row scope: LoadMesh, utilities.h:781-840) ------------------------------- */

/* Reads a Wavefront OBJ with LoadMesh's semantics: one FfTriangle per face from the face's first three
 * indexed vertices; missing vt/vn yield zeros instead of the reference's out-of-bounds read.
 * *out_triangles is malloc'ed by the library; release with ff_free_triangles. */
FF_API int ff_load_obj(const char* path, FfTriangle** out_triangles, int* out_count);
FF_API void ff_free_triangles(FfTriangle* triangles);

/* ---- scene description file (next-row scope: the reference's "TODO: Load scene from file", kernel.cu:261) -------- */

/* A scene file replaces the literals of kernel.cu:227-259 (geometries, BXDFs) and kernel.cu:311-321 (camera).  Plain text,
 * one statement per line, '#' starts a comment:
 *
 *   camera position X Y Z yaw DEG pitch DEG fov DEG near N far F            (every key optional: kernel.cu:312-321 defaults)
 *          [aperture R] [focus F] [filter corner|box]                       (ff_set_camera_sampling's lens_radius, focus_distance
 *                                                                             and pixel_filter; what it would refuse - a
 *                                                                             focus <= 0 only beside an aperture > 0 - is
 *                                                                             FF_ERR_INVALID_ARG naming the line)
 *   bxdf NAME diffuse|emitter|mirror|glass [albedo R G B] [specular R G B] [transmittance R G B] [ior N] [color R G B] [intensity I]
 *                                            [roughness R]                  (mirror only, R in [0, 1]; anything else is
 *                                                                             FF_ERR_INVALID_ARG naming the line)
 *   mesh FILE.obj [position X Y Z] [rotation X Y Z] [scale X Y Z] bxdf NAME (path relative to the scene file)
 *   plane [position X Y Z] [rotation X Y Z] [scale X Y Z] bxdf NAME
 *   sphere radius R [position X Y Z] [rotation X Y Z] [scale X Y Z] bxdf NAME
 *   environment FILE.hdr [intensity I] [rotation DEG]                       (at most one; path relative to the scene file;
 *                                                                             intensity 1 and rotation 0 by default)
 *   texture NAME FILE.(hdr|ppm) [srgb] [clamp] [nearest]                    (path relative to the scene file; names are unique;
 *                                                                             srgb: the .ppm's bytes are sRGB-encoded)
 *   ... and on mesh, plane and sphere statements, before or after `bxdf NAME`:  [albedo_map NAME [scale U V] [offset U V]]
 *                                                                            (a texture statement earlier in the file)
 *
 * Geometries keep file order (it is the reference's iteration order, kernel.cu:133).  The returned object owns the
 * triangles and BXDFs its FfGeometry array points to. */
typedef struct FfSceneFile FfSceneFile;
FF_API int ff_scene_file_load(const char* path, FfSceneFile** out_scene);
FF_API const FfGeometry* ff_scene_file_geometries(const FfSceneFile* scene, int* out_count);
/* Camera of the file for a width x height image (UpdateBasisAxis applied). */
FF_API int ff_scene_file_camera(const FfSceneFile* scene, int width, int height, FfCamera* out_camera);
FF_API void ff_scene_file_free(FfSceneFile* scene);
/* The file's environment statement: 1 with the resolved path (owned by the scene), intensity and rotation in degrees; 0 if the
 * file has none (the outputs are left alone).  Loading the map and ff_set_environment are the caller's. */
FF_API int ff_scene_file_environment(const FfSceneFile* scene, const char** out_path, float* out_intensity, float* out_rotation_deg);
/* The file's texture statements: their number, and statement `index`: name and resolved path (owned by the scene) and flags
 * (FF_TEX_* bits; bit 8, FF_SCENE_TEX_SRGB, for `srgb`).  Loading the image and ff_texture_create are the caller's. */
#define FF_SCENE_TEX_SRGB 256
FF_API int ff_scene_file_texture_count(const FfSceneFile* scene);
FF_API int ff_scene_file_texture(const FfSceneFile* scene, int index, const char** out_name, const char** out_path, int* out_flags);
/* The albedo_map of geometry `geometry_index`: 1 with the index of its texture statement, scale and offset (2 floats each; 1 1 and
 * 0 0 by default); 0 if the geometry has none (the outputs are left alone).  ff_set_albedo_texture is the caller's. */
FF_API int ff_scene_file_albedo_map(const FfSceneFile* scene, int geometry_index, int* out_texture, float* out_scale2, float* out_offset2);
/* The `roughness` of geometry `geometry_index`'s bxdf: 1 with the value; 0 if it has none (or 0: the output is left alone).
 * ff_set_roughness is the caller's. */
FF_API int ff_scene_file_roughness(const FfSceneFile* scene, int geometry_index, float* out_roughness);
/* The camera statement's `aperture`, `focus` and `filter` keys: 1 with the setting they describe (keys not given keep
 * ff_camera_sampling_init's values); 0 if none of them was given (the output is left alone).  ff_set_camera_sampling is the caller's. */
FF_API int ff_scene_file_camera_sampling(const FfSceneFile* scene, FfCameraSampling* out);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* FIREFLY_FF_API_H */
