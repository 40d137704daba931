// ff_state.h — the tracer state behind the opaque FfState handle and the internal render steps shared by the
// translation units of the library (ff_api.cpp: the handle's lifetime and measurement; ff_scene_api.cpp: the scene on the device;
// ff_render_api.cpp: the single-device render entry points; ff_frame.cpp: one frame; ff_dist.cpp: multi-GPU entry points;
// ff_adaptive_api.cpp: ff_render_adaptive; the image-space *_api.cpp files, whose own state is described in ff_image.h).
#pragma once

#include <vector>

#include <hip/hip_runtime.h>

#include "ff_build.h"
#include "ff_image.h"
#include "ff_internal.h"
#include "ff_kernels.h"
#include "ff_texture.h"

struct FfDistContext; // ff_dist.cpp

struct FfState {
    int device = 0;
    int num_cus = 0;
    size_t device_mem_bytes = 0; // total global memory of the device (caps the buffers the library allocates on its own initiative)
    hipStream_t stream = nullptr;
    // scene (device)
    ff::GeomRecord* d_geoms = nullptr;
    ff::TriRecord* d_tris = nullptr;
    ff::TriNormals* d_normals = nullptr; // vertex normals, parallel to d_tris
    ff::TriUVs* d_uvs = nullptr;         // vertex UVs, parallel to d_tris (read only where an albedo texture is bound)
    // Normal tables (KParams::tri_world_normals / geom_world_normals; scenes of up to kChunkGeometries geometries, null otherwise): one
    // allocation of the upload, num_tris entries parallel to d_tris, then num_geoms parallel to d_geoms.  Rewritten by finalize_layout,
    // which every change of the scene ends with (upload, ff_update_transforms, ff_update_mesh).
    float4* d_world_normals = nullptr;
    ff::BvhNode* d_nodes = nullptr;   // binary trees: what the builders write and refit works on
    ff::WallTable walls = {};          // the axis-aligned planes among the records every query screens (finalize_layout)
    int num_scan = 0;                  // big scenes: leading plane records kept out of the geometry tree (count_scan_planes)
    ff::Bvh4Node* d_nodes4 = nullptr; // 4-wide trees derived from them (gpu_collapse_mesh): what the trace kernels traverse;
                                      // mesh i's nodes start at its binary slot's index (slots[i].node_first)
    int num_geoms = 0, num_planes = 0, num_quads = 0, num_nodes = 0, max_depth = 0;
    int num_nodes4 = 0, max_depth4 = 0;   // 4-wide nodes in use (sum over meshes), deepest 4-wide tree
    // scenes of more than kChunkGeometries geometries: the 4-wide tree over the geometries' world boxes, kept in d_nodes4
    // from index node_capacity on (0 nodes: a small scene)
    int top_count = 0, top_depth = 0, top_lds_count = 0;
    int stack_entries = 1;                // traversal stack entries per lane the BVH kernels need for this scene
    int stack_lds_levels = 1;             // ... of which this many live in LDS (finalize_layout); the rest in d_stack_spill
    unsigned long long* d_cull_mask = nullptr; // primary-ray cull: one bit per pixel item (KParams::cull_mask)
    size_t cull_mask_bytes = 0;
    float4* d_primary_cache = nullptr; // KParams::primary_cache
    size_t primary_cache_bytes = 0;
    // The start records that go with the stored hits (KParams::start_records): kept under the same rule, and only for the bounce
    // count and shade mode they were classified for
    float4* d_start_records = nullptr;
    size_t start_records_bytes = 0;
    bool primary_has_start = false;
    int start_bounces = 0, start_shade = 0;
    // The stored primary hits (and the mask of pixels that see nothing) belong to a camera, a pixel mapping and a scene: while those
    // stay what they were - a viewer that accumulates 1-spp frames with the camera at rest (kernel.cu:266,342) - the next frame starts
    // from them without a pre-pass.  primary_key: what they were computed for; any change of the scene clears primary_valid.
    struct PrimaryKey {
        float cam[24];
        int dims[12];
        unsigned pix_items;
    } primary_key = {};
    bool primary_valid = false;
    PrimaryKey last_key = {};                // the key of the frame before this one, stored hits or not ("has the camera come to rest?")
    bool last_key_valid = false;
    bool primary_has_mask = false;           // ... and d_cull_mask holds the mask that goes with them
    unsigned long long primary_culled_pixels = 0; // pixels marked in it (FfStats::rays_answered of frames that reuse it)
    bool pending_mask_reused = false, pending_mask_built = false;
    float4* d_park = nullptr;          // KParams::park (job-pool kernel)
    size_t park_bytes = 0;
    int* d_stack_spill = nullptr;         // (stack_entries - stack_lds_levels) x launch threads ints
    size_t stack_spill_bytes = 0;
    bool use_pool = false;                    // the scene renders with the job-pool kernel (finalize_layout): its LDS layout leaves room for the pool
    int scene_block_threads = 0, lds_cap = 0; // BVH kernel workgroup size and LDS node slots chosen for this scene (finalize_layout)
    bool has_specular = false;
    uint64_t num_tris = 0;
    bool has_scene = false;
    // scene bookkeeping for updates (ff_update_transforms / ff_update_mesh)
    struct MeshSlot {
        int node_first = 0, node_count = 0, node_capacity = 0, depth = 0;
        int node4_count = 0, depth4 = 0; // its 4-wide tree: nodes [node_first, node_first + node4_count) of d_nodes4
        bool parents_linked = false;
    };
    int builder = FF_BUILD_HOST_SAH;       // builder for the next upload (ff_set_builder)
    int scene_builder = FF_BUILD_HOST_SAH; // builder that produced the scene on the device
    std::vector<ff::GeomRecord> h_geoms;       // the uploaded records, processing order
    std::vector<MeshSlot> slots;           // parallel to h_geoms (meshes only)
    size_t node_capacity = 0;              // nodes allocated in d_nodes
    int* d_parent = nullptr;               // node_capacity ints (refit)
    unsigned char* d_role = nullptr;       // node_capacity bytes: which binary nodes are 4-wide nodes (gpu_collapse_mesh keeps it across refits)
    FfTriangle* d_stage = nullptr;         // staging copy of a caller triangle array (device builder / refit)
    size_t stage_bytes = 0;
    ff::BuildScratch scratch;
    FfBuildStats build_stats = {};
    // work buffers (device)
    float* d_blocksums = nullptr;
    size_t blocksums_bytes = 0;
    // where a render call's outputs go when the caller gave host buffers (ff::RenderOutputs): filled and copied back within the call
    unsigned char* d_rgb8 = nullptr;
    size_t rgb8_bytes = 0;
    float* d_radiance = nullptr;
    size_t radiance_bytes = 0;
    // fine-grained tail (KParams::tail_samples)
    float4* d_tail_samples = nullptr;
    size_t tail_samples_bytes = 0;
    bool tail_forced = false; // FF_TAIL_GROUP given: the fine-grained tail also for one-part frames
    int tail_min_blocks = 4;  // launches with fewer sample blocks keep whole-block items (FF_TAIL_MIN_BLOCKS)
    int tail_group_spp = 8;  // FF_TAIL_GROUP (0 = off): samples per tail item of a multi-part frame.  8 since the samples start from stored hits (r04: eight ranks +0.5, four +0.7 points; rounds 2-3: 16)
                             // (slowest of 8 ranks at 95.6 % of full-frame time / 8 instead of 93.8 %, of 4 ranks 97.4 / 96.7: tools/strip_scaling.py)
    // progressive accumulation (ff_render_progressive)
    float* d_accum = nullptr;
    size_t accum_bytes = 0;
    float* d_frame = nullptr;
    size_t frame_bytes = 0;
    int accum_width = 0, accum_height = 0, accum_frames = 0;
    // The image work buffer, the one device buffer every image-space entry point (ff_gbuffer, the denoisers, ff_taa*, ff_upscale,
    // ff_display, ff_motion_blur, ff_depth_of_field, ff_despeckle, ff_sharpen, ff_local_tonemap, ff_interpolate, ff_encode_yuv,
    // ff_resize, ff_color_grade, ff_lens) works in: the running entry point's own scratch at the head (counts, grids, a packed plane, the bloom pyramid; each
    // *_api.cpp says what), the staging of host buffers behind it (ff::Staging).  Grown on demand, and nothing in it outlives the
    // call that put it there.  Not reset by uploads.
    void* d_img_work = nullptr;
    size_t img_work_bytes = 0;
    // G-buffer and denoiser (ff_gbuffer / ff_denoise, ff_image_api.cpp, ff_denoise.hip): ff_gbuffer's own primary hits ([3][pix_items]
    // float4, never the frame's d_primary_cache), the filter's packed guides and its two colour buffers
    float4* d_gb_hits = nullptr;
    size_t gb_hits_bytes = 0;
    float4* d_dn_work = nullptr; // 4 float4 per pixel: guide_pos, guide_nrm, colour 0, colour 1
    size_t dn_work_bytes = 0;
    // The reprojection histories (ff_image.h).  ff_denoise_temporal (ff_temporal.hip): two sets of 4 float4 per pixel (guide position
    // and class, unit normal, colour history, moments {l, l^2, len}), then the two working colour buffers and the motion (float2 per
    // pixel).  ff_taa (ff_taa.hip): two buffers of one float4 per pixel {rgb, len}, then the motion.  ff_taa_upscale
    // (ff_taa_upscale.hip): ff_taa's layout on the high grid; its history also belongs to the low size of the call that wrote it.
    enum { kHistoryTemporal = 0, kHistoryTaa = 1, kHistoryTaaUpscale = 2 };
    ff::ReprojectionHistory history[3];
    int taa_upscale_lo_width = 0, taa_upscale_lo_height = 0;
    // sub-pixel jitter of the primary rays (ff_set_pixel_jitter): composed into the ray matrix of ff_render* and ff_gbuffer
    float jitter_x = 0.f, jitter_y = 0.f;
    // Per-sample camera rays (ff_camera.cpp, ff_set_camera_sampling): belongs to the state, like the jitter, so it outlives uploads and
    // updates of the scene.  While it is active (cam_active), FF_SHADE_DIFFUSE_PATH and FF_SHADE_DIFFUSE_PATH_NEE frames run
    // nee_path_kernel with NeeParams::cam_active set, and a box frame's ray matrix is the unjittered one.
    FfCameraSampling cam_sampling = { FF_PIXEL_CORNER, 0.f, 1.f, 0 };
    bool cam_active() const { return cam_sampling.pixel_filter == FF_PIXEL_BOX || cam_sampling.lens_radius > 0.f; }
    // Next-event estimation (ff_nee.cpp): what the light table is built from - the uploaded geometries (caller order) with their
    // materials and, for meshes, the object-space triangles kept since the upload or the last ff_update_mesh - and the device table
    std::vector<FfGeometry> nee_geoms;
    std::vector<FfBXDF> nee_bxdfs;
    std::vector<std::vector<FfTriangle>> nee_tris;
    bool nee_valid = false;            // the device table belongs to the uploaded scene (scenes uploaded compiled have none)
    int nee_num_lights = 0;
    float4* d_nee_lights = nullptr;    // ff::NeeParams::lights
    size_t nee_lights_bytes = 0;
    float* d_nee_pdf = nullptr;        // ff::NeeParams::light_pdf
    size_t nee_pdf_bytes = 0;
    // Environment light (ff_env.cpp, ff_set_environment): belongs to the state, so it outlives uploads and updates of the scene.
    // While it is set, FF_SHADE_DIFFUSE_PATH and FF_SHADE_DIFFUSE_PATH_NEE frames run nee_path_kernel<..., ENV = 1>.
    bool env_set = false;
    bool env_sampled = false;          // the map's total luminance is positive (else its table is empty: no environment light samples)
    int env_w = 0, env_h = 0;
    float env_rotation = 0.f;          // radians, in [0, 2 pi)
    float4* d_env_texels = nullptr;    // ff::NeeParams::env_texels
    size_t env_texels_bytes = 0;
    float2* d_env_alias = nullptr;     // ff::NeeParams::env_alias
    size_t env_alias_bytes = 0;
    float* d_env_z = nullptr;          // ff::NeeParams::env_z
    size_t env_z_bytes = 0;
    // Albedo textures (ff_texture.cpp).  Textures belong to the state (id = index into `textures`; d_texels null: a free id); bindings
    // belong to the scene (one per CALLER geometry index; an upload drops them).  The device tables - one TexBinding per record in
    // processing order, one TexDesc per id - are rewritten whenever either changes.  While tex_bound > 0, FF_SHADE_DIFFUSE_PATH and
    // FF_SHADE_DIFFUSE_PATH_NEE frames run nee_path_kernel<..., TEX = 1> and ff_gbuffer's resolve reads the tables.
    struct Texture {
        float4* d_texels = nullptr;
        int w = 0, h = 0, flags = 0;
    };
    std::vector<Texture> textures;
    std::vector<ff::TexBinding> tex_bindings; // per caller geometry index (tex < 0: none)
    int tex_bound = 0;                        // bindings in force
    ff::TexBinding* d_tex_bind = nullptr;
    size_t tex_bind_bytes = 0;
    ff::TexDesc* d_tex_desc = nullptr;
    size_t tex_desc_bytes = 0;
    // Rough-specular mirrors (ff_glossy.cpp, ff_set_roughness).  Bindings belong to the scene (one roughness per CALLER geometry index,
    // 0: none; an upload drops them).  A binding is APPLIED while its geometry's record is FF_BXDF_MIRROR; glossy_applied counts them.
    // The device table - one alpha = roughness^2 per record in processing order, 0 where nothing is applied or alpha < 1e-3 - is
    // rewritten whenever a binding or the records' materials change.  While glossy_applied > 0, FF_SHADE_DIFFUSE_PATH and
    // FF_SHADE_DIFFUSE_PATH_NEE frames run nee_path_kernel<..., GLOSSY = 1>.
    std::vector<float> glossy_roughness;
    int glossy_applied = 0;
    float* d_glossy_alpha = nullptr; // ff::NeeParams::glossy_alpha
    size_t glossy_alpha_bytes = 0;
    // display transform (ff_display, ff_display.hip): the adapted exposure, the last call's results (ff_display_state) and the
    // 256 histogram counters and the 255 sRGB thresholds in d_disp_const.  Not reset by uploads.
    void* d_disp_const = nullptr;
    size_t disp_const_bytes = 0;
    bool disp_has_prev = false, disp_called = false;
    float disp_prev_exposure = 0.f;           // E of the last automatic call (the next one adapts from it)
    float disp_exposure = 0.f, disp_target = 0.f;
    uint32_t disp_histogram[256] = {};
    // adaptive sampling (ff_render_adaptive, ff_adaptive_api.cpp): the two running sums (W*H*3 floats each) and behind them the
    // compact rectangle a pass renders into; per tile the error, the pass count and the list of tiles to check; the staging of host
    // buffers (ff_adaptive_tile_error's inputs, the per-pixel pass counts).  The last call's grid and per-tile results stay for
    // ff_adaptive_state.  Reset per call; not reset by uploads.
    struct Adaptive {
        float* d_planes = nullptr;
        size_t planes_bytes = 0;
        void* d_tiles = nullptr;
        size_t tiles_bytes = 0;
        void* d_stage = nullptr;
        size_t stage_bytes = 0;
        bool valid = false;                   // a call has completed: the fields below describe it
        int width = 0, height = 0, tile = 0;
        std::vector<uint16_t> tile_passes;    // n_t per tile, row-major
        std::vector<float> tile_error;        // E_t of each tile's last check
    } adaptive;
    // video planes (ff_encode_yuv): the knot tables of the three transfers (ff_yuv.h kYuvKnotStride floats apart, each uploaded on
    // its first use).  Not reset by uploads.
    void* d_yuv_knots = nullptr;
    bool yuv_knots_loaded[3] = { false, false, false };
    // resampling (ff_resize): the intermediate image of the horizontal pass (W' x H float3) and, per axis (0: horizontal, 1:
    // vertical), the table uploaded last - first[out_size], then from a multiple of 16 bytes on the weights - with its key
    // (in_size, out_size, filter): rebuilt and uploaded only when the key changes.  Not reset by uploads.
    void* d_resize_mid = nullptr;
    size_t resize_mid_bytes = 0;
    struct ResizeTable {
        void* d_table = nullptr;
        size_t bytes = 0;
        bool valid = false;
        int in_size = 0, out_size = 0, filter = 0;
        int taps = 0, span = 0; // T, and for axis 0 the longest input span of a tile (ff_resize.h ResizeAxis)
    } resize_table[2];
    // colour grade (ff_color_grade, ff_grade_api.cpp): the LUT objects (id = index; neither device array: a free id).  d_table holds
    // the lattice as float4 texels, d_curves the 3 K knots; `desc` is the caller's descriptor without its pointers.  They belong to
    // the state: not reset by uploads.
    struct GradeLut {
        float4* d_table = nullptr;
        float* d_curves = nullptr;
        FfGradeLut desc = {};
    };
    std::vector<GradeLut> grade_luts;
    // lens (ff_lens, ff_lens_api.cpp): the device table of FF_LENS_KNOTS + 1 knots {e, gain} uploaded last, with its key - the
    // parameters that feed it (k1, k2, k3, center_x, center_y, zoom, vignette, vignette_falloff as bits; the direction) and the
    // image size: rebuilt and uploaded only when the key changes (`builds` counts how often).  Not reset by uploads.
    struct LensTable {
        void* d_table = nullptr;
        size_t bytes = 0;
        bool valid = false;
        struct Key {
            uint32_t f[8];
            int direction, width, height;
        } key = {};
        uint64_t builds = 0;
    } lens_table;
    unsigned* d_queue = nullptr;               // work-queue counter: lives right behind the counters (one memset clears both)
    unsigned long long* d_counters = nullptr;  // 28 counters + 4 queue words
    unsigned long long* h_counters = nullptr;  // pinned mirror for the per-frame read-back
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    bool collect_stats = false;
    // Experiment switches (DESIGN.md "knobs"): read from the environment ONCE, at ff_create (ff_debug_reload_switches re-reads them on
    // request: the A/B tests); the render and layout paths only look here, so a state behaves the same from frame to frame and no
    // getenv runs next to another thread's setenv.
    struct Switches {
        bool no_last_bounce_cut = false, no_primary_cull = false, no_primary_reuse = false; // per frame (render_enqueue)
        bool no_start_records = false; // FF_NO_START_RECORDS: every sample starts from the pixel's raw stored hit (the kernel without START)
        bool no_world_normals = false; // FF_NO_WORLD_NORMALS: the shading pass computes every hit's world normal (the kernels without WN)
        bool no_primary_cache = false; // FF_NO_PRIMARY_CACHE: every frame runs its own pre-pass (the stored hits are not kept from frame to frame)
        int tail_blocks = 0;           // FF_TAIL_BLOCKS: how many of the frame's last sample blocks go out as short items (0: the library's choice)
        int reuse_min_spp = 2;         // FF_REUSE_MIN_SPP: frames of fewer samples per pixel trace their primary rays themselves unless the hits are there
        int reuse_quorum = 1;
        int queue_chunk = 0, queue_counters = 0; // 0: the library's choice
        int queue_tail = -1;           // FF_QUEUE_TAIL: items per wave in the as-asked tail zone of the work queue (-1: the library's choice, 0: off)
        bool no_wall_table = false, no_wall_pairs = false, no_stack_spill = false, no_scan_planes = false; // layout (finalize_layout / scene compile)
        bool lds_fill = false;         // FF_DEBUG_LDS_FILL=words,pattern
        unsigned long lds_fill_words = 0, lds_fill_pattern = 0;
        int pool = -1;                 // FF_POOL: -1 the library's choice, 0 the lane-owned traversal kernel, 1 the job-pool kernel
        int pool_quorum = 0;           // FF_POOL_QUORUM: ready lanes a wave waits for before a setup pass (0: the library's choice)
        int pool_quorum_min = 0;       // FF_POOL_QUORUM_MIN: ... when the job queue is empty
        int pool_refill = 0;           // FF_POOL_REFILL: free lanes of a traversing wave that trigger a fetch of new jobs
        int pool_slice = 0;            // FF_POOL_SLICE: inner-node rounds per traversal slice
        int pool_batch_min = 0;        // FF_POOL_BATCH_MIN: jobs the queue must hold before a wave goes and takes some (fewer only after a few empty looks)
        int lds_node_cap = -1;         // FF_DEBUG_LDS_NODE_CAP: at most this many tree nodes in LDS (experiments on partial residency)
        int pool_leave = -1;           // FF_POOL_LEAVE: jobs a wave may still hold when it leaves the traverse role for a setup pass (they are put down)
        int pool_stack_levels = 0;     // FF_POOL_STACK_LEVELS: traversal stack levels kept in LDS (the deeper ones spill)
        bool grade_no_lds = false;     // FF_GRADE_NO_LDS: ff_color_grade reads every lattice from global memory
    } sw;
    int block_threads = ff::kBlockThreadsMax; // BVH kernel workgroup size (512 or 1024); FF_BLOCK_THREADS overrides for experiments
    bool setup_threshold_forced = false;
    int setup_threshold = 14, leaf_threshold = 20; // BVH kernel scheduling knobs: traversal time slice in inner rounds (0 = none) and
                                                   // early-leaf quorum (FF_SETUP_THRESHOLD / FF_LEAF_THRESHOLD)
    FfStats stats;
    const char* last_kernel_name = nullptr; // trace kernel instantiation of the last frame (rocprofv3's spelling)
    unsigned long long raw_counters[32] = {};
    // GL interop
    hipGraphicsResource* pbo_resource = nullptr;
    int pbo_width = 0, pbo_height = 0;
    // multi-GPU (ff_dist_init): communicator, rank and the packed strip / gather buffers
    FfDistContext* dist = nullptr;
    // a frame enqueued by render_enqueue and not yet finished by render_finish
    int pending_launches = 0;
    uint32_t pending_flags = 0;
    unsigned pending_culled_rays_per_pixel = 0; // primary-ray cull: rays each culled pixel stands for in FfStats::rays_answered
    bool pending = false;
    // fault injection for tests (FF_DEBUG_FAIL_ALLOC=k: the k-th scene allocation of every upload reports out-of-memory)
    int debug_fail_alloc = -1, alloc_countdown = -1;
    // FF_DEBUG_TIMELINE_US=bucket: instrumented launches histogram ray completions over the launch's wall clock (ff_debug_timeline)
    int timeline_bucket_us = 0;
    unsigned* d_timeline = nullptr;
    unsigned h_timeline[1024] = {};
    std::vector<unsigned> h_timeline_rows; // one row per wave, added up by ff_debug_timeline
};

#define FF_HIP(call)                                                                                          \
    do {                                                                                                      \
        hipError_t _e = (call);                                                                               \
        if (_e != hipSuccess) return fail(_e == hipErrorOutOfMemory ? FF_ERR_OOM : FF_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

namespace ff {

int ensure_bytes(void** ptr, size_t* cap, size_t need);

// What every render entry point checks before it touches the device.
int check_render_call(const FfState* s, const FfCamera* camera, const FfRenderParams* params, const char* who);

// One frame (or this part's strips / one tile of it), in two steps so that several devices can work at once:
// render_enqueue puts clears, trace launches, the combine pass and the counter read-back on the state's stream and
// returns; render_finish waits for them and fills the state's FfStats.  rgb8_dev / radiance_dev are device pointers to
// the LOCAL image (local_rows x win_w).  The window is [x0, x0 + win_w) x (y0 + the strip layout's rows); whole-width
// strips pass x0 = y0 = 0, win_w = -1.
int render_enqueue(FfState* s, const FfCamera* camera, const FfRenderParams* prm, int strip_rows, int part, int num_parts, int local_rows,
                   unsigned char* rgb8_dev, float* radiance_dev, int x0 = 0, int y0 = 0, int win_w = -1);
int render_finish(FfState* s);

// The two optional outputs of a render entry point of `pixels` pixels, as the frame gets them: the caller's device pointers, or the
// state's d_rgb8 / d_radiance grown to size, which copy_back() copies to the caller's host buffers after the frame.  Null stays
// null.  status: FF_OK, or what ensure_bytes returned for a failed allocation (its message is the thread's last error).  The
// render-side twin of StagedOutputs (ff_image.h).
struct RenderOutputs {
    unsigned char* rgb8 = nullptr;
    float* radiance = nullptr;
    int status = FF_OK;
    RenderOutputs() = default; // no outputs (a rank that gathers nothing)
    RenderOutputs(FfState* s, size_t pixels, void* rgb8_out, int rgb8_on_device, float* radiance_out, int radiance_on_device)
        : rgb8((unsigned char*)rgb8_out), radiance(radiance_out)
    {
        if (rgb8_out && !rgb8_on_device) {
            status = ensure_bytes((void**)&s->d_rgb8, &s->rgb8_bytes, pixels * 3 + 16);
            if (status != FF_OK) return;
            rgb8 = s->d_rgb8;
            host_rgb8 = rgb8_out;
            rgb8_bytes = pixels * 3;
        }
        if (radiance_out && !radiance_on_device) {
            status = ensure_bytes((void**)&s->d_radiance, &s->radiance_bytes, pixels * 12 + 16);
            if (status != FF_OK) return;
            radiance = s->d_radiance;
            host_radiance = radiance_out;
            radiance_bytes = pixels * 12;
        }
    }
    // After the frame has finished: the outputs placed in the state's buffers, to the host (an output of no bytes - a part without
    // rows - is skipped).
    int copy_back() const
    {
        if (rgb8_bytes) FF_HIP(hipMemcpy(host_rgb8, rgb8, rgb8_bytes, hipMemcpyDeviceToHost));
        if (radiance_bytes) FF_HIP(hipMemcpy(host_radiance, radiance, radiance_bytes, hipMemcpyDeviceToHost));
        return FF_OK;
    }

private:
    void* host_rgb8 = nullptr;
    float* host_radiance = nullptr;
    size_t rgb8_bytes = 0, radiance_bytes = 0; // what copy_back() copies (0: a device output, or none)
};

// What render_enqueue's frame shares with enqueue_nee's and with frame_primary_hits (ff_frame.cpp), one copy each:
// the camera's ray matrix into `k`;
void set_camera_matrix(KParams& k, const FfMat4& cm);
// d_stack_spill grown for a launch of grid x block_threads threads and attached to `k`, where the scene's stacks spill at all;
int attach_stack_spill(FfState* s, KParams& k, int grid, int block_threads);
// the clears of the local image that FF_GRID_REFERENCE_FLOOR needs (either pointer may be null);
int clear_floor_grid(int grid_mode, unsigned char* rgb8_dev, float* radiance_dev, size_t local_pixels, hipStream_t stream);
// the sample blocks of launch number `launch`: block_begin, block_end, whole_blocks, total_items;
void set_launch_blocks(KParams& k, int launch, int blocks_per_launch);
// what render_finish reads of an enqueued frame (the state's pending_* fields; sets `pending`).
void commit_pending(FfState* s, int launches, uint32_t flags, unsigned culled_rays_per_pixel, bool mask_reused, bool mask_built);

// Geometry records the BVH kernels keep in LDS: all of them up to kMaxLdsRecords, none beyond (read from global memory).
inline int lds_records(const FfState* s) { return s->num_geoms > kMaxLdsRecords ? 0 : s->num_geoms; }

// This camera's primary hits for a whole width x height frame (ff_render's pixel mapping: one part, strips of height rows, the
// window is the image), for ff_gbuffer (ff_image_api.cpp): the hits the state keeps from its last frame if they were computed for
// this camera and mapping, else a pre-pass into d_gb_hits on the state's stream (fresh; the work-queue counters are zeroed behind
// it and the loop-guard counter is the caller's to read).  Nothing of the frame's state - stored hits, key, cull mask - is written.
struct PrimaryHits {
    const float4* hits;
    bool fresh;
    unsigned pix_items;
    int tiles_per_row, xlim, ylim;
};
int frame_primary_hits(FfState* s, const FfCamera* camera, const FfRenderParams* params, PrimaryHits* out);

void dist_release(FfState* s); // ff_dist.cpp: frees s->dist (called by ff_destroy)

// Next-event estimation (ff_nee.cpp): keep the geometries the light table is built from (upload: drop the old ones first), take a
// mesh's replaced triangles, rebuild the device table, and enqueue a frame of FF_SHADE_DIFFUSE_PATH_NEE (called by render_enqueue).
void nee_capture(FfState* s, const FfGeometry* g, int n, bool upload);
void nee_replace_mesh(FfState* s, int geometry_index, const FfTriangle* tris, int count);
int nee_rebuild(FfState* s);
int enqueue_nee(FfState* s, KParams& k, const FfCamera* camera, const FfRenderParams* prm, int launches, int blocks_per_launch, size_t local_pixels);
// Per-sample camera rays (ff_camera.cpp): what ff_set_camera_sampling and its host twin refuse (who: the prefix of the error's text).
int check_camera_sampling(const FfCameraSampling* cs, const char* who);
// Environment light (ff_env.cpp): frees the state's device table (ff_destroy).
void env_release(FfState* s);
// Albedo textures (ff_texture.cpp): drop the scene's bindings (ff_upload_scene), rewrite the device tables, free everything (ff_destroy).
void tex_drop_bindings(FfState* s);
int tex_sync_tables(FfState* s);
void tex_release(FfState* s);
// Rough-specular mirrors (ff_glossy.cpp): drop the scene's bindings (ff_upload_scene), rewrite the device table from the bindings and
// the records' materials (ff_set_roughness, ff_update_transforms), free it (ff_destroy).
void glossy_drop_bindings(FfState* s);
int glossy_sync_table(FfState* s);
void glossy_release(FfState* s);
// Display transform (ff_display_api.cpp): frees the counters and the threshold table (ff_destroy).
void display_release(FfState* s);
// Adaptive sampling (ff_adaptive_api.cpp): frees the state's buffers (ff_destroy).
void adaptive_release(FfState* s);
// Video planes (ff_yuv_api.cpp): frees the knot tables (ff_destroy).
void yuv_release(FfState* s);
// Resampling (ff_resize_api.cpp): frees the intermediate image and the two tables (ff_destroy).
void resize_release(FfState* s);
// Colour grade (ff_grade_api.cpp): frees the LUT objects (ff_destroy).
void grade_release(FfState* s);
// Lens (ff_lens_api.cpp): frees the device table (ff_destroy).
void lens_release(FfState* s);
// The pixel buffer registered with ff_register_gl_pbo, mapped on the state's stream (kernel.cu:338-339) and unmapped again
// (kernel.cu:344): what ff_render_to_pbo and ff_display_to_pbo write (ff_render_api.cpp).  need_bytes: the least size the mapping
// must have.
int map_pbo(FfState* s, size_t need_bytes, void** out_ptr);
int unmap_pbo(FfState* s, int status);

// ff_upload_scene for a scene already compiled on the host (ff_scene_api.cpp).
int upload_compiled_scene(FfState* s, const CompiledScene& cs, double build_ms);
// The scene on the device (ff_scene_api.cpp): frees its arrays and forgets it (an upload's first step; ff_destroy).
void free_scene(FfState* s);

} // namespace ff
