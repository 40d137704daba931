// ff_frame.cpp — one frame on one device: the camera and pixel mapping, the frame's plan (every decision about how it is fed to the
// kernels, made before anything is touched), and the steps that carry the plan out - grow the state's buffers, fill the launch
// parameters, put the work on the stream, commit the cross-frame state.  Host side of kernel.cu:335-344 (per-frame
// map -> clear -> kernel -> unmap).  ff_nee.cpp's frame (enqueue_nee) and ff_gbuffer's pre-pass (frame_primary_hits) share the helpers.
#include <algorithm>
#include <cmath>
#include <cstring>

#include <hip/hip_runtime.h>

#include "ff_state.h"

using namespace ff;

namespace {

// Every decision render_enqueue makes about a frame.  The plan_* functions fill it from the state, the camera and the parameters; they
// call nothing of HIP, allocate nothing and write nothing to the state.
struct FramePlan {
    size_t local_pixels;
    bool bvh;                                                        // prm->trace_mode == FF_TRACE_BVH
    bool debug, env, tex, glossy, cam;                               // plan_modes
    bool nee;                                                        // ... the frame runs enqueue_nee's kernels
    int spp, bounces, block_spp, num_blocks, blocks_per_launch, launches; // plan_sample_blocks
    int block_threads, grid;                                         // plan_workgroup
    int cut_last;                                                    // plan_last_bounce_cut
    unsigned emitter_mask;
    float scene_min[3], scene_max[3];                                // plan_scene_box
    bool box_cull;                                                   // the camera is outside the box (what the work queue is sized by)
    bool timeline;                                                   // plan_pool (an instrumented frame with a timeline)
    bool pool;
    int pool_quorum, pool_quorum_min, pool_refill, pool_slice, pool_leave, pool_batch_min;
    bool key_valid, vertex_normals, hits_kept, start_kept;           // plan_primary_reuse
    FfState::PrimaryKey key;
    bool reuse, use_start;
    unsigned queue_chunk, queue_tail_items;                          // plan_work_queue
    int queue_counters;
    struct {                                                         // plan_tail
        bool mode, wanted;
        int blocks, n, step;
        size_t bytes;
    } tail;
    bool cull, exact_cull, kept;                                     // plan_cull
    unsigned culled_rays_per_pixel;
};

size_t primary_hits_bytes(unsigned pix_items) { return (size_t)3 * (size_t)pix_items * sizeof(float4); }
size_t cull_mask_bytes(unsigned pix_items) { return ((size_t)pix_items / 64 + 2) * sizeof(unsigned long long); }
size_t timeline_rows(const FfState* s) { return (size_t)s->num_cus * 2 * (kBlockThreads / 64); } // one row per wave of the largest grid
bool stack_spills(const FfState* s) { return s->stack_lds_levels < s->stack_entries; }

// The camera and the pixel mapping of a frame part into `k`: strips of strip_rows rows dealt to num_parts parts, of which this is
// `part` with local_rows rows, and the window [x0, x0 + win_w) x (y0 + ...) of the W x H image.
void fill_frame_mapping(const FfState* s, KParams& k, const FfCamera* camera, int W, int H, int grid_mode, int strip_rows, int part, int num_parts,
                        int local_rows, int x0, int y0, int win_w)
{
    FfMat4 cm;
    ff_camera_ray_matrix_jittered(camera, s->jitter_x, s->jitter_y, &cm); // (the state's pixel jitter; 0 0: ff_camera_ray_matrix)
    set_camera_matrix(k, cm);
    k.cam_pos[0] = camera->m_position.x;
    k.cam_pos[1] = camera->m_position.y;
    k.cam_pos[2] = camera->m_position.z;
    k.far_clip = camera->m_farClip;
    k.screen_w = camera->m_screenWidth;
    k.screen_h = camera->m_screenHeight;
    k.width = W;
    k.height = H;
    k.xlim = W;
    k.ylim = H;
    if (grid_mode == FF_GRID_REFERENCE_FLOOR) { // kernel.cu:306-309
        k.xlim = (W / 16) * 16;
        k.ylim = (H / 16) * 16;
    }
    k.strip_rows = strip_rows;
    k.part = part;
    k.num_parts = num_parts;
    k.local_rows = local_rows;
    k.x0 = x0;
    k.y0 = y0;
    k.local_width = win_w;
    k.tiles_per_row = (win_w + 7) / 8;
    k.pix_items = (unsigned)((uint64_t)k.tiles_per_row * (uint64_t)((local_rows + 7) / 8) * 64);
}

// num_blocks: the sample blocks a pixel item is queued for (the work queue counts items in 31 bits); who: the prefix of that error's text.
int check_queue_range(const KParams& k, int num_blocks, const char* who)
{
    const uint64_t tiles = (uint64_t)k.tiles_per_row * (uint64_t)((k.local_rows + 7) / 8);
    if (tiles * 64 * (uint64_t)(num_blocks + 64) >= (1ull << 31)) return fail(FF_ERR_INVALID_ARG, "%simage too large for the work queue", who);
    return FF_OK;
}

// The uploaded scene and its LDS layout (finalize_layout) into `k`.  smooth: the frame shades with vertex normals; lds_block_threads:
// the BVH kernel's workgroup size, for FF_DEBUG_LDS_FILL (0: a brute-force frame, which has no such layout).
void fill_scene(const FfState* s, KParams& k, bool smooth, int lds_block_threads)
{
    k.setup_threshold = s->setup_threshold;
    k.leaf_threshold = s->leaf_threshold;
    k.num_geoms = s->num_geoms;
    k.num_planes = s->num_planes;
    k.num_quads = s->num_quads;
    k.has_specular = s->has_specular ? 1 : 0;
    k.geoms = s->d_geoms;
    k.tris = s->d_tris;
    k.trinormals = smooth ? reinterpret_cast<const float4*>(s->d_normals) : nullptr;
    k.nodes4 = s->d_nodes4;
    k.tri_world_normals = s->d_world_normals;
    k.geom_world_normals = s->d_world_normals ? s->d_world_normals + s->num_tris : nullptr;
    if (s->sw.lds_fill && lds_block_threads > 0) {
        const size_t bytes = bvh_lds_bytes(s->lds_cap, s->stack_lds_levels, lds_block_threads, lds_records(s)); // (the pool behind it is initialised by the kernel)
        k.debug_lds_words = (unsigned)std::min<size_t>(s->sw.lds_fill_words, bytes / 4);
        k.debug_lds_pattern = (unsigned)s->sw.lds_fill_pattern;
    }
    k.stack_depth = s->stack_lds_levels;
    k.stack_spill = nullptr;
    k.lds_nodes = s->lds_cap;
    k.top_first = (int)s->node_capacity;
    k.top_lds_first = 0;
    k.top_lds_count = s->top_lds_count;
    k.num_scan = s->num_scan;
    k.walls = s->walls;
}

// The stack levels that did not get LDS (finalize_layout): one int per level and thread of the launch.
int grow_stack_spill(FfState* s, int grid, int block_threads)
{
    if (!stack_spills(s)) return FF_OK;
    return ensure_bytes((void**)&s->d_stack_spill, &s->stack_spill_bytes,
                        (size_t)(s->stack_entries - s->stack_lds_levels) * (size_t)grid * (size_t)block_threads * sizeof(int));
}

// The work queue's counters for a launch of `grid` workgroups, and its as-asked tail zone: tail_per_wave items (FF_QUEUE_TAIL
// overrides) for every wave that draws from a counter.
void size_work_queue(const FfState* s, int grid, int block_threads, int tail_per_wave, int* counters, unsigned* tail_items)
{
    *counters = std::min(kQueueCountersDefault, grid);
    if (s->sw.queue_counters > 0) *counters = std::min(std::min(kQueueCounters, grid), s->sw.queue_counters);
    const int waves_per_counter = (grid * (block_threads / 64) + *counters - 1) / *counters;
    *tail_items = (unsigned)(waves_per_counter * (s->sw.queue_tail >= 0 ? s->sw.queue_tail : tail_per_wave));
}

// What stored primary hits were computed for: the camera and the pixel mapping in `k` (fill_frame_mapping), and whether the stored
// normal is the interpolated one (the frame shades with vertex normals).  Compared bytewise.
FfState::PrimaryKey primary_key(const KParams& k, bool smooth)
{
    FfState::PrimaryKey key;
    std::memset(&key, 0, sizeof key);
    std::memcpy(key.cam, k.cam_c0, 16 * sizeof(float));
    std::memcpy(key.cam + 16, k.cam_pos, 3 * sizeof(float));
    key.cam[19] = k.far_clip; key.cam[20] = k.screen_w; key.cam[21] = k.screen_h;
    const int dims[12] = { k.width, k.height, k.xlim, k.ylim, k.strip_rows, k.part, k.num_parts, k.local_rows, k.x0, k.y0, k.local_width, smooth ? 1 : 0 };
    std::memcpy(key.dims, dims, sizeof dims);
    key.pix_items = k.pix_items;
    return key;
}

// The pre-pass of a frame whose launch parameters are `k`: the same persistent kernel, one item per pixel, one primary ray each, the
// hit stored per pixel in `hits` (settle_hit) and the pixels that hit nothing marked in mask_out (may be null).  Its rays are not path
// segments of the frame: the kernel does not count them, and the work queue starts from zero again behind it.  (Always the lane-owned
// kernel, never instrumented: the frame's own launches are what the statistics describe.)
int enqueue_prepass(FfState* s, const KParams& k, float4* hits, unsigned long long* mask_out, int frame_blocks, int grid, int block_threads)
{
    KParams kp = k;
    kp.shade_mode = kShadePrimaryPass;
    kp.primary_hits = hits;
    kp.bounces = 1;
    kp.spp_total = 1;
    kp.block_spp = 1;
    kp.num_blocks = 1;
    kp.block_begin = 0;
    kp.block_end = 1;
    kp.whole_blocks = 1u;
    kp.total_items = kp.pix_items;
    kp.tail_block = -1;
    kp.cull_mask = nullptr; // (every pixel gets its stored hit: a culled pixel's tail items - its last block, traced sample by sample - read it too)
    kp.cull_mask_out = mask_out;
    kp.frame_blocks = frame_blocks;
    kp.cut_last = 0;
    kp.timeline = nullptr;
    kp.queue_chunk = 32u;
    if (s->sw.queue_chunk > 0) kp.queue_chunk = (unsigned)s->sw.queue_chunk;
    FF_HIP(launch_trace(kp, FF_TRACE_BVH, false, grid, block_threads, s->stream, nullptr, false, /*prepass=*/true));
    FF_HIP(hipMemsetAsync(s->d_queue, 0, (size_t)k.queue_counters * kQueueStride * sizeof(unsigned), s->stream));
    return FF_OK;
}

// ---- the plan -----------------------------------------------------------------------------------------------------------------------

// What the frame shades with, and the combinations FF_SHADE_DIFFUSE_PATH_SMOOTH refuses.
int plan_modes(const FfState* s, const FfRenderParams* prm, FramePlan& f)
{
    f.bvh = prm->trace_mode == FF_TRACE_BVH;
    f.debug = prm->shade_mode == FF_SHADE_NORMAL_DEBUG;
    f.env = s->env_set && !f.debug; // (FF_SHADE_NORMAL_DEBUG ignores the environment)
    f.tex = s->tex_bound > 0 && !f.debug; // (... and albedo textures)
    f.glossy = s->glossy_applied > 0 && !f.debug; // (... and rough-specular bindings)
    f.cam = s->cam_active() && !f.debug; // (... and per-sample camera rays)
    const struct { bool on; const char* what; const char* remedy; } refused[4] = {
        { f.env, "under an environment light (ff_set_environment)", "clear it" },
        { f.tex, "albedo textures (ff_set_albedo_texture)", "unbind them" },
        { f.glossy, "rough-specular mirrors (ff_set_roughness)", "unbind them" },
        { f.cam, "per-sample camera rays (ff_set_camera_sampling)", "clear the setting" },
    };
    for (const auto& r : refused)
        if (r.on && prm->shade_mode == FF_SHADE_DIFFUSE_PATH_SMOOTH)
            return fail(FF_ERR_UNSUPPORTED, "FF_SHADE_DIFFUSE_PATH_SMOOTH does not render %s; %s or use FF_SHADE_DIFFUSE_PATH / FF_SHADE_DIFFUSE_PATH_NEE",
                        r.what, r.remedy);
    // (its own kernels: the mega-kernels' part of the plan is not made; under an environment, with albedo textures
    // or rough-specular mirrors bound or with per-sample camera rays, FF_SHADE_DIFFUSE_PATH runs there too, with no light table)
    f.nee = prm->shade_mode == FF_SHADE_DIFFUSE_PATH_NEE || f.env || f.tex || f.glossy || f.cam;
    return FF_OK;
}

void plan_sample_blocks(const FfRenderParams* prm, FramePlan& f)
{
    f.spp = f.debug ? 1 : prm->spp;
    f.bounces = f.debug ? 1 : prm->bounces;
    // Samples are accumulated in blocks (a multiple of 64, at most 16 blocks per pixel up to 1024 spp and beyond): a
    // block sums its samples sequentially, the combine kernel adds a pixel's blocks in order.  (pixel, block) is the unit
    // of work, which keeps the persistent lanes balanced at the end of a frame and when a frame is split over GPUs.
    f.block_spp = 64 * ((f.spp + 1023) / 1024);
    f.num_blocks = (f.spp + f.block_spp - 1) / f.block_spp;
    f.blocks_per_launch = f.num_blocks;
    if (prm->spp_per_launch > 0 && !f.debug) f.blocks_per_launch = std::max(1, (prm->spp_per_launch + f.block_spp - 1) / f.block_spp);
    f.launches = (f.num_blocks + f.blocks_per_launch - 1) / f.blocks_per_launch;
}

// The mega-kernels' workgroup size and grid (enqueue_nee has its own grid rule).
int plan_workgroup(const FfState* s, const KParams& k, FramePlan& f)
{
    f.block_threads = kBlockThreads;
    if (f.bvh) {
        f.block_threads = s->scene_block_threads;
        if (f.block_threads == 0)
            return fail(FF_ERR_UNSUPPORTED, "4-wide BVH of depth %d does not fit the LDS traversal stack (512 threads x %d levels + %d geometry records > 160 KiB); "
                        "upload with FF_BUILD_HOST_SAH or render with FF_TRACE_BRUTE_FORCE", s->max_depth4, s->max_depth4 + 1, s->num_geoms);
    }
    const int blocks_per_cu = f.bvh ? 1 : 2;
    f.grid = s->num_cus * blocks_per_cu;
    const uint64_t max_useful = ((uint64_t)k.pix_items * (uint64_t)f.num_blocks + (uint64_t)f.block_threads - 1) / (uint64_t)f.block_threads;
    if ((uint64_t)f.grid > max_useful) f.grid = (int)max_useful;
    if (f.grid < 1) f.grid = 1;
    return FF_OK;
}

void plan_last_bounce_cut(const FfState* s, FramePlan& f)
{
    f.emitter_mask = 0u;
    f.cut_last = 0;
    if (f.bvh && !f.debug && !s->sw.no_last_bounce_cut) {
        // The last segment of a path adds radiance only when it ends on an emitter.  If every emitter is one of the analytic records
        // all queries screen before anything else (all planes and spheres of a small scene, the scan planes of a big one), a
        // last-bounce query that holds no emitter after that screening is over (scan_records).
        const int screened = s->num_geoms > kChunkGeometries ? s->num_scan : s->num_planes;
        bool all_screened = true;
        for (int i = 0; i < s->num_geoms; ++i) {
            if (s->h_geoms[i].bxdf_type != FF_BXDF_EMITTER) continue;
            if (i < screened && i < 32) f.emitter_mask |= 1u << i;
            else all_screened = false;
        }
        f.cut_last = all_screened ? 1 : 0;
    }
}

void plan_scene_box(const FfState* s, const FfCamera* camera, FramePlan& f)
{
    // the padded world box around everything (the records' own boxes are padded); a camera outside it lets the work queue
    // drop the pixels whose primary ray misses it (acquire_pixel)
    float mn[3] = { 3.0e38f, 3.0e38f, 3.0e38f }, mx[3] = { -3.0e38f, -3.0e38f, -3.0e38f };
    for (const GeomRecord& r : s->h_geoms) {
        if (!(r.wmin[0] <= r.wmax[0])) continue;
        for (int a = 0; a < 3; ++a) { mn[a] = std::min(mn[a], r.wmin[a]); mx[a] = std::max(mx[a], r.wmax[a]); }
    }
    const float cp[3] = { camera->m_position.x, camera->m_position.y, camera->m_position.z };
    bool outside = false, valid = true;
    for (int a = 0; a < 3; ++a) {
        f.scene_min[a] = mn[a];
        f.scene_max[a] = mx[a];
        valid = valid && mn[a] <= mx[a] && std::fabs(mn[a]) < 1e30f && std::fabs(mx[a]) < 1e30f;
        outside = outside || !(cp[a] >= mn[a] && cp[a] <= mx[a]);
    }
    f.box_cull = f.bvh && valid && outside && !s->sw.no_primary_cull;
}

void plan_pool(const FfState* s, FramePlan& f)
{
    f.timeline = s->collect_stats && s->timeline_bucket_us > 0;
    // job-pool kernel: the defaults are where the same-box sweeps put them (profiles/r04_*pool_sweep*)
    f.pool_quorum = s->sw.pool_quorum > 0 ? s->sw.pool_quorum : 40;
    f.pool_quorum_min = std::min(f.pool_quorum, s->sw.pool_quorum_min > 0 ? s->sw.pool_quorum_min : 16);
    f.pool_refill = s->sw.pool_refill > 0 ? s->sw.pool_refill : 16;
    f.pool_slice = s->sw.pool_slice > 0 ? s->sw.pool_slice : 4;
    f.pool_leave = s->sw.pool_leave >= 0 ? s->sw.pool_leave : 24;
    f.pool_batch_min = s->sw.pool_batch_min > 0 ? s->sw.pool_batch_min : 48;
    // (instrumented launches with a timeline run the lane-owned kernel, which keeps it; the LDS layout serves both)
    f.pool = s->use_pool && f.bvh && !f.timeline;
}

// k: the frame's camera and pixel mapping (fill_frame_mapping), which the key is made of.
void plan_primary_reuse(const FfState* s, const FfRenderParams* prm, const KParams& k, FramePlan& f)
{
    // Every sample of a pixel starts with the same ray (kernel.cu:200-205 has no jitter): a pre-pass traces it once per pixel and the
    // frame's samples start from the stored hit (trace_bvh_kernel).  One slot of 3 x 16 bytes per pixel item.
    // The stored hits are KEPT: the next frame from the same camera, pixel mapping and scene starts from them without a pre-pass
    // (a viewer that accumulates 1-spp frames with the camera at rest, kernel.cu:266,342).  A frame of 2 spp or more always runs on
    // stored hits (the pre-pass pays within the frame: +1.3 % at 2 spp).  A 1-spp frame does when the hits are there already (+8 %),
    // or when the frame before it had the same key - the camera has come to rest, so this frame's pre-pass (-4 % for this frame) is
    // the last one; a one-off 1-spp frame traces its primary rays itself (profiles/r04_j_*).
    const bool reuse_possible = f.bvh && !f.debug && !s->sw.no_primary_reuse;
    // (the stored normal is the interpolated one when the frame shades with vertex normals: part of the key)
    f.vertex_normals = prm->shade_mode == FF_SHADE_DIFFUSE_PATH_SMOOTH && s->d_normals != nullptr;
    std::memset(&f.key, 0, sizeof f.key);
    if (reuse_possible) f.key = primary_key(k, f.vertex_normals);
    f.key_valid = reuse_possible;
    const bool keeping = reuse_possible && !s->sw.no_primary_cache;
    f.hits_kept = keeping && s->primary_valid && std::memcmp(&f.key, &s->primary_key, sizeof f.key) == 0;
    const bool at_rest = keeping && s->last_key_valid && std::memcmp(&f.key, &s->last_key, sizeof f.key) == 0;
    f.reuse = reuse_possible && (f.spp >= s->sw.reuse_min_spp || f.hits_kept || at_rest);
    // Start records: diffuse scenes of up to 32 geometries (the instantiation without the extras) on the lane-owned kernel start every
    // sample from the pre-pass's SHADED hit (trace_bvh_kernel<..., START>).  The class of a pixel depends on the bounce count and the
    // shade mode, so the kept records serve only a frame that agrees in both; the raw hits are written and kept as before (the job-pool
    // kernel, ff_gbuffer and FF_NO_START_RECORDS read them).
    f.use_start = f.reuse && !f.pool && !s->sw.no_start_records && s->num_geoms <= kChunkGeometries && s->num_planes == s->num_quads &&
                  !s->has_specular && !f.vertex_normals;
    f.start_kept = true;
    if (f.use_start) // (records in a buffer that is about to move are not there: grow_frame_buffers)
        f.start_kept = s->primary_has_start && s->start_records_bytes >= (size_t)2 * (size_t)k.pix_items * sizeof(float4) &&
                       s->start_bounces == f.bounces && s->start_shade == prm->shade_mode;
}

void plan_work_queue(const FfState* s, int num_parts, FramePlan& f)
{
    // Work queue (csrc/ff_k_shade.h acquire_pixel): 16 counters in different memory channels, and a wave takes at least
    // queue_chunk consecutive items per atomic.  One counter asked for every item serves about 10^8 requests a second, which
    // held every frame of short items far below the saturated rate (1080p C2, before -> after: the reference's own 1-ray frame
    // 0.40 -> 0.19 ms, path-traced 1 spp 2.98 -> 1.33 ms, 4 spp 7.3 -> 4.8, 16 spp 20.8 -> 18.0; the 1 024-spp frame from the
    // reference's default camera, whose 64-sample items are mostly one-ray paths, 164 -> 84 ms).  With 16 counters the chunk
    // hardly matters for the atomics between 8 and 64 items (profiles/r02_q_queue_sweep.txt); what it decides is WHICH items a
    // wave's lanes hold.  Whole 64-sample blocks: 64 items, i.e. the blocks of four neighbouring pixels (one 8x8 tile when a
    // pixel has one block): the lanes' rays start from the same few surface points and walk the same corner of the trees
    // (1 024 spp, ms with chunks of 4 / 16 / 64 / 128: C4, whose tree lives in L2, 570 / 530 / 491 / 488; C2 977 / 968 / 956 /
    // 959; at 64-512 spp C4 gains 10-14 %, C2 1-2 %: profiles/r02_y_chunk_sweep_whole_blocks.txt).  Shorter items (frames of a few samples): 64
    // samples of work, at most 32 items; there what a wave holds back at the end of the launch counts (1 spp: 1.33 ms with
    // 16-32, 1.36 with 64).
    const int samples_per_item = std::max(1, std::min(f.block_spp, f.spp));
    // (the strips of a multi-GPU rank: 32; slowest of eight ranks 125.5 ms against 126.9 with 64 and 125.9 with 16)
    f.queue_chunk = samples_per_item >= 64 ? (num_parts > 1 ? 32u : 64u) : (unsigned)std::min(32, std::max(4, 64 / samples_per_item));
    if (s->sw.queue_chunk > 0) f.queue_chunk = (unsigned)s->sw.queue_chunk;
    // The last items of every counter's share go out exactly as asked for (acquire_pixel: no private stock at the end of a launch):
    // one per lane of the waves that draw from the counter where items are long (sample blocks), an eighth of that where they are
    // short (a 1-spp frame's paths: single-item requests cost an atomic each, which is what the chunks are there to avoid).
    // (measured on one box, profiles/r04_b_queue_tail.txt: long items 64 per wave; frames that drop most of their items at the
    // queue - a camera outside the scene - lose with a long zone, every dropped item there being a request of its own: 8)
    size_work_queue(s, f.grid, f.block_threads, samples_per_item >= 16 && !f.box_cull ? 64 : 8, &f.queue_counters, &f.queue_tail_items);
}

void plan_tail(const FfState* s, const KParams& k, int num_parts, FramePlan& f)
{
    // Fine-grained tail: in the launch that finishes the frame, the last sample block is traced as items of a few samples
    // with per-sample storage (see KParams::tail_samples), so that the launch runs dry on short items.
    const int last_launch_blocks = f.num_blocks - (f.launches - 1) * f.blocks_per_launch;
    // It pays where a launch is short against its items: the ranks of a multi-GPU frame (+3.3 % at eight ranks) and one-GPU
    // frames of up to eight blocks (1080p C2 with / without, ms: 64 spp 66.0 / 71.4, 128 spp 128.4 / 132.3, 256 spp 247.8 / 251.1).
    // It costs a per-sample buffer (2.1 GB written and read back at 1080p), which the 1 024-spp one-GPU frame does not earn back
    // (+0.4 %, and 4x its HBM traffic): off there.  FF_TAIL_GROUP forces it (with that group size) wherever a launch has
    // FF_TAIL_MIN_BLOCKS blocks.  Frames whose buffer would pass 16 GiB render without it (FfStats::flags).
    const bool short_frame = num_parts == 1 && !s->tail_forced && f.num_blocks <= 8;
    // How many of the frame's last blocks go out that way.  A lane that takes one of the last WHOLE blocks finishes up to two block
    // times later (path lengths vary by that much between pixels); the short items must last that long for the launch to end on
    // them, so a rank's strips - where a block time is 6 % of the launch - hand out TWO blocks in groups (eight ranks 94.5 -> 96 % of
    // ideal, profiles/r04_n_*).  The kernels see one "tail block" of up to 2 x block_spp samples starting at block tail_block; the
    // combine pass adds each block's samples in order.
    // (two where a lane gets fewer than 24 whole blocks in the launch - eight ranks at 1080p and 1 024 spp: 16 -, one where it gets
    // more: there the short items' own overhead outweighs the shorter end, 4 ranks 97.7 -> 97.3 %, 2 ranks 98.9 -> 98.5 %)
    const double blocks_per_lane = (double)k.pix_items * (double)last_launch_blocks / ((double)f.grid * (double)f.block_threads);
    const int tail_blocks_wanted = s->sw.tail_blocks > 0 ? s->sw.tail_blocks : (num_parts > 1 && blocks_per_lane < 24.0 ? 2 : 1);
    f.tail.blocks = std::max(1, std::min(std::min(tail_blocks_wanted, 3), last_launch_blocks - 1));
    f.tail.n = f.spp - (f.num_blocks - f.tail.blocks) * f.block_spp; // samples of the frame's last block(s)
    // group size: the given one (multi-part frames: 32 samples), scaled with the block size beyond 1 024 spp and at least an
    // eighth of the block; short one-GPU frames: a quarter of the block, at least 4 samples
    f.tail.step = short_frame ? std::max(4, (f.tail.n + 3) / 4) : std::max(s->tail_group_spp * (f.block_spp / 64), (f.tail.n + 15) / 16);
    f.tail.wanted = !f.debug && f.bvh && s->tail_group_spp > 0 && f.tail.step < f.tail.n &&
                    (short_frame || ((num_parts > 1 || s->tail_forced) && last_launch_blocks >= s->tail_min_blocks));
    f.tail.bytes = (size_t)k.pix_items * (size_t)f.tail.n * sizeof(float4); // [sample of the block][pixel item]
    // The buffer stays allocated between frames.  Where the tail is this library's own choice (short one-GPU frames: a viewer at
    // 64 spp) it may take at most 4 GiB and 2 % of the device's memory (1080p at up to 1 024 spp: 2.1 GB; a 64-spp 4K frame would
    // need 8.5 GB and goes without); where the caller set up a multi-GPU frame or forced it, up to 16 GiB (also keeps slot indices
    // in 31 bits; C5's ranks at eight GPUs need 4.2 GB).  FfStats::flags tells which way a frame went.
    const size_t tail_cap = short_frame ? std::min<size_t>(4ull << 30, s->device_mem_bytes / 50) : (16ull << 30);
    f.tail.mode = f.tail.wanted && f.tail.bytes <= tail_cap;
}

void plan_cull(const FfState* s, FramePlan& f)
{
    // (after the tail decision: the tail block's samples are stored one by one and are not part of the cull - a frame whose only
    // block is the tail block has nothing to drop and skips the mask pass.  Dropping tail items too was measured in round 4: a dropped
    // item costs the queue what its 16 samples cost a lane that starts them from a stored miss; no gain, profiles/r04_f_*)
    // (... and so does the reference's own frame - one primary ray per pixel, shaded by its normal: tracing a ray that misses
    // everything costs what the mask pass costs, and the pass is a second launch: 0.089 instead of 0.064 ms at 1080p)
    f.cull = f.box_cull && f.num_blocks - (f.tail.mode ? f.tail.blocks : 0) > 0 && !f.debug;
    // ... and where a pre-pass stores every pixel's primary hit (below), it marks the pixels that hit NOTHING in the same mask: the
    // exact version of the box test, also for a camera inside the scene's box (an open room seen from within)
    f.exact_cull = f.reuse && !s->sw.no_primary_cull && f.num_blocks - (f.tail.mode ? f.tail.blocks : 0) > 0;
    // Can this frame start from the hits (and the mask) the last one stored?  Same camera, same pixel mapping, no change of the scene
    // since (every upload / update clears primary_valid), and a mask there if this frame wants one.
    f.kept = f.reuse && f.hits_kept && (!(f.cull || f.exact_cull) || s->primary_has_mask) && f.start_kept;
    // (a culled pixel's whole-block items are dropped; with a fine-grained tail its last block is still traced sample by sample)
    f.culled_rays_per_pixel = f.cull || f.exact_cull ? (unsigned)(f.spp - (f.tail.mode ? f.tail.n : 0)) : 0u;
}

// The whole plan, in the order the decisions depend on each other.  k: the frame's camera and pixel mapping.
int plan_frame(const FfState* s, const FfCamera* camera, const FfRenderParams* prm, const KParams& k, FramePlan& f)
{
    int st = plan_modes(s, prm, f);
    if (st != FF_OK) return st;
    plan_sample_blocks(prm, f);
    st = check_queue_range(k, f.num_blocks, "");
    if (st != FF_OK) return st;
    st = plan_workgroup(s, k, f);
    if (st != FF_OK || f.nee) return st;
    plan_last_bounce_cut(s, f);
    plan_scene_box(s, camera, f);
    plan_pool(s, f);
    plan_primary_reuse(s, prm, k, f);
    plan_work_queue(s, k.num_parts, f);
    plan_tail(s, k, k.num_parts, f);
    plan_cull(s, f);
    return FF_OK;
}

// ---- the steps that carry it out ------------------------------------------------------------------------------------------------------

// Every buffer of the state the planned frame needs, at the size it needs.  The stored hits and start records do not survive a buffer
// that moves.
int grow_frame_buffers(FfState* s, const FramePlan& f, unsigned pix_items)
{
    int st = ensure_bytes((void**)&s->d_blocksums, &s->blocksums_bytes, (size_t)pix_items * (size_t)f.num_blocks * 4 * sizeof(float));
    if (st != FF_OK || f.nee) return st; // (enqueue_nee sizes the stack spill for its own grid)
    if (f.timeline && !s->d_timeline) FF_HIP(hipMalloc((void**)&s->d_timeline, timeline_rows(s) * kTimelineBuckets * sizeof(unsigned)));
    if (f.reuse) {
        if (s->primary_cache_bytes < primary_hits_bytes(pix_items)) s->primary_valid = false; // (the buffer is about to move)
        st = ensure_bytes((void**)&s->d_primary_cache, &s->primary_cache_bytes, primary_hits_bytes(pix_items));
        if (st != FF_OK) return st;
    }
    if (f.use_start) {
        const size_t need = (size_t)2 * (size_t)pix_items * sizeof(float4);
        if (s->start_records_bytes < need) s->primary_has_start = false; // (the buffer is about to move)
        st = ensure_bytes((void**)&s->d_start_records, &s->start_records_bytes, need);
        if (st != FF_OK) return st;
    }
    if (f.pool) {
        // where a lane's own path and query state waits between setup passes (trace_pool_kernel): 7 x 16 bytes per thread of the launch
        st = ensure_bytes((void**)&s->d_park, &s->park_bytes, (size_t)7 * (size_t)f.grid * (size_t)f.block_threads * sizeof(float4));
        if (st != FF_OK) return st;
    }
    if (f.bvh) {
        st = grow_stack_spill(s, f.grid, f.block_threads);
        if (st != FF_OK) return st;
    }
    if (!f.tail.mode && s->d_tail_samples && s->tail_samples_bytes > (256ull << 20)) {
        // a frame that does not use it gives a large buffer back (the stream has drained: every render call is synchronous)
        (void)hipFree(s->d_tail_samples);
        s->d_tail_samples = nullptr;
        s->tail_samples_bytes = 0;
    }
    if (f.tail.mode) {
        st = ensure_bytes((void**)&s->d_tail_samples, &s->tail_samples_bytes, f.tail.bytes);
        if (st != FF_OK) return st;
    }
    if ((f.cull || f.exact_cull) && !f.kept) return ensure_bytes((void**)&s->d_cull_mask, &s->cull_mask_bytes, cull_mask_bytes(pix_items));
    return FF_OK;
}

// The launch parameters of the planned frame into `k` (which holds the camera and the pixel mapping), from the grown buffers.  What the
// mask pass and the pre-pass produce - cull_mask, primary_hits, start_records - is attached where they are enqueued (enqueue_primaries).
void fill_frame_params(const FfState* s, const FramePlan& f, const FfCamera* camera, const FfRenderParams* prm, unsigned char* rgb8_dev, float* radiance_dev,
                       KParams& k)
{
    k.bounces = f.bounces;
    k.spp_total = f.spp;
    k.block_spp = f.block_spp;
    k.num_blocks = f.num_blocks;
    k.blocksums = reinterpret_cast<float4*>(s->d_blocksums);
    k.key = (unsigned)prm->seed ^ (unsigned)(prm->seed >> 32);
    k.shade_mode = prm->shade_mode;
    fill_scene(s, k, prm->shade_mode == FF_SHADE_DIFFUSE_PATH_SMOOTH, f.bvh ? f.block_threads : 0);
    k.rgb8 = rgb8_dev;
    k.radiance = radiance_dev;
    if (f.nee) {
        if (f.cam && s->cam_sampling.pixel_filter == FF_PIXEL_BOX) {
            // the sample's own point of the pixel replaces the state's jitter: the unjittered matrix
            FfMat4 cm;
            ff_camera_ray_matrix(camera, &cm);
            set_camera_matrix(k, cm);
        }
        return; // (enqueue_nee fills in the rest)
    }
    k.emitter_mask = f.emitter_mask;
    k.cut_last = f.cut_last;
    for (int a = 0; a < 3; ++a) {
        k.scene_min[a] = f.scene_min[a];
        k.scene_max[a] = f.scene_max[a];
    }
    k.queue = s->d_queue;
    k.counters = s->d_counters;
    k.timeline = f.timeline ? s->d_timeline : nullptr;
    k.timeline_ticks = f.timeline ? (unsigned)s->timeline_bucket_us * 100u : 1u; // the wall clock ticks at 100 MHz
    k.reuse_quorum = s->sw.reuse_quorum;
    k.pool_quorum = f.pool_quorum;
    k.pool_quorum_min = f.pool_quorum_min;
    k.pool_refill = f.pool_refill;
    k.pool_slice = f.pool_slice;
    k.pool_leave = f.pool_leave;
    k.pool_batch_min = f.pool_batch_min;
    k.park = f.pool ? s->d_park : nullptr;
    if (f.bvh && stack_spills(s)) k.stack_spill = s->d_stack_spill;
    k.queue_chunk = f.queue_chunk;
    k.queue_counters = f.queue_counters;
    k.queue_tail_items = f.queue_tail_items;
    k.tail_block = -1;
    if (f.tail.mode) {
        k.tail_samples = s->d_tail_samples;
        k.tail_samples_in_block = f.tail.n;
        // (Grading the groups down to an eighth of a block on multi-GPU ranks was measured: the 8-sample items cost more
        // than the tail they save, 92.3 % instead of 93.3 % of ideal at eight ranks.)
        int g = 0;
        k.tail_start[0] = 0;
        while (k.tail_start[g] < f.tail.n && g < 16) { k.tail_start[g + 1] = std::min(f.tail.n, k.tail_start[g] + f.tail.step); ++g; }
        k.tail_groups = g;
    }
}

// On the stream, in this order: the clears, the mask pass (or the mask's memset) and the pre-pass.
int enqueue_primaries(FfState* s, const FramePlan& f, const FfRenderParams* prm, KParams& k)
{
    hipStream_t st = s->stream;
    if (f.timeline) FF_HIP(hipMemsetAsync(s->d_timeline, 0, timeline_rows(s) * kTimelineBuckets * sizeof(unsigned), st));
    const int cst = clear_floor_grid(prm->grid_mode, k.rgb8, k.radiance, f.local_pixels, st);
    if (cst != FF_OK) return cst;
    FF_HIP(hipMemsetAsync(s->d_counters, 0, (size_t)(1 + k.queue_counters) * kQueueStride * sizeof(unsigned), st)); // counters and the work queue behind them
    FF_HIP(hipEventRecord(s->ev_begin, st));
    if (f.cull || f.exact_cull) {
        if (!f.kept) {
            if (f.cull) FF_HIP(launch_cull_mask(k, s->d_cull_mask, st));
            else FF_HIP(hipMemsetAsync(s->d_cull_mask, 0, cull_mask_bytes(k.pix_items), st));
        }
        k.cull_mask = s->d_cull_mask;
    }
    if (f.reuse && f.kept) k.primary_hits = s->d_primary_cache;
    k.start_records = f.use_start ? s->d_start_records : nullptr;
    k.start_bounces = f.bounces;
    if (f.reuse && !f.kept) {
        const int pst = enqueue_prepass(s, k, s->d_primary_cache, f.exact_cull ? s->d_cull_mask : nullptr, f.num_blocks, f.grid, f.block_threads);
        if (pst != FF_OK) return pst;
        k.primary_hits = s->d_primary_cache;
    }
    return FF_OK;
}

// ... then the launch loop, the combine pass, the events and the read-backs.
int enqueue_samples(FfState* s, const FramePlan& f, const FfRenderParams* prm, KParams& k)
{
    hipStream_t st = s->stream;
    for (int l = 0; l < f.launches; ++l) {
        set_launch_blocks(k, l, f.blocks_per_launch);
        if (f.tail.mode && l == f.launches - 1) {
            const unsigned groups = (unsigned)k.tail_groups;
            k.tail_block = f.num_blocks - f.tail.blocks;
            k.whole_blocks = (unsigned)(k.block_end - f.tail.blocks - k.block_begin);
            k.tail_first_item = k.pix_items * k.whole_blocks;
            k.total_items = k.tail_first_item + k.pix_items * groups;
        }
        if (l > 0) FF_HIP(hipMemsetAsync(s->d_queue, 0, (size_t)k.queue_counters * kQueueStride * sizeof(unsigned), st));
        FF_HIP(launch_trace(k, prm->trace_mode, s->collect_stats, f.grid, f.block_threads, st, &s->last_kernel_name, f.pool, /*prepass=*/false, /*start=*/f.use_start,
                            /*world_normals=*/!s->sw.no_world_normals));
    }
    FF_HIP(launch_combine(k, st));
    FF_HIP(hipEventRecord(s->ev_end, st));
    FF_HIP(hipMemcpyAsync(s->h_counters, s->d_counters, kCounterWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    if (k.timeline) {
        s->h_timeline_rows.resize(timeline_rows(s) * kTimelineBuckets);
        FF_HIP(hipMemcpyAsync(s->h_timeline_rows.data(), s->d_timeline, timeline_rows(s) * kTimelineBuckets * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    }
    return FF_OK;
}

// ---- the commit step: every write to the state that a later frame reads (with commit_pending below) ---------------------------------

// Before anything of the frame can fail: the next frame's "has the camera come to rest?" holds against this one, enqueued or not.
void commit_frame_key(FfState* s, const FramePlan& f)
{
    s->last_key = f.key;
    s->last_key_valid = f.key_valid;
}

// Once the mask pass and the pre-pass are on the stream: what d_cull_mask, d_primary_cache and d_start_records now hold.
void commit_primaries(FfState* s, const FramePlan& f, int shade_mode)
{
    if (f.cull && !f.reuse) s->primary_has_mask = false; // (the mask that went with the stored hits has just been overwritten; the hits stay)
    if (f.reuse && !f.kept) {
        s->primary_key = f.key;
        s->primary_valid = true;
        s->primary_has_mask = f.cull || f.exact_cull;
        s->primary_has_start = f.use_start;
        s->start_bounces = f.bounces;
        s->start_shade = shade_mode;
    }
}

} // namespace

namespace ff {

void set_camera_matrix(KParams& k, const FfMat4& cm)
{
    std::memcpy(k.cam_c0, &cm.m[0], 16);
    std::memcpy(k.cam_c1, &cm.m[4], 16);
    std::memcpy(k.cam_c2, &cm.m[8], 16);
    std::memcpy(k.cam_c3, &cm.m[12], 16);
}

int attach_stack_spill(FfState* s, KParams& k, int grid, int block_threads)
{
    const int st = grow_stack_spill(s, grid, block_threads);
    if (st == FF_OK && stack_spills(s)) k.stack_spill = s->d_stack_spill;
    return st;
}

// cudaMemset(pbo, 0) of kernel.cu:340: untraced pixels read 0.  With the full grid the combine pass writes every pixel
// of the window (a missed pixel gets its zero sum), so the clears are only needed for the reference's floor grid.
int clear_floor_grid(int grid_mode, unsigned char* rgb8_dev, float* radiance_dev, size_t local_pixels, hipStream_t stream)
{
    if (grid_mode != FF_GRID_REFERENCE_FLOOR) return FF_OK;
    if (rgb8_dev) FF_HIP(hipMemsetAsync(rgb8_dev, 0, local_pixels * 3, stream));
    if (radiance_dev) FF_HIP(hipMemsetAsync(radiance_dev, 0, local_pixels * 3 * sizeof(float), stream));
    return FF_OK;
}

void set_launch_blocks(KParams& k, int launch, int blocks_per_launch)
{
    k.block_begin = launch * blocks_per_launch;
    k.block_end = std::min(k.num_blocks, (launch + 1) * blocks_per_launch);
    k.whole_blocks = (unsigned)(k.block_end - k.block_begin);
    k.total_items = k.pix_items * k.whole_blocks;
}

void commit_pending(FfState* s, int launches, uint32_t flags, unsigned culled_rays_per_pixel, bool mask_reused, bool mask_built)
{
    s->pending_culled_rays_per_pixel = culled_rays_per_pixel;
    s->pending_mask_reused = mask_reused;
    s->pending_mask_built = mask_built;
    s->pending_flags = flags;
    s->pending = true;
    s->pending_launches = launches;
}

// Core of every render entry point (declared in ff_state.h): plan, grow buffers, fill parameters, enqueue, commit state.
int render_enqueue(FfState* s, const FfCamera* camera, const FfRenderParams* prm, int strip_rows, int part, int num_parts, int local_rows,
                   unsigned char* rgb8_dev, float* radiance_dev, int x0, int y0, int win_w)
{
    if (win_w < 0) win_w = prm->width;
    s->stats = FfStats();
    s->pending = false;
    FramePlan f = {};
    f.local_pixels =(size_t)local_rows * (size_t)win_w;
    if (f.local_pixels == 0) return FF_OK;

    KParams k;
    std::memset(&k, 0, sizeof k);
    fill_frame_mapping(s, k, camera, prm->width, prm->height, prm->grid_mode, strip_rows, part, num_parts, local_rows, x0, y0, win_w);
    int st = plan_frame(s, camera, prm, k, f);
    if (st != FF_OK) return st;
    if (!f.nee) commit_frame_key(s, f); // (enqueue_nee's frames neither use nor touch the mega-kernels' keys)
    st = grow_frame_buffers(s, f, k.pix_items);
    if (st != FF_OK) return st;
    fill_frame_params(s, f, camera, prm, rgb8_dev, radiance_dev, k);
    if (f.nee) return enqueue_nee(s, k, camera, prm, f.launches, f.blocks_per_launch, f.local_pixels);
    st = enqueue_primaries(s, f, prm, k);
    if (st != FF_OK) return st;
    commit_primaries(s, f, prm->shade_mode);
    st = enqueue_samples(s, f, prm, k);
    if (st != FF_OK) return st;
    const bool masked = f.cull || f.exact_cull;
    commit_pending(s, f.launches, (f.tail.mode ? FF_STATS_TAIL_ITEMS : 0u) | (f.tail.wanted && !f.tail.mode ? FF_STATS_TAIL_SKIPPED_TOO_LARGE : 0u),
                   f.culled_rays_per_pixel, masked && f.kept, masked && !f.kept);
    return FF_OK;
}

// (declared in ff_state.h)
int frame_primary_hits(FfState* s, const FfCamera* camera, const FfRenderParams* params, PrimaryHits* out)
{
    const int W = params->width, H = params->height;
    KParams k;
    std::memset(&k, 0, sizeof k);
    fill_frame_mapping(s, k, camera, W, H, params->grid_mode, H, 0, 1, H, 0, 0, W);
    int st = check_queue_range(k, 1, "ff_gbuffer: ");
    if (st != FF_OK) return st;
    // The frame's stored hits serve if they were computed for this camera and pixel mapping: with either kind of stored normal, which
    // the G-buffer's resolve does not read.
    const size_t hits_bytes = primary_hits_bytes(k.pix_items);
    bool kept = false;
    for (int smooth = 0; smooth < 2 && !kept; ++smooth) {
        const FfState::PrimaryKey key = primary_key(k, smooth != 0);
        kept = s->primary_valid && s->primary_cache_bytes >= hits_bytes && std::memcmp(&key, &s->primary_key, sizeof key) == 0;
    }
    *out = { s->d_primary_cache, !kept, k.pix_items, k.tiles_per_row, k.xlim, k.ylim };
    if (kept) return FF_OK;
    // a pre-pass of its own (geometric normals; the resolve recomputes a triangle's from its record anyway)
    st = ensure_bytes((void**)&s->d_gb_hits, &s->gb_hits_bytes, hits_bytes);
    if (st != FF_OK) return st;
    out->hits = s->d_gb_hits;
    const int block_threads = s->scene_block_threads;
    const int grid = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)s->num_cus, ((uint64_t)k.pix_items + (uint64_t)block_threads - 1) / (uint64_t)block_threads));
    fill_scene(s, k, false, block_threads);
    st = attach_stack_spill(s, k, grid, block_threads);
    if (st != FF_OK) return st;
    k.reuse_quorum = s->sw.reuse_quorum;
    k.queue = s->d_queue;
    k.counters = s->d_counters;
    k.timeline_ticks = 1;
    size_work_queue(s, grid, block_threads, 8, &k.queue_counters, &k.queue_tail_items);
    FF_HIP(hipMemsetAsync(s->d_counters, 0, (size_t)(1 + k.queue_counters) * kQueueStride * sizeof(unsigned), s->stream));
    return enqueue_prepass(s, k, s->d_gb_hits, nullptr, 1, grid, block_threads);
}

int render_finish(FfState* s)
{
    if (!s->pending) return FF_OK; // nothing was enqueued (an empty part)
    s->pending = false;
    FF_HIP(hipStreamSynchronize(s->stream));
    float ms = 0.f;
    FF_HIP(hipEventElapsedTime(&ms, s->ev_begin, s->ev_end));
    unsigned long long c[32];
    std::memcpy(c, s->h_counters, sizeof c);
    std::memcpy(s->raw_counters, c, sizeof c);
    if (c[0] != 0)
        return fail(FF_ERR_HIP, "the traversal loop guard cut %llu queries short (a malformed or absurdly deep tree): the frame is not valid", c[0]);
    s->stats.rays_traced = 0;
    for (int j = 0; j < kRaySlots; ++j) s->stats.rays_traced += s->h_counters[kRaySlotStride * (kRaySlotFirst + j)];
    s->stats.rays_answered = 0;
    {
        // the rays of culled pixels: counted by the passes that built the mask - or, for a frame that took the mask over from the
        // last one, as many pixels as that frame counted
        unsigned long long culled = 0;
        for (int j = 0; j < kRaySlots; ++j) culled += s->h_counters[kCulledPixelsWord + kRaySlotStride * j];
        if (s->pending_mask_reused) culled = s->primary_culled_pixels;
        else if (s->pending_mask_built) s->primary_culled_pixels = culled;
        s->stats.rays_answered += culled * s->pending_culled_rays_per_pixel;
    }
    for (int j = 0; j < kRaySlots; ++j) s->stats.rays_answered += s->h_counters[kAnsweredWord + kRaySlotStride * j]; // + repeated primaries
    s->stats.rays_cut_short = 0;
    for (int j = 0; j < kRaySlots; ++j) s->stats.rays_cut_short += s->h_counters[kCutShortWord + kRaySlotStride * j];
    s->raw_counters[0] = s->stats.rays_traced;
    s->stats.nodes_visited = c[1];
    s->stats.tris_tested = c[2];
    s->stats.planes_tested = c[3];
    s->stats.kernel_ms = ms;
    s->stats.kernel_launches = (uint32_t)s->pending_launches;
    s->stats.flags = s->pending_flags;
    s->stats.scene_bytes_nodes = (uint64_t)s->num_nodes4 * sizeof(Bvh4Node);
    s->stats.scene_bytes_tris = s->num_tris * sizeof(TriRecord);
    return FF_OK;
}

} // namespace ff
