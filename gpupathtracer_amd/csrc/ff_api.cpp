// ff_api.cpp — the tracer handle behind the C ABI (include/firefly/ff_api.h): its lifetime (ff_create / ff_destroy), the experiment
// switches, the stream, the pixel jitter and measurement.  The scene on the device is ff_scene_api.cpp, the render entry points are
// ff_render_api.cpp, the frame itself (kernel.cu:335-344) is ff_frame.cpp.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include <hip/hip_runtime.h>

#include "ff_state.h"

using namespace ff;

namespace ff {

int ensure_bytes(void** ptr, size_t* cap, size_t need)
{
    if (*cap >= need && *ptr) return FF_OK;
    if (*ptr) (void)hipFree(*ptr);
    *ptr = nullptr;
    *cap = 0;
    hipError_t e = hipMalloc(ptr, need);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? FF_ERR_OOM : FF_ERR_HIP, "hipMalloc(%zu) failed: %s", need, hipGetErrorString(e));
    *cap = need;
    return FF_OK;
}

} // namespace ff

namespace {

// The experiment switches of FfState::Switches, from the environment (ff_create; ff_debug_reload_switches).
void read_switches(FfState* s)
{
    FfState::Switches w;
    w.no_last_bounce_cut = std::getenv("FF_NO_LAST_BOUNCE_CUT") != nullptr;
    w.no_primary_cull = std::getenv("FF_NO_PRIMARY_CULL") != nullptr;
    w.no_primary_reuse = std::getenv("FF_NO_PRIMARY_REUSE") != nullptr;
    w.no_primary_cache = std::getenv("FF_NO_PRIMARY_CACHE") != nullptr;
    w.no_start_records = std::getenv("FF_NO_START_RECORDS") != nullptr;
    w.no_world_normals = std::getenv("FF_NO_WORLD_NORMALS") != nullptr;
    if (const char* e = std::getenv("FF_TAIL_BLOCKS")) w.tail_blocks = std::max(1, std::min(3, std::atoi(e)));
    if (const char* e = std::getenv("FF_REUSE_MIN_SPP")) w.reuse_min_spp = std::max(1, std::atoi(e));
    if (const char* e = std::getenv("FF_REUSE_QUORUM")) w.reuse_quorum = std::max(1, std::min(65, std::atoi(e)));
    if (const char* e = std::getenv("FF_QUEUE_CHUNK")) w.queue_chunk = std::max(1, std::min(4096, std::atoi(e)));
    if (const char* e = std::getenv("FF_QUEUE_COUNTERS")) w.queue_counters = std::max(1, std::min(kQueueCounters, std::atoi(e)));
    w.no_wall_table = std::getenv("FF_NO_WALL_TABLE") != nullptr;
    w.no_wall_pairs = std::getenv("FF_NO_WALL_PAIRS") != nullptr;
    w.no_stack_spill = std::getenv("FF_NO_STACK_SPILL") != nullptr;
    w.no_scan_planes = std::getenv("FF_NO_SCAN_PLANES") != nullptr;
    if (const char* e = std::getenv("FF_DEBUG_LDS_FILL")) w.lds_fill = std::sscanf(e, "%lu,%lx", &w.lds_fill_words, &w.lds_fill_pattern) == 2;
    if (const char* e = std::getenv("FF_POOL")) w.pool = std::atoi(e) != 0 ? 1 : 0;
    if (const char* e = std::getenv("FF_POOL_QUORUM")) w.pool_quorum = std::max(1, std::min(64, std::atoi(e)));
    if (const char* e = std::getenv("FF_POOL_QUORUM_MIN")) w.pool_quorum_min = std::max(1, std::min(64, std::atoi(e)));
    if (const char* e = std::getenv("FF_POOL_REFILL")) w.pool_refill = std::max(1, std::min(64, std::atoi(e)));
    if (const char* e = std::getenv("FF_POOL_SLICE")) w.pool_slice = std::max(1, std::min(64, std::atoi(e)));
    if (const char* e = std::getenv("FF_POOL_BATCH_MIN")) w.pool_batch_min = std::max(1, std::min(1024, std::atoi(e)));
    if (const char* e = std::getenv("FF_DEBUG_LDS_NODE_CAP")) w.lds_node_cap = std::max(0, std::atoi(e));
    if (const char* e = std::getenv("FF_QUEUE_TAIL")) w.queue_tail = std::max(0, std::min(4096, std::atoi(e)));
    if (const char* e = std::getenv("FF_POOL_LEAVE")) w.pool_leave = std::max(0, std::min(64, std::atoi(e)));
    if (const char* e = std::getenv("FF_POOL_STACK_LEVELS")) w.pool_stack_levels = std::max(1, std::min(64, std::atoi(e)));
    w.grade_no_lds = std::getenv("FF_GRADE_NO_LDS") != nullptr;
    s->sw = w;
}

} // namespace

extern "C" {

int ff_debug_reload_switches(FfState* s)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_debug_reload_switches: state is null");
    read_switches(s);
    s->primary_valid = s->last_key_valid = false; // (what the stored hits and their mask were computed under may just have changed)
    return FF_OK;
}

int ff_create(FfState** out_state, int device_id)
{
    clear_error();
    if (!out_state) return fail(FF_ERR_INVALID_ARG, "ff_create: out_state is null");
    *out_state = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) return fail(FF_ERR_NO_DEVICE, "ff_create: no HIP device (%s)", hipGetErrorString(e));
    if (device_id < 0 || device_id >= count) return fail(FF_ERR_INVALID_ARG, "ff_create: device %d out of range (0..%d)", device_id, count - 1);
    FF_HIP(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    FF_HIP(hipGetDeviceProperties(&prop, device_id));
    FfState* s = new (std::nothrow) FfState();
    if (!s) return fail(FF_ERR_OOM, "ff_create: out of host memory");
    s->device = device_id;
    s->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    s->device_mem_bytes = prop.totalGlobalMem;
    if (const char* bt = std::getenv("FF_BLOCK_THREADS")) {
        const int v = std::atoi(bt);
        if (v == 512 || v == 768 || v == 1024) {
            s->block_threads = v;
        }
    }
    read_switches(s);
    if (const char* e = std::getenv("FF_DEBUG_FAIL_ALLOC")) s->debug_fail_alloc = std::atoi(e);
    if (const char* e = std::getenv("FF_DEBUG_TIMELINE_US")) s->timeline_bucket_us = std::max(0, std::atoi(e));
    if (const char* e = std::getenv("FF_TAIL_MIN_BLOCKS")) s->tail_min_blocks = std::max(1, std::atoi(e));
    if (const char* e = std::getenv("FF_TAIL_GROUP")) {
        s->tail_group_spp = std::max(0, std::min(64, std::atoi(e)));
        s->tail_forced = true;
    }
    if (const char* e = std::getenv("FF_SETUP_THRESHOLD")) {
        s->setup_threshold = std::max(0, std::min(1 << 14, std::atoi(e)));
        s->setup_threshold_forced = true;
    }
    if (const char* e = std::getenv("FF_LEAF_THRESHOLD")) s->leaf_threshold = std::max(1, std::min(64, std::atoi(e)));
    hipError_t pe = prepare_kernels();
    if (pe != hipSuccess) {
        delete s;
        return fail(FF_ERR_HIP, "ff_create: kernel preparation failed: %s (is this a gfx950 device?)", hipGetErrorString(pe));
    }
    if (hipMalloc((void**)&s->d_counters, (size_t)(1 + kQueueCounters) * kQueueStride * sizeof(unsigned)) != hipSuccess || // counters, then the work-queue counters 4 KiB apart
        hipHostMalloc((void**)&s->h_counters, kCounterWords * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess ||
        hipEventCreate(&s->ev_begin) != hipSuccess || hipEventCreate(&s->ev_end) != hipSuccess) {
        ff_destroy(s);
        return fail(FF_ERR_HIP, "ff_create: allocating work buffers failed");
    }
    s->d_queue = reinterpret_cast<unsigned*>(s->d_counters) + kQueueStride;
    *out_state = s;
    return FF_OK;
}

int ff_destroy(FfState* s)
{
    if (!s) return FF_OK;
    (void)hipSetDevice(s->device);
    if (s->pbo_resource) (void)hipGraphicsUnregisterResource(s->pbo_resource);
    dist_release(s);
    free_scene(s);
    if (s->d_stage) (void)hipFree(s->d_stage);
    if (s->d_tail_samples) (void)hipFree(s->d_tail_samples);
    if (s->d_stack_spill) (void)hipFree(s->d_stack_spill);
    if (s->d_cull_mask) (void)hipFree(s->d_cull_mask);
    if (s->d_primary_cache) (void)hipFree(s->d_primary_cache);
    if (s->d_start_records) (void)hipFree(s->d_start_records);
    if (s->d_park) (void)hipFree(s->d_park);
    if (s->d_accum) (void)hipFree(s->d_accum);
    if (s->d_frame) (void)hipFree(s->d_frame);
    if (s->d_gb_hits) (void)hipFree(s->d_gb_hits);
    if (s->d_img_work) (void)hipFree(s->d_img_work);
    if (s->d_dn_work) (void)hipFree(s->d_dn_work);
    for (ReprojectionHistory& h : s->history) h.release();
    if (s->d_nee_lights) (void)hipFree(s->d_nee_lights);
    if (s->d_nee_pdf) (void)hipFree(s->d_nee_pdf);
    env_release(s);
    tex_release(s);
    glossy_release(s);
    display_release(s);
    adaptive_release(s);
    yuv_release(s);
    resize_release(s);
    grade_release(s);
    lens_release(s);
    free_build_scratch(s->scratch);
    if (s->d_blocksums) (void)hipFree(s->d_blocksums);
    if (s->d_rgb8) (void)hipFree(s->d_rgb8);
    if (s->d_radiance) (void)hipFree(s->d_radiance);
    if (s->d_counters) (void)hipFree(s->d_counters);
    if (s->d_timeline) (void)hipFree(s->d_timeline);
    if (s->h_counters) (void)hipHostFree(s->h_counters);
    if (s->ev_begin) (void)hipEventDestroy(s->ev_begin);
    if (s->ev_end) (void)hipEventDestroy(s->ev_end);
    delete s;
    return FF_OK;
}

int ff_set_stream(FfState* s, void* hip_stream)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_set_stream: state is null");
    s->stream = (hipStream_t)hip_stream;
    return FF_OK;
}

// ---- sub-pixel jitter of the primary rays (composed into the ray matrix by fill_frame_mapping) ------------------------

int ff_set_pixel_jitter(FfState* s, float jx, float jy)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_set_pixel_jitter: state is null");
    if (!(jx >= 0.f && jx < 1.f && jy >= 0.f && jy < 1.f))
        return fail(FF_ERR_INVALID_ARG, "ff_set_pixel_jitter: the jitter must be finite and in [0, 1) (got %g %g)", (double)jx, (double)jy);
    s->jitter_x = jx;
    s->jitter_y = jy;
    return FF_OK;
}

// ---- measurement ---------------------------------------------------------------------------------------------------

int ff_set_collect_stats(FfState* s, int on)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_set_collect_stats: state is null");
    s->collect_stats = on != 0;
    return FF_OK;
}

int ff_debug_timeline(FfState* s, unsigned* out1024, int* bucket_us)
{
    clear_error();
    if (!s || !out1024 || !bucket_us) return fail(FF_ERR_INVALID_ARG, "ff_debug_timeline: null argument");
    std::memset(s->h_timeline, 0, sizeof s->h_timeline);
    for (size_t i = 0; i < s->h_timeline_rows.size(); ++i) s->h_timeline[i % kTimelineBuckets] += s->h_timeline_rows[i];
    std::memcpy(out1024, s->h_timeline, sizeof s->h_timeline);
    *bucket_us = s->timeline_bucket_us;
    return FF_OK;
}

int ff_debug_counters(FfState* s, unsigned long long* out32)
{
    clear_error();
    if (!s || !out32) return fail(FF_ERR_INVALID_ARG, "ff_debug_counters: null argument");
    std::memcpy(out32, s->raw_counters, sizeof s->raw_counters);
    return FF_OK;
}

int ff_debug_check_ieee(FfState* s, unsigned long long* out_mismatches2)
{
    clear_error();
    if (!s || !out_mismatches2) return fail(FF_ERR_INVALID_ARG, "ff_debug_check_ieee: null argument");
    FF_HIP(hipSetDevice(s->device));
    FF_HIP(hipMemsetAsync(s->d_counters, 0, 2 * sizeof(unsigned long long), s->stream));
    FF_HIP(launch_ieee_check(s->d_counters, s->stream));
    FF_HIP(hipMemcpyAsync(out_mismatches2, s->d_counters, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->stream));
    FF_HIP(hipStreamSynchronize(s->stream));
    return FF_OK;
}

const char* ff_debug_kernel_name(FfState* s) { return s && s->last_kernel_name ? s->last_kernel_name : ""; }

int ff_debug_layout(FfState* s, int* out8)
{
    clear_error();
    if (!s || !out8) return fail(FF_ERR_INVALID_ARG, "ff_debug_layout: null argument");
    if (!s->has_scene) return fail(FF_ERR_NO_SCENE, "ff_debug_layout: no scene uploaded");
    const int v[8] = { s->scene_block_threads, s->stack_entries, s->stack_lds_levels, s->lds_cap, s->setup_threshold, s->leaf_threshold, s->max_depth4, s->top_depth };
    std::memcpy(out8, v, sizeof v);
    return FF_OK;
}

// No stack entry equals this word (ff_k_traverse.h inner_step / pop_entry are the only writers): a leaf is ~ref, negative, and so is
// a geometry-tree leaf ~(kGeomLeaf | record); an inner link is a node index below 1 << 22; a packed entry has kPackedEntry (bit 30)
// set.  The sentinel is non-negative, at least 1 << 22 and has bit 30 clear.
constexpr unsigned kSpillSentinel = 0x2A5A5A5Au;
static_assert((int)kSpillSentinel >= (1 << 22) && (kSpillSentinel & 0x40000000u) == 0u, "the sentinel must lie outside the stack entries' encodings");

int ff_debug_stack_spill(FfState* s, int reset, unsigned long long* words)
{
    clear_error();
    if (!s || !words) return fail(FF_ERR_INVALID_ARG, "ff_debug_stack_spill: null argument");
    *words = 0;
    const size_t n = s->d_stack_spill ? s->stack_spill_bytes / sizeof(unsigned) : 0;
    if (n == 0) return FF_OK;
    FF_HIP(hipSetDevice(s->device));
    if (reset) {
        std::vector<unsigned> fill(n, kSpillSentinel);
        FF_HIP(hipMemcpyAsync(s->d_stack_spill, fill.data(), n * sizeof(unsigned), hipMemcpyHostToDevice, s->stream));
        FF_HIP(hipStreamSynchronize(s->stream)); // (`fill` goes out of scope)
        return FF_OK;
    }
    std::vector<unsigned> got(n);
    FF_HIP(hipMemcpyAsync(got.data(), s->d_stack_spill, n * sizeof(unsigned), hipMemcpyDeviceToHost, s->stream));
    FF_HIP(hipStreamSynchronize(s->stream));
    *words = (unsigned long long)std::count_if(got.begin(), got.end(), [](unsigned w) { return w != kSpillSentinel; });
    return FF_OK;
}

int ff_stats(FfState* s, FfStats* out)
{
    clear_error();
    if (!s || !out) return fail(FF_ERR_INVALID_ARG, "ff_stats: null argument");
    *out = s->stats;
    return FF_OK;
}

} // extern "C"
