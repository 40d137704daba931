// ff_render_api.cpp — the single-device render entry points behind the C ABI (include/firefly/ff_api.h): the parameter checks, whole
// frames, strips and tiles into host or device buffers (RenderOutputs, ff_state.h), ray batches, HIP-GL pixel-buffer interop and
// progressive accumulation.  The frame itself (kernel.cu:335-344) is ff_frame.cpp; every entry point here goes through its
// render_enqueue / render_finish.
#include <chrono>

#include <hip/hip_runtime.h>
// (the interop header relies on hip_runtime.h having been included first)
#include <hip/hip_gl_interop.h>

#include "ff_state.h"

using namespace ff;

namespace {

int check_params(const FfRenderParams* p)
{
    if (!p) return fail(FF_ERR_INVALID_ARG, "render params are null");
    if (p->width <= 0 || p->height <= 0) return fail(FF_ERR_INVALID_ARG, "image size %dx%d is invalid", p->width, p->height);
    if (p->width > 65535 || p->height > 65535) return fail(FF_ERR_INVALID_ARG, "image size %dx%d exceeds 65535 per side", p->width, p->height);
    if (p->bounces < 1 || p->bounces > 255) return fail(FF_ERR_INVALID_ARG, "bounces must be in 1..255 (got %d)", p->bounces);
    if (p->spp < 1 || p->spp >= (1 << 24)) return fail(FF_ERR_INVALID_ARG, "spp must be in 1..2^24-1 (got %d)", p->spp);
    if (p->trace_mode != FF_TRACE_BRUTE_FORCE && p->trace_mode != FF_TRACE_BVH) return fail(FF_ERR_INVALID_ARG, "unknown trace_mode %d", p->trace_mode);
    if (p->shade_mode != FF_SHADE_NORMAL_DEBUG && p->shade_mode != FF_SHADE_DIFFUSE_PATH && p->shade_mode != FF_SHADE_DIFFUSE_PATH_SMOOTH &&
        p->shade_mode != FF_SHADE_DIFFUSE_PATH_NEE) return fail(FF_ERR_INVALID_ARG, "unknown shade_mode %d", p->shade_mode);
    if (p->grid_mode != FF_GRID_FULL && p->grid_mode != FF_GRID_REFERENCE_FLOOR) return fail(FF_ERR_INVALID_ARG, "unknown grid_mode %d", p->grid_mode);
    if (p->spp_per_launch < 0) return fail(FF_ERR_INVALID_ARG, "spp_per_launch must be >= 0");
    return FF_OK;
}

int render_local(FfState* s, const FfCamera* camera, const FfRenderParams* prm, int strip_rows, int part, int num_parts, int local_rows,
                 unsigned char* rgb8_dev, float* radiance_dev, int x0 = 0, int y0 = 0, int win_w = -1)
{
    const int st = render_enqueue(s, camera, prm, strip_rows, part, num_parts, local_rows, rgb8_dev, radiance_dev, x0, y0, win_w);
    if (st != FF_OK) return st;
    return render_finish(s);
}

// Frame `frame_index` of a progressive sequence into device buffers: an ordinary frame with seed + frame_index, added to
// the running sum; outputs are the mean over frames 0..frame_index.
int progressive_frame(FfState* s, const FfCamera* camera, const FfRenderParams* params, int frame_index, unsigned char* rgb8_dev, float* mean_dev)
{
    if (frame_index < 0) return fail(FF_ERR_INVALID_ARG, "ff_render_progressive: frame index %d", frame_index);
    if (frame_index > 0 && (params->width != s->accum_width || params->height != s->accum_height || frame_index != s->accum_frames))
        return fail(FF_ERR_INVALID_ARG, "ff_render_progressive: frame %d does not continue the running sequence (%d frames of %dx%d); restart with frame 0",
                    frame_index, s->accum_frames, s->accum_width, s->accum_height);
    const size_t values = (size_t)params->width * (size_t)params->height * 3;
    int st = ensure_bytes((void**)&s->d_frame, &s->frame_bytes, values * sizeof(float) + 16);
    if (st == FF_OK) st = ensure_bytes((void**)&s->d_accum, &s->accum_bytes, values * sizeof(float) + 16);
    if (st != FF_OK) return st;
    FfRenderParams p = *params;
    p.seed = params->seed + (uint64_t)frame_index;
    st = render_local(s, camera, &p, params->height, 0, 1, params->height, nullptr, s->d_frame);
    if (st != FF_OK) return st;
    const float inv = 1.0f / (float)(frame_index + 1);
    FF_HIP(launch_accumulate(s->d_accum, s->d_frame, mean_dev, rgb8_dev, values, frame_index == 0 ? 1 : 0, inv, s->stream));
    FF_HIP(hipStreamSynchronize(s->stream));
    s->accum_width = params->width;
    s->accum_height = params->height;
    s->accum_frames = frame_index + 1;
    return FF_OK;
}

} // namespace

namespace ff {

int check_render_call(const FfState* s, const FfCamera* camera, const FfRenderParams* params, const char* who)
{
    if (!s) return fail(FF_ERR_INVALID_ARG, "%s: state is null", who);
    if (!camera) return fail(FF_ERR_INVALID_ARG, "%s: camera is null", who);
    const int st = check_params(params);
    if (st != FF_OK) return st;
    if (!s->has_scene) return fail(FF_ERR_NO_SCENE, "%s: no scene uploaded", who);
    return FF_OK;
}

// The registered pixel buffer, mapped for writing: the device pointer of at least need_bytes.  A mapping that gives no such
// pointer is undone here, so the caller unmaps (unmap_pbo) exactly when this returned FF_OK.
int map_pbo(FfState* s, size_t need_bytes, void** out_ptr)
{
    size_t nbytes = 0;
    FF_HIP(hipGraphicsMapResources(1, &s->pbo_resource, s->stream));
    hipError_t e = hipGraphicsResourceGetMappedPointer(out_ptr, &nbytes, s->pbo_resource);
    if (e == hipSuccess && nbytes < need_bytes) e = hipErrorInvalidValue;
    if (e == hipSuccess) return FF_OK;
    const int st = fail(FF_ERR_HIP, "mapping the pixel buffer failed: %s", hipGetErrorString(e));
    (void)hipGraphicsUnmapResources(1, &s->pbo_resource, s->stream);
    return st;
}

// ... and unmapped; status: what the work in between returned (it is kept; a failing unmap shows only after a success).
int unmap_pbo(FfState* s, int status)
{
    const hipError_t ue = hipGraphicsUnmapResources(1, &s->pbo_resource, s->stream);
    if (status == FF_OK && ue != hipSuccess) return fail(FF_ERR_HIP, "hipGraphicsUnmapResources failed: %s", hipGetErrorString(ue));
    return status;
}

} // namespace ff

extern "C" {

int ff_check_render_params(const FfRenderParams* params)
{
    clear_error();
    return check_params(params);
}

int ff_strips_local_rows(int height, int strip_rows, int part, int num_parts)
{
    if (height <= 0 || strip_rows <= 0 || num_parts <= 0 || part < 0 || part >= num_parts) return 0;
    const int nstrips = (height + strip_rows - 1) / strip_rows;
    int rows = 0;
    for (int sidx = part; sidx < nstrips; sidx += num_parts) {
        const int y0 = sidx * strip_rows;
        rows += (y0 + strip_rows <= height) ? strip_rows : height - y0;
    }
    return rows;
}

int ff_render_strips(FfState* s, const FfCamera* camera, const FfRenderParams* params, int strip_rows, int part, int num_parts, void* rgb8,
                     int rgb8_on_device, float* radiance, int radiance_on_device, int* out_local_rows)
{
    clear_error();
    const auto t0 = std::chrono::steady_clock::now();
    int st = check_render_call(s, camera, params, "ff_render");
    if (st != FF_OK) return st;
    if (strip_rows <= 0 || num_parts <= 0 || part < 0 || part >= num_parts) return fail(FF_ERR_INVALID_ARG, "ff_render_strips: bad strip partition (%d rows, part %d of %d)", strip_rows, part, num_parts);
    FF_HIP(hipSetDevice(s->device));
    const int local_rows = ff_strips_local_rows(params->height, strip_rows, part, num_parts);
    if (out_local_rows) *out_local_rows = local_rows;
    const size_t local_pixels = (size_t)local_rows * (size_t)params->width;
    RenderOutputs out(s, local_pixels, rgb8, rgb8_on_device, radiance, radiance_on_device);
    if (out.status != FF_OK) return out.status;
    st = render_local(s, camera, params, strip_rows, part, num_parts, local_rows, out.rgb8, out.radiance);
    if (st != FF_OK) return st;
    st = out.copy_back();
    if (st != FF_OK) return st;
    s->stats.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return FF_OK;
}

int ff_render_tile(FfState* s, const FfCamera* camera, const FfRenderParams* params, int x0, int y0, int w, int h, void* rgb8, int rgb8_on_device,
                   float* radiance, int radiance_on_device)
{
    clear_error();
    const auto t0 = std::chrono::steady_clock::now();
    int st = check_render_call(s, camera, params, "ff_render_tile");
    if (st != FF_OK) return st;
    if (x0 < 0 || y0 < 0 || w <= 0 || h <= 0 || x0 + w > params->width || y0 + h > params->height)
        return fail(FF_ERR_INVALID_ARG, "ff_render_tile: tile %dx%d at (%d, %d) is not inside the %dx%d image", w, h, x0, y0, params->width, params->height);
    FF_HIP(hipSetDevice(s->device));
    RenderOutputs out(s, (size_t)w * (size_t)h, rgb8, rgb8_on_device, radiance, radiance_on_device);
    if (out.status != FF_OK) return out.status;
    st = render_local(s, camera, params, h, 0, 1, h, out.rgb8, out.radiance, x0, y0, w);
    if (st != FF_OK) return st;
    st = out.copy_back();
    if (st != FF_OK) return st;
    s->stats.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return FF_OK;
}

int ff_render(FfState* s, const FfCamera* camera, const FfRenderParams* params, void* rgb8, int rgb8_on_device, float* radiance,
              int radiance_on_device)
{
    const int h = params ? params->height : 1;
    return ff_render_strips(s, camera, params, h > 0 ? h : 1, 0, 1, rgb8, rgb8_on_device, radiance, radiance_on_device, nullptr);
}

int ff_deinterleave_strips(FfState* s, const void* src_dev, void* dst_dev, int width, int height, int strip_rows, int num_parts, int elem_bytes)
{
    clear_error();
    if (!s || !src_dev || !dst_dev) return fail(FF_ERR_INVALID_ARG, "ff_deinterleave_strips: null argument");
    if (width <= 0 || height <= 0 || strip_rows <= 0 || num_parts <= 0 || elem_bytes <= 0) return fail(FF_ERR_INVALID_ARG, "ff_deinterleave_strips: bad geometry");
    FF_HIP(hipSetDevice(s->device));
    FF_HIP(launch_deinterleave(src_dev, dst_dev, width, height, strip_rows, num_parts, elem_bytes, s->stream));
    FF_HIP(hipStreamSynchronize(s->stream));
    return FF_OK;
}

int ff_intersect_rays(FfState* s, const FfRay* rays, int n, FfIntersect* out, int trace_mode)
{
    clear_error();
    if (!s || !rays || !out) return fail(FF_ERR_INVALID_ARG, "ff_intersect_rays: null argument");
    if (n < 0) return fail(FF_ERR_INVALID_ARG, "ff_intersect_rays: negative count");
    if (trace_mode != FF_TRACE_BRUTE_FORCE && trace_mode != FF_TRACE_BVH) return fail(FF_ERR_INVALID_ARG, "unknown trace_mode %d", trace_mode);
    if (!s->has_scene) return fail(FF_ERR_NO_SCENE, "ff_intersect_rays: no scene uploaded");
    if (n == 0) return FF_OK;
    if (trace_mode == FF_TRACE_BVH && s->scene_block_threads == 0)
        return fail(FF_ERR_UNSUPPORTED, "ff_intersect_rays: 4-wide BVH of depth %d does not fit the LDS traversal stack; use FF_TRACE_BRUTE_FORCE or a host-built tree", s->max_depth4);
    FF_HIP(hipSetDevice(s->device));
    FfRay* d_rays = nullptr;
    FfIntersect* d_out = nullptr;
    FF_HIP(hipMalloc((void**)&d_rays, (size_t)n * sizeof(FfRay)));
    hipError_t e = hipMalloc((void**)&d_out, (size_t)n * sizeof(FfIntersect));
    if (e != hipSuccess) {
        (void)hipFree(d_rays);
        return fail(FF_ERR_HIP, "hipMalloc failed: %s", hipGetErrorString(e));
    }
    RayBatchParams p;
    p.rays = d_rays;
    p.out = d_out;
    p.n = n;
    p.num_geoms = s->num_geoms;
    p.num_planes = s->num_planes;
    p.num_quads = s->num_quads;
    p.geoms = s->d_geoms;
    p.tris = s->d_tris;
    p.nodes4 = s->d_nodes4;
    p.stack_depth = s->stack_lds_levels;
    p.stack_spill = nullptr;
    if (trace_mode == FF_TRACE_BVH && s->stack_lds_levels < s->stack_entries) {
        const size_t threads = (size_t)((n + kBlockThreads - 1) / kBlockThreads) * (size_t)kBlockThreads;
        const int sst = ensure_bytes((void**)&s->d_stack_spill, &s->stack_spill_bytes, (size_t)(s->stack_entries - s->stack_lds_levels) * threads * sizeof(int));
        if (sst != FF_OK) {
            (void)hipFree(d_rays);
            (void)hipFree(d_out);
            return sst;
        }
        p.stack_spill = s->d_stack_spill;
    }
    p.top_first = (int)s->node_capacity;
    p.top_lds_first = 0;
    p.top_lds_count = s->top_lds_count;
    p.num_scan = s->num_scan;
    p.walls = s->walls;
    p.guard_hits = s->d_counters;
    e = hipMemsetAsync(s->d_counters, 0, sizeof(unsigned long long), s->stream);
    p.lds_nodes = s->lds_cap; // (the records' LDS shares were laid out for the trace kernel's workgroup; 512 threads leave more room, never less)
    if (e == hipSuccess) e = hipMemcpy(d_rays, rays, (size_t)n * sizeof(FfRay), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_ray_batch(p, trace_mode, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    unsigned long long cut = 0;
    if (e == hipSuccess) e = hipMemcpy(&cut, s->d_counters, sizeof cut, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out, d_out, (size_t)n * sizeof(FfIntersect), hipMemcpyDeviceToHost);
    (void)hipFree(d_rays);
    (void)hipFree(d_out);
    if (e != hipSuccess) return fail(FF_ERR_HIP, "ff_intersect_rays failed: %s", hipGetErrorString(e));
    if (cut != 0) return fail(FF_ERR_HIP, "ff_intersect_rays: the traversal loop guard cut %llu queries short (a malformed or absurdly deep tree)", cut);
    return FF_OK;
}

// ---- OpenGL pixel-buffer interop ---------------------------------------------------------------------------------

int ff_register_gl_pbo(FfState* s, unsigned int pbo, int width, int height)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_register_gl_pbo: state is null");
    if (width <= 0 || height <= 0) return fail(FF_ERR_INVALID_ARG, "ff_register_gl_pbo: bad size");
    (void)hipSetDevice(s->device);
    if (s->pbo_resource) {
        (void)hipGraphicsUnregisterResource(s->pbo_resource);
        s->pbo_resource = nullptr;
    }
    // utilities.h:618: cudaGraphicsGLRegisterBuffer(&pboCudaResource, pbo, cudaGraphicsRegisterFlagsWriteDiscard)
    hipGraphicsResource* res = nullptr;
    hipError_t e = hipGraphicsGLRegisterBuffer(&res, (GLuint)pbo, hipGraphicsRegisterFlagsWriteDiscard);
    if (e != hipSuccess || !res) {
        (void)hipGetLastError();
        return fail(FF_ERR_GL_UNAVAILABLE, "hipGraphicsGLRegisterBuffer(%u) failed: %s (is a GL context current on this thread?)", pbo, hipGetErrorString(e));
    }
    s->pbo_resource = res;
    s->pbo_width = width;
    s->pbo_height = height;
    return FF_OK;
}

int ff_unregister_gl_pbo(FfState* s)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_unregister_gl_pbo: state is null");
    if (!s->pbo_resource) return FF_OK;
    (void)hipSetDevice(s->device);
    hipError_t e = hipGraphicsUnregisterResource(s->pbo_resource); // utilities.h:516
    s->pbo_resource = nullptr;
    if (e != hipSuccess) return fail(FF_ERR_HIP, "hipGraphicsUnregisterResource failed: %s", hipGetErrorString(e));
    return FF_OK;
}

int ff_render_to_pbo(FfState* s, const FfCamera* camera, const FfRenderParams* params)
{
    clear_error();
    const auto t0 = std::chrono::steady_clock::now();
    if (s && !s->pbo_resource) return fail(FF_ERR_GL_UNAVAILABLE, "ff_render_to_pbo: no pixel buffer registered");
    int st = check_render_call(s, camera, params, "ff_render_to_pbo");
    if (st != FF_OK) return st;
    if (params->width != s->pbo_width || params->height != s->pbo_height)
        return fail(FF_ERR_INVALID_ARG, "ff_render_to_pbo: params are %dx%d but the registered buffer is %dx%d", params->width, params->height, s->pbo_width, s->pbo_height);
    FF_HIP(hipSetDevice(s->device));
    // kernel.cu:335-344
    void* dptr = nullptr;
    st = map_pbo(s, (size_t)params->width * (size_t)params->height * 3, &dptr); // :338-339
    if (st == FF_OK) {
        st = render_local(s, camera, params, params->height, 0, 1, params->height, (unsigned char*)dptr, nullptr); // :340-342
        st = unmap_pbo(s, st);                                                                                       // :344
    }
    s->stats.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return st;
}

// ---- progressive accumulation ("progressive accumulation across frames while the camera is still") ----

int ff_render_progressive(FfState* s, const FfCamera* camera, const FfRenderParams* params, int frame_index, void* rgb8, int rgb8_on_device, float* radiance,
                          int radiance_on_device)
{
    clear_error();
    const auto t0 = std::chrono::steady_clock::now();
    int st = check_render_call(s, camera, params, "ff_render_progressive");
    if (st != FF_OK) return st;
    FF_HIP(hipSetDevice(s->device));
    // (the frame itself goes to d_frame, so d_radiance is free for the mean)
    RenderOutputs out(s, (size_t)params->width * (size_t)params->height, rgb8, rgb8_on_device, radiance, radiance_on_device);
    if (out.status != FF_OK) return out.status;
    st = progressive_frame(s, camera, params, frame_index, out.rgb8, out.radiance);
    if (st != FF_OK) return st;
    st = out.copy_back();
    if (st != FF_OK) return st;
    s->stats.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return FF_OK;
}

int ff_render_to_pbo_progressive(FfState* s, const FfCamera* camera, const FfRenderParams* params, int frame_index)
{
    clear_error();
    const auto t0 = std::chrono::steady_clock::now();
    if (s && !s->pbo_resource) return fail(FF_ERR_GL_UNAVAILABLE, "ff_render_to_pbo_progressive: no pixel buffer registered");
    int st = check_render_call(s, camera, params, "ff_render_to_pbo_progressive");
    if (st != FF_OK) return st;
    if (params->width != s->pbo_width || params->height != s->pbo_height)
        return fail(FF_ERR_INVALID_ARG, "ff_render_to_pbo_progressive: params are %dx%d but the registered buffer is %dx%d", params->width, params->height,
                    s->pbo_width, s->pbo_height);
    FF_HIP(hipSetDevice(s->device));
    void* dptr = nullptr;
    st = map_pbo(s, (size_t)params->width * (size_t)params->height * 3, &dptr);
    if (st == FF_OK) st = unmap_pbo(s, progressive_frame(s, camera, params, frame_index, (unsigned char*)dptr, nullptr));
    s->stats.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return st;
}

} // extern "C"
