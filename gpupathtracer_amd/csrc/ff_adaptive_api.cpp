// ff_adaptive_api.cpp — host side of ff_render_adaptive (include/firefly/ff_api.h): the argument checks, the rectangle plan, the
// driver that renders pass after pass through render_enqueue / render_finish (ff_state.h; one pair per rectangle) and spends the
// later passes only on the tiles whose error estimate is still at or above the threshold, the state's buffers, and the loops of the
// host-only twin ff_adaptive_tile_error_host over ff_adaptive.h's inline functions.  The kernels are in ff_adaptive.hip.  Nothing of
// a pass's tracing is decided here: a rectangle is a frame's window, as ff_render_tile's is.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

#include <hip/hip_runtime.h>

#include "ff_adaptive.h"
#include "ff_state.h"

using namespace ff;

namespace {

// What ff_render_adaptive refuses of its own parameter block, in the order of the fields.
int check_adaptive_params(const FfAdaptiveParams* ap, const char* who)
{
    if (!ap) return fail(FF_ERR_INVALID_ARG, "%s: adaptive params (ap) are null", who);
    if (!adaptive_tile_ok(ap->tile)) return fail(FF_ERR_INVALID_ARG, "%s: tile must be 16, 32, 64 or 128 (got %d)", who, ap->tile);
    if (ap->min_passes < 2 || (ap->min_passes & 1)) return fail(FF_ERR_INVALID_ARG, "%s: min_passes must be even and >= 2 (got %d)", who, ap->min_passes);
    if (ap->max_passes < ap->min_passes || (ap->max_passes & 1) || ap->max_passes > kAdaptiveMaxPasses)
        return fail(FF_ERR_INVALID_ARG, "%s: max_passes must be even and min_passes .. %d (got %d)", who, kAdaptiveMaxPasses, ap->max_passes);
    if (ap->threshold != ap->threshold || ap->threshold == -INFINITY)
        return fail(FF_ERR_INVALID_ARG, "%s: threshold must be finite or +inf (got %g)", who, (double)ap->threshold);
    if (ap->flags & ~(uint32_t)FF_ADAPTIVE_GUARD_NEIGHBOURS) return fail(FF_ERR_INVALID_ARG, "%s: unknown flags 0x%x", who, ap->flags);
    if (ap->reserved != 0) return fail(FF_ERR_INVALID_ARG, "%s: reserved must be 0", who);
    return FF_OK;
}

// What both tile-error entry points check; fills the kernel arguments.
int check_tile_error(int width, int height, int tile, int n, const float* sum, const float* sum_even, const float* out_error, AdaptiveArgs* a, const char* who)
{
    if (check_image_size(width, height, who) != FF_OK) return FF_ERR_INVALID_ARG;
    if (!adaptive_tile_ok(tile)) return fail(FF_ERR_INVALID_ARG, "%s: tile must be 16, 32, 64 or 128 (got %d)", who, tile);
    if (n < 2 || (n & 1) || n > kAdaptiveMaxPasses) return fail(FF_ERR_INVALID_ARG, "%s: n must be even and 2 .. %d (got %d)", who, kAdaptiveMaxPasses, n);
    if (!sum) return fail(FF_ERR_INVALID_ARG, "%s: sum is null", who);
    if (!sum_even) return fail(FF_ERR_INVALID_ARG, "%s: sum_even is null", who);
    if (!out_error) return fail(FF_ERR_INVALID_ARG, "%s: out_error is null", who);
    *a = make_adaptive_args(width, height, tile, n);
    return FF_OK;
}

// The places of the per-tile arrays in FfState::Adaptive::d_tiles: the errors, the list of tiles to check, the pass counts.
struct TileBuffers {
    float* error;
    uint32_t* list;
    uint16_t* passes;
};

int tile_buffers(FfState* s, size_t tiles, TileBuffers* out)
{
    const int st = ensure_bytes(&s->adaptive.d_tiles, &s->adaptive.tiles_bytes, tiles * (sizeof(float) + sizeof(uint32_t) + sizeof(uint16_t)) + 16);
    if (st != FF_OK) return st;
    out->error = (float*)s->adaptive.d_tiles;
    out->list = (uint32_t*)(out->error + tiles);
    out->passes = (uint16_t*)(out->list + tiles);
    return FF_OK;
}

// One check of the driver: the tiles whose error is below the threshold stop; under `guard`, only those whose neighbours are below
// it too (a neighbour that stopped at an earlier check counts as below).  Returns the number of tiles still active.
int stop_converged_tiles(int tiles_x, int tiles_y, const std::vector<float>& error, float threshold, bool guard, std::vector<uint8_t>& active)
{
    const size_t tiles = active.size();
    std::vector<uint8_t> below(tiles);
    for (size_t t = 0; t < tiles; ++t) below[t] = !active[t] || error[t] < threshold;
    int left = 0;
    for (int ty = 0; ty < tiles_y; ++ty)
        for (int tx = 0; tx < tiles_x; ++tx) {
            const size_t t = (size_t)ty * (size_t)tiles_x + (size_t)tx;
            if (!active[t]) continue;
            bool stop = below[t] != 0;
            if (guard)
                for (int qy = ty - 1; qy <= ty + 1 && stop; ++qy)
                    for (int qx = tx - 1; qx <= tx + 1 && stop; ++qx)
                        if (qx >= 0 && qy >= 0 && qx < tiles_x && qy < tiles_y) stop = below[(size_t)qy * (size_t)tiles_x + (size_t)qx] != 0;
            if (stop) active[t] = 0;
            else ++left;
        }
    return left;
}

} // namespace

namespace ff {

void adaptive_release(FfState* s)
{
    FfState::Adaptive& ad = s->adaptive;
    if (ad.d_planes) (void)hipFree(ad.d_planes);
    if (ad.d_tiles) (void)hipFree(ad.d_tiles);
    if (ad.d_stage) (void)hipFree(ad.d_stage);
    ad = FfState::Adaptive();
}

} // namespace ff

extern "C" {

void ff_adaptive_params_init(FfAdaptiveParams* p)
{
    if (!p) return;
    // 
    p->tile = 64;
    p->min_passes = 2;
    p->max_passes = 64;
    p->threshold = 0.0002f;
    p->flags = 0;
    p->reserved = 0;
}

int ff_adaptive_plan_host(int tiles_x, int tiles_y, const uint8_t* active, int32_t* out_rects4, int max_rects)
{
    clear_error();
    if (tiles_x < 1 || tiles_y < 1) return fail(FF_ERR_INVALID_ARG, "ff_adaptive_plan_host: grid size %dx%d is invalid", tiles_x, tiles_y), -1;
    if (!active) return fail(FF_ERR_INVALID_ARG, "ff_adaptive_plan_host: active is null"), -1;
    if (!out_rects4) return fail(FF_ERR_INVALID_ARG, "ff_adaptive_plan_host: out_rects4 is null"), -1;
    int count = 0;
    std::vector<int> open, next; // the rectangles that reach the row above / this row (indices into out_rects4)
    for (int ty = 0; ty < tiles_y; ++ty) {
        const uint8_t* row = active + (size_t)ty * (size_t)tiles_x;
        next.clear();
        for (int tx = 0; tx < tiles_x;) {
            if (!row[tx]) {
                ++tx;
                continue;
            }
            int tx1 = tx;
            while (tx1 < tiles_x && row[tx1]) ++tx1;
            int found = -1;
            for (int r : open)
                if (out_rects4[4 * r] == tx && out_rects4[4 * r + 2] == tx1) found = r;
            if (found >= 0) out_rects4[4 * found + 3] = ty + 1;
            else {
                if (count >= max_rects) return fail(FF_ERR_INVALID_ARG, "ff_adaptive_plan_host: max_rects %d is too small for the list", max_rects), -1;
                found = count++;
                out_rects4[4 * found] = tx;
                out_rects4[4 * found + 1] = ty;
                out_rects4[4 * found + 2] = tx1;
                out_rects4[4 * found + 3] = ty + 1;
            }
            next.push_back(found);
            tx = tx1;
        }
        open.swap(next);
    }
    return count;
}

int ff_render_adaptive(FfState* s, const FfCamera* camera, const FfRenderParams* params, const FfAdaptiveParams* ap, void* rgb8, int rgb8_on_device,
                       float* radiance, int radiance_on_device, uint16_t* passes_out, int passes_on_device, FfAdaptiveInfo* out_info)
{
    clear_error();
    const auto t0 = std::chrono::steady_clock::now();
    int st = check_adaptive_params(ap, "ff_render_adaptive");
    if (st != FF_OK) return st;
    st = check_render_call(s, camera, params, "ff_render_adaptive");
    if (st != FF_OK) return st;
    FF_HIP(hipSetDevice(s->device));
    hipStream_t stream = s->stream;
    const int W = params->width, H = params->height;
    const size_t px = (size_t)W * (size_t)H, plane = px * 3;
    const TileGrid grid = make_tile_grid(W, H, ap->tile);
    const size_t tiles = tile_count(grid);
    FfState::Adaptive& ad = s->adaptive;
    ad.valid = false; // (a call that fails on its way leaves no results)

    // the buffers: the two sums and the pass's rectangle, the per-tile arrays, the outputs' places
    st = ensure_bytes((void**)&ad.d_planes, &ad.planes_bytes, 3 * plane * sizeof(float) + 16);
    if (st != FF_OK) return st;
    float* d_sum = ad.d_planes;
    float* d_even = d_sum + plane;
    float* d_work = d_even + plane;
    TileBuffers tb;
    st = tile_buffers(s, tiles, &tb);
    if (st != FF_OK) return st;
    RenderOutputs out(s, px, rgb8, rgb8_on_device, radiance, radiance_on_device);
    if (out.status != FF_OK) return out.status;
    uint16_t* passes_dev = passes_out;
    if (passes_out && !passes_on_device) {
        st = ensure_bytes(&ad.d_stage, &ad.stage_bytes, px * sizeof(uint16_t) + 16);
        if (st != FF_OK) return st;
        passes_dev = (uint16_t*)ad.d_stage;
    }

    std::vector<uint8_t> active(tiles, 1);
    std::vector<uint16_t> tile_passes(tiles, 0);
    std::vector<float> tile_error(tiles, 0.f);
    std::vector<int32_t> rects(4 * tiles); // (no list is longer than the number of tiles)
    std::vector<uint32_t> list(tiles);
    const bool guard = (ap->flags & FF_ADAPTIVE_GUARD_NEIGHBOURS) != 0;
    FfAdaptiveInfo info = {};
    info.tiles = (int32_t)tiles;
    int left = (int)tiles;
    for (int k = 0; k < ap->max_passes && left > 0; ++k) {
        const int count = ff_adaptive_plan_host(grid.tiles_x, grid.tiles_y, active.data(), rects.data(), (int)tiles);
        if (count < 0) return FF_ERR_INVALID_ARG;
        FfRenderParams p = *params;
        p.seed = params->seed + (uint64_t)k;
        for (int r = 0; r < count; ++r) {
            const int x0 = rects[4 * r] * grid.k, y0 = rects[4 * r + 1] * grid.k;
            const int x1 = std::min(W, rects[4 * r + 2] * grid.k), y1 = std::min(H, rects[4 * r + 3] * grid.k);
            const int w = x1 - x0, h = y1 - y0;
            st = render_enqueue(s, camera, &p, h, 0, 1, h, nullptr, d_work, x0, y0, w);
            if (st != FF_OK) return st;
            FF_HIP(launch_adaptive_accumulate(d_sum, d_even, d_work, W, x0, y0, w, h, k == 0 ? 1 : 0, (k & 1) ? 0 : 1, stream));
            st = render_finish(s);
            if (st != FF_OK) return st;
            info.samples += (uint64_t)w * (uint64_t)h * (uint64_t)params->spp;
        }
        info.rectangles += count;
        const int n = k + 1;
        for (size_t t = 0; t < tiles; ++t)
            if (active[t]) tile_passes[t] = (uint16_t)n;
        info.passes_run = n;
        if ((n & 1) || n < ap->min_passes) continue;
        // the check: E_t of the active tiles on the device, read back; the host decides
        int listed = 0;
        for (size_t t = 0; t < tiles; ++t)
            if (active[t]) list[listed++] = (uint32_t)t;
        FF_HIP(hipMemcpyAsync(tb.list, list.data(), (size_t)listed * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        FF_HIP(launch_adaptive_tile_error(make_adaptive_args(W, H, ap->tile, n), d_sum, d_even, tb.list, listed, tb.error, stream));
        FF_HIP(hipStreamSynchronize(stream));
        // (the kernel writes the listed tiles only and the call's first check lists them all: a stopped tile's entry stays what its
        // last check found)
        FF_HIP(hipMemcpy(tile_error.data(), tb.error, tiles * sizeof(float), hipMemcpyDeviceToHost));
        left = stop_converged_tiles(grid.tiles_x, grid.tiles_y, tile_error, ap->threshold, guard, active);
    }

    // resolve: the means, the 8-bit image and the pass counts
    FF_HIP(hipMemcpyAsync(tb.passes, tile_passes.data(), tiles * sizeof(uint16_t), hipMemcpyHostToDevice, stream));
    if (out.radiance || out.rgb8 || passes_dev) FF_HIP(launch_adaptive_resolve(grid, d_sum, tb.passes, out.radiance, out.rgb8, passes_dev, stream));
    FF_HIP(hipStreamSynchronize(stream));
    st = out.copy_back();
    if (st != FF_OK) return st;
    if (passes_out && !passes_on_device) FF_HIP(hipMemcpy(passes_out, passes_dev, px * sizeof(uint16_t), hipMemcpyDeviceToHost));

    for (size_t t = 0; t < tiles; ++t) {
        if (tile_passes[t] < ap->max_passes) ++info.tiles_stopped_early;
        if (tile_error[t] > info.max_tile_error) info.max_tile_error = tile_error[t];
    }
    if (out_info) *out_info = info;
    ad.width = W;
    ad.height = H;
    ad.tile = ap->tile;
    ad.tile_passes.swap(tile_passes);
    ad.tile_error.swap(tile_error);
    ad.valid = true;
    s->stats.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return FF_OK;
}

int ff_adaptive_state(FfState* s, float* sum, float* sum_even, uint16_t* tile_passes, float* tile_error, int on_device)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_adaptive_state: state is null");
    const FfState::Adaptive& ad = s->adaptive;
    if (!ad.valid) return fail(FF_ERR_INVALID_ARG, "ff_adaptive_state: no ff_render_adaptive call has completed on this state");
    FF_HIP(hipSetDevice(s->device));
    const size_t plane = (size_t)ad.width * (size_t)ad.height * 3, tiles = ad.tile_passes.size();
    const hipMemcpyKind from_device = on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, from_host = on_device ? hipMemcpyHostToDevice : hipMemcpyHostToHost;
    if (sum) FF_HIP(hipMemcpy(sum, ad.d_planes, plane * sizeof(float), from_device));
    if (sum_even) FF_HIP(hipMemcpy(sum_even, ad.d_planes + plane, plane * sizeof(float), from_device));
    if (tile_passes) FF_HIP(hipMemcpy(tile_passes, ad.tile_passes.data(), tiles * sizeof(uint16_t), from_host));
    if (tile_error) FF_HIP(hipMemcpy(tile_error, ad.tile_error.data(), tiles * sizeof(float), from_host));
    return FF_OK;
}

int ff_adaptive_tile_error(FfState* s, int width, int height, int tile, int n, const float* sum, const float* sum_even, int inputs_on_device, float* out_error)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_adaptive_tile_error: state is null");
    AdaptiveArgs a;
    const int st = check_tile_error(width, height, tile, n, sum, sum_even, out_error, &a, "ff_adaptive_tile_error");
    if (st != FF_OK) return st;
    FF_HIP(hipSetDevice(s->device));
    hipStream_t stream = s->stream;
    const size_t plane = (size_t)width * (size_t)height * 3, tiles = tile_count(a.grid);
    // the errors at the head of the staging buffer (the last call's per-tile arrays stay as they are); the inputs follow
    FfState::Adaptive& ad = s->adaptive;
    Staging stage(&ad.d_stage, &ad.stage_bytes, (tiles * sizeof(float) + 15) & ~(size_t)15);
    if (!inputs_on_device) {
        stage.in(&sum, sum, plane * sizeof(float));
        stage.in(&sum_even, sum_even, plane * sizeof(float));
    }
    const int staged = stage.commit(stream, "ff_adaptive_tile_error: staging the inputs failed");
    if (staged != FF_OK) return staged;
    float* d_error = (float*)ad.d_stage;
    FF_HIP(launch_adaptive_tile_error(a, sum, sum_even, nullptr, (int)tiles, d_error, stream));
    FF_HIP(hipStreamSynchronize(stream));
    FF_HIP(hipMemcpy(out_error, d_error, tiles * sizeof(float), hipMemcpyDeviceToHost));
    return stage.finish();
}

int ff_adaptive_tile_error_host(int width, int height, int tile, int n, const float* sum, const float* sum_even, float* out_error)
{
    clear_error();
    AdaptiveArgs a;
    const int st = check_tile_error(width, height, tile, n, sum, sum_even, out_error, &a, "ff_adaptive_tile_error_host");
    if (st != FF_OK) return st;
    float v[kAdaptiveLanes];
    for (int ty = 0; ty < a.grid.tiles_y; ++ty)
        for (int tx = 0; tx < a.grid.tiles_x; ++tx) {
            for (int lane = 0; lane < kAdaptiveLanes; ++lane) v[lane] = adaptive_lane_sum(a, tx, ty, lane, sum, sum_even);
            out_error[(size_t)ty * (size_t)a.grid.tiles_x + (size_t)tx] = adaptive_tile_scale(a, adaptive_tree(v), adaptive_tile_pixels(a.grid, tx, ty));
        }
    return FF_OK;
}

} // extern "C"
