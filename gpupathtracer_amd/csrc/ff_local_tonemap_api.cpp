// ff_local_tonemap_api.cpp — host side of ff_local_tonemap (include/firefly/ff_api.h): the argument checks, its use of the state's
// image work buffer (the two grids, then the staging of host buffers through ff_image.h's helpers), the launches (kernels in
// ff_local_tonemap.hip) and the loops of the host-only twins ff_local_tonemap_host and ff_local_tonemap_grid_host over
// ff_local_tonemap.h's functions.  A pure image operation: no scene, no G-buffer, no history, nothing kept in the state.
#include <cmath>
#include <vector>

#include <hip/hip_runtime.h>

#include "ff_local_tonemap.h"
#include "ff_state.h"

using namespace ff;

namespace {

// What every entry point checks of the parameter block, the size and the input, in this order.  Fills the kernel arguments.
int check_ltm_params(int width, int height, const FfLocalTonemapParams* p, const float* radiance_in, LtmArgs* a, const char* who)
{
    if (!p) return fail(FF_ERR_INVALID_ARG, "%s: params are null", who);
    if (check_image_size(width, height, who) != FF_OK) return FF_ERR_INVALID_ARG;
    if (!(p->compression >= 0.f && p->compression <= 1.f)) // (false for NaN)
        return fail(FF_ERR_INVALID_ARG, "%s: compression must be 0 .. 1 and finite (got %g)", who, (double)p->compression);
    if (!(p->detail >= 0.f && p->detail <= 4.f)) return fail(FF_ERR_INVALID_ARG, "%s: detail must be 0 .. 4 and finite (got %g)", who, (double)p->detail);
    if (!(p->pivot >= kLtmFloor && p->pivot < 16777216.f))
        return fail(FF_ERR_INVALID_ARG, "%s: pivot must be finite and in [2^-16, 2^24) (got %g)", who, (double)p->pivot);
    int shift = 0;
    switch (p->cell) {
    case 8: shift = 3; break;
    case 16: shift = 4; break;
    case 32: shift = 5; break;
    case 64: shift = 6; break;
    default: return fail(FF_ERR_INVALID_ARG, "%s: cell must be 8, 16, 32 or 64 (got %d)", who, p->cell);
    }
    if (p->flags != 0) return fail(FF_ERR_INVALID_ARG, "%s: unknown flags 0x%x", who, p->flags);
    if (p->reserved[0] != 0 || p->reserved[1] != 0 || p->reserved[2] != 0) return fail(FF_ERR_INVALID_ARG, "%s: reserved must be 0", who);
    if (!radiance_in) return fail(FF_ERR_INVALID_ARG, "%s: radiance_in is null", who);
    a->width = width;
    a->height = height;
    a->cell = p->cell;
    a->shift = shift;
    a->gw = (width + p->cell - 1) >> shift;
    a->gh = (height + p->cell - 1) >> shift;
    a->inv_cell = 1.0f / (float)p->cell;
    a->cm1 = p->compression - 1.0f;
    a->dm1 = p->detail - 1.0f;
    a->pivot_log = ltm_lf(ltm_q16(p->pivot));
    a->identity = (p->compression == 1.0f && p->detail == 1.0f) ? 1 : 0;
    return FF_OK;
}

// ... and of the outputs' places: rgb8 off the input, radiance_out the input itself or off it, the two off each other.
int check_ltm(int width, int height, const FfLocalTonemapParams* p, const float* radiance_in, const void* rgb8, const float* radiance_out, LtmArgs* a,
              const char* who)
{
    const int st = check_ltm_params(width, height, p, radiance_in, a, who);
    if (st != FF_OK) return st;
    const size_t px = (size_t)width * (size_t)height;
    const Span in = { radiance_in, px * 12, "radiance_in" };
    // (in place: every pixel is read before it is written, and the grid is complete before any pixel is written)
    if (radiance_out == radiance_in) {
        if (rgb8 && overlaps({ rgb8, px * 3, "rgb8" }, in)) return fail(FF_ERR_INVALID_ARG, "%s: rgb8 overlaps radiance_in", who);
        return FF_OK;
    }
    return check_outputs_disjoint(rgb8, radiance_out, px, { in }, who);
}

// Steps 1 and 2 on the host: the grid of int32 cells.
void ltm_splat_host(const LtmArgs& a, const float* radiance_in, std::vector<LtmCellI>& grid)
{
    grid.assign(ltm_grid_cells(a), LtmCellI{ 0, 0 });
    for (int y = 0; y < a.height; ++y)
        for (int x = 0; x < a.width; ++x) {
            const float* c = radiance_in + 3 * ((size_t)y * (size_t)a.width + (size_t)x);
            const float l = ltm_luminance(c);
            if (!ltm_mapped(c, l)) continue;
            const int q10 = ltm_q10(ltm_q16(l));
            LtmCellI& cell = grid[((size_t)(y >> a.shift) * (size_t)a.gw + (size_t)(x >> a.shift)) * kLtmBins + ltm_bin(q10)];
            cell.n += 1;
            cell.S += q10;
        }
}

// Step 3 on the host, one axis: the cells `stride` apart are neighbours, `at` of `count` along the axis.
void ltm_blur_host(const LtmArgs& a, int axis, const std::vector<LtmCellF>& src, std::vector<LtmCellF>& dst)
{
    const size_t stride = axis == 0 ? (size_t)kLtmBins : (axis == 1 ? (size_t)a.gw * kLtmBins : (size_t)1);
    const LtmCellF zero = { 0.0f, 0.0f };
    size_t i = 0;
    for (int cy = 0; cy < a.gh; ++cy)
        for (int cx = 0; cx < a.gw; ++cx)
            for (int z = 0; z < kLtmBins; ++z, ++i) {
                const int at = axis == 0 ? cx : (axis == 1 ? cy : z);
                const int last = axis == 0 ? a.gw - 1 : (axis == 1 ? a.gh - 1 : kLtmBins - 1);
                const LtmCellF lo = at > 0 ? src[i - stride] : zero, hi = at < last ? src[i + stride] : zero;
                dst[i].n = ltm_blur3(lo.n, src[i].n, hi.n);
                dst[i].S = ltm_blur3(lo.S, src[i].S, hi.S);
            }
}

} // namespace

extern "C" {

void ff_local_tonemap_params_init(FfLocalTonemapParams* p)
{
    if (!p) return;
    // 
    p->compression = 0.5f;
    p->detail = 1.f;
    p->pivot = 0.18f;
    p->cell = 32;
    p->flags = 0;
    p->reserved[0] = p->reserved[1] = p->reserved[2] = 0;
}

int ff_local_tonemap(FfState* s, int width, int height, const FfLocalTonemapParams* p, const float* radiance_in, int input_on_device, void* rgb8,
                     int rgb8_on_device, float* radiance_out, int radiance_out_on_device)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_local_tonemap: state is null");
    LtmArgs a;
    const int st = check_ltm(width, height, p, radiance_in, rgb8, radiance_out, &a, "ff_local_tonemap");
    if (st != FF_OK) return st;
    FF_HIP(hipSetDevice(s->device));
    hipStream_t stream = s->stream;
    const size_t px = (size_t)width * (size_t)height;
    // the two grids at the head of the work buffer (none for a copy); the staging follows from a multiple of 16 bytes on
    const size_t grid_bytes = a.identity ? 0 : 2 * ltm_grid_cells(a) * sizeof(LtmCellF);
    Staging stage(&s->d_img_work, &s->img_work_bytes, (grid_bytes + 15) & ~(size_t)15);
    if (!input_on_device) stage.in(&radiance_in, radiance_in, px * 12);
    StagedOutputs out(stage, px, rgb8, rgb8_on_device, radiance_out, radiance_out_on_device);
    const int staged = stage.commit(stream, "ff_local_tonemap: staging the input failed");
    if (staged != FF_OK) return staged;
    FF_HIP(launch_local_tonemap(a, radiance_in, s->d_img_work, out.rgb8, out.radiance, stream));
    FF_HIP(hipStreamSynchronize(stream));
    return stage.finish();
}

int ff_local_tonemap_host(int width, int height, const FfLocalTonemapParams* p, const float* radiance_in, unsigned char* rgb8, float* radiance_out)
{
    clear_error();
    LtmArgs a;
    const int st = check_ltm(width, height, p, radiance_in, rgb8, radiance_out, &a, "ff_local_tonemap_host");
    if (st != FF_OK) return st;
    std::vector<LtmCellF> g0, g1;
    if (!a.identity) {
        std::vector<LtmCellI> raw;
        ltm_splat_host(a, radiance_in, raw);
        g0.resize(raw.size());
        g1.resize(raw.size());
        for (size_t i = 0; i < raw.size(); ++i) {
            g0[i].n = (float)raw[i].n;
            g0[i].S = (float)raw[i].S;
        }
        ltm_blur_host(a, 0, g0, g1);
        ltm_blur_host(a, 1, g1, g0);
        ltm_blur_host(a, 2, g0, g1);
    }
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t i = (size_t)y * (size_t)width + (size_t)x;
            const float rad[3] = { radiance_in[3 * i], radiance_in[3 * i + 1], radiance_in[3 * i + 2] };
            float v[3];
            ltm_pixel(a, g1.data(), x, y, rad, v);
            store_rgb(i, v, rgb8, radiance_out);
        }
    return FF_OK;
}

int ff_local_tonemap_grid_host(int width, int height, const FfLocalTonemapParams* p, const float* radiance_in, int32_t* out_n, int32_t* out_S)
{
    clear_error();
    LtmArgs a;
    const int st = check_ltm_params(width, height, p, radiance_in, &a, "ff_local_tonemap_grid_host");
    if (st != FF_OK) return st;
    if (!out_n) return fail(FF_ERR_INVALID_ARG, "ff_local_tonemap_grid_host: out_n is null");
    if (!out_S) return fail(FF_ERR_INVALID_ARG, "ff_local_tonemap_grid_host: out_S is null");
    std::vector<LtmCellI> raw;
    ltm_splat_host(a, radiance_in, raw);
    for (size_t i = 0; i < raw.size(); ++i) {
        out_n[i] = raw[i].n;
        out_S[i] = raw[i].S;
    }
    return FF_OK;
}

} // extern "C"
