// ff_upscale_api.cpp — host side of ff_upscale (include/firefly/ff_api.h): the argument checks, the staging of host buffers and the
// launch (kernel in ff_upscale.hip), and the host-only twin ff_upscale_host, which runs ff_upscale.h's per-pixel function in a loop.
// A pure image operation: no scene, no history, nothing kept in the state.
#include <cmath>

#include <hip/hip_runtime.h>

#include "ff_state.h"
#include "ff_upscale.h"

using namespace ff;

namespace {

// What both entry points check, in this order: the parameter block, the sizes, the parameters, the buffers.  Fills the kernel
// arguments' scalar half.
int check_upscale(const FfUpscaleParams* p, int lo_width, int lo_height, const float* radiance_lo, const float* position_lo, const float* normal_lo,
                  const float* albedo_lo, const int32_t* ids_lo, int width, int height, const float* position, const float* normal, const float* albedo,
                  const int32_t* ids, UpscaleArgs* a, const char* who)
{
    if (!p) return fail(FF_ERR_INVALID_ARG, "%s: params are null", who);
    if (lo_width < 1 || lo_height < 1) return fail(FF_ERR_INVALID_ARG, "%s: lo_width x lo_height %dx%d is invalid", who, lo_width, lo_height);
    if (width > 65535 || height > 65535) return fail(FF_ERR_INVALID_ARG, "%s: width x height %dx%d is invalid (at most 65535)", who, width, height);
    if (width < lo_width || (long long)width > 8ll * lo_width)
        return fail(FF_ERR_INVALID_ARG, "%s: width %d must be in lo_width .. 8 lo_width (lo_width %d)", who, width, lo_width);
    if (height < lo_height || (long long)height > 8ll * lo_height)
        return fail(FF_ERR_INVALID_ARG, "%s: height %d must be in lo_height .. 8 lo_height (lo_height %d)", who, height, lo_height);
    if (!(p->sigma_normal > 0.f) || !std::isfinite(p->sigma_normal))
        return fail(FF_ERR_INVALID_ARG, "%s: sigma_normal must be positive and finite (got %g)", who, (double)p->sigma_normal);
    if (!(p->sigma_plane > 0.f) || !std::isfinite(p->sigma_plane))
        return fail(FF_ERR_INVALID_ARG, "%s: sigma_plane must be positive and finite (got %g)", who, (double)p->sigma_plane);
    if (p->flags & ~(uint32_t)(FF_DENOISE_SAME_GEOMETRY | FF_DENOISE_DEMODULATE_ALBEDO)) return fail(FF_ERR_INVALID_ARG, "%s: unknown flags 0x%x", who, p->flags);
    if (!(p->lo_jitter[0] >= 0.f && p->lo_jitter[0] < 1.f && p->lo_jitter[1] >= 0.f && p->lo_jitter[1] < 1.f))
        return fail(FF_ERR_INVALID_ARG, "%s: lo_jitter must be in [0, 1) (got %g %g)", who, (double)p->lo_jitter[0], (double)p->lo_jitter[1]);
    if (!(p->hi_jitter[0] >= 0.f && p->hi_jitter[0] < 1.f && p->hi_jitter[1] >= 0.f && p->hi_jitter[1] < 1.f))
        return fail(FF_ERR_INVALID_ARG, "%s: hi_jitter must be in [0, 1) (got %g %g)", who, (double)p->hi_jitter[0], (double)p->hi_jitter[1]);
    if (p->reserved != 0) return fail(FF_ERR_INVALID_ARG, "%s: reserved must be 0", who);
    const int demod = (p->flags & FF_DENOISE_DEMODULATE_ALBEDO) ? 1 : 0;
    if (!radiance_lo) return fail(FF_ERR_INVALID_ARG, "%s: radiance_lo is null", who);
    if (!position_lo) return fail(FF_ERR_INVALID_ARG, "%s: position_lo is null", who);
    if (!normal_lo) return fail(FF_ERR_INVALID_ARG, "%s: normal_lo is null", who);
    if (!ids_lo) return fail(FF_ERR_INVALID_ARG, "%s: ids_lo is null", who);
    if (!position) return fail(FF_ERR_INVALID_ARG, "%s: position is null", who);
    if (!normal) return fail(FF_ERR_INVALID_ARG, "%s: normal is null", who);
    if (!ids) return fail(FF_ERR_INVALID_ARG, "%s: ids is null", who);
    if (demod && !albedo_lo) return fail(FF_ERR_INVALID_ARG, "%s: albedo_lo is null with FF_DENOISE_DEMODULATE_ALBEDO", who);
    if (demod && !albedo) return fail(FF_ERR_INVALID_ARG, "%s: albedo is null with FF_DENOISE_DEMODULATE_ALBEDO", who);
    a->lo_width = lo_width;
    a->lo_height = lo_height;
    a->width = width;
    a->height = height;
    a->sigma_normal = p->sigma_normal;
    a->sigma_plane2 = p->sigma_plane * p->sigma_plane;
    a->lo_jx = p->lo_jitter[0];
    a->lo_jy = p->lo_jitter[1];
    a->hi_jx = p->hi_jitter[0];
    a->hi_jy = p->hi_jitter[1];
    a->same_geometry = (p->flags & FF_DENOISE_SAME_GEOMETRY) ? 1 : 0;
    a->demodulate = demod;
    a->radiance_lo = radiance_lo;
    a->position_lo = position_lo;
    a->normal_lo = normal_lo;
    a->albedo_lo = demod ? albedo_lo : nullptr;
    a->ids_lo = ids_lo;
    a->position = position;
    a->normal = normal;
    a->albedo = demod ? albedo : nullptr;
    a->ids = ids;
    return FF_OK;
}

} // namespace

extern "C" {

void ff_upscale_params_init(FfUpscaleParams* p)
{
    if (!p) return;
    // (ff_denoise's edge-stopping sigmas: DESIGN.md section 8 row 14)
    p->sigma_normal = 0.1f;
    p->sigma_plane = 0.1f;
    p->flags = FF_DENOISE_SAME_GEOMETRY | FF_DENOISE_DEMODULATE_ALBEDO;
    p->lo_jitter[0] = p->lo_jitter[1] = 0.f;
    p->hi_jitter[0] = p->hi_jitter[1] = 0.f;
    p->reserved = 0;
}

int ff_upscale(FfState* s, const FfUpscaleParams* p, int lo_width, int lo_height, const float* radiance_lo, const float* position_lo,
               const float* normal_lo, const float* albedo_lo, const int32_t* ids_lo, int width, int height, const float* position, const float* normal,
               const float* albedo, const int32_t* ids, int inputs_on_device, void* rgb8, int rgb8_on_device, float* radiance_out,
               int radiance_out_on_device)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_upscale: state is null");
    UpscaleArgs a;
    int st = check_upscale(p, lo_width, lo_height, radiance_lo, position_lo, normal_lo, albedo_lo, ids_lo, width, height, position, normal, albedo, ids, &a,
                           "ff_upscale");
    if (st != FF_OK) return st;
    FF_HIP(hipSetDevice(s->device));
    const size_t lo_px = (size_t)lo_width * (size_t)lo_height, px = (size_t)width * (size_t)height;
    hipStream_t stream = s->stream;
    // host buffers are staged, as in ff_denoise: the inputs the call reads, the outputs it writes
    Staging stage(&s->d_img_work, &s->img_work_bytes);
    if (!inputs_on_device) {
        stage.in(&a.radiance_lo, radiance_lo, lo_px * 12);
        stage.in(&a.position_lo, position_lo, lo_px * 12);
        stage.in(&a.normal_lo, normal_lo, lo_px * 12);
        if (a.demodulate) stage.in(&a.albedo_lo, albedo_lo, lo_px * 12);
        stage.in(&a.ids_lo, ids_lo, lo_px * 12);
        stage.in(&a.position, position, px * 12);
        stage.in(&a.normal, normal, px * 12);
        if (a.demodulate) stage.in(&a.albedo, albedo, px * 12);
        stage.in(&a.ids, ids, px * 12);
    }
    StagedOutputs out(stage, px, rgb8, rgb8_on_device, radiance_out, radiance_out_on_device);
    st = stage.commit(stream, "ff_upscale: staging the inputs failed");
    if (st != FF_OK) return st;
    FF_HIP(launch_upscale(a, out.rgb8, out.radiance, stream));
    FF_HIP(hipStreamSynchronize(stream));
    return stage.finish();
}

int ff_upscale_host(const FfUpscaleParams* p, int lo_width, int lo_height, const float* radiance_lo, const float* position_lo, const float* normal_lo,
                    const float* albedo_lo, const int32_t* ids_lo, int width, int height, const float* position, const float* normal, const float* albedo,
                    const int32_t* ids, unsigned char* rgb8, float* radiance_out)
{
    clear_error();
    UpscaleArgs a;
    const int st = check_upscale(p, lo_width, lo_height, radiance_lo, position_lo, normal_lo, albedo_lo, ids_lo, width, height, position, normal, albedo, ids,
                                 &a, "ff_upscale_host");
    if (st != FF_OK) return st;
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t i = (size_t)y * (size_t)width + (size_t)x;
            float v[3];
            upscale_pixel(a, x, y, v);
            store_rgb(i, v, rgb8, radiance_out);
        }
    return FF_OK;
}

} // extern "C"
