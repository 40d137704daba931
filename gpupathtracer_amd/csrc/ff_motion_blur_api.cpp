// ff_motion_blur_api.cpp — host side of ff_motion_blur (include/firefly/ff_api.h): the argument checks and the entry points.  The use
// of the state's image work buffer, the staging of host buffers, the three launches (kernels in ff_motion_blur.hip) and the loops of
// the host-only twin ff_motion_blur_host are ff_tile_filter.h's, over ff_motion_blur.h's per-pixel functions.  A pure image
// operation: no scene, no history, nothing kept in the state.
#include <cmath>

#include <hip/hip_runtime.h>

#include "ff_motion_blur.h"
#include "ff_state.h"

using namespace ff;

namespace {

// What both entry points check, in this order: the parameter block, the size, the parameters, the inputs, the outputs' places.
// Fills the kernel arguments.
int check_motion_blur(int width, int height, const FfMotionBlurParams* p, const float* radiance_in, const float* motion, const float* depth, const void* rgb8,
                      const float* radiance_out, MotionBlurArgs* a, const char* who)
{
    if (!p) return fail(FF_ERR_INVALID_ARG, "%s: params are null", who);
    if (check_image_size(width, height, who) != FF_OK) return FF_ERR_INVALID_ARG;
    if (!(p->shutter >= 0.f && p->shutter <= 4.f)) return fail(FF_ERR_INVALID_ARG, "%s: shutter must be in 0 .. 4 (got %g)", who, (double)p->shutter);
    if (p->max_radius < 1 || p->max_radius > 64) return fail(FF_ERR_INVALID_ARG, "%s: max_radius must be 1 .. 64 (got %d)", who, p->max_radius);
    if (p->samples < 1 || p->samples > 64) return fail(FF_ERR_INVALID_ARG, "%s: samples must be 1 .. 64 (got %d)", who, p->samples);
    if (!(p->depth_extent > 0.f) || !std::isfinite(p->depth_extent))
        return fail(FF_ERR_INVALID_ARG, "%s: depth_extent must be positive and finite (got %g)", who, (double)p->depth_extent);
    if (p->flags != 0) return fail(FF_ERR_INVALID_ARG, "%s: unknown flags 0x%x", who, p->flags);
    if (p->reserved != 0) return fail(FF_ERR_INVALID_ARG, "%s: reserved must be 0", who);
    if (!radiance_in) return fail(FF_ERR_INVALID_ARG, "%s: radiance_in is null", who);
    if (!motion) return fail(FF_ERR_INVALID_ARG, "%s: motion is null", who);
    if (!depth) return fail(FF_ERR_INVALID_ARG, "%s: depth is null", who);
    const size_t px = (size_t)width * (size_t)height;
    if (check_outputs_disjoint(rgb8, radiance_out, px, { { radiance_in, px * 12, "radiance_in" }, { motion, px * 8, "motion" }, { depth, px * 4, "depth" } }, who) != FF_OK)
        return FF_ERR_INVALID_ARG;
    a->grid = make_tile_grid(width, height, p->max_radius);
    a->samples = p->samples;
    a->half_shutter = 0.5f * p->shutter;
    a->depth_extent = p->depth_extent;
    return FF_OK;
}

} // namespace

extern "C" {

void ff_motion_blur_params_init(FfMotionBlurParams* p)
{
    if (!p) return;
    // 
    p->shutter = 0.5f;
    p->max_radius = 16;
    p->samples = 15;
    p->depth_extent = 0.1f;
    p->flags = 0;
    p->reserved = 0;
}

int ff_motion_blur(FfState* s, int width, int height, const FfMotionBlurParams* p, const float* radiance_in, const float* motion, const float* depth,
                   int inputs_on_device, void* rgb8, int rgb8_on_device, float* radiance_out, int radiance_out_on_device)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_motion_blur: state is null");
    MotionBlurArgs a;
    const int st = check_motion_blur(width, height, p, radiance_in, motion, depth, rgb8, radiance_out, &a, "ff_motion_blur");
    if (st != FF_OK) return st;
    return tile_filter_device<MotionBlurFilter>(s, a, radiance_in, motion, depth, inputs_on_device, rgb8, rgb8_on_device, radiance_out, radiance_out_on_device,
                                                "ff_motion_blur");
}

int ff_motion_blur_host(int width, int height, const FfMotionBlurParams* p, const float* radiance_in, const float* motion, const float* depth,
                        unsigned char* rgb8, float* radiance_out)
{
    clear_error();
    MotionBlurArgs a;
    const int st = check_motion_blur(width, height, p, radiance_in, motion, depth, rgb8, radiance_out, &a, "ff_motion_blur_host");
    if (st != FF_OK) return st;
    tile_filter_host<MotionBlurFilter>(a, radiance_in, motion, depth, rgb8, radiance_out);
    return FF_OK;
}

} // extern "C"
