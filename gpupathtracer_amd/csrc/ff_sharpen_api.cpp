// ff_sharpen_api.cpp — host side of ff_sharpen (include/firefly/ff_api.h): the argument checks, the staging of host buffers in
// the state's image work buffer (ff_image.h's helpers), the one launch (kernel in ff_sharpen.hip) and the loops of the host-only
// twin ff_sharpen_host over ff_sharpen.h's per-pixel functions.  A pure image operation: no scene, no G-buffer, no history,
// nothing kept in the state.
#include <cmath>
#include <vector>

#include <hip/hip_runtime.h>

#include "ff_sharpen.h"
#include "ff_state.h"

using namespace ff;

namespace {

// What both entry points check, in this order: the parameter block, the size, the parameters, the input, the outputs' places.
// Fills the kernel arguments.
int check_sharpen(int width, int height, const FfSharpenParams* p, const float* radiance_in, const void* rgb8, const float* radiance_out, SharpenArgs* a,
                  const char* who)
{
    if (!p) return fail(FF_ERR_INVALID_ARG, "%s: params are null", who);
    if (check_image_size(width, height, who) != FF_OK) return FF_ERR_INVALID_ARG;
    if (!(p->strength >= 0.f && p->strength <= 1.f)) // (false for NaN)
        return fail(FF_ERR_INVALID_ARG, "%s: strength must be 0 .. 1 and finite (got %g)", who, (double)p->strength);
    if (p->flags & ~(uint32_t)FF_SHARPEN_NOISE_AWARE) return fail(FF_ERR_INVALID_ARG, "%s: unknown flags 0x%x", who, p->flags);
    if (p->reserved != 0) return fail(FF_ERR_INVALID_ARG, "%s: reserved must be 0", who);
    if (!radiance_in) return fail(FF_ERR_INVALID_ARG, "%s: radiance_in is null", who);
    const size_t px = (size_t)width * (size_t)height;
    if (check_outputs_disjoint(rgb8, radiance_out, px, { { radiance_in, px * 12, "radiance_in" } }, who) != FF_OK) return FF_ERR_INVALID_ARG;
    a->width = width;
    a->height = height;
    a->strength = p->strength;
    a->noise_aware = (p->flags & FF_SHARPEN_NOISE_AWARE) ? 1 : 0;
    return FF_OK;
}

// The twin's steps 2 to 6 for every pixel, over the plane of step 1's cells.
template <bool NOISE>
void sharpen_rows(const SharpenArgs& a, const std::vector<SharpenCell>& cells, const float* radiance_in, unsigned char* rgb8, float* radiance_out)
{
    SharpenCell outside;
    outside.t[0] = outside.t[1] = outside.t[2] = 0.f;
    outside.l = kSharpenOutside;
    const size_t w = (size_t)a.width;
    for (int y = 0; y < a.height; ++y)
        for (int x = 0; x < a.width; ++x) {
            const size_t p = (size_t)y * w + (size_t)x;
            const SharpenCell& B = y > 0 ? cells[p - w] : outside;
            const SharpenCell& D = x > 0 ? cells[p - 1] : outside;
            const SharpenCell& F = x + 1 < a.width ? cells[p + 1] : outside;
            const SharpenCell& H = y + 1 < a.height ? cells[p + w] : outside;
            float v[3];
            sharpen_pixel<NOISE>(a.strength, cells[p], B, D, F, H, radiance_in + 3 * p, v);
            store_rgb(p, v, rgb8, radiance_out);
        }
}

} // namespace

extern "C" {

void ff_sharpen_params_init(FfSharpenParams* p)
{
    if (!p) return;
    // 
    p->strength = 0.5f;
    p->flags = FF_SHARPEN_NOISE_AWARE;
    p->reserved = 0;
}

int ff_sharpen(FfState* s, int width, int height, const FfSharpenParams* p, const float* radiance_in, int input_on_device, void* rgb8, int rgb8_on_device,
               float* radiance_out, int radiance_out_on_device)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_sharpen: state is null");
    SharpenArgs a;
    const int st = check_sharpen(width, height, p, radiance_in, rgb8, radiance_out, &a, "ff_sharpen");
    if (st != FF_OK) return st;
    FF_HIP(hipSetDevice(s->device));
    hipStream_t stream = s->stream;
    const size_t px = (size_t)width * (size_t)height;
    Staging stage(&s->d_img_work, &s->img_work_bytes);
    if (!input_on_device) stage.in(&radiance_in, radiance_in, px * 12);
    StagedOutputs out(stage, px, rgb8, rgb8_on_device, radiance_out, radiance_out_on_device);
    const int staged = stage.commit(stream, "ff_sharpen: staging the input failed");
    if (staged != FF_OK) return staged;
    FF_HIP(launch_sharpen(a, radiance_in, out.rgb8, out.radiance, stream));
    FF_HIP(hipStreamSynchronize(stream));
    return stage.finish();
}

int ff_sharpen_host(int width, int height, const FfSharpenParams* p, const float* radiance_in, unsigned char* rgb8, float* radiance_out)
{
    clear_error();
    SharpenArgs a;
    const int st = check_sharpen(width, height, p, radiance_in, rgb8, radiance_out, &a, "ff_sharpen_host");
    if (st != FF_OK) return st;
    const size_t px = (size_t)width * (size_t)height;
    std::vector<SharpenCell> cells(px);
    for (size_t i = 0; i < px; ++i) cells[i] = sharpen_compress(radiance_in + 3 * i);
    if (a.noise_aware)
        sharpen_rows<true>(a, cells, radiance_in, rgb8, radiance_out);
    else
        sharpen_rows<false>(a, cells, radiance_in, rgb8, radiance_out);
    return FF_OK;
}

} // extern "C"
