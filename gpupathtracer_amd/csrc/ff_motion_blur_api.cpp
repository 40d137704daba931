// ff_motion_blur_api.cpp — host side of ff_motion_blur (include/firefly/ff_api.h): the argument checks, the work buffer and the staging
// of host buffers, the three launches (kernels in ff_motion_blur.hip), and the host-only twin ff_motion_blur_host, which runs
// ff_motion_blur.h's per-pixel functions in loops.  A pure image operation: no scene, no history, nothing kept in the state but the
// work buffer.
#include <cmath>
#include <vector>

#include <hip/hip_runtime.h>

#include "ff_motion_blur.h"
#include "ff_state.h"

using namespace ff;

namespace {

struct Span {
    const void* ptr;
    size_t bytes;
    const char* name;
};

bool overlaps(const Span& a, const Span& b)
{
    const char* p = (const char*)a.ptr;
    const char* q = (const char*)b.ptr;
    return p < q + b.bytes && q < p + a.bytes;
}

// What both entry points check, in this order: the parameter block, the size, the parameters, the inputs, the outputs' places.
// Fills the kernel arguments.
int check_motion_blur(int width, int height, const FfMotionBlurParams* p, const float* radiance_in, const float* motion, const float* depth, const void* rgb8,
                      const float* radiance_out, MotionBlurArgs* a, const char* who)
{
    if (!p) return fail(FF_ERR_INVALID_ARG, "%s: params are null", who);
    if (width < 1 || height < 1 || width > 65535 || height > 65535) return fail(FF_ERR_INVALID_ARG, "%s: image size %dx%d is invalid", who, width, height);
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
    // the gather reads neighbours: no output may lie on an input, and the two outputs are written by different lanes
    const size_t px = (size_t)width * (size_t)height;
    const Span in[3] = { { radiance_in, px * 12, "radiance_in" }, { motion, px * 8, "motion" }, { depth, px * 4, "depth" } };
    const Span out[2] = { { rgb8, px * 3, "rgb8" }, { radiance_out, px * 12, "radiance_out" } };
    for (const Span& o : out)
        for (const Span& i : in)
            if (o.ptr && overlaps(o, i)) return fail(FF_ERR_INVALID_ARG, "%s: %s overlaps %s", who, o.name, i.name);
    if (rgb8 && radiance_out && overlaps(out[0], out[1])) return fail(FF_ERR_INVALID_ARG, "%s: rgb8 overlaps radiance_out", who);
    a->width = width;
    a->height = height;
    a->k = p->max_radius;
    a->samples = p->samples;
    a->tiles_x = (width + a->k - 1) / a->k;
    a->tiles_y = (height + a->k - 1) / a->k;
    a->half_shutter = 0.5f * p->shutter;
    a->depth_extent = p->depth_extent;
    return FF_OK;
}

} // namespace

namespace ff {

void motion_blur_release(FfState* s)
{
    if (s->d_mblur_work) (void)hipFree(s->d_mblur_work);
    s->d_mblur_work = nullptr;
    s->mblur_work_bytes = 0;
}

} // namespace ff

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
    int st = check_motion_blur(width, height, p, radiance_in, motion, depth, rgb8, radiance_out, &a, "ff_motion_blur");
    if (st != FF_OK) return st;
    FF_HIP(hipSetDevice(s->device));
    hipStream_t stream = s->stream;
    const size_t px = (size_t)width * (size_t)height, tiles = (size_t)a.tiles_x * (size_t)a.tiles_y;
    // the work buffer: the packed plane, T and N, then the staging of host buffers
    const size_t plane_bytes = px * sizeof(float4), tile_bytes = tiles * sizeof(float4);
    unsigned char* d_rgb8 = (unsigned char*)rgb8;
    float* d_out = radiance_out;
    Staging stage(&s->d_mblur_work, &s->mblur_work_bytes, plane_bytes + 2 * tile_bytes);
    if (!inputs_on_device) {
        stage.in(&radiance_in, radiance_in, px * 12);
        stage.in(&motion, motion, px * 8);
        stage.in(&depth, depth, px * 4);
    }
    if (rgb8 && !rgb8_on_device) stage.out(&d_rgb8, rgb8, px * 3);
    if (radiance_out && !radiance_out_on_device) stage.out(&d_out, radiance_out, px * 12);
    st = stage.commit(stream, "ff_motion_blur: staging the inputs failed");
    if (st != FF_OK) return st;
    float4* plane = (float4*)s->d_mblur_work;
    float4* tile_max = plane + px;
    float4* neighbour_max = tile_max + tiles;
    FF_HIP(launch_mblur_pack_tile_max(a, motion, depth, plane, tile_max, stream));
    FF_HIP(launch_mblur_neighbour_max(a, tile_max, neighbour_max, stream));
    if (d_rgb8 || d_out) FF_HIP(launch_mblur_gather(a, plane, neighbour_max, radiance_in, d_rgb8, d_out, stream));
    FF_HIP(hipStreamSynchronize(stream));
    return stage.finish();
}

int ff_motion_blur_host(int width, int height, const FfMotionBlurParams* p, const float* radiance_in, const float* motion, const float* depth,
                        unsigned char* rgb8, float* radiance_out)
{
    clear_error();
    MotionBlurArgs a;
    const int st = check_motion_blur(width, height, p, radiance_in, motion, depth, rgb8, radiance_out, &a, "ff_motion_blur_host");
    if (st != FF_OK) return st;
    const size_t px = (size_t)width * (size_t)height, tiles = (size_t)a.tiles_x * (size_t)a.tiles_y;
    std::vector<float4> plane(px), tile_max(tiles), neighbour_max(tiles);
    // steps 1 and 2: a tile's pixels in row-major order, a later one replaces the best only when its key is larger
    for (int ty = 0; ty < a.tiles_y; ++ty)
        for (int tx = 0; tx < a.tiles_x; ++tx) {
            const int x0 = tx * a.k, y0 = ty * a.k;
            const int tw = std::min(a.k, width - x0), th = std::min(a.k, height - y0);
            unsigned long long best = 0;
            float4 best_p = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int i = 0; i < tw * th; ++i) {
                const size_t q = (size_t)(y0 + i / tw) * (size_t)width + (size_t)(x0 + i % tw);
                const float4 v = mblur_pack(a, motion[2 * q], motion[2 * q + 1], depth[q]);
                plane[q] = v;
                const unsigned long long key = mblur_key(v.x, v.y, (unsigned)i);
                if (key > best) {
                    best = key;
                    best_p = v;
                }
            }
            tile_max[(size_t)ty * (size_t)a.tiles_x + (size_t)tx] = make_float4(best_p.x, best_p.y, best_p.z, 0.f);
        }
    for (int ty = 0; ty < a.tiles_y; ++ty)
        for (int tx = 0; tx < a.tiles_x; ++tx) neighbour_max[(size_t)ty * (size_t)a.tiles_x + (size_t)tx] = mblur_neighbour_max(a, tile_max.data(), tx, ty);
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t i = (size_t)y * (size_t)width + (size_t)x;
            float v[3];
            mblur_gather(a, x, y, plane.data(), radiance_in, neighbour_max[(size_t)(y / a.k) * (size_t)a.tiles_x + (size_t)(x / a.k)], v);
            if (radiance_out) { radiance_out[3 * i] = v[0]; radiance_out[3 * i + 1] = v[1]; radiance_out[3 * i + 2] = v[2]; }
            if (rgb8) { rgb8[3 * i] = mblur_u8(v[0]); rgb8[3 * i + 1] = mblur_u8(v[1]); rgb8[3 * i + 2] = mblur_u8(v[2]); }
        }
    return FF_OK;
}

} // extern "C"
