// ff_despeckle_api.cpp — host side of ff_despeckle (include/firefly/ff_api.h): the argument checks, its use of the state's image work
// buffer (the partial counts of clamped pixels, then the staging of host buffers through ff_image.h's helpers), the one launch (kernel
// in ff_despeckle.hip) and the loops of the host-only twin ff_despeckle_host over ff_despeckle.h's per-pixel functions.  A pure
// image operation: no scene, no history, nothing kept in the state.
#include <cmath>
#include <vector>

#include <hip/hip_runtime.h>

#include "ff_despeckle.h"
#include "ff_state.h"

using namespace ff;

namespace {

// the partial counts at the head of the work buffer; the staging follows from here
constexpr size_t kCountBytes = (size_t)kDespeckleSlots * kDespeckleSlotStride * sizeof(uint32_t);

// What both entry points check, in this order: the parameter block, the size, the parameters, the inputs, the outputs' places.
// Fills the kernel arguments.
int check_despeckle(int width, int height, const FfDespeckleParams* p, const float* radiance_in, const float* albedo, const int32_t* ids, const void* rgb8,
                    const float* radiance_out, DespeckleArgs* a, const char* who)
{
    if (!p) return fail(FF_ERR_INVALID_ARG, "%s: params are null", who);
    if (check_image_size(width, height, who) != FF_OK) return FF_ERR_INVALID_ARG;
    if (p->radius < 1 || p->radius > kDespeckleMaxRadius)
        return fail(FF_ERR_INVALID_ARG, "%s: radius must be 1 .. %d (got %d)", who, kDespeckleMaxRadius, p->radius);
    if (p->rank < 1 || p->rank > kDespeckleMaxRank) return fail(FF_ERR_INVALID_ARG, "%s: rank must be 1 .. %d (got %d)", who, kDespeckleMaxRank, p->rank);
    const int window = (2 * p->radius + 1) * (2 * p->radius + 1) - 1;
    if (p->min_neighbours < p->rank || p->min_neighbours > window)
        return fail(FF_ERR_INVALID_ARG, "%s: min_neighbours must be rank .. (2 radius + 1)^2 - 1 = %d .. %d (got %d)", who, p->rank, window, p->min_neighbours);
    if (!(p->threshold >= 1.f) || !std::isfinite(p->threshold))
        return fail(FF_ERR_INVALID_ARG, "%s: threshold must be >= 1 and finite (got %g)", who, (double)p->threshold);
    if (!(p->floor >= 0.f) || !std::isfinite(p->floor)) return fail(FF_ERR_INVALID_ARG, "%s: floor must be >= 0 and finite (got %g)", who, (double)p->floor);
    if (p->flags & ~(uint32_t)FF_DESPECKLE_DEMODULATE_ALBEDO) return fail(FF_ERR_INVALID_ARG, "%s: unknown flags 0x%x", who, p->flags);
    if (p->reserved != 0) return fail(FF_ERR_INVALID_ARG, "%s: reserved must be 0", who);
    const bool demodulate = (p->flags & FF_DESPECKLE_DEMODULATE_ALBEDO) != 0;
    if (!radiance_in) return fail(FF_ERR_INVALID_ARG, "%s: radiance_in is null", who);
    if (demodulate && !albedo) return fail(FF_ERR_INVALID_ARG, "%s: albedo is null under FF_DESPECKLE_DEMODULATE_ALBEDO", who);
    if (!ids) return fail(FF_ERR_INVALID_ARG, "%s: ids is null", who);
    const size_t px = (size_t)width * (size_t)height;
    // (an albedo that is not read may lie anywhere)
    const Span albedo_read = { demodulate ? albedo : nullptr, demodulate ? px * 12 : 0, "albedo" };
    if (check_outputs_disjoint(rgb8, radiance_out, px, { { radiance_in, px * 12, "radiance_in" }, albedo_read, { ids, px * 12, "ids" } }, who) != FF_OK)
        return FF_ERR_INVALID_ARG;
    a->width = width;
    a->height = height;
    a->radius = p->radius;
    a->rank = p->rank;
    a->min_neighbours = p->min_neighbours;
    a->threshold = p->threshold;
    a->floor = p->floor;
    a->demodulate = demodulate ? 1 : 0;
    return FF_OK;
}

// The twin's step 2 and 3 for every pixel, over the plane of step 1's cells.
template <int RANK>
uint32_t despeckle_rows(const DespeckleArgs& a, const std::vector<DespeckleCell>& cells, const float* radiance_in, const float* albedo, unsigned char* rgb8,
                        float* radiance_out)
{
    uint32_t clamped = 0;
    const int r = a.radius;
    for (int y = 0; y < a.height; ++y)
        for (int x = 0; x < a.width; ++x) {
            const size_t p = (size_t)y * (size_t)a.width + (size_t)x;
            const DespeckleCell X = cells[p];
            DespeckleTop<RANK> top;
            despeckle_begin(top);
            for (int qy = y - r; qy <= y + r; ++qy)
                for (int qx = x - r; qx <= x + r; ++qx) {
                    if ((qx == x && qy == y) || qx < 0 || qy < 0 || qx >= a.width || qy >= a.height) continue;
                    despeckle_take(top, X, cells[(size_t)qy * (size_t)a.width + (size_t)qx]);
                }
            float v[3];
            clamped += despeckle_clamp(a, X, top, radiance_in + 3 * p, albedo ? albedo + 3 * p : nullptr, v) ? 1u : 0u;
            store_rgb(p, v, rgb8, radiance_out);
        }
    return clamped;
}

} // namespace

extern "C" {

void ff_despeckle_params_init(FfDespeckleParams* p)
{
    if (!p) return;
    // 
    p->radius = 1;
    p->rank = 2;
    p->min_neighbours = 3;
    p->threshold = 2.f;
    p->floor = 0.f;
    p->flags = FF_DESPECKLE_DEMODULATE_ALBEDO;
    p->reserved = 0;
}

int ff_despeckle(FfState* s, int width, int height, const FfDespeckleParams* p, const float* radiance_in, const float* albedo, const int32_t* ids,
                 int inputs_on_device, void* rgb8, int rgb8_on_device, float* radiance_out, int radiance_out_on_device, uint32_t* out_clamped)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_despeckle: state is null");
    DespeckleArgs a;
    const int st = check_despeckle(width, height, p, radiance_in, albedo, ids, rgb8, radiance_out, &a, "ff_despeckle");
    if (st != FF_OK) return st;
    FF_HIP(hipSetDevice(s->device));
    hipStream_t stream = s->stream;
    const size_t px = (size_t)width * (size_t)height;
    if (!a.demodulate) albedo = nullptr;
    Staging stage(&s->d_img_work, &s->img_work_bytes, kCountBytes);
    if (!inputs_on_device) {
        stage.in(&radiance_in, radiance_in, px * 12);
        if (albedo) stage.in(&albedo, albedo, px * 12);
        stage.in(&ids, ids, px * 12);
    }
    StagedOutputs out(stage, px, rgb8, rgb8_on_device, radiance_out, radiance_out_on_device);
    const int staged = stage.commit(stream, "ff_despeckle: staging the inputs failed");
    if (staged != FF_OK) return staged;
    uint32_t* d_count = (uint32_t*)s->d_img_work;
    FF_HIP(hipMemsetAsync(d_count, 0, kCountBytes, stream));
    FF_HIP(launch_despeckle(a, radiance_in, albedo, ids, out.rgb8, out.radiance, d_count, stream));
    FF_HIP(hipStreamSynchronize(stream));
    if (out_clamped) {
        std::vector<uint32_t> slots(kCountBytes / sizeof(uint32_t));
        FF_HIP(hipMemcpy(slots.data(), d_count, kCountBytes, hipMemcpyDeviceToHost));
        uint32_t sum = 0;
        for (int i = 0; i < kDespeckleSlots; ++i) sum += slots[(size_t)i * kDespeckleSlotStride];
        *out_clamped = sum;
    }
    return stage.finish();
}

int ff_despeckle_host(int width, int height, const FfDespeckleParams* p, const float* radiance_in, const float* albedo, const int32_t* ids,
                      unsigned char* rgb8, float* radiance_out, uint32_t* out_clamped)
{
    clear_error();
    DespeckleArgs a;
    const int st = check_despeckle(width, height, p, radiance_in, albedo, ids, rgb8, radiance_out, &a, "ff_despeckle_host");
    if (st != FF_OK) return st;
    const size_t px = (size_t)width * (size_t)height;
    if (!a.demodulate) albedo = nullptr;
    std::vector<DespeckleCell> cells(px);
    for (size_t i = 0; i < px; ++i) cells[i] = despeckle_measure(radiance_in + 3 * i, albedo ? albedo + 3 * i : nullptr, ids + 3 * i);
    uint32_t clamped = 0;
    switch (a.rank) {
    case 1: clamped = despeckle_rows<1>(a, cells, radiance_in, albedo, rgb8, radiance_out); break;
    case 2: clamped = despeckle_rows<2>(a, cells, radiance_in, albedo, rgb8, radiance_out); break;
    case 3: clamped = despeckle_rows<3>(a, cells, radiance_in, albedo, rgb8, radiance_out); break;
    default: clamped = despeckle_rows<4>(a, cells, radiance_in, albedo, rgb8, radiance_out); break;
    }
    if (out_clamped) *out_clamped = clamped;
    return FF_OK;
}

} // extern "C"
