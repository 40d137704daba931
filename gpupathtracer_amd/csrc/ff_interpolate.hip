// ff_interpolate.hip — the kernels behind ff_interpolate: an in-between frame from two rendered neighbours.  A translation unit of
// its own beside the other image kernels and the trace kernels, which it does not touch.  The operator
// is in include/firefly/ff_api.h and, as code, in ff_interpolate.h, which the host twin ff_interpolate_host compiles too.
//
//   interpolate_gather_kernel   one pixel per lane, a wave on 64 consecutive pixels of a row (256 x 1 workgroups).  Steps 1 to 3: the
//                               two lookups, at most 2 x 4 taps, the blend; one 16-byte store of {rgb, state} per pixel.  A backward
//                               gather: no scatter, no atomics.
//   interpolate_fill_kernel     one workgroup of 256 threads per tile of 32 x 8 pixels.  A thread loads its own work pixel; one
//                               __syncthreads_or says whether the tile has a hole.  Without one, every thread stores its pixel and the
//                               workgroup is done.  With one, the tile and its apron of fill_radius pixels all round - {rgb, state}
//                               as one 16-byte cell and {geometry, bxdf} of the mid G-buffer as one 8-byte cell, dynamic LDS of
//                               (32 + 2 r) (8 + 2 r) cells of each - are staged, and the threads on a hole walk their window in LDS.
//                               A cell outside the image carries the hole mark and so is never a donor.  The five counts go through
//                               wave ballots and five LDS counters into at most five integer atomics per workgroup: order-free.
#include "ff_interpolate.h"

namespace ff {
namespace {

constexpr int kTileW = 32, kTileH = 8, kThreads = kTileW * kTileH;

__global__ __launch_bounds__(kThreads) void interpolate_gather_kernel(const InterpArgs a, float4* __restrict__ work)
{
    const int x = blockIdx.x * kThreads + threadIdx.x, y = blockIdx.y;
    if (x >= a.width) return;
    work[(size_t)y * (size_t)a.width + (size_t)x] = interp_gather(a, x, y);
}

__global__ __launch_bounds__(kThreads) void interpolate_fill_kernel(const InterpArgs a, const float4* __restrict__ work, unsigned char* __restrict__ rgb8,
                                                                    float* __restrict__ radiance_out, uint32_t* __restrict__ counts)
{
    extern __shared__ float4 s_dyn[];
    __shared__ uint32_t s_count[5];
    const int r = a.fill_radius;
    const int cw = kTileW + 2 * r, ch = kTileH + 2 * r;
    float4* s_cell = s_dyn;                                   // cw * ch cells {rgb, state}
    int2* s_kind = reinterpret_cast<int2*>(s_dyn + cw * ch);  // cw * ch cells {geometry, bxdf}
    const int tx = threadIdx.x & (kTileW - 1), ty = threadIdx.x / kTileW;
    const int x = blockIdx.x * kTileW + tx, y = blockIdx.y * kTileH + ty;
    const bool inside = x < a.width && y < a.height;
    const size_t p = (size_t)y * (size_t)a.width + (size_t)x;
    if (threadIdx.x < 5) s_count[threadIdx.x] = 0u;
    float4 own = make_float4(0.f, 0.f, 0.f, kInterpHole);
    if (inside) own = work[p];
    const bool hole = inside && own.w == kInterpHole;
    const int any_hole = __syncthreads_or(hole ? 1 : 0); // (also orders the zeroing of s_count)

    float v[3] = { own.x, own.y, own.z };
    int state = (int)own.w;
    if (any_hole) {
        // the tile with its apron; cell (0, 0) is pixel (x0, y0)
        const int x0 = blockIdx.x * kTileW - r, y0 = blockIdx.y * kTileH - r;
        for (int i = threadIdx.x; i < cw * ch; i += kThreads) {
            const int cy = i / cw, cx = i - cy * cw;
            const int qx = x0 + cx, qy = y0 + cy;
            float4 c = make_float4(0.f, 0.f, 0.f, kInterpHole);
            int2 kd = make_int2(0, 0);
            if (qx >= 0 && qy >= 0 && qx < a.width && qy < a.height) {
                const size_t q = (size_t)qy * (size_t)a.width + (size_t)qx;
                c = work[q];
                kd = make_int2(a.ids[3 * q], a.ids[3 * q + 2]);
            }
            s_cell[i] = c;
            s_kind[i] = kd;
        }
        __syncthreads();
        if (hole) {
            const int centre = (ty + r) * cw + (tx + r);
            const int2 mine = s_kind[centre];
            UpscaleMean m;
            for (int dy = -r; dy <= r; ++dy)
                for (int dx = -r; dx <= r; ++dx) {
                    const int i = centre + dy * cw + dx;
                    const float4 c = s_cell[i];
                    if (c.w == kInterpHole) continue; // (a hole, p itself among them, or outside the image)
                    const int2 kd = s_kind[i];
                    if (kd.x != mine.x || kd.y != mine.y) continue;
                    m.add(interp_fill_weight(dx, dy), c.x, c.y, c.z);
                }
            if (m.n > 0) {
                m.get(v);
                state = kInterpFilled;
            } else {
                interp_fallback(a, p, v);
                state = kInterpFallback;
            }
        }
    }
    if (inside) store_rgb(p, v, rgb8, radiance_out);

    // the counts: a ballot per state and wave, the workgroup's sums in LDS, then at most five atomics
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        const unsigned long long mask = __ballot(inside && state == c);
        if (lane == 0 && mask) atomicAdd(&s_count[c], (uint32_t)__popcll(mask));
    }
    __syncthreads();
    if (threadIdx.x < 5 && s_count[threadIdx.x]) atomicAdd(&counts[threadIdx.x], s_count[threadIdx.x]);
}

} // namespace

hipError_t launch_interpolate(const InterpArgs& a, float4* work, unsigned char* rgb8, float* radiance_out, uint32_t* counts, hipStream_t stream)
{
    if (a.width <= 0 || a.height <= 0) return hipSuccess;
    const dim3 ggrid((unsigned)((a.width + kThreads - 1) / kThreads), (unsigned)a.height);
    hipLaunchKernelGGL(interpolate_gather_kernel, ggrid, dim3(kThreads), 0, stream, a, work);
    const int cw = kTileW + 2 * a.fill_radius, ch = kTileH + 2 * a.fill_radius;
    const size_t lds = (size_t)cw * (size_t)ch * (sizeof(float4) + sizeof(int2));
    const dim3 fgrid((unsigned)((a.width + kTileW - 1) / kTileW), (unsigned)((a.height + kTileH - 1) / kTileH));
    hipLaunchKernelGGL(interpolate_fill_kernel, fgrid, dim3(kThreads), lds, stream, a, work, rgb8, radiance_out, counts);
    return hipGetLastError();
}

} // namespace ff
