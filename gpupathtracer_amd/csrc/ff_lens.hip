// ff_lens.hip — the kernel behind ff_lens: lens distortion, lateral chromatic aberration and vignetting of a radiance image as one
// gather.  A translation unit of its own beside the other image kernels and the trace kernels, which it does not touch (DESIGN.md
// section 8 row 26).  The operator is in include/firefly/ff_api.h and, as code, in ff_lens.h, which the host twin ff_lens_host
// compiles too.
//
//   lens_kernel<FILTER, PER_CHANNEL>   workgroups of 256 threads, each on one tile of 32 x 8 output pixels per pass, a wave on two
//                           rows of 32 (ff_sharpen's shape).  A workgroup copies the table - FF_LENS_KNOTS + 1 knots {e, gain},
//                           8200 bytes - into LDS once and then walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ... in
//                           row-major tile order, so that the workgroups in flight at one time work on neighbouring tiles and
//                           share their taps' lines in L2.  A thread reads its two knots with two 8-byte LDS reads (lanes of one
//                           row differ by a fraction of a cell: mostly one address, a broadcast) and its taps straight from
//                           global memory: neighbouring lanes read neighbouring texels.  No barrier after the table's.
//                           FILTER: bilinear, Catmull-Rom, Catmull-Rom with the anti-ring clamp; PER_CHANNEL: either chromatic
//                           aberration is nonzero and each channel has its own position and taps.  Six instantiations; the
//                           border mode is a uniform branch.
#include "ff_lens.h"

namespace ff {
namespace {

constexpr int kTileW = 32, kTileH = 8, kThreads = kTileW * kTileH;

template <int FILTER, bool PER_CHANNEL>
__global__ __launch_bounds__(kThreads) void lens_kernel(const LensArgs a, const LensKnot* __restrict__ table, const float* __restrict__ radiance,
                                                        unsigned char* __restrict__ rgb8, float* __restrict__ radiance_out, int tiles_x, int tiles)
{
    __shared__ LensKnot s_table[kLensKnots + 1];
    for (int i = threadIdx.x; i < kLensKnots + 1; i += kThreads) s_table[i] = table[i];
    __syncthreads();

    const int tx = threadIdx.x & (kTileW - 1), ty = threadIdx.x / kTileW;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int x = (tile % tiles_x) * kTileW + tx, y = (tile / tiles_x) * kTileH + ty;
        if (x < a.width && y < a.height) {
            float v[3];
            lens_pixel<FILTER, PER_CHANNEL>(a, s_table, radiance, x, y, v);
            store_rgb((size_t)y * (size_t)a.width + (size_t)x, v, rgb8, radiance_out);
        }
    }
}

template <int FILTER, bool PER_CHANNEL>
void launch(const LensArgs& a, const LensKnot* table, const float* radiance, unsigned char* rgb8, float* radiance_out, int max_blocks, hipStream_t stream)
{
    const int tiles_x = (a.width + kTileW - 1) / kTileW, tiles_y = (a.height + kTileH - 1) / kTileH;
    const long long tiles = (long long)tiles_x * tiles_y; // at most 2048 * 8192
    const int blocks = tiles < (long long)max_blocks ? (int)tiles : max_blocks;
    hipLaunchKernelGGL((lens_kernel<FILTER, PER_CHANNEL>), dim3((unsigned)blocks), dim3(kThreads), 0, stream, a, table, radiance, rgb8, radiance_out, tiles_x,
                       (int)tiles);
}

template <int FILTER>
void launch_filter(const LensArgs& a, const LensKnot* table, const float* radiance, unsigned char* rgb8, float* radiance_out, int max_blocks,
                   hipStream_t stream)
{
    if (a.per_channel)
        launch<FILTER, true>(a, table, radiance, rgb8, radiance_out, max_blocks, stream);
    else
        launch<FILTER, false>(a, table, radiance, rgb8, radiance_out, max_blocks, stream);
}

} // namespace

hipError_t launch_lens(const LensArgs& a, const LensKnot* table, const float* radiance, unsigned char* rgb8, float* radiance_out, int max_blocks,
                       hipStream_t stream)
{
    if (a.width <= 0 || a.height <= 0) return hipSuccess;
    if (max_blocks < 1) max_blocks = 1;
    if (a.filter == kLensBilinear)
        launch_filter<kLensBilinear>(a, table, radiance, rgb8, radiance_out, max_blocks, stream);
    else if (a.filter == kLensCatmullRom)
        launch_filter<kLensCatmullRom>(a, table, radiance, rgb8, radiance_out, max_blocks, stream);
    else
        launch_filter<kLensCatmullRomClamped>(a, table, radiance, rgb8, radiance_out, max_blocks, stream);
    return hipGetLastError();
}

} // namespace ff
