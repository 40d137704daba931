// ff_yuv.hip — the kernel behind ff_encode_yuv: display-linear float3 into the NV12 / P010 planes of a video encoder.  A translation
// unit of its own beside the other image kernels and the trace kernels, which it does not touch.  The
// operator is in include/firefly/ff_api.h and, as code, in ff_yuv.h, which the host twin ff_encode_yuv_host compiles too.
//
//   yuv_kernel<DEPTH, LEFT>   one workgroup of 256 threads copies the transfer's 4 097 knots into LDS (16 388 bytes) once and then
//                             walks tiles of 64 x 32 pixels, grid-strided.  A lane owns a block of 4 x 2 luma pixels - two chroma
//                             samples - and a wave 16 x 4 such blocks, so a wave reads 768 consecutive bytes of each of its eight
//                             rows.  The twelve halving steps of step 4 read the knots out of LDS.  With LEFT siting the tap at
//                             column 4 lx - 1 is the last column of the lane to the left: it comes over by a cross-lane move of the
//                             two rows' cb and cr; the 16 lanes on a tile's left edge compute that column themselves (column 0 of
//                             the image is its own clamped tap).  When the width is a multiple of 4 and the buffers are 16-byte
//                             aligned (YuvArgs::vec), a lane loads each row as three float4 and every store is whole dwords: four Y
//                             bytes per row and one Cb Cr Cb Cr dword for NV12, twice that for P010.  Otherwise a scalar path with
//                             clamped coordinates covers the right remainder; the bottom one (an odd height) repeats the last row.
//                             No global atomics, no scratch.  DEPTH = 8 | 10, LEFT = FF_YUV_SITING_LEFT: four instantiations.
#include "ff_yuv.h"

namespace ff {
namespace {

constexpr int kThreads = 256;
constexpr int kLanesX = 16, kLanesY = kThreads / kLanesX;     // lanes of a tile
constexpr int kTileW = 4 * kLanesX, kTileH = 2 * kLanesY;     // 64 x 32 pixels
constexpr int kMaxBlocks = 2048;

template <int DEPTH>
__device__ __forceinline__ void store_codes4(void* plane, size_t first, bool vec, int n, int c0, int c1, int c2, int c3)
{
    // codes c0 .. c3 to samples first .. first + 3 of `plane`; only the first n of them exist (vec: n == 4 and `first` is a multiple of 4)
    if (DEPTH == 8) {
        unsigned char* p = (unsigned char*)plane + first;
        if (vec) {
            *reinterpret_cast<uint32_t*>(p) = (uint32_t)c0 | ((uint32_t)c1 << 8) | ((uint32_t)c2 << 16) | ((uint32_t)c3 << 24);
        } else {
            if (n > 0) p[0] = (unsigned char)c0;
            if (n > 1) p[1] = (unsigned char)c1;
            if (n > 2) p[2] = (unsigned char)c2;
            if (n > 3) p[3] = (unsigned char)c3;
        }
    } else {
        uint16_t* p = (uint16_t*)plane + first;
        if (vec) {
            uint2 q;
            q.x = ((uint32_t)c0 << 6) | ((uint32_t)c1 << 22);
            q.y = ((uint32_t)c2 << 6) | ((uint32_t)c3 << 22);
            *reinterpret_cast<uint2*>(p) = q;
        } else {
            if (n > 0) p[0] = (uint16_t)(c0 << 6);
            if (n > 1) p[1] = (uint16_t)(c1 << 6);
            if (n > 2) p[2] = (uint16_t)(c2 << 6);
            if (n > 3) p[3] = (uint16_t)(c3 << 6);
        }
    }
}

template <int DEPTH, bool LEFT>
__global__ __launch_bounds__(kThreads) void yuv_kernel(const YuvArgs a, const float* __restrict__ in, void* __restrict__ luma, void* __restrict__ chroma,
                                                       int tiles_x, int tiles)
{
    __shared__ float s_k[kYuvKnots];
    for (int i = threadIdx.x; i < kYuvKnots; i += kThreads) s_k[i] = a.knots[i];
    __syncthreads();

    const int lx = threadIdx.x & (kLanesX - 1), ly = threadIdx.x / kLanesX;
    const size_t w = (size_t)a.width;
    const size_t cw = (size_t)((a.width + 1) >> 1);
    const bool vec = a.vec != 0;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
        const int x0 = tx * kTileW + 4 * lx, y0 = ty * kTileH + 2 * ly; // the lane's block; x0 < width and y0 < height, or the lane idles
        const bool active = x0 < a.width && y0 < a.height;
        const bool two_rows = y0 + 1 < a.height;
        YuvPixel px[2][4];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                px[r][k].y = 0;
                px[r][k].cb = px[r][k].cr = 0.f;
            }
        if (active) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                if (r == 1 && !two_rows) { // the row below the image is the last row again
#pragma unroll
                    for (int k = 0; k < 4; ++k) px[1][k] = px[0][k];
                    break;
                }
                const size_t row = (size_t)(y0 + r) * w;
                float c[12];
                if (vec) {
                    const float4* q = reinterpret_cast<const float4*>(in + 3 * (row + (size_t)x0));
                    const float4 q0 = q[0], q1 = q[1], q2 = q[2];
                    c[0] = q0.x; c[1] = q0.y; c[2] = q0.z; c[3] = q0.w;
                    c[4] = q1.x; c[5] = q1.y; c[6] = q1.z; c[7] = q1.w;
                    c[8] = q2.x; c[9] = q2.y; c[10] = q2.z; c[11] = q2.w;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int xx = x0 + k < a.width ? x0 + k : a.width - 1; // a column right of the image is the last column again
                        const float* q = in + 3 * (row + (size_t)xx);
                        c[3 * k] = q[0];
                        c[3 * k + 1] = q[1];
                        c[3 * k + 2] = q[2];
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) px[r][k] = yuv_pixel<DEPTH>(a, s_k, c + 3 * k);
            }
        }

        float cb0, cr0, cb1, cr1; // the lane's two chroma samples, unquantised
        if (LEFT) {
            // column x0 - 1 of both rows: the left neighbour's last column (every lane of the wave takes part in the move)
            float ecb[2], ecr[2];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                ecb[r] = __shfl_up(px[r][3].cb, 1);
                ecr[r] = __shfl_up(px[r][3].cr, 1);
            }
            if (active && lx == 0) {
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    if (x0 == 0) { // clamped into the image: column 0 itself
                        ecb[r] = px[r][0].cb;
                        ecr[r] = px[r][0].cr;
                    } else if (r == 1 && !two_rows) {
                        ecb[1] = ecb[0];
                        ecr[1] = ecr[0];
                    } else {
                        const float* q = in + 3 * ((size_t)(y0 + r) * w + (size_t)(x0 - 1));
                        const float c[3] = { q[0], q[1], q[2] };
                        const YuvPixel e = yuv_pixel<DEPTH>(a, s_k, c);
                        ecb[r] = e.cb;
                        ecr[r] = e.cr;
                    }
                }
            }
            cb0 = yuv_chroma_left(ecb[0], px[0][0].cb, px[0][1].cb, ecb[1], px[1][0].cb, px[1][1].cb);
            cr0 = yuv_chroma_left(ecr[0], px[0][0].cr, px[0][1].cr, ecr[1], px[1][0].cr, px[1][1].cr);
            cb1 = yuv_chroma_left(px[0][1].cb, px[0][2].cb, px[0][3].cb, px[1][1].cb, px[1][2].cb, px[1][3].cb);
            cr1 = yuv_chroma_left(px[0][1].cr, px[0][2].cr, px[0][3].cr, px[1][1].cr, px[1][2].cr, px[1][3].cr);
        } else {
            cb0 = yuv_chroma_center(px[0][0].cb, px[0][1].cb, px[1][0].cb, px[1][1].cb);
            cr0 = yuv_chroma_center(px[0][0].cr, px[0][1].cr, px[1][0].cr, px[1][1].cr);
            cb1 = yuv_chroma_center(px[0][2].cb, px[0][3].cb, px[1][2].cb, px[1][3].cb);
            cr1 = yuv_chroma_center(px[0][2].cr, px[0][3].cr, px[1][2].cr, px[1][3].cr);
        }
        if (!active) continue;

        const int nx = a.width - x0 < 4 ? a.width - x0 : 4; // luma columns of the block inside the image
        store_codes4<DEPTH>(luma, (size_t)y0 * w + (size_t)x0, vec, nx, px[0][0].y, px[0][1].y, px[0][2].y, px[0][3].y);
        if (two_rows) store_codes4<DEPTH>(luma, (size_t)(y0 + 1) * w + (size_t)x0, vec, nx, px[1][0].y, px[1][1].y, px[1][2].y, px[1][3].y);
        // the chroma row y0 / 2 holds cw interleaved pairs; the lane's samples are x0 / 2 and, where column x0 + 2 exists, x0 / 2 + 1
        const size_t first = 2 * ((size_t)(y0 >> 1) * cw + (size_t)(x0 >> 1));
        store_codes4<DEPTH>(chroma, first, vec, nx > 2 ? 4 : 2, yuv_quant_chroma<DEPTH>(cb0, a.full), yuv_quant_chroma<DEPTH>(cr0, a.full),
                            yuv_quant_chroma<DEPTH>(cb1, a.full), yuv_quant_chroma<DEPTH>(cr1, a.full));
    }
}

template <int DEPTH, bool LEFT>
void launch(const YuvArgs& a, const float* in, void* luma, void* chroma, hipStream_t stream)
{
    const int tiles_x = (a.width + kTileW - 1) / kTileW, tiles_y = (a.height + kTileH - 1) / kTileH;
    const long long tiles = (long long)tiles_x * tiles_y; // at most 1024 x 2048
    const unsigned grid = (unsigned)(tiles < kMaxBlocks ? tiles : kMaxBlocks);
    hipLaunchKernelGGL((yuv_kernel<DEPTH, LEFT>), dim3(grid), dim3(kThreads), 0, stream, a, in, luma, chroma, tiles_x, (int)tiles);
}

} // namespace

hipError_t launch_encode_yuv(const YuvArgs& a, const float* linear_in, void* luma, void* chroma, hipStream_t stream)
{
    if (a.width <= 0 || a.height <= 0) return hipSuccess;
    if (a.depth == 8) {
        if (a.left)
            launch<8, true>(a, linear_in, luma, chroma, stream);
        else
            launch<8, false>(a, linear_in, luma, chroma, stream);
    } else {
        if (a.left)
            launch<10, true>(a, linear_in, luma, chroma, stream);
        else
            launch<10, false>(a, linear_in, luma, chroma, stream);
    }
    return hipGetLastError();
}

} // namespace ff
