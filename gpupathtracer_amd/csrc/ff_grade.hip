// ff_grade.hip — the kernel behind ff_color_grade: a primary grade, per-channel curves and a 3D lattice per pixel.  A translation unit
// of its own beside the other image kernels and the trace kernels, which it does not touch.  The
// operator is in include/firefly/ff_api.h and, as code, in ff_grade.h, which the host twin ff_color_grade_host compiles too.
//
//   grade_kernel<PRIMARY, CURVES, LUT, HOME>   a fixed grid of at most kGradeMaxBlocks workgroups of 256 threads.  A workgroup first
//                             copies what its HOME keeps in LDS - the lattice as float3 texels (N <= kGradeLdsMaxSize: 58 956 bytes at
//                             17), then the curves (12 K bytes) while they fit beside it - once, and after one barrier walks the
//                             image's quads of four consecutive pixels, grid-strided, a lane on a quad: 48 bytes in, 48 + 12 out.  When
//                             a buffer is 16-byte aligned (rgb8: 4-byte) the lane moves its quad as three float4 (three dwords of
//                             bytes); otherwise, and in the last quad of an image whose pixel count is no multiple of 4, pixel by
//                             pixel.  A lane reads its whole quad before it writes, so radiance_out may be radiance_in.
//                             HOME = kGradeHomeGlobal reads the lattice from global memory, padded to float4 texels so that a
//                             vertex is one 16-byte load: 33^3 is 575 KB and 65^3 4.4 MB, served from L2 and the Infinity Cache.
//                             PRIMARY, CURVES: the stage is compiled in; LUT = 0 none | 1 tetrahedral (four vertices) | 2 trilinear
//                             (eight).  No atomics, no scratch.  The instantiations are FF_GRADE_KERNELS' rows.
#include "ff_grade.h"

namespace ff {
namespace {

struct FetchGlobal {
    const float4* t;
    FF_PIXEL_HD void operator()(int index, float* out) const
    {
        const float4 q = t[index];
        out[0] = q.x;
        out[1] = q.y;
        out[2] = q.z;
    }
};

struct FetchLds {
    const float* t;
    FF_PIXEL_HD void operator()(int index, float* out) const
    {
        out[0] = t[3 * index];
        out[1] = t[3 * index + 1];
        out[2] = t[3 * index + 2];
    }
};

template <bool PRIMARY, bool CURVES, int LUT, int HOME>
__global__ __launch_bounds__(kGradeThreads) void grade_kernel(const GradeArgs a, const float* in, unsigned char* rgb8, float* out, size_t px)
{
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    constexpr bool kLatticeLds = LUT != 0 && HOME != kGradeHomeGlobal;
    constexpr bool kCurvesLds = CURVES && HOME != kGradeHomeLdsCurvesOut;
    float* s_curves = s_mem;
    if (kLatticeLds) {
        const int texels = a.size * a.size * a.size;
        for (int i = threadIdx.x; i < texels; i += kGradeThreads) {
            const float4 q = a.table[i];
            s_mem[3 * i] = q.x;
            s_mem[3 * i + 1] = q.y;
            s_mem[3 * i + 2] = q.z;
        }
        s_curves = s_mem + grade_lattice_lds_bytes(a.size) / sizeof(float);
    }
    if (kCurvesLds)
        for (int i = threadIdx.x; i < 3 * a.curve_size; i += kGradeThreads) s_curves[i] = a.curves[i];
    if (kLatticeLds || kCurvesLds) __syncthreads();

    const size_t quads = (px + kGradePixelsPerLane - 1) / kGradePixelsPerLane;
    for (size_t q = (size_t)blockIdx.x * kGradeThreads + threadIdx.x; q < quads; q += (size_t)gridDim.x * kGradeThreads) {
        const size_t first = q * kGradePixelsPerLane;
        const int n = px - first < (size_t)kGradePixelsPerLane ? (int)(px - first) : kGradePixelsPerLane; // pixels of the quad inside the image
        const bool whole = n == kGradePixelsPerLane;
        float c[12], r[12];
        if (a.vec_in && whole) {
            const float4* src = reinterpret_cast<const float4*>(in + 3 * first);
            const float4 q0 = src[0], q1 = src[1], q2 = src[2];
            c[0] = q0.x; c[1] = q0.y; c[2] = q0.z; c[3] = q0.w;
            c[4] = q1.x; c[5] = q1.y; c[6] = q1.z; c[7] = q1.w;
            c[8] = q2.x; c[9] = q2.y; c[10] = q2.z; c[11] = q2.w;
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k) c[k] = k < 3 * n ? in[3 * first + k] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < kGradePixelsPerLane; ++k) {
            // (a pixel beyond the image is +0 and stores nothing: its lookups stay inside the tables)
            if (kLatticeLds)
                grade_pixel<PRIMARY, CURVES, LUT>(a, kCurvesLds ? s_curves : a.curves, FetchLds{ s_mem }, c + 3 * k, r + 3 * k);
            else
                grade_pixel<PRIMARY, CURVES, LUT>(a, kCurvesLds ? s_curves : a.curves, FetchGlobal{ a.table }, c + 3 * k, r + 3 * k);
        }
        if (out) {
            if (a.vec_out && whole) {
                float4* dst = reinterpret_cast<float4*>(out + 3 * first);
                dst[0] = make_float4(r[0], r[1], r[2], r[3]);
                dst[1] = make_float4(r[4], r[5], r[6], r[7]);
                dst[2] = make_float4(r[8], r[9], r[10], r[11]);
            } else {
#pragma unroll
                for (int k = 0; k < 12; ++k)
                    if (k < 3 * n) out[3 * first + k] = r[k];
            }
        }
        if (rgb8) {
            if (a.vec_rgb8 && whole) {
                uint32_t w[3];
#pragma unroll
                for (int d = 0; d < 3; ++d)
                    w[d] = (uint32_t)pixel_u8(r[4 * d]) | ((uint32_t)pixel_u8(r[4 * d + 1]) << 8) | ((uint32_t)pixel_u8(r[4 * d + 2]) << 16) |
                           ((uint32_t)pixel_u8(r[4 * d + 3]) << 24);
                uint32_t* dst = reinterpret_cast<uint32_t*>(rgb8 + 3 * first);
                dst[0] = w[0];
                dst[1] = w[1];
                dst[2] = w[2];
            } else {
#pragma unroll
                for (int k = 0; k < 12; ++k)
                    if (k < 3 * n) rgb8[3 * first + k] = pixel_u8(r[k]);
            }
        }
    }
}

// The instantiations, X(PRIMARY, CURVES, LUT, HOME): without a lattice HOME is kGradeHomeGlobal (the curves in LDS); with one, the
// lattice in global memory or in LDS, and with curves as well, the third home whose curves stay in global memory.  The first row
// is the copy of flags = 0.
#define FF_GRADE_KERNELS_OF(X, P)                                                                                      \
    X(P, false, 0, 0) X(P, true, 0, 0)                                                                                 \
    X(P, false, 1, 0) X(P, false, 1, 1) X(P, false, 2, 0) X(P, false, 2, 1)                                            \
    X(P, true, 1, 0) X(P, true, 1, 1) X(P, true, 1, 2) X(P, true, 2, 0) X(P, true, 2, 1) X(P, true, 2, 2)
#define FF_GRADE_KERNELS(X) FF_GRADE_KERNELS_OF(X, false) FF_GRADE_KERNELS_OF(X, true)
static_assert(kGradeHomeGlobal == 0 && kGradeHomeLds == 1 && kGradeHomeLdsCurvesOut == 2, "the HOME column spells the homes as numerals");

} // namespace

hipError_t launch_color_grade(const GradeArgs& a, size_t px, const float* radiance_in, unsigned char* rgb8, float* radiance_out, hipStream_t stream)
{
    if (px == 0) return hipSuccess;
    const bool primary = (a.flags & FF_GRADE_PRIMARY) != 0, curves = (a.flags & FF_GRADE_CURVES) != 0;
    const int lut = !(a.flags & FF_GRADE_LUT3D) ? 0 : ((a.flags & FF_GRADE_TRILINEAR) ? 2 : 1);
    if (curves && (a.curve_size < 2 || a.curve_size > kGradeMaxCurve || !a.curves)) return hipErrorInvalidValue;
    if (lut && (a.size < 2 || a.size > kGradeMaxSize || !a.table)) return hipErrorInvalidValue;
    if (a.home != kGradeHomeGlobal && (!lut || a.size > kGradeLdsMaxSize)) return hipErrorInvalidValue;
    const size_t lds = grade_lds_bytes(a.home, curves, a.curve_size, lut != 0, a.size);
    if (lds > kGradeLdsBytes) return hipErrorInvalidValue;
    const size_t quads = (px + kGradePixelsPerLane - 1) / kGradePixelsPerLane;
    const size_t blocks = (quads + kGradeThreads - 1) / kGradeThreads;
    const dim3 grid((unsigned)(blocks < (size_t)kGradeMaxBlocks ? blocks : (size_t)kGradeMaxBlocks));
#define FF_X(P, C, L, H)                                                                                               \
    if (primary == P && curves == C && lut == L && a.home == H)                                                        \
        hipLaunchKernelGGL((grade_kernel<P, C, L, H>), grid, dim3(kGradeThreads), lds, stream, a, radiance_in, rgb8, radiance_out, px); \
    else
    FF_GRADE_KERNELS(FF_X) return hipErrorInvalidValue;
#undef FF_X
    return hipGetLastError();
}

} // namespace ff
