// ff_grade.h — the colour grade behind ff_color_grade: per pixel a primary grade (an affine 3 x 3 matrix and a saturation), one
// piecewise-linear curve per channel on a linear or a float-bit-pattern ("log") knot axis, and a 3D lattice read tetrahedrally or
// trilinearly, each stage run only when its flag is set.  The per-pixel functions are inline and compiled for the host and the device
// alike: the kernels (ff_grade.hip) and the host twin ff_color_grade_host (ff_grade_api.cpp) call the same code.  The operator is
// spelled out in include/firefly/ff_api.h.
//
// Arithmetic: float32 + - * / and floorf, integer work on the bit pattern, every product rounded before the sum that takes it (the
// library is built with -ffp-contract=off), min and max as written below; nothing else, so the two sides agree bit for bit.
//
// Not offered: other channel counts, a per-channel curve axis, shaper curves stored inside a 3D .cube, lattices that are not cubes,
// a row pitch, a grade fused into ff_display.
#pragma once

#include "../../include/firefly/ff_types.h"

#include "ff_pixel.h"

namespace ff {

constexpr int kGradeMaxLuts = 16;         // LUT objects per state
constexpr int kGradeMaxCurve = 4096;      // K
constexpr int kGradeMaxSize = 65;         // N
constexpr int kGradeLdsMaxSize = 17;      // the largest N whose lattice the kernels keep in LDS (58 956 bytes as float3)
constexpr size_t kGradeLdsBytes = 65536;  // what a workgroup may take: the lattice, then the curves while they fit beside it
// The kernels' launch (ff_grade.hip): a fixed grid of at most kGradeMaxBlocks workgroups of kGradeThreads lanes walks the image's
// quads of kGradePixelsPerLane consecutive pixels, grid-strided.
constexpr int kGradeThreads = 256;
constexpr int kGradePixelsPerLane = 4;
constexpr int kGradeMaxBlocks = 512;

// Where a kernel finds the lattice and the curves (a template argument of the kernels).
enum GradeHome {
    kGradeHomeGlobal = 0,    // the lattice in global memory (float4 texels); the curves in LDS
    kGradeHomeLds = 1,       // the lattice (float3 texels) and the curves in LDS
    kGradeHomeLdsCurvesOut = 2 // the lattice in LDS, the curves in global memory: they did not fit beside it
};

// Everything one call needs besides its image buffers; passed by value (kernel arguments).
struct GradeArgs {
    uint32_t flags;       // FF_GRADE_*
    float m[9], o[3], saturation;
    // the curves: 3 * K floats, channel-major
    int curve_size, curve_axis, curve_shift;
    float curve_lo, curve_hi, curve_range, curve_scale; // hi - lo and float(K - 1), each rounded once
    uint32_t curve_lo_bits;
    float curve_unit;     // float(1 << shift)
    const float* curves;
    // the lattice: N^3 texels, red fastest
    int size;
    float dmin[3], dmax[3], drange[3], size_scale; // dmax - dmin per channel and float(N - 1)
    const float4* table;  // device: padded texels; the twin reads FfGradeLut::table itself
    // the kernels alone
    int home;             // GradeHome
    int vec_in, vec_out, vec_rgb8; // whole-dword moves: the buffer is 16-byte (rgb8: 4-byte) aligned
};

// min and max as the header defines them: a NaN first argument gives the second (only an overflowed primary stage makes one).
FF_PIXEL_HD float grade_max(float a, float b) { return a > b ? a : b; }
FF_PIXEL_HD float grade_min(float a, float b) { return a < b ? a : b; }
FF_PIXEL_HD float grade_clamp(float x, float lo, float hi) { return grade_min(grade_max(x, lo), hi); }

FF_PIXEL_HD uint32_t grade_bits(float v)
{
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    return u;
}

// Stage 1: the affine matrix, then the saturation about the Rec. 709 luminance.
FF_PIXEL_HD void grade_primary(const GradeArgs& a, float* c)
{
    const float r = c[0], g = c[1], b = c[2];
    const float cr = ((a.m[0] * r + a.m[1] * g) + a.m[2] * b) + a.o[0];
    const float cg = ((a.m[3] * r + a.m[4] * g) + a.m[5] * b) + a.o[1];
    const float cb = ((a.m[6] * r + a.m[7] * g) + a.m[8] * b) + a.o[2];
    const float l = (0.2126f * cr + 0.7152f * cg) + 0.0722f * cb;
    c[0] = l + a.saturation * (cr - l);
    c[1] = l + a.saturation * (cg - l);
    c[2] = l + a.saturation * (cb - l);
}

// Stage 2, one channel: knots C[0 .. K-1] of that channel.
FF_PIXEL_HD float grade_curve(const GradeArgs& a, const float* C, float x)
{
    const float xc = grade_clamp(x, a.curve_lo, a.curve_hi);
    int k;
    float t;
    if (a.curve_axis == FF_GRADE_AXIS_LOG) {
        const uint32_t d = grade_bits(xc) - a.curve_lo_bits;
        const uint32_t cell = d >> a.curve_shift;
        k = cell < (uint32_t)(a.curve_size - 2) ? (int)cell : a.curve_size - 2;
        t = (float)(d - ((uint32_t)k << a.curve_shift)) / a.curve_unit;
    } else {
        const float p = ((xc - a.curve_lo) / a.curve_range) * a.curve_scale;
        const int cell = (int)floorf(p);
        k = cell < a.curve_size - 2 ? cell : a.curve_size - 2;
        t = p - (float)k;
    }
    const float c0 = C[k], c1 = C[k + 1];
    return c0 + t * (c1 - c0);
}

// Stage 3: the cell and the fraction of one channel ...
FF_PIXEL_HD void grade_cell(const GradeArgs& a, int ch, float x, int& i, float& f)
{
    const float u = (grade_clamp(x, a.dmin[ch], a.dmax[ch]) - a.dmin[ch]) / a.drange[ch];
    const float p = u * a.size_scale;
    const int cell = (int)floorf(p);
    i = cell < a.size - 2 ? cell : a.size - 2;
    f = p - (float)i;
}

// ... and the lattice read.  fetch(index, out[3]) returns texel `index` = i + N (j + N k).
template <bool TRILINEAR, class Fetch>
FF_PIXEL_HD void grade_lattice(const GradeArgs& a, const Fetch& fetch, float* c)
{
    int i, j, k;
    float fr, fg, fb;
    grade_cell(a, 0, c[0], i, fr);
    grade_cell(a, 1, c[1], j, fg);
    grade_cell(a, 2, c[2], k, fb);
    const int N = a.size, NN = N * N;
    const int base = i + N * (j + N * k);
    if (TRILINEAR) {
        float v[8][3];
#pragma unroll
        for (int n = 0; n < 8; ++n) fetch(base + (n & 1) + ((n >> 1) & 1) * N + (n >> 2) * NN, v[n]);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float r00 = v[0][ch] + fr * (v[1][ch] - v[0][ch]);
            const float r10 = v[2][ch] + fr * (v[3][ch] - v[2][ch]);
            const float r01 = v[4][ch] + fr * (v[5][ch] - v[4][ch]);
            const float r11 = v[6][ch] + fr * (v[7][ch] - v[6][ch]);
            const float g0 = r00 + fg * (r10 - r00);
            const float g1 = r01 + fg * (r11 - r01);
            c[ch] = g0 + fb * (g1 - g0);
        }
    } else {
        // the three fractions in descending order under a stable sort (ties keep r before g before b): a >= b >= c on axes A, B
        float fa, fm, fc;
        int da, dm;
        if (fr >= fg) {
            if (fg >= fb) { fa = fr; fm = fg; fc = fb; da = 1; dm = N; }        // r g b
            else if (fr >= fb) { fa = fr; fm = fb; fc = fg; da = 1; dm = NN; }  // r b g
            else { fa = fb; fm = fr; fc = fg; da = NN; dm = 1; }                // b r g
        } else {
            if (fb > fg) { fa = fb; fm = fg; fc = fr; da = NN; dm = N; }        // b g r
            else if (fb > fr) { fa = fg; fm = fb; fc = fr; da = N; dm = NN; }   // g b r
            else { fa = fg; fm = fr; fc = fb; da = N; dm = 1; }                 // g r b
        }
        float p0[3], p1[3], p2[3], p3[3];
        fetch(base, p0);
        fetch(base + da, p1);
        fetch(base + da + dm, p2);
        fetch(base + 1 + N + NN, p3);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) c[ch] = ((p0[ch] + fa * (p1[ch] - p0[ch])) + fm * (p2[ch] - p1[ch])) + fc * (p3[ch] - p2[ch]);
    }
}

// One pixel through the stages that are compiled in.  CC: the three channels' knots, K floats apart.
template <bool PRIMARY, bool CURVES, int LUT /* 0 none, 1 tetrahedral, 2 trilinear */, class Fetch>
FF_PIXEL_HD void grade_pixel(const GradeArgs& a, const float* CC, const Fetch& fetch, const float* in, float* out)
{
    out[0] = in[0];
    out[1] = in[1];
    out[2] = in[2];
    if (!(pixel_finite(in[0]) && pixel_finite(in[1]) && pixel_finite(in[2]))) return; // copied bit for bit
    if (PRIMARY) grade_primary(a, out);
    if (CURVES) {
        out[0] = grade_curve(a, CC, out[0]);
        out[1] = grade_curve(a, CC + a.curve_size, out[1]);
        out[2] = grade_curve(a, CC + 2 * a.curve_size, out[2]);
    }
    if (LUT == 1) grade_lattice<false>(a, fetch, out);
    if (LUT == 2) grade_lattice<true>(a, fetch, out);
}

// The LDS bytes a workgroup takes under `home`: the lattice as float3 (rounded up to 16 bytes), then the curves.
FF_PIXEL_HD size_t grade_lattice_lds_bytes(int size) { return (((size_t)size * size * size * 12) + 15) & ~(size_t)15; }
inline size_t grade_lds_bytes(int home, bool curves, int curve_size, bool lattice, int size)
{
    size_t n = 0;
    if (lattice && home != kGradeHomeGlobal) n += grade_lattice_lds_bytes(size);
    if (curves && home != kGradeHomeLdsCurvesOut) n += (size_t)curve_size * 12;
    return n;
}

// The kernel (ff_grade.hip): radiance_in (px pixels) -> rgb8 / radiance_out, either of which may be null; radiance_out may be
// radiance_in itself.  hipErrorInvalidValue for a key no instantiation serves.
hipError_t launch_color_grade(const GradeArgs& a, size_t px, const float* radiance_in, unsigned char* rgb8, float* radiance_out, hipStream_t stream);

} // namespace ff
