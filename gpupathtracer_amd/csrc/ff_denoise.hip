// ff_denoise.hip — image kernels beside the trace kernels: the G-buffer resolve of ff_gbuffer and the
// edge-avoiding à-trous filter of ff_denoise (Dammertz et al. 2010).  Nothing here is inlined into, or shares a translation unit
// with, the trace kernels: their schedule moves with any edit around them.
//
// Numerics of the resolve: compiled with the library's flags (-ffp-contract=off, IEEE-correct sqrt and divide), it restates the
// few lines of the trace kernels it needs - the world-normal transform of Intersect::m_normal and the tile-major item order - with
// the same operation order, so every channel is bit for bit what ff_intersect_rays returns for the pixel's primary ray.
#include "ff_denoise.h"

namespace ff {
namespace {

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz)
{
    // glm dot(vec3): (x + y) + z, as the trace kernels evaluate it
    const float px = ax * bx, py = ay * by, pz = az * bz;
    return (px + py) + pz;
}

// One thread per pixel, rows of 64 pixels per wave: every output row is written as whole cache lines; the stored hits of a wave's
// pixels are eight runs of 128 bytes (an 8x8 tile row) per plane.
__global__ __launch_bounds__(256) void gbuffer_resolve_kernel(const GbufferResolveParams p)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= p.width || y >= p.height) return;
    const size_t i = (size_t)y * (size_t)p.width + (size_t)x;
    float t = 0.f, px = 0.f, py = 0.f, pz = 0.f, nx = 0.f, ny = 0.f, nz = 0.f, ax = 0.f, ay = 0.f, az = 0.f;
    int geom = -1, tri = -1, bxdf = -1;
    if (x < p.xlim && y < p.ylim) { // (pixels the frame does not trace read as misses: kernel.cu:308-309)
        // the pixel's item: 64 per 8x8 tile, tiles row by row (the trace kernels' work-queue order)
        const unsigned pitem = (unsigned)(((y >> 3) * p.tiles_per_row + (x >> 3)) * 64 + ((y & 7) * 8 + (x & 7)));
        const float4 h1 = p.hits[(size_t)p.pix_items + pitem];
        const int g = __float_as_int(h1.w);
        const int rec = __float_as_int(p.hits[2 * (size_t)p.pix_items + pitem].x);
        if (g >= 0 && g < p.num_geoms && rec < p.num_tris) { // (the records a hit names; the bounds only guard the reads)
            const float4 h0 = p.hits[pitem];
            const GeomRecord& G = p.geoms[g];
            t = h0.x;
            px = h0.y;
            py = h0.z;
            pz = h0.w;
            // object-space normal: a triangle's face normal cross(e1, e2), normalised in object space (kernel.cu:101, what
            // Intersect::m_normal carries).  Recomputed from the record: the hits of a FF_SHADE_DIFFUSE_PATH_SMOOTH frame hold
            // the interpolated vertex normal there.  A plane's m_normal; a sphere's unit normal as the pre-pass stored it.
            float ox, oy, oz;
            if (rec >= 0) {
                const TriRecord& R = p.tris[rec];
                const float e1x = R.e1[0], e1y = R.e1[1], e1z = R.e1[2], e2x = R.e2[0], e2y = R.e2[1], e2z = R.e2[2];
                ox = e1y * e2z - e2y * e1z;
                oy = e1z * e2x - e2z * e1x;
                oz = e1x * e2y - e2x * e1y;
                const float inv = 1.0f / sqrtf(dot3(ox, oy, oz, ox, oy, oz)); // (correctly rounded, as ieee_rcp(ieee_sqrt()))
                ox = ox * inv;
                oy = oy * inv;
                oz = oz * inv;
                tri = R.orig_index;
            } else if (G.type == FF_GEOM_PLANE) {
                ox = G.plane_n[0];
                oy = G.plane_n[1];
                oz = G.plane_n[2];
            } else {
                ox = h1.x;
                oy = h1.y;
                oz = h1.z;
            }
            // inverse(transpose(model)) * vec4(n, 0) (kernel.cu:117): the w slots hold column3 * 0, the signed zero glm adds
            nx = (G.nrm_c0[0] * ox + G.nrm_c1[0] * oy) + (G.nrm_c2[0] * oz + G.nrm_c0[3]);
            ny = (G.nrm_c0[1] * ox + G.nrm_c1[1] * oy) + (G.nrm_c2[1] * oz + G.nrm_c1[3]);
            nz = (G.nrm_c0[2] * ox + G.nrm_c1[2] * oy) + (G.nrm_c2[2] * oz + G.nrm_c2[3]);
            // the colour the surface multiplies or emits (the scene compiler's record slots: ff_scene.cpp): emitter m_emissiveColor *
            // m_intensity, mirror m_specularColor and diffuse m_albedo (the tint slot), glass m_transmittanceColor (the emission slot)
            bxdf = G.bxdf_type;
            const float* col = (bxdf == FF_BXDF_EMITTER || bxdf == FF_BXDF_GLASS) ? G.emission : G.albedo;
            ax = col[0];
            ay = col[1];
            az = col[2];
            if (p.tex_bind && bxdf == FF_BXDF_DIFFUSE) {
                // the integrator's lookup (nee_path_kernel): the same function of the same world point, so the same bits
                float texel[3];
                if (tex_albedo(p.tex_bind, p.tex_desc, p.uvs, g, rec, G.type, reinterpret_cast<const float*>(&G), reinterpret_cast<const float*>(p.tris), px, py, pz,
                               texel)) {
                    ax = ax * texel[0];
                    ay = ay * texel[1];
                    az = az * texel[2];
                }
            }
            geom = G.orig_index;
        }
    }
    if (p.depth) p.depth[i] = t;
    if (p.position) { p.position[3 * i] = px; p.position[3 * i + 1] = py; p.position[3 * i + 2] = pz; }
    if (p.normal) { p.normal[3 * i] = nx; p.normal[3 * i + 1] = ny; p.normal[3 * i + 2] = nz; }
    if (p.albedo) { p.albedo[3 * i] = ax; p.albedo[3 * i + 1] = ay; p.albedo[3 * i + 2] = az; }
    if (p.ids) { p.ids[3 * i] = geom; p.ids[3 * i + 1] = tri; p.ids[3 * i + 2] = bxdf; }
}

// ---- edge-avoiding à-trous filter ------------------------------------------------------------------------------------

constexpr int kTile = 16;                   // 16 x 16 pixels per workgroup (four waves of 16 x 4): a wave's 25 taps fall on few lines
constexpr float kColorEps = 1e-30f;         // keeps |c_p|^2 = 0 finite; far below any radiance the integrator produces (scale-free)
constexpr float kPlaneEps = 1e-30f;         // ... and |x_q - x_p|^2 = 0 for coincident points
constexpr float kMaxExponent = 30.f;        // a tap whose weight is below e^-30 of its B3 factor weighs 0: its products would be far below the
                                            // pixel's colour, some of them subnormal, which rounds differently at another scale of the input
__constant__ float kB3[5] = { 1.f / 16.f, 1.f / 4.f, 3.f / 8.f, 1.f / 4.f, 1.f / 16.f }; // B3-spline taps

__global__ __launch_bounds__(256) void denoise_pack_kernel(const DenoiseBuffers b, const float* __restrict__ radiance, const float* __restrict__ position,
                                                           const float* __restrict__ normal, const float* __restrict__ albedo, const int* __restrict__ ids,
                                                           int demodulate)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= b.width || y >= b.height) return;
    const size_t i = (size_t)y * (size_t)b.width + (size_t)x;
    const int geom = ids[3 * i], bxdf = ids[3 * i + 2];
    // filterable: a hit on a surface that is neither an emitter (exact at the primary hit) nor specular (its guides describe the
    // mirror, not what it shows)
    const bool filt = geom >= 0 && bxdf != FF_BXDF_EMITTER && bxdf != FF_BXDF_MIRROR && bxdf != FF_BXDF_GLASS;
    float nx = normal[3 * i], ny = normal[3 * i + 1], nz = normal[3 * i + 2];
    const float n2 = dot3(nx, ny, nz, nx, ny, nz);
    const float inv = n2 > 0.f ? 1.0f / sqrtf(n2) : 0.f; // (the G-buffer normal is not unit length under non-uniform scale)
    nx *= inv;
    ny *= inv;
    nz *= inv;
    b.guide_pos[i] = make_float4(position[3 * i], position[3 * i + 1], position[3 * i + 2], __int_as_float(filt ? geom : -1));
    b.guide_nrm[i] = make_float4(nx, ny, nz, 0.f);
    float cx = radiance[3 * i], cy = radiance[3 * i + 1], cz = radiance[3 * i + 2];
    if (demodulate && filt) {
        const float ax = albedo[3 * i], ay = albedo[3 * i + 1], az = albedo[3 * i + 2];
        if (ax > 0.f) cx = cx / ax;
        if (ay > 0.f) cy = cy / ay;
        if (az > 0.f) cz = cz / az;
    }
    b.color[0][i] = make_float4(cx, cy, cz, 0.f);
}

// One à-trous pass: out_p = c_p - sum_q w_q (c_p - c_q) / sum_q w_q over the 5x5 taps 2^pass apart (= sum w c_q / sum w; the form
// returns a constant colour exactly), w = h(dx) h(dy) exp(-(a_c + a_n + a_x)) with
//   a_c = |c_p - c_q|^2 / (sigma_i^2 (|c_p|^2 + eps)),  a_n = (1 - n_p.n_q) / sigma_normal,  a_x = (n_p.(x_q - x_p))^2 / (sigma_plane^2 |x_q - x_p|^2 + eps).
// The centre tap weighs h(0) h(0); a tap with a_c + a_n + a_x > 30 weighs 0.  Taps outside the image, on pixels that are not filterable or (same_geometry) on another
// geometry weigh 0.  Only filterable pixels are written: nobody reads the others.  Plain loads: the guides and colours of a
// 1080p frame (96 MB) stay in L2 / MALL between taps and passes.
__global__ __launch_bounds__(256) void denoise_pass_kernel(const DenoiseBuffers b, int src, int step, float inv_sigma_color2, float inv_sigma_normal,
                                                           float sigma_plane2, int same_geometry)
{
    const int x = blockIdx.x * kTile + (threadIdx.x & (kTile - 1)), y = blockIdx.y * kTile + (threadIdx.x / kTile);
    if (x >= b.width || y >= b.height) return;
    const int W = b.width, H = b.height;
    const size_t i = (size_t)y * (size_t)W + (size_t)x;
    const float4 gp = b.guide_pos[i];
    const int cls = __float_as_int(gp.w);
    if (cls < 0) return;
    const float4 np = b.guide_nrm[i];
    const float4* __restrict__ cin = b.color[src];
    const float4 cp = cin[i];
    const float ccoef = inv_sigma_color2 * __builtin_amdgcn_rcpf(dot3(cp.x, cp.y, cp.z, cp.x, cp.y, cp.z) + kColorEps);
    float wsum = kB3[2] * kB3[2], sx = 0.f, sy = 0.f, sz = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int yy = y + dy * step;
        if (yy < 0 || yy >= H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            if (dx == 0 && dy == 0) continue;
            const int xx = x + dx * step;
            if (xx < 0 || xx >= W) continue;
            const size_t j = (size_t)yy * (size_t)W + (size_t)xx;
            const float4 gq = b.guide_pos[j];
            const int qcls = __float_as_int(gq.w);
            if (qcls < 0 || (same_geometry && qcls != cls)) continue;
            const float4 nq = b.guide_nrm[j];
            const float4 cq = cin[j];
            const float dcx = cp.x - cq.x, dcy = cp.y - cq.y, dcz = cp.z - cq.z;
            const float a_c = dot3(dcx, dcy, dcz, dcx, dcy, dcz) * ccoef;
            const float a_n = (1.0f - dot3(np.x, np.y, np.z, nq.x, nq.y, nq.z)) * inv_sigma_normal;
            const float vx = gq.x - gp.x, vy = gq.y - gp.y, vz = gq.z - gp.z;
            const float pd = dot3(np.x, np.y, np.z, vx, vy, vz);
            const float a_x = pd * pd * __builtin_amdgcn_rcpf(sigma_plane2 * dot3(vx, vy, vz, vx, vy, vz) + kPlaneEps);
            const float e = a_c + a_n + a_x;
            if (!(e <= kMaxExponent)) continue;
            const float w = (kB3[dx + 2] * kB3[dy + 2]) * __expf(-e);
            wsum += w;
            sx += w * dcx;
            sy += w * dcy;
            sz += w * dcz;
        }
    }
    const float r = __builtin_amdgcn_rcpf(wsum);
    b.color[1 - src][i] = make_float4(cp.x - sx * r, cp.y - sy * r, cp.z - sz * r, 0.f);
}

__device__ __forceinline__ unsigned char to_u8(float v)
{
    // the project's 8-bit rule (kernel.cu:214 truncation, out-of-range values clamped): ff_k_shade.h to_u8
    const float s = v * 255.0f;
    if (!(s > 0.0f)) return 0;
    if (s >= 255.0f) return 255;
    return (unsigned char)s;
}

__global__ __launch_bounds__(256) void denoise_finish_kernel(const DenoiseBuffers b, int src, const float* radiance_in, const float* __restrict__ albedo,
                                                             int demodulate, unsigned char* __restrict__ rgb8, float* radiance_out)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= b.width || y >= b.height) return;
    const size_t i = (size_t)y * (size_t)b.width + (size_t)x;
    // (radiance_out may alias radiance_in: this thread alone reads and writes pixel i)
    float vx = radiance_in[3 * i], vy = radiance_in[3 * i + 1], vz = radiance_in[3 * i + 2];
    if (src >= 0 && __float_as_int(b.guide_pos[i].w) >= 0) {
        const float4 c = b.color[src][i];
        vx = c.x;
        vy = c.y;
        vz = c.z;
        if (demodulate) {
            const float ax = albedo[3 * i], ay = albedo[3 * i + 1], az = albedo[3 * i + 2];
            if (ax > 0.f) vx = vx * ax;
            if (ay > 0.f) vy = vy * ay;
            if (az > 0.f) vz = vz * az;
        }
    }
    if (radiance_out) { radiance_out[3 * i] = vx; radiance_out[3 * i + 1] = vy; radiance_out[3 * i + 2] = vz; }
    if (rgb8) { rgb8[3 * i] = to_u8(vx); rgb8[3 * i + 1] = to_u8(vy); rgb8[3 * i + 2] = to_u8(vz); }
}

dim3 rows_grid(int width, int height) { return dim3((unsigned)((width + 63) / 64), (unsigned)((height + 3) / 4)); }

} // namespace

hipError_t launch_gbuffer_resolve(const GbufferResolveParams& p, hipStream_t stream)
{
    if (p.width <= 0 || p.height <= 0) return hipSuccess;
    hipLaunchKernelGGL(gbuffer_resolve_kernel, rows_grid(p.width, p.height), dim3(64, 4), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_denoise_pack(const DenoiseBuffers& b, const float* radiance, const float* position, const float* normal, const float* albedo,
                               const int* ids, int demodulate, hipStream_t stream)
{
    if (b.width <= 0 || b.height <= 0) return hipSuccess;
    hipLaunchKernelGGL(denoise_pack_kernel, rows_grid(b.width, b.height), dim3(64, 4), 0, stream, b, radiance, position, normal, albedo, ids, demodulate);
    return hipGetLastError();
}

hipError_t launch_denoise_pass(const DenoiseBuffers& b, int src, int pass, float inv_sigma_color2, float inv_sigma_normal, float sigma_plane2,
                               int same_geometry, hipStream_t stream)
{
    if (b.width <= 0 || b.height <= 0) return hipSuccess;
    const dim3 grid((unsigned)((b.width + kTile - 1) / kTile), (unsigned)((b.height + kTile - 1) / kTile));
    hipLaunchKernelGGL(denoise_pass_kernel, grid, dim3(kTile * kTile), 0, stream, b, src, 1 << pass, inv_sigma_color2, inv_sigma_normal, sigma_plane2,
                       same_geometry);
    return hipGetLastError();
}

hipError_t launch_denoise_finish(const DenoiseBuffers& b, int src, const float* radiance_in, const float* albedo, int demodulate, unsigned char* rgb8,
                                 float* radiance_out, hipStream_t stream)
{
    if (b.width <= 0 || b.height <= 0) return hipSuccess;
    hipLaunchKernelGGL(denoise_finish_kernel, rows_grid(b.width, b.height), dim3(64, 4), 0, stream, b, src, radiance_in, albedo, demodulate, rgb8,
                       radiance_out);
    return hipGetLastError();
}

} // namespace ff
