// ff_frame_kernels.hip — the frame kernels that traverse nothing (cull mask, combine, the ieee_rcp / ieee_sqrt self-check, progressive
// accumulation, the two strip gathers) and their launchers.  Split from ff_kernels.hip so that an edit here recompiles in seconds.
#include "ff_k_shade.h" // primary_ray, to_u8; through it ff_k_lds.h (make_world_slab, slab_may_hit) and ff_k_core.h

namespace ff {
namespace {

// Which pixels of the local image can the camera not see anything in?  One thread per pixel item (tile-major, like the work
// queue's): primary ray (kernel.cu:197-205) against the padded box around all geometries - conservative like slab_may_hit:
// approximate reciprocals, inflated exit, NaN counts as "may hit" - one mask word per 64 items, and the block sums of a culled
// pixel zeroed for every block of the frame (the combine pass reads them all).
__global__ void cull_mask_kernel(const KParams p, unsigned long long* mask)
{
    const unsigned pitem = blockIdx.x * blockDim.x + threadIdx.x;
    bool culled = false;
    if (pitem < p.pix_items) {
        const int tile = (int)(pitem >> 6), in = (int)(pitem & 63u);
        const int lx = (tile % p.tiles_per_row) * 8 + (in & 7);
        const int ly = (tile / p.tiles_per_row) * 8 + (in >> 3);
        const int strip = ly / p.strip_rows;
        const int gy = p.y0 + (strip * p.num_parts + p.part) * p.strip_rows + (ly - strip * p.strip_rows);
        const int gx = p.x0 + lx;
        if (lx < p.local_width && gx < p.xlim && ly < p.local_rows && gy < p.ylim) {
            Ray r;
            primary_ray(p, (unsigned)gx | ((unsigned)gy << 16), r);
            culled = !slab_may_hit(p.scene_min[0], p.scene_min[1], p.scene_min[2], p.scene_max[0], p.scene_max[1], p.scene_max[2], make_world_slab(r), kInf);
            if (culled)
                for (int b = 0; b < p.num_blocks; ++b) p.blocksums[(size_t)pitem * p.num_blocks + b] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    const unsigned long long word = __ballot(culled);
    if ((threadIdx.x & 63) == 0 && pitem < ((p.pix_items + 63u) & ~63u)) {
        mask[pitem >> 6] = word;
        // (the host adds the slots and turns pixels into rays; on ONE address the 32 000 atomics of a 1080p frame queue up for
        // 0.3 ms - five times the reference's whole 1-spp frame)
        if (word) atomicAdd(&p.counters[kCulledPixelsWord + kRaySlotStride * ((pitem >> 6) % kRaySlots)], (unsigned long long)__popcll(word));
    }
}

// Final pass of a frame: add every pixel's sample-block sums in block order, scale by 1/spp (kernel.cu:214 stores the
// colour as 8 bits; the float radiance is kept next to it), write rows coalesced.  Untraced pixels keep the cleared 0.
__global__ void combine_kernel(const KParams p)
{
    const int lx = blockIdx.x * blockDim.x + threadIdx.x;
    const int ly = blockIdx.y;
    if (lx >= p.local_width || ly >= p.local_rows) return;
    const int strip = ly / p.strip_rows;
    const int gy = p.y0 + (strip * p.num_parts + p.part) * p.strip_rows + (ly - strip * p.strip_rows);
    if (p.x0 + lx >= p.xlim || gy >= p.ylim) return;
    const unsigned pitem = (unsigned)(((ly >> 3) * p.tiles_per_row + (lx >> 3)) * 64 + ((ly & 7) * 8 + (lx & 7)));
    float ax = 0.f, ay = 0.f, az = 0.f;
    // (a pixel that sees nothing is black whatever its sums hold: a frame that takes the mask over from the last one - same camera, same
    // scene - runs no pass that zeroes them, and its dropped items wrote none)
    const bool culled = p.cull_mask != nullptr && ((p.cull_mask[pitem >> 6] >> (pitem & 63u)) & 1ull) != 0ull;
    for (int b = 0; b < (culled ? 0 : p.num_blocks); ++b) {
        float4 v;
        if (p.tail_block >= 0 && b >= p.tail_block) {
            // this block was traced sample by sample (the frame's last block, or its last two): the sequential sum a lane would have
            // kept in registers.  The stored samples are numbered from the first of those blocks on.
            float bx = 0.f, by = 0.f, bz = 0.f;
            const float4* sp = p.tail_samples + pitem; // sample-major: neighbouring threads read neighbouring values
            const int first = (b - p.tail_block) * p.block_spp, past = min(p.tail_samples_in_block, first + p.block_spp);
            for (int i = first; i < past; ++i) {
                const float4 l = sp[(size_t)i * p.pix_items];
                bx = bx + l.x;
                by = by + l.y;
                bz = bz + l.z;
            }
            v = make_float4(bx, by, bz, 0.f);
        } else {
            v = p.blocksums[(size_t)pitem * p.num_blocks + b];
        }
        ax = ax + v.x;
        ay = ay + v.y;
        az = az + v.z;
    }
    float rx = ax, ry = ay, rz = az;
    if (p.shade_mode != FF_SHADE_NORMAL_DEBUG) {
        const float inv = 1.0f / (float)p.spp_total;
        rx = ax * inv; ry = ay * inv; rz = az * inv;
    }
    const size_t lpix = (size_t)ly * (size_t)p.local_width + (size_t)lx;
    if (p.radiance) {
        p.radiance[3 * lpix] = rx;
        p.radiance[3 * lpix + 1] = ry;
        p.radiance[3 * lpix + 2] = rz;
    }
    if (p.rgb8) {
        p.rgb8[3 * lpix] = to_u8(rx);
        p.rgb8[3 * lpix + 1] = to_u8(ry);
        p.rgb8[3 * lpix + 2] = to_u8(rz);
    }
}

// Exhaustive self-check of ieee_rcp / ieee_sqrt against the compiler's IEEE expansions: every float bit pattern.
__global__ void ieee_check_kernel(unsigned long long* mismatches)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    unsigned long long bad_rcp = 0, bad_sqrt = 0;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < (1ull << 32); i += stride) {
        const float x = __uint_as_float((unsigned)i);
        const float a = ieee_rcp(x), ra = 1.0f / x;
        const float b = ieee_sqrt(x), rb = sqrtf(x);
        if (__float_as_uint(a) != __float_as_uint(ra) && !(a != a && ra != ra)) ++bad_rcp;
        if (__float_as_uint(b) != __float_as_uint(rb) && !(b != b && rb != rb)) ++bad_sqrt;
    }
    if (bad_rcp) atomicAdd(&mismatches[0], bad_rcp);
    if (bad_sqrt) atomicAdd(&mismatches[1], bad_sqrt);
}

// Progressive accumulation (ff_render_progressive): running sum of whole frames, output = sum * (1 / frames).
__global__ void accumulate_kernel(float* __restrict__ sum, const float* __restrict__ frame, float* __restrict__ mean, unsigned char* __restrict__ rgb8,
                                  size_t values, int first_frame, float inv_frames)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= values) return;
    const float acc = first_frame ? frame[i] : sum[i] + frame[i];
    sum[i] = acc;
    const float m = acc * inv_frames;
    if (mean) mean[i] = m;
    if (rgb8) rgb8[i] = to_u8(m);
}

// Strip de-interleave after the framebuffer gather: src = parts' compact row blocks back to back, dst = image order.
__global__ void deinterleave_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, int width, int height,
                                    int strip_rows, int num_parts, int elem_bytes)
{
    const size_t row_bytes = (size_t)width * (size_t)elem_bytes;
    const int y = blockIdx.y;
    if (y >= height) return;
    const int strip = y / strip_rows, part = strip % num_parts, local_strip = strip / num_parts;
    // rows owned by parts before `part`
    size_t rows_before = 0;
    const int nstrips = (height + strip_rows - 1) / strip_rows;
    for (int q = 0; q < part; ++q) {
        const int owned = (nstrips - q + num_parts - 1) / num_parts; // strips q, q+P, ...
        size_t rows = (size_t)owned * (size_t)strip_rows;
        // the last strip of the image may be short
        const int last = nstrips - 1;
        if (owned > 0 && last % num_parts == q) rows -= (size_t)(nstrips * strip_rows - height);
        rows_before += rows;
    }
    const size_t local_row = (size_t)local_strip * (size_t)strip_rows + (size_t)(y - strip * strip_rows);
    const unsigned char* s = src + (rows_before + local_row) * row_bytes;
    unsigned char* d = dst + (size_t)y * row_bytes;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < row_bytes; i += (size_t)gridDim.x * blockDim.x) d[i] = s[i];
}

// Multi-GPU gather, last step (ff_dist.cpp): `src` holds every part's packed strips, part after part, each part as
// [rows x width float3 radiance][rows x width rgb8], both sections padded to 16 bytes; one pass scatters all rows of both
// framebuffers to image order.  Row y belongs to strip y / strip_rows, which part (strip % num_parts) rendered as its
// local strip strip / num_parts.
__global__ void unpack_strips_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ rgb8, float* __restrict__ radiance, int width,
                                     int height, int strip_rows, int num_parts)
{
    const int y = blockIdx.y;
    if (y >= height) return;
    const int nstrips = (height + strip_rows - 1) / strip_rows;
    const int strip = y / strip_rows, part = strip % num_parts, local_strip = strip / num_parts;
    auto part_rows = [&](int q) {
        const int owned = (nstrips - q + num_parts - 1) / num_parts; // strips q, q + P, ...
        size_t rows = (size_t)owned * (size_t)strip_rows;
        if (owned > 0 && (nstrips - 1) % num_parts == q) rows -= (size_t)(nstrips * strip_rows - height); // the image's last strip may be short
        return rows;
    };
    auto pad16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    size_t base = 0;
    for (int q = 0; q < part; ++q) base += pad16(part_rows(q) * (size_t)width * 12) + pad16(part_rows(q) * (size_t)width * 3);
    const size_t rows = part_rows(part);
    const size_t local_row = (size_t)local_strip * (size_t)strip_rows + (size_t)(y - strip * strip_rows);
    const size_t stride = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (radiance) {
        const float* s = reinterpret_cast<const float*>(src + base) + local_row * (size_t)width * 3;
        float* d = radiance + (size_t)y * (size_t)width * 3;
        for (size_t i = first; i < (size_t)width * 3; i += stride) d[i] = s[i];
    }
    if (rgb8) {
        const unsigned char* s = src + base + pad16(rows * (size_t)width * 12) + local_row * (size_t)width * 3;
        unsigned char* d = rgb8 + (size_t)y * (size_t)width * 3;
        for (size_t i = first; i < (size_t)width * 3; i += stride) d[i] = s[i];
    }
}

// The normal tables of the scene (KParams::tri_world_normals / geom_world_normals): what the shading pass computes per hit -
// fill_object_normal and unit_world_normal, the functions it calls, on the records it reads - once per triangle record and per
// geometry record.  One row of workgroups per geometry (blockIdx.y); an analytic record's one entry is written by its first thread.
__global__ void world_normals_kernel(const GeomRecord* __restrict__ geoms, const TriRecord* __restrict__ tris, float4* __restrict__ tri_out,
                                     float4* __restrict__ geom_out)
{
    const int g = (int)blockIdx.y;
    const GeomRecord& G = geoms[g];
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool mesh = G.type == FF_GEOM_TRIANGLEMESH;
    if (mesh ? i >= (unsigned)G.tri_count : i != 0u) return;
    Best best;
    best.dist = 0.f;
    best.geom = g;
    best.rec = mesh ? G.tri_first + (int)i : -1;
    best.px = best.py = best.pz = 0.f;
    fill_object_normal(geoms, tris, best);
    MaterialRef M;
    M.global = &G;
    M.geom_base = 0;
    M.g = g;
    float ux, uy, uz;
    unit_world_normal(M, best, ux, uy, uz);
    if (mesh) tri_out[best.rec] = make_float4(ux, uy, uz, 0.f);
    else geom_out[g] = make_float4(ux, uy, uz, 0.f);
}
} // namespace

hipError_t launch_world_normals(const GeomRecord* geoms, const TriRecord* tris, int num_geoms, int max_tri_count, float4* tri_out, float4* geom_out,
                                hipStream_t stream)
{
    if (num_geoms <= 0) return hipSuccess;
    const dim3 block(256), grid((unsigned)(((max_tri_count > 1 ? max_tri_count : 1) + 255) / 256), (unsigned)num_geoms);
    hipLaunchKernelGGL(world_normals_kernel, grid, block, 0, stream, geoms, tris, tri_out, geom_out);
    return hipGetLastError();
}

hipError_t launch_combine(const KParams& p, hipStream_t stream)
{
    if (p.local_width <= 0 || p.local_rows <= 0) return hipSuccess;
    const dim3 block(256), grid((p.local_width + 255) / 256, p.local_rows);
    hipLaunchKernelGGL(combine_kernel, grid, block, 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_cull_mask(const KParams& p, unsigned long long* mask, hipStream_t stream)
{
    if (p.pix_items == 0) return hipSuccess;
    hipLaunchKernelGGL(cull_mask_kernel, dim3((p.pix_items + 255) / 256), dim3(256), 0, stream, p, mask);
    return hipGetLastError();
}

hipError_t launch_ieee_check(unsigned long long* mismatches2, hipStream_t stream)
{
    hipLaunchKernelGGL(ieee_check_kernel, dim3(256 * 8), dim3(256), 0, stream, mismatches2);
    return hipGetLastError();
}

hipError_t launch_accumulate(float* sum, const float* frame, float* mean, unsigned char* rgb8, size_t values, int first_frame, float inv_frames,
                             hipStream_t stream)
{
    if (values == 0) return hipSuccess;
    hipLaunchKernelGGL(accumulate_kernel, dim3((unsigned)((values + 255) / 256)), dim3(256), 0, stream, sum, frame, mean, rgb8, values, first_frame,
                       inv_frames);
    return hipGetLastError();
}

hipError_t launch_deinterleave(const void* src, void* dst, int width, int height, int strip_rows, int num_parts, int elem_bytes,
                               hipStream_t stream)
{
    if (width <= 0 || height <= 0) return hipSuccess;
    const dim3 grid(4, height), block(256);
    hipLaunchKernelGGL(deinterleave_kernel, grid, block, 0, stream, (const unsigned char*)src, (unsigned char*)dst, width, height,
                       strip_rows, num_parts, elem_bytes);
    return hipGetLastError();
}

hipError_t launch_unpack_strips(const void* src, unsigned char* rgb8, float* radiance, int width, int height, int strip_rows, int num_parts,
                                hipStream_t stream)
{
    if (width <= 0 || height <= 0 || (!rgb8 && !radiance)) return hipSuccess;
    const dim3 grid(std::max(1, std::min(8, (width * 3 + 255) / 256)), height), block(256);
    hipLaunchKernelGGL(unpack_strips_kernel, grid, block, 0, stream, (const unsigned char*)src, rgb8, radiance, width, height, strip_rows, num_parts);
    return hipGetLastError();
}

} // namespace ff
