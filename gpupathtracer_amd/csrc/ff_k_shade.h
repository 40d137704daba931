// ff_k_shade.h — device code of the trace kernels: materials, Philox, paths, the work queue, settle_hit / scatter / shade_and_advance.
#pragma once
#include "ff_k_lds.h"

namespace ff {
namespace {

// ---- shading --------------------------------------------------------------------------------------------------------

// What shading needs from the hit geometry's record, fetched piece by piece when it is used (loading the whole record up
// front costs ~25 registers at the kernel's pressure peak).  BVH kernels read the LDS copy, brute-force kernels the
// global one.
struct MaterialRef {
    const GeomRecord* global; // non-null: read the global record
    int geom_base;            // else: the LDS copy (uint4 index of record 0, Lds::geom_base)
    int g;
};

__device__ __forceinline__ float4 mat_f4(const MaterialRef& M, int k)
{
    if (M.global) return reinterpret_cast<const float4*>(M.global)[k];
    return reinterpret_cast<const float4*>(ff_smem)[M.geom_base + M.g * kGeomVec4 + k];
}
__device__ __forceinline__ int mat_bxdf(const MaterialRef& M)
{
    if (M.global) return M.global->bxdf_type;
    return reinterpret_cast<const int4*>(ff_smem)[M.geom_base + M.g * kGeomVec4 + 16].y;
}

// `unit_object_normal`: normalise a triangle's face normal in object space first (kernel.cu:101, what Intersect::m_normal
// and the NORMAL_DEBUG shade carry); the path integrator transforms the raw cross product and normalises once in world space.
// WN: the instantiation of the caller (trace_bvh_kernel<..., WN>).  The kernels on the normal tables keep a plane's unit world normal in
// quarter 8 of its LDS record - the first of the columns read here - so nothing in them may come this way: it does not compile.
template <bool WN = false>
__device__ __forceinline__ void world_normal(const MaterialRef& M, const Best& best, bool unit_object_normal, float& nx, float& ny, float& nz)
{
    static_assert(!WN, "the kernels on the normal tables overwrite the inverse-transpose in LDS: take the normal from Best::cx, cy, cz");
    float ox = best.cx, oy = best.cy, oz = best.cz;
    if (best.rec >= 0 && unit_object_normal) {
        const float inv = ieee_rcp(ieee_sqrt(dot3(ox, oy, oz, ox, oy, oz)));
        ox = ox * inv;
        oy = oy * inv;
        oz = oz * inv;
    }
    const float4 n0 = mat_f4(M, 8), n1 = mat_f4(M, 9), n2 = mat_f4(M, 10); // inverse-transpose columns (w = column3 * 0)
    nx = (n0.x * ox + n1.x * oy) + (n2.x * oz + n0.w);
    ny = (n0.y * ox + n1.y * oy) + (n2.y * oz + n1.w);
    nz = (n0.z * ox + n1.z * oy) + (n2.z * oz + n2.w);
}

// The unit world normal of a hit before the flip against the ray: the object-space normal as found (Best::cx, cy, cz - a triangle's
// raw cross product, a plane's m_normal) through the record's inverse-transpose, normalised once in world space.  A function of the
// scene alone: the shading passes evaluate it per hit, world_normals_kernel (ff_frame_kernels.hip) once per triangle and plane -
// the same operations in the same order, so the stored bits are the bits computed here (a zero-area triangle's NaN included).
template <bool WN = false>
__device__ __forceinline__ void unit_world_normal(const MaterialRef& M, const Best& best, float& ux, float& uy, float& uz)
{
    float nx, ny, nz;
    world_normal<WN>(M, best, false, nx, ny, nz);
    const float ninv = ieee_rcp(ieee_sqrt(dot3(nx, ny, nz, nx, ny, nz)));
    ux = nx * ninv;
    uy = ny * ninv;
    uz = nz * ninv;
}

// ---- build-defined integrator pieces (DESIGN.md "Integrator"; mirrored by the oracle) ------------------------------

// Philox2x32-10 (Salmon et al., SC'11): counter-based, so a sample's random numbers depend only on
// (global pixel index, sample, bounce, seed) and not on which lane, wave, launch or GPU computes it.
__device__ __forceinline__ void philox2x32_10(unsigned c0, unsigned c1, unsigned key, unsigned& o0, unsigned& o1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r > 0) key += 0x9E3779B9u;
        const unsigned long long prod = (unsigned long long)c0 * 0xD256D193ull; // one v_mad_u64_u32 yields both halves
        c0 = (unsigned)(prod >> 32) ^ key ^ c1;
        c1 = (unsigned)prod;
    }
    o0 = c0;
    o1 = c1;
}

// utilities.h:46-55 CosineSampleHemisphere with theta = 2*pi*k24/2^24 reduced exactly to an octant on the integer and
// fixed-order polynomials on [0, pi/4] (bit-identical to the oracle).
__device__ __forceinline__ void cosine_sample(float u1, unsigned k24, float& x, float& y, float& z)
{
    const unsigned oct = k24 >> 21, f = k24 & 0x1FFFFFu;
    const unsigned m = (oct & 1u) ? (0x200000u - f) : f;
    const float a = (float)m * 3.7450704e-07f;
    const float a2 = a * a;
    float sp = -1.9841270e-04f + a2 * 2.7557319e-06f;
    sp = 8.3333333e-03f + a2 * sp;
    sp = -1.6666667e-01f + a2 * sp;
    const float s = a + (a * a2) * sp;
    float cp = -1.3888889e-03f + a2 * 2.4801587e-05f;
    cp = 4.1666667e-02f + a2 * cp;
    cp = -0.5f + a2 * cp;
    const float c = 1.0f + a2 * cp;
    float sn, cs;
    if ((oct + 1u) & 2u) { sn = c; cs = s; } else { sn = s; cs = c; }
    if (oct >= 4u) sn = -sn;
    if (oct >= 2u && oct <= 5u) cs = -cs;
    const float r = ieee_sqrt(u1);
    x = r * cs;
    y = r * sn;
    z = ieee_sqrt(fmaxf(0.0f, 1.0f - u1));
}

__device__ __forceinline__ unsigned char to_u8(float v)
{
    // kernel.cu:214 float -> unsigned char (truncation); out-of-range values are UB there and clamp here
    const float s = v * 255.0f;
    if (!(s > 0.0f)) return 0;
    if (s >= 255.0f) return 255;
    return (unsigned char)s;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
    unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned olo = __shfl_xor(lo, off), ohi = __shfl_xor(hi, off);
        const unsigned long long s = (((unsigned long long)hi << 32) | lo) + (((unsigned long long)ohi << 32) | olo);
        lo = (unsigned)s;
        hi = (unsigned)(s >> 32);
    }
    return ((unsigned long long)hi << 32) | lo;
}

// Per-lane path state.
struct Path {
    int item;      // pitem | block << 25 (the pixel's tile-major item number and the sample block whose sum this lane keeps: blocksums[pitem][block]);
                   // negative (kItemTail | pitem): a tail item, whose samples are stored one by one (tail_samples[sample of the block][pitem])
    int send;      // one past the last sample of the block
    unsigned gxy;  // global pixel coordinates x | y << 16; the RNG counter is the pixel index y*W+x (kernel.cu:191)
    int s, b;      // current sample / segment
    float pdx, pdy, pdz; // primary direction of the pixel (every sample starts with the same ray: kernel.cu:200-205 has no jitter)
    Ray ray;       // current world-space ray
    float bx, by, bz; // throughput
    float ax, ay, az; // running sum over samples
};

// kernel.cu:197-205 for global pixel (x, y): origin = camera position, direction through the pixel corner.
__device__ __forceinline__ void primary_ray(const KParams& p, unsigned gxy, Ray& ray)
{
    const int x = (int)(gxy & 0xFFFFu), y = (int)(gxy >> 16);
    const float Px = ((float)x / p.screen_w) * 2.f - 1.f;  // :200
    const float Py = 1.f - ((float)y / p.screen_h) * 2.f;  // :201
    const float v0 = Px * p.far_clip, v1 = Py * p.far_clip, v2 = 1.f * p.far_clip, v3 = 1.f * p.far_clip;
    const float wx = (p.cam_c0[0] * v0 + p.cam_c1[0] * v1) + (p.cam_c2[0] * v2 + p.cam_c3[0] * v3); // :203
    const float wy = (p.cam_c0[1] * v0 + p.cam_c1[1] * v1) + (p.cam_c2[1] * v2 + p.cam_c3[1] * v3);
    const float wz = (p.cam_c0[2] * v0 + p.cam_c1[2] * v1) + (p.cam_c2[2] * v2 + p.cam_c3[2] * v3);
    const float ddx = wx - p.cam_pos[0], ddy = wy - p.cam_pos[1], ddz = wz - p.cam_pos[2];
    const float inv = ieee_rcp(ieee_sqrt(dot3(ddx, ddy, ddz, ddx, ddy, ddz))); // :205
    ray.ox = p.cam_pos[0];
    ray.oy = p.cam_pos[1];
    ray.oz = p.cam_pos[2];
    ray.dx = ddx * inv;
    ray.dy = ddy * inv;
    ray.dz = ddz * inv;
}

__device__ __forceinline__ void start_sample(const KParams& p, Path& P)
{
    P.b = 0;
    P.ray.ox = p.cam_pos[0];
    P.ray.oy = p.cam_pos[1];
    P.ray.oz = p.cam_pos[2];
    P.ray.dx = P.pdx;
    P.ray.dy = P.pdy;
    P.ray.dz = P.pdz;
    P.bx = P.by = P.bz = 1.f;
}

// The part of the work queue a wave owns: items [next, end).  Wave-uniform (scalar registers).
struct WaveQueue {
    unsigned next, end; // in the counter's own numbering (see queue_item)
    unsigned counter;   // which counter the wave draws from
    unsigned owned;     // how many items that counter owns
    unsigned main_end;  // its items [0, main_end) go out in chunks, the last ones [main_end, owned) exactly as asked for (acquire_pixel)
    bool in_tail;       // the chunked part has run dry: the wave draws from the tail counter
    bool dry;           // nothing left at all
};

// The launch's items are dealt to the counters in stripes of kQueueStripe: counter c of n owns the stripes c, c + n, ... so
// every counter covers the whole image evenly and they run dry together.  Number v of counter c is this item:
__device__ __forceinline__ unsigned queue_item(const KParams& p, const WaveQueue& Q, unsigned v)
{
    return ((v / kQueueStripe) * (unsigned)p.queue_counters + Q.counter) * kQueueStripe + (v % kQueueStripe);
}

__device__ __forceinline__ WaveQueue make_wave_queue(const KParams& p)
{
    WaveQueue Q;
    const unsigned n = (unsigned)p.queue_counters, c = blockIdx.x % n;
    const unsigned stripes = (p.total_items + kQueueStripe - 1) / kQueueStripe;
    const unsigned mine = stripes > c ? (stripes - c + n - 1) / n : 0u;
    // the last stripe of the range may be short
    const unsigned cut = mine > 0u && (stripes - 1u) % n == c ? stripes * kQueueStripe - p.total_items : 0u;
    Q.next = Q.end = 0u;
    Q.counter = c;
    Q.owned = mine * kQueueStripe - cut;
    Q.main_end = Q.owned - min(Q.owned, p.queue_tail_items);
    Q.in_tail = Q.main_end == 0u;
    Q.dry = Q.owned == 0u;
    return Q;
}

// Pull the next traceable pixel for every calling lane.  Two levels: a wave takes a CHUNK of consecutive items from the global
// counter (one atomic: what its idle lanes ask for, at least queue_chunk items) and deals them to its lanes with no memory
// traffic; what is left over serves the wave's next requests.  One counter serves about 10^8 atomics a second, each waiting
// behind the others': a wave asking it for every item held 1-spp frames (two million one-path items) to a third of the
// saturated rate.  So the launch spreads its waves over several counters in different memory channels (queue_item: each owns
// an even share of the image; no stealing: they run dry together), and queue_chunk is sized by the host so that a chunk is a
// few dozen samples of work, whatever the item length.  (Chunks that shrink with what is left - guided self-scheduling, up to a
// tile of pixels per wave - were measured: the big early chunks unbalance frames whose cost varies across the image, the
// reference's default camera 191 ms instead of 84.)
// Called by ALL lanes of the wave (Q must stay wave-uniform); `need` marks the lanes that want a pixel.  Returns false for lanes
// that did not ask or saw the end of the queue.
// START (trace_bvh_kernel on start records): a pixel whose path ends at its first hit (kStartEnds) never reaches the caller - its
// item is answered here from the record's constant radiance, its rays counted (`answered`: wave-uniform, like Counters::reused).
template <bool START = false>
__device__ __forceinline__ bool acquire_pixel(const KParams& p, int lane, Path& P, WaveQueue& Q, bool need, unsigned& rays, unsigned* answered = nullptr)
{
    bool got = false, exhausted = !need;
    unsigned ended = 0u; // START: samples of kStartEnds items this lane answered
    for (;;) {
        const bool want = !got && !exhausted;
        const unsigned long long m = __ballot(want);
        if (m == 0ull) break;
        if (Q.next >= Q.end) {
            if (Q.dry) {
                exhausted = true;
                continue;
            }
            const int leader = __ffsll((long long)m) - 1;
            if (!Q.in_tail) {
                const unsigned size = max((unsigned)__popcll(m), p.queue_chunk);
                unsigned base = 0u;
                if (lane == leader) base = atomicAdd(p.queue + Q.counter * kQueueStride, size);
                base = (unsigned)__builtin_amdgcn_readlane((int)base, leader);
                if (base < Q.main_end) {
                    Q.next = base;
                    Q.end = min(base + size, Q.main_end);
                } else {
                    Q.in_tail = true;
                }
            }
            if (Q.in_tail && Q.next >= Q.end) {
                // The LAST items of the counter's share are handed out exactly as asked for, from a counter of their own.  A chunk is
                // the wave's private stock: it deals it to its own lanes as they fall idle, and a wave that takes 64 sample blocks when
                // two of its lanes are idle works through the other 62 long after every other wave has run dry - the launch's dry end
                // (an eighth of a multi-GPU rank's frame; 40 % of a 1-spp frame: tools/timeline_probe.py).  In the tail zone a wave holds
                // nothing it has no lane for.
                const unsigned size = (unsigned)__popcll(m);
                unsigned base = 0u;
                if (lane == leader) base = atomicAdd(p.queue + Q.counter * kQueueStride + kQueueTailWord, size);
                base = (unsigned)__builtin_amdgcn_readlane((int)base, leader);
                if (Q.main_end + base >= Q.owned) {
                    Q.dry = true;
                    Q.next = Q.end = Q.owned;
                    continue;
                }
                Q.next = Q.main_end + base;
                Q.end = min(Q.next + size, Q.owned);
            }
        }
        const unsigned rank = (unsigned)__popcll(m & ((1ull << lane) - 1ull));
        const unsigned avail = Q.end - Q.next, asked = (unsigned)__popcll(m);
        const bool take = want && rank < avail;
        const unsigned item = queue_item(p, Q, Q.next + rank);
        Q.next += min(asked, avail);
        if (take) {
            {
                // an item is one sample block of one pixel; pixels walk 8x8 tiles of the local image (padding items and
                // untraced pixels are consumed and skipped)
                // items [0, tail_first_item): (pixel, whole block), PIXEL-major: a wave's chunk covers the blocks of one or a few
                // pixels, whose sums are neighbours in blocksums[pixel][block]: stored by one wave, they meet in one XCD's L2
                // and leave it as whole lines instead of one masked 64-byte write per 16-byte sum (0.59 instead of 1.93 GB of
                // HBM writes per 1080p 1 024-spp frame); beyond: (pixel, sample group) of the tail block, group-major
                const bool tail = p.tail_block >= 0 && item >= p.tail_first_item;
                const unsigned rel = tail ? item - p.tail_first_item : item;
                unsigned blk, pitem; // tail: blk is the group index
                // (Five divisions by launch constants per item.  Host-computed magic multipliers - mulhi, two shifts, two adds each -
                // were measured: C2 -0.6 %, C3 -1.5 %, the 1-spp frame +-0: v_mul_hi_u32 is a quarter-rate instruction and the compiler's
                // reciprocal-based expansion is not slower.)
                if (tail) {
                    blk = rel / p.pix_items;
                    pitem = rel - blk * p.pix_items;
                } else {
                    pitem = rel / p.whole_blocks;
                    blk = rel - pitem * p.whole_blocks;
                }
                // A camera outside the scene (the reference's default one looks at its box from 12.5 units away: 96 % of the frame is
                // background): cull_mask_kernel has marked the pixels whose primary ray misses the padded box around ALL geometries
                // and zeroed their block sums - kernel.cu:200-205 has no jitter, every sample of the pixel starts with that ray.
                // Their items end here: the rays are counted (each is a closest-hit query with the answer "nothing", as in the
                // brute-force loop, which takes no such shortcut) and the lane asks for the next item.
                if (p.cull_mask != nullptr && !tail && ((p.cull_mask[pitem >> 6] >> (pitem & 63u)) & 1ull) != 0ull) {
                    const int s0 = (p.block_begin + (int)blk) * p.block_spp;
                    rays += (unsigned)(p.shade_mode == FF_SHADE_NORMAL_DEBUG ? 1 : min(p.spp_total, s0 + p.block_spp) - s0);
                    continue;
                }
                const int tile = (int)(pitem >> 6), in = (int)(pitem & 63u);
                const int lx = (tile % p.tiles_per_row) * 8 + (in & 7);
                const int ly = (tile / p.tiles_per_row) * 8 + (in >> 3);
                const int strip = ly / p.strip_rows;
                const int gy = p.y0 + (strip * p.num_parts + p.part) * p.strip_rows + (ly - strip * p.strip_rows);
                const int gx = p.x0 + lx;
                if (lx < p.local_width && gx < p.xlim && ly < p.local_rows && gy < p.ylim) {
                    if constexpr (START) {
                        if (((unsigned)__float_as_int(p.start_records[pitem].w) >> kStartClassShift) == kStartEnds) {
                            // Every sample of this pixel ends at the first hit with the same radiance (an emitter, nothing, a one-bounce
                            // frame): the item is the sum a lane would have kept - n sequential additions from zero - or, for a tail
                            // item, the constant stored per sample.  Each sample is a path segment answered without a traversal.
                            const float4 l = p.start_records[p.pix_items + pitem];
                            int n;
                            if (tail) {
                                const int s0 = p.tail_block * p.block_spp + p.tail_start[blk];
                                n = min(p.spp_total, p.tail_block * p.block_spp + p.tail_start[blk + 1]) - s0;
                                for (int i = 0; i < n; ++i) p.tail_samples[(size_t)(p.tail_start[blk] + i) * p.pix_items + pitem] = make_float4(l.x, l.y, l.z, 0.f);
                            } else {
                                const int block = p.block_begin + (int)blk;
                                n = min(p.spp_total, (block + 1) * p.block_spp) - block * p.block_spp;
                                float ax = 0.f, ay = 0.f, az = 0.f;
                                for (int i = 0; i < n; ++i) {
                                    ax = ax + l.x;
                                    ay = ay + l.y;
                                    az = az + l.z;
                                }
                                p.blocksums[(size_t)pitem * p.num_blocks + block] = make_float4(ax, ay, az, 0.f);
                            }
                            rays += (unsigned)max(n, 0);
                            ended += (unsigned)max(n, 0);
                            continue;
                        }
                    }
                    got = true;
                    P.gxy = (unsigned)gx | ((unsigned)gy << 16);
                    if (tail) {
                        const int first = p.tail_start[blk], past = p.tail_start[blk + 1]; // the group's samples inside the block
                        P.item = (int)(kItemTail | pitem);
                        P.s = p.tail_block * p.block_spp + first;
                        P.send = min(p.spp_total, p.tail_block * p.block_spp + past);
                    } else {
                        const int block = p.block_begin + (int)blk;
                        P.item = (int)(((unsigned)block << kItemBlockShift) | pitem);
                        P.s = block * p.block_spp;
                        P.send = min(p.spp_total, P.s + p.block_spp);
                    }
                    P.ax = P.ay = P.az = 0.f;
                    if constexpr (!START) { // (a start record holds what the primary ray was needed for)
                        primary_ray(p, P.gxy, P.ray); // once per (pixel, block); its samples reuse the direction
                        P.pdx = P.ray.dx;
                        P.pdy = P.ray.dy;
                        P.pdz = P.ray.dz;
                    }
                    start_sample(p, P);
                    // A camera outside the scene (the reference's default one looks at its box from 12.5 units away: 96 % of the
                    // frame is background): a pixel whose primary ray misses the padded box around ALL geometries has no hit in any
                    // sample - kernel.cu:200-205 has no jitter, every sample starts with the same ray - so the whole item is a sum of
                    // zeros.  It is written at once, its rays are counted (each is a closest-hit query with the answer "nothing", as
                    // in the brute-force loop, which takes no such shortcut), and the lane asks for the next item.
                }
            }
        }
    }
    if constexpr (START) {
        if (__ballot(ended != 0u) != 0ull) *answered += (unsigned)wave_sum((unsigned long long)ended);
    }
    return got;
}

// Shading comes in two steps so that the trace kernel can run the expensive one once per iteration (trace_bvh_kernel):
//   settle_hit: what the finished segment means for the path - it ends (on an emitter, on nothing, at the last bounce; the sample's
//     radiance goes to the block sum and the next sample or the end of the block follows) or it goes on from this hit;
//   scatter:    the next ray of a path that goes on (normal, random numbers, new direction).
// settle_hit returns kPixelDone (the lane gives the pixel up), kNewSample (the next sample's primary ray is in P.ray) or kGoesOn
// (scatter must follow with the same hit).  SPECULAR = false: the caller guarantees a scene without MIRROR / GLASS surfaces.
enum { kPixelDone = 0, kNewSample = 1, kGoesOn = 2 };
template <bool SPECULAR = true, bool PREPASS = false, bool WN = false>
__device__ __forceinline__ int settle_hit(const KParams& p, const Best& best, bool hit, const MaterialRef& M, Path& P)
{
    if constexpr (PREPASS) {
        // The pre-pass of a frame: every pixel's primary ray, traced ONCE (kernel.cu:200-205 sends all samples of a pixel through the
        // pixel's corner: no jitter), its closest hit stored per pixel; the frame's samples start from there (trace_bvh_kernel).
        float4* out = p.primary_hits + ((unsigned)P.item & kItemPixelMask);
        out[0] = make_float4(best.dist, best.px, best.py, best.pz);
        out[p.pix_items] = make_float4(best.cx, best.cy, best.cz, __int_as_float(hit ? best.geom : -1));
        out[2 * (size_t)p.pix_items] = make_float4(__int_as_float(best.rec), 0.f, 0.f, 0.f);
        if (p.start_records != nullptr) {
            // ... and the start record: what settle_hit and scatter below compute from this hit for EVERY sample of the pixel, computed
            // once - the same operations in the same order on the same operands (the throughput is 1, the direction the primary ray's).
            unsigned cls = kStartEnds;
            float4 q0 = make_float4(0.f, 0.f, 0.f, 0.f), q1 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (hit) {
                const int bxdf = mat_bxdf(M);
                if (bxdf == FF_BXDF_EMITTER) {
                    const float4 emission = mat_f4(M, 13);
                    q1.x = 0.f + P.bx * emission.x;
                    q1.y = 0.f + P.by * emission.y;
                    q1.z = 0.f + P.bz * emission.z;
                } else if (SPECULAR && (bxdf == FF_BXDF_MIRROR || bxdf == FF_BXDF_GLASS)) {
                    cls = kStartGeneral;
                } else if (p.start_bounces > 1) {
                    cls = kStartGoesOn;
                    float ux, uy, uz;
                    unit_world_normal(M, best, ux, uy, uz);
                    if (dot3(ux, uy, uz, P.ray.dx, P.ray.dy, P.ray.dz) > 0.0f) { ux = -ux; uy = -uy; uz = -uz; }
                    q0.x = best.px + ux * kRayEps;
                    q0.y = best.py + uy * kRayEps;
                    q0.z = best.pz + uz * kRayEps;
                    q1.x = ux; q1.y = uy; q1.z = uz;
                }
            }
            q0.w = __int_as_float((int)((cls << kStartClassShift) | ((unsigned)(hit ? best.geom : 0) & kStartGeomMask)));
            float4* rec = p.start_records + ((unsigned)P.item & kItemPixelMask);
            rec[0] = q0;
            rec[p.pix_items] = q1;
        }
        if (!hit && p.cull_mask_out != nullptr) {
            // Nothing in view: every sample of the pixel adds zero.  Its bit goes into the mask the work queue consults (acquire_pixel:
            // its whole-block items are dropped when they are decoded, their rays counted), its block sums are zeroed and it is counted -
            // exactly what cull_mask_kernel does for the pixels whose ray misses the box around the scene, for those that miss the
            // scene itself (a pixel that pass has marked already is left alone).
            const unsigned pitem = (unsigned)P.item & kItemPixelMask;
            const unsigned long long bit = 1ull << (pitem & 63u);
            const unsigned long long old = atomicOr(&p.cull_mask_out[pitem >> 6], bit);
            if ((old & bit) == 0ull) {
                for (int b = 0; b < p.frame_blocks; ++b) p.blocksums[(size_t)pitem * p.frame_blocks + b] = make_float4(0.f, 0.f, 0.f, 0.f);
                atomicAdd(&p.counters[kCulledPixelsWord + kRaySlotStride * ((pitem >> 6) % kRaySlots)], 1ull);
            }
        }
        return kPixelDone;
    }
    // (WN: the kernels that carry the unit world normal in `best` run path frames only; the reference's own shade wants the object-space one)
    const bool debug_shade = !WN && p.shade_mode == FF_SHADE_NORMAL_DEBUG;
    // Radiance of the path: it is zero until the path ends on an emitter (the only light transport here), so it is not
    // carried across segments; "0 + beta*Le" of the integrator is beta*Le bit for bit.
    float Lx = 0.f, Ly = 0.f, Lz = 0.f;
    if (hit) {
        if (debug_shade) {
            // shade(), kernel.cu:178-184
            if constexpr (!WN) {
                float nx, ny, nz;
                world_normal<WN>(M, best, true, nx, ny, nz);
                Lx = fabsf(nx); Ly = fabsf(ny); Lz = fabsf(nz);
            }
        } else if (mat_bxdf(M) == FF_BXDF_EMITTER) {
            // utilities.h:96-103: two-sided emitter, m_emissiveColor * m_intensity
            const float4 emission = mat_f4(M, 13);
            Lx = 0.f + P.bx * emission.x;
            Ly = 0.f + P.by * emission.y;
            Lz = 0.f + P.bz * emission.z;
        } else {
            // MIRROR: throughput *= m_specularColor (the record's tint slot holds it).  GLASS: the tint depends on the choice between
            // reflection and refraction (scatter).  Everything else is diffuse (utilities.h:109): cosine-weighted sampling, so
            // f*cos/pdf = albedo.
            const bool glass = SPECULAR && mat_bxdf(M) == FF_BXDF_GLASS;
            const float4 albedo = mat_f4(M, 12);
            if (!glass) {
                P.bx = P.bx * albedo.x;
                P.by = P.by * albedo.y;
                P.bz = P.bz * albedo.z;
            }
            if (P.b != p.bounces - 1) return kGoesOn;
        }
    }
    if (P.item < 0) {
        // tail item: every sample is stored on its own (sample-major: [sample of the block][pixel item]); the combine pass adds the
        // block's samples in order
        p.tail_samples[(size_t)(P.s - p.tail_block * p.block_spp) * p.pix_items + ((unsigned)P.item & kItemPixelMask)] = make_float4(Lx, Ly, Lz, 0.f);
    } else {
        P.ax = P.ax + Lx;
        P.ay = P.ay + Ly;
        P.az = P.az + Lz;
    }
    ++P.s;
    if (P.s < P.send && !debug_shade) {
        start_sample(p, P);
        return kNewSample;
    }
    // sample block finished: its sum goes to the block buffer (the combine kernel adds a pixel's blocks in order)
    if (P.item >= 0) p.blocksums[(size_t)((unsigned)P.item & kItemPixelMask) * p.num_blocks + ((unsigned)P.item >> kItemBlockShift)] = make_float4(P.ax, P.ay, P.az, 0.f);
    return kPixelDone;
}

// The two halves of a diffuse bounce: the cosine-weighted direction about +z from the sample's random numbers (they depend only on
// pixel, sample, segment and seed), and that direction carried into the orthonormal basis about the unit normal u.
__device__ __forceinline__ void diffuse_local_direction(const KParams& p, const Path& P, float& wlx, float& wly, float& wlz)
{
    unsigned r0, r1;
    const unsigned gpix = (P.gxy >> 16) * (unsigned)p.width + (P.gxy & 0xFFFFu);
    philox2x32_10(gpix, ((unsigned)P.s << 8) | ((unsigned)P.b & 0xFFu), p.key, r0, r1);
    const float u1 = (float)(r0 >> 8) * 5.9604644775390625e-08f;
    cosine_sample(u1, r1 >> 8, wlx, wly, wlz);
}
__device__ __forceinline__ void to_world_about(float ux, float uy, float uz, float wlx, float wly, float wlz, float& wox, float& woy, float& woz)
{
    // orthonormal basis (Duff et al. 2017)
    const float sign = copysignf(1.0f, uz);
    const float aa = -ieee_rcp(sign + uz); // -1 / x == -(1 / x)
    const float bb = (ux * uy) * aa;
    const float t0 = 1.0f + ((sign * ux) * ux) * aa, t1 = sign * bb, t2 = -sign * ux;
    const float s0 = bb, s1 = sign + (uy * uy) * aa, s2 = -uy;
    wox = (t0 * wlx + s0 * wly) + ux * wlz;
    woy = (t1 * wlx + s1 * wly) + uy * wlz;
    woz = (t2 * wlx + s2 * wly) + uz * wlz;
}

// The next ray of a path that goes on from `best` (settle_hit returned kGoesOn; the throughput already carries the surface's
// albedo, glass excepted).  MIRROR: perfect reflection.  GLASS: smooth dielectric, Fresnel-weighted choice between reflection and
// refraction (oracle/ff_oracle.c is the definition).  Everything else: cosine-weighted direction about the world normal.
// WN (diffuse small-scene kernels on the scene's normal tables): best.cx, cy, cz hold the unit world normal already (finish_segment).
template <bool SPECULAR = true, bool WN = false>
__device__ __forceinline__ void scatter(const KParams& p, const Best& best, const MaterialRef& M, Path& P)
{
    float ux = best.cx, uy = best.cy, uz = best.cz;
    if constexpr (!WN) unit_world_normal<WN>(M, best, ux, uy, uz);
    const int bxdf = mat_bxdf(M);
    const bool mirror = SPECULAR && bxdf == FF_BXDF_MIRROR, glass = SPECULAR && bxdf == FF_BXDF_GLASS;
    const float4 albedo = mat_f4(M, 12);
    bool flipped = false;
    if (dot3(ux, uy, uz, P.ray.dx, P.ray.dy, P.ray.dz) > 0.0f) { ux = -ux; uy = -uy; uz = -uz; flipped = true; }
    float wox, woy, woz;
    float sx = ux, sy = uy, sz = uz; // the next ray starts on this side of the surface
    if (glass) {
        const float dx = P.ray.dx, dy = P.ray.dy, dz = P.ray.dz;
        const float ior = albedo.w;
        const float eta = flipped ? ior : ieee_rcp(ior);
        const float ci = -dot3(ux, uy, uz, dx, dy, dz);
        const float s2 = (eta * eta) * (1.0f - ci * ci);
        bool reflect = true;
        float ct = 0.f;
        if (s2 < 1.0f) {
            ct = ieee_sqrt(1.0f - s2);
            const float a = eta * ci, bq = eta * ct;
            const float rs = (a - ct) / (a + ct), rp = (ci - bq) / (ci + bq);
            const float F = 0.5f * (rs * rs + rp * rp);
            unsigned r0, r1;
            const unsigned gpix = (P.gxy >> 16) * (unsigned)p.width + (P.gxy & 0xFFFFu);
            philox2x32_10(gpix, ((unsigned)P.s << 8) | ((unsigned)P.b & 0xFFu), p.key, r0, r1);
            const float u1 = (float)(r0 >> 8) * 5.9604644775390625e-08f;
            reflect = u1 < F;
        }
        float tx, ty, tz;
        if (reflect) {
            const float k2 = 2.0f * ci;
            wox = dx + k2 * ux;
            woy = dy + k2 * uy;
            woz = dz + k2 * uz;
            tx = albedo.x; ty = albedo.y; tz = albedo.z;
        } else {
            const float k = eta * ci - ct;
            wox = eta * dx + k * ux;
            woy = eta * dy + k * uy;
            woz = eta * dz + k * uz;
            const float4 tr = mat_f4(M, 13);
            tx = tr.x; ty = tr.y; tz = tr.z;
            sx = -ux; sy = -uy; sz = -uz;
        }
        P.bx = P.bx * tx;
        P.by = P.by * ty;
        P.bz = P.bz * tz;
    } else if (mirror) {
        const float k2 = 2.0f * dot3(ux, uy, uz, P.ray.dx, P.ray.dy, P.ray.dz);
        wox = P.ray.dx - k2 * ux;
        woy = P.ray.dy - k2 * uy;
        woz = P.ray.dz - k2 * uz;
    } else {
        float wlx, wly, wlz;
        diffuse_local_direction(p, P, wlx, wly, wlz);
        to_world_about(ux, uy, uz, wlx, wly, wlz, wox, woy, woz);
    }
    P.ray.ox = best.px + sx * kRayEps;
    P.ray.oy = best.py + sy * kRayEps;
    P.ray.oz = best.pz + sz * kRayEps;
    P.ray.dx = wox; // unit local direction in an orthonormal basis: used as is (|wo| = 1 +- 1e-6)
    P.ray.dy = woy;
    P.ray.dz = woz;
    ++P.b;
}

// scatter for the kernel that runs on start records (diffuse scenes: SPECULAR = false).  Lanes in it go on either from the hit they
// just traced (settle_hit returned kGoesOn) or, `from_rec`, from their pixel's start record {q0, q1}: a new sample whose first segment
// the pre-pass answered and shaded.  For those the throughput, the normal, the flip and the origin come from the record; the random
// numbers, the cosine sample, the basis and the direction are common code.  The record's quarters are first touched behind the
// Philox rounds: the caller issued their loads just before, and the rounds cover the latency.
template <bool WN = false>
__device__ __forceinline__ void scatter_start(const KParams& p, const Best& best, MaterialRef& M, Path& P, bool from_rec, const float4& q0, const float4& q1)
{
    float ux = 0.f, uy = 0.f, uz = 1.f, ox = 0.f, oy = 0.f, oz = 0.f;
    if (!from_rec) {
        if constexpr (WN) { ux = best.cx; uy = best.cy; uz = best.cz; }
        else unit_world_normal<WN>(M, best, ux, uy, uz);
        if (dot3(ux, uy, uz, P.ray.dx, P.ray.dy, P.ray.dz) > 0.0f) { ux = -ux; uy = -uy; uz = -uz; }
        ox = best.px + ux * kRayEps;
        oy = best.py + uy * kRayEps;
        oz = best.pz + uz * kRayEps;
    }
    float wlx, wly, wlz;
    diffuse_local_direction(p, P, wlx, wly, wlz);
    if (from_rec) {
        M.g = (int)((unsigned)__float_as_int(q0.w) & kStartGeomMask);
        const float4 albedo = mat_f4(M, 12);
        P.bx = P.bx * albedo.x; // (1 * albedo: the expression settle_hit evaluates)
        P.by = P.by * albedo.y;
        P.bz = P.bz * albedo.z;
        ux = q1.x; uy = q1.y; uz = q1.z;
        ox = q0.x; oy = q0.y; oz = q0.z;
    }
    float wox, woy, woz;
    to_world_about(ux, uy, uz, wlx, wly, wlz, wox, woy, woz);
    P.ray.ox = ox;
    P.ray.oy = oy;
    P.ray.oz = oz;
    P.ray.dx = wox;
    P.ray.dy = woy;
    P.ray.dz = woz;
    ++P.b;
}

// Both steps in a row (the brute-force kernel).  Returns true when the lane still owns its pixel (either the path continues with
// a new ray in P.ray, or the next sample's primary ray was generated), false when the pixel is finished.
template <bool SPECULAR = true>
__device__ __forceinline__ bool shade_and_advance(const KParams& p, const Best& best, bool hit, const MaterialRef& M, Path& P)
{
    const int r = settle_hit<SPECULAR>(p, best, hit, M, P);
    if (r == kGoesOn) scatter<SPECULAR>(p, best, M, P);
    return r != kPixelDone;
}

__device__ __forceinline__ void flush_counters(const KParams& p, int lane, const Counters& cnt, bool stats)
{
    // (the pre-pass of a frame traces primary rays that are not path segments of the frame: only a tripped loop guard is reported)
    if (p.shade_mode == kShadePrimaryPass) {
        if (cnt.guard_hits != 0ull && lane == 0) atomicAdd(&p.counters[0], (unsigned long long)__popcll(cnt.guard_hits));
        return;
    }
    // wave-reduced counters, one atomic per wave and counter
    const unsigned long long rays = wave_sum((unsigned long long)cnt.rays);
    // (spread over kRaySlots addresses 128 bytes apart: thousands of waves end within microseconds of each other in a short
    // launch, and atomics on one address are served one after the other, ~10 ns each; the host adds the slots)
    if (lane == 0 && rays) atomicAdd(&p.counters[kRaySlotStride * (kRaySlotFirst + (blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave) % kRaySlots)], rays);
    if (lane == 0 && cnt.reused) atomicAdd(&p.counters[kAnsweredWord + kRaySlotStride * ((blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave) % kRaySlots)], (unsigned long long)cnt.reused);
    if (lane == 0 && cnt.cut) atomicAdd(&p.counters[kCutShortWord + kRaySlotStride * ((blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave) % kRaySlots)], (unsigned long long)cnt.cut);
    if (cnt.guard_hits != 0ull && lane == 0) atomicAdd(&p.counters[0], (unsigned long long)__popcll(cnt.guard_hits)); // (never in a healthy launch)
    if (stats) {
        const unsigned long long n = wave_sum((unsigned long long)cnt.nodes), t = wave_sum((unsigned long long)cnt.tris),
                                 pl = wave_sum((unsigned long long)cnt.planes);
        const unsigned long long r0 = wave_sum((unsigned long long)cnt.inner_rounds), r1 = wave_sum((unsigned long long)cnt.leaf_rounds),
                                 r2 = wave_sum((unsigned long long)cnt.tri_rounds), r3 = wave_sum((unsigned long long)cnt.plane_rounds),
                                 r4 = wave_sum((unsigned long long)cnt.segment_rounds), r5 = wave_sum((unsigned long long)cnt.no_mesh),
                                 r6 = wave_sum((unsigned long long)cnt.plane_exact), r7 = wave_sum((unsigned long long)cnt.stack_overflow),
                                 r8 = wave_sum((unsigned long long)cnt.wall_rounds);
        if (lane == 0) {
            if (n) atomicAdd(&p.counters[1], n);
            if (t) atomicAdd(&p.counters[2], t);
            if (pl) atomicAdd(&p.counters[3], pl);
            atomicAdd(&p.counters[8], r0);
            atomicAdd(&p.counters[9], r1);
            atomicAdd(&p.counters[10], r2);
            atomicAdd(&p.counters[11], r3);
            atomicAdd(&p.counters[12], r4);
            atomicAdd(&p.counters[14], r5);
            atomicAdd(&p.counters[15], r6);
            atomicAdd(&p.counters[26], r7);
            atomicAdd(&p.counters[31], r8);
        }
        {
            const unsigned long long u0 = wave_sum(cnt.t_start), u1 = wave_sum(cnt.t_inner), u2 = wave_sum(cnt.t_leaf);
            if (lane == 0) { atomicAdd(&p.counters[1 + 15], u0); atomicAdd(&p.counters[2 + 15], u1); atomicAdd(&p.counters[3 + 15], u2); }
            const unsigned long long w0 = wave_sum(cnt.t_b1), w1 = wave_sum(cnt.t_b2), w2 = wave_sum(cnt.t_b3);
            if (lane == 0) { atomicAdd(&p.counters[19], w0); atomicAdd(&p.counters[20], w1); atomicAdd(&p.counters[21], w2); }
            const unsigned long long l0 = wave_sum(cnt.t_l1), l1 = wave_sum(cnt.t_l2), l2 = wave_sum(cnt.t_l3);
            if (lane == 0) { atomicAdd(&p.counters[28], l0); atomicAdd(&p.counters[29], l1); atomicAdd(&p.counters[30], l2); }
        }
    }
}

__device__ __forceinline__ void init_path(Path& P)
{
    P.item = 0; P.send = 0; P.gxy = 0; P.s = 0; P.b = 0;
    P.pdx = P.pdy = 0.f; P.pdz = 1.f;
    P.ray = { 0.f, 0.f, 0.f, 0.f, 0.f, 1.f };
    P.bx = P.by = P.bz = 1.f;
    P.ax = P.ay = P.az = 0.f;
}

} // namespace
} // namespace ff
