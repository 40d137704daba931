// ff_k_lds.h — device code of the trace kernels: the LDS layout of the BVH kernels, staging, the traversal stack, world slabs.
#pragma once
#include "ff_k_core.h"

namespace ff {
namespace {

// ---- LDS layout of the BVH kernels -----------------------------------------------------------------------------------
//
//   [ nodes: 7 planes of node_cap x 16 B ][ traversal stacks: stack_depth x BLOCK x 4 B, lane-strided ][ geometry records: G x 288 B ]
//
// ff_smem is indexed directly (never through a generic pointer) so that every access compiles to ds_read/ds_write.
extern __shared__ uint4 ff_smem[];

constexpr int kGeomVec4 = (int)(sizeof(GeomRecord) / 16); // 18 float4 per geometry record
constexpr int kGeomWorldNormalVec4 = 8;                   // kernels on the normal tables: this quarter of a PLANE's LDS record (nrm_c0, which they never read) holds its unit world normal
constexpr int kNodeVec4 = (int)(sizeof(Bvh4Node) / 16);   // 7 quarters per 4-wide node: six box planes + links
constexpr int kDone = 0x7fffffff;                         // traversal cursor of a lane with nothing left to visit
constexpr int kMeshDone = 0x7ffffffe;                     // big scenes: the current mesh is exhausted, the walk through the geometry tree resumes
constexpr int kGeomLeaf = 0x40000000;                     // big scenes: ~link of a geometry-tree leaf = kGeomLeaf | geometry record index
constexpr int kPackedEntry = 0x40000000;                  // stack entry that names a node and up to three of its slots (see inner_step)
constexpr unsigned kItemPixelMask = 0x1FFFFFFu;           // Path::item: the pixel item number (the host keeps pix_items below 2^25) ...
constexpr int kItemBlockShift = 25;                       // ... the sample block above it (at most 16 blocks per pixel) ...
constexpr unsigned kItemTail = 0x80000000u;               // ... and the sign bit for tail items
// Start records (KParams::start_records): the class of a pixel sits above the geometry index in word 3 of quarter 0
constexpr int kStartClassShift = 24;
constexpr unsigned kStartGeomMask = 0xFFFFFFu;
constexpr unsigned kStartGoesOn = 1u;  // a diffuse surface and more than one bounce: {second segment's origin, class | geometry} {flipped unit world normal, 0}
constexpr unsigned kStartEnds = 2u;    // the path ends at the first hit (an emitter, nothing in view, a one-bounce frame): {0, 0, 0, class} {the sample's radiance, 0}
constexpr unsigned kStartGeneral = 3u; // anything else (MIRROR / GLASS at the first hit): the raw hit serves

struct LdsBase {
    int node_cap;   // LDS node slots: quarter k of LDS node j lives at uint4 index k * node_cap + j
    int stack_base; // uint index of this lane's stack slot 0 (in units of 4 bytes from ff_smem)
    int stack_slot; // whose stack that is: the thread's own (its index in the workgroup), or, in the job-pool kernel, the job's slot
    int stack_depth; // entries per lane kept in LDS
    int* spill;      // deeper entries: entry e >= stack_depth of thread g of the launch at spill[(e - stack_depth) * threads + g] (null: none).
                     // Wave-uniform (scalar registers); the lane's own address is formed in the rare branch that needs it
    int block;       // workgroup size
    int stride;     // uints between consecutive stack entries of one lane (= block size)
    int geom_base;  // uint4 index of geometry record 0
    int num_quads;  // geometry records [0, num_quads) are planes; [num_quads, num_planes) spheres; meshes follow
    const float4* smooth_normals; // non-null: triangle hits carry the interpolated vertex normal (FF_SHADE_DIFFUSE_PATH_SMOOTH)
    // Scenes of more than 32 geometries ("big", a compile-time property of the kernel instantiation): the records stay in
    // global memory (L1/L2) and a query finds its candidates by walking a tree over the geometries' world boxes (tlas).
    // The geometry tree is a 4-wide tree like the meshes' (same nodes, same inner step, in WORLD space); its leaves are
    // geometries: link = ~(kGeomLeaf | record index).
    const float4* geoms_g;
    int top_first, top_lds_first, top_lds_count; // its first node in the node array and its share of the LDS node slots
    int num_scan; // ... and the records [0, num_scan) are planes that stay out of that tree (the walls of a room): every query screens them first
};
// (`big` is part of the TYPE, not a field: with a field the optimiser meets a select between an LDS and a global pointer in
// the record accessors before it has folded the flag, and this compiler crashes on it.)
// BIG: 0 = up to 32 geometries (records in LDS, every query screens them all); 1 = more, records still in LDS (up to
// kMaxLdsRecords); 2 = more than that, records read from global memory.
template <int BIG>
struct LdsT : LdsBase {
    static constexpr bool big = BIG != 0;
    static constexpr bool records_lds = BIG != 2;
};

template <int BIG = 0>
__device__ __forceinline__ LdsT<BIG> make_lds(int node_cap, int stack_depth, int block, int tid, int num_quads, const float4* smooth_normals = nullptr,
                                              const GeomRecord* geoms = nullptr, int top_first = 0, int top_lds_first = 0, int top_lds_count = 0,
                                              int num_scan = 0, int* spill = nullptr)
{
    LdsT<BIG> L;
    // Stack entries beyond the LDS levels live in global memory, lane-strided over the whole launch (the host trades the deepest,
    // rarely used stack levels for tree nodes in LDS: finalize_layout).  (Fetching the pointer from the kernel arguments only when
    // an entry spills, instead of keeping it in registers, was measured: no gain.)
    L.spill = spill;
    L.block = block;
    L.num_scan = num_scan;
    L.geoms_g = reinterpret_cast<const float4*>(geoms);
    L.top_first = top_first;
    L.top_lds_first = top_lds_first;
    L.top_lds_count = top_lds_count;
    L.num_quads = num_quads;
    L.smooth_normals = smooth_normals;
    L.node_cap = node_cap;
    L.stride = block;
    L.stack_base = node_cap * (kNodeVec4 * 4) + tid;
    L.stack_slot = tid;
    L.stack_depth = stack_depth;
    L.geom_base = node_cap * kNodeVec4 + (stack_depth * block) / 4;
    return L;
}

// Stage the top of every mesh's 4-wide tree and the geometry records: coalesced 16-byte loads, 1 KiB per wave-instruction.
// Persistent workgroups pay this once per launch, not per ray.  Which nodes of which mesh are cached was decided on the
// host (GeomRecord::lds_nodes nodes from the mesh's root on, at LDS node index lds_first: the trees are numbered level by
// level, so that is the top of each tree).
template <class LDS>
__device__ __forceinline__ void stage_scene(const LDS& L, const uint4* __restrict__ nodes4, const GeomRecord* __restrict__ geoms, int num_geoms,
                                            int num_planes, int tid, int block)
{
    // Nodes are stored as seven planes of 16-byte quarters: lanes fetch quarter k of unrelated nodes with one
    // ds_read_b128, and in this layout those addresses spread over all LDS banks, whereas whole nodes would put every
    // lane's quarter k on the same banks.
    for (int g = num_planes; g < num_geoms; ++g) {
        const int count = geoms[g].lds_nodes;
        if (count <= 0) continue;
        const int base = __float_as_int(geoms[g].wmin[3]);
        const uint4* src = nodes4 + (size_t)geoms[g].node4_first * kNodeVec4;
        for (int i = tid; i < count * kNodeVec4; i += block) {
            const int j = i / kNodeVec4, k = i - j * kNodeVec4;
            ff_smem[k * L.node_cap + base + j] = src[i];
        }
    }
    if constexpr (LDS::big) {
        const uint4* src = nodes4 + (size_t)L.top_first * kNodeVec4;
        for (int i = tid; i < L.top_lds_count * kNodeVec4; i += block) {
            const int j = i / kNodeVec4, k = i - j * kNodeVec4;
            ff_smem[k * L.node_cap + L.top_lds_first + j] = src[i];
        }
    }
    if constexpr (LDS::records_lds) {
        const uint4* gsrc = reinterpret_cast<const uint4*>(geoms);
        for (int i = tid; i < num_geoms * kGeomVec4; i += block) ff_smem[L.geom_base + i] = gsrc[i];
    }
    __syncthreads();
}

// Quarter k of geometry record g.
template <class LDS>
__device__ __forceinline__ float4 lds_geom4(const LDS& L, int g, int k)
{
    if constexpr (!LDS::records_lds) return L.geoms_g[(size_t)g * kGeomVec4 + k];
    return reinterpret_cast<const float4*>(ff_smem)[L.geom_base + g * kGeomVec4 + k];
}
template <class LDS>
__device__ __forceinline__ int4 lds_geom_i4(const LDS& L, int g, int k)
{
    if constexpr (!LDS::records_lds) return reinterpret_cast<const int4*>(L.geoms_g)[(size_t)g * kGeomVec4 + k];
    return reinterpret_cast<const int4*>(ff_smem)[L.geom_base + g * kGeomVec4 + k];
}
template <class LDS>
__device__ __forceinline__ void stack_push(const LDS& L, int sp, int v)
{
    if (__builtin_expect(sp < L.stack_depth, 1)) reinterpret_cast<int*>(ff_smem)[L.stack_base + sp * L.stride] = v;
    else L.spill[((size_t)(sp - L.stack_depth) * gridDim.x + blockIdx.x) * (size_t)L.block + (size_t)L.stack_slot] = v;
}
template <class LDS>
__device__ __forceinline__ int stack_pop(const LDS& L, int sp)
{
    // (each load pinned inside its branch: left alone the compiler merges the LDS and the global one into a single flat_load_dword
    // through a generic pointer, which takes the long way round for the LDS case and waits on both memory counters)
    int v;
    if (__builtin_expect(sp < L.stack_depth, 1)) {
        v = reinterpret_cast<const int*>(ff_smem)[L.stack_base + sp * L.stride];
        asm volatile("" : "+v"(v));
    } else {
        v = L.spill[((size_t)(sp - L.stack_depth) * gridDim.x + blockIdx.x) * (size_t)L.block + (size_t)L.stack_slot];
        asm volatile("" : "+v"(v));
    }
    return v;
}

// kernel.cu:138 with the geometry record gathered from LDS by a lane-varying index (same arithmetic as object_space_ray).
template <class LDS>
__device__ __forceinline__ void object_space_ray_lds(const LDS& L, int g, const Ray& r, Ray& o, float& len)
{
    const float4 c0 = lds_geom4(L, g, 0), c1 = lds_geom4(L, g, 1), c2 = lds_geom4(L, g, 2), c3 = lds_geom4(L, g, 3);
    o.ox = (c0.x * r.ox + c1.x * r.oy) + (c2.x * r.oz + c3.x);
    o.oy = (c0.y * r.ox + c1.y * r.oy) + (c2.y * r.oz + c3.y);
    o.oz = (c0.z * r.ox + c1.z * r.oy) + (c2.z * r.oz + c3.z);
    const float tx = (c0.x * r.dx + c1.x * r.dy) + (c2.x * r.dz + c0.w);
    const float ty = (c0.y * r.dx + c1.y * r.dy) + (c2.y * r.dz + c1.w);
    const float tz = (c0.z * r.dx + c1.z * r.dy) + (c2.z * r.dz + c2.w);
    const float dd = (tx * tx + ty * ty) + tz * tz;
    len = ieee_sqrt(dd);
    const float inv = ieee_rcp(len);
    o.dx = tx * inv;
    o.dy = ty * inv;
    o.dz = tz * inv;
}

// Per-ray constants for the conservative world-space AABB test of each geometry (pruning only).
struct WorldSlab {
    float ix, iy, iz, ox, oy, oz; // 1/d and -o/d
    float inv_len;                // 1 / |d|: converts a world distance into the ray parameter
};

__device__ __forceinline__ float safe_rcp(float d)
{
    const float s = fabsf(d) < 1e-30f ? copysignf(1e-30f, d) : d;
    return __builtin_amdgcn_rcpf(s);
}

__device__ __forceinline__ WorldSlab make_world_slab(const Ray& wr)
{
    WorldSlab w;
    w.ix = safe_rcp(wr.dx);
    w.iy = safe_rcp(wr.dy);
    w.iz = safe_rcp(wr.dz);
    w.ox = -wr.ox * w.ix;
    w.oy = -wr.oy * w.iy;
    w.oz = -wr.oz * w.iz;
    w.inv_len = __builtin_amdgcn_rsqf(__builtin_fmaf(wr.dx, wr.dx, __builtin_fmaf(wr.dy, wr.dy, wr.dz * wr.dz)));
    return w;
}

// Can the ray reach a world box before world distance `limit`?  Conservative: approximate arithmetic, inflated bounds,
// padded boxes; a `false` only ever skips work that could not have produced the closest hit.
__device__ __forceinline__ bool slab_may_hit(float mnx, float mny, float mnz, float mxx, float mxy, float mxz, const WorldSlab& w, float limit)
{
    const float a0 = __builtin_fmaf(mnx, w.ix, w.ox), a1 = __builtin_fmaf(mxx, w.ix, w.ox);
    const float b0 = __builtin_fmaf(mny, w.iy, w.oy), b1 = __builtin_fmaf(mxy, w.iy, w.oy);
    const float c0 = __builtin_fmaf(mnz, w.iz, w.oz), c1 = __builtin_fmaf(mxz, w.iz, w.oz);
    const float bound = (limit * 1.001f + 1.0e-3f) * w.inv_len * 1.00001f;
    const float tn = fmaxf(fmaxf(fminf(a0, a1), fminf(b0, b1)), fmaxf(fminf(c0, c1), 0.0f));
    const float tf = fminf(fminf(fmaxf(a0, a1), fmaxf(b0, b1)), fminf(fmaxf(c0, c1), bound));
    return tn <= tf * 1.000002f;
}

} // namespace
} // namespace ff
