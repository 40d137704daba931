// ff_k_core.h — device code of the trace kernels: constants, rays and hits, the exact arithmetic (ieee_rcp, ieee_sqrt), the
// primitive tests and normals.  The ff_k_*.h headers are included by the kernel units only (ff_kernels.hip, ff_frame_kernels.hip).
#pragma once
#include "ff_kernels.h"

namespace ff {
namespace {

constexpr float kInf = __builtin_huge_valf();
constexpr float kTriEpsilon = 0.000001f;  // kernel.cu:38
constexpr float kPlaneDenomMin = 1e-7f;   // kernel.cu:12 compares a float with the double 1e-7: (double)|d| > 1e-7 <=> |d| >= float(1e-7)
constexpr float kRayEps = 1.0e-4f;        // origin offset of bounce rays along the unit normal (build-defined)
constexpr int kWave = 64;

struct Ray {
    float ox, oy, oz, dx, dy, dz;
};

// Closest hit.  rec = TriRecord index for triangles, -1 for planes; (px,py,pz) = world-space hit point.
struct Best {
    float dist;
    int geom;
    int rec;
    float px, py, pz;
    float cx, cy, cz; // object-space normal as found: cross(e1, e2) (not normalised) for a triangle, m_normal for a plane
};

// What a query carries while it is in flight: the exact distance and identity of the best resolved candidate.  The hit
// point is produced once, at the end (finish_segment), to keep three registers out of the traversal loop.
struct BestId {
    float dist;
    int geom;
    int rec;
};

struct Counters {
    unsigned rays, nodes, tris, planes; // per lane and launch (flushed into 64-bit device counters)
    unsigned cut;      // WAVE-uniform: last-bounce queries that ended after the analytic records (no emitter among the candidates)
    unsigned reused;   // WAVE-uniform (a scalar register): of the wave's `rays`, the repeated primary rays answered from the block's cache
    // occupancy probes (instrumented launches only): wave-level rounds of each phase.  The active-lane totals of the
    // phases are the counters above (nodes = inner-step lanes, tris = triangle-test lanes, planes, rays).
    unsigned inner_rounds, leaf_rounds, tri_rounds, plane_rounds, segment_rounds;
    unsigned no_mesh; // queries that needed no mesh traversal (planes only)
    unsigned stack_overflow; // instrumented launches: pushes beyond the stack's depth (must stay 0: the depth is a bound)
    unsigned plane_exact; // plane tests that fell inside a screening margin and ran the exact reference test
    unsigned wall_rounds; // wave-level passes over the table of axis-aligned walls
    unsigned long long guard_hits; // ALL launches, wave-uniform (a scalar register pair): lanes whose query the traversal loop guard cut short
                                   // (must stay 0; the host turns it into an error)
    unsigned long long t_start, t_inner, t_leaf; // instrumented launches: wave cycles in mesh starts / inner phases / leaf phases
    unsigned long long t_b1, t_b2, t_b3;         // ... and in the three parts of begin_segment (quad boxes / quad screens / mesh boxes)
    unsigned long long t_l1, t_l2, t_l3;         // ... and of a leaf visit: waiting for the triangle records / the tests / the pop that follows
};

// Count one wave-level round of a phase: exactly one of the active lanes (the lowest) records it.
__device__ __forceinline__ void probe_round(unsigned& counter)
{
    const unsigned long long m = __ballot(true);
    if ((int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) counter += 1;
}

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz)
{
    // glm dot(vec3): (x + y) + z  (GLM/detail/func_geometric.inl:52-53)
    const float px = ax * bx, py = ay * by, pz = az * bz;
    return (px + py) + pz;
}

// Correctly rounded 1/x and sqrt(x) (== the compiler's IEEE expansions, bit for bit, for every float: checked over all
// 2^32 inputs by tools/diag/ieee_check.hip and tests/test_gpu_properties.py).  In the range 2^-60 .. 2^60, where every
// operand of this renderer lives, one Newton step on the hardware estimate is already exact and replaces the 11 / 17
// instruction expansions with their denormal scaling; outside the range the full expansion runs.
__device__ __forceinline__ float ieee_rcp(float x)
{
    const unsigned a = __float_as_uint(x) & 0x7fffffffu;
    if (__builtin_expect(a - 0x21800000u < 0x3c000000u, 1)) { // 2^-60 <= |x| < 2^60
        const float y = __builtin_amdgcn_rcpf(x);
        const float e = __builtin_fmaf(-x, y, 1.0f);
        return __builtin_fmaf(e, y, y);
    }
    return 1.0f / x;
}
__device__ __forceinline__ float ieee_sqrt(float x)
{
    if (__builtin_expect(__float_as_uint(x) - 0x21800000u < 0x3c000000u, 1)) { // 2^-60 <= x < 2^60
        const float r = __builtin_amdgcn_rsqf(x);
        const float g = x * r, h = 0.5f * r;
        const float e = __builtin_fmaf(-g, g, x);
        return __builtin_fmaf(e, h, g);
    }
    return sqrtf(x);
}

} // namespace
} // namespace ff

// the rough-specular lobe (shared with the host twins), on the kernels' reciprocal and root
#define FF_GLOSSY_HD __device__ __forceinline__
#define FF_GLOSSY_RCP(x) ieee_rcp(x)
#define FF_GLOSSY_SQRT(x) ieee_sqrt(x)
#include "ff_glossy.h"
// the per-sample camera ray (shared with the host twin), likewise
#define FF_CAMERA_HD __device__ __forceinline__
#define FF_CAMERA_RCP(x) ieee_rcp(x)
#define FF_CAMERA_SQRT(x) ieee_sqrt(x)
#include "ff_camera.h"

namespace ff {
namespace {


// kernel.cu:138 — Ray(invM * vec4(o,1), normalize(invM * vec4(d,0))).  `len` is |invM*d| before normalisation: an
// object-space parameter t corresponds to the world distance t * |d_world| / len.
__device__ __forceinline__ void object_space_ray(const GeomRecord& G, const Ray& r, Ray& o, float& len)
{
    o.ox = (G.inv_c0[0] * r.ox + G.inv_c1[0] * r.oy) + (G.inv_c2[0] * r.oz + G.inv_c3[0]);
    o.oy = (G.inv_c0[1] * r.ox + G.inv_c1[1] * r.oy) + (G.inv_c2[1] * r.oz + G.inv_c3[1]);
    o.oz = (G.inv_c0[2] * r.ox + G.inv_c1[2] * r.oy) + (G.inv_c2[2] * r.oz + G.inv_c3[2]);
    const float tx = (G.inv_c0[0] * r.dx + G.inv_c1[0] * r.dy) + (G.inv_c2[0] * r.dz + G.inv_c0[3]);
    const float ty = (G.inv_c0[1] * r.dx + G.inv_c1[1] * r.dy) + (G.inv_c2[1] * r.dz + G.inv_c1[3]);
    const float tz = (G.inv_c0[2] * r.dx + G.inv_c1[2] * r.dy) + (G.inv_c2[2] * r.dz + G.inv_c2[3]);
    // normalize(vec4) with w == +-0: dot4 = (x*x + y*y) + (z*z + 0)
    const float dd = (tx * tx + ty * ty) + tz * tz;
    len = ieee_sqrt(dd);
    const float inv = ieee_rcp(len); // glm inversesqrt = 1 / sqrt
    o.dx = tx * inv;
    o.dy = ty * inv;
    o.dz = tz * inv;
}

// kernel.cu:110-125 on a candidate at object-space parameter t (brute-force kernels).  Ties on the world distance
// resolve like the reference's iteration order (lowest geometry index, then lowest triangle index).
__device__ __forceinline__ void consider(const GeomRecord& G, int g, int rec, int orig_tri, float t, const Ray& osr, const Ray& wr,
                                         const GeomRecord* __restrict__ geoms, const TriRecord* __restrict__ tris, Best& best)
{
    const float Px = osr.ox + osr.dx * t, Py = osr.oy + osr.dy * t, Pz = osr.oz + osr.dz * t; // kernel.cu:99 / :16
    const float wx = (G.mod_c0[0] * Px + G.mod_c1[0] * Py) + (G.mod_c2[0] * Pz + G.mod_c3[0]); // kernel.cu:113
    const float wy = (G.mod_c0[1] * Px + G.mod_c1[1] * Py) + (G.mod_c2[1] * Pz + G.mod_c3[1]);
    const float wz = (G.mod_c0[2] * Px + G.mod_c1[2] * Py) + (G.mod_c2[2] * Pz + G.mod_c3[2]);
    const float vx = wr.ox - wx, vy = wr.oy - wy, vz = wr.oz - wz;
    const float d2 = (vx * vx + vy * vy) + vz * vz;
    // sqrt is monotonic: a squared distance clearly above the best one cannot win or tie; skip the IEEE sqrt for it
    if (d2 > best.dist * best.dist * 1.00001f) return;
    const float dist = ieee_sqrt(d2); // glm distance, kernel.cu:114
    bool take = dist < best.dist; // kernel.cu:115
    if (!take && dist == best.dist && best.geom >= 0) {
        const int bo = geoms[best.geom].orig_index;
        if (G.orig_index < bo) take = true;
        else if (G.orig_index == bo && rec >= 0 && best.rec >= 0) take = orig_tri < tris[best.rec].orig_index;
    }
    if (take) {
        best.dist = dist;
        best.geom = g;
        best.rec = rec;
        best.px = wx;
        best.py = wy;
        best.pz = wz;
    }
}

// Object-space normal of a finished brute-force hit (the BVH path gets it from the exact evaluation of the winner).
__device__ __forceinline__ void fill_object_normal(const GeomRecord* __restrict__ geoms, const TriRecord* __restrict__ tris, Best& best)
{
    if (best.geom < 0) return;
    if (best.rec >= 0) {
        const float4* tp = reinterpret_cast<const float4*>(tris) + (size_t)best.rec * 3;
        const float4 b = tp[1], c = tp[2];
        const float e1x = b.x, e1y = b.y, e1z = b.z;
        const float e2x = c.x, e2y = c.y, e2z = c.z;
        best.cx = e1y * e2z - e2y * e1z;
        best.cy = e1z * e2x - e2z * e1x;
        best.cz = e1x * e2y - e2x * e1y;
    } else {
        const GeomRecord& G = geoms[best.geom];
        best.cx = G.plane_n[0];
        best.cy = G.plane_n[1];
        best.cz = G.plane_n[2];
    }
}


// kernel.cu:35-108 (Möller-Trumbore, division deferred, back faces culled).  Returns the object-space t or -1.
// A = (v0, original index), E1 = (v1 - v0, cull margin), E2 = (v2 - v0, -): the edges of :44-45 come with the record.
__device__ __forceinline__ float triangle_t(const float4 A, const float4 E1, const float4 E2, const Ray& r)
{
    const float e1x = E1.x, e1y = E1.y, e1z = E1.z; // :44
    const float e2x = E2.x, e2y = E2.y, e2z = E2.z; // :45
    const float nx = e1y * e2z - e2y * e1z, ny = e1z * e2x - e2z * e1x, nz = e1x * e2y - e2x * e1y; // :48 glm cross
    if (dot3(r.dx, r.dy, r.dz, nx, ny, nz) > 0.0f) return -1.0f;                                        // :49
    const float px = r.dy * e2z - e2y * r.dz, py = r.dz * e2x - e2z * r.dx, pz = r.dx * e2y - e2x * r.dy; // :53
    const float det = dot3(e1x, e1y, e1z, px, py, pz);                                                   // :54
    if (det < kTriEpsilon) return -1.0f;                                                                 // :57
    const float tx = r.ox - A.x, ty = r.oy - A.y, tz = r.oz - A.z;                                       // :61
    const float u = dot3(tx, ty, tz, px, py, pz);                                                        // :62
    if (u < 0.0f || u > det) return -1.0f;                                                               // :64
    const float qx = ty * e1z - e1y * tz, qy = tz * e1x - e1z * tx, qz = tx * e1y - e1x * ty;            // :68
    const float v = dot3(r.dx, r.dy, r.dz, qx, qy, qz);                                                  // :70
    if (v < 0.0f || u + v > det) return -1.0f;                                                           // :71
    float t = dot3(e2x, e2y, e2z, qx, qy, qz);                                                           // :75
    const float invDet = ieee_rcp(det); // :77 (a double division narrowed to float == the float division)
    t = t * invDet;                  // :79
    return t > kTriEpsilon ? t : -1.0f; // :97
}

// The barycentrics of kernel.cu:62,70,80-81 (u = dot(tvec, pvec) * invDet, v = dot(d, qvec) * invDet) for a triangle the
// ray is known to hit, and the vertex normals interpolated with them: n = ((1 - u) - v) n0 + u n1 + v n2.  A triangle whose
// three vertex normals are zero (an OBJ without vn) keeps its geometric normal: returns false.
__device__ __forceinline__ bool smooth_normal(const float4 A, const float4 E1, const float4 E2, const float4* __restrict__ nrm, const Ray& r, float& nx,
                                              float& ny, float& nz)
{
    const float px = r.dy * E2.z - E2.y * r.dz, py = r.dz * E2.x - E2.z * r.dx, pz = r.dx * E2.y - E2.x * r.dy;
    const float det = dot3(E1.x, E1.y, E1.z, px, py, pz);
    const float tx = r.ox - A.x, ty = r.oy - A.y, tz = r.oz - A.z;
    float u = dot3(tx, ty, tz, px, py, pz);
    const float qx = ty * E1.z - E1.y * tz, qy = tz * E1.x - E1.z * tx, qz = tx * E1.y - E1.x * ty;
    float v = dot3(r.dx, r.dy, r.dz, qx, qy, qz);
    const float invDet = ieee_rcp(det);
    u = u * invDet;
    v = v * invDet;
    const float4 n0 = nrm[0], n1 = nrm[1], n2 = nrm[2];
    const float w = (1.0f - u) - v;
    const float sx = (w * n0.x + u * n1.x) + v * n2.x;
    const float sy = (w * n0.y + u * n1.y) + v * n2.y;
    const float sz = (w * n0.z + u * n1.z) + v * n2.z;
    if (sx == 0.0f && sy == 0.0f && sz == 0.0f) return false;
    nx = sx;
    ny = sy;
    nz = sz;
    return true;
}

// kernel.cu:8-32 for an object-space ray and plane normal n.  Returns t or -1.
__device__ __forceinline__ float plane_t(float nx, float ny, float nz, const Ray& r)
{
    const float denom = dot3(nx, ny, nz, r.dx, r.dy, r.dz); // :11
    if (!(fabsf(denom) >= kPlaneDenomMin)) return -1.0f;    // :12
    const float t = dot3(-r.ox, -r.oy, -r.oz, nx, ny, nz) / denom; // :14-15
    const float Px = r.ox + t * r.dx, Py = r.oy + t * r.dy;        // :16
    if (!(Px >= -0.5f && Px <= 0.5f && Py >= -0.5f && Py <= 0.5f)) return -1.0f; // :18
    return t > 0.0f ? t : -1.0f;                                   // :23
}

// Sphere of radius `rad` about the object-space origin (build-defined: the reference only printf's at kernel.cu:166-169;
// oracle/ff_oracle.c orc_intersect_sphere is the definition).  Two-sided, nearest root above EPSILON.  Returns t or -1.
__device__ __forceinline__ float sphere_t(float rad, const Ray& r)
{
    const float b = dot3(r.ox, r.oy, r.oz, r.dx, r.dy, r.dz);
    const float c = dot3(r.ox, r.oy, r.oz, r.ox, r.oy, r.oz) - rad * rad;
    const float disc = b * b - c;
    if (!(disc >= 0.0f)) return -1.0f;
    const float sq = ieee_sqrt(disc);
    float t = -b - sq;
    if (!(t > kTriEpsilon)) {
        t = -b + sq;
        if (!(t > kTriEpsilon)) return -1.0f;
    }
    return t;
}

// Unit object-space normal of a sphere hit at parameter t: P * (1 / rad).
__device__ __forceinline__ void sphere_normal(float rad, const Ray& r, float t, float& nx, float& ny, float& nz)
{
    const float inv = ieee_rcp(rad);
    nx = (r.ox + r.dx * t) * inv;
    ny = (r.oy + r.dy * t) * inv;
    nz = (r.oz + r.dz * t) * inv;
}

// The same for a sphere: the winning hit is evaluated once more (same arithmetic, same result) for its object-space point.
__device__ __forceinline__ void fill_sphere_normal(const GeomRecord* __restrict__ geoms, const Ray& wr, Best& best)
{
    if (best.geom < 0 || geoms[best.geom].type != FF_GEOM_SPHERE) return;
    const GeomRecord& G = geoms[best.geom];
    Ray osr;
    float len;
    object_space_ray(G, wr, osr, len);
    const float t = sphere_t(G.plane_n[3], osr);
    sphere_normal(G.plane_n[3], osr, t, best.cx, best.cy, best.cz);
}

// Brute-force path: the interpolated vertex normal of a finished triangle hit (FF_SHADE_DIFFUSE_PATH_SMOOTH).
__device__ __forceinline__ void fill_smooth_normal(const GeomRecord* __restrict__ geoms, const TriRecord* __restrict__ tris,
                                                   const float4* __restrict__ trinormals, const Ray& wr, Best& best)
{
    if (!trinormals || best.geom < 0 || best.rec < 0) return;
    Ray osr;
    float len;
    object_space_ray(geoms[best.geom], wr, osr, len);
    const float4* tp = reinterpret_cast<const float4*>(tris) + (size_t)best.rec * 3;
    smooth_normal(tp[0], tp[1], tp[2], trinormals + (size_t)best.rec * 3, osr, best.cx, best.cy, best.cz);
}

} // namespace
} // namespace ff
