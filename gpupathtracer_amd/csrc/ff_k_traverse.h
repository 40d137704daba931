// ff_k_traverse.h — device code of the trace kernels: closest hit (screening, the wall table, the 4-wide tree walk, traverse_budget).
#pragma once
#include "ff_k_lds.h"

namespace ff {
namespace {

// ---- closest hit, BVH mode -------------------------------------------------------------------------------------------
//
// intersectRays (kernel.cu:127-176) reorganised for 64-wide waves.  The result is the reference's result bit for bit;
// what changes is WHEN the expensive exact arithmetic runs:
//
//   * Every lane first screens all geometries against their world boxes (wave-uniform loop, scalar loads) and keeps a
//     bit mask of candidates; it then works through ITS OWN candidates, so a lane never executes code for a geometry it
//     has culled while its neighbours test it.
//   * Hit tests run in a fast form: the exact reference arithmetic up to (not including) the IEEE division, an
//     approximate reciprocal to place the hit along the ray, and an explicit margin.  A test that is clearly a hit
//     becomes the lane's PENDING candidate when it is not clearly farther than what the lane already holds; a test
//     that is clearly a miss is dropped; anything within the margin is decided at once by the exact reference test.
//   * The exact world distance (kernel.cu:113-114: IEEE divide, model transform, IEEE sqrt) is computed only when a
//     pending candidate is resolved: once per ray in the common case, and immediately whenever two candidates are too
//     close to rank approximately.  Ranking therefore always happens on exact reference distances.

constexpr int kLoopGuard = 1 << 16;              // upper bound on wave-level traversal rounds per query
constexpr float kRel = 1.0e-4f, kAbs = 1.0e-4f; // screening margins, far above the rounding error of the fast forms

struct Pending {
    float dist; // approximate world distance, +inf when empty
    int geom;   // record index, -1 when empty
    int rec;    // TriRecord index, -1 for a plane
};

// Per-lane state of one closest-hit query in flight.
struct Segment {
    BestId best;
    Pending pend;
    unsigned meshes;           // candidate meshes not started yet (bit = record index; scenes of up to 32 geometries)
    int cur, sp, mesh;         // traversal cursor (4-wide node relative to the mesh's root >= 0, leaf < 0, kDone), stack height, record index of the current mesh
    int tl_sp;                 // big scenes, while a mesh is being traversed: stack entries [0, tl_sp) are the pending entries of the
                               // geometry tree, the mesh's own entries sit above them (0 otherwise)
    int node_base;             // the current mesh's first node in the global 4-wide node array
    int lds_first, lds_count;  // its nodes [0, lds_count) sit in LDS from LDS node index lds_first on
    int bnx, bny, bnz;         // box planes (quarters of a node) the ray enters through, as byte offsets into the LDS node image (set_box_planes)
    int bfx, bfy, bfz;         // ... and leaves through
    Ray osr;                   // object-space ray of the current mesh
    float ix, iy, iz, ox, oy, oz; // 1/d and -o/d of osr (box tests)
    float scale;               // object-space t per unit of world distance
    float tbound;              // object-space ray parameter beyond which nothing can beat what the lane holds (box pruning)
    int resume;                // > 0: triangle resume-1 of the leaf under the cursor met a near tie with the pending candidate;
                               //      the caller resolves the pending one exactly, then the leaf continues from that triangle
};

__device__ __forceinline__ float inv_length(const Ray& r)
{
    return __builtin_amdgcn_rsqf(__builtin_fmaf(r.dx, r.dx, __builtin_fmaf(r.dy, r.dy, r.dz * r.dz)));
}

// Exact reference evaluation (kernel.cu:35-125) of candidate (g, rec) for world ray wr: world distance and hit point.
// Returns false if the exact test rejects it (cannot happen for a screened candidate; kept so that a wrong margin
// could never corrupt a result).
struct HitPoint {
    float wx, wy, wz; // world-space point
    float cx, cy, cz; // object-space normal as found (see Best)
};

// WN (the kernels on the scene's normal tables, KParams::tri_world_normals): H.cx, cy, cz is the candidate's unit WORLD normal instead - a
// triangle's from the table, fetched with its record; a plane's from quarter 8 of its LDS record, where those kernels keep it.
template <bool WN = false, class LDS>
__device__ __forceinline__ bool exact_hit(const LDS& L, const TriRecord* __restrict__ tris, const Ray& wr, int g, int rec, float& dist, HitPoint& H,
                                          int& orig_tri, const float4* __restrict__ wn_tris = nullptr)
{
    Ray osr;
    float len;
    object_space_ray_lds(L, g, wr, osr, len);
    float t;
    orig_tri = -1;
    if (rec >= 0) {
        const float4* tp = reinterpret_cast<const float4*>(tris) + (size_t)rec * 3;
        const float4 a = tp[0], b = tp[1], c = tp[2];
        orig_tri = __float_as_int(a.w);
        if constexpr (WN) {
            const float4 n = wn_tris[rec];
            t = triangle_t(a, b, c, osr);
            H.cx = n.x;
            H.cy = n.y;
            H.cz = n.z;
        } else {
            t = triangle_t(a, b, c, osr);
            const float e1x = b.x, e1y = b.y, e1z = b.z;
            const float e2x = c.x, e2y = c.y, e2z = c.z;
            H.cx = e1y * e2z - e2y * e1z; // kernel.cu:101 cross(edge1, edge2), shading normalises it where the reference does
            H.cy = e1z * e2x - e2z * e1x;
            H.cz = e1x * e2y - e2x * e1y;
            if (L.smooth_normals) smooth_normal(a, b, c, L.smooth_normals + (size_t)rec * 3, osr, H.cx, H.cy, H.cz);
        }
    } else {
        const float4 pn = lds_geom4(L, g, 11);
        if (g >= L.num_quads) {
            t = sphere_t(pn.w, osr);
            sphere_normal(pn.w, osr, t, H.cx, H.cy, H.cz);
        } else {
            t = plane_t(pn.x, pn.y, pn.z, osr);
            if constexpr (WN) {
                const float4 n = lds_geom4(L, g, kGeomWorldNormalVec4);
                H.cx = n.x;
                H.cy = n.y;
                H.cz = n.z;
            } else {
                H.cx = pn.x; // kernel.cu:26
                H.cy = pn.y;
                H.cz = pn.z;
            }
        }
    }
    if (!(t > 0.0f)) return false;
    const float4 m0 = lds_geom4(L, g, 4), m1 = lds_geom4(L, g, 5), m2 = lds_geom4(L, g, 6), m3 = lds_geom4(L, g, 7);
    const float Px = osr.ox + osr.dx * t, Py = osr.oy + osr.dy * t, Pz = osr.oz + osr.dz * t; // kernel.cu:99 / :16
    H.wx = (m0.x * Px + m1.x * Py) + (m2.x * Pz + m3.x);                                      // kernel.cu:113
    H.wy = (m0.y * Px + m1.y * Py) + (m2.y * Pz + m3.y);
    H.wz = (m0.z * Px + m1.z * Py) + (m2.z * Pz + m3.z);
    const float vx = wr.ox - H.wx, vy = wr.oy - H.wy, vz = wr.oz - H.wz;
    dist = ieee_sqrt((vx * vx + vy * vy) + vz * vz); // kernel.cu:114
    return true;
}

// Resolve the pending candidate exactly and merge it into `best` (kernel.cu:115-121).  Returns true if it became the
// best; then H is its hit point and normal.
template <bool WN = false, class LDS>
__device__ __forceinline__ bool resolve_pending(const LDS& L, const TriRecord* __restrict__ tris, const Ray& wr, Pending& pend, BestId& best,
                                                HitPoint& H, const float4* __restrict__ wn_tris = nullptr)
{
    const int g = pend.geom, rec = pend.rec;
    pend.geom = -1;
    pend.dist = kInf;
    float dist;
    int orig_tri;
    if (!exact_hit<WN>(L, tris, wr, g, rec, dist, H, orig_tri, wn_tris)) return false;
    bool take = dist < best.dist; // kernel.cu:115
    if (!take && dist == best.dist && best.geom >= 0) {
        // the reference keeps the first hit in (geometry, triangle) iteration order among equal distances
        const int go = lds_geom_i4(L, g, 17).y, bo = lds_geom_i4(L, best.geom, 17).y;
        if (go < bo) take = true;
        else if (go == bo && rec >= 0 && best.rec >= 0) take = orig_tri < tris[best.rec].orig_index;
    }
    if (take) {
        best.dist = dist;
        best.geom = g;
        best.rec = rec;
    }
    return take;
}

// Offer a certain hit at approximate world distance d to the lane's pending slot.  Returns true when the slot holds a
// candidate that is too close to rank approximately: the caller must resolve the held one exactly (resolve_pending) and
// offer this one again.  The exact code is kept OUT of the hot loops on purpose: it runs at wave-loop level, where the
// loops' temporaries are dead, which keeps the kernel within the register budget of 4 waves per SIMD.
__device__ __forceinline__ bool offer(float d, int g, int rec, Pending& pend, const BestId& best)
{
    const float lim = fminf(best.dist, pend.dist);
    if (d > lim * (1.0f + kRel) + kAbs) return false;                             // clearly farther than something already held
    if (pend.geom >= 0 && !(pend.dist > d * (1.0f + kRel) + kAbs)) return true;   // near tie with the held candidate
    pend.dist = d;
    pend.geom = g;
    pend.rec = rec;
    return false;
}

// One plane or sphere against the lane's query.  Planes are screened WITHOUT the IEEE sqrt/divide of kernel.cu:138: the hit
// position on the unit quad does not depend on the length of the object-space direction, so the screen works on the
// un-normalised direction M^-1*d, for which the ray parameter is the world-space parameter.  Anything within the margins
// (quad edges, t ~ 0, |n.d| ~ 1e-7) is decided by the exact reference test at once.
template <bool STATS, class LDS>
__device__ __forceinline__ void screen_analytic(const LDS& L, int g, const TriRecord* __restrict__ tris, const Ray& wr, float wlen, Segment& S, Counters& cnt)
{
    if (STATS) { cnt.planes += 1; probe_round(cnt.plane_rounds); }
    if (g >= L.num_quads) {
        // spheres have no screening form: the exact test runs here and yields the approximate world distance
        Ray osr;
        float len;
        object_space_ray_lds(L, g, wr, osr, len);
        const float tt = sphere_t(lds_geom4(L, g, 11).w, osr);
        const float sdist = tt * wlen * __builtin_amdgcn_rcpf(len);
        if (tt > 0.0f && offer(sdist, g, -1, S.pend, S.best)) {
            HitPoint H;
            resolve_pending(L, tris, wr, S.pend, S.best, H);
            offer(sdist, g, -1, S.pend, S.best);
        }
        return;
    }
    const float4 c0 = lds_geom4(L, g, 0), c1 = lds_geom4(L, g, 1), c2 = lds_geom4(L, g, 2), c3 = lds_geom4(L, g, 3);
    const float4 pn = lds_geom4(L, g, 11);
    // object-space origin and un-normalised direction (screening only: FMA form)
    const float ox = __builtin_fmaf(c0.x, wr.ox, __builtin_fmaf(c1.x, wr.oy, __builtin_fmaf(c2.x, wr.oz, c3.x)));
    const float oy = __builtin_fmaf(c0.y, wr.ox, __builtin_fmaf(c1.y, wr.oy, __builtin_fmaf(c2.y, wr.oz, c3.y)));
    const float oz = __builtin_fmaf(c0.z, wr.ox, __builtin_fmaf(c1.z, wr.oy, __builtin_fmaf(c2.z, wr.oz, c3.z)));
    const float ux = __builtin_fmaf(c0.x, wr.dx, __builtin_fmaf(c1.x, wr.dy, c2.x * wr.dz));
    const float uy = __builtin_fmaf(c0.y, wr.dx, __builtin_fmaf(c1.y, wr.dy, c2.y * wr.dz));
    const float uz = __builtin_fmaf(c0.z, wr.dx, __builtin_fmaf(c1.z, wr.dy, c2.z * wr.dz));
    const float nx = pn.x, ny = pn.y, nz = pn.z;
    const float dn = __builtin_fmaf(nx, ux, __builtin_fmaf(ny, uy, nz * uz));         // n . (M^-1 d)
    const float num = -__builtin_fmaf(nx, ox, __builtin_fmaf(ny, oy, nz * oz));       // -(n . o')
    const float len2 = __builtin_fmaf(ux, ux, __builtin_fmaf(uy, uy, uz * uz));
    // kernel.cu:12 |n.d'| >= 1e-7 with d' = u/len  <=>  dn^2 >= 1e-14 * len2
    const float q = dn * dn, qlim = 1.0e-14f * len2;
    const float ta = num * __builtin_amdgcn_rcpf(dn);                                 // world ray parameter of the plane
    const float Pxa = __builtin_fmaf(ta, ux, ox), Pya = __builtin_fmaf(ta, uy, oy);
    const float omag = fabsf(ox) + fabsf(oy) + fabsf(oz);
    // (an error of the parameter moves the point by that times u / dn: the margin grows with the ray's obliquity to the plane)
    const float delta = 1.0e-5f * (1.0f + omag) * __builtin_fmaf(fabsf(ux) + fabsf(uy), fabsf(__builtin_amdgcn_rcpf(dn)), 1.0f);
    const float ex = fabsf(Pxa), ey = fabsf(Pya);
    const bool front_sure = ta > 0.0f && fabsf(num) > 1.0e-5f * omag * (fabsf(nx) + fabsf(ny) + fabsf(nz));
    bool hit = ex <= 0.5f - delta && ey <= 0.5f - delta && front_sure && q >= qlim * 1.01f;
    float dist = ta * wlen; // approximate world distance
    if (!hit && ex <= 0.5f + delta && ey <= 0.5f + delta && q >= qlim * 0.99f && (front_sure || fabsf(num) <= 1.0e-5f * omag * (fabsf(nx) + fabsf(ny) + fabsf(nz)))) {
        // within a margin: decide with the exact reference test (kernel.cu:138 + :8-32)
        if (STATS) cnt.plane_exact += 1;
        Ray osr;
        float len;
        object_space_ray_lds(L, g, wr, osr, len);
        const float tt = plane_t(nx, ny, nz, osr);
        hit = tt > 0.0f;
        dist = tt * wlen * __builtin_amdgcn_rcpf(len);
    }
    if (hit && offer(dist, g, -1, S.pend, S.best)) {
        // two planes too close to rank approximately (a ray into an edge of the box): settle the held one exactly
        HitPoint H;
        resolve_pending(L, tris, wr, S.pend, S.best, H);
        offer(dist, g, -1, S.pend, S.best);
    }
}

// ---- axis-aligned walls (WallTable) ---------------------------------------------------------------------------------------
//
// One wall normal to world axis k against the calling lanes' rays, in world space: t = (c - o_k) / d_k through the slab
// constants of the ray, the hit point's other two coordinates against the rectangle.  (u, v) are the two other axes in the
// table's order.  Three outcomes per lane: a certain hit (the candidate of the lane if it is clearly the nearest so far), a
// certain miss, or `slow` gets the wall's bit: the per-lane screen of the plane's record decides, with the exact reference test
// where it is close (kernel.cu:8-32).  Certain means: by more than `dl` in the rectangle's plane - a multiple of the rounding
// error of BOTH this form and the reference's object-space arithmetic, which grows with the ray's obliquity to the wall (an
// error of the parameter moves the point by that times d_u / d_k) - and by more than `tt` in the parameter's sign.  NaNs (an
// origin beyond 1e8) compare false everywhere and land in `slow`.
__device__ __forceinline__ void wall_test(const Wall& w, float ixk, float oxk, float ou, float du, float ov, float dv, float dl, float tt, bool steep,
                                          float wlen, float& best_d, int& best_g, bool& tie, unsigned& slow)
{
    const float t = __builtin_fmaf(w.c, ixk, oxk);
    const float pu = __builtin_fmaf(t, du, ou), pv = __builtin_fmaf(t, dv, ov);
    const float m = fmaxf(fabsf(pu - w.cu) - w.hu, fabsf(pv - w.cv) - w.hv); // > 0: outside the rectangle by that much
    const bool hit = m <= -dl && t > tt && steep;
    const bool miss = m > dl || t < -tt;
    // Straight-line selects throughout.  (The two rare cases - a lane inside a margin, a second certain hit that is not clearly
    // nearer - behind wave-uniform branches instead: C2 -3 %, the default camera -4 %.  A branch costs this loop more than the
    // five vector instructions it skips.)
    slow |= (!hit && !miss) ? 1u << w.geom : 0u;
    // offer(): clearly farther than the lane's candidate -> dropped; clearly nearer -> the new candidate; else a near tie
    const float d = t * wlen;
    const bool nearer = hit && best_d > __builtin_fmaf(d, 1.0f + kRel, kAbs);
    const bool farther = d > __builtin_fmaf(best_d, 1.0f + kRel, kAbs);
    tie = tie || (hit && !nearer && !farther);
    best_d = nearer ? d : best_d;
    best_g = nearer ? w.geom : best_g;
}

// An entry that holds two walls with one rectangle, at w.c < w.hi_c (floor and ceiling, left and right wall of a box).  A ray
// that starts between them can reach only the one its direction points at: the rectangle is tested once, at that wall's parameter;
// the other wall is a certain miss when its own parameter is certainly negative (the same criterion as above) and goes to the
// per-lane screen otherwise (an origin outside the pair, or on the wall itself).
__device__ __forceinline__ void wall_test_pair(const Wall& w, float ixk, float oxk, float ou, float du, float ov, float dv, float dl, float tt, bool steep,
                                               float wlen, float& best_d, int& best_g, bool& tie, unsigned& slow)
{
    const float tlo = __builtin_fmaf(w.c, ixk, oxk), thi = __builtin_fmaf(w.hi_c, ixk, oxk);
    const bool up = ixk > 0.0f;
    const float t = up ? thi : tlo, tother = up ? tlo : thi;
    const int g = up ? w.hi_geom1 - 1 : w.geom, gother = up ? w.geom : w.hi_geom1 - 1;
    slow |= !(tother < -tt) ? 1u << gother : 0u;
    const float pu = __builtin_fmaf(t, du, ou), pv = __builtin_fmaf(t, dv, ov);
    const float m = fmaxf(fabsf(pu - w.cu) - w.hu, fabsf(pv - w.cv) - w.hv);
    const bool hit = m <= -dl && t > tt && steep;
    const bool miss = m > dl || t < -tt;
    slow |= (!hit && !miss) ? 1u << g : 0u;
    const float d = t * wlen;
    const bool nearer = hit && best_d > __builtin_fmaf(d, 1.0f + kRel, kAbs);
    const bool farther = d > __builtin_fmaf(best_d, 1.0f + kRel, kAbs);
    tie = tie || (hit && !nearer && !farther);
    best_d = nearer ? d : best_d;
    best_g = nearer ? g : best_g;
}

// All walls of the table against the calling lanes' rays (wave-uniform loops; the table comes through scalar loads).  Must run
// on a query that holds nothing yet (begin_segment).  A lane that met a near tie between two walls gives all of them to the
// per-lane screens, which rank on exact distances.
template <bool STATS>
__device__ __forceinline__ void screen_walls(const WallTable& W, const Ray& wr, const WorldSlab& ws, float wlen, Segment& S, unsigned& slow, Counters& cnt)
{
    const int nx = W.count[0], ny = nx + W.count[1], nz = ny + W.count[2];
    if (nz == 0) return;
    if (STATS) { cnt.planes += (unsigned)nz; probe_round(cnt.wall_rounds); }
    const float D = 2.0e-5f * ((fabsf(wr.ox) + fabsf(wr.oy)) + (fabsf(wr.oz) + W.margin_s));
    const float th = 0.05f * D;
    const float ax = fabsf(wr.dx), ay = fabsf(wr.dy), az = fabsf(wr.dz);
    const float aix = fabsf(ws.ix), aiy = fabsf(ws.iy), aiz = fabsf(ws.iz);
    const float gmin = W.graze * wlen;
    float best_d = kInf;
    int best_g = -1;
    bool tie = false;
    // (the record of the next wall is requested before the current one is tested: a scalar load per iteration would otherwise
    // sit in front of every test)
    Wall cur = W.w[0];
    int i = 0;
    {
        const float dl = D * __builtin_fmaf(fmaxf(ay, az), aix, 1.0f), tt = th * aix;
        const bool steep = ax >= gmin;
        for (; i < nx; ++i) {
            const Wall nxt = W.w[min(i + 1, kMaxWalls - 1)];
            if (cur.hi_geom1) wall_test_pair(cur, ws.ix, ws.ox, wr.oy, wr.dy, wr.oz, wr.dz, dl, tt, steep, wlen, best_d, best_g, tie, slow);
            else wall_test(cur, ws.ix, ws.ox, wr.oy, wr.dy, wr.oz, wr.dz, dl, tt, steep, wlen, best_d, best_g, tie, slow);
            cur = nxt;
        }
    }
    {
        const float dl = D * __builtin_fmaf(fmaxf(az, ax), aiy, 1.0f), tt = th * aiy;
        const bool steep = ay >= gmin;
        for (; i < ny; ++i) {
            const Wall nxt = W.w[min(i + 1, kMaxWalls - 1)];
            if (cur.hi_geom1) wall_test_pair(cur, ws.iy, ws.oy, wr.oz, wr.dz, wr.ox, wr.dx, dl, tt, steep, wlen, best_d, best_g, tie, slow);
            else wall_test(cur, ws.iy, ws.oy, wr.oz, wr.dz, wr.ox, wr.dx, dl, tt, steep, wlen, best_d, best_g, tie, slow);
            cur = nxt;
        }
    }
    {
        const float dl = D * __builtin_fmaf(fmaxf(ax, ay), aiz, 1.0f), tt = th * aiz;
        const bool steep = az >= gmin;
        for (; i < nz; ++i) {
            const Wall nxt = W.w[min(i + 1, kMaxWalls - 1)];
            if (cur.hi_geom1) wall_test_pair(cur, ws.iz, ws.oz, wr.ox, wr.dx, wr.oy, wr.dy, dl, tt, steep, wlen, best_d, best_g, tie, slow);
            else wall_test(cur, ws.iz, ws.oz, wr.ox, wr.dx, wr.oy, wr.dy, dl, tt, steep, wlen, best_d, best_g, tie, slow);
            cur = nxt;
        }
    }
    if (tie) {
        slow |= W.mask;
    } else if (best_g >= 0) {
        S.pend.dist = best_d;
        S.pend.geom = best_g;
        S.pend.rec = -1;
    }
}

// Start a closest-hit query: test every plane (fast form) and remember which meshes the ray can reach.
//
// Planes are pre-filtered by their world boxes in a wave-uniform loop, then screened per lane WITHOUT the IEEE sqrt/divide
// of kernel.cu:138: the hit position on the unit quad does not depend on the length of the object-space direction, so
// the screen works on the un-normalised direction M^-1*d, for which the ray parameter is the world-space parameter.
// Anything within the margins (quad edges, t ~ 0, |n.d| ~ 1e-7) is decided by the exact reference test at once.
// Scenes of up to 32 geometries (the reference has 5): every query screens all planes / spheres and collects its candidate meshes
// in a bit mask (larger scenes walk the geometry tree instead: enter_top / geom_step).
// Bit mask of the records in the query's candidate slots (records 0..31: the analytic records screened before anything else).
__device__ __forceinline__ unsigned holds(const Segment& S)
{
    return (S.pend.geom >= 0 ? 1u << (S.pend.geom & 31) : 0u) | (S.best.geom >= 0 ? 1u << (S.best.geom & 31) : 0u);
}

template <bool STATS, class LDS>
__device__ __forceinline__ bool scan_records(const LDS& L, const WallTable& W, const GeomRecord* __restrict__ geoms, int num_geoms, int num_planes,
                                           const TriRecord* __restrict__ tris, const Ray& wr, Segment& S, Counters& cnt, bool cut, unsigned emitters)
{
    const int prim_end = num_planes;
    const float wlen = __builtin_amdgcn_rcpf(inv_length(wr)); // |world direction| (1 for the integrator's rays)

    // Stage 1, wave-uniform: which quads can the ray reach at all?  The padded world box of a quad is flat, so for the
    // axis-aligned walls of a box scene this conservative slab test already singles out the one wall the ray hits.
    unsigned long long tb0 = 0, tb1 = 0, tb2 = 0;
    if (STATS) tb0 = __builtin_amdgcn_s_memtime();
    const WorldSlab ws = make_world_slab(wr);
    unsigned quads = 0u;
    // Stage 0, wave-uniform: the axis-aligned walls in world space (one multiply-add and two range checks each; the walls of a box
    // scene never reach the per-lane screens below except on their edges)
    screen_walls<STATS>(W, wr, ws, wlen, S, quads, cnt);
    for (int g = 0; g < prim_end; ++g) {
        if ((W.mask >> g) & 1u) continue;
        const float4 bmin = lds_geom4(L, g, 14), bmax = lds_geom4(L, g, 15);
        if (slab_may_hit(bmin.x, bmin.y, bmin.z, bmax.x, bmax.y, bmax.z, ws, kInf)) quads |= 1u << g;
    }
    if (STATS) tb1 = __builtin_amdgcn_s_memtime();
    // Stage 2, per lane: screen the lane's own candidates (records from the LDS copy at per-lane addresses).
    for (int guard = 0; __ballot(quads != 0u) != 0ull && guard < 32; ++guard) {
        if (quads == 0u) continue;
        const int g = __ffs((int)quads) - 1;
        quads &= quads - 1u;
        screen_analytic<STATS>(L, g, tris, wr, wlen, S, cnt);
    }

    if (STATS) tb2 = __builtin_amdgcn_s_memtime();
    // meshes: conservative world-box test against what the planes already found
    S.meshes = 0u;
    const float limit = fminf(S.best.dist, S.pend.dist);
    {
        // (the boxes of the meshes that have a tree come with the table: scalar loads, the next one requested before the test)
        // (one 32-byte scalar load per box: read field by field the compiler issues seven loads and as many address computations)
        typedef unsigned box_words __attribute__((ext_vector_type(8)));
        static_assert(sizeof(WallTable::MeshBox) == 32, "one box, one load");
        box_words cur = *reinterpret_cast<const box_words*>(&W.box[0]);
        for (int i = 0; i < W.num_boxes; ++i) {
            const box_words nxt = *reinterpret_cast<const box_words*>(&W.box[min(i + 1, 31)]);
            S.meshes |= slab_may_hit(__uint_as_float(cur.s0), __uint_as_float(cur.s1), __uint_as_float(cur.s2), __uint_as_float(cur.s4), __uint_as_float(cur.s5),
                                     __uint_as_float(cur.s6), ws, limit) ? 1u << cur.s3 : 0u;
            cur = nxt;
        }
    }
    // A path's last segment adds radiance only if it ends on an emitter.  Every analytic record has been screened: the nearest
    // of them is one of the (at most two) candidates held.  If neither is an emitter, the closest hit of the whole query is a
    // non-emitter or nothing, whatever the meshes hold: the query ends here.  (Returned, and counted by the caller at wave level.)
    const bool over = cut && (holds(S) & emitters) == 0u;
    if (over) S.meshes = 0u;
    if (STATS && S.meshes == 0u) cnt.no_mesh += 1;
    if (STATS) {
        const unsigned long long tb3 = __builtin_amdgcn_s_memtime();
        if ((threadIdx.x & 63) == __ffsll((long long)__ballot(true)) - 1) { cnt.t_b1 += tb1 - tb0; cnt.t_b2 += tb2 - tb1; cnt.t_b3 += tb3 - tb2; }
    }
    return over;
}

template <class LDS>
__device__ __forceinline__ void enter_top(const LDS& L, const Ray& wr, Segment& S);

// Big scenes: the planes kept out of the geometry tree (records [0, num_scan); host: count_scan_planes), screened like the planes
// of a small scene - world-box pre-filter in a wave-uniform loop, then every lane screens its own candidates - before the walk
// through the tree starts: the wall the ray ends on bounds that walk from its first node.
template <bool STATS, class LDS>
__device__ __forceinline__ void scan_walls(const LDS& L, const WallTable& W, const TriRecord* __restrict__ tris, const Ray& wr, Segment& S, Counters& cnt)
{
    const float wlen = __builtin_amdgcn_rcpf(inv_length(wr));
    const WorldSlab ws = make_world_slab(wr);
    unsigned prims = 0u;
    screen_walls<STATS>(W, wr, ws, wlen, S, prims, cnt);
    for (int g = 0; g < L.num_scan; ++g) {
        if ((W.mask >> g) & 1u) continue;
        const float4 bmin = lds_geom4(L, g, 14), bmax = lds_geom4(L, g, 15);
        if (slab_may_hit(bmin.x, bmin.y, bmin.z, bmax.x, bmax.y, bmax.z, ws, kInf)) prims |= 1u << g;
    }
    for (int guard = 0; __ballot(prims != 0u) != 0ull && guard < 8; ++guard) {
        if (prims == 0u) continue;
        const int g = __ffs((int)prims) - 1;
        prims &= prims - 1u;
        screen_analytic<STATS>(L, g, tris, wr, wlen, S, cnt);
    }
}

// Start a closest-hit query: empty candidate slots, then the geometry records (small scenes) or the root of the geometry tree.
// Returns true for a last-bounce query (`cut`) that is already over (scan_records).
template <bool STATS, class LDS>
__device__ __forceinline__ bool begin_segment(const LDS& L, const WallTable& W, const GeomRecord* __restrict__ geoms, int num_geoms, int num_planes,
                                              const TriRecord* __restrict__ tris, const Ray& wr, Segment& S, Counters& cnt, bool cut = false,
                                              unsigned emitters = 0u)
{
    S.best.dist = kInf; // kernel.cu:131
    S.best.geom = -1;
    S.best.rec = -1;
    S.pend.dist = kInf;
    S.pend.geom = -1;
    S.pend.rec = -1;
    S.cur = kDone;
    S.sp = 0;
    S.tl_sp = 0;
    S.mesh = -1;
    S.resume = 0;
    if constexpr (LDS::big) {
        // big scenes: the query starts at the root of the tree over the geometries, in world space
        S.meshes = 0u;
        if (L.num_scan > 0) scan_walls<STATS>(L, W, tris, wr, S, cnt);
        const bool over = cut && (holds(S) & emitters) == 0u; // (see scan_records: here every emitter is among the scanned planes)
        if (over) return true;
        enter_top(L, wr, S);
        S.cur = 0;
        return false;
    }
    return scan_records<STATS>(L, W, geoms, num_geoms, num_planes, tris, wr, S, cnt, cut, emitters);
}

// Box-pruning bound of the current mesh: refreshed whenever the lane's best/pending distance or its mesh changes, so the
// inner-node step reads one register instead of recomputing it per node.
__device__ __forceinline__ void refresh_tbound(Segment& S)
{
    S.tbound = (fminf(S.best.dist, S.pend.dist) * 1.001f + 1.0e-3f) * S.scale * 1.00001f;
}

// The links of a node are needed only after its box tests.  Left alone, the compiler merges the LDS load and the global load
// of the two branches into one load through a generic pointer placed after the tests: four flat_load_dword.  Pinning the
// loaded value inside each branch keeps them ds_read_b128 / global_load_dwordx4.
#define FF_PIN4(q) asm volatile("" : "+v"((q).x), "+v"((q).y), "+v"((q).z), "+v"((q).w))

// q[c] for a lane-varying c in 0..3 without control flow (the compiler turns a ?: chain on c into nested branches): two
// sign-extended bit fields as masks and three bit-field inserts.
__device__ __forceinline__ int select_slot(const uint4 q, int c)
{
    const unsigned m0 = (unsigned)((c << 31) >> 31), m1 = (unsigned)((c << 30) >> 31); // all ones where bit 0 / bit 1 of c is set
    const unsigned lo = (q.y & m0) | (q.x & ~m0), hi = (q.w & m0) | (q.z & ~m0);
    return (int)((hi & m1) | (lo & ~m1));
}

// Take the next subtree off the lane's stack.  An entry is a link (the common case: one sibling was pending) or names a
// node and two or three of its slots, nearest first (kPackedEntry | node << 8 | slots << 2 | count): then the node's link
// quarter is read again, the nearest slot becomes the cursor and the entry is rewritten for the rest.  One entry per
// visited node bounds the stack by the depth of the tree.
template <class LDS>
__device__ __forceinline__ void pop_entry(const LDS& L, const uint4* __restrict__ nodes4, Segment& S, int e)
{
    // (`e` is the entry on top of the lane's stack, already read; the caller has checked that the stack is not empty)
    if (e >= 0 && (e & kPackedEntry) != 0) {
        const int node = (e >> 8) & 0x3FFFFF;
        uint4 lk;
        if ((unsigned)node < (unsigned)S.lds_count) {
            lk = ff_smem[S.lds_first + node + 6 * L.node_cap];
            FF_PIN4(lk);
        } else {
            lk = *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(nodes4) + ((unsigned)(S.node_base + node) * (unsigned)(kNodeVec4 * 16) + 96u));
            FF_PIN4(lk);
        }
        S.cur = select_slot(lk, (e >> 2) & 3);
        const int rest = (e & 3) == 2 ? select_slot(lk, (e >> 4) & 3)                // one slot left: its link
                                      : ((e & ~0xFF) | (((e >> 4) & 0xF) << 2) | 2); // two left
        stack_push(L, S.sp - 1, rest);
    } else {
        S.cur = e;
        --S.sp;
    }
}

template <class LDS>
__device__ __forceinline__ void pop_subtree(const LDS& L, const uint4* __restrict__ nodes4, Segment& S)
{
    if (S.sp == (LDS::big ? S.tl_sp : 0)) {
        // nothing of the current tree is left; under a mesh of a big scene wait the pending entries of the geometry tree
        S.cur = LDS::big && S.mesh >= 0 ? kMeshDone : kDone;
        return;
    }
    pop_entry(L, nodes4, S, stack_pop(L, S.sp - 1));
}

// The quarters of a node the ray enters through (min planes 0/1/2 or max planes 3/4/5 by the signs of its direction) and leaves
// through, as BYTE offsets into the LDS node image (quarter k of node j: (k * node_cap + j) * 16): the inner step forms each of its
// six addresses with one add.  (Nodes outside LDS: inner_step derives the quarters from the same signs.)
template <class LDS>
__device__ __forceinline__ void set_box_planes(const LDS& L, Segment& S)
{
    const int q = L.node_cap * 16;
    S.bnx = S.ix < 0.0f ? 3 * q : 0;
    S.bny = S.iy < 0.0f ? 4 * q : q;
    S.bnz = S.iz < 0.0f ? 5 * q : 2 * q;
    S.bfx = 3 * q - S.bnx;
    S.bfy = 5 * q - S.bny;
    S.bfz = 7 * q - S.bnz;
}

// Put the lane's cursor on the root of mesh g's tree: object-space ray (kernel.cu:138), slab constants, box planes by the
// signs of the direction.
template <class LDS>
__device__ __forceinline__ void enter_mesh(const LDS& L, int g, const Ray& wr, Segment& S)
{
    const int4 tree = lds_geom_i4(L, g, 17); // bvh_root, orig_index, node4_first, lds_nodes
    if (tree.x < 0) return;
    float len;
    object_space_ray_lds(L, g, wr, S.osr, len);
    S.ix = safe_rcp(S.osr.dx);
    S.iy = safe_rcp(S.osr.dy);
    S.iz = safe_rcp(S.osr.dz);
    S.ox = -S.osr.ox * S.ix;
    S.oy = -S.osr.oy * S.iy;
    S.oz = -S.osr.oz * S.iz;
    set_box_planes(L, S);
    S.scale = len * inv_length(wr); // object-space t per unit of world distance
    refresh_tbound(S);
    S.mesh = g;
    S.node_base = tree.z;
    S.lds_count = tree.w;
    S.lds_first = __float_as_int(lds_geom4(L, g, 14).w);
    S.cur = 0;
    if constexpr (!LDS::big) S.sp = 0;
}

// Idle lane with candidate meshes left: enter the next one.
template <class LDS>
__device__ __forceinline__ void start_next_mesh(const LDS& L, const Ray& wr, Segment& S)
{
    const int g = __ffs((int)S.meshes) - 1;
    S.meshes &= S.meshes - 1u;
    enter_mesh(L, g, wr, S);
}

// Big scenes: the world-space half of the two-level traversal.  The lane's traversal state (ray, slab constants, box planes,
// node range) describes EITHER the geometry tree in world space (S.mesh < 0) OR one mesh in object space; the same inner
// step serves both.
template <class LDS>
__device__ __forceinline__ void enter_top(const LDS& L, const Ray& wr, Segment& S)
{
    S.osr = wr;
    S.ix = safe_rcp(wr.dx);
    S.iy = safe_rcp(wr.dy);
    S.iz = safe_rcp(wr.dz);
    S.ox = -wr.ox * S.ix;
    S.oy = -wr.oy * S.iy;
    S.oz = -wr.oz * S.iz;
    set_box_planes(L, S);
    S.scale = inv_length(wr); // ray parameter per unit of world distance (ff_intersect_rays takes rays of any length)
    refresh_tbound(S);
    S.mesh = -1;
    S.tl_sp = 0;
    S.node_base = L.top_first;
    S.lds_first = L.top_lds_first;
    S.lds_count = L.top_lds_count;
}

// A mesh is exhausted (S.cur == kMeshDone): back to the geometry tree, whose pending entries are on the stack below.
template <class LDS>
__device__ __forceinline__ void leave_mesh(const LDS& L, const uint4* __restrict__ nodes4, const Ray& wr, Segment& S)
{
    enter_top(L, wr, S);
    pop_subtree(L, nodes4, S);
}

// The cursor is on a leaf of the geometry tree: a plane or sphere is screened at once (kernel.cu:157-165 with the margins of
// screen_analytic), a mesh becomes the lane's current tree (kernel.cu:138: its object-space ray).  The slot's box test in
// the inner step has already pruned the geometry against what the lane held then.
template <bool STATS, class LDS>
__device__ __forceinline__ void geom_step(const LDS& L, int num_planes, const TriRecord* __restrict__ tris, const uint4* __restrict__ nodes4, const Ray& wr,
                                          Segment& S, Counters& cnt)
{
    const int g = (~S.cur) & (kGeomLeaf - 1);
    if (g < num_planes) {
        const float wlen = __builtin_amdgcn_rcpf(inv_length(wr));
        screen_analytic<STATS>(L, g, tris, wr, wlen, S, cnt);
        refresh_tbound(S);
        pop_subtree(L, nodes4, S);
    } else {
        const int floor = S.sp;
        if (STATS) cnt.no_mesh += 1; // (big scenes: the counter of plane-only queries counts mesh entries instead)
        enter_mesh(L, g, wr, S); // (leaves the cursor alone for a mesh without a tree)
        if (S.mesh == g) {
            S.tl_sp = floor;
            S.sp = floor;
        } else {
            pop_subtree(L, nodes4, S);
        }
    }
}

// One visit of a 4-wide node: test the four slot boxes, descend into the nearest hit, leave the others on the stack
// (nearest on top), or pop.  Pruning only: FMA + approximate 1/d on padded boxes with inflated bounds.
template <bool STATS, class LDS>
__device__ __forceinline__ void inner_step(const LDS& L, const uint4* __restrict__ nodes4, Segment& S, Counters& cnt)
{
    const int rel = S.cur;
    uint4 nx, ny, nz, fx, fy, fz, lk;
    if ((unsigned)rel < (unsigned)S.lds_count) {
        const char* const nb = reinterpret_cast<const char*>(ff_smem) + (S.lds_first + rel) * 16;
        nx = *reinterpret_cast<const uint4*>(nb + S.bnx);
        ny = *reinterpret_cast<const uint4*>(nb + S.bny);
        nz = *reinterpret_cast<const uint4*>(nb + S.bnz);
        fx = *reinterpret_cast<const uint4*>(nb + S.bfx);
        fy = *reinterpret_cast<const uint4*>(nb + S.bfy);
        fz = *reinterpret_cast<const uint4*>(nb + S.bfz);
        lk = *reinterpret_cast<const uint4*>(nb + 6 * 16 * L.node_cap);
        FF_PIN4(lk);
    } else {
        // (32-bit byte offsets from the array's base - a node index has 22 bits, kPackedEntry - so that the seven loads take the
        // base from a scalar register pair and one add each, instead of 64-bit address arithmetic per quarter)
        const char* const base = reinterpret_cast<const char*>(nodes4);
        static_assert(kNodeVec4 * 16 == 112, "node size");
        // (x 112 as two shifts: the compiler folds them back into the quarter-rate 32-bit multiply unless one is hidden from it)
        const unsigned ni = (unsigned)(S.node_base + rel);
        unsigned nb = ni << 7;
        asm volatile("" : "+v"(nb));
        nb -= ni << 4;
        const unsigned gx = S.ix < 0.0f ? 48u : 0u, gy = S.iy < 0.0f ? 64u : 16u, gz = S.iz < 0.0f ? 80u : 32u; // (set_box_planes)
        nx = *reinterpret_cast<const uint4*>(base + (nb + gx));
        ny = *reinterpret_cast<const uint4*>(base + (nb + gy));
        nz = *reinterpret_cast<const uint4*>(base + (nb + gz));
        fx = *reinterpret_cast<const uint4*>(base + (nb + (48u - gx)));
        fy = *reinterpret_cast<const uint4*>(base + (nb + (80u - gy)));
        fz = *reinterpret_cast<const uint4*>(base + (nb + (112u - gz)));
        lk = *reinterpret_cast<const uint4*>(base + (nb + 96u));
        FF_PIN4(lk);
    }
    if (STATS) { cnt.nodes += 1; probe_round(cnt.inner_rounds); }
    const float tbound = S.tbound;
    // slot c: entry parameter = the latest of the three near planes (and 0), exit = the earliest of the far planes (and the
    // pruning bound).  A hit slot sorts by its entry parameter: the key keeps the parameter's bits (non-negative floats
    // order like unsigned integers) with the slot number in the two low bits; a missed slot gets the largest key.
#define FF_SLOT_KEY(c, id)                                                                                                                       \
    ([&]() -> unsigned {                                                                                                                         \
        const float tn = fmaxf(fmaxf(__builtin_fmaf(__uint_as_float(nx.c), S.ix, S.ox), __builtin_fmaf(__uint_as_float(ny.c), S.iy, S.oy)),      \
                               fmaxf(__builtin_fmaf(__uint_as_float(nz.c), S.iz, S.oz), 0.0f));                                                  \
        const float tf = fminf(fminf(__builtin_fmaf(__uint_as_float(fx.c), S.ix, S.ox), __builtin_fmaf(__uint_as_float(fy.c), S.iy, S.oy)),      \
                               fminf(__builtin_fmaf(__uint_as_float(fz.c), S.iz, S.oz), tbound));                                                \
        return tn <= tf * 1.000002f ? ((__float_as_uint(tn) & ~3u) | (unsigned)(id)) : 0xFFFFFFFFu;                                              \
    }())
    unsigned k0 = FF_SLOT_KEY(x, 0), k1 = FF_SLOT_KEY(y, 1), k2 = FF_SLOT_KEY(z, 2), k3 = FF_SLOT_KEY(w, 3);
#undef FF_SLOT_KEY
    // five-comparator sorting network: k0 <= k1 <= k2 <= k3
    unsigned lo, hi;
    lo = min(k0, k1); hi = max(k0, k1); k0 = lo; k1 = hi;
    lo = min(k2, k3); hi = max(k2, k3); k2 = lo; k3 = hi;
    lo = min(k0, k2); hi = max(k0, k2); k0 = lo; k2 = hi;
    lo = min(k1, k3); hi = max(k1, k3); k1 = lo; k3 = hi;
    lo = min(k1, k2); hi = max(k1, k2); k1 = lo; k2 = hi;
    // Straight-line selects (the lanes of a wave disagree on every one of these cases): the nearest slot's link, and the
    // entry for the siblings to come back to: one -> its link; more -> the node and their slots, nearest first.
    const int near_link = select_slot(lk, (int)(k0 & 3u));
    const int second_link = select_slot(lk, (int)(k1 & 3u));
    const int packed = (int)((unsigned)kPackedEntry | ((unsigned)rel << 8) | ((k3 & 3u) << 6) | ((k2 & 3u) << 4) | ((k1 & 3u) << 2) |
                             (k3 != 0xFFFFFFFFu ? 3u : 2u));
    const int entry = k2 == 0xFFFFFFFFu ? second_link : packed;
    if (k1 != 0xFFFFFFFFu) {
        if (STATS && S.sp >= L.stack_depth) cnt.stack_overflow += 1; // (with a spill area: entries that went there)
        stack_push(L, S.sp, entry);
        ++S.sp;
    }
    if (k0 != 0xFFFFFFFFu) S.cur = near_link;
    else pop_subtree(L, nodes4, S);
}

// One leaf visit: test the leaf's triangles (fast form), then take the next entry off the stack.  On a near tie with the
// pending candidate the leaf is left under the cursor with S.resume set; the caller resolves the pending candidate and
// the leaf continues from the triangle that met the tie.
template <bool STATS, class LDS>
__device__ __forceinline__ void leaf_step(const LDS& L, const TriRecord* __restrict__ tris, const uint4* __restrict__ nodes4, const Ray& wr, Segment& S,
                                          Counters& cnt)
{
    const int ref = ~S.cur;
    const int first = ref >> 3, count = (ref & 7) + 1;
    const float4* tp = reinterpret_cast<const float4*>(tris) + (size_t)first * 3;
    const Ray& r = S.osr;
    int k = S.resume > 0 ? S.resume - 1 : 0;
    S.resume = 0;
    if (STATS) probe_round(cnt.leaf_rounds);
    unsigned long long tl_wait = 0, tl_test = 0, tl0 = 0;
    // The next triangle's record is requested before this one is tested (its wait overlaps the arithmetic; the last round asks
    // for its own record again, a hit in the L1).
    float4 An = tp[3 * k], E1n = tp[3 * k + 1], E2n = tp[3 * k + 2];
    for (; k < count; ++k) {
        if (STATS) tl0 = __builtin_amdgcn_s_memtime();
        const float4 A = An, E1 = E1n, E2 = E2n;
        {
            const int kn = min(k + 1, count - 1);
            An = tp[3 * kn]; E1n = tp[3 * kn + 1]; E2n = tp[3 * kn + 2];
        }
        if (STATS) {
            // (instrumented launches only: the wait for THIS triangle's three loads is made explicit so that it can be told from the
            // arithmetic; the three youngest loads - the next triangle's, issued just above - stay in flight as in the real kernel)
            asm volatile("s_waitcnt vmcnt(3) lgkmcnt(0)" ::: "memory");
            const unsigned long long tl1 = __builtin_amdgcn_s_memtime();
            if ((threadIdx.x & 63) == __ffsll((long long)__ballot(true)) - 1) tl_wait += tl1 - tl0; // one lane per round keeps the wave's time
            tl0 = tl1;
        }
        if (STATS) { cnt.tris += 1; probe_round(cnt.tri_rounds); }
        // kernel.cu:44-75: exact up to the division; every accept/reject comparison is the reference's own
        const float e1x = E1.x, e1y = E1.y, e1z = E1.z;
        const float e2x = E2.x, e2y = E2.y, e2z = E2.z;
        const float px = r.dy * e2z - e2y * r.dz, py = r.dz * e2x - e2z * r.dx, pz = r.dx * e2y - e2x * r.dy;
        const float det = dot3(e1x, e1y, e1z, px, py, pz);
        const float tx = r.ox - A.x, ty = r.oy - A.y, tz = r.oz - A.z;
        const float u = dot3(tx, ty, tz, px, py, pz);
        const float qx = ty * e1z - e1y * tz, qy = tz * e1x - e1z * tx, qz = tx * e1y - e1x * ty;
        const float v = dot3(r.dx, r.dy, r.dz, qx, qy, qz);
        const float tn = dot3(e2x, e2y, e2z, qx, qy, qz);
        bool ok = !(det < kTriEpsilon) && !(u < 0.0f || u > det) && !(v < 0.0f || u + v > det);
        if (ok && det < kTriEpsilon + E1.w) {
            // the back-face test of kernel.cu:48-49 could disagree with the sign of det only this close to edge-on
            const float nx = e1y * e2z - e2y * e1z, ny = e1z * e2x - e2z * e1x, nz = e1x * e2y - e2x * e1y;
            ok = !(dot3(r.dx, r.dy, r.dz, nx, ny, nz) > 0.0f);
        }
        if (ok) {
            float ta = tn * __builtin_amdgcn_rcpf(det); // approximate t (kernel.cu:77-79 is exact: 1/det, then multiply)
            if (ta < kTriEpsilon * 1.001f) {
                if (ta > kTriEpsilon * 0.999f) {
                    ta = tn * ieee_rcp(det); // within the margin of the t > EPSILON test: decide exactly (kernel.cu:97)
                    ok = ta > kTriEpsilon;
                } else {
                    ok = false;
                }
            }
            if (ok && offer(ta * __builtin_amdgcn_rcpf(S.scale), S.mesh, first + k, S.pend, S.best)) {
                S.resume = k + 1;
                if (STATS) tl_test += __builtin_amdgcn_s_memtime() - tl0; // (a near tie: rare, the lane's own count)
                break;
            }
        }
        if (STATS) {
            const unsigned long long tl2 = __builtin_amdgcn_s_memtime();
            if ((threadIdx.x & 63) == __ffsll((long long)__ballot(true)) - 1) tl_test += tl2 - tl0;
        }
    }
    refresh_tbound(S);
    if (STATS) {
        cnt.t_l1 += tl_wait;
        cnt.t_l2 += tl_test;
        tl0 = __builtin_amdgcn_s_memtime();
    }
    if (S.resume > 0) return;
    pop_subtree(L, nodes4, S);
    if (STATS) {
        const unsigned long long tl3 = __builtin_amdgcn_s_memtime();
        if ((threadIdx.x & 63) == __ffsll((long long)__ballot(true)) - 1) cnt.t_l3 += tl3 - tl0;
    }
}

// Settle what is still pending (the common case: the one exact evaluation of the ray, all hitting lanes together) and
// produce the hit point of the winner.  WN: best.cx, cy, cz receive its unit world normal (exact_hit).
template <bool WN = false, class LDS>
__device__ __forceinline__ void finish_segment(const LDS& L, const TriRecord* __restrict__ tris, const Ray& wr, Segment& S, Best& best,
                                               const float4* __restrict__ wn_tris = nullptr)
{
    bool have_point = false;
    HitPoint H = { 0.f, 0.f, 0.f, 0.f, 0.f, 1.f };
    if (S.pend.geom >= 0) have_point = resolve_pending<WN>(L, tris, wr, S.pend, S.best, H, wn_tris);
    if (!have_point && S.best.geom >= 0) {
        // the winner was resolved earlier (two candidates had been too close to rank approximately): recompute its point
        float dist;
        int orig_tri;
        exact_hit<WN>(L, tris, wr, S.best.geom, S.best.rec, dist, H, orig_tri, wn_tris);
    }
    best.dist = S.best.dist;
    best.geom = S.best.geom;
    best.rec = S.best.rec;
    best.px = H.wx; best.py = H.wy; best.pz = H.wz;
    best.cx = H.cx; best.cy = H.cy; best.cz = H.cz;
}

// Nothing left to do in the query.
__device__ __forceinline__ bool segment_done(const Segment& S) { return S.cur == kDone && S.meshes == 0u && S.resume == 0; }

// Advance the queries of the calling lanes: mesh starts, inner-node phases, leaf phases and near-tie resolutions alternate
// wave-wide until every calling lane is done or `budget` inner-node rounds have been spent (budget <= 0: no limit).
// Unfinished lanes keep their state in S and continue on the next call.
template <bool STATS, class LDS>
__device__ __forceinline__ void traverse_budget(const LDS& L, const TriRecord* __restrict__ tris, const uint4* __restrict__ nodes4, const Ray& wr,
                                                Segment& S, Counters& cnt, int budget, int leaf_threshold, int num_planes = 0)
{
    const int limit = budget > 0 ? budget : kLoopGuard;
    int rounds = 0, guard = 0;
    for (;;) {
        unsigned long long ta = 0, tb = 0, tc = 0, td = 0;
        if (STATS) ta = __builtin_amdgcn_s_memtime();
        if constexpr (LDS::big) {
            // lanes whose mesh is exhausted resume the geometry tree; lanes on a geometry leaf screen it or enter its mesh.
            // ONE round per iteration: a lane that pops straight into another geometry leaf waits for the next quorum instead of
            // being served with the two or three others in its situation (108 geometries: +5 %, 258: +8 %).
            {
                const bool back = S.cur == kMeshDone, geom = S.cur < 0 && ((~S.cur) & kGeomLeaf) != 0;
                if (__ballot(back || geom) != 0ull) {
                    if (back) leave_mesh(L, nodes4, wr, S);
                    else if (geom) geom_step<STATS>(L, num_planes, tris, nodes4, wr, S, cnt);
                }
            }
        } else {
            // A lane enters its next candidate mesh (object-space ray, slab constants: ~80 instructions) together with the lanes that
            // start their query, at the top of a slice; in mid-slice, where one or two lanes at a time would ask for it, it waits for
            // the next slice - unless no lane of the wave has anything else to traverse.
            if (guard == 0 || budget <= 0 || __ballot(S.cur != kDone) == 0ull)
                while (S.cur == kDone && S.meshes != 0u) start_next_mesh(L, wr, S);
        }
        if (STATS) tb = __builtin_amdgcn_s_memtime();
        if (__ballot(S.cur != kDone) == 0ull) break;
        bool leaves_due = true;
        for (;;) {
            const bool inner = (unsigned)S.cur < (unsigned)kMeshDone;
            if (__ballot(inner) == 0ull) break;
            // enough lanes hold a leaf: test the leaves now instead of idling them until the last lane finds one
            const bool tri_leaf = S.cur < 0 && !(LDS::big && ((~S.cur) & kGeomLeaf) != 0);
            if (__popcll(__ballot(tri_leaf)) >= leaf_threshold) break;
            if (rounds >= limit) break;
            if constexpr (LDS::big) {
                // enough lanes wait on the geometry tree (a geometry leaf, an exhausted mesh): serve them first; the few lanes
                // that hold triangles keep them for a fuller leaf phase
                if (__popcll(__ballot(S.cur == kMeshDone || (S.cur < 0 && !tri_leaf))) >= leaf_threshold) {
                    leaves_due = false;
                    break;
                }
            }
            ++rounds;
            if (inner) inner_step<STATS>(L, nodes4, S, cnt);
        }
        if (STATS) tc = __builtin_amdgcn_s_memtime();
        if (leaves_due && S.cur < 0 && !(LDS::big && ((~S.cur) & kGeomLeaf) != 0)) leaf_step<STATS>(L, tris, nodes4, wr, S, cnt);
        if (STATS) {
            td = __builtin_amdgcn_s_memtime();
            if ((threadIdx.x & 63) == __ffsll((long long)__ballot(true)) - 1) { cnt.t_start += tb - ta; cnt.t_inner += tc - tb; cnt.t_leaf += td - tc; }
        }
        // (a lane can wait with its leaf half tested for several turns in a big scene, where an iteration may serve the geometry
        // tree instead of the leaves: its pending candidate is resolved once, the first time round)
        if (__ballot(S.resume > 0 && S.pend.geom >= 0) != 0ull) {
            if (S.resume > 0 && S.pend.geom >= 0) {
                HitPoint H;
                resolve_pending(L, tris, wr, S.pend, S.best, H);
                refresh_tbound(S);
            }
        }
        if (rounds >= limit) break;
        if (++guard > kLoopGuard) break; // never reached by a well-formed tree; bounds the loop so no wave can spin forever
    }
    // The guard is a bound on a hang, not a way to end a query: a lane it cut short holds a truncated closest hit.  Make that
    // visible in every build (run-to-completion callers: any unfinished lane; time-sliced callers: only the iteration guard).
    if (budget <= 0 || guard > kLoopGuard) cnt.guard_hits |= __ballot(!segment_done(S));
}

// A complete closest-hit query for every calling lane (ray-batch kernel).
template <bool STATS, class LDS>
__device__ __forceinline__ void closest_hit_deferred(const LDS& L, const WallTable& W, const GeomRecord* __restrict__ geoms, int num_geoms, int num_planes,
                                                     const TriRecord* __restrict__ tris, const uint4* __restrict__ nodes4, const Ray& wr,
                                                     Best& best, Counters& cnt)
{
    Segment S;
    if (STATS) probe_round(cnt.segment_rounds);
    begin_segment<STATS>(L, W, geoms, num_geoms, num_planes, tris, wr, S, cnt);
    traverse_budget<STATS>(L, tris, nodes4, wr, S, cnt, 0, 64, num_planes);
    finish_segment(L, tris, wr, S, best);
    cnt.rays += 1;
}

// Brute-force closest hit: the reference's loop (kernel.cu:133-155) with the triangle array streamed through LDS in
// batches that the whole workgroup stages with coalesced 16-byte loads and then reads at a wave-uniform address.
// Must be called by every thread of the workgroup (it contains barriers); `live` masks lanes without a ray.
template <bool STATS>
__device__ __forceinline__ void closest_hit_brute(const GeomRecord* __restrict__ geoms, int num_geoms, const TriRecord* __restrict__ tris,
                                                  float4* batch, bool live, const Ray& wr, Best& best, Counters& cnt,
                                                  const float4* __restrict__ trinormals = nullptr)
{
    best.dist = kInf;
    best.geom = -1;
    best.rec = -1;
    best.px = best.py = best.pz = 0.0f;
    best.cx = best.cy = 0.0f;
    best.cz = 1.0f;
    for (int g = 0; g < num_geoms; ++g) {
        const GeomRecord& G = geoms[g];
        Ray osr;
        float len;
        object_space_ray(G, wr, osr, len);
        if (G.type == FF_GEOM_TRIANGLEMESH) {
            for (int base = 0; base < G.tri_count; base += kBruteBatchTris) {
                const int nb = min(kBruteBatchTris, G.tri_count - base);
                __syncthreads();
                const float4* src = reinterpret_cast<const float4*>(tris) + (size_t)(G.tri_first + base) * 3;
                for (int i = threadIdx.x; i < nb * 3; i += blockDim.x) batch[i] = src[i];
                __syncthreads();
                if (live) {
                    for (int k = 0; k < nb; ++k) {
                        const float4 a = batch[3 * k], b = batch[3 * k + 1], c = batch[3 * k + 2];
                        const float t = triangle_t(a, b, c, osr);
                        if (t > 0.0f) consider(G, g, G.tri_first + base + k, __float_as_int(a.w), t, osr, wr, geoms, tris, best);
                    }
                    if (STATS) cnt.tris += (unsigned)nb;
                }
            }
        } else if (live) {
            if (STATS) cnt.planes += 1;
            const float t = G.type == FF_GEOM_SPHERE ? sphere_t(G.plane_n[3], osr) : plane_t(G.plane_n[0], G.plane_n[1], G.plane_n[2], osr);
            if (t > 0.0f) consider(G, g, -1, -1, t, osr, wr, geoms, tris, best);
        }
    }
    if (live) {
        fill_object_normal(geoms, tris, best);
        fill_sphere_normal(geoms, wr, best);
        fill_smooth_normal(geoms, tris, trinormals, wr, best);
        cnt.rays += 1;
    }
}

} // namespace
} // namespace ff
