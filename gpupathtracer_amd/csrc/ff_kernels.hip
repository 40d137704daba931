// ff_kernels.hip — the gfx950 (CDNA4, wave64) trace kernels.
//
// What the reference runs per pixel (kernel.cu:186-221: primary ray, brute-force closest hit over all geometries and
// triangles, shade, 8-bit store) is restructured here as a persistent mega-kernel:
//
//   * one workgroup per CU; the top of every mesh's 4-wide tree (the whole tree where it fits: the benchmark scene's does)
//     and all geometry records are staged ONCE per workgroup into LDS (112-byte nodes: six box planes for four slots + four
//     links, kept as seven planes of 16-byte quarters so that a wave's reads spread over all banks) and every lane keeps
//     its traversal stack in LDS (lane-strided: pushes / pops are bank-conflict free; one entry per visited node);
//   * lanes pull (pixel, sample block) work items with a wave-wide ballot + prefix compaction from the wave's own chunk of
//     the work queue (a chunk per atomic, 16 counters in different memory channels: acquire_pixel); a lane sums its block's
//     samples in order, terminated paths regenerate in place, and a combine pass adds a pixel's blocks in order;
//   * traversal is time-sliced: after a budget of inner-node rounds the lanes whose query is complete resolve, shade and
//     spawn their next ray TOGETHER while the long-tail lanes keep their traversal state; inside a slice the wave
//     alternates inner-node phases and leaf phases.  This keeps the 64 lanes occupied although neighbouring rays need
//     very different amounts of work;
//   * the per-pixel camera matrix work of kernel.cu:203 is hoisted to the host; the per-hit 4x4 inverse of
//     kernel.cu:117 is hoisted to the scene compiler.
//
// Numerics: the file is compiled with -ffp-contract=off and IEEE-correct sqrt/divide (1/x and sqrt through lean sequences
// that are verified bit-identical to the IEEE expansions on all 2^32 inputs).  Every value that decides or
// becomes part of a hit (object-space ray, Möller-Trumbore, world point, world distance, normal) is computed with
// the reference's / glm's exact operation order, so hits are bit-identical to the brute-force reference loop.  Only
// pruning (box tests, candidate screening) uses fused multiply-adds and approximate reciprocals, always with explicit
// margins: it can skip work that cannot matter, it never feeds a result.
#include "ff_k_traverse.h" // closest hit; below it ff_k_lds.h (LDS layout) and ff_k_core.h (exact arithmetic, primitive tests)
#include "ff_k_shade.h"    // the integrator and the work queue

namespace ff {
namespace {

// ---- the BVH mega-kernel -------------------------------------------------------------------------------------------------
//
// Time-sliced: every lane is a small state machine (no query / query in flight / query finished).  One iteration of the main
// loop lets the lanes whose query is finished - or that have none - resolve, shade, fetch work and start their next query
// TOGETHER (the setup block is large: it only pays at good occupancy), then every lane with a query in flight traverses for
// one slice of `setup_threshold` inner-node rounds (traverse_budget).  Lanes whose query outlives the slice keep their
// traversal state in registers and in their LDS stack and simply continue in the next iteration: per-ray traversal cost is
// heavy-tailed, and run to completion the inner-node phase had 11 % of its lanes busy.  Latency is hidden by occupancy: 1024
// threads per workgroup = 4 waves per SIMD.
//
// One iteration, in order (each a pass the whole wave walks through, whatever the number of lanes in it - which is why the
// expensive ones run once per iteration and the cheap one as often as needed):
//   finish_segment  exact evaluation of the finished queries' winners (kernel.cu:110-125)
//   settle_hit      does the path end here?  radiance, next sample, end of block; repeated for the lanes whose next sample starts
//                   from the block's parked primary hit (every sample of a pixel starts with the same ray)
//                   (START: once - a lane whose next sample starts loads its pixel's start record and joins scatter_start)
//   scatter         normal, random numbers, next ray: once, for paths that go on from a traced hit and from a parked hit alike
//   acquire_pixel   new (pixel, sample block) items for the lanes without work
//   begin_segment   walls (wall table), other planes / spheres, candidate meshes; a last-bounce query that holds no emitter ends here
//   traverse_budget one time slice of the 4-wide trees (a lane enters its next candidate mesh at the top of a slice)

// EXTRAS = false is the instantiation for scenes made of what the reference itself renders (planes and meshes, diffuse
// and emitting surfaces): the plane/sphere boundary becomes a compile-time "never" and the MIRROR / GLASS branches of the
// shader drop out (together they cost the reference-like scenes 3.5 % otherwise, measured on one box).
// BIG = 1 / 2 (with EXTRAS) are the instantiations for scenes of more than 32 geometries: candidates found by walking the tree
// over the geometries (enter_top / geom_step) instead of scanning all records; 2: records read from global memory.
// PREPASS = true is the instantiation that traces every pixel's primary ray once and stores its hit (settle_hit): the same loop on
// one-ray items; a compile-time switch because its store / mask code inside the shading loop would cost the frame's own kernel
// twenty spilled registers.
// START = true (diffuse scenes of up to 32 geometries: EXTRAS = false, BIG = 0) is the instantiation that runs on the pre-pass's start
// records instead of its raw hits: a sample starts inside the shading pass that ended the one before it, and the settle loop below
// is not part of it; a template parameter and not a branch for the reason PREPASS is one.
// WN = true (the same scenes, with START and without) is the instantiation that runs on the scene's normal tables (KParams::tri_world_normals,
// geom_world_normals): the unit world normal of a hit depends on the scene alone, so finish_segment fetches the winner's - a triangle's
// with its record, a plane's from its LDS record - into Best::cx, cy, cz, which otherwise carry the object-space normal, and the shading
// pass starts at the flip against the ray: no inverse-transpose product and no normalisation per hit (the cross product is still formed
// inside the winner's exact triangle test, which needs it; what goes is its second copy's way through the matrix).  WN = false computes them
// there (FF_NO_WORLD_NORMALS; the reference's own shade, which wants the object-space normal).
template <bool STATS, int BLOCK, bool EXTRAS, int BIG = 0, bool PREPASS = false, bool START = false, bool WN = false>
__global__ __launch_bounds__(BLOCK) void trace_bvh_kernel(const KParams p)
{
    static_assert(!START || (!EXTRAS && BIG == 0 && !PREPASS), "start records: the diffuse small-scene kernel only");
    static_assert(!WN || (!EXTRAS && BIG == 0 && !PREPASS), "normal tables: the diffuse small-scene kernels only");
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const LdsT<BIG> L = make_lds<BIG>(p.lds_nodes, p.stack_depth, BLOCK, tid, EXTRAS ? p.num_quads : 0x7fffffff, EXTRAS ? p.trinormals : nullptr,
                                      p.geoms, p.top_first, p.top_lds_first, p.top_lds_count, BIG ? p.num_scan : 0, p.stack_spill);
    const uint4* nodes4 = reinterpret_cast<const uint4*>(p.nodes4);
    if (p.debug_lds_words != 0u) {
        for (unsigned i = tid; i < p.debug_lds_words; i += BLOCK) reinterpret_cast<unsigned*>(ff_smem)[i] = p.debug_lds_pattern;
        __syncthreads();
    }
    stage_scene(L, nodes4, p.geoms, p.num_geoms, p.num_planes, tid, BLOCK);
    if constexpr (WN) {
        // a plane's unit world normal takes the place of the first inverse-transpose column in its LDS record (nothing else read those)
        for (int g = tid; g < p.num_planes; g += BLOCK) reinterpret_cast<float4*>(ff_smem)[L.geom_base + g * kGeomVec4 + kGeomWorldNormalVec4] = p.geom_world_normals[g];
        __syncthreads();
    }

    Counters cnt = {};
    Path P;
    init_path(P);
    WaveQueue Q = make_wave_queue(p);
    Segment S;
    S.best = { kInf, -1, -1 };
    S.pend = { kInf, -1, -1 };
    S.meshes = 0u;
    S.cur = kDone; S.sp = 0; S.mesh = -1; S.resume = 0;
    S.osr = { 0.f, 0.f, 0.f, 0.f, 0.f, 1.f };
    S.ix = S.iy = S.iz = S.ox = S.oy = S.oz = 0.f;
    S.scale = 1.f;
    S.tbound = 0.f;
    S.node_base = 0; S.lds_first = 0; S.lds_count = 0; S.tl_sp = 0;
    S.bnx = S.bny = S.bnz = S.bfx = S.bfy = S.bfz = 0;
    bool active = false, exhausted = false, inflight = false; // inflight: S holds a query of this lane (finished or not)
    // Every sample of a pixel starts with the same ray (kernel.cu:200-205: the pixel's corner, no jitter), so its closest hit is the
    // same hit spp times over.  A pre-pass of the frame (this kernel with shade_mode kShadePrimaryPass: one item per pixel, the hit
    // stored by settle_hit) traces it ONCE per pixel; here every sample starts from the stored hit: no query, no traversal, no
    // resolution for the primary segment - one fifth of the headline frame's path segments.  (Rounds 3 kept the hit per lane and sample
    // block: one traced primary ray per 64 samples and 1.6 GB of parked hits written per 1080p frame.)
    const bool reuse = START || (!PREPASS && p.primary_hits != nullptr); // wave-uniform
    // (the address is formed where it is used - a few instructions - rather than held in registers through the loop)
    auto stored_hit = [&](int k) { return p.primary_hits + (size_t)k * p.pix_items + ((unsigned)P.item & kItemPixelMask); };
    // instrumented launches only: wave cycles per phase (s_memtime), [0] resolve [1] shade [2] acquire [3] begin [4] traverse
    unsigned long long tphase[5] = { 0, 0, 0, 0, 0 };
    const unsigned long long wave_t0 = STATS ? wall_clock64() : 0ull;
    unsigned long long epoch = 0ull;
    if (STATS && p.timeline) {
        if (lane == 0) {
            const unsigned long long seen = atomicCAS(&p.counters[27], 0ull, wave_t0);
            epoch = seen ? seen : wave_t0;
        }
        epoch = __shfl(epoch, 0);
    }
    unsigned* const tl_row = STATS && p.timeline ? p.timeline + (size_t)(blockIdx.x * (BLOCK / kWave) + tid / kWave) * kTimelineBuckets : nullptr;
    int tl_bucket = 0;
    unsigned tl_count = 0u;
    for (;;) {
        unsigned long long t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0;
        if (STATS) t0 = __builtin_amdgcn_s_memtime();
        // Lanes whose query is finished (or that have none) resolve + shade + spawn together; lanes still traversing skip.
        const bool setup = !inflight || segment_done(S);
        if (STATS && p.timeline) {
            // every wave keeps its own row of the histogram (plain stores when the bucket changes: atomics on shared buckets
            // would throttle the launch they are meant to observe); the host adds the rows
            const int finished = __popcll(__ballot(setup && inflight));
            if (finished) {
                const unsigned long long now = wall_clock64();
                const unsigned long long bb = now > epoch ? (now - epoch) / p.timeline_ticks : 0ull;
                const int b = bb < (unsigned long long)kTimelineBuckets ? (int)bb : kTimelineBuckets - 1;
                if (b != tl_bucket) {
                    if (lane == 0 && tl_count) tl_row[tl_bucket] += tl_count;
                    tl_bucket = b;
                    tl_count = 0u;
                }
                tl_count += (unsigned)finished;
            }
        }
        Best best;
        bool hit = false;
        bool shade_now = setup && inflight; // lanes with a finished query
        if (shade_now) {
            finish_segment<WN>(L, p.tris, P.ray, S, best, p.tri_world_normals);
            hit = best.geom >= 0;
        }
        if (STATS) t1 = __builtin_amdgcn_s_memtime();
        if constexpr (START) {
            // Shading on start records.  Every sample of a pixel starts with the same ray, and the pre-pass has shaded its hit: a lane
            // whose path ends here (settle_hit: kNewSample) - or that took a new item in the last iteration - has its next sample's
            // first segment answered already.  It issues the loads of its pixel's record, counts the segment and joins THIS pass's
            // scatter as a lane that goes on.  One settle, one scatter per iteration; no lane waits for a second trip.  (Pixels whose
            // path ends at the first hit never get here: acquire_pixel answers their items.)
            bool from_rec = setup && !inflight && active && P.b == 0;
            bool goes_on = false;
            MaterialRef M;
            M.global = nullptr;
            M.geom_base = L.geom_base;
            M.g = 0;
            if (shade_now) {
                M.g = best.geom;
                const int r = settle_hit<false, false, WN>(p, best, hit, M, P);
                inflight = false;
                active = r != kPixelDone;
                goes_on = r == kGoesOn;
                from_rec = r == kNewSample;
            }
            float4 q0 = make_float4(0.f, 0.f, 0.f, 0.f), q1 = q0;
            if (from_rec) {
                const float4* rec = p.start_records + ((unsigned)P.item & kItemPixelMask);
                q0 = rec[0];
                q1 = rec[p.pix_items];
                cnt.rays += 1; // a path segment like any other, answered without a traversal (counted apart below)
                goes_on = true;
            }
            {
                const unsigned reused_now = (unsigned)__popcll(__ballot(from_rec));
                cnt.reused += reused_now;
                if (STATS && p.timeline) tl_count += reused_now; // (the launch timeline counts every path segment where it completes)
            }
            if (goes_on) scatter_start<WN>(p, best, M, P, from_rec, q0, q1);
        } else {
            // A lane that waits with a new sample (it starts from the pixel's stored primary hit, see below) joins this iteration's shading.
            bool from_cache = setup && !inflight && active && P.b == 0 && reuse;
            // Shading in two steps (settle_hit / scatter).  A lane whose path ended and whose next sample starts with the parked hit
            // settles again - at once if at least reuse_quorum lanes of the wave are in that position, else together with the next
            // iteration's finished queries - until every settling lane has a path that goes on from a hit, a first-of-block primary ray
            // to trace, a parked hit to wait with, or no work left.  Settling is cheap (a material lookup, a few multiplications); the
            // expensive step - normal, random numbers, new direction - then runs ONCE, for the lanes that go on from the hit they just
            // found and for those that go on from their parked primary hit alike.
            bool settle_now = shade_now, goes_on = false;
            for (;;) { // (every pass ends a sample of each lane in it: at most a block's samples)
                if (from_cache) {
                    const float4 c0 = *stored_hit(0), c1 = *stored_hit(1), c2 = *stored_hit(2);
                    best.dist = c0.x; best.px = c0.y; best.py = c0.z; best.pz = c0.w;
                    best.cx = c1.x; best.cy = c1.y; best.cz = c1.z;
                    best.geom = __float_as_int(c1.w);
                    best.rec = __float_as_int(c2.x);
                    hit = best.geom >= 0;
                    if constexpr (WN) {
                        // (the pre-pass stores the object-space normal, for every reader of the hits: this kernel wants the table's)
                        float4 n = make_float4(0.f, 0.f, 1.f, 0.f);
                        if (hit) {
                            if (best.rec >= 0) n = p.tri_world_normals[best.rec];
                            else n = lds_geom4(L, best.geom, kGeomWorldNormalVec4);
                        }
                        best.cx = n.x; best.cy = n.y; best.cz = n.z;
                    }
                    cnt.rays += 1; // a path segment like any other, answered without a traversal (counted apart below)
                    settle_now = true;
                }
                {
                    const unsigned reused_now = (unsigned)__popcll(__ballot(from_cache));
                    cnt.reused += reused_now;
                    if (STATS && p.timeline) tl_count += reused_now; // (the launch timeline counts every path segment where it completes)
                }
                if (__ballot(settle_now) == 0ull) break;
                bool waiting = false;
                if (settle_now) {
                    MaterialRef M;
                    M.global = BIG == 2 ? p.geoms + (hit ? best.geom : 0) : nullptr;
                    M.geom_base = L.geom_base;
                    M.g = best.geom;
                    const int r = settle_hit<EXTRAS, PREPASS, WN>(p, best, hit, M, P);
                    inflight = false;
                    active = r != kPixelDone;
                    goes_on = r == kGoesOn;
                    waiting = r == kNewSample && reuse; // a new sample: it starts from the pixel's stored primary hit
                }
                settle_now = false;
                from_cache = waiting && __popcll(__ballot(waiting)) >= p.reuse_quorum;
            }
            if (goes_on) {
                MaterialRef M;
                M.global = BIG == 2 ? p.geoms + best.geom : nullptr;
                M.geom_base = L.geom_base;
                M.g = best.geom;
                scatter<EXTRAS, WN>(p, best, M, P);
            }
        }
        if (STATS) t2 = __builtin_amdgcn_s_memtime();
        {
            const bool need = setup && !active && !exhausted;
            if (__ballot(need) != 0ull) {
                const unsigned rays_before = cnt.rays;
                const bool got = acquire_pixel<START>(p, lane, P, Q, need, cnt.rays, &cnt.reused); // (all lanes call: the wave's chunk of the queue is wave state)
                if (STATS && p.timeline) tl_count += (unsigned)wave_sum((unsigned long long)(cnt.rays - rays_before)); // (the rays of items dropped at the queue)
                if (need) {
                    active = got;
                    exhausted = !got;
                    if (STATS && exhausted) atomicMax(&p.counters[23], ~(unsigned long long)wall_clock64()); // (complemented) first lane to find the queue empty
                }
            }
        }
        if (STATS) t3 = __builtin_amdgcn_s_memtime();
        bool over = false; // a last-bounce query that ended after the planes
        if (setup && active && !(P.b == 0 && reuse)) { // (a lane whose sample starts from the stored primary hit waits for the next shading pass)
            if (STATS) probe_round(cnt.segment_rounds);
            over = begin_segment<STATS>(L, p.walls, p.geoms, p.num_geoms, p.num_planes, p.tris, P.ray, S, cnt, p.cut_last != 0 && P.b == p.bounces - 1, p.emitter_mask);
            cnt.rays += 1;
            inflight = true;
        }
        cnt.cut += (unsigned)__popcll(__ballot(over));
        if (STATS) t4 = __builtin_amdgcn_s_memtime();
        if (__ballot(inflight || (active && P.b == 0 && reuse)) == 0ull) break; // (a lane that waits with a stored hit still has work)
        // Time-sliced traversal: after `setup_threshold` inner-node rounds the finished lanes go and fetch new rays while the
        // long-tail lanes keep their state (per-ray traversal cost is heavy-tailed: a few rays need 10x the mean).
        if (inflight) traverse_budget<STATS>(L, p.tris, nodes4, P.ray, S, cnt, p.setup_threshold, p.leaf_threshold, p.num_planes);
        if (STATS) {
            const unsigned long long t5 = __builtin_amdgcn_s_memtime();
            tphase[0] += t1 - t0; tphase[1] += t2 - t1; tphase[2] += t3 - t2; tphase[3] += t4 - t3; tphase[4] += t5 - t4;
        }
    }
    if (STATS && p.timeline && lane == 0 && tl_count) tl_row[tl_bucket] += tl_count;
    if (STATS && lane == 0) {
        atomicAdd(&p.counters[4], tphase[0]);
        atomicAdd(&p.counters[5], tphase[1]);
        atomicAdd(&p.counters[6], tphase[2]);
        atomicAdd(&p.counters[7], tphase[3]);
        atomicAdd(&p.counters[13], tphase[4]);
        atomicMax(&p.counters[22], tphase[0] + tphase[1] + tphase[2] + tphase[3] + tphase[4]); // slowest wave
        atomicMax(&p.counters[24], ~(unsigned long long)wave_t0); // (complemented) first wave start, 100 MHz wall clock
        atomicMax(&p.counters[25], (unsigned long long)wall_clock64()); // last wave end
    }
    flush_counters(p, lane, cnt, STATS);
}

// ---- the job-pool mega-kernel ------------------------------------------------------------------------------------------------
//
// trace_bvh_kernel keeps a query in the lane that owns its path: when neighbouring rays need very different numbers of node
// visits, the lanes that are through idle until the wave's next setup pass (inner-node phase: a third of the lanes busy).
// Here the traversal of one (ray, mesh) pair is a JOB parked in LDS, and ANY wave of the workgroup executes jobs:
//
//   * a lane still owns its path (the path state never leaves its registers).  In a SETUP pass the lanes of a wave whose query is
//     complete (or that have none) resolve, shade, fetch work and screen the planes of their next ray together, exactly as in
//     trace_bvh_kernel; a lane whose ray can reach a mesh then writes the job - object-space ray, scale, bounds, cursor: 48 bytes
//     in its own slot of the job array - and puts the slot's number in the workgroup's queue (a ring in LDS);
//   * in the TRAVERSE role a wave takes jobs from the queue, 64 at a time, and walks them through the 4-wide trees in slices of a
//     few inner-node rounds; after a slice the lanes whose job is finished hand it back (16 bytes + a flag the owner polls) and,
//     once enough lanes are free, the wave takes as many new jobs: the inner-node phase runs on nearly full waves whatever the
//     spread of work between rays.  The traversal stack of a job lives in LDS under the job's slot, so a job can be put down by
//     one wave (16 bytes written back) and picked up by another;
//   * a wave runs a setup pass when enough of its own lanes are ready for one (pool_quorum) - or when the queue has nothing
//     to offer - and traverses otherwise.
//
// What crosses the hand-over is only what the walk needs; everything exact stays with the owner: a near tie between a triangle
// and the candidate the query holds (offer) ends the job with its leaf under the cursor, the owner resolves the held candidate
// exactly (kernel.cu:110-125) and posts the job again.  Per ray the sequence of box tests, triangle tests, offers and exact
// evaluations is the one trace_bvh_kernel performs: same bits, same ray counts.
//
// Scenes of up to 32 geometries (the reference has five); larger ones run trace_bvh_kernel.

constexpr int kPoolRing = 2048;          // queue entries (16-bit slot numbers): twice the most jobs that can be outstanding, so an
                                         // entry claimed by a consumer is never the one a producer writes
constexpr unsigned kRingEmpty = 0xFFFFu;
constexpr int kPoolSpinLimit = 1 << 20;  // bound on every wait of the pool kernel (a wait that long is a bug: the launch ends with an error instead of hanging)
constexpr int kPendEmpty = -2;           // job's pending tag: the query holds no pending candidate
constexpr int kPendOwner = -3;           // ... holds one whose identity stays with the owner (a plane, a triangle of an earlier mesh)
constexpr unsigned kJobReturned = 0x80000000u; // job word 9 (sp | mesh << 8 | resume << 16): set by the wave that hands the job back
constexpr unsigned kJobTie = 0x40000000u;      // ... because triangle resume - 1 of the leaf under the cursor met a near tie with the pending candidate

// Wave-uniform tallies of the traverse role, kept by every build (scalar registers): how full its rounds run.
struct PoolOccupancy {
    unsigned inner_rounds, inner_lanes; // inner-node rounds of the wave, and the lanes that visited a node in them (= node visits)
    unsigned leaf_rounds, leaf_lanes;   // leaf phases, and the lanes that held a leaf in them
};

struct PoolRef {
    int job_base;  // uint4 index: quarter q of job j at job_base + q * BLOCK + j
    int ring_base; // 16-bit index of ring entry 0
    int ctrl;      // 32-bit index of [head, tail]
};

__device__ __forceinline__ unsigned* pool_u32() { return reinterpret_cast<unsigned*>(ff_smem); }
__device__ __forceinline__ unsigned short* pool_u16() { return reinterpret_cast<unsigned short*>(ff_smem); }

// Put the calling lanes' slots (post) into the queue.  Called by all lanes of the wave.
__device__ __forceinline__ void pool_push(const PoolRef& Q, int lane, int slot, bool post)
{
    const unsigned long long m = __ballot(post);
    if (m == 0ull) return;
    // what the job's slot holds was written by this wave before this point: LDS executes a wave's instructions in order, and
    // the fence keeps the compiler from moving them behind the queue entry
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    const int leader = __ffsll((long long)m) - 1;
    unsigned base = 0u;
    if (lane == leader) base = __hip_atomic_fetch_add(&pool_u32()[Q.ctrl + 1], (unsigned)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    base = (unsigned)__builtin_amdgcn_readlane((int)base, leader);
    if (post) {
        const unsigned rank = (unsigned)__popcll(m & ((1ull << lane) - 1ull));
        __hip_atomic_store(&pool_u16()[Q.ring_base + (int)((base + rank) & (unsigned)(kPoolRing - 1))], (unsigned short)slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

// Take up to one job per asking lane (want) from the queue: returns the lane's job slot or -1.  Called by all lanes of the wave
// in wave-uniform control flow.
__device__ __forceinline__ int pool_pop(const PoolRef& Q, int lane, bool want, bool& stuck)
{
    const unsigned long long m = __ballot(want);
    const unsigned asked = (unsigned)__popcll(m);
    unsigned h = 0u, n = 0u;
    if (lane == 0) {
        for (int tries = 0; tries < kPoolSpinLimit; ++tries) {
            h = __hip_atomic_load(&pool_u32()[Q.ctrl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const unsigned t = __hip_atomic_load(&pool_u32()[Q.ctrl + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            n = min(asked, t - h);
            if (n == 0u) break;
            unsigned expect = h;
            if (__hip_atomic_compare_exchange_strong(&pool_u32()[Q.ctrl], &expect, h + n, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) break;
            n = 0u; // (if the tries run out: nothing taken)
        }
    }
    h = (unsigned)__builtin_amdgcn_readfirstlane((int)h);
    n = (unsigned)__builtin_amdgcn_readfirstlane((int)n);
    int slot = -1;
    const unsigned rank = (unsigned)__popcll(m & ((1ull << lane) - 1ull));
    if (want && rank < n) {
        unsigned short* e = &pool_u16()[Q.ring_base + (int)((h + rank) & (unsigned)(kPoolRing - 1))];
        unsigned v;
        // (the producer reserves its entries with one atomic and writes them straight after: a reserved entry that is still
        // empty is filled within a few instructions of another wave, which nothing here can hold up)
        int spins = 0;
        do { v = __hip_atomic_load(e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); } while (v == kRingEmpty && ++spins < kPoolSpinLimit);
        if (v != kRingEmpty) {
            __hip_atomic_store(e, (unsigned short)kRingEmpty, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            slot = (int)v;
        } else {
            stuck = true; // (never in a healthy launch: the caller gives up and the host reports it)
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    return slot;
}

// Jobs waiting in the queue (a snapshot).
__device__ __forceinline__ unsigned pool_waiting(const PoolRef& Q)
{
    const unsigned h = __hip_atomic_load(&pool_u32()[Q.ctrl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    const unsigned t = __hip_atomic_load(&pool_u32()[Q.ctrl + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return t - h;
}

// The third quarter of a job: what a traversal changes.  (cursor, sp | mesh << 8 | resume << 16 [| kJobReturned], pending distance, pending tag)
__device__ __forceinline__ uint4 job_state_quarter(const Segment& J, unsigned flags)
{
    return make_uint4((unsigned)J.cur, (unsigned)J.sp | ((unsigned)J.mesh << 8) | ((unsigned)J.resume << 16) | flags, __float_as_uint(J.pend.dist),
                      (unsigned)J.pend.rec);
}

// Write the whole job of the calling lane: the object-space ray and scale of the mesh just entered (enter_mesh), the exact distance
// the query has resolved so far, the state quarter.
template <int BLOCK>
__device__ __forceinline__ void job_write(const PoolRef& Q, int slot, const Segment& J)
{
    ff_smem[Q.job_base + slot] = make_uint4(__float_as_uint(J.osr.ox), __float_as_uint(J.osr.oy), __float_as_uint(J.osr.oz), __float_as_uint(J.scale));
    ff_smem[Q.job_base + BLOCK + slot] = make_uint4(__float_as_uint(J.osr.dx), __float_as_uint(J.osr.dy), __float_as_uint(J.osr.dz), __float_as_uint(J.best.dist));
    ff_smem[Q.job_base + 2 * BLOCK + slot] = job_state_quarter(J, 0u);
}

// Pick a job up: the traversal state of trace_bvh_kernel's Segment, rebuilt from the 48 bytes (slab constants, box planes,
// pruning bound) and the mesh's record.
template <int BLOCK, class LDS>
__device__ __forceinline__ void job_load(const PoolRef& Q, const LDS& L, int slot, Segment& J)
{
    const uint4 a = ff_smem[Q.job_base + slot], b = ff_smem[Q.job_base + BLOCK + slot], c = ff_smem[Q.job_base + 2 * BLOCK + slot];
    J.osr.ox = __uint_as_float(a.x); J.osr.oy = __uint_as_float(a.y); J.osr.oz = __uint_as_float(a.z);
    J.scale = __uint_as_float(a.w);
    J.osr.dx = __uint_as_float(b.x); J.osr.dy = __uint_as_float(b.y); J.osr.dz = __uint_as_float(b.z);
    J.best.dist = __uint_as_float(b.w);
    J.best.geom = -1;
    J.best.rec = -1;
    J.cur = (int)c.x;
    J.sp = (int)(c.y & 0xFFu);
    J.mesh = (int)((c.y >> 8) & 0xFFu);
    J.resume = (int)((c.y >> 16) & 0x3FFFu); // (> 0: the leaf under the cursor continues from triangle resume - 1: leaf_step)
    J.pend.dist = __uint_as_float(c.z);
    J.pend.rec = (int)c.w;
    J.pend.geom = (int)c.w == kPendEmpty ? -1 : J.mesh; // (only its sign matters to offer(); the owner knows whose it is)
    J.meshes = 0u;
    J.tl_sp = 0;
    J.ix = safe_rcp(J.osr.dx);
    J.iy = safe_rcp(J.osr.dy);
    J.iz = safe_rcp(J.osr.dz);
    J.ox = -J.osr.ox * J.ix;
    J.oy = -J.osr.oy * J.iy;
    J.oz = -J.osr.oz * J.iz;
    set_box_planes(L, J);
    refresh_tbound(J);
    const int4 tree = lds_geom_i4(L, J.mesh, 17);
    J.node_base = tree.z;
    J.lds_count = tree.w;
    J.lds_first = __float_as_int(lds_geom4(L, J.mesh, 14).w);
}

// One time slice of the traverse role: inner-node phases and leaf phases alternate wave-wide (traverse_budget without the parts
// that belong to the owner: mesh entry and exact resolution) until `limit` inner rounds have been spent or no lane can go on.
// A lane is busy while its cursor is on a node or a leaf and no near tie is waiting for its owner (`tied`: leaf_step left the leaf
// under the cursor with J.resume set).
template <bool STATS, class LDS>
__device__ __forceinline__ void pool_slice(const LDS& L, const TriRecord* __restrict__ tris, const uint4* __restrict__ nodes4, Segment& J, bool& tied,
                                           Counters& cnt, int limit, int leaf_threshold, PoolOccupancy& occ)
{
    const Ray none = { 0.f, 0.f, 0.f, 0.f, 0.f, 1.f };
    int rounds = 0;
    for (int guard = 0; guard < 4 * kWave; ++guard) {
        unsigned long long tb = 0, tc = 0;
        if (STATS) tb = __builtin_amdgcn_s_memtime();
        const bool busy = J.cur != kDone && !tied;
        if (__ballot(busy) == 0ull) break;
        for (;;) {
            const bool inner = !tied && (unsigned)J.cur < (unsigned)kMeshDone;
            if (__ballot(inner) == 0ull) break;
            const bool tri_leaf = !tied && J.cur < 0;
            if (__popcll(__ballot(tri_leaf)) >= leaf_threshold) break;
            if (rounds >= limit) break;
            ++rounds;
            if (!STATS) { occ.inner_rounds += 1u; occ.inner_lanes += (unsigned)__popcll(__ballot(inner)); }
            if (inner) inner_step<STATS>(L, nodes4, J, cnt);
        }
        if (STATS) tc = __builtin_amdgcn_s_memtime();
        if (!STATS) {
            const unsigned at_leaf = (unsigned)__popcll(__ballot(!tied && J.cur < 0));
            occ.leaf_rounds += at_leaf ? 1u : 0u;
            occ.leaf_lanes += at_leaf;
        }
        if (!tied && J.cur < 0) {
            leaf_step<STATS>(L, tris, nodes4, none, J, cnt);
            tied = J.resume > 0;
        }
        if (STATS) {
            const unsigned long long td = __builtin_amdgcn_s_memtime();
            if ((threadIdx.x & 63) == __ffsll((long long)__ballot(true)) - 1) { cnt.t_inner += tc - tb; cnt.t_leaf += td - tc; }
        }
        if (rounds >= limit) break;
    }
}

// The traverse role of trace_pool_kernel: take jobs from the workgroup's queue, walk them in slices, hand finished ones back, take
// new ones as lanes fall free; leave when enough of the wave's own lanes are ready for a setup pass (`waiting`: this lane has a job
// out; `nojob_ready`: it is ready without one) or when there is nothing to walk.  Returns true if a wait ran into the watchdog.
//
// A function of its own, NOT inlined, on purpose.  Walking needs every register a wave has at four waves per SIMD (128); inlined,
// the register allocator treats the kernel's two bodies - setup pass and traversal - as one, holds three dozen values of the one
// through the other and spills inside the loops of both (first build: 154 spills, the frame 41 % SLOWER than the lane-owned
// kernel).  Behind a call the walk gets an allocation of its own; what the kernel holds across the call is a few flags.  Its
// wave-uniform inputs come through a pointer to the kernel arguments and are made scalar on entry.
template <bool STATS, int BLOCK>
__device__ __attribute__((noinline)) bool pool_role(int job_base_in, int tid, bool waiting, bool nojob_ready, Counters* stats)
{
    auto uni = [](unsigned v) { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); };
    auto uni_ptr = [&](unsigned lo, unsigned hi) { return (void*)(((unsigned long long)uni(hi) << 32) | uni(lo)); };
    const int lane = tid & (kWave - 1);
    PoolRef Q;
    Q.job_base = (int)uni((unsigned)job_base_in);
    Q.ring_base = (Q.job_base + 3 * BLOCK) * 8;
    Q.ctrl = (Q.job_base + 3 * BLOCK) * 4 + kPoolRing / 2;
    // (the kernel left the role's wave-uniform inputs behind the queue's counters: taking the address of the kernel arguments
    // instead would make the compiler copy all 2 KB of them into every lane's scratch memory)
    const uint4 c0 = ff_smem[Q.ctrl / 4 + 1], c1 = ff_smem[Q.ctrl / 4 + 2], c2 = ff_smem[Q.ctrl / 4 + 3];
    const TriRecord* tris = static_cast<const TriRecord*>(uni_ptr(c0.x, c0.y));
    const uint4* nodes4 = static_cast<const uint4*>(uni_ptr(c0.z, c0.w));
    int* spill = static_cast<int*>(uni_ptr(c1.x, c1.y));
    const int slice = (int)uni(c1.z), leaf_threshold = (int)uni(c1.w), refill = (int)uni(c2.x), leave = (int)uni(c2.y), quorum = (int)uni(c2.z);
    const unsigned layout = uni(c2.w); // lds_nodes | stack_depth << 24
    const LdsT<0> L = make_lds<0>((int)(layout & 0xFFFFFFu), (int)(layout >> 24), BLOCK, tid, 0x7fffffff, nullptr, nullptr, 0, 0, 0, 0, spill);
    Counters cnt = {};
    PoolOccupancy occ = { 0u, 0u, 0u, 0u };
    bool stuck = false;
    Segment J;
    J.cur = kDone;
    J.resume = 0;
    J.sp = 0;
    J.mesh = 0;
    J.pend = { kInf, -1, kPendEmpty };
    J.best = { kInf, -1, -1 };
    int jslot = -1;
    bool tied = false;
    LdsT<0> Lj = L;
    bool leaving = false; // enough of this wave's own lanes are ready for a setup pass: no new jobs, the held ones run on for a while
    for (int turns = 0;; ++turns) {
        if (turns > kPoolSpinLimit) { stuck = true; break; } // (a job that never ends: a malformed tree)
        // free lanes take new jobs once there are enough of them (one atomic for all)
        const int held = __popcll(__ballot(jslot >= 0));
        if (leaving && held <= leave) {
            // put the stragglers down (16 bytes each; another wave picks them up together with other waves' stragglers) and go
            const bool down = jslot >= 0;
            if (down) ff_smem[Q.job_base + 2 * BLOCK + jslot] = job_state_quarter(J, 0u);
            pool_push(Q, lane, jslot, down);
            break;
        }
        if (!leaving && (kWave - held >= refill || held == 0) && (held == 0 || uni(pool_waiting(Q)) != 0u)) {
            const int got = pool_pop(Q, lane, jslot < 0, stuck);
            if (got >= 0) {
                jslot = got;
                Lj.stack_base = L.node_cap * (kNodeVec4 * 4) + got;
                Lj.stack_slot = got;
                job_load<BLOCK>(Q, Lj, got, J);
            }
        }
        if (__ballot(stuck) != 0ull) { stuck = true; break; }
        if (__ballot(jslot >= 0) == 0ull) break; // nothing held, nothing queued
        pool_slice<STATS>(Lj, tris, nodes4, J, tied, cnt, slice, leaf_threshold, occ);
        // finished jobs (and jobs that met a near tie) go back to their owners
        const bool back = jslot >= 0 && (J.cur == kDone || tied);
        if (__ballot(back) != 0ull) {
            if (back) {
                // (the state first, then - in an instruction of its own - the flag its owner polls)
                const uint4 st = job_state_quarter(J, tied ? kJobTie : 0u);
                ff_smem[Q.job_base + 2 * BLOCK + jslot] = st;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __hip_atomic_store(&pool_u32()[(Q.job_base + 2 * BLOCK + jslot) * 4 + 1], st.y | kJobReturned, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                jslot = -1;
                tied = false;
                J.cur = kDone;
                J.resume = 0;
            }
        }
        // enough of this wave's own lanes ready for a setup pass?
        if (!leaving) {
            bool ret2 = false;
            if (waiting) ret2 = (__hip_atomic_load(&pool_u32()[(Q.job_base + 2 * BLOCK + tid) * 4 + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & kJobReturned) != 0u;
            leaving = __popcll(__ballot(ret2 || nojob_ready)) >= quorum;
        }
    }
    if (!STATS && lane == 0) {
        // (the workgroup's tallies sit behind the role's inputs; thread 0 adds them to the launch's counters when the workgroup ends)
        unsigned long long* t = reinterpret_cast<unsigned long long*>(&pool_u32()[Q.ctrl + 16]);
        __hip_atomic_fetch_add(&t[0], (unsigned long long)occ.inner_rounds, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(&t[1], (unsigned long long)occ.inner_lanes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(&t[2], (unsigned long long)occ.leaf_rounds, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(&t[3], (unsigned long long)occ.leaf_lanes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    if (STATS && stats != nullptr) {
        stats->nodes += cnt.nodes; stats->tris += cnt.tris;
        stats->inner_rounds += cnt.inner_rounds; stats->leaf_rounds += cnt.leaf_rounds; stats->tri_rounds += cnt.tri_rounds;
        stats->stack_overflow += cnt.stack_overflow;
        stats->t_inner += cnt.t_inner; stats->t_leaf += cnt.t_leaf;
        stats->t_l1 += cnt.t_l1; stats->t_l2 += cnt.t_l2; stats->t_l3 += cnt.t_l3;
    }
    return __ballot(stuck) != 0ull;
}

template <bool STATS, int BLOCK, bool EXTRAS>
__global__ __launch_bounds__(BLOCK) void trace_pool_kernel(const KParams p)
{
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const LdsT<0> L = make_lds<0>(p.lds_nodes, p.stack_depth, BLOCK, tid, EXTRAS ? p.num_quads : 0x7fffffff, EXTRAS ? p.trinormals : nullptr, p.geoms, 0, 0, 0,
                                  0, p.stack_spill);
    const uint4* nodes4 = reinterpret_cast<const uint4*>(p.nodes4);
    if (p.debug_lds_words != 0u) {
        for (unsigned i = tid; i < p.debug_lds_words; i += BLOCK) reinterpret_cast<unsigned*>(ff_smem)[i] = p.debug_lds_pattern;
        __syncthreads();
    }
    // the pool sits behind the geometry records: [jobs: 3 quarters x BLOCK x 16 B][ring: kPoolRing x 2 B][head, tail, -, -]
    PoolRef Q;
    Q.job_base = L.geom_base + p.num_geoms * kGeomVec4;
    Q.ring_base = (Q.job_base + 3 * BLOCK) * 8;
    Q.ctrl = (Q.job_base + 3 * BLOCK) * 4 + kPoolRing / 2;
    for (int i = tid; i < kPoolRing / 2; i += BLOCK) pool_u32()[Q.ring_base / 2 + i] = 0xFFFFFFFFu;
    if (tid < 4) pool_u32()[Q.ctrl + tid] = 0u;
    if (tid < 16) pool_u32()[Q.ctrl + 16 + tid] = 0u; // the workgroup's tallies (pool_role, and the waves' time split below)
    if (tid == 0) {
        // the traverse role's wave-uniform inputs (pool_role reads them back from here)
        const unsigned long long a = (unsigned long long)p.tris, b = (unsigned long long)p.nodes4, c = (unsigned long long)p.stack_spill;
        ff_smem[Q.ctrl / 4 + 1] = make_uint4((unsigned)a, (unsigned)(a >> 32), (unsigned)b, (unsigned)(b >> 32));
        ff_smem[Q.ctrl / 4 + 2] = make_uint4((unsigned)c, (unsigned)(c >> 32), (unsigned)p.pool_slice, (unsigned)p.leaf_threshold);
        ff_smem[Q.ctrl / 4 + 3] = make_uint4((unsigned)p.pool_refill, (unsigned)p.pool_leave, (unsigned)p.pool_quorum, (unsigned)p.lds_nodes | ((unsigned)p.stack_depth << 24));
    }
    ff_smem[Q.job_base + 2 * BLOCK + tid] = make_uint4((unsigned)kDone, 0u, 0u, (unsigned)kPendEmpty);
    stage_scene(L, nodes4, p.geoms, p.num_geoms, p.num_planes, tid, BLOCK); // (ends with the workgroup's barrier)

    Counters cnt = {};
    WaveQueue WQ = make_wave_queue(p);
    // The lane's own path (Path) and what it keeps of its query while a job is out (the exactly resolved winner so far, the pending
    // candidate, the meshes to come; its ray count) live in the lane's slot of a global array (KParams::park, 7 x 16 bytes, lane-
    // strided) BETWEEN setup passes: a pass loads them, works, and stores them back.  While the lane walks other lanes' jobs they
    // would be 30 registers of dead weight, and walking needs every register the wave has (four waves per SIMD: 128); carried
    // through the loop they were spilled and re-loaded piecemeal in every phase (first build: 154 spills, -41 %).  What IS carried
    // from iteration to iteration is a handful of flags.
    // (`me` is the thread's index behind an optimisation barrier, taken afresh in every pass: formed from `tid` the seven slot
    // addresses - and a dozen others - are loop invariants that the compiler computes once and then holds in registers through
    // BOTH roles: 80 VGPRs that neither could spare)
    auto park_slot = [&](int k, int me) { return p.park + ((size_t)k * gridDim.x + blockIdx.x) * (size_t)BLOCK + (size_t)me; };
    auto opaque = [](int v) { asm volatile("" : "+v"(v)); return v; };
    auto park_store = [&](int me, const Path& P, const BestId& obest, const Pending& opend, unsigned omeshes, unsigned rays) {
        *park_slot(0, me) = make_float4(__int_as_float(P.item), __int_as_float(P.send), __uint_as_float(P.gxy), __int_as_float(P.s));
        *park_slot(1, me) = make_float4(__int_as_float(P.b), P.pdx, P.pdy, P.pdz);
        *park_slot(2, me) = make_float4(P.ray.ox, P.ray.oy, P.ray.oz, P.ray.dx);
        *park_slot(3, me) = make_float4(P.ray.dy, P.ray.dz, P.bx, P.by);
        *park_slot(4, me) = make_float4(P.bz, P.ax, P.ay, P.az);
        *park_slot(5, me) = make_float4(obest.dist, __int_as_float(obest.geom), __int_as_float(obest.rec), opend.dist);
        *park_slot(6, me) = make_float4(__int_as_float(opend.geom), __int_as_float(opend.rec), __uint_as_float(omeshes), __uint_as_float(rays));
    };
    {
        Path P0;
        init_path(P0);
        park_store(tid, P0, BestId{ kInf, -1, -1 }, Pending{ kInf, -1, -1 }, 0u, 0u);
    }
    bool more_meshes = false; // the lane's query has candidate meshes left (omeshes != 0)
    bool active = false, exhausted = false, inflight = false; // inflight: the lane has a query (begun, not yet shaded)
    bool waiting = false;                                     // ... and a job of it is out (queued, being walked, or handed back and not yet read)
    const bool reuse = p.primary_hits != nullptr; // every sample starts from its pixel's stored primary hit (trace_bvh_kernel)
    unsigned long long tphase[5] = { 0, 0, 0, 0, 0 };
    const unsigned long long wave_t0 = STATS ? wall_clock64() : 0ull;
    const int quorum = p.pool_quorum, qmin = p.pool_quorum_min;
    int starved = 0; // consecutive polls that found nothing to do
    // Watchdog: every loop of this kernel is bounded.  A wave that sleeps kPoolSpinLimit times in a row, or waits that long for a
    // queue entry, gives up: it reports through the guard counter (the host turns it into an error, as for the traversal loop
    // guard) and leaves, so a scheduling bug is a failed frame, not a hung GPU.
    bool stuck = false;
    int idle_polls = 0;
    // where the wave's time goes (every build: three stamps per turn of the loop, scalar): setup passes, the traverse role, the rest
    // (deciding, waiting); raw counters [16] [17] [18] and the number of setup passes / role visits in [11] [12]
    unsigned long long tw_setup = 0ull, tw_role = 0ull, tw_rest = 0ull, tw_mark = __builtin_amdgcn_s_memtime();
    unsigned n_setup = 0u, n_role = 0u;
    for (unsigned turns = 0;; ++turns) {
        (void)turns; // (counted, never read: what is left of a debug watchdog.  The loop compiles to other, equivalent code without the
                     // counter, and this kernel's machine code is kept as it was measured.)
        if (stuck || idle_polls > kPoolSpinLimit) {
            cnt.guard_hits |= 1ull;
            break;
        }
        // ---- what can this wave do? ----
        const int me_d = opaque(tid);
        bool returned = false;
        if (waiting) returned = (__hip_atomic_load(&pool_u32()[(Q.job_base + 2 * BLOCK + me_d) * 4 + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & kJobReturned) != 0u;
        const bool mine = returned || (!waiting && (inflight || active || !exhausted)); // lanes a setup pass would serve
        const int nready = __popcll(__ballot(mine));
        const unsigned queued = (unsigned)__builtin_amdgcn_readfirstlane((int)pool_waiting(Q));
        const bool any_waiting = __ballot(waiting) != 0ull;
        // What to do next.  A setup pass when enough lanes are ready for one; else a visit to the queue when it holds a batch worth
        // taking (pool_batch_min jobs: a wave that takes a handful walks them on a handful of lanes - and the inner-node phase is
        // back where the lane-owned kernel had it); else a setup pass for a smaller company (pool_quorum_min); else wait a moment
        // for the other waves to post or hand back - and after a few empty looks take whatever there is, ready lanes first, so that
        // nothing waits for ever.
        bool do_setup = nready >= quorum || (nready > 0 && !any_waiting && queued == 0u);
        bool do_role = !do_setup && queued >= (unsigned)p.pool_batch_min;
        if (!do_setup && !do_role) {
            if (nready == 0 && !any_waiting && queued == 0u) break; // nothing left for this wave: no work, no query, no job out, nothing to walk
            if (nready >= qmin || (nready > 0 && starved >= 4)) do_setup = true;
            else if (queued > 0u && starved >= 4) do_role = true;
            else {
                ++starved;
                ++idle_polls;
                __builtin_amdgcn_s_sleep(4);
                continue;
            }
        }
        starved = 0;
        idle_polls = 0;
        {
            const unsigned long long now = __builtin_amdgcn_s_memtime();
            tw_rest += now - tw_mark;
            tw_mark = now;
        }
        if (do_setup) {
            unsigned long long t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0;
            if (STATS) t0 = __builtin_amdgcn_s_memtime();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            const int me = opaque(tid);
            Path P;
            BestId obest;
            Pending opend;
            unsigned omeshes;
            {
                const float4 a0 = *park_slot(0, me), a1 = *park_slot(1, me), a2 = *park_slot(2, me), a3 = *park_slot(3, me), a4 = *park_slot(4, me), a5 = *park_slot(5, me),
                             a6 = *park_slot(6, me);
                P.item = __float_as_int(a0.x); P.send = __float_as_int(a0.y); P.gxy = __float_as_uint(a0.z); P.s = __float_as_int(a0.w);
                P.b = __float_as_int(a1.x); P.pdx = a1.y; P.pdy = a1.z; P.pdz = a1.w;
                P.ray.ox = a2.x; P.ray.oy = a2.y; P.ray.oz = a2.z; P.ray.dx = a2.w;
                P.ray.dy = a3.x; P.ray.dz = a3.y; P.bx = a3.z; P.by = a3.w;
                P.bz = a4.x; P.ax = a4.y; P.ay = a4.z; P.az = a4.w;
                obest.dist = a5.x; obest.geom = __float_as_int(a5.y); obest.rec = __float_as_int(a5.z); opend.dist = a5.w;
                opend.geom = __float_as_int(a6.x); opend.rec = __float_as_int(a6.y); omeshes = __float_as_uint(a6.z); cnt.rays = __float_as_uint(a6.w);
            }
            // -- jobs that came back: merge what they found; a near tie is resolved exactly and the job goes out again --
            bool repost = false;
            if (returned) {
                const uint4 c = ff_smem[Q.job_base + 2 * BLOCK + me];
                const int mesh = (int)((c.y >> 8) & 0xFFu);
                if ((int)c.w >= 0) {
                    opend.dist = __uint_as_float(c.z);
                    opend.geom = mesh;
                    opend.rec = (int)c.w;
                }
                waiting = false;
                repost = (c.y & kJobTie) != 0u;
            }
            if (__ballot(repost) != 0ull) {
                if (repost) {
                    HitPoint H;
                    resolve_pending(L, p.tris, P.ray, opend, obest, H);
                    // (the job's ray, cursor, stack height and leaf position are where the walk left them; the pending slot is empty now)
                    pool_u32()[(Q.job_base + BLOCK + me) * 4 + 3] = __float_as_uint(obest.dist);
                    unsigned* st = &pool_u32()[(Q.job_base + 2 * BLOCK + me) * 4];
                    st[1] = st[1] & ~(kJobReturned | kJobTie);
                    st[2] = __float_as_uint(kInf);
                    st[3] = (unsigned)kPendEmpty;
                    waiting = true;
                }
            }
            // Lanes whose query is complete (or that have none) resolve + shade + spawn together.
            const bool setup = mine && !waiting && !(inflight && omeshes != 0u);
            (void)more_meshes;
            Best best;
            bool hit = false;
            bool shade_now = setup && inflight;
            if (shade_now) {
                Segment S;
                S.best = obest;
                S.pend = opend;
                finish_segment(L, p.tris, P.ray, S, best);
                hit = best.geom >= 0;
            }
            bool from_cache = setup && !inflight && active && P.b == 0 && reuse;
            if (STATS) t1 = __builtin_amdgcn_s_memtime();
            bool settle_now = shade_now, goes_on = false;
            for (;;) {
                if (from_cache) {
                    const unsigned off = ((unsigned)P.item & kItemPixelMask) * 16u, plane = p.pix_items * 16u;
                    const char* stored = reinterpret_cast<const char*>(p.primary_hits);
                    const float4 c0 = *reinterpret_cast<const float4*>(stored + off), c1 = *reinterpret_cast<const float4*>(stored + (off + plane)),
                                 c2 = *reinterpret_cast<const float4*>(stored + (off + 2u * plane));
                    best.dist = c0.x; best.px = c0.y; best.py = c0.z; best.pz = c0.w;
                    best.cx = c1.x; best.cy = c1.y; best.cz = c1.z;
                    best.geom = __float_as_int(c1.w);
                    best.rec = __float_as_int(c2.x);
                    hit = best.geom >= 0;
                    cnt.rays += 1;
                    settle_now = true;
                }
                cnt.reused += (unsigned)__popcll(__ballot(from_cache));
                if (__ballot(settle_now) == 0ull) break;
                bool again = false;
                if (settle_now) {
                    MaterialRef M;
                    M.global = nullptr;
                    M.geom_base = L.geom_base;
                    M.g = best.geom;
                    const int r = settle_hit<EXTRAS>(p, best, hit, M, P);
                    inflight = false;
                    active = r != kPixelDone;
                    goes_on = r == kGoesOn;
                    again = r == kNewSample && reuse;
                }
                settle_now = false;
                from_cache = again && __popcll(__ballot(again)) >= p.reuse_quorum;
            }
            if (goes_on) {
                MaterialRef M;
                M.global = nullptr;
                M.geom_base = L.geom_base;
                M.g = best.geom;
                scatter<EXTRAS>(p, best, M, P);
            }
            if (STATS) t2 = __builtin_amdgcn_s_memtime();
            {
                const bool need = setup && !active && !exhausted;
                if (__ballot(need) != 0ull) {
                    const bool got = acquire_pixel(p, lane, P, WQ, need, cnt.rays);
                    if (need) {
                        active = got;
                        exhausted = !got;
                    }
                }
            }
            if (STATS) t3 = __builtin_amdgcn_s_memtime();
            // -- the next ray's query: planes first; a lane whose ray can reach a mesh enters it and posts the job --
            Segment S;
            S.cur = kDone;
            bool over = false;
            const bool begin = setup && active && !(P.b == 0 && reuse);
            if (begin) {
                if (STATS) probe_round(cnt.segment_rounds);
                over = begin_segment<STATS>(L, p.walls, p.geoms, p.num_geoms, p.num_planes, p.tris, P.ray, S, cnt, p.cut_last != 0 && P.b == p.bounces - 1, p.emitter_mask);
                cnt.rays += 1;
                inflight = true;
                obest = S.best;
                opend = S.pend;
                omeshes = S.meshes;
            }
            cnt.cut += (unsigned)__popcll(__ballot(over));
            // (a query that is going on - its last job came back without a tie - enters its next candidate mesh here as well)
            const bool enter = mine && inflight && !waiting && omeshes != 0u;
            bool post = false;
            if (enter) {
                S.best = obest;
                S.pend = opend;
                S.meshes = omeshes;
                S.cur = kDone;
                S.resume = 0;
                while (S.cur == kDone && S.meshes != 0u) start_next_mesh(L, P.ray, S);
                omeshes = S.meshes;
                if (S.cur != kDone) {
                    // (the pending candidate's identity stays here: the job only needs to know that there is one, and how far)
                    S.pend.rec = opend.geom >= 0 ? kPendOwner : kPendEmpty;
                    S.sp = 0;
                    job_write<BLOCK>(Q, me, S);
                    post = true;
                    waiting = true;
                }
            }
            pool_push(Q, lane, me, post || repost);
            more_meshes = omeshes != 0u;
            park_store(me, P, obest, opend, omeshes, cnt.rays);
            if (STATS) {
                t4 = __builtin_amdgcn_s_memtime();
                tphase[0] += t1 - t0; tphase[1] += t2 - t1; tphase[2] += t3 - t2; tphase[3] += t4 - t3;
            }
            {
                const unsigned long long now = __builtin_amdgcn_s_memtime();
                tw_setup += now - tw_mark;
                tw_mark = now;
                n_setup += 1u;
            }
            continue;
        }

        // ---- the traverse role (a function of its own: see pool_role) ----
        {
            unsigned long long t4 = 0;
            if (STATS) t4 = __builtin_amdgcn_s_memtime();
            const int me_r = opaque(tid);
            const bool nojob_ready = !waiting && (inflight || active || !exhausted);
            if (pool_role<STATS, BLOCK>(Q.job_base, me_r, waiting, nojob_ready, STATS ? &cnt : nullptr)) stuck = true;
            if (STATS) tphase[4] += __builtin_amdgcn_s_memtime() - t4;
            {
                const unsigned long long now = __builtin_amdgcn_s_memtime();
                tw_role += now - tw_mark;
                tw_mark = now;
                n_role += 1u;
            }
        }
    }
    if (STATS && lane == 0) {
        atomicAdd(&p.counters[4], tphase[0]);
        atomicAdd(&p.counters[5], tphase[1]);
        atomicAdd(&p.counters[6], tphase[2]);
        atomicAdd(&p.counters[7], tphase[3]);
        atomicAdd(&p.counters[13], tphase[4]);
        atomicMax(&p.counters[22], tphase[0] + tphase[1] + tphase[2] + tphase[3] + tphase[4]);
        atomicMax(&p.counters[24], ~(unsigned long long)wave_t0);
        atomicMax(&p.counters[25], (unsigned long long)wall_clock64());
    }
    flush_counters(p, lane, cnt, STATS);
    if (!STATS && lane == 0) {
        unsigned long long* t = reinterpret_cast<unsigned long long*>(&pool_u32()[Q.ctrl + 16]);
        __hip_atomic_fetch_add(&t[4], tw_setup, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(&t[5], tw_role, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(&t[6], tw_rest + (__builtin_amdgcn_s_memtime() - tw_mark), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(&t[7], (unsigned long long)n_setup | ((unsigned long long)n_role << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    if (!STATS) {
        // node visits and round counts of the production kernel (the instrumented build counts them per lane): raw counters [1], [8],
        // [9] and, for the lanes that held a leaf in a leaf phase, [14]
        __syncthreads();
        if (tid == 0) {
            const unsigned long long* t = reinterpret_cast<const unsigned long long*>(&pool_u32()[Q.ctrl + 16]);
            atomicAdd(&p.counters[8], t[0]);
            atomicAdd(&p.counters[1], t[1]);
            atomicAdd(&p.counters[9], t[2]);
            atomicAdd(&p.counters[14], t[3]);
            atomicAdd(&p.counters[16], t[4]);
            atomicAdd(&p.counters[17], t[5]);
            atomicAdd(&p.counters[18], t[6]);
            atomicAdd(&p.counters[11], t[7] & 0xFFFFFFFFull);
            atomicAdd(&p.counters[12], t[7] >> 32);
        }
    }
}

// ---- the brute-force mega-kernel (reference loop, validation path) ---------------------------------------------------

template <bool STATS>
__global__ __launch_bounds__(kBlockThreads) void trace_brute_kernel(const KParams p)
{
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    float4* batch = reinterpret_cast<float4*>(ff_smem); // triangle batch buffer
    Counters cnt = {};
    Path P;
    init_path(P);
    WaveQueue Q = make_wave_queue(p);
    bool active = false, exhausted = false;
    for (;;) {
        {
            const bool need = !active && !exhausted;
            if (__ballot(need) != 0ull) {
                const bool got = acquire_pixel(p, lane, P, Q, need, cnt.rays);
                if (need) {
                    active = got;
                    exhausted = !got;
                }
            }
        }
        // every thread of the workgroup takes part in staging the triangle batches
        if (__syncthreads_or(active ? 1 : 0) == 0) break;
        Best best;
        closest_hit_brute<STATS>(p.geoms, p.num_geoms, p.tris, batch, active, P.ray, best, cnt, p.trinormals);
        if (!active) continue;
        const bool hit = best.geom >= 0;
        MaterialRef M;
        M.global = hit ? &p.geoms[best.geom] : p.geoms;
        M.geom_base = 0;
        M.g = 0;
        active = shade_and_advance(p, best, hit, M, P);
    }
    flush_counters(p, lane, cnt, STATS);
}

// Batch closest-hit query: intersectRays (kernel.cu:127-176) for caller-supplied rays, one thread per ray.
template <int MODE, int BIG = 0>
__global__ __launch_bounds__(kBlockThreads) void ray_batch_kernel(const RayBatchParams p)
{
    const int tid = threadIdx.x;
    const LdsT<BIG> L = make_lds<BIG>(p.lds_nodes, p.stack_depth, kBlockThreads, tid, p.num_quads, nullptr, p.geoms, p.top_first, p.top_lds_first,
                                      p.top_lds_count, BIG ? p.num_scan : 0, p.stack_spill);
    const uint4* nodes4 = reinterpret_cast<const uint4*>(p.nodes4);
    if (MODE == FF_TRACE_BVH) stage_scene(L, nodes4, p.geoms, p.num_geoms, p.num_planes, tid, kBlockThreads);
    float4* batch = reinterpret_cast<float4*>(ff_smem);
    const int i = blockIdx.x * kBlockThreads + tid;
    const bool live = i < p.n;
    Ray wr = { 0.f, 0.f, 0.f, 0.f, 0.f, 1.f };
    if (live) {
        const FfRay r = p.rays[i];
        wr.ox = r.m_origin.x; wr.oy = r.m_origin.y; wr.oz = r.m_origin.z;
        wr.dx = r.m_direction.x; wr.dy = r.m_direction.y; wr.dz = r.m_direction.z;
    }
    Best best;
    best.dist = kInf; best.geom = -1; best.rec = -1; best.px = best.py = best.pz = 0.f; best.cx = best.cy = 0.f; best.cz = 1.f;
    Counters cnt = {};
    if (MODE == FF_TRACE_BRUTE_FORCE) closest_hit_brute<false>(p.geoms, p.num_geoms, p.tris, batch, live, wr, best, cnt);
    else if (live) closest_hit_deferred<false>(L, p.walls, p.geoms, p.num_geoms, p.num_planes, p.tris, nodes4, wr, best, cnt);
    if (live && ((cnt.guard_hits >> (threadIdx.x & 63)) & 1ull) != 0ull && p.guard_hits) atomicAdd(p.guard_hits, 1ull);
    if (!live) return;
    FfIntersect out;
    out.m_intersectionPoint.x = 0.f; out.m_intersectionPoint.y = 0.f; out.m_intersectionPoint.z = 0.f;
    out.m_normal.x = 0.f; out.m_normal.y = 0.f; out.m_normal.z = 0.f;
    out.m_t = 0.f;          // utilities.h:62
    out.m_hit = 0;          // :63
    out._pad[0] = out._pad[1] = out._pad[2] = 0;
    out.geometryIndex = -1; // :64
    out.triangleIndex = -1; // :65
    if (best.geom >= 0) {
        const GeomRecord& G = p.geoms[best.geom];
        MaterialRef M;
        M.global = &G;
        M.geom_base = L.geom_base;
        M.g = 0;
        float nx, ny, nz;
        world_normal(M, best, true, nx, ny, nz);
        out.m_intersectionPoint.x = best.px; out.m_intersectionPoint.y = best.py; out.m_intersectionPoint.z = best.pz;
        out.m_normal.x = nx; out.m_normal.y = ny; out.m_normal.z = nz;
        out.m_t = best.dist;   // kernel.cu:119: the world distance
        out.m_hit = 1;
        out.geometryIndex = G.orig_index;
        out.triangleIndex = best.rec >= 0 ? p.tris[best.rec].orig_index : -1;
    }
    p.out[i] = out;
}

} // namespace
} // namespace ff

// nee_path_kernel: a section of this unit and not a unit of its own
#include "ff_k_nee.h"

namespace ff {

#if defined(FF_PROBE) || defined(FF_PROBE_NEE)
// Register-pressure probes (tools/diag/probe_kernel.sh): compile ONE instantiation to ISA in a few seconds.
namespace {
#ifdef FF_PROBE
template __global__ void FF_PROBE(const KParams);
#else
template __global__ void FF_PROBE_NEE(const NeeParams); // (nee_path_kernel takes the frame's parameters plus the light tables)
#endif
}
#else
// (num_geoms: the records cached in LDS; 0 for scenes of more than 32 geometries, whose records stay in global memory)
size_t bvh_lds_bytes(int lds_nodes, int stack_depth, int block_threads, int num_geoms)
{
    return (size_t)lds_nodes * sizeof(Bvh4Node) + (size_t)stack_depth * (size_t)block_threads * sizeof(unsigned) +
           (size_t)num_geoms * sizeof(GeomRecord);
}

int max_lds_nodes(int stack_depth, int block_threads, int num_geoms, size_t reserve)
{
    const long avail = (long)kLdsBudgetBytes - (long)reserve - (long)stack_depth * (long)block_threads * (long)sizeof(unsigned) -
                       (long)num_geoms * (long)sizeof(GeomRecord);
    return avail > 0 ? (int)(avail / (long)sizeof(Bvh4Node)) : 0;
}

// The scene-size class BIG of the BVH kernels: 0 = up to kChunkGeometries geometries (records scanned in LDS), 1 = up to
// kMaxLdsRecords (tree over the geometries, records in LDS), 2 = more (records read from global memory).
static int scene_size_class(int num_geoms) { return num_geoms <= kChunkGeometries ? 0 : (num_geoms <= kMaxLdsRecords ? 1 : 2); }

// Dynamic LDS of a launch on a scene of class `big`: the BVH layout, or the brute-force kernels' triangle batch.
static size_t trace_lds_bytes(bool bvh, int lds_nodes, int stack_depth, int block_threads, int num_geoms, int big)
{
    return bvh ? bvh_lds_bytes(lds_nodes, stack_depth, block_threads, big == 2 ? 0 : num_geoms) : (size_t)kBruteBatchTris * sizeof(TriRecord);
}

// Does a scene of up to kChunkGeometries geometries need the full kernel (EXTRAS): non-quad planes or spheres, MIRROR / GLASS, smooth normals?
static bool needs_extras(const KParams& p) { return p.num_planes > p.num_quads || p.has_specular != 0 || p.trinormals != nullptr; }

// Only the BVH kernels go past the 64 KiB default (node cache + stacks + geometry records); the brute-force kernels
// use a 48 KiB batch buffer plus a little static LDS, and asking for 160 KiB on top of static LDS is rejected.
template <class K>
static hipError_t allow_full_lds(K* kernel)
{
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBudgetBytes);
}

// ---- launch tables ---------------------------------------------------------------------------------------------------
// Every kernel family has ONE list of its instantiations (an X-macro).  prepare_kernels walks the lists to raise each BVH
// instantiation's dynamic-LDS limit, and the family's launcher walks the same list to find the instantiation that matches the
// run-time key: what can be launched has its attribute, and a key outside the list is hipErrorInvalidValue.

// The instantiations of trace_bvh_kernel, X(STATS, BLOCK, EXTRAS, BIG, PREPASS, START, WN), for each workgroup size: the frame's kernel
// for scenes of up to kChunkGeometries geometries without and with extras and for the two classes of larger scenes (always with
// extras), with and without statistics; the pre-pass, one per scene class (the general kernel, no statistics); the kernel that runs
// on start records (diffuse small scenes); the two diffuse small-scene kernels once more on the scene's normal tables (WN).
// The reported name is "trace_bvh_kernel<STATS, BLOCK, EXTRAS, BIG, PREPASS>" - the five parameters there were before START, as
// tools and tests parse it - and START = true appends ", true"; the pre-pass reports one literal for all its instantiations.  WN does
// not show in the name: it is the same kernel of the frame, computing the same bits, with one chain of arithmetic taken out.
#define FF_TRACE_BVH_KERNELS_OF(X, B)                                                                                                                \
    X(false, B, false, 0, false, false, false) X(true, B, false, 0, false, false, false) X(false, B, true, 0, false, false, false)                   \
    X(true, B, true, 0, false, false, false) X(false, B, true, 1, false, false, false) X(true, B, true, 1, false, false, false)                      \
    X(false, B, true, 2, false, false, false) X(true, B, true, 2, false, false, false)                                                               \
    X(false, B, true, 0, true, false, false) X(false, B, true, 1, true, false, false) X(false, B, true, 2, true, false, false)                       \
    X(false, B, false, 0, false, true, false) X(true, B, false, 0, false, true, false)                                                               \
    X(false, B, false, 0, false, false, true) X(true, B, false, 0, false, false, true)                                                               \
    X(false, B, false, 0, false, true, true) X(true, B, false, 0, false, true, true)
#define FF_TRACE_BVH_KERNELS(X) FF_TRACE_BVH_KERNELS_OF(X, 512) FF_TRACE_BVH_KERNELS_OF(X, 768) FF_TRACE_BVH_KERNELS_OF(X, 1024)
#define FF_NAME_START_false ""
#define FF_NAME_START_true ", true"
// ... and of ray_batch_kernel, X(MODE, BIG).
#define FF_RAY_BATCH_KERNELS(X) X(FF_TRACE_BVH, 0) X(FF_TRACE_BVH, 1) X(FF_TRACE_BVH, 2) X(FF_TRACE_BRUTE_FORCE, 0)

// The instantiations of trace_pool_kernel, X(STATS, BLOCK, EXTRAS), reported as "trace_pool_kernel<STATS, BLOCK, EXTRAS>"
// (an experiment: only the workgroup size the production kernel runs is instantiated).
#define FF_TRACE_POOL_KERNELS(X) X(false, 1024, false) X(false, 1024, true) X(true, 1024, false) X(true, 1024, true)

// The instantiations of nee_path_kernel, X(MODE, BIG, ENV, TEX, GLOSSY, CAM, name tail): the sixteen feature combinations for each of
// BVH mode's three scene-size classes and for brute force (MODE 1 = FF_TRACE_BVH, 0 = FF_TRACE_BRUTE_FORCE).
// The reported name is "nee_path_kernel<MODE, BIG" plus as many of ENV, TEX, GLOSSY, CAM as reach the last one that is 1 - each
// parameter was added with a default of 0 and the older names stayed as tools and tests parse them - hence the tail column.
#define FF_NEE_KERNELS_OF(X, MODE, BIG)                                                                               \
    X(MODE, BIG, 0, 0, 0, 0, "")           X(MODE, BIG, 1, 0, 0, 0, ", 1")                                            \
    X(MODE, BIG, 0, 1, 0, 0, ", 0, 1")     X(MODE, BIG, 1, 1, 0, 0, ", 1, 1")                                         \
    X(MODE, BIG, 0, 0, 1, 0, ", 0, 0, 1")  X(MODE, BIG, 1, 0, 1, 0, ", 1, 0, 1")                                      \
    X(MODE, BIG, 0, 1, 1, 0, ", 0, 1, 1")  X(MODE, BIG, 1, 1, 1, 0, ", 1, 1, 1")                                      \
    X(MODE, BIG, 0, 0, 0, 1, ", 0, 0, 0, 1") X(MODE, BIG, 1, 0, 0, 1, ", 1, 0, 0, 1")                                 \
    X(MODE, BIG, 0, 1, 0, 1, ", 0, 1, 0, 1") X(MODE, BIG, 1, 1, 0, 1, ", 1, 1, 0, 1")                                 \
    X(MODE, BIG, 0, 0, 1, 1, ", 0, 0, 1, 1") X(MODE, BIG, 1, 0, 1, 1, ", 1, 0, 1, 1")                                 \
    X(MODE, BIG, 0, 1, 1, 1, ", 0, 1, 1, 1") X(MODE, BIG, 1, 1, 1, 1, ", 1, 1, 1, 1")
#define FF_NEE_KERNELS(X) FF_NEE_KERNELS_OF(X, 1, 0) FF_NEE_KERNELS_OF(X, 1, 1) FF_NEE_KERNELS_OF(X, 1, 2) FF_NEE_KERNELS_OF(X, 0, 0)
static_assert(FF_TRACE_BVH == 1 && FF_TRACE_BRUTE_FORCE == 0, "the MODE column and the reported names spell the trace modes as numerals");

hipError_t prepare_kernels()
{
    hipError_t e;
#define FF_X(STATS, B, EXTRAS, BIG, PREPASS, START, WN) \
    if ((e = allow_full_lds(&trace_bvh_kernel<STATS, B, EXTRAS, BIG, PREPASS, START, WN>)) != hipSuccess) return e;
    FF_TRACE_BVH_KERNELS(FF_X)
#undef FF_X
#define FF_X(STATS, B, EXTRAS) \
    if ((e = allow_full_lds(&trace_pool_kernel<STATS, B, EXTRAS>)) != hipSuccess) return e;
    FF_TRACE_POOL_KERNELS(FF_X)
#undef FF_X
#define FF_X(MODE, BIG) \
    if (MODE == FF_TRACE_BVH && (e = allow_full_lds(&ray_batch_kernel<MODE, BIG>)) != hipSuccess) return e;
    FF_RAY_BATCH_KERNELS(FF_X)
#undef FF_X
#define FF_X(MODE, BIG, ENV, TEX, GLOSSY, CAM, TAIL) \
    if (MODE == FF_TRACE_BVH && (e = allow_full_lds(&nee_path_kernel<MODE, BIG, ENV, TEX, GLOSSY, CAM>)) != hipSuccess) return e;
    FF_NEE_KERNELS(FF_X)
#undef FF_X
    return hipSuccess;
}

size_t pool_lds_bytes(int block_threads) { return (size_t)block_threads * 48 + (size_t)kPoolRing * 2 + 128; } // jobs, ring, [head, tail, -, -], the role's inputs, the workgroup's tallies

// (launch_trace sends scenes of up to kChunkGeometries geometries here, and workgroups of 1024 threads)
static hipError_t launch_pool(const KParams& p, bool collect_stats, int grid_blocks, int block_threads, hipStream_t stream, const char** kernel_name)
{
    const dim3 grid(grid_blocks), block(block_threads);
    const size_t lds = bvh_lds_bytes(p.lds_nodes, p.stack_depth, block_threads, p.num_geoms) + pool_lds_bytes(block_threads);
    const bool extras = needs_extras(p);
    const char* name = "";
#define FF_X(STATS, B, EXTRAS)                                                                                  \
    if (collect_stats == STATS && block_threads == B && extras == EXTRAS) {                                     \
        hipLaunchKernelGGL((trace_pool_kernel<STATS, B, EXTRAS>), grid, block, lds, stream, p);                 \
        name = "trace_pool_kernel<" #STATS ", " #B ", " #EXTRAS ">";                                            \
    } else
    FF_TRACE_POOL_KERNELS(FF_X) return hipErrorInvalidValue;
#undef FF_X
    if (kernel_name) *kernel_name = name;
    return hipGetLastError();
}

hipError_t launch_trace(const KParams& p, int trace_mode, bool collect_stats, int grid_blocks, int block_threads, hipStream_t stream,
                        const char** kernel_name, bool pool, bool prepass, bool start, bool world_normals)
{
    const dim3 grid(grid_blocks);
    const char* name = "";
    // (the pre-pass of a frame (KParams::primary_hits) runs the BVH kernels whatever the frame's trace mode)
    if (!prepass && trace_mode == FF_TRACE_BVH && pool && p.num_geoms <= kChunkGeometries && block_threads == 1024)
        return launch_pool(p, collect_stats, grid_blocks, block_threads, stream, kernel_name);
    if (prepass || trace_mode == FF_TRACE_BVH) {
        const dim3 block(block_threads);
        const int big = scene_size_class(p.num_geoms);
        const size_t lds = trace_lds_bytes(true, p.lds_nodes, p.stack_depth, block_threads, p.num_geoms, big);
        if (!prepass && start && (big != 0 || needs_extras(p) || p.start_records == nullptr)) return hipErrorInvalidValue; // (the host asks for it on diffuse small scenes only)
        // the key of the instantiation: the pre-pass has one per workgroup size and scene size, the general one; larger scenes always run the full kernel
        const int threads = block_threads == 1024 ? 1024 : (block_threads == 768 ? 768 : 512);
        const bool stats = !prepass && collect_stats, extras = prepass || big != 0 || needs_extras(p), from_start = !prepass && start;
        // (the normal tables serve the kernels without the extras, on path frames: the reference's own shade wants the object-space normal)
        const bool wn = world_normals && !extras && p.shade_mode == FF_SHADE_DIFFUSE_PATH && p.tri_world_normals != nullptr && p.geom_world_normals != nullptr;
#define FF_X(STATS, B, EXTRAS, BIG, PREPASS, START, WN)                                                                                              \
    if (stats == STATS && threads == B && extras == EXTRAS && big == BIG && prepass == PREPASS && from_start == START && wn == WN) {                 \
        hipLaunchKernelGGL((trace_bvh_kernel<STATS, B, EXTRAS, BIG, PREPASS, START, WN>), grid, block, lds, stream, p);                              \
        name = "trace_bvh_kernel<" #STATS ", " #B ", " #EXTRAS ", " #BIG ", " #PREPASS FF_NAME_START_##START ">";                                    \
    } else
        FF_TRACE_BVH_KERNELS(FF_X) return hipErrorInvalidValue;
#undef FF_X
        if (prepass) name = "trace_bvh_kernel<false, B, true, big, true>"; // (the frame's own launches name their kernel exactly; nobody asks for this one)
    } else {
        const size_t lds = (size_t)kBruteBatchTris * sizeof(TriRecord);
        const dim3 block(kBlockThreads);
        if (collect_stats) hipLaunchKernelGGL((trace_brute_kernel<true>), grid, block, lds, stream, p);
        else hipLaunchKernelGGL((trace_brute_kernel<false>), grid, block, lds, stream, p);
        name = collect_stats ? "trace_brute_kernel<true>" : "trace_brute_kernel<false>";
    }
    if (kernel_name) *kernel_name = name;
    return hipGetLastError();
}

hipError_t launch_ray_batch(const RayBatchParams& p, int trace_mode, hipStream_t stream)
{
    if (p.n <= 0) return hipSuccess;
    const bool bvh = trace_mode == FF_TRACE_BVH;
    const int mode = bvh ? FF_TRACE_BVH : FF_TRACE_BRUTE_FORCE, big = scene_size_class(p.num_geoms), big_key = bvh ? big : 0;
    const size_t lds = trace_lds_bytes(bvh, p.lds_nodes, p.stack_depth, kBlockThreads, p.num_geoms, big);
    const dim3 grid((p.n + kBlockThreads - 1) / kBlockThreads), block(kBlockThreads);
#define FF_X(MODE, BIG) \
    if (mode == MODE && big_key == BIG) hipLaunchKernelGGL((ray_batch_kernel<MODE, BIG>), grid, block, lds, stream, p); else
    FF_RAY_BATCH_KERNELS(FF_X) return hipErrorInvalidValue;
#undef FF_X
    return hipGetLastError();
}

hipError_t launch_nee(const NeeParams& np, int trace_mode, bool env, bool tex, bool glossy, int grid_blocks, hipStream_t stream, const char** kernel_name)
{
    if (np.items == 0u) return hipSuccess;
    const KParams& p = np.k;
    const bool bvh = trace_mode == FF_TRACE_BVH, cam = np.cam_active != 0; // (cam: per-sample camera rays)
    const int mode = bvh ? 1 : 0, big = scene_size_class(p.num_geoms), big_key = bvh ? big : 0;
    const size_t lds = trace_lds_bytes(bvh, p.lds_nodes, p.stack_depth, kBlockThreads, p.num_geoms, big);
    const dim3 grid(grid_blocks), block(kBlockThreads);
    const char* name = "";
#define FF_X(MODE, BIG, ENV, TEX, GLOSSY, CAM, TAIL)                                                                  \
    if (mode == MODE && big_key == BIG && env == (ENV != 0) && tex == (TEX != 0) && glossy == (GLOSSY != 0) && cam == (CAM != 0)) { \
        hipLaunchKernelGGL((nee_path_kernel<MODE, BIG, ENV, TEX, GLOSSY, CAM>), grid, block, lds, stream, np);        \
        name = "nee_path_kernel<" #MODE ", " #BIG TAIL ">";                                                           \
    } else
    FF_NEE_KERNELS(FF_X) return hipErrorInvalidValue;
#undef FF_X
    if (kernel_name) *kernel_name = name;
    return hipGetLastError();
}

#endif // FF_PROBE
} // namespace ff
