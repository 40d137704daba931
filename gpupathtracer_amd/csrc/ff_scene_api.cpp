// ff_scene_api.cpp — the scene on the device behind the C ABI (include/firefly/ff_api.h): upload with the host or a device builder,
// transform and mesh updates, the LDS layout every change of the scene ends with (finalize_layout), and the scene's getters.  Host
// side of the seam the reference has at kernel.cu:268-298; the compilation itself is ff_scene.cpp, the builders ff_build.hip.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "ff_state.h"

using namespace ff;

namespace ff {

void free_scene(FfState* s)
{
    s->primary_valid = s->last_key_valid = false;
    if (s->d_geoms) (void)hipFree(s->d_geoms);
    if (s->d_tris) (void)hipFree(s->d_tris);
    if (s->d_normals) (void)hipFree(s->d_normals);
    if (s->d_world_normals) (void)hipFree(s->d_world_normals);
    if (s->d_uvs) (void)hipFree(s->d_uvs);
    if (s->d_nodes) (void)hipFree(s->d_nodes);
    if (s->d_nodes4) (void)hipFree(s->d_nodes4);
    s->top_count = s->top_depth = 0;
    s->num_scan = 0;
    if (s->d_parent) (void)hipFree(s->d_parent);
    if (s->d_role) (void)hipFree(s->d_role);
    s->d_nodes4 = nullptr;
    s->num_nodes4 = s->max_depth4 = 0;
    s->scene_block_threads = s->lds_cap = 0;
    s->d_geoms = nullptr;
    s->d_tris = nullptr;
    s->d_normals = nullptr;
    s->d_world_normals = nullptr;
    s->d_uvs = nullptr;
    s->d_nodes = nullptr;
    s->d_parent = nullptr;
    s->d_role = nullptr;
    s->h_geoms.clear();
    s->slots.clear();
    s->node_capacity = 0;
    s->has_scene = false;
    s->num_geoms = s->num_nodes = s->max_depth = 0;
    s->num_tris = 0;
}

} // namespace ff

namespace {

double ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// hipMalloc for the scene arrays (with the test hook FfState::alloc_countdown).
hipError_t scene_alloc(FfState* s, void** ptr, size_t bytes)
{
    if (s->alloc_countdown >= 0 && s->alloc_countdown-- == 0) {
        *ptr = nullptr;
        return hipErrorOutOfMemory;
    }
    return hipMalloc(ptr, bytes);
}

// The normal tables of a scene of `geoms` records and `tris` triangle records (FfState::d_world_normals): the scenes whose frames can
// run the kernels that read them.
hipError_t alloc_world_normals(FfState* s, size_t geoms, size_t tris)
{
    if (geoms > (size_t)kChunkGeometries) return hipSuccess;
    return scene_alloc(s, (void**)&s->d_world_normals, (tris + geoms) * sizeof(float4));
}

// Workgroup size of the BVH kernel for the uploaded scene: the preferred size if the lane-strided traversal stacks
// (4 bytes x workgroup size per tree level) and the geometry records fit the 160 KiB of LDS, else the largest smaller
// instantiation that does; 0 if even 512 threads do not fit (a degenerate, chain-like device-built tree).
int bvh_block_threads(const FfState* s, int preferred, int stack_levels)
{
    const int sizes[3] = { 1024, 768, 512 };
    for (int b : sizes) {
        if (b > preferred) continue;
        if (bvh_lds_bytes(0, stack_levels, b, lds_records(s)) + (s->use_pool ? pool_lds_bytes(b) : 0) <= (size_t)kLdsBudgetBytes) return b;
    }
    return 0;
}

// After every change of the trees (upload, rebuild) or of the records (transform update): choose the BVH kernel's
// workgroup size for the scene, divide the LDS node slots among the meshes (each mesh caches the top of its 4-wide tree:
// its first lds_nodes nodes) and write that into the geometry records, then copy the records to the device.
int finalize_layout(FfState* s)
{
    int nodes4 = 0, depth4 = 0;
    for (size_t i = 0; i < s->slots.size(); ++i) {
        if (s->h_geoms[i].type != FF_GEOM_TRIANGLEMESH || s->slots[i].node4_count == 0) continue;
        nodes4 += s->slots[i].node4_count;
        depth4 = std::max(depth4, s->slots[i].depth4);
    }
    s->num_nodes4 = nodes4;
    s->max_depth4 = depth4;
    // Scenes of more than kChunkGeometries geometries: the tree over the geometries' world boxes (rebuilt here because
    // transforms and refits move those boxes; a few hundred records take microseconds).
    // It lives behind the meshes' trees in the 4-wide node array (the upload reserved num_geoms nodes there).
    s->top_count = s->top_depth = 0;
    if (s->num_geoms > kChunkGeometries) {
        std::vector<BvhNode> top2;
        std::vector<Bvh4Node> top4;
        s->num_scan = s->sw.no_scan_planes ? 0 : count_scan_planes(s->h_geoms, s->num_quads);
        build_geometry_tree(s->h_geoms, top2, s->num_scan);
        s->top_depth = collapse_geometry_tree(top2, top4);
        s->top_count = (int)top4.size();
        if (top4.size() > (size_t)s->num_geoms) return fail(FF_ERR_HIP, "geometry tree of %zu nodes for %d geometries", top4.size(), s->num_geoms);
        FF_HIP(hipMemcpyAsync(s->d_nodes4 + s->node_capacity, top4.data(), top4.size() * sizeof(Bvh4Node), hipMemcpyHostToDevice, s->stream));
        FF_HIP(hipStreamSynchronize(s->stream)); // (`top4` goes out of scope)
    }
    // the axis-aligned walls among the planes every query screens (all planes of a small scene, the leading num_scan of a big one)
    build_wall_table(s->h_geoms.data(), s->sw.no_wall_table ? 0 : (s->num_geoms > kChunkGeometries ? s->num_scan : s->num_quads), s->walls, !s->sw.no_wall_pairs);
    if (s->num_geoms <= kChunkGeometries) add_mesh_boxes(s->h_geoms.data(), s->num_planes, s->num_geoms, s->walls);
    // one entry per visited node above the cursor (inner_step) plus a spare; in big scenes the pending entries of the
    // geometry tree sit below a mesh's own
    s->stack_entries = depth4 + 1 + (s->top_depth > 0 ? s->top_depth + 1 : 0);
    if (!s->setup_threshold_forced) {
        // Traversal time slice, in inner-node rounds (trace_bvh_kernel): long enough for most queries of the scene's biggest
        // tree to finish inside one slice.  Measured best on one MI355X (round 3's kernel, profiles/r03_r_slice_sweep.txt): 7 for C2
        // (1 200 nodes), 12 for the 983 040-triangle sphere (180 000 nodes); both sit on 1.5 log4(nodes) - 0.7.
        int biggest = 1;
        for (size_t i = 0; i < s->slots.size(); ++i) biggest = std::max(biggest, s->slots[i].node4_count);
        s->setup_threshold = std::max(4, std::min(24, (int)std::lround(1.5 * std::log((double)biggest) / std::log(4.0) - 0.7)));
        s->setup_threshold = std::min(32, s->setup_threshold + 2 * s->top_depth); // big scenes: plus the walk through the geometry tree
    }
    // The job-pool kernel (trace_pool_kernel; scenes of up to kChunkGeometries geometries) parks its traversal jobs in LDS: 48 bytes
    // per thread + the queue, taken off the node cache.  Its stacks keep a fixed few levels in LDS whether or not the trees fit
    // (kPoolStackLevels; the deeper entries go to the global spill area): with the jobs in LDS a tree of more than a few hundred
    // nodes does not fit anyway, and a level costs 36 nodes.
    s->use_pool = s->sw.pool > 0 && s->num_geoms <= kChunkGeometries && nodes4 > 0; // (FF_POOL=1; the library's own choice is the lane-owned kernel until the pool kernel beats it)
    constexpr int kPoolStackLevels = 5;
    const int pool_levels = std::min(s->stack_entries, s->sw.pool_stack_levels > 0 ? s->sw.pool_stack_levels : kPoolStackLevels);
    s->scene_block_threads = bvh_block_threads(s, s->block_threads, s->use_pool ? pool_levels : s->stack_entries);
    if (s->use_pool && s->scene_block_threads != 1024) { // (the experiment is instantiated for 1 024 threads only)
        s->use_pool = false;
        s->scene_block_threads = bvh_block_threads(s, s->block_threads, s->stack_entries);
    }
    // (a tree too deep even for 512 threads still uploads: brute-force rendering works, BVH rendering reports it)
    const int block = s->scene_block_threads > 0 ? s->scene_block_threads : kBlockThreads;
    // LDS holds tree nodes and the lanes' traversal stacks.  A stack level costs 4 bytes x workgroup size = 36 nodes at 1 024
    // threads, and the deepest levels are hardly ever reached: when the scene's trees would fit LDS whole but for the stacks, the
    // stacks keep as many levels as are left (at least kMinLdsStack) and the deeper entries go to global memory (stack_push /
    // stack_pop).  The benchmark scene: 1 202 nodes + 5 of 11 levels instead of 1 040 nodes + 11 levels; a node fetched from
    // global memory costs a query hundreds of cycles, a spilled stack entry is rare.  Trees that do not fit anyway keep the
    // whole stack in LDS.
    constexpr int kMinLdsStack = 4;
    const size_t reserve = s->use_pool ? pool_lds_bytes(block) : 0;
    s->stack_lds_levels = s->stack_entries;
    if (s->use_pool) {
        s->stack_lds_levels = pool_levels;
        // (where everything fits with more levels, take them)
        while (s->stack_lds_levels < s->stack_entries && max_lds_nodes(s->stack_lds_levels + 1, block, lds_records(s), reserve) >= nodes4) ++s->stack_lds_levels;
    } else if (s->scene_block_threads > 0 && !s->sw.no_stack_spill) {
        const int want = nodes4 + s->top_count;
        if (want > max_lds_nodes(s->stack_entries, block, lds_records(s))) {
            int levels = s->stack_entries;
            while (levels > kMinLdsStack && max_lds_nodes(levels, block, lds_records(s)) < want) --levels;
            if (max_lds_nodes(levels, block, lds_records(s)) >= want) s->stack_lds_levels = levels;
        }
    }
    int cap = s->scene_block_threads > 0 ? std::max(0, max_lds_nodes(s->stack_lds_levels, block, lds_records(s), reserve)) : 0;
    if (s->sw.lds_node_cap >= 0) cap = std::min(cap, s->sw.lds_node_cap); // FF_DEBUG_LDS_NODE_CAP: experiments on partial residency
    s->lds_cap = std::min(cap, nodes4 + s->top_count);
    // the geometry tree first (every query of a big scene starts there), the meshes share the rest
    s->top_lds_count = std::min(s->top_count, cap);
    const int mesh_cap = cap - s->top_lds_count;
    // Every mesh first gets the top of its tree up to kSmallTree nodes (a crowd of small objects: their whole trees; a query
    // that enters one must not pay a global fetch for a three-node tree), then the big trees share what is left in proportion
    // to their sizes.
    constexpr int kSmallTree = 8;
    std::vector<int> share(s->h_geoms.size(), 0);
    int left = mesh_cap, wanting = 0;
    for (size_t i = 0; i < s->h_geoms.size(); ++i) {
        if (s->h_geoms[i].type != FF_GEOM_TRIANGLEMESH || s->slots[i].node4_count == 0) continue;
        share[i] = std::min(std::min(s->slots[i].node4_count, kSmallTree), left);
        left -= share[i];
        wanting += s->slots[i].node4_count - share[i];
    }
    const int pool = left;
    for (size_t i = 0; i < s->h_geoms.size() && wanting > 0; ++i) {
        if (s->h_geoms[i].type != FF_GEOM_TRIANGLEMESH || s->slots[i].node4_count == 0) continue;
        const int want = s->slots[i].node4_count - share[i];
        share[i] += wanting <= pool ? want : (int)((int64_t)pool * want / wanting);
    }
    int next = s->top_lds_count;
    for (size_t i = 0; i < s->h_geoms.size(); ++i) {
        GeomRecord& r = s->h_geoms[i];
        r.node4_first = 0;
        r.lds_nodes = 0;
        r.wmin[3] = 0.0f;
        if (r.type != FF_GEOM_TRIANGLEMESH || s->slots[i].node4_count == 0) continue;
        r.node4_first = s->slots[i].node_first;
        r.lds_nodes = std::min(s->slots[i].node4_count, share[i]);
        std::memcpy(&r.wmin[3], &next, sizeof(int));
        next += r.lds_nodes;
    }
    FF_HIP(hipMemcpyAsync(s->d_geoms, s->h_geoms.data(), s->h_geoms.size() * sizeof(GeomRecord), hipMemcpyHostToDevice, s->stream));
    // The normal tables follow the records and the triangle records just written (behind the builders and the refit on the stream): a
    // transform moves every normal of its geometry, a mesh update the mesh's own.  All of them, each time: one short launch (16 bytes
    // written per triangle), and no bookkeeping of what moved.
    if (s->d_world_normals) {
        int max_tris = 0;
        for (const GeomRecord& g : s->h_geoms) max_tris = std::max(max_tris, g.type == FF_GEOM_TRIANGLEMESH ? g.tri_count : 0);
        FF_HIP(launch_world_normals(s->d_geoms, s->d_tris, s->num_geoms, max_tris, s->d_world_normals, s->d_world_normals + s->num_tris, s->stream));
    }
    FF_HIP(hipStreamSynchronize(s->stream));
    return FF_OK;
}

// Derive mesh slot `gi`'s 4-wide tree from its binary tree (after a build: with_info, one stream synchronisation; after a
// refit: boxes only, asynchronous).
int collapse_slot(FfState* s, size_t gi, bool with_info)
{
    FfState::MeshSlot& slot = s->slots[gi];
    if (slot.node_count <= 0) return FF_OK;
    int st = FF_OK;
    if (!slot.parents_linked) {
        st = gpu_link_parents(s->stream, s->d_nodes, slot.node_first, slot.node_count, s->d_parent + slot.node_first);
        if (st != FF_OK) return st;
        slot.parents_linked = true;
    }
    Collapse4Info info;
    st = gpu_collapse_mesh(s->stream, s->scratch, s->d_nodes, slot.node_first, slot.node_count, s->d_parent + slot.node_first, s->d_nodes4, slot.node_first, s->d_role + slot.node_first,
                           with_info ? &info : nullptr);
    if (st != FF_OK) return st;
    if (with_info) {
        if (info.node_count >= (1 << 22)) return fail(FF_ERR_UNSUPPORTED, "a mesh's tree has %d 4-wide nodes; the traversal stack encodes at most %d", info.node_count, (1 << 22) - 1);
        slot.node4_count = info.node_count;
        slot.depth4 = info.depth;
    }
    return FF_OK;
}

// Copy a caller triangle array into the device staging buffer (input of the device builder and of refit).
int stage_triangles(FfState* s, const FfTriangle* tris, int count, double* copy_ms)
{
    const auto t0 = std::chrono::steady_clock::now();
    int st = ensure_bytes((void**)&s->d_stage, &s->stage_bytes, (size_t)count * sizeof(FfTriangle));
    if (st != FF_OK) return st;
    FF_HIP(hipMemcpyAsync(s->d_stage, tris, (size_t)count * sizeof(FfTriangle), hipMemcpyHostToDevice, s->stream));
    FF_HIP(hipStreamSynchronize(s->stream));
    *copy_ms += ms_since(t0);
    return FF_OK;
}

// Leaf size of the device builders: subtrees of up to this many triangles collapse into one leaf (FF_GPU_LEAF overrides).
int device_leaf_tris(const BvhBuildParams& bp)
{
    int v = bp.device_leaf_tris;
    if (const char* e = std::getenv("FF_GPU_LEAF")) v = std::atoi(e);
    return std::max(1, std::min(bp.max_leaf_tris, v));
}

// A mesh that fits one leaf: the host builder's single node, re-based into the device arrays.
int place_single_leaf_mesh(FfState* s, const FfTriangle* tris, int count, const BvhBuildParams& bp, int tri_first, int node_base, int* out_nodes, int* out_depth)
{
    std::vector<BvhNode> tn;
    std::vector<TriRecord> tt;
    std::vector<TriNormals> nn;
    std::vector<TriUVs> uu;
    int depth = 0;
    build_mesh_bvh(tris, count, bp, tn, tt, &depth, &nn, &uu);
    for (BvhNode& nd : tn) {
        int* links[2] = { &nd.left, &nd.right };
        for (int* l : links) {
            if (*l >= 0) {
                *l += node_base;
            } else {
                const int ref = ~*l;
                *l = ~((((ref >> 3) + tri_first) << 3) | (ref & 7));
            }
        }
    }
    FF_HIP(hipMemcpy(s->d_nodes + node_base, tn.data(), tn.size() * sizeof(BvhNode), hipMemcpyHostToDevice));
    FF_HIP(hipMemcpy(s->d_tris + tri_first, tt.data(), tt.size() * sizeof(TriRecord), hipMemcpyHostToDevice));
    FF_HIP(hipMemcpy(s->d_normals + tri_first, nn.data(), nn.size() * sizeof(TriNormals), hipMemcpyHostToDevice));
    FF_HIP(hipMemcpy(s->d_uvs + tri_first, uu.data(), uu.size() * sizeof(TriUVs), hipMemcpyHostToDevice));
    *out_nodes = (int)tn.size();
    *out_depth = depth;
    return FF_OK;
}

void refresh_scene_extent(FfState* s)
{
    int end = 0, depth = 0;
    for (size_t i = 0; i < s->slots.size(); ++i) {
        if (s->h_geoms[i].type != FF_GEOM_TRIANGLEMESH || s->slots[i].node_count == 0) continue;
        end = std::max(end, s->slots[i].node_first + s->slots[i].node_count);
        depth = std::max(depth, s->slots[i].depth);
    }
    s->num_nodes = end;
    s->max_depth = depth;
    s->build_stats.builder = s->scene_builder;
    s->build_stats.bvh_nodes = end;
    s->build_stats.bvh_max_depth = depth;
    s->build_stats.num_triangles = s->num_tris;
}

int upload_with_device_builder(FfState* s, const FfGeometry* host_geometries, int n, const BvhBuildParams& bp)
{
    FfBuildStats& bs = s->build_stats;
    CompiledScene cs;
    int st = compile_scene(host_geometries, n, bp, cs, /*build_bvh=*/false);
    if (st != FF_OK) return st;
    FF_HIP(hipSetDevice(s->device));
    free_scene(s);
    s->alloc_countdown = s->debug_fail_alloc;
    const int device_leaf = device_leaf_tris(bp);
    size_t node_cap = 0;
    for (const GeomRecord& g : cs.geoms)
        if (g.type == FF_GEOM_TRIANGLEMESH && g.tri_count > 0) node_cap += gpu_build_max_nodes(g.tri_count);
    FF_HIP(scene_alloc(s, (void**)&s->d_geoms, cs.geoms.size() * sizeof(GeomRecord)));
    FF_HIP(scene_alloc(s, (void**)&s->d_tris, (cs.total_tris ? (size_t)cs.total_tris : 1) * sizeof(TriRecord)));
    FF_HIP(scene_alloc(s, (void**)&s->d_normals, (cs.total_tris ? (size_t)cs.total_tris : 1) * sizeof(TriNormals)));
    FF_HIP(alloc_world_normals(s, cs.geoms.size(), (size_t)cs.total_tris));
    FF_HIP(hipMalloc((void**)&s->d_uvs, (cs.total_tris ? (size_t)cs.total_tris : 1) * sizeof(TriUVs)));
    FF_HIP(scene_alloc(s, (void**)&s->d_nodes, (node_cap ? node_cap : 1) * sizeof(BvhNode)));
    // (the kernels address a node by a 32-bit byte offset from the array's base)
    if ((uint64_t)(node_cap + cs.geoms.size() + 1) * sizeof(Bvh4Node) >= (1ull << 32))
        return fail(FF_ERR_UNSUPPORTED, "scene needs %llu 4-wide BVH nodes: more than the 38 million (4 GiB) the kernels address", (unsigned long long)(node_cap + cs.geoms.size() + 1));
    FF_HIP(scene_alloc(s, (void**)&s->d_nodes4, (node_cap + cs.geoms.size() + 1) * sizeof(Bvh4Node))); // (+ the geometry tree of a big scene)
    FF_HIP(scene_alloc(s, (void**)&s->d_parent, (node_cap ? node_cap : 1) * sizeof(int)));
    FF_HIP(scene_alloc(s, (void**)&s->d_role, node_cap ? node_cap : 1));
    s->node_capacity = node_cap;
    s->slots.assign(cs.geoms.size(), FfState::MeshSlot());
    int node_base = 0;
    for (size_t gi = 0; gi < cs.geoms.size(); ++gi) {
        GeomRecord& r = cs.geoms[gi];
        if (r.type != FF_GEOM_TRIANGLEMESH || r.tri_count <= 0) continue;
        const FfTriangle* src = host_geometries[r.orig_index].m_triangles;
        FfState::MeshSlot& slot = s->slots[gi];
        slot.node_first = node_base;
        slot.node_capacity = (int)gpu_build_max_nodes(r.tri_count);
        if (r.tri_count <= device_leaf) {
            st = place_single_leaf_mesh(s, src, r.tri_count, bp, r.tri_first, node_base, &slot.node_count, &slot.depth);
            if (st != FF_OK) return st;
        } else {
            st = stage_triangles(s, src, r.tri_count, &bs.copy_ms);
            if (st != FF_OK) return st;
            const auto t0 = std::chrono::steady_clock::now();
            MeshBuildInfo info;
            st = gpu_build_mesh(s->stream, s->scratch, s->d_stage, r.tri_count, r.tri_first, node_base, device_leaf, s->d_tris, s->d_normals, s->d_uvs, s->d_nodes, &info,
                                s->builder == FF_BUILD_GPU_PLOC);
            if (st != FF_OK) return st;
            FF_HIP(hipStreamSynchronize(s->stream));
            bs.build_ms += ms_since(t0);
            slot.node_count = info.node_count;
            slot.depth = info.depth;
        }
        {
            const auto t0 = std::chrono::steady_clock::now();
            st = collapse_slot(s, gi, /*with_info=*/true);
            if (st != FF_OK) return st;
            bs.build_ms += ms_since(t0);
        }
        r.bvh_root = node_base;
        node_base += slot.node_capacity;
    }
    s->h_geoms = cs.geoms;
    s->num_geoms = (int)cs.geoms.size();
    s->num_planes = s->num_quads = 0;
    for (const GeomRecord& g : cs.geoms) {
        s->num_planes += g.type != FF_GEOM_TRIANGLEMESH ? 1 : 0; // analytic shapes lead the records: planes, then spheres
        s->num_quads += g.type == FF_GEOM_PLANE ? 1 : 0;
    }
    s->has_specular = false;
    for (const GeomRecord& g : cs.geoms) s->has_specular = s->has_specular || g.bxdf_type == FF_BXDF_MIRROR || g.bxdf_type == FF_BXDF_GLASS;
    s->num_tris = cs.total_tris;
    s->scene_builder = s->builder;
    refresh_scene_extent(s);
    st = finalize_layout(s);
    if (st != FF_OK) return st;
    s->has_scene = true;
    return FF_OK;
}

// A scene compiled on the host (records, triangle records in leaf order, binary trees) onto the state's device: the copies,
// then the 4-wide trees derived there.  The same compiled scene may go to several devices (ff_multi_upload_scene).
int upload_compiled(FfState* s, const CompiledScene& cs)
{
    int st = FF_OK;
    FF_HIP(hipSetDevice(s->device));
    free_scene(s);
    s->alloc_countdown = s->debug_fail_alloc;
    const auto t_copy = std::chrono::steady_clock::now();
    // One allocation + one copy per array (the reference issues a cudaMallocManaged + two cudaMemcpy per geometry, kernel.cu:277-298).
    FF_HIP(scene_alloc(s, (void**)&s->d_geoms, cs.geoms.size() * sizeof(GeomRecord)));
    // Keep the triangle / node arrays non-null so the kernels can form addresses even for plane-only scenes.
    const size_t tri_bytes = (cs.tris.size() ? cs.tris.size() : 1) * sizeof(TriRecord);
    const size_t node_bytes = (cs.nodes.size() ? cs.nodes.size() : 1) * sizeof(BvhNode);
    FF_HIP(scene_alloc(s, (void**)&s->d_tris, tri_bytes));
    FF_HIP(scene_alloc(s, (void**)&s->d_normals, tri_bytes));
    FF_HIP(alloc_world_normals(s, cs.geoms.size(), cs.tris.size()));
    static_assert(sizeof(TriNormals) == sizeof(TriRecord), "parallel arrays of equal stride");
    if (!cs.normals.empty()) FF_HIP(hipMemcpy(s->d_normals, cs.normals.data(), cs.normals.size() * sizeof(TriNormals), hipMemcpyHostToDevice));
    FF_HIP(hipMalloc((void**)&s->d_uvs, (cs.uvs.size() ? cs.uvs.size() : 1) * sizeof(TriUVs)));
    if (!cs.uvs.empty()) FF_HIP(hipMemcpy(s->d_uvs, cs.uvs.data(), cs.uvs.size() * sizeof(TriUVs), hipMemcpyHostToDevice));
    FF_HIP(scene_alloc(s, (void**)&s->d_nodes, node_bytes));
    // (the kernels address a node by a 32-bit byte offset from the array's base)
    if ((uint64_t)(cs.nodes.size() + cs.geoms.size() + 1) * sizeof(Bvh4Node) >= (1ull << 32))
        return fail(FF_ERR_UNSUPPORTED, "scene needs %llu 4-wide BVH nodes: more than the 38 million (4 GiB) the kernels address", (unsigned long long)(cs.nodes.size() + cs.geoms.size() + 1));
    FF_HIP(scene_alloc(s, (void**)&s->d_nodes4, (cs.nodes.size() + cs.geoms.size() + 1) * sizeof(Bvh4Node))); // (+ the geometry tree of a big scene)
    FF_HIP(scene_alloc(s, (void**)&s->d_parent, (cs.nodes.size() ? cs.nodes.size() : 1) * sizeof(int)));
    FF_HIP(scene_alloc(s, (void**)&s->d_role, cs.nodes.size() ? cs.nodes.size() : 1));
    if (!cs.tris.empty()) FF_HIP(hipMemcpy(s->d_tris, cs.tris.data(), cs.tris.size() * sizeof(TriRecord), hipMemcpyHostToDevice));
    if (!cs.nodes.empty()) FF_HIP(hipMemcpy(s->d_nodes, cs.nodes.data(), cs.nodes.size() * sizeof(BvhNode), hipMemcpyHostToDevice));
    s->build_stats.copy_ms = ms_since(t_copy);
    s->num_geoms = (int)cs.geoms.size();
    s->num_planes = s->num_quads = 0;
    for (const GeomRecord& g : cs.geoms) {
        s->num_planes += g.type != FF_GEOM_TRIANGLEMESH ? 1 : 0; // analytic shapes lead the records: planes, then spheres
        s->num_quads += g.type == FF_GEOM_PLANE ? 1 : 0;
    }
    s->has_specular = false;
    for (const GeomRecord& g : cs.geoms) s->has_specular = s->has_specular || g.bxdf_type == FF_BXDF_MIRROR || g.bxdf_type == FF_BXDF_GLASS;
    s->num_tris = cs.tris.size();
    s->node_capacity = cs.nodes.size();
    // Each mesh's nodes are contiguous with the root first: slot = [root, next mesh's root).
    s->h_geoms = cs.geoms;
    s->slots.assign(cs.geoms.size(), FfState::MeshSlot());
    std::vector<int> roots;
    for (const GeomRecord& g : cs.geoms)
        if (g.type == FF_GEOM_TRIANGLEMESH && g.bvh_root >= 0) roots.push_back(g.bvh_root);
    std::sort(roots.begin(), roots.end());
    for (size_t gi = 0; gi < cs.geoms.size(); ++gi) {
        const GeomRecord& g = cs.geoms[gi];
        if (g.type != FF_GEOM_TRIANGLEMESH || g.bvh_root < 0) continue;
        const auto next = std::upper_bound(roots.begin(), roots.end(), g.bvh_root);
        FfState::MeshSlot& slot = s->slots[gi];
        slot.node_first = g.bvh_root;
        slot.node_count = (next == roots.end() ? (int)cs.nodes.size() : *next) - g.bvh_root;
        slot.node_capacity = slot.node_count;
        slot.depth = cs.max_depth; // per-mesh depths are not kept by the host compiler; the scene maximum is a valid bound
    }
    s->scene_builder = FF_BUILD_HOST_SAH;
    refresh_scene_extent(s);
    s->num_nodes = (int)cs.nodes.size();
    s->max_depth = cs.max_depth;
    s->build_stats.bvh_nodes = s->num_nodes;
    s->build_stats.bvh_max_depth = s->max_depth;
    // the 4-wide trees the kernels traverse, derived on the device from the binary ones just copied
    const auto t_collapse = std::chrono::steady_clock::now();
    for (size_t gi = 0; gi < s->slots.size(); ++gi) {
        st = collapse_slot(s, gi, /*with_info=*/true);
        if (st != FF_OK) return st;
    }
    s->build_stats.build_ms += ms_since(t_collapse);
    st = finalize_layout(s);
    if (st != FF_OK) return st;
    s->has_scene = true;
    return FF_OK;
}

int upload_host_built(FfState* s, const FfGeometry* host_geometries, int n, const BvhBuildParams& bp)
{
    CompiledScene cs;
    const auto t_build = std::chrono::steady_clock::now();
    int st = compile_scene(host_geometries, n, bp, cs);
    if (st != FF_OK) return st;
    s->build_stats.build_ms = ms_since(t_build);
    return upload_compiled(s, cs);
}

} // namespace

namespace ff {

// ff_upload_scene with a scene the caller compiled (ff_multi_upload_scene: one host build for all devices).  build_ms: what the
// compilation took, for the state's FfBuildStats.
int upload_compiled_scene(FfState* s, const CompiledScene& cs, double build_ms)
{
    const auto t_call = std::chrono::steady_clock::now();
    s->primary_valid = s->last_key_valid = false;
    for (ReprojectionHistory& h : s->history) h.invalidate();
    s->nee_valid = false; // (no light table: FF_SHADE_DIFFUSE_PATH_NEE is not offered on a compiled upload)
    tex_drop_bindings(s);
    glossy_drop_bindings(s);
    s->nee_geoms.clear();
    s->nee_tris.clear();
    s->build_stats = FfBuildStats();
    s->build_stats.build_ms = build_ms;
    const int st = upload_compiled(s, cs);
    if (st != FF_OK) free_scene(s);
    s->build_stats.total_ms = ms_since(t_call) + build_ms;
    return st;
}

} // namespace ff

extern "C" {

int ff_set_builder(FfState* s, int builder)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_set_builder: state is null");
    if (builder != FF_BUILD_HOST_SAH && builder != FF_BUILD_GPU_LBVH && builder != FF_BUILD_GPU_PLOC) return fail(FF_ERR_INVALID_ARG, "ff_set_builder: unknown builder %d", builder);
    s->builder = builder;
    return FF_OK;
}

int ff_upload_scene(FfState* s, const FfGeometry* host_geometries, int n)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_upload_scene: state is null");
    s->primary_valid = s->last_key_valid = false; // (the stored primary hits belong to the scene that goes)
    for (ReprojectionHistory& h : s->history) h.invalidate(); // (and so do the temporal denoiser's and the TAA history)
    const auto t_call = std::chrono::steady_clock::now();
    s->build_stats = FfBuildStats();
    const BvhBuildParams bp = default_bvh_params();
    s->nee_valid = false; // (the light table belongs to the scene that goes)
    tex_drop_bindings(s); // (and so do the albedo-texture bindings; the textures stay)
    glossy_drop_bindings(s); // (and the roughness bindings)
    if (s->builder != FF_BUILD_HOST_SAH) {
        int st = upload_with_device_builder(s, host_geometries, n, bp);
        if (st == FF_OK) {
            nee_capture(s, host_geometries, n, /*upload=*/true);
            st = nee_rebuild(s);
        }
        s->build_stats.total_ms = ms_since(t_call);
        if (st != FF_OK) free_scene(s);
        return st;
    }
    int st = upload_host_built(s, host_geometries, n, bp);
    if (st == FF_OK) {
        nee_capture(s, host_geometries, n, /*upload=*/true);
        st = nee_rebuild(s);
    }
    if (st != FF_OK) free_scene(s); // never leave a half-allocated scene behind (has_scene is false again)
    s->build_stats.total_ms = ms_since(t_call);
    return st;
}

int ff_update_transforms(FfState* s, const FfGeometry* host_geometries, int n)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_update_transforms: state is null");
    if (!s->has_scene) return fail(FF_ERR_NO_SCENE, "ff_update_transforms: no scene uploaded");
    s->primary_valid = s->last_key_valid = false;
    const auto t_call = std::chrono::steady_clock::now();
    CompiledScene cs;
    int st = compile_scene(host_geometries, n, default_bvh_params(), cs, /*build_bvh=*/false);
    if (st != FF_OK) return st;
    if (cs.geoms.size() != s->h_geoms.size()) return fail(FF_ERR_INVALID_ARG, "ff_update_transforms: %d geometries, the uploaded scene has %zu", n, s->h_geoms.size());
    // The compiler orders the planes by the size of their world boxes, which a transform changes: match the new records to the
    // uploaded ones by the caller's index and keep the UPLOADED order (the mesh slots are parallel to it).  That the leading
    // planes are the largest is only an optimisation (count_scan_planes); a stale order stays correct.
    {
        std::vector<int> where(cs.geoms.size(), -1);
        for (size_t i = 0; i < cs.geoms.size(); ++i) {
            const int o = cs.geoms[i].orig_index;
            if (o >= 0 && (size_t)o < where.size()) where[o] = (int)i;
        }
        std::vector<GeomRecord> ordered(cs.geoms.size());
        for (size_t i = 0; i < s->h_geoms.size(); ++i) {
            const GeomRecord& b = s->h_geoms[i];
            const int j = b.orig_index >= 0 && (size_t)b.orig_index < where.size() ? where[b.orig_index] : -1;
            if (j < 0) return fail(FF_ERR_INVALID_ARG, "ff_update_transforms: geometry %d of the uploaded scene is missing", b.orig_index);
            GeomRecord a = cs.geoms[j];
            if (a.type != b.type || a.tri_count != b.tri_count || a.tri_first != b.tri_first)
                return fail(FF_ERR_INVALID_ARG, "ff_update_transforms: geometry %d differs in kind or triangle count from the uploaded one", a.orig_index);
            a.bvh_root = b.bvh_root;
            ordered[i] = a;
        }
        cs.geoms.swap(ordered);
    }
    FF_HIP(hipSetDevice(s->device));
    s->h_geoms = cs.geoms;
    st = finalize_layout(s); // (fills the records' tree fields again and copies them to the device)
    if (st != FF_OK) return st;
    s->has_specular = false; // materials may have changed
    for (const GeomRecord& g : cs.geoms) s->has_specular = s->has_specular || g.bxdf_type == FF_BXDF_MIRROR || g.bxdf_type == FF_BXDF_GLASS;
    st = glossy_sync_table(s); // (a roughness binding is applied while its geometry is a mirror)
    if (st != FF_OK) return st;
    if (!s->nee_geoms.empty() || s->nee_valid) { // (the light table follows the emitters' new transforms and materials)
        nee_capture(s, host_geometries, n, /*upload=*/false);
        st = nee_rebuild(s);
        if (st != FF_OK) return st;
    }
    s->build_stats.last_operation = 3;
    s->build_stats.total_ms = ms_since(t_call);
    s->build_stats.copy_ms = s->build_stats.total_ms;
    s->build_stats.build_ms = 0.0;
    return FF_OK;
}

int ff_update_mesh(FfState* s, int geometry_index, const FfTriangle* triangles, int count, int mode)
{
    clear_error();
    if (!s || !triangles) return fail(FF_ERR_INVALID_ARG, "ff_update_mesh: null argument");
    if (!s->has_scene) return fail(FF_ERR_NO_SCENE, "ff_update_mesh: no scene uploaded");
    s->primary_valid = s->last_key_valid = false;
    if (mode != FF_UPDATE_REFIT && mode != FF_UPDATE_REBUILD) return fail(FF_ERR_INVALID_ARG, "ff_update_mesh: unknown mode %d", mode);
    int gi = -1;
    for (size_t i = 0; i < s->h_geoms.size(); ++i)
        if (s->h_geoms[i].orig_index == geometry_index) gi = (int)i;
    if (gi < 0 || s->h_geoms[gi].type != FF_GEOM_TRIANGLEMESH) return fail(FF_ERR_INVALID_ARG, "ff_update_mesh: geometry %d is not an uploaded mesh", geometry_index);
    GeomRecord& rec = s->h_geoms[gi];
    if (count != rec.tri_count || count <= 0) return fail(FF_ERR_INVALID_ARG, "ff_update_mesh: %d triangles, the uploaded mesh has %d", count, rec.tri_count);
    if (mode == FF_UPDATE_REBUILD && s->scene_builder == FF_BUILD_HOST_SAH)
        return fail(FF_ERR_UNSUPPORTED, "ff_update_mesh: rebuilding in place needs a scene uploaded with a device builder (host-built trees are packed)");
    for (ReprojectionHistory& h : s->history) h.mark_replaced(geometry_index); // (the mesh's temporal and TAA histories restart)
    const auto t_call = std::chrono::steady_clock::now();
    FfBuildStats& bs = s->build_stats;
    bs.copy_ms = bs.build_ms = 0.0;
    FF_HIP(hipSetDevice(s->device));
    FfState::MeshSlot& slot = s->slots[gi];
    const BvhBuildParams bp = default_bvh_params();
    int st = stage_triangles(s, triangles, count, &bs.copy_ms);
    if (st != FF_OK) return st;
    const auto t_build = std::chrono::steady_clock::now();
    if (mode == FF_UPDATE_REBUILD) {
        if (count <= device_leaf_tris(bp)) {
            st = place_single_leaf_mesh(s, triangles, count, bp, rec.tri_first, slot.node_first, &slot.node_count, &slot.depth);
        } else {
            MeshBuildInfo info = MeshBuildInfo();
            st = gpu_build_mesh(s->stream, s->scratch, s->d_stage, count, rec.tri_first, slot.node_first, device_leaf_tris(bp), s->d_tris, s->d_normals, s->d_uvs, s->d_nodes, &info,
                                s->scene_builder == FF_BUILD_GPU_PLOC);
            if (st == FF_OK) {
                slot.node_count = info.node_count;
                slot.depth = info.depth;
            }
        }
        if (st != FF_OK) {
            // the mesh's records and nodes may be half rewritten: nothing may render from them
            s->has_scene = false;
            return st;
        }
        slot.parents_linked = false;
        st = collapse_slot(s, (size_t)gi, /*with_info=*/true);
        if (st != FF_OK) {
            s->has_scene = false;
            return st;
        }
        bs.last_operation = 2;
    } else {
        if (!slot.parents_linked) {
            st = gpu_link_parents(s->stream, s->d_nodes, slot.node_first, slot.node_count, s->d_parent + slot.node_first);
            if (st != FF_OK) return st;
            slot.parents_linked = true;
        }
        st = gpu_refit_mesh(s->stream, s->scratch, s->d_stage, count, rec.tri_first, slot.node_first, slot.node_count, s->d_parent + slot.node_first, s->d_tris,
                            s->d_normals, s->d_uvs, s->d_nodes);
        if (st != FF_OK) return st;
        st = collapse_slot(s, (size_t)gi, /*with_info=*/false); // same topology: the boxes of the 4-wide nodes follow
        if (st != FF_OK) return st;
        bs.last_operation = 1;
    }
    // the geometry's world box follows the new vertices
    float omn[3] = { 3.0e38f, 3.0e38f, 3.0e38f }, omx[3] = { -3.0e38f, -3.0e38f, -3.0e38f };
    for (int t = 0; t < count; ++t) {
        const FfVec3* v[3] = { &triangles[t].m_v0, &triangles[t].m_v1, &triangles[t].m_v2 };
        for (const FfVec3* p : v) {
            omn[0] = std::min(omn[0], p->x); omn[1] = std::min(omn[1], p->y); omn[2] = std::min(omn[2], p->z);
            omx[0] = std::max(omx[0], p->x); omx[1] = std::max(omx[1], p->y); omx[2] = std::max(omx[2], p->z);
        }
    }
    set_world_box(rec, omn, omx);
    refresh_scene_extent(s);
    if (s->nee_valid && (size_t)geometry_index < s->nee_geoms.size()) {
        const FfBXDF* m = s->nee_geoms[(size_t)geometry_index].m_bxdf;
        nee_replace_mesh(s, geometry_index, triangles, count);
        if (m && m->m_type == FF_BXDF_EMITTER) {
            st = nee_rebuild(s);
            if (st != FF_OK) return st;
        }
    }
    if (s->scene_builder == FF_BUILD_HOST_SAH) s->num_nodes = (int)s->node_capacity;
    st = finalize_layout(s); // (a rebuilt tree may differ in size and depth: LDS shares and workgroup size follow; copies the records)
    if (st != FF_OK) return st;
    bs.build_ms = ms_since(t_build);
    bs.total_ms = ms_since(t_call);
    return FF_OK;
}

int ff_build_stats(FfState* s, FfBuildStats* out)
{
    clear_error();
    if (!s || !out) return fail(FF_ERR_INVALID_ARG, "ff_build_stats: null argument");
    *out = s->build_stats;
    return FF_OK;
}

int ff_debug_download_bvh(FfState* s, void* nodes, int max_nodes, int* out_nodes, void* tris, int max_tris, int* out_tris, int* mesh_table,
                          int max_geometries)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_debug_download_bvh: state is null");
    if (!s->has_scene) return fail(FF_ERR_NO_SCENE, "ff_debug_download_bvh: no scene uploaded");
    if (out_nodes) *out_nodes = s->num_nodes;
    if (out_tris) *out_tris = (int)s->num_tris;
    FF_HIP(hipSetDevice(s->device));
    if (nodes && max_nodes > 0) FF_HIP(hipMemcpy(nodes, s->d_nodes, (size_t)std::min(max_nodes, s->num_nodes) * sizeof(BvhNode), hipMemcpyDeviceToHost));
    if (tris && max_tris > 0) FF_HIP(hipMemcpy(tris, s->d_tris, (size_t)std::min<uint64_t>((uint64_t)max_tris, s->num_tris) * sizeof(TriRecord), hipMemcpyDeviceToHost));
    if (mesh_table) {
        for (size_t i = 0; i < s->h_geoms.size(); ++i) {
            const GeomRecord& g = s->h_geoms[i];
            if (g.orig_index < 0 || g.orig_index >= max_geometries) continue;
            int* row = mesh_table + 5 * g.orig_index;
            const bool mesh = g.type == FF_GEOM_TRIANGLEMESH && g.bvh_root >= 0;
            row[0] = mesh ? g.bvh_root : -1;
            row[1] = mesh ? s->slots[i].node_count : 0;
            row[2] = g.tri_first;
            row[3] = g.tri_count;
            row[4] = mesh ? s->slots[i].depth : 0;
        }
    }
    return FF_OK;
}

int ff_debug_download_bvh4(FfState* s, void* nodes4, int max_nodes, int* out_capacity, int* mesh_table, int max_geometries)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_debug_download_bvh4: state is null");
    if (!s->has_scene) return fail(FF_ERR_NO_SCENE, "ff_debug_download_bvh4: no scene uploaded");
    if (out_capacity) *out_capacity = (int)s->node_capacity;
    FF_HIP(hipSetDevice(s->device));
    if (nodes4 && max_nodes > 0)
        FF_HIP(hipMemcpy(nodes4, s->d_nodes4, (size_t)std::min<size_t>((size_t)max_nodes, s->node_capacity) * sizeof(Bvh4Node), hipMemcpyDeviceToHost));
    if (mesh_table) {
        for (size_t i = 0; i < s->h_geoms.size(); ++i) {
            const GeomRecord& g = s->h_geoms[i];
            if (g.orig_index < 0 || g.orig_index >= max_geometries) continue;
            int* row = mesh_table + 6 * g.orig_index;
            const bool mesh = g.type == FF_GEOM_TRIANGLEMESH && g.bvh_root >= 0;
            int lds_first = 0;
            std::memcpy(&lds_first, &g.wmin[3], sizeof(int));
            row[0] = mesh ? g.node4_first : -1;
            row[1] = mesh ? s->slots[i].node4_count : 0;
            row[2] = mesh ? s->slots[i].depth4 : 0;
            row[3] = mesh ? lds_first : 0;
            row[4] = mesh ? g.lds_nodes : 0;
            row[5] = s->lds_cap;
        }
    }
    return FF_OK;
}

} // extern "C"
