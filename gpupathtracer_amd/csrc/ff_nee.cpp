// ff_nee.cpp — next-event estimation (FF_SHADE_DIFFUSE_PATH_NEE): the light table on the host and the frames of the mode.
//
// The table holds one entry per emitting plane (the world image of its unit quad) and per triangle of an emitting mesh.  Spheres
// (an ellipsoid under a general model matrix has no closed-form area sampling) and emitters of zero luminance are left out; BSDF
// sampling still finds them, with MIS weight 1.  Entries are chosen with probability area x luminance / sum (a Vose alias table),
// so the pdf of a light sample per unit area is luminance / sum on every entry of a geometry: one number per geometry.
// The estimator itself is in ff_api.h; the kernel is nee_path_kernel (ff_k_nee.h).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ff_state.h"

using namespace ff;

namespace {

struct LightEntryD {
    int geom, prim;
    double v0[3], e1[3], e2[3], n[3];
    double area, lum, prob, alias_prob;
    int alias;
};

struct LightTableD {
    std::vector<LightEntryD> entries;
    std::vector<double> pdf_area; // per caller geometry: luminance / sum, 0 outside the table
    double sum = 0.0;
};

void mat_point(const FfMat4& m, const double p[3], double out[3])
{
    for (int r = 0; r < 3; ++r) out[r] = (double)m.m[r] * p[0] + (double)m.m[4 + r] * p[1] + (double)m.m[8 + r] * p[2] + (double)m.m[12 + r];
}

void mat_vector(const FfMat4& m, const double v[3], double out[3])
{
    for (int r = 0; r < 3; ++r) out[r] = (double)m.m[r] * v[0] + (double)m.m[4 + r] * v[1] + (double)m.m[8 + r] * v[2];
}

void cross(const double a[3], const double b[3], double out[3])
{
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}

// Appends the entry if its area is positive; the area is |e1 x e2| (parallelogram) or half of it (triangle).
void add_entry(LightTableD& t, int geom, int prim, double lum, const double v0[3], const double e1[3], const double e2[3])
{
    double c[3];
    cross(e1, e2, c);
    const double len = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    const double area = prim < 0 ? len : 0.5 * len;
    if (!(area > 0.0) || !std::isfinite(area)) return;
    LightEntryD e = {};
    e.geom = geom;
    e.prim = prim;
    for (int k = 0; k < 3; ++k) {
        e.v0[k] = v0[k];
        e.e1[k] = e1[k];
        e.e2[k] = e2[k];
        e.n[k] = c[k] / len;
    }
    e.area = area;
    e.lum = lum;
    t.entries.push_back(e);
}

// The table of a host scene (caller order), in double.
int compute_light_table(const FfGeometry* g, int n, LightTableD& t)
{
    t = LightTableD();
    t.pdf_area.assign((size_t)std::max(n, 0), 0.0);
    for (int i = 0; i < n; ++i) {
        const FfGeometry& G = g[i];
        if (!G.m_bxdf || G.m_bxdf->m_type != FF_BXDF_EMITTER) continue;
        // (the record's emission: m_emissiveColor * m_intensity in float, as the kernels read it)
        const float er = G.m_bxdf->m_emissiveColor.x * G.m_bxdf->m_intensity, eg = G.m_bxdf->m_emissiveColor.y * G.m_bxdf->m_intensity,
                    eb = G.m_bxdf->m_emissiveColor.z * G.m_bxdf->m_intensity;
        const double lum = 0.2126 * (double)er + 0.7152 * (double)eg + 0.0722 * (double)eb;
        if (!(lum > 0.0)) continue;
        if (G.m_geometryType == FF_GEOM_PLANE) {
            // object space: {P : m_normal . P = 0, |P.x| <= 0.5, |P.y| <= 0.5} (kernel.cu:11-18), i.e. P(u, v) = (u, v, -(nx u + ny v) / nz)
            const double nx = G.m_normal.x, ny = G.m_normal.y, nz = G.m_normal.z;
            if (nz == 0.0) continue;
            const double c0[3] = { -0.5, -0.5, (0.5 * nx + 0.5 * ny) / nz }, a[3] = { 1.0, 0.0, -nx / nz }, b[3] = { 0.0, 1.0, -ny / nz };
            double v0[3], e1[3], e2[3];
            mat_point(G.m_modelMatrix, c0, v0);
            mat_vector(G.m_modelMatrix, a, e1);
            mat_vector(G.m_modelMatrix, b, e2);
            add_entry(t, i, -1, lum, v0, e1, e2);
        } else if (G.m_geometryType == FF_GEOM_TRIANGLEMESH) {
            if (!G.m_triangles) continue;
            for (int k = 0; k < G.m_numberOfTriangles; ++k) {
                const FfTriangle& T = G.m_triangles[k];
                const double a[3] = { T.m_v0.x, T.m_v0.y, T.m_v0.z }, b[3] = { T.m_v1.x, T.m_v1.y, T.m_v1.z }, c[3] = { T.m_v2.x, T.m_v2.y, T.m_v2.z };
                double wa[3], wb[3], wc[3];
                mat_point(G.m_modelMatrix, a, wa);
                mat_point(G.m_modelMatrix, b, wb);
                mat_point(G.m_modelMatrix, c, wc);
                const double e1[3] = { wb[0] - wa[0], wb[1] - wa[1], wb[2] - wa[2] }, e2[3] = { wc[0] - wa[0], wc[1] - wa[1], wc[2] - wa[2] };
                add_entry(t, i, k, lum, wa, e1, e2);
            }
        }
        // (spheres: left out, see the file comment)
    }
    for (const LightEntryD& e : t.entries) t.sum += e.area * e.lum;
    if (t.entries.empty() || !(t.sum > 0.0) || !std::isfinite(t.sum)) {
        t.entries.clear();
        t.sum = 0.0;
        return FF_OK;
    }
    for (LightEntryD& e : t.entries) {
        e.prob = e.area * e.lum / t.sum;
        t.pdf_area[(size_t)e.geom] = e.lum / t.sum;
    }
    // Vose's alias method: scaled probabilities n q_k split into "small" (< 1) and "large"; each small entry is topped up by a large one
    const size_t m = t.entries.size();
    std::vector<double> q(m);
    std::vector<size_t> small, large;
    for (size_t k = 0; k < m; ++k) {
        q[k] = t.entries[k].prob * (double)m;
        t.entries[k].alias = (int)k;
        (q[k] < 1.0 ? small : large).push_back(k);
    }
    while (!small.empty() && !large.empty()) {
        const size_t s = small.back(), l = large.back();
        small.pop_back();
        large.pop_back();
        t.entries[s].alias_prob = q[s];
        t.entries[s].alias = (int)l;
        q[l] = (q[l] + q[s]) - 1.0;
        (q[l] < 1.0 ? small : large).push_back(l);
    }
    for (size_t k : large) t.entries[k].alias_prob = 1.0;
    for (size_t k : small) t.entries[k].alias_prob = 1.0; // (rounding leftovers)
    return FF_OK;
}

int check_geometries(const FfGeometry* g, int n, const char* who)
{
    if (n < 0 || (n > 0 && !g)) return fail(FF_ERR_INVALID_ARG, "%s: invalid geometry array", who);
    return FF_OK;
}

} // namespace

namespace ff {

// Keeps what the light table is built from (ff_upload_scene, ff_update_transforms).  Triangles of meshes are copied when the state
// holds none for that geometry yet (an upload drops them all first), so that ff_update_mesh's replacements stay.
void nee_capture(FfState* s, const FfGeometry* g, int n, bool upload)
{
    if (upload) {
        s->nee_tris.clear();
        s->nee_valid = false;
    }
    s->nee_geoms.assign(g, g + n);
    s->nee_bxdfs.resize((size_t)n);
    s->nee_tris.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        FfGeometry& G = s->nee_geoms[(size_t)i];
        if (g[i].m_bxdf) s->nee_bxdfs[(size_t)i] = *g[i].m_bxdf;
        else std::memset(&s->nee_bxdfs[(size_t)i], 0, sizeof(FfBXDF));
        G.m_bxdf = g[i].m_bxdf ? &s->nee_bxdfs[(size_t)i] : nullptr;
        std::vector<FfTriangle>& tv = s->nee_tris[(size_t)i];
        // (only emitters' triangles are kept: the table reads nothing else, and a big scene's meshes are big)
        const bool emitter = G.m_bxdf && G.m_bxdf->m_type == FF_BXDF_EMITTER;
        if (!emitter) tv.clear();
        else if (G.m_geometryType == FF_GEOM_TRIANGLEMESH && tv.empty() && g[i].m_triangles && g[i].m_numberOfTriangles > 0)
            tv.assign(g[i].m_triangles, g[i].m_triangles + g[i].m_numberOfTriangles);
        G.m_triangles = tv.empty() ? nullptr : tv.data();
    }
}

// ff_update_mesh: the mesh's new object-space triangles.
void nee_replace_mesh(FfState* s, int geometry_index, const FfTriangle* tris, int count)
{
    if (geometry_index < 0 || (size_t)geometry_index >= s->nee_geoms.size()) return;
    std::vector<FfTriangle>& tv = s->nee_tris[(size_t)geometry_index];
    FfGeometry& G = s->nee_geoms[(size_t)geometry_index];
    if (G.m_bxdf && G.m_bxdf->m_type == FF_BXDF_EMITTER) tv.assign(tris, tris + count);
    else tv.clear();
    G.m_triangles = tv.empty() ? nullptr : tv.data();
}

// Builds the table from the captured geometries and copies it to the device (records in processing order: s->h_geoms).
int nee_rebuild(FfState* s)
{
    s->nee_valid = false;
    LightTableD t;
    int st = compute_light_table(s->nee_geoms.data(), (int)s->nee_geoms.size(), t);
    if (st != FF_OK) return st;
    std::vector<int> record_of(s->nee_geoms.size(), -1);
    for (size_t r = 0; r < s->h_geoms.size(); ++r) {
        const int o = s->h_geoms[r].orig_index;
        if (o >= 0 && (size_t)o < record_of.size()) record_of[(size_t)o] = (int)r;
    }
    std::vector<float> pdf(std::max<size_t>(s->h_geoms.size(), 1), 0.f);
    for (size_t i = 0; i < t.pdf_area.size(); ++i)
        if (record_of[i] >= 0) pdf[(size_t)record_of[i]] = (float)t.pdf_area[i];
    std::vector<float> lights(std::max<size_t>(t.entries.size(), 1) * 20, 0.f);
    for (size_t k = 0; k < t.entries.size(); ++k) {
        const LightEntryD& e = t.entries[k];
        float* q = &lights[20 * k];
        const int rec = record_of[(size_t)e.geom];
        if (rec < 0) return fail(FF_ERR_INVALID_ARG, "light table: geometry %d has no uploaded record", e.geom);
        for (int a = 0; a < 3; ++a) {
            q[a] = (float)e.v0[a];
            q[4 + a] = (float)e.e1[a];
            q[8 + a] = (float)e.e2[a];
            q[12 + a] = (float)e.n[a];
        }
        std::memcpy(&q[3], &rec, 4);
        std::memcpy(&q[7], &e.prim, 4);
        std::memcpy(&q[11], &e.alias, 4);
        q[15] = (float)e.alias_prob;
        q[16] = (float)t.pdf_area[(size_t)e.geom];
    }
    st = ensure_bytes((void**)&s->d_nee_lights, &s->nee_lights_bytes, lights.size() * sizeof(float));
    if (st != FF_OK) return st;
    st = ensure_bytes((void**)&s->d_nee_pdf, &s->nee_pdf_bytes, pdf.size() * sizeof(float));
    if (st != FF_OK) return st;
    FF_HIP(hipMemcpy(s->d_nee_lights, lights.data(), lights.size() * sizeof(float), hipMemcpyHostToDevice));
    FF_HIP(hipMemcpy(s->d_nee_pdf, pdf.data(), pdf.size() * sizeof(float), hipMemcpyHostToDevice));
    s->nee_num_lights = (int)t.entries.size();
    s->nee_valid = true;
    return FF_OK;
}

// The frame of FF_SHADE_DIFFUSE_PATH_NEE (render_enqueue has filled k's camera, image, block and scene fields).  The mega-kernels'
// stored primary hits, keys and cull mask are neither used nor touched: the next FF_SHADE_DIFFUSE_PATH frame finds them as they were.
int enqueue_nee(FfState* s, KParams& k, const FfCamera* camera, const FfRenderParams* prm, int launches, int blocks_per_launch, size_t local_pixels)
{
    if (!s->nee_valid) {
        if (s->tex_bound > 0 && prm->shade_mode != FF_SHADE_DIFFUSE_PATH_NEE && !s->env_set)
            return fail(FF_ERR_UNSUPPORTED, "albedo textures need a scene uploaded with ff_upload_scene (this one has no light table)");
        if (s->glossy_applied > 0 && prm->shade_mode != FF_SHADE_DIFFUSE_PATH_NEE && !s->env_set)
            return fail(FF_ERR_UNSUPPORTED, "rough-specular mirrors need a scene uploaded with ff_upload_scene (this one has no light table)");
        if (s->env_set)
            return fail(FF_ERR_UNSUPPORTED, "an environment light needs a scene uploaded with ff_upload_scene (this one has no light table)");
        if (s->cam_active())
            return fail(FF_ERR_UNSUPPORTED, "per-sample camera rays (ff_set_camera_sampling) need a scene uploaded with ff_upload_scene (this one has no light table)");
        return fail(FF_ERR_UNSUPPORTED, "FF_SHADE_DIFFUSE_PATH_NEE needs a scene uploaded with ff_upload_scene (this one has no light table)");
    }
    hipStream_t st = s->stream;
    k.tail_block = -1;
    k.cull_mask = nullptr;
    k.cull_mask_out = nullptr;
    k.primary_hits = nullptr;
    k.trinormals = nullptr;
    k.emitter_mask = 0u;
    k.cut_last = 0;
    k.timeline = nullptr;
    k.counters = s->d_counters;
    k.queue = s->d_queue;
    k.queue_counters = 1;
    k.lds_nodes = s->lds_cap; // (laid out for the trace kernel's workgroup; 512 threads leave more room, never less)
    // persistent workgroups: enough to fill the device a few times over, never more than the items need
    const uint64_t most_items = (uint64_t)k.pix_items * (uint64_t)std::min(blocks_per_launch, k.num_blocks);
    int grid = (int)std::min<uint64_t>((most_items + kBlockThreads - 1) / kBlockThreads, (uint64_t)s->num_cus * 8);
    if (grid < 1) grid = 1;
    k.stack_spill = nullptr;
    int sst = prm->trace_mode == FF_TRACE_BVH ? attach_stack_spill(s, k, grid, kBlockThreads) : FF_OK;
    if (sst == FF_OK) sst = clear_floor_grid(prm->grid_mode, k.rgb8, k.radiance, local_pixels, st);
    if (sst != FF_OK) return sst;
    NeeParams np;
    std::memset(&np, 0, sizeof np);
    np.lights = s->d_nee_lights;
    np.num_lights = s->nee_num_lights;
    np.light_pdf = s->d_nee_pdf;
    const bool env = s->env_set; // (render_enqueue sends FF_SHADE_NORMAL_DEBUG elsewhere)
    const bool tex = s->tex_bound > 0;
    const bool glossy = s->glossy_applied > 0;
    // FF_SHADE_DIFFUSE_PATH comes here under an environment or with albedo textures or rough-specular mirrors bound: it samples no
    // light at all
    if (prm->shade_mode != FF_SHADE_DIFFUSE_PATH_NEE) np.num_lights = 0;
    if (tex) {
        np.tex_bind = s->d_tex_bind;
        np.tex_desc = s->d_tex_desc;
        np.uvs = s->d_uvs;
    }
    if (glossy) np.glossy_alpha = s->d_glossy_alpha;
    if (s->cam_active()) {
        // (render_enqueue has put the unjittered matrix into k for a box frame)
        np.cam_active = 1;
        np.cam_box = s->cam_sampling.pixel_filter == FF_PIXEL_BOX ? 1 : 0;
        np.cam_lens_radius = s->cam_sampling.lens_radius;
        np.cam_focus = s->cam_sampling.focus_distance;
        const FfVec3 f = camera->m_forward, r = camera->m_right, u = camera->m_up;
        np.cam_fwd[0] = f.x; np.cam_fwd[1] = f.y; np.cam_fwd[2] = f.z;
        np.cam_right[0] = r.x; np.cam_right[1] = r.y; np.cam_right[2] = r.z;
        np.cam_up[0] = u.x; np.cam_up[1] = u.y; np.cam_up[2] = u.z;
    }
    if (env) {
        // the environment as one more light (ff_api.h); without light samples p_env = 0
        np.env_texels = s->d_env_texels;
        np.env_alias = s->d_env_alias;
        np.env_z = s->d_env_z;
        np.env_w = s->env_w;
        np.env_h = s->env_h;
        np.env_rotation = s->env_rotation;
        np.p_env = (prm->shade_mode != FF_SHADE_DIFFUSE_PATH_NEE || !s->env_sampled) ? 0.f : (np.num_lights > 0 ? 0.5f : 1.f);
        np.p_area = 1.f - np.p_env;
    }
    FF_HIP(hipMemsetAsync(s->d_counters, 0, (size_t)kCounterWords * sizeof(unsigned long long), st));
    FF_HIP(hipEventRecord(s->ev_begin, st));
    for (int l = 0; l < launches; ++l) {
        set_launch_blocks(k, l, blocks_per_launch);
        np.k = k;
        np.items = k.total_items;
        FF_HIP(launch_nee(np, prm->trace_mode, env, tex, glossy, grid, st, &s->last_kernel_name));
    }
    FF_HIP(launch_combine(k, st));
    FF_HIP(hipEventRecord(s->ev_end, st));
    FF_HIP(hipMemcpyAsync(s->h_counters, s->d_counters, kCounterWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    commit_pending(s, launches, 0u, 0u, false, false);
    return FF_OK;
}

} // namespace ff

extern "C" {

int ff_light_table(const FfGeometry* host_geometries, int n, FfLightEntry* out_entries, int max_entries, float* out_pdf_area)
{
    clear_error();
    int st = check_geometries(host_geometries, n, "ff_light_table");
    if (st != FF_OK) return -st;
    if (max_entries < 0 || (max_entries > 0 && !out_entries)) return -fail(FF_ERR_INVALID_ARG, "ff_light_table: invalid output array");
    LightTableD t;
    st = compute_light_table(host_geometries, n, t);
    if (st != FF_OK) return -st;
    const int count = (int)t.entries.size();
    for (int k = 0; k < std::min(count, max_entries); ++k) {
        const LightEntryD& e = t.entries[(size_t)k];
        FfLightEntry& o = out_entries[k];
        o.geometry = e.geom;
        o.primitive = e.prim;
        o.area = (float)e.area;
        o.probability = (float)e.prob;
        o.v0 = FfVec3{ (float)e.v0[0], (float)e.v0[1], (float)e.v0[2] };
        o.e1 = FfVec3{ (float)e.e1[0], (float)e.e1[1], (float)e.e1[2] };
        o.e2 = FfVec3{ (float)e.e2[0], (float)e.e2[1], (float)e.e2[2] };
        o.normal = FfVec3{ (float)e.n[0], (float)e.n[1], (float)e.n[2] };
        o.alias_probability = (float)e.alias_prob;
        o.alias = e.alias;
    }
    if (out_pdf_area)
        for (int i = 0; i < n; ++i) out_pdf_area[i] = (float)t.pdf_area[(size_t)i];
    return count;
}

} // extern "C"
