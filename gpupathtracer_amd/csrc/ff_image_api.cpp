// ff_image_api.cpp — host side of the image-space entry points of the C ABI (include/firefly/ff_api.h): ff_gbuffer's resolve,
// ff_denoise, ff_denoise_temporal, ff_taa and ff_taa_upscale with their histories (kernels in ff_denoise.hip, ff_temporal.hip,
// ff_taa.hip, ff_taa_upscale.hip), and
// what they share with ff_display_api.cpp (ff_image.h).  No trace kernel is launched from here: ff_gbuffer's primary hits come
// from frame_primary_hits (ff_frame.cpp).
#include <algorithm>
#include <cmath>
#include <cstring>

#include <hip/hip_runtime.h>

#include "ff_denoise.h"
#include "ff_state.h"
#include "ff_taa.h"
#include "ff_taa_upscale.h"
#include "ff_temporal.h"

using namespace ff;

namespace ff {

int Staging::commit(hipStream_t stream, const char* copy_failed)
{
    if (used == 0) return FF_OK;
    const int st = ensure_bytes(buf, cap, used);
    if (st != FF_OK) return st;
    for (const Piece& p : pieces) {
        *p.dev = (char*)*buf + p.offset;
        if (!p.src) continue;
        if (!copy_failed) FF_HIP(hipMemcpyAsync(*p.dev, p.src, p.bytes, p.kind, stream));
        else if (hipMemcpyAsync(*p.dev, p.src, p.bytes, p.kind, stream) != hipSuccess) return fail(FF_ERR_HIP, "%s", copy_failed);
    }
    return FF_OK;
}

int Staging::finish()
{
    for (const Piece& p : pieces)
        if (p.host) FF_HIP(hipMemcpy(p.host, *p.dev, p.bytes, hipMemcpyDeviceToHost));
    return FF_OK;
}

} // namespace ff

namespace ff {

// inverse of a 4x4 matrix in double (Gauss-Jordan with partial pivoting); column-major in and out.  False if singular.
bool invert4(const double* m, double* out)
{
    double a[4][8];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            a[r][c] = m[c * 4 + r];
            a[r][4 + c] = r == c ? 1.0 : 0.0;
        }
    for (int c = 0; c < 4; ++c) {
        int piv = c;
        for (int r = c + 1; r < 4; ++r)
            if (std::fabs(a[r][c]) > std::fabs(a[piv][c])) piv = r;
        if (a[piv][c] == 0.0) return false;
        if (piv != c)
            for (int k = 0; k < 8; ++k) std::swap(a[c][k], a[piv][k]);
        const double d = a[c][c];
        for (int k = 0; k < 8; ++k) a[c][k] /= d;
        for (int r = 0; r < 4; ++r) {
            if (r == c || a[r][c] == 0.0) continue;
            const double f = a[r][c];
            for (int k = 0; k < 8; ++k) a[r][k] -= f * a[c][k];
        }
    }
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) out[c * 4 + r] = a[r][4 + c];
    return true;
}

} // namespace ff

namespace {

// the model matrix of a record as 12 floats (columns, xyz)
void record_model(const GeomRecord& g, float* out12)
{
    const float* cols[4] = { g.mod_c0, g.mod_c1, g.mod_c2, g.mod_c3 };
    for (int c = 0; c < 4; ++c)
        for (int r = 0; r < 3; ++r) out12[c * 3 + r] = cols[c][r];
}

// The table row of one geometry: A = M_prev * inverse(M_cur) from the previous call's model matrix and this record's inverse model
// matrix, composed in double; N = inverse(A)^T (3x3: the cofactors over the determinant).
TemporalGeom temporal_row(const float* prev12, const GeomRecord& g, int flags)
{
    TemporalGeom row;
    double A[3][4] = { { 1, 0, 0, 0 }, { 0, 1, 0, 0 }, { 0, 0, 1, 0 } };
    if (flags & kTpMoved) {
        const float* inv[4] = { g.inv_c0, g.inv_c1, g.inv_c2, g.inv_c3 };
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) {
                double v = c == 3 ? (double)prev12[9 + r] : 0.0;
                for (int k = 0; k < 3; ++k) v += (double)prev12[k * 3 + r] * (double)inv[c][k];
                A[r][c] = v;
            }
    }
    double cof[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const int r1 = (r + 1) % 3, r2 = (r + 2) % 3, c1 = (c + 1) % 3, c2 = (c + 2) % 3;
            cof[r][c] = A[r1][c1] * A[r2][c2] - A[r1][c2] * A[r2][c1];
        }
    const double det = A[0][0] * cof[0][0] + A[0][1] * cof[0][1] + A[0][2] * cof[0][2];
    const double id = det != 0.0 ? 1.0 / det : 0.0;
    for (int r = 0; r < 3; ++r) {
        row.a[r] = make_float4((float)A[r][0], (float)A[r][1], (float)A[r][2], (float)A[r][3]);
        row.n[r] = make_float4((float)(cof[r][0] * id), (float)(cof[r][1] * id), (float)(cof[r][2] * id), 0.f);
    }
    std::memcpy(&row.n[0].w, &flags, sizeof flags);
    return row;
}

} // namespace

namespace ff {

// inverse(ff_camera_ray_matrix(c)) in double, rounded to float; false if singular
bool inverse_ray_matrix(const FfCamera* c, float* out16, FfMat4* ray)
{
    ff_camera_ray_matrix(c, ray);
    double m[16], inv[16];
    for (int k = 0; k < 16; ++k) m[k] = ray->m[k];
    if (!invert4(m, inv)) return false;
    for (int k = 0; k < 16; ++k) out16[k] = (float)inv[k];
    return true;
}

int ReprojectionHistory::begin(const std::vector<GeomRecord>& records, int w, int h, size_t work_bytes_needed, hipStream_t stream, Frame* out)
{
    const bool has_history = valid && w == width && h == height;
    valid = last = false; // (from here on the history sets are being rewritten)
    int st = ensure_bytes((void**)&d_work, &work_bytes, work_bytes_needed);
    if (st != FF_OK) return st;
    // the per-geometry table, indexed by the caller's geometry index
    int num = 0;
    for (const GeomRecord& g : records) num = std::max(num, g.orig_index + 1);
    h_geoms.assign((size_t)num * sizeof(TemporalGeom), 0);
    TemporalGeom* rows = (TemporalGeom*)h_geoms.data();
    for (const GeomRecord& g : records) {
        const int o = g.orig_index;
        if (o < 0) continue;
        float cur12[12];
        record_model(g, cur12);
        int flags = 0;
        const float* prev12 = cur12;
        if (has_history && (size_t)o < has_model.size() && has_model[o]) {
            prev12 = &model[(size_t)o * 12];
            if (std::memcmp(prev12, cur12, sizeof cur12) != 0) flags |= kTpMoved;
        }
        if ((size_t)o < replaced.size() && replaced[o]) flags |= kTpReplaced;
        rows[o] = temporal_row(prev12, g, flags);
    }
    if (num > 0) {
        st = ensure_bytes(&d_geoms, &geoms_bytes, h_geoms.size());
        if (st != FF_OK) return st;
        FF_HIP(hipMemcpyAsync(d_geoms, h_geoms.data(), h_geoms.size(), hipMemcpyHostToDevice, stream));
    }
    *out = { has_history, has_history ? 1 - cur : 0, num, (const TemporalGeom*)d_geoms };
    return FF_OK;
}

void ReprojectionHistory::commit(const std::vector<GeomRecord>& records, const FfCamera* cam, int w, int h, const Frame& f)
{
    valid = last = true;
    cur = f.cur;
    width = w;
    height = h;
    camera = *cam;
    model.assign((size_t)f.num * 12, 0.f);
    has_model.assign((size_t)f.num, 0);
    for (const GeomRecord& g : records) {
        if (g.orig_index < 0) continue;
        record_model(g, &model[(size_t)g.orig_index * 12]);
        has_model[g.orig_index] = 1;
    }
    replaced.assign((size_t)f.num, 0);
}

void ReprojectionHistory::release()
{
    if (d_work) (void)hipFree(d_work);
    if (d_geoms) (void)hipFree(d_geoms);
    d_work = nullptr;
    d_geoms = nullptr;
    work_bytes = geoms_bytes = 0;
    invalidate();
}

} // namespace ff

namespace {

// What every filter entry point checks first, in this order: the state, the camera (where the call takes one), the parameter
// block, the image size.  The state is not read.
int check_image_call(const FfState* s, bool takes_camera, const FfCamera* camera, const void* params, int width, int height, const char* who)
{
    if (!s) return fail(FF_ERR_INVALID_ARG, "%s: state is null", who);
    if (takes_camera && !camera) return fail(FF_ERR_INVALID_ARG, "%s: camera is null", who);
    if (!params) return fail(FF_ERR_INVALID_ARG, "%s: params are null", who);
    return check_image_size(width, height, who);
}

int check_iterations(int iterations, const char* who)
{
    if (iterations < 0 || iterations > 10) return fail(FF_ERR_INVALID_ARG, "%s: iterations must be in 0..10 (got %d)", who, iterations);
    return FF_OK;
}

int check_sigmas(float a, float b, float c, const char* who)
{
    if (!(a > 0.f && b > 0.f && c > 0.f) || !std::isfinite(a) || !std::isfinite(b) || !std::isfinite(c))
        return fail(FF_ERR_INVALID_ARG, "%s: the sigmas must be positive and finite", who);
    return FF_OK;
}

// The FF_DENOISE_* flags and the guide buffers they ask for; *demod: FF_DENOISE_DEMODULATE_ALBEDO is set.
int check_guides(int flags, const float* radiance, const float* position, const float* normal, const float* albedo, const int32_t* ids, int* demod,
                 const char* who)
{
    if (flags & ~(FF_DENOISE_SAME_GEOMETRY | FF_DENOISE_DEMODULATE_ALBEDO)) return fail(FF_ERR_INVALID_ARG, "%s: unknown flags 0x%x", who, flags);
    *demod = (flags & FF_DENOISE_DEMODULATE_ALBEDO) ? 1 : 0;
    if (!radiance || !position || !normal || !ids || (*demod && !albedo))
        return fail(FF_ERR_INVALID_ARG, "%s: radiance, position, normal and ids are required (and albedo with FF_DENOISE_DEMODULATE_ALBEDO)", who);
    return FF_OK;
}

// ff_denoise_temporal's history and working buffers: 10 float4 and one float2 per pixel (ff_state.h)
TemporalBuffers temporal_buffers(float4* base, int width, int height)
{
    const size_t px = (size_t)width * (size_t)height;
    TemporalBuffers b;
    b.width = width;
    b.height = height;
    for (int k = 0; k < 2; ++k) {
        b.pos[k] = base + (4 * k + 0) * px;
        b.nrm[k] = base + (4 * k + 1) * px;
        b.col[k] = base + (4 * k + 2) * px;
        b.mom[k] = base + (4 * k + 3) * px;
        b.work[k] = base + (8 + k) * px;
    }
    b.motion = (float2*)(base + 10 * px);
    return b;
}

// ff_taa's history and motion: two float4 per pixel {rgb, len} and one float2 (ff_state.h)
TaaArgs taa_buffers(float4* base, int width, int height, int cur)
{
    const size_t px = (size_t)width * (size_t)height;
    TaaArgs a;
    std::memset(&a, 0, sizeof a);
    a.width = width;
    a.height = height;
    a.cur = cur;
    a.hist[0] = base;
    a.hist[1] = base + px;
    a.motion = (float2*)(base + 2 * px);
    return a;
}

int history_reset(FfState* s, int which, const char* who)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "%s: state is null", who);
    s->history[which].invalidate();
    return FF_OK;
}

// ff_temporal_history / ff_taa_history: the last call's motion and lengths, written by `launch` into the caller's device buffers or
// staged for the host's.
template <class Launch>
int history_readback(FfState* s, int which, const char* who, const char* filter, float* motion, float* length, int on_device, Launch launch)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "%s: state is null", who);
    const ReprojectionHistory& h = s->history[which];
    if (!h.last) return fail(FF_ERR_INVALID_ARG, "%s: no %s call since the last reset", who, filter);
    if (!motion && !length) return FF_OK;
    FF_HIP(hipSetDevice(s->device));
    const size_t px = (size_t)h.width * (size_t)h.height;
    float* d_motion = motion;
    float* d_length = length;
    Staging stage(&s->d_img_work, &s->img_work_bytes);
    if (!on_device && motion) stage.out(&d_motion, motion, px * 8);
    if (!on_device && length) stage.out(&d_length, length, px * 4);
    const int st = stage.commit(s->stream, nullptr);
    if (st != FF_OK) return st;
    FF_HIP(launch(h, d_motion, d_length));
    FF_HIP(hipStreamSynchronize(s->stream));
    return stage.finish();
}

} // namespace

extern "C" {

// ---- G-buffer and denoiser (kernels in ff_denoise.hip) ---------------------

int ff_gbuffer(FfState* s, const FfCamera* camera, const FfRenderParams* params, float* depth, float* position, float* normal, float* albedo,
               int32_t* ids, int on_device)
{
    clear_error();
    int st = check_render_call(s, camera, params, "ff_gbuffer");
    if (st != FF_OK) return st;
    if (s->scene_block_threads == 0)
        return fail(FF_ERR_UNSUPPORTED, "ff_gbuffer: 4-wide BVH of depth %d does not fit the LDS traversal stack; upload with FF_BUILD_HOST_SAH", s->max_depth4);
    FF_HIP(hipSetDevice(s->device));
    PrimaryHits ph;
    st = frame_primary_hits(s, camera, params, &ph);
    if (st != FF_OK) return st;
    // outputs: the caller's device buffers, or the staging area and a copy back
    const size_t px = (size_t)params->width * (size_t)params->height;
    GbufferResolveParams r;
    r.hits = ph.hits;
    r.pix_items = ph.pix_items;
    r.tiles_per_row = ph.tiles_per_row;
    r.width = params->width;
    r.height = params->height;
    r.xlim = ph.xlim;
    r.ylim = ph.ylim;
    r.geoms = s->d_geoms;
    r.tris = s->d_tris;
    r.num_geoms = s->num_geoms;
    r.num_tris = (long long)s->num_tris;
    r.tex_bind = s->tex_bound > 0 ? s->d_tex_bind : nullptr;
    r.tex_desc = s->d_tex_desc;
    r.uvs = s->d_uvs;
    r.depth = depth;
    r.position = position;
    r.normal = normal;
    r.albedo = albedo;
    r.ids = ids;
    Staging stage(&s->d_img_work, &s->img_work_bytes);
    if (!on_device) {
        if (depth) stage.out(&r.depth, depth, px * 4);
        if (position) stage.out(&r.position, position, px * 12);
        if (normal) stage.out(&r.normal, normal, px * 12);
        if (albedo) stage.out(&r.albedo, albedo, px * 12);
        if (ids) stage.out(&r.ids, ids, px * 12);
    }
    st = stage.commit(s->stream, nullptr);
    if (st != FF_OK) return st;
    FF_HIP(launch_gbuffer_resolve(r, s->stream));
    FF_HIP(hipStreamSynchronize(s->stream));
    if (ph.fresh) {
        unsigned long long cut = 0;
        FF_HIP(hipMemcpy(&cut, s->d_counters, sizeof cut, hipMemcpyDeviceToHost));
        if (cut != 0) return fail(FF_ERR_HIP, "ff_gbuffer: the traversal loop guard cut %llu queries short (a malformed or absurdly deep tree)", cut);
    }
    return stage.finish();
}

void ff_denoise_params_init(FfDenoiseParams* p)
{
    if (!p) return;
    // (cornell_wahoo at the C2 pose, 320x180, 16 spp against 4 096 spp: the MSE falls to 0.32 of the raw frame's;
    // sigma_color 1 / 2 / 4 / 8 leave 0.38 / 0.34 / 0.32 / 0.33; the other two sigmas move it by less than 0.002)
    p->iterations = 5;
    p->sigma_color = 4.0f;
    p->sigma_normal = 0.1f;
    p->sigma_plane = 0.1f;
    p->flags = FF_DENOISE_SAME_GEOMETRY | FF_DENOISE_DEMODULATE_ALBEDO;
}

int ff_denoise(FfState* s, int width, int height, const FfDenoiseParams* dn, const float* radiance_in, const float* position, const float* normal,
               const float* albedo, const int32_t* ids, int inputs_on_device, void* rgb8, int rgb8_on_device, float* radiance_out,
               int radiance_out_on_device)
{
    clear_error();
    int st = check_image_call(s, false, nullptr, dn, width, height, "ff_denoise");
    if (st == FF_OK) st = check_iterations(dn->iterations, "ff_denoise");
    if (st == FF_OK) st = check_sigmas(dn->sigma_color, dn->sigma_normal, dn->sigma_plane, "ff_denoise");
    int demod = 0;
    if (st == FF_OK) st = check_guides(dn->flags, radiance_in, position, normal, albedo, ids, &demod, "ff_denoise");
    if (st != FF_OK) return st;
    FF_HIP(hipSetDevice(s->device));
    const size_t px = (size_t)width * (size_t)height;
    const bool filter = dn->iterations > 0;
    hipStream_t stream = s->stream;
    // host buffers are staged: the inputs the call reads, the outputs it writes
    const float* d_rad = radiance_in;
    const float* d_pos = position;
    const float* d_nrm = normal;
    const float* d_alb = demod ? albedo : nullptr;
    const int* d_ids = ids;
    Staging stage(&s->d_img_work, &s->img_work_bytes);
    if (!inputs_on_device) {
        stage.in(&d_rad, radiance_in, px * 12);
        if (filter) {
            stage.in(&d_pos, position, px * 12);
            stage.in(&d_nrm, normal, px * 12);
            if (demod) stage.in(&d_alb, albedo, px * 12);
            stage.in(&d_ids, ids, px * 12);
        }
    }
    StagedOutputs out(stage, px, rgb8, rgb8_on_device, radiance_out, radiance_out_on_device);
    st = stage.commit(stream, "ff_denoise: staging the inputs failed");
    if (st != FF_OK) return st;
    DenoiseBuffers b;
    b.width = width;
    b.height = height;
    b.guide_pos = b.guide_nrm = b.color[0] = b.color[1] = nullptr;
    int src = -1;
    if (filter) {
        st = ensure_bytes((void**)&s->d_dn_work, &s->dn_work_bytes, 4 * px * sizeof(float4));
        if (st != FF_OK) return st;
        b.guide_pos = s->d_dn_work;
        b.guide_nrm = s->d_dn_work + px;
        b.color[0] = s->d_dn_work + 2 * px;
        b.color[1] = s->d_dn_work + 3 * px;
        FF_HIP(launch_denoise_pack(b, d_rad, d_pos, d_nrm, d_alb, d_ids, demod, stream));
        src = 0;
        const int same = (dn->flags & FF_DENOISE_SAME_GEOMETRY) ? 1 : 0;
        for (int i = 0; i < dn->iterations; ++i) {
            const double sigma_i = (double)dn->sigma_color * std::ldexp(1.0, -i); // halved every pass
            FF_HIP(launch_denoise_pass(b, src, i, (float)(1.0 / (sigma_i * sigma_i)), (float)(1.0 / (double)dn->sigma_normal),
                                       dn->sigma_plane * dn->sigma_plane, same, stream));
            src = 1 - src;
        }
    }
    FF_HIP(launch_denoise_finish(b, src, d_rad, d_alb, demod, out.rgb8, out.radiance, stream));
    FF_HIP(hipStreamSynchronize(stream));
    return stage.finish();
}

// ---- temporal denoiser (SVGF; kernels in ff_temporal.hip) ---------------------------------------------------------

void ff_temporal_params_init(FfTemporalParams* p)
{
    if (!p) return;
    // (the paper's values, with max_history chosen on the C2 scene's moving camera)
    p->iterations = 5;
    p->sigma_luminance = 4.0f;
    p->sigma_normal = 0.1f;
    p->sigma_plane = 0.1f;
    p->flags = FF_DENOISE_SAME_GEOMETRY | FF_DENOISE_DEMODULATE_ALBEDO;
    p->max_history = 16;
    p->variance_history = 4;
    p->feedback_pass = 0;
    p->reuse_normal = 0.9f;
    p->reuse_plane = 0.01f;
}

int ff_denoise_temporal(FfState* s, const FfCamera* camera, int width, int height, const FfTemporalParams* tp, const float* radiance_in,
                        const float* position, const float* normal, const float* albedo, const int32_t* ids, int inputs_on_device, void* rgb8,
                        int rgb8_on_device, float* radiance_out, int radiance_out_on_device)
{
    clear_error();
    int st = check_image_call(s, true, camera, tp, width, height, "ff_denoise_temporal");
    if (st == FF_OK) st = check_iterations(tp->iterations, "ff_denoise_temporal");
    if (st != FF_OK) return st;
    if (tp->feedback_pass < -1 || tp->feedback_pass >= tp->iterations)
        return fail(FF_ERR_INVALID_ARG, "ff_denoise_temporal: feedback_pass must be in -1..iterations-1 (got %d)", tp->feedback_pass);
    if (tp->max_history < 1) return fail(FF_ERR_INVALID_ARG, "ff_denoise_temporal: max_history must be at least 1 (got %d)", tp->max_history);
    if (tp->variance_history < 1) return fail(FF_ERR_INVALID_ARG, "ff_denoise_temporal: variance_history must be at least 1 (got %d)", tp->variance_history);
    st = check_sigmas(tp->sigma_luminance, tp->sigma_normal, tp->sigma_plane, "ff_denoise_temporal");
    if (st != FF_OK) return st;
    if (!std::isfinite(tp->reuse_normal) || !(tp->reuse_plane >= 0.f) || !std::isfinite(tp->reuse_plane))
        return fail(FF_ERR_INVALID_ARG, "ff_denoise_temporal: reuse_normal must be finite and reuse_plane finite and >= 0");
    int demod = 0;
    st = check_guides(tp->flags, radiance_in, position, normal, albedo, ids, &demod, "ff_denoise_temporal");
    if (st != FF_OK) return st;
    if (!s->has_scene) return fail(FF_ERR_NO_SCENE, "ff_denoise_temporal: no scene uploaded (the history follows its geometries)");
    FF_HIP(hipSetDevice(s->device));
    const size_t px = (size_t)width * (size_t)height;
    hipStream_t stream = s->stream;
    // host buffers are staged, as in ff_denoise
    const float* d_rad = radiance_in;
    const float* d_pos = position;
    const float* d_nrm = normal;
    const float* d_alb = demod ? albedo : nullptr;
    const int* d_ids = ids;
    Staging stage(&s->d_img_work, &s->img_work_bytes);
    if (!inputs_on_device) {
        stage.in(&d_rad, radiance_in, px * 12);
        stage.in(&d_pos, position, px * 12);
        stage.in(&d_nrm, normal, px * 12);
        if (demod) stage.in(&d_alb, albedo, px * 12);
        stage.in(&d_ids, ids, px * 12);
    }
    StagedOutputs out(stage, px, rgb8, rgb8_on_device, radiance_out, radiance_out_on_device);
    st = stage.commit(stream, "ff_denoise_temporal: staging the inputs failed");
    if (st != FF_OK) return st;
    // history: kept only for the same image size (a new size, a reset or a new scene start afresh)
    ReprojectionHistory& hist = s->history[FfState::kHistoryTemporal];
    ReprojectionHistory::Frame f;
    st = hist.begin(s->h_geoms, width, height, 10 * px * sizeof(float4) + px * sizeof(float2), stream, &f);
    if (st != FF_OK) return st;
    const TemporalBuffers b = temporal_buffers(hist.d_work, width, height);
    TemporalReproject r;
    std::memset(&r, 0, sizeof r);
    r.cur = f.cur;
    r.has_history = f.has_history ? 1 : 0;
    r.num_geoms = f.num;
    r.geoms = f.geoms;
    if (f.has_history) {
        r.at_rest = std::memcmp(camera, &hist.camera, sizeof(FfCamera)) == 0 ? 1 : 0;
        FfMat4 cm;
        if (!inverse_ray_matrix(&hist.camera, r.proj, &cm)) return fail(FF_ERR_INVALID_ARG, "ff_denoise_temporal: the previous camera's ray matrix is singular");
        r.eye[0] = hist.camera.m_position.x;
        r.eye[1] = hist.camera.m_position.y;
        r.eye[2] = hist.camera.m_position.z;
        r.screen_w = hist.camera.m_screenWidth;
        r.screen_h = hist.camera.m_screenHeight;
    }
    r.reuse_normal = tp->reuse_normal;
    r.reuse_plane = tp->reuse_plane;
    r.max_history = (float)tp->max_history;
    r.variance_history = (float)tp->variance_history;
    r.demodulate = demod;
    r.feedback_unfiltered = tp->feedback_pass < 0 ? 1 : 0;
    FF_HIP(launch_temporal_reproject(b, r, d_rad, d_pos, d_nrm, d_alb, d_ids, stream));
    int src = 0;
    if (tp->iterations > 0) {
        const float inv_sigma_normal = (float)(1.0 / (double)tp->sigma_normal), sigma_plane2 = tp->sigma_plane * tp->sigma_plane;
        FF_HIP(launch_temporal_variance(b, r.cur, r.variance_history, inv_sigma_normal, sigma_plane2, stream));
        const int same = (tp->flags & FF_DENOISE_SAME_GEOMETRY) ? 1 : 0;
        for (int i = 0; i < tp->iterations; ++i) {
            FF_HIP(launch_temporal_pass(b, r.cur, src, i, tp->sigma_luminance, inv_sigma_normal, sigma_plane2, same,
                                        i == tp->feedback_pass ? b.col[r.cur] : nullptr, stream));
            src = 1 - src;
        }
    }
    // output: ff_denoise's finish on the last colour buffer (the class in the guide's w decides what is copied through)
    DenoiseBuffers fb;
    fb.width = width;
    fb.height = height;
    fb.guide_pos = b.pos[r.cur];
    fb.guide_nrm = b.nrm[r.cur];
    fb.color[0] = b.work[src];
    fb.color[1] = b.work[1 - src];
    FF_HIP(launch_denoise_finish(fb, 0, d_rad, d_alb, demod, out.rgb8, out.radiance, stream));
    FF_HIP(hipStreamSynchronize(stream));
    hist.commit(s->h_geoms, camera, width, height, f);
    return stage.finish();
}

int ff_temporal_reset(FfState* s) { return history_reset(s, FfState::kHistoryTemporal, "ff_temporal_reset"); }

int ff_temporal_history(FfState* s, float* motion, float* length, int on_device)
{
    return history_readback(s, FfState::kHistoryTemporal, "ff_temporal_history", "ff_denoise_temporal", motion, length, on_device,
                            [s](const ReprojectionHistory& h, float* d_motion, float* d_length) {
                                return launch_temporal_history(temporal_buffers(h.d_work, h.width, h.height), h.cur, d_motion, d_length, s->stream);
                            });
}

// ---- temporal anti-aliasing (kernel in ff_taa.hip) ------------------------------------------------------------------

void ff_taa_params_init(FfTaaParams* p)
{
    if (!p) return;
    // 
    p->alpha_min = 0.1f;
    p->gamma = 1.0f;
    p->flags = 0;
    p->reserved = 0;
}

int ff_taa(FfState* s, const FfCamera* camera, int width, int height, const FfTaaParams* p, const float* radiance_in, const float* position,
           const int32_t* ids, int inputs_on_device, void* rgb8, int rgb8_on_device, float* radiance_out, int radiance_out_on_device)
{
    clear_error();
    int st = check_image_call(s, true, camera, p, width, height, "ff_taa");
    if (st != FF_OK) return st;
    if (!(p->alpha_min > 0.f && p->alpha_min <= 1.f)) return fail(FF_ERR_INVALID_ARG, "ff_taa: alpha_min must be in (0, 1] (got %g)", (double)p->alpha_min);
    if (!(p->gamma > 0.f) || !std::isfinite(p->gamma)) return fail(FF_ERR_INVALID_ARG, "ff_taa: gamma must be positive and finite (got %g)", (double)p->gamma);
    if (p->flags & ~(FF_TAA_BILINEAR | FF_TAA_NO_CLAMP)) return fail(FF_ERR_INVALID_ARG, "ff_taa: unknown flags 0x%x", p->flags);
    if (p->reserved != 0) return fail(FF_ERR_INVALID_ARG, "ff_taa: reserved must be 0");
    if (!radiance_in || !position || !ids) return fail(FF_ERR_INVALID_ARG, "ff_taa: radiance, position and ids are required");
    if (!s->has_scene) return fail(FF_ERR_NO_SCENE, "ff_taa: no scene uploaded (the history follows its geometries)");
    FF_HIP(hipSetDevice(s->device));
    const size_t px = (size_t)width * (size_t)height;
    hipStream_t stream = s->stream;
    // host buffers are staged, as in ff_denoise; a device radiance_out that overlaps radiance_in reads a copy of the input (the
    // kernel's apron reads neighbours that another workgroup may already have written)
    const bool in_host = !inputs_on_device, out_host = radiance_out && !radiance_out_on_device;
    const char* rin = (const char*)radiance_in;
    const char* rout = (const char*)radiance_out;
    const bool alias = !in_host && !out_host && radiance_out && rin < rout + px * 12 && rout < rin + px * 12;
    const float* d_rad = radiance_in;
    const float* d_pos = position;
    const int* d_ids = ids;
    Staging stage(&s->d_img_work, &s->img_work_bytes);
    if (in_host) {
        stage.in(&d_rad, radiance_in, px * 12);
        stage.in(&d_pos, position, px * 12);
        stage.in(&d_ids, ids, px * 12);
    } else if (alias) {
        stage.in(&d_rad, radiance_in, px * 12, hipMemcpyDeviceToDevice);
    }
    StagedOutputs out(stage, px, rgb8, rgb8_on_device, radiance_out, radiance_out_on_device);
    st = stage.commit(stream, in_host ? "ff_taa: staging the inputs failed" : "ff_taa: copying the input failed");
    if (st != FF_OK) return st;
    // history: kept only for the same image size (a new size, a reset or a new scene start afresh); the per-geometry table holds
    // ff_denoise_temporal's rows from the TAA history's model matrices
    ReprojectionHistory& hist = s->history[FfState::kHistoryTaa];
    ReprojectionHistory::Frame f;
    st = hist.begin(s->h_geoms, width, height, 2 * px * sizeof(float4) + px * sizeof(float2), stream, &f);
    if (st != FF_OK) return st;
    TaaArgs a = taa_buffers(hist.d_work, width, height, f.cur);
    a.has_history = f.has_history ? 1 : 0;
    a.bilinear = (p->flags & FF_TAA_BILINEAR) ? 1 : 0;
    a.clamp = (p->flags & FF_TAA_NO_CLAMP) ? 0 : 1;
    a.alpha_min = p->alpha_min;
    a.gamma = p->gamma;
    FfMat4 cm;
    if (!inverse_ray_matrix(camera, a.inv_cur, &cm)) return fail(FF_ERR_INVALID_ARG, "ff_taa: the camera's ray matrix is singular");
    std::memcpy(a.ray, cm.m, sizeof a.ray);
    a.far_clip = camera->m_farClip;
    a.screen_w = camera->m_screenWidth;
    a.screen_h = camera->m_screenHeight;
    a.num_geoms = f.num;
    a.geoms = f.geoms;
    if (f.has_history) {
        a.cam_rest = std::memcmp(camera, &hist.camera, sizeof(FfCamera)) == 0 ? 1 : 0;
        FfMat4 pm;
        if (!inverse_ray_matrix(&hist.camera, a.inv_prev, &pm)) return fail(FF_ERR_INVALID_ARG, "ff_taa: the previous camera's ray matrix is singular");
        a.prev_screen_w = hist.camera.m_screenWidth;
        a.prev_screen_h = hist.camera.m_screenHeight;
    }
    FF_HIP(launch_taa(a, d_rad, d_pos, d_ids, out.rgb8, out.radiance, stream));
    FF_HIP(hipStreamSynchronize(stream));
    hist.commit(s->h_geoms, camera, width, height, f);
    return stage.finish();
}

int ff_taa_reset(FfState* s) { return history_reset(s, FfState::kHistoryTaa, "ff_taa_reset"); }

int ff_taa_history(FfState* s, float* motion, float* length, int on_device)
{
    return history_readback(s, FfState::kHistoryTaa, "ff_taa_history", "ff_taa", motion, length, on_device,
                            [s](const ReprojectionHistory& h, float* d_motion, float* d_length) {
                                return launch_taa_history(taa_buffers(h.d_work, h.width, h.height, h.cur), d_motion, d_length, s->stream);
                            });
}

// ---- temporal upsampling (kernel in ff_taa_upscale.hip) ---------------------------------------------------------------------

void ff_taa_upscale_params_init(FfTaaUpscaleParams* p)
{
    if (!p) return;
    // (ff_taa's: DESIGN.md section 8 rows 7 and 15)
    p->alpha_min = 0.1f;
    p->gamma = 1.0f;
    p->lo_jitter[0] = p->lo_jitter[1] = 0.f;
    p->flags = 0;
    p->reserved = 0;
}

int ff_taa_upscale(FfState* s, const FfCamera* camera, const FfTaaUpscaleParams* p, int lo_width, int lo_height, const float* radiance_lo,
                   const int32_t* ids_lo, int width, int height, const float* position, const int32_t* ids, int inputs_on_device, void* rgb8,
                   int rgb8_on_device, float* radiance_out, int radiance_out_on_device)
{
    const char* who = "ff_taa_upscale";
    clear_error();
    // every check comes before the device and the history are touched: a refused call leaves both as they were
    if (!s) return fail(FF_ERR_INVALID_ARG, "%s: state is null", who);
    if (!camera) return fail(FF_ERR_INVALID_ARG, "%s: camera is null", who);
    if (!p) return fail(FF_ERR_INVALID_ARG, "%s: params are null", who);
    if (lo_width < 1 || lo_height < 1) return fail(FF_ERR_INVALID_ARG, "%s: lo_width x lo_height %dx%d is invalid", who, lo_width, lo_height);
    if (width > 65535 || height > 65535) return fail(FF_ERR_INVALID_ARG, "%s: width x height %dx%d is invalid (at most 65535)", who, width, height);
    if (width < lo_width || (long long)width > 8ll * lo_width)
        return fail(FF_ERR_INVALID_ARG, "%s: width %d must be in lo_width .. 8 lo_width (lo_width %d)", who, width, lo_width);
    if (height < lo_height || (long long)height > 8ll * lo_height)
        return fail(FF_ERR_INVALID_ARG, "%s: height %d must be in lo_height .. 8 lo_height (lo_height %d)", who, height, lo_height);
    if (!(p->alpha_min > 0.f && p->alpha_min <= 1.f)) return fail(FF_ERR_INVALID_ARG, "%s: alpha_min must be in (0, 1] (got %g)", who, (double)p->alpha_min);
    if (!(p->gamma > 0.f) || !std::isfinite(p->gamma)) return fail(FF_ERR_INVALID_ARG, "%s: gamma must be positive and finite (got %g)", who, (double)p->gamma);
    if (!(p->lo_jitter[0] >= 0.f && p->lo_jitter[0] < 1.f && p->lo_jitter[1] >= 0.f && p->lo_jitter[1] < 1.f))
        return fail(FF_ERR_INVALID_ARG, "%s: lo_jitter must be in [0, 1) (got %g %g)", who, (double)p->lo_jitter[0], (double)p->lo_jitter[1]);
    if (p->flags & ~(FF_TAA_BILINEAR | FF_TAA_NO_CLAMP)) return fail(FF_ERR_INVALID_ARG, "%s: unknown flags 0x%x", who, p->flags);
    if (p->reserved != 0) return fail(FF_ERR_INVALID_ARG, "%s: reserved must be 0", who);
    if (!radiance_lo) return fail(FF_ERR_INVALID_ARG, "%s: radiance_lo is null", who);
    if (!ids_lo) return fail(FF_ERR_INVALID_ARG, "%s: ids_lo is null", who);
    if (!position) return fail(FF_ERR_INVALID_ARG, "%s: position is null", who);
    if (!ids) return fail(FF_ERR_INVALID_ARG, "%s: ids is null", who);
    TaaUpscaleArgs a;
    std::memset(&a, 0, sizeof a);
    FfMat4 cm;
    bool invertible = inverse_ray_matrix(camera, a.taa.inv_cur, &cm);
    for (int k = 0; k < 16; ++k) invertible = invertible && std::isfinite(a.taa.inv_cur[k]); // (a degenerate camera gives NaN, not 0)
    if (!invertible) return fail(FF_ERR_INVALID_ARG, "%s: the camera's ray matrix is singular", who);
    if (!s->has_scene) return fail(FF_ERR_NO_SCENE, "%s: no scene uploaded (the history follows its geometries)", who);
    ReprojectionHistory& hist = s->history[FfState::kHistoryTaaUpscale];
    float inv_prev[16] = {};
    if (hist.valid) {
        FfMat4 pm;
        if (!inverse_ray_matrix(&hist.camera, inv_prev, &pm)) return fail(FF_ERR_INVALID_ARG, "%s: the previous camera's ray matrix is singular", who);
    }
    FF_HIP(hipSetDevice(s->device));
    const size_t lo_px = (size_t)lo_width * (size_t)lo_height, px = (size_t)width * (size_t)height;
    hipStream_t stream = s->stream;
    // host buffers are staged, as in ff_upscale: the inputs the call reads, the outputs it writes
    const float* d_rad = radiance_lo;
    const int* d_ids_lo = ids_lo;
    const float* d_pos = position;
    const int* d_ids = ids;
    Staging stage(&s->d_img_work, &s->img_work_bytes);
    if (!inputs_on_device) {
        stage.in(&d_rad, radiance_lo, lo_px * 12);
        stage.in(&d_ids_lo, ids_lo, lo_px * 12);
        stage.in(&d_pos, position, px * 12);
        stage.in(&d_ids, ids, px * 12);
    }
    StagedOutputs out(stage, px, rgb8, rgb8_on_device, radiance_out, radiance_out_on_device);
    int st = stage.commit(stream, "ff_taa_upscale: staging the inputs failed");
    if (st != FF_OK) return st;
    // history: ff_taa's, on the high grid; kept only while both sizes stay what they were
    if (lo_width != s->taa_upscale_lo_width || lo_height != s->taa_upscale_lo_height) hist.invalidate();
    ReprojectionHistory::Frame f;
    st = hist.begin(s->h_geoms, width, height, 2 * px * sizeof(float4) + px * sizeof(float2), stream, &f);
    if (st != FF_OK) return st;
    const TaaArgs buffers = taa_buffers(hist.d_work, width, height, f.cur);
    a.taa.width = width;
    a.taa.height = height;
    a.taa.cur = f.cur;
    a.taa.hist[0] = buffers.hist[0];
    a.taa.hist[1] = buffers.hist[1];
    a.taa.motion = buffers.motion;
    a.taa.has_history = f.has_history ? 1 : 0;
    a.taa.bilinear = (p->flags & FF_TAA_BILINEAR) ? 1 : 0;
    a.taa.clamp = (p->flags & FF_TAA_NO_CLAMP) ? 0 : 1;
    a.taa.alpha_min = p->alpha_min;
    a.taa.gamma = p->gamma;
    std::memcpy(a.taa.ray, cm.m, sizeof a.taa.ray);
    a.taa.far_clip = camera->m_farClip;
    a.taa.screen_w = camera->m_screenWidth;
    a.taa.screen_h = camera->m_screenHeight;
    a.taa.num_geoms = f.num;
    a.taa.geoms = f.geoms;
    if (f.has_history) {
        a.taa.cam_rest = std::memcmp(camera, &hist.camera, sizeof(FfCamera)) == 0 ? 1 : 0;
        std::memcpy(a.taa.inv_prev, inv_prev, sizeof inv_prev);
        a.taa.prev_screen_w = hist.camera.m_screenWidth;
        a.taa.prev_screen_h = hist.camera.m_screenHeight;
    }
    a.lo_width = lo_width;
    a.lo_height = lo_height;
    a.lo_jx = p->lo_jitter[0];
    a.lo_jy = p->lo_jitter[1];
    a.sx = (float)width / (float)lo_width;
    a.sy = (float)height / (float)lo_height;
    FF_HIP(launch_taa_upscale(a, d_rad, d_ids_lo, d_pos, d_ids, out.rgb8, out.radiance, stream));
    FF_HIP(hipStreamSynchronize(stream));
    hist.commit(s->h_geoms, camera, width, height, f);
    s->taa_upscale_lo_width = lo_width;
    s->taa_upscale_lo_height = lo_height;
    return stage.finish();
}

int ff_taa_upscale_reset(FfState* s) { return history_reset(s, FfState::kHistoryTaaUpscale, "ff_taa_upscale_reset"); }

int ff_taa_upscale_history(FfState* s, float* motion, float* length, int on_device)
{
    return history_readback(s, FfState::kHistoryTaaUpscale, "ff_taa_upscale_history", "ff_taa_upscale", motion, length, on_device,
                            [s](const ReprojectionHistory& h, float* d_motion, float* d_length) {
                                return launch_taa_history(taa_buffers(h.d_work, h.width, h.height, h.cur), d_motion, d_length, s->stream);
                            });
}

} // extern "C"
