// ff_glossy.cpp — rough-specular mirrors (include/firefly/ff_api.h): the scene's roughness bindings with their device table, and the
// host twins of the lobe (ff_glossy_eval, ff_glossy_sample: ff_glossy.h's inline functions compiled for the host).
#include <cmath>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "ff_state.h"
#include "ff_glossy.h"

using namespace ff;

namespace {

int check_lobe(float alpha, const float* f0_rgb, const char* who)
{
    if (!std::isfinite(alpha) || !(alpha > 0.f) || alpha > 1.f) return fail(FF_ERR_INVALID_ARG, "%s: alpha %g is not in (0, 1]", who, (double)alpha);
    if (!f0_rgb) return fail(FF_ERR_INVALID_ARG, "%s: f0_rgb is null", who);
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(f0_rgb[k])) return fail(FF_ERR_INVALID_ARG, "%s: f0_rgb[%d] is not finite", who, k);
    return FF_OK;
}

} // namespace

namespace ff {

void glossy_drop_bindings(FfState* s)
{
    s->glossy_roughness.clear();
    s->glossy_applied = 0;
}

// The device table from the bindings: alpha per record (processing order), 0 where no binding is applied or the lobe is too narrow.
int glossy_sync_table(FfState* s)
{
    s->glossy_applied = 0;
    if (!s->has_scene) return FF_OK;
    std::vector<float> alpha(std::max<size_t>(s->h_geoms.size(), 1), 0.f);
    for (size_t r = 0; r < s->h_geoms.size(); ++r) {
        const GeomRecord& g = s->h_geoms[r];
        const int o = g.orig_index;
        if (o < 0 || (size_t)o >= s->glossy_roughness.size()) continue;
        const float rough = s->glossy_roughness[(size_t)o];
        if (!(rough > 0.f) || g.bxdf_type != FF_BXDF_MIRROR) continue;
        ++s->glossy_applied;
        const float a = rough * rough;
        alpha[r] = a < kGlossyMinAlpha ? 0.f : a;
    }
    if (s->glossy_applied == 0) return FF_OK;
    FF_HIP(hipSetDevice(s->device));
    FF_HIP(hipStreamSynchronize(s->stream)); // (a frame in flight may still read the table)
    const int st = ensure_bytes((void**)&s->d_glossy_alpha, &s->glossy_alpha_bytes, alpha.size() * sizeof(float));
    if (st != FF_OK) return st;
    FF_HIP(hipMemcpy(s->d_glossy_alpha, alpha.data(), alpha.size() * sizeof(float), hipMemcpyHostToDevice));
    return FF_OK;
}

void glossy_release(FfState* s)
{
    glossy_drop_bindings(s);
    if (s->d_glossy_alpha) (void)hipFree(s->d_glossy_alpha);
    s->d_glossy_alpha = nullptr;
    s->glossy_alpha_bytes = 0;
}

} // namespace ff

extern "C" {

int ff_set_roughness(FfState* s, int geometry_index, float roughness)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_set_roughness: state is null");
    if (!s->has_scene) return fail(FF_ERR_NO_SCENE, "ff_set_roughness: no scene uploaded");
    const GeomRecord* rec = nullptr;
    for (const GeomRecord& g : s->h_geoms)
        if (g.orig_index == geometry_index) rec = &g;
    if (geometry_index < 0 || !rec) return fail(FF_ERR_INVALID_ARG, "ff_set_roughness: geometry %d is not in the uploaded scene", geometry_index);
    if (!std::isfinite(roughness) || roughness < 0.f || roughness > 1.f)
        return fail(FF_ERR_INVALID_ARG, "ff_set_roughness: roughness %g is not in [0, 1]", (double)roughness);
    if (roughness > 0.f && rec->bxdf_type != FF_BXDF_MIRROR)
        return fail(FF_ERR_UNSUPPORTED, "ff_set_roughness: geometry %d is not FF_BXDF_MIRROR (rough glass and a glossy coat over diffuse are not offered)",
                    geometry_index);
    if (s->glossy_roughness.size() <= (size_t)geometry_index) {
        if (roughness == 0.f) return FF_OK; // (nothing is bound to it)
        s->glossy_roughness.resize((size_t)geometry_index + 1, 0.f);
    }
    s->glossy_roughness[(size_t)geometry_index] = roughness;
    s->primary_valid = s->last_key_valid = false; // (as a texture binding does: the mega-kernels' frames start afresh)
    return glossy_sync_table(s);
}

int ff_glossy_eval(float alpha, const float* f0_rgb, const float* wo, const float* wi, int n, float* out_f_rgb, float* out_pdf)
{
    clear_error();
    const int st = check_lobe(alpha, f0_rgb, "ff_glossy_eval");
    if (st != FF_OK) return st;
    if (n < 0 || (n > 0 && (!wo || !wi || !out_f_rgb || !out_pdf))) return fail(FF_ERR_INVALID_ARG, "ff_glossy_eval: bad direction or output array");
    for (int i = 0; i < n; ++i) {
        const float* o = wo + 3 * (size_t)i;
        const float* w = wi + 3 * (size_t)i;
        const GlossyLobe l = glossy_eval(alpha, f0_rgb[0], f0_rgb[1], f0_rgb[2], o[0], o[1], fmaxf(o[2], kGlossyMinCos), w[0], w[1], w[2]);
        out_f_rgb[3 * (size_t)i] = l.fr;
        out_f_rgb[3 * (size_t)i + 1] = l.fg;
        out_f_rgb[3 * (size_t)i + 2] = l.fb;
        out_pdf[i] = l.pdf;
    }
    return FF_OK;
}

int ff_glossy_sample(float alpha, const float* f0_rgb, const float* wo, const float* u, int n, float* out_wi, float* out_weight_rgb, float* out_pdf)
{
    clear_error();
    const int st = check_lobe(alpha, f0_rgb, "ff_glossy_sample");
    if (st != FF_OK) return st;
    if (n < 0 || (n > 0 && (!wo || !u || !out_wi || !out_weight_rgb || !out_pdf))) return fail(FF_ERR_INVALID_ARG, "ff_glossy_sample: bad input or output array");
    for (int i = 0; i < n; ++i) {
        const float u1 = u[2 * (size_t)i], u2 = u[2 * (size_t)i + 1];
        if (!(u1 >= 0.f && u1 < 1.f && u2 >= 0.f && u2 < 1.f)) return fail(FF_ERR_INVALID_ARG, "ff_glossy_sample: u[%d] is not in [0, 1)^2", i);
        const float* o = wo + 3 * (size_t)i;
        float* w = out_wi + 3 * (size_t)i;
        // (the kernel's u1 is a 24-bit integer over 2^24: the integer is what the direction is computed from)
        const GlossyLobe l = glossy_sample(alpha, f0_rgb[0], f0_rgb[1], f0_rgb[2], o[0], o[1], fmaxf(o[2], kGlossyMinCos), (unsigned)(u1 * 16777216.0f), u2,
                                           w[0], w[1], w[2]);
        out_weight_rgb[3 * (size_t)i] = l.wr;
        out_weight_rgb[3 * (size_t)i + 1] = l.wg;
        out_weight_rgb[3 * (size_t)i + 2] = l.wb;
        out_pdf[i] = l.pdf;
    }
    return FF_OK;
}

} // extern "C"
