// ff_display_api.cpp — host side of the display transform (kernels in ff_display.hip): parameter checks, the exposure from the
// luminance histogram (double), the sRGB threshold table, the call itself, its host-only twins (ff_display_curve,
// ff_display_exposure, ff_srgb_thresholds) and the Radiance .hdr writer.  The formulas are in include/firefly/ff_api.h.
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ff_display.h"
#include "ff_state.h"

using namespace ff;

namespace {

// T_1 .. T_255: float(eotf((b - 0.5) / 255)), computed once
const float* srgb_thresholds()
{
    static const struct Table {
        float t[kDisplayThresholds + 1];
        Table()
        {
            for (int b = 1; b <= kDisplayThresholds; ++b) {
                const double s = ((double)b - 0.5) / 255.0;
                t[b - 1] = (float)(s <= 0.04045 ? s / 12.92 : std::pow((s + 0.055) / 1.055, 2.4));
            }
            t[kDisplayThresholds] = INFINITY;
        }
    } table;
    return table.t;
}

bool finite_positive(float v) { return v > 0.f && std::isfinite(v); }
bool finite_non_negative(float v) { return v >= 0.f && std::isfinite(v); }

// Every range of FfDisplayParams' comments; the message names the field.
int check_params(const FfDisplayParams* p, const char* who)
{
    if (!p) return fail(FF_ERR_INVALID_ARG, "%s: params are null", who);
    if (p->curve != FF_CURVE_CLAMP && p->curve != FF_CURVE_REINHARD && p->curve != FF_CURVE_ACES)
        return fail(FF_ERR_INVALID_ARG, "%s: unknown curve %d", who, p->curve);
    if (p->encoding != FF_ENCODE_LINEAR && p->encoding != FF_ENCODE_SRGB) return fail(FF_ERR_INVALID_ARG, "%s: unknown encoding %d", who, p->encoding);
    if (p->flags & ~(FF_DISPLAY_AUTO_EXPOSURE | FF_DISPLAY_BLOOM)) return fail(FF_ERR_INVALID_ARG, "%s: unknown flags 0x%x", who, p->flags);
    if (!finite_positive(p->exposure)) return fail(FF_ERR_INVALID_ARG, "%s: exposure must be finite and > 0 (got %g)", who, (double)p->exposure);
    if (!finite_positive(p->white)) return fail(FF_ERR_INVALID_ARG, "%s: white must be finite and > 0 (got %g)", who, (double)p->white);
    if (!finite_positive(p->key)) return fail(FF_ERR_INVALID_ARG, "%s: key must be finite and > 0 (got %g)", who, (double)p->key);
    if (!(p->low_percentile >= 0.f && p->low_percentile < 1.f))
        return fail(FF_ERR_INVALID_ARG, "%s: low_percentile must be in [0, 1) (got %g)", who, (double)p->low_percentile);
    if (!(p->high_percentile > p->low_percentile && p->high_percentile <= 1.f))
        return fail(FF_ERR_INVALID_ARG, "%s: high_percentile must be in (low_percentile, 1] (got %g)", who, (double)p->high_percentile);
    if (!finite_positive(p->min_exposure)) return fail(FF_ERR_INVALID_ARG, "%s: min_exposure must be finite and > 0 (got %g)", who, (double)p->min_exposure);
    if (!(p->max_exposure >= p->min_exposure) || !std::isfinite(p->max_exposure))
        return fail(FF_ERR_INVALID_ARG, "%s: max_exposure must be finite and >= min_exposure (got %g)", who, (double)p->max_exposure);
    if (!finite_non_negative(p->adapt_darken)) return fail(FF_ERR_INVALID_ARG, "%s: adapt_darken must be finite and >= 0 (got %g)", who, (double)p->adapt_darken);
    if (!finite_non_negative(p->adapt_brighten))
        return fail(FF_ERR_INVALID_ARG, "%s: adapt_brighten must be finite and >= 0 (got %g)", who, (double)p->adapt_brighten);
    if (!std::isfinite(p->dt)) return fail(FF_ERR_INVALID_ARG, "%s: dt must be finite (got %g)", who, (double)p->dt);
    if (!finite_non_negative(p->bloom_threshold))
        return fail(FF_ERR_INVALID_ARG, "%s: bloom_threshold must be finite and >= 0 (got %g)", who, (double)p->bloom_threshold);
    if (!finite_non_negative(p->bloom_strength))
        return fail(FF_ERR_INVALID_ARG, "%s: bloom_strength must be finite and >= 0 (got %g)", who, (double)p->bloom_strength);
    if (p->bloom_levels < 1 || p->bloom_levels > kDisplayMaxLevels)
        return fail(FF_ERR_INVALID_ARG, "%s: bloom_levels must be 1 .. %d (got %d)", who, kDisplayMaxLevels, p->bloom_levels);
    return FF_OK;
}

// Step 2 of ff_api.h, in double; prev <= 0: no previous exposure.
void compute_exposure(const FfDisplayParams& p, const uint32_t* hist, float prev, float* out_target, float* out_exposure)
{
    if (!(p.flags & FF_DISPLAY_AUTO_EXPOSURE)) {
        *out_target = *out_exposure = p.exposure;
        return;
    }
    const bool has_prev = prev > 0.f;
    double n[kDisplayBins];
    double total = 0.0;
    for (int b = 0; b < kDisplayBins; ++b) {
        n[b] = (double)hist[b];
        total += n[b];
    }
    double target = has_prev ? (double)prev : (double)p.exposure;
    if (total > 0.0) {
        double cut = (double)p.low_percentile * total;
        for (int b = 0; b < kDisplayBins && cut > 0.0; ++b) {
            const double take = std::min(n[b], cut);
            n[b] -= take;
            cut -= take;
        }
        cut = (1.0 - (double)p.high_percentile) * total;
        for (int b = kDisplayBins - 1; b >= 0 && cut > 0.0; --b) {
            const double take = std::min(n[b], cut);
            n[b] -= take;
            cut -= take;
        }
        double mass = 0.0, weighted = 0.0;
        for (int b = 0; b < kDisplayBins; ++b) {
            mass += n[b];
            weighted += n[b] * (((double)b + 0.5) / 8.0 - 16.0);
        }
        if (mass > 0.0) {
            const double m = weighted / mass;
            target = std::min(std::max((double)p.key / std::exp2(m), (double)p.min_exposure), (double)p.max_exposure) * (double)p.exposure;
        }
    }
    double e = target;
    if (has_prev && p.dt > 0.f) {
        const double rate = target < (double)prev ? (double)p.adapt_darken : (double)p.adapt_brighten;
        e = (double)prev * std::exp2((std::log2(target) - std::log2((double)prev)) * (1.0 - std::exp(-(double)p.dt * rate)));
    }
    *out_target = (float)target;
    *out_exposure = (float)e;
}

template <int CURVE>
void curve_values(const FfDisplayParams& p, const float* exposed, int n, float* out_y, unsigned char* out_bytes)
{
    const float w2 = p.white * p.white;
    const float* t = srgb_thresholds();
    for (int i = 0; i < n; ++i) {
        const float y = display_curve<CURVE>(exposed[i], w2);
        if (out_y) out_y[i] = y;
        if (out_bytes) out_bytes[i] = (unsigned char)(p.encoding == FF_ENCODE_SRGB ? display_srgb_u8(y, t) : display_linear_u8(y));
    }
}

// The call behind ff_display and ff_display_to_pbo; the arguments are checked.
int display_run(FfState* s, int width, int height, const FfDisplayParams* p, const float* radiance_in, int input_on_device, void* rgb8,
                int rgb8_on_device, float* display_out, int display_out_on_device)
{
    FF_HIP(hipSetDevice(s->device));
    hipStream_t stream = s->stream;
    const size_t px = (size_t)width * (size_t)height;
    const bool in_host = !input_on_device, out_host = display_out && !display_out_on_device;
    const bool automatic = (p->flags & FF_DISPLAY_AUTO_EXPOSURE) != 0, bloom = (p->flags & FF_DISPLAY_BLOOM) != 0;
    // a device display_out that overlaps radiance_in without being it: the kernel reads a copy of the input
    const char* rin = (const char*)radiance_in;
    const char* rout = (const char*)display_out;
    const bool overlap = !in_host && display_out && !out_host && rin != rout && rin < rout + px * 12 && rout < rin + px * 12;
    // the constants: 256 counters, then the threshold table (uploaded when the buffer is made)
    if (!s->d_disp_const) {
        const int st = ensure_bytes(&s->d_disp_const, &s->disp_const_bytes, 2 * 1024);
        if (st != FF_OK) return st;
        const hipError_t e = hipMemcpy((char*)s->d_disp_const + 1024, srgb_thresholds(), 1024, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            display_release(s);
            return fail(FF_ERR_HIP, "ff_display: uploading the threshold table failed: %s", hipGetErrorString(e));
        }
    }
    unsigned* d_counters = (unsigned*)s->d_disp_const;
    // its use of the state's image work buffer: the pyramid's levels ({rgb, 0} float4 per texel, levels 1 .. n one after another),
    // then the staging of host buffers (and the copy of an overlapping input)
    BloomLevel level[kDisplayMaxLevels + 1] = {};
    size_t need = 0, level_at[kDisplayMaxLevels + 1] = {};
    const int levels = bloom ? p->bloom_levels : 0;
    int lw = width, lh = height;
    for (int j = 1; j <= levels; ++j) {
        lw = (lw + 1) / 2;
        lh = (lh + 1) / 2;
        level[j].w = lw;
        level[j].h = lh;
        level_at[j] = need;
        need += ((size_t)lw * (size_t)lh * sizeof(float4) + 15) & ~(size_t)15;
    }
    const float* d_in = radiance_in;
    Staging stage(&s->d_img_work, &s->img_work_bytes, need);
    if (in_host || overlap) stage.in(&d_in, radiance_in, px * 12, in_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice);
    StagedOutputs out(stage, px, rgb8, rgb8_on_device, display_out, display_out_on_device);
    const int sst = stage.commit(stream, nullptr);
    if (sst != FF_OK) return sst;
    for (int j = 1; j <= levels; ++j) level[j].texels = (float4*)((char*)s->d_img_work + level_at[j]);
    // steps 1 and 2
    uint32_t hist[kDisplayBins] = {};
    if (automatic) {
        FF_HIP(hipMemsetAsync(d_counters, 0, kDisplayBins * sizeof(unsigned), stream));
        FF_HIP(launch_display_histogram(d_in, px, d_counters, s->num_cus, stream));
        FF_HIP(hipMemcpyAsync(hist, d_counters, sizeof hist, hipMemcpyDeviceToHost, stream));
        FF_HIP(hipStreamSynchronize(stream));
    }
    float target = 0.f, exposure = 0.f;
    compute_exposure(*p, hist, s->disp_has_prev ? s->disp_prev_exposure : 0.f, &target, &exposure);
    // step 4: the pyramid down and up again; its last tap is the display kernel's
    if (bloom) {
        FF_HIP(launch_bloom_bright_down(d_in, width, height, exposure, p->bloom_threshold, level[1], stream));
        for (int j = 2; j <= levels; ++j) FF_HIP(launch_bloom_down(level[j - 1], level[j], stream));
        for (int j = levels - 1; j >= 1; --j) FF_HIP(launch_bloom_up(level[j + 1], level[j], stream));
    }
    DisplayArgs a;
    std::memset(&a, 0, sizeof a);
    a.width = width;
    a.height = height;
    a.curve = p->curve;
    a.encoding = p->encoding;
    a.bloom = bloom ? 1 : 0;
    a.exposure = exposure;
    a.w2 = p->white * p->white;
    a.bloom_scale = bloom ? p->bloom_strength / (float)levels : 0.f;
    a.thresholds = (const float*)((const char*)s->d_disp_const + 1024);
    if (bloom) {
        a.u1 = level[1].texels;
        a.u1_w = level[1].w;
        a.u1_h = level[1].h;
    }
    if (out.rgb8 || out.radiance) FF_HIP(launch_display(a, d_in, out.rgb8, out.radiance, stream));
    FF_HIP(hipStreamSynchronize(stream));
    const int fst = stage.finish();
    if (fst != FF_OK) return fst;
    // the state now describes this call
    if (automatic) {
        s->disp_has_prev = true;
        s->disp_prev_exposure = exposure;
    }
    s->disp_called = true;
    s->disp_exposure = exposure;
    s->disp_target = target;
    std::memcpy(s->disp_histogram, hist, sizeof hist);
    return FF_OK;
}

int check_display_call(FfState* s, int width, int height, const FfDisplayParams* p, const float* radiance_in, const char* who)
{
    if (!s) return fail(FF_ERR_INVALID_ARG, "%s: state is null", who);
    const int st = check_params(p, who);
    if (st != FF_OK) return st;
    if (!radiance_in) return fail(FF_ERR_INVALID_ARG, "%s: radiance_in is null", who);
    return check_image_size(width, height, who);
}

} // namespace

namespace ff {

void display_release(FfState* s)
{
    if (s->d_disp_const) (void)hipFree(s->d_disp_const);
    s->d_disp_const = nullptr;
    s->disp_const_bytes = 0;
}

} // namespace ff

extern "C" {

void ff_display_params_init(FfDisplayParams* p)
{
    if (!p) return;
    // 
    p->curve = FF_CURVE_ACES;
    p->encoding = FF_ENCODE_SRGB;
    p->flags = 0;
    p->exposure = 1.f;
    p->white = 4.f;
    p->key = 0.18f;
    p->low_percentile = 0.5f;
    p->high_percentile = 0.95f;
    p->min_exposure = 0.0009765625f; // 2^-10
    p->max_exposure = 1024.f;        // 2^10
    p->adapt_darken = 3.f;
    p->adapt_brighten = 1.f;
    p->dt = 0.f;
    p->bloom_threshold = 1.f;
    p->bloom_strength = 0.05f;
    p->bloom_levels = 5;
}

int ff_display(FfState* s, int width, int height, const FfDisplayParams* p, const float* radiance_in, int input_on_device, void* rgb8, int rgb8_on_device,
               float* display_out, int display_out_on_device)
{
    clear_error();
    const int st = check_display_call(s, width, height, p, radiance_in, "ff_display");
    if (st != FF_OK) return st;
    return display_run(s, width, height, p, radiance_in, input_on_device, rgb8, rgb8_on_device, display_out, display_out_on_device);
}

int ff_display_to_pbo(FfState* s, int width, int height, const FfDisplayParams* p, const float* radiance_in, int input_on_device)
{
    clear_error();
    if (s && !s->pbo_resource) return fail(FF_ERR_GL_UNAVAILABLE, "ff_display_to_pbo: no pixel buffer registered");
    int st = check_display_call(s, width, height, p, radiance_in, "ff_display_to_pbo");
    if (st != FF_OK) return st;
    if (width != s->pbo_width || height != s->pbo_height)
        return fail(FF_ERR_INVALID_ARG, "ff_display_to_pbo: the image is %dx%d but the registered buffer is %dx%d", width, height, s->pbo_width, s->pbo_height);
    FF_HIP(hipSetDevice(s->device));
    void* dptr = nullptr;
    st = map_pbo(s, (size_t)width * (size_t)height * 3, &dptr);
    if (st != FF_OK) return st;
    return unmap_pbo(s, display_run(s, width, height, p, radiance_in, input_on_device, dptr, 1, nullptr, 0));
}

int ff_display_reset(FfState* s)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_display_reset: state is null");
    s->disp_has_prev = false;
    return FF_OK;
}

int ff_display_state(FfState* s, float* out_exposure, float* out_target, uint32_t* out_histogram256)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_display_state: state is null");
    if (!s->disp_called) return fail(FF_ERR_INVALID_ARG, "ff_display_state: no ff_display call yet");
    if (out_exposure) *out_exposure = s->disp_exposure;
    if (out_target) *out_target = s->disp_target;
    if (out_histogram256) std::memcpy(out_histogram256, s->disp_histogram, sizeof s->disp_histogram);
    return FF_OK;
}

int ff_srgb_thresholds(float* out255)
{
    clear_error();
    if (!out255) return fail(FF_ERR_INVALID_ARG, "ff_srgb_thresholds: null argument");
    std::memcpy(out255, srgb_thresholds(), kDisplayThresholds * sizeof(float));
    return FF_OK;
}

int ff_display_curve(const FfDisplayParams* p, const float* exposed, int n, float* out_y, unsigned char* out_bytes)
{
    clear_error();
    const int st = check_params(p, "ff_display_curve");
    if (st != FF_OK) return st;
    if (n < 0 || (n > 0 && !exposed)) return fail(FF_ERR_INVALID_ARG, "ff_display_curve: %d values from a null array", n);
    if (p->curve == FF_CURVE_ACES) curve_values<FF_CURVE_ACES>(*p, exposed, n, out_y, out_bytes);
    else if (p->curve == FF_CURVE_REINHARD) curve_values<FF_CURVE_REINHARD>(*p, exposed, n, out_y, out_bytes);
    else curve_values<FF_CURVE_CLAMP>(*p, exposed, n, out_y, out_bytes);
    return FF_OK;
}

int ff_display_exposure(const FfDisplayParams* p, const uint32_t* histogram256, float previous_exposure, float* out_target, float* out_exposure)
{
    clear_error();
    const int st = check_params(p, "ff_display_exposure");
    if (st != FF_OK) return st;
    if (!histogram256) return fail(FF_ERR_INVALID_ARG, "ff_display_exposure: histogram is null");
    if (!std::isfinite(previous_exposure))
        return fail(FF_ERR_INVALID_ARG, "ff_display_exposure: previous_exposure must be finite (got %g)", (double)previous_exposure);
    float target = 0.f, exposure = 0.f;
    compute_exposure(*p, histogram256, previous_exposure, &target, &exposure);
    if (out_target) *out_target = target;
    if (out_exposure) *out_exposure = exposure;
    return FF_OK;
}

int ff_save_hdr(const char* path, const float* rgb, int width, int height)
{
    clear_error();
    if (!path || !rgb) return fail(FF_ERR_INVALID_ARG, "ff_save_hdr: null argument");
    if (width < 1 || height < 1) return fail(FF_ERR_INVALID_ARG, "ff_save_hdr: the image must be at least 1x1 (got %dx%d)", width, height);
    const size_t n = (size_t)width * (size_t)height;
    std::vector<unsigned char> bytes(n * 4);
    for (size_t i = 0; i < n; ++i) {
        const float* c = rgb + 3 * i;
        for (int k = 0; k < 3; ++k)
            if (!(c[k] >= 0.f) || !(c[k] < 1.7014118346046923e38f)) // 2^127
                return fail(FF_ERR_INVALID_ARG, "ff_save_hdr: texel %zu (row %zu, column %zu) has a value RGBE cannot hold: %g", i, i / (size_t)width,
                            i % (size_t)width, (double)c[k]);
        unsigned char* o = &bytes[4 * i];
        const float m = std::max(c[0], std::max(c[1], c[2]));
        if (m < 1e-32f) {
            o[0] = o[1] = o[2] = o[3] = 0;
            continue;
        }
        int e = 0;
        const float f = std::frexp(m, &e);
        const float scale = (f * 256.f) / m;
        for (int k = 0; k < 3; ++k) o[k] = (unsigned char)std::min((int)(c[k] * scale), 255);
        o[3] = (unsigned char)(e + 128);
    }
    std::FILE* f = std::fopen(path, "wb");
    if (!f) return fail(FF_ERR_IO, "ff_save_hdr: cannot open '%s' for writing: %s", path, std::strerror(errno));
    std::fprintf(f, "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n", height, width);
    const bool wrote = std::fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
    const bool ok = wrote && std::fflush(f) == 0 && !std::ferror(f);
    std::fclose(f);
    if (!ok) return fail(FF_ERR_IO, "ff_save_hdr: write to '%s' failed", path);
    return FF_OK;
}

} // extern "C"
