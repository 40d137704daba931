// ff_resize_api.cpp — host side of ff_resize (include/firefly/ff_api.h): the argument checks, the per-axis tables (computed here in
// double, cached in the state under their key), the intermediate image, the staging of host buffers in the state's image work
// buffer (ff_image.h's helpers), the two launches (kernels in ff_resize.hip) and the loops of the host-only twin ff_resize_host over ff_resize.h's per-tap functions.
// A pure image operation: no scene, no G-buffer, no history.
#include <cmath>
#include <vector>

#include <hip/hip_runtime.h>

#include "ff_resize.h"
#include "ff_state.h"

using namespace ff;

namespace {

bool known_filter(int filter) { return filter >= FF_RESIZE_BOX && filter <= FF_RESIZE_LANCZOS3; }

// k(t) of the header, every formula left to right as written there.
double resize_k(int filter, double t)
{
    const double a = std::fabs(t);
    switch (filter) {
    case FF_RESIZE_BOX:
        return (-0.5 <= t && t < 0.5) ? 1.0 : 0.0;
    case FF_RESIZE_TRIANGLE:
        return a < 1.0 ? 1.0 - a : 0.0;
    case FF_RESIZE_MITCHELL: {
        const double B = 1.0 / 3.0, C = 1.0 / 3.0;
        if (a < 1.0) return ((12.0 - 9.0 * B - 6.0 * C) * a * a * a + (-18.0 + 12.0 * B + 6.0 * C) * a * a + (6.0 - 2.0 * B)) / 6.0;
        if (a < 2.0) return ((-B - 6.0 * C) * a * a * a + (6.0 * B + 30.0 * C) * a * a + (-12.0 * B - 48.0 * C) * a + (8.0 * B + 24.0 * C)) / 6.0;
        return 0.0;
    }
    default: { // FF_RESIZE_LANCZOS3
        const double pi = 3.14159265358979323846;
        if (a >= 3.0) return 0.0;
        if (t == 0.0) return 1.0;
        if (t == std::floor(t)) return 0.0;
        return 3.0 * std::sin(pi * t) * std::sin(pi * t / 3.0) / (pi * pi * t * t);
    }
    }
}

// One axis of n input and N output samples: s, f and r of the header, and T.
struct AxisScale {
    double s, f, r;
    int taps;
};

AxisScale axis_scale(int n, int N, int filter)
{
    static const double radius[4] = { 0.5, 1.0, 2.0, 3.0 };
    AxisScale a;
    a.s = (double)n / (double)N;
    a.f = a.s > 1.0 ? a.s : 1.0;
    a.r = radius[filter] * a.f;
    a.taps = (int)std::ceil(2.0 * a.r);
    return a;
}

// The table of the axis, output-major: first[N], weights[N * T].
void build_table(int n, int N, int filter, int32_t* first, float* weights)
{
    const AxisScale a = axis_scale(n, N, filter);
    double k[kResizeMaxTaps];
    for (int X = 0; X < N; ++X) {
        const double c = ((double)X + 0.5) * a.s - 0.5;
        const int f0 = (int)std::ceil(c - a.r);
        double S = 0.0;
        for (int j = 0; j < a.taps; ++j) {
            k[j] = resize_k(filter, ((double)(f0 + j) - c) / a.f);
            S = S + k[j];
        }
        first[X] = f0;
        for (int j = 0; j < a.taps; ++j) weights[(size_t)X * a.taps + j] = (float)(k[j] / S);
    }
}

// What an axis may be: both sizes 1 .. 65535, neither more than 16 times the other.
int check_axis(int n, int N, const char* in_name, const char* out_name, const char* who)
{
    if (n < 1 || n > 65535) return fail(FF_ERR_INVALID_ARG, "%s: %s %d is outside 1 .. 65535", who, in_name, n);
    if (N < 1 || N > 65535) return fail(FF_ERR_INVALID_ARG, "%s: %s %d is outside 1 .. 65535", who, out_name, N);
    if (N > kResizeMaxRatio * n || n > kResizeMaxRatio * N)
        return fail(FF_ERR_INVALID_ARG, "%s: %s %d and %s %d are more than a factor of %d apart", who, in_name, n, out_name, N, kResizeMaxRatio);
    return FF_OK;
}

// What both entry points check, in this order: the parameter block, the sizes, the parameters, the input, the outputs' places.
int check_resize(const FfResizeParams* p, int in_width, int in_height, const float* radiance_in, int out_width, int out_height, const void* rgb8,
                 const float* radiance_out, const char* who)
{
    if (!p) return fail(FF_ERR_INVALID_ARG, "%s: params are null", who);
    if (check_axis(in_width, out_width, "in_width", "out_width", who) != FF_OK) return FF_ERR_INVALID_ARG;
    if (check_axis(in_height, out_height, "in_height", "out_height", who) != FF_OK) return FF_ERR_INVALID_ARG;
    if (!known_filter(p->filter)) return fail(FF_ERR_INVALID_ARG, "%s: unknown filter %d", who, p->filter);
    if (p->flags & ~(uint32_t)FF_RESIZE_ANTI_RING) return fail(FF_ERR_INVALID_ARG, "%s: unknown flags 0x%x", who, p->flags);
    if (p->reserved != 0) return fail(FF_ERR_INVALID_ARG, "%s: reserved must be 0", who);
    if (!radiance_in) return fail(FF_ERR_INVALID_ARG, "%s: radiance_in is null", who);
    const size_t in_px = (size_t)in_width * (size_t)in_height, out_px = (size_t)out_width * (size_t)out_height;
    return check_outputs_disjoint(rgb8, radiance_out, out_px, { { radiance_in, in_px * 12, "radiance_in" } }, who);
}

// One pass of the twin over one axis: `count` lines of n samples (of 3 floats, `step` samples apart, lines `line` samples apart)
// give lines of N samples in `dst`, laid out the same way with its own strides.
template <bool RING>
void resample_lines(int n, int N, int taps, const int32_t* first, const float* weights, size_t count, const float* src, size_t src_step, size_t src_line,
                    float* dst, size_t dst_step, size_t dst_line)
{
    for (size_t l = 0; l < count; ++l)
        for (int X = 0; X < N; ++X) {
            ResizeSum s[3] = { resize_begin(), resize_begin(), resize_begin() };
            for (int j = 0; j < taps; ++j) {
                const float w = weights[(size_t)X * taps + j];
                const float* v = src + 3 * (l * src_line + (size_t)resize_index(first[X], j, n) * src_step);
                for (int c = 0; c < 3; ++c) resize_tap<RING>(s[c], w, resize_value(v[c]));
            }
            float* o = dst + 3 * (l * dst_line + (size_t)X * dst_step);
            for (int c = 0; c < 3; ++c) o[c] = resize_finish<RING>(s[c]);
        }
}

template <bool RING>
void resize_host(int in_w, int in_h, int out_w, int out_h, int filter, const float* radiance_in, unsigned char* rgb8, float* radiance_out)
{
    const int tx = axis_scale(in_w, out_w, filter).taps, ty = axis_scale(in_h, out_h, filter).taps;
    std::vector<int32_t> fx(out_w), fy(out_h);
    std::vector<float> wx((size_t)out_w * tx), wy((size_t)out_h * ty);
    build_table(in_w, out_w, filter, fx.data(), wx.data());
    build_table(in_h, out_h, filter, fy.data(), wy.data());
    std::vector<float> mid((size_t)out_w * in_h * 3), out((size_t)out_w * out_h * 3);
    resample_lines<RING>(in_w, out_w, tx, fx.data(), wx.data(), (size_t)in_h, radiance_in, 1, (size_t)in_w, mid.data(), 1, (size_t)out_w); // rows
    resample_lines<RING>(in_h, out_h, ty, fy.data(), wy.data(), (size_t)out_w, mid.data(), (size_t)out_w, 1, out.data(), (size_t)out_w, 1); // columns
    for (size_t i = 0; i < (size_t)out_w * out_h; ++i) store_rgb(i, out.data() + 3 * i, rgb8, radiance_out);
}

// The device table of one axis (0: horizontal, tap-major weights; 1: vertical, output-major), rebuilt and uploaded only when its
// key (in, out, filter) changes.
int axis_table(FfState* s, int axis, int n, int N, int filter, hipStream_t stream, ResizeAxis* out)
{
    FfState::ResizeTable& t = s->resize_table[axis];
    const size_t weights_at = ((size_t)N * sizeof(int32_t) + 15) & ~(size_t)15;
    if (!(t.valid && t.in_size == n && t.out_size == N && t.filter == filter)) {
        t.valid = false;
        const int taps = axis_scale(n, N, filter).taps;
        std::vector<int32_t> first(N);
        std::vector<float> weights((size_t)N * taps);
        build_table(n, N, filter, first.data(), weights.data());
        int span = 0;
        if (axis == 0) {
            for (int X0 = 0; X0 < N; X0 += kResizeTileX) {
                const int X1 = X0 + kResizeTileX < N ? X0 + kResizeTileX : N;
                const int len = resize_index(first[X1 - 1], taps - 1, n) - resize_index(first[X0], 0, n) + 1;
                span = len > span ? len : span;
            }
            std::vector<float> by_tap((size_t)N * taps);
            for (int X = 0; X < N; ++X)
                for (int j = 0; j < taps; ++j) by_tap[(size_t)j * N + X] = weights[(size_t)X * taps + j];
            weights.swap(by_tap);
        }
        const int st = ensure_bytes(&t.d_table, &t.bytes, weights_at + weights.size() * sizeof(float));
        if (st != FF_OK) return st;
        FF_HIP(hipMemcpyAsync(t.d_table, first.data(), first.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
        FF_HIP(hipMemcpyAsync((char*)t.d_table + weights_at, weights.data(), weights.size() * sizeof(float), hipMemcpyHostToDevice, stream));
        FF_HIP(hipStreamSynchronize(stream)); // (the host vectors end here, and a failed copy must not leave the key set)
        t.in_size = n;
        t.out_size = N;
        t.filter = filter;
        t.taps = taps;
        t.span = span;
        t.valid = true;
    }
    out->first = (const int32_t*)t.d_table;
    out->weights = (const float*)((const char*)t.d_table + weights_at);
    out->in_size = n;
    out->out_size = N;
    out->taps = t.taps;
    out->span = t.span;
    return FF_OK;
}

} // namespace

namespace ff {

void resize_release(FfState* s)
{
    if (s->d_resize_mid) (void)hipFree(s->d_resize_mid);
    s->d_resize_mid = nullptr;
    s->resize_mid_bytes = 0;
    for (FfState::ResizeTable& t : s->resize_table) {
        if (t.d_table) (void)hipFree(t.d_table);
        t = FfState::ResizeTable();
    }
}

} // namespace ff

extern "C" {

void ff_resize_params_init(FfResizeParams* p)
{
    if (!p) return;
    // 
    p->filter = FF_RESIZE_LANCZOS3;
    p->flags = FF_RESIZE_ANTI_RING;
    p->reserved = 0;
}

int ff_resize_taps(int in_size, int out_size, int filter, int* out_taps)
{
    clear_error();
    if (check_axis(in_size, out_size, "in_size", "out_size", "ff_resize_taps") != FF_OK) return FF_ERR_INVALID_ARG;
    if (!known_filter(filter)) return fail(FF_ERR_INVALID_ARG, "ff_resize_taps: unknown filter %d", filter);
    if (!out_taps) return fail(FF_ERR_INVALID_ARG, "ff_resize_taps: out_taps is null");
    *out_taps = axis_scale(in_size, out_size, filter).taps;
    return FF_OK;
}

int ff_resize_weights(int in_size, int out_size, int filter, int32_t* out_first, float* out_weights)
{
    clear_error();
    if (check_axis(in_size, out_size, "in_size", "out_size", "ff_resize_weights") != FF_OK) return FF_ERR_INVALID_ARG;
    if (!known_filter(filter)) return fail(FF_ERR_INVALID_ARG, "ff_resize_weights: unknown filter %d", filter);
    if (!out_first) return fail(FF_ERR_INVALID_ARG, "ff_resize_weights: out_first is null");
    if (!out_weights) return fail(FF_ERR_INVALID_ARG, "ff_resize_weights: out_weights is null");
    build_table(in_size, out_size, filter, out_first, out_weights);
    return FF_OK;
}

int ff_resize(FfState* s, const FfResizeParams* p, int in_width, int in_height, const float* radiance_in, int input_on_device, int out_width, int out_height,
              void* rgb8, int rgb8_on_device, float* radiance_out, int radiance_out_on_device)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_resize: state is null");
    const int st = check_resize(p, in_width, in_height, radiance_in, out_width, out_height, rgb8, radiance_out, "ff_resize");
    if (st != FF_OK) return st;
    FF_HIP(hipSetDevice(s->device));
    hipStream_t stream = s->stream;
    ResizeArgs a;
    int tst = axis_table(s, 0, in_width, out_width, p->filter, stream, &a.x);
    if (tst == FF_OK) tst = axis_table(s, 1, in_height, out_height, p->filter, stream, &a.y);
    if (tst != FF_OK) return tst;
    a.anti_ring = (p->flags & FF_RESIZE_ANTI_RING) ? 1 : 0;
    a.rows_h = resize_lds_bytes(kResizeRowsH, a.x.span, a.x.taps) <= kResizeLdsBytes ? kResizeRowsH : kResizeRowsHSmall;
    const int mst = ensure_bytes(&s->d_resize_mid, &s->resize_mid_bytes, (size_t)out_width * (size_t)in_height * 12);
    if (mst != FF_OK) return mst;
    const size_t in_px = (size_t)in_width * (size_t)in_height, out_px = (size_t)out_width * (size_t)out_height;
    Staging stage(&s->d_img_work, &s->img_work_bytes);
    if (!input_on_device) stage.in(&radiance_in, radiance_in, in_px * 12);
    StagedOutputs out(stage, out_px, rgb8, rgb8_on_device, radiance_out, radiance_out_on_device);
    const int staged = stage.commit(stream, "ff_resize: staging the input failed");
    if (staged != FF_OK) return staged;
    FF_HIP(launch_resize(a, radiance_in, (float*)s->d_resize_mid, out.rgb8, out.radiance, stream));
    FF_HIP(hipStreamSynchronize(stream));
    return stage.finish();
}

int ff_resize_host(const FfResizeParams* p, int in_width, int in_height, const float* radiance_in, int out_width, int out_height, unsigned char* rgb8,
                   float* radiance_out)
{
    clear_error();
    const int st = check_resize(p, in_width, in_height, radiance_in, out_width, out_height, rgb8, radiance_out, "ff_resize_host");
    if (st != FF_OK) return st;
    if (p->flags & FF_RESIZE_ANTI_RING)
        resize_host<true>(in_width, in_height, out_width, out_height, p->filter, radiance_in, rgb8, radiance_out);
    else
        resize_host<false>(in_width, in_height, out_width, out_height, p->filter, radiance_in, rgb8, radiance_out);
    return FF_OK;
}

} // extern "C"
