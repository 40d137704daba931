// ff_yuv_api.cpp — host side of ff_encode_yuv (include/firefly/ff_api.h): the knots of the three transfers (double, once), the
// argument checks, the knot tables in the state and the staging of host buffers in its image work buffer, the one launch (kernel in
// ff_yuv.hip), the loops of the host-only twin ff_encode_yuv_host over ff_yuv.h's functions, and the YUV4MPEG2 writer.  A pure
// image operation: no scene, no G-buffer, no history.
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include <hip/hip_runtime.h>

#include "ff_state.h"
#include "ff_yuv.h"

using namespace ff;

namespace {

// The three EOTFs of step 4, in double; s in [0, 1], the result in [0, 1].
double eotf(int transfer, double s)
{
    if (transfer == FF_YUV_TRANSFER_SRGB) return s <= 0.04045 ? s / 12.92 : std::pow((s + 0.055) / 1.055, 2.4);
    if (transfer == FF_YUV_TRANSFER_BT709) {
        // BT.709's OETF steps from 0.081 to 0.08125 at 0.081 / 4.5: its inverse is level across that gap.  Without the max the power
        // branch starts BELOW the linear one's end and K_332 < K_331.
        if (s < 0.081) return s / 4.5;
        const double v = std::pow((s + 0.099) / 1.099, 1.0 / 0.45), floor_ = 0.081 / 4.5;
        return v > floor_ ? v : floor_;
    }
    // ST 2084
    const double m1 = 2610.0 / 16384.0, m2 = 2523.0 / 4096.0 * 128.0, c1 = 3424.0 / 4096.0, c2 = 2413.0 / 4096.0 * 32.0, c3 = 2392.0 / 4096.0 * 32.0;
    const double p = std::pow(s, 1.0 / m2);
    const double num = p - c1 > 0.0 ? p - c1 : 0.0;
    return std::pow(num / (c2 - c3 * p), 1.0 / m1);
}

// K_0 .. K_4096 of a transfer, computed once; null for a table that is not strictly increasing from 0 to 1.
const float* yuv_knots(int transfer)
{
    static const struct Tables {
        float k[3][kYuvKnots];
        bool ok[3];
        Tables()
        {
            for (int t = 0; t < 3; ++t) {
                for (int j = 0; j <= kYuvCells; ++j) k[t][j] = (float)eotf(t, (double)j / (double)kYuvCells);
                ok[t] = k[t][0] == 0.f && k[t][kYuvCells] == 1.f;
                for (int j = 0; j < kYuvCells; ++j) ok[t] = ok[t] && k[t][j] < k[t][j + 1];
            }
        }
    } tables;
    return tables.ok[transfer] ? tables.k[transfer] : nullptr;
}

bool known_transfer(int t) { return t == FF_YUV_TRANSFER_BT709 || t == FF_YUV_TRANSFER_SRGB || t == FF_YUV_TRANSFER_PQ; }

// What every entry point that takes the parameter block checks, in this order: the block, the size, the fields.
int check_yuv_params(int width, int height, const FfYuvParams* p, const char* who)
{
    if (!p) return fail(FF_ERR_INVALID_ARG, "%s: params are null", who);
    if (check_image_size(width, height, who) != FF_OK) return FF_ERR_INVALID_ARG;
    if (!known_transfer(p->transfer)) return fail(FF_ERR_INVALID_ARG, "%s: unknown transfer %d", who, p->transfer);
    if (p->matrix != FF_YUV_MATRIX_BT709 && p->matrix != FF_YUV_MATRIX_BT2020) return fail(FF_ERR_INVALID_ARG, "%s: unknown matrix %d", who, p->matrix);
    if (p->range != FF_YUV_RANGE_LIMITED && p->range != FF_YUV_RANGE_FULL) return fail(FF_ERR_INVALID_ARG, "%s: unknown range %d", who, p->range);
    if (p->depth != 8 && p->depth != 10) return fail(FF_ERR_INVALID_ARG, "%s: depth must be 8 or 10 (got %d)", who, p->depth);
    if (p->siting != FF_YUV_SITING_CENTER && p->siting != FF_YUV_SITING_LEFT) return fail(FF_ERR_INVALID_ARG, "%s: unknown siting %d", who, p->siting);
    if (!(p->reference_white_nits > 0.f && p->reference_white_nits <= 10000.f)) // (false for NaN)
        return fail(FF_ERR_INVALID_ARG, "%s: reference_white_nits must be finite and within (0, 10000] (got %g)", who, (double)p->reference_white_nits);
    return FF_OK;
}

void plane_bytes(int width, int height, int depth, size_t* luma_bytes, size_t* chroma_bytes)
{
    const size_t sample = depth == 8 ? 1 : 2;
    *luma_bytes = (size_t)width * (size_t)height * sample;
    *chroma_bytes = (size_t)((width + 1) / 2) * (size_t)((height + 1) / 2) * 2 * sample;
}

// What ff_encode_yuv and its twin check after the parameters: the buffers and their places.  Fills the kernel arguments but the knots.
int check_yuv(int width, int height, const FfYuvParams* p, const float* linear_in, const void* luma, const void* chroma, YuvArgs* a, const char* who)
{
    const int st = check_yuv_params(width, height, p, who);
    if (st != FF_OK) return st;
    if (!linear_in) return fail(FF_ERR_INVALID_ARG, "%s: linear_in is null", who);
    if (!luma) return fail(FF_ERR_INVALID_ARG, "%s: luma is null", who);
    if (!chroma) return fail(FF_ERR_INVALID_ARG, "%s: chroma is null", who);
    size_t lb, cb;
    plane_bytes(width, height, p->depth, &lb, &cb);
    const Span out[2] = { { luma, lb, "luma" }, { chroma, cb, "chroma" } };
    if (check_disjoint(out, { { linear_in, (size_t)width * (size_t)height * 12, "linear_in" } }, who) != FF_OK) return FF_ERR_INVALID_ARG;
    a->width = width;
    a->height = height;
    a->bt2020 = p->matrix == FF_YUV_MATRIX_BT2020;
    a->pq = p->transfer == FF_YUV_TRANSFER_PQ;
    a->full = p->range == FF_YUV_RANGE_FULL;
    a->depth = p->depth;
    a->left = p->siting == FF_YUV_SITING_LEFT;
    a->vec = 0;
    a->scale = p->reference_white_nits / 10000.0f;
    a->knots = nullptr;
    return FF_OK;
}

// The twin: step 5's planes for every pixel, then steps 6 to 8 per chroma sample.
template <int DEPTH>
void encode_host(const YuvArgs& a, const float* in, void* luma, void* chroma)
{
    typedef typename std::conditional<DEPTH == 8, unsigned char, uint16_t>::type Sample;
    constexpr int shift = DEPTH == 8 ? 0 : 6;
    const int w = a.width, h = a.height, cw = (w + 1) / 2, ch = (h + 1) / 2;
    std::vector<float> cb((size_t)w * h), cr((size_t)w * h);
    Sample* L = (Sample*)luma;
    Sample* C = (Sample*)chroma;
    for (size_t i = 0; i < (size_t)w * h; ++i) {
        const YuvPixel px = yuv_pixel<DEPTH>(a, a.knots, in + 3 * i);
        L[i] = (Sample)(px.y << shift);
        cb[i] = px.cb;
        cr[i] = px.cr;
    }
    // plane value at (x, y) with both coordinates clamped into the image
    auto at = [&](const std::vector<float>& plane, int x, int y) {
        x = x < 0 ? 0 : (x > w - 1 ? w - 1 : x);
        y = y > h - 1 ? h - 1 : y;
        return plane[(size_t)y * w + x];
    };
    auto sample = [&](const std::vector<float>& plane, int X, int Y) {
        if (a.left)
            return yuv_chroma_left(at(plane, 2 * X - 1, 2 * Y), at(plane, 2 * X, 2 * Y), at(plane, 2 * X + 1, 2 * Y), at(plane, 2 * X - 1, 2 * Y + 1),
                                   at(plane, 2 * X, 2 * Y + 1), at(plane, 2 * X + 1, 2 * Y + 1));
        return yuv_chroma_center(at(plane, 2 * X, 2 * Y), at(plane, 2 * X + 1, 2 * Y), at(plane, 2 * X, 2 * Y + 1), at(plane, 2 * X + 1, 2 * Y + 1));
    };
    for (int Y = 0; Y < ch; ++Y)
        for (int X = 0; X < cw; ++X) {
            const size_t o = 2 * ((size_t)Y * cw + X);
            C[o] = (Sample)(yuv_quant_chroma<DEPTH>(sample(cb, X, Y), a.full) << shift);
            C[o + 1] = (Sample)(yuv_quant_chroma<DEPTH>(sample(cr, X, Y), a.full) << shift);
        }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

} // namespace

namespace ff {

void yuv_release(FfState* s)
{
    if (s->d_yuv_knots) (void)hipFree(s->d_yuv_knots);
    s->d_yuv_knots = nullptr;
    s->yuv_knots_loaded[0] = s->yuv_knots_loaded[1] = s->yuv_knots_loaded[2] = false;
}

} // namespace ff

extern "C" {

void ff_yuv_params_init(FfYuvParams* p)
{
    if (!p) return;
    // 
    p->transfer = FF_YUV_TRANSFER_BT709;
    p->matrix = FF_YUV_MATRIX_BT709;
    p->range = FF_YUV_RANGE_LIMITED;
    p->depth = 8;
    p->siting = FF_YUV_SITING_LEFT;
    p->reference_white_nits = 203.f;
}

int ff_yuv_plane_bytes(int width, int height, const FfYuvParams* p, uint64_t* luma_bytes, uint64_t* chroma_bytes)
{
    clear_error();
    const int st = check_yuv_params(width, height, p, "ff_yuv_plane_bytes");
    if (st != FF_OK) return st;
    size_t lb, cb;
    plane_bytes(width, height, p->depth, &lb, &cb);
    if (luma_bytes) *luma_bytes = lb;
    if (chroma_bytes) *chroma_bytes = cb;
    return FF_OK;
}

int ff_yuv_knots(int transfer, float* out4097)
{
    clear_error();
    if (!known_transfer(transfer)) return fail(FF_ERR_INVALID_ARG, "ff_yuv_knots: unknown transfer %d", transfer);
    if (!out4097) return fail(FF_ERR_INVALID_ARG, "ff_yuv_knots: out4097 is null");
    const float* k = yuv_knots(transfer);
    if (!k) return fail(FF_ERR_UNSUPPORTED, "ff_yuv_knots: the knots of transfer %d do not rise strictly from 0 to 1", transfer);
    std::memcpy(out4097, k, kYuvKnots * sizeof(float));
    return FF_OK;
}

int ff_encode_yuv(FfState* s, int width, int height, const FfYuvParams* p, const float* linear_in, int input_on_device, void* luma, void* chroma,
                  int outputs_on_device)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_encode_yuv: state is null");
    YuvArgs a;
    const int st = check_yuv(width, height, p, linear_in, luma, chroma, &a, "ff_encode_yuv");
    if (st != FF_OK) return st;
    const float* knots = yuv_knots(p->transfer);
    if (!knots) return fail(FF_ERR_UNSUPPORTED, "ff_encode_yuv: the knots of transfer %d do not rise strictly from 0 to 1", p->transfer);
    FF_HIP(hipSetDevice(s->device));
    hipStream_t stream = s->stream;
    // the three transfers' tables, each uploaded on first use
    if (!s->d_yuv_knots) {
        size_t cap = 0;
        const int kst = ensure_bytes(&s->d_yuv_knots, &cap, 3 * (size_t)kYuvKnotStride * sizeof(float));
        if (kst != FF_OK) return kst;
    }
    float* d_knots = (float*)s->d_yuv_knots + (size_t)p->transfer * kYuvKnotStride;
    if (!s->yuv_knots_loaded[p->transfer]) {
        FF_HIP(hipMemcpyAsync(d_knots, knots, kYuvKnots * sizeof(float), hipMemcpyHostToDevice, stream));
        FF_HIP(hipStreamSynchronize(stream)); // (the host table is static, but a failed copy must not leave the flag set)
        s->yuv_knots_loaded[p->transfer] = true;
    }
    a.knots = d_knots;
    size_t lb, cb;
    plane_bytes(width, height, p->depth, &lb, &cb);
    void* d_luma = luma;
    void* d_chroma = chroma;
    Staging stage(&s->d_img_work, &s->img_work_bytes);
    if (!input_on_device) stage.in(&linear_in, linear_in, (size_t)width * (size_t)height * 12);
    if (!outputs_on_device) {
        stage.out(&d_luma, luma, lb);
        stage.out(&d_chroma, chroma, cb);
    }
    const int staged = stage.commit(stream, "ff_encode_yuv: staging the input failed");
    if (staged != FF_OK) return staged;
    a.vec = (width % 4 == 0 && aligned16(linear_in) && aligned16(d_luma) && aligned16(d_chroma)) ? 1 : 0;
    FF_HIP(launch_encode_yuv(a, linear_in, d_luma, d_chroma, stream));
    FF_HIP(hipStreamSynchronize(stream));
    return stage.finish();
}

int ff_encode_yuv_host(int width, int height, const FfYuvParams* p, const float* linear_in, void* luma, void* chroma)
{
    clear_error();
    YuvArgs a;
    const int st = check_yuv(width, height, p, linear_in, luma, chroma, &a, "ff_encode_yuv_host");
    if (st != FF_OK) return st;
    a.knots = yuv_knots(p->transfer);
    if (!a.knots) return fail(FF_ERR_UNSUPPORTED, "ff_encode_yuv_host: the knots of transfer %d do not rise strictly from 0 to 1", p->transfer);
    if (a.depth == 8)
        encode_host<8>(a, linear_in, luma, chroma);
    else
        encode_host<10>(a, linear_in, luma, chroma);
    return FF_OK;
}

int ff_save_y4m(const char* path, int append, int width, int height, const FfYuvParams* p, const void* luma, const void* chroma)
{
    clear_error();
    if (!path) return fail(FF_ERR_INVALID_ARG, "ff_save_y4m: path is null");
    const int st = check_yuv_params(width, height, p, "ff_save_y4m");
    if (st != FF_OK) return st;
    if (!luma) return fail(FF_ERR_INVALID_ARG, "ff_save_y4m: luma is null");
    if (!chroma) return fail(FF_ERR_INVALID_ARG, "ff_save_y4m: chroma is null");
    const size_t px = (size_t)width * (size_t)height, cpx = (size_t)((width + 1) / 2) * (size_t)((height + 1) / 2);
    const size_t sample = p->depth == 8 ? 1 : 2;
    // planar Y, Cb, Cr; depth 10 as low-aligned little-endian 16-bit codes
    std::vector<unsigned char> frame((px + 2 * cpx) * sample);
    if (p->depth == 8) {
        const unsigned char* C = (const unsigned char*)chroma;
        std::memcpy(frame.data(), luma, px);
        for (size_t i = 0; i < cpx; ++i) {
            frame[px + i] = C[2 * i];
            frame[px + cpx + i] = C[2 * i + 1];
        }
    } else {
        const uint16_t* L = (const uint16_t*)luma;
        const uint16_t* C = (const uint16_t*)chroma;
        auto put = [&](size_t i, uint16_t v) {
            const unsigned code = v >> 6;
            frame[2 * i] = (unsigned char)(code & 255);
            frame[2 * i + 1] = (unsigned char)(code >> 8);
        };
        for (size_t i = 0; i < px; ++i) put(i, L[i]);
        for (size_t i = 0; i < cpx; ++i) {
            put(px + i, C[2 * i]);
            put(px + cpx + i, C[2 * i + 1]);
        }
    }
    FILE* f = std::fopen(path, append ? "ab" : "wb");
    if (!f) return fail(FF_ERR_IO, "ff_save_y4m: cannot open %s: %s", path, std::strerror(errno));
    bool ok = true;
    if (!append) {
        const char* cs = p->depth == 10 ? "C420p10" : (p->siting == FF_YUV_SITING_LEFT ? "C420mpeg2" : "C420jpeg");
        ok = std::fprintf(f, "YUV4MPEG2 W%d H%d F30:1 Ip A1:1 %s XCOLORRANGE=%s\n", width, height, cs, p->range == FF_YUV_RANGE_FULL ? "FULL" : "LIMITED") > 0;
    }
    ok = ok && std::fputs("FRAME\n", f) >= 0;
    ok = ok && std::fwrite(frame.data(), 1, frame.size(), f) == frame.size();
    ok = (std::fclose(f) == 0) && ok;
    if (!ok) return fail(FF_ERR_IO, "ff_save_y4m: writing %s failed", path);
    return FF_OK;
}

} // extern "C"
