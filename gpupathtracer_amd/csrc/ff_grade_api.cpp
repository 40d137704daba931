// ff_grade_api.cpp — host side of ff_color_grade (include/firefly/ff_api.h): the argument checks, the state's LUT objects, the staging
// of host buffers in the state's image work buffer (ff_image.h's helpers), the launch (kernel in ff_grade.hip), the loop of the
// host-only twin ff_color_grade_host over ff_grade.h's per-pixel functions, and the .cube reader and writer.
// A pure image operation: no scene, no G-buffer, no history.
#include <cerrno>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "ff_grade.h"
#include "ff_state.h"

using namespace ff;

namespace {

constexpr uint32_t kGradeFlags = FF_GRADE_PRIMARY | FF_GRADE_CURVES | FF_GRADE_LUT3D | FF_GRADE_TRILINEAR;
constexpr float kGradeMaxValue = FLT_MAX / 2; // a knot or a lattice value: no difference of two overflows

bool finite_f(float v) { return std::isfinite(v); }

// The descriptor's checks, in the header's order.  need_curves / need_table: the half must be there.
int check_lut(const FfGradeLut* l, const char* who)
{
    if (!l) return fail(FF_ERR_INVALID_ARG, "%s: lut is null", who);
    const bool has_curves = l->curve_size != 0 || l->curves, has_table = l->size != 0 || l->table;
    if (!has_curves && !has_table) return fail(FF_ERR_INVALID_ARG, "%s: the lut has neither curves (curve_size, curves) nor a lattice (size, table)", who);
    if (has_curves) {
        if (!l->curves) return fail(FF_ERR_INVALID_ARG, "%s: curve_size %d without curves", who, l->curve_size);
        if (l->curve_size < 2 || l->curve_size > kGradeMaxCurve) return fail(FF_ERR_INVALID_ARG, "%s: curve_size %d is outside 2 .. %d", who, l->curve_size, kGradeMaxCurve);
        if (l->curve_axis != FF_GRADE_AXIS_LINEAR && l->curve_axis != FF_GRADE_AXIS_LOG) return fail(FF_ERR_INVALID_ARG, "%s: unknown curve_axis %d", who, l->curve_axis);
        if (!finite_f(l->curve_lo) || !finite_f(l->curve_hi) || !(l->curve_lo < l->curve_hi) || !finite_f(l->curve_hi - l->curve_lo))
            return fail(FF_ERR_INVALID_ARG, "%s: curve_lo %g and curve_hi %g must be finite, lo < hi, with a finite difference", who, (double)l->curve_lo, (double)l->curve_hi);
        if (l->curve_axis == FF_GRADE_AXIS_LOG) {
            if (!(l->curve_lo > 0.f)) return fail(FF_ERR_INVALID_ARG, "%s: curve_lo %g must be > 0 on FF_GRADE_AXIS_LOG", who, (double)l->curve_lo);
            if (l->curve_shift < 8 || l->curve_shift > 23) return fail(FF_ERR_INVALID_ARG, "%s: curve_shift %d is outside 8 .. 23", who, l->curve_shift);
            const uint32_t lo = grade_bits(l->curve_lo), hi = grade_bits(l->curve_hi), mask = (1u << l->curve_shift) - 1u;
            if ((lo & mask) || (hi & mask))
                return fail(FF_ERR_INVALID_ARG, "%s: the low curve_shift = %d bits of curve_lo's and curve_hi's bit patterns must be 0", who, l->curve_shift);
            const uint32_t knots = ((hi - lo) >> l->curve_shift) + 1u;
            if (knots != (uint32_t)l->curve_size)
                return fail(FF_ERR_INVALID_ARG, "%s: curve_size %d is not the %u knots of curve_lo .. curve_hi at curve_shift %d", who, l->curve_size, knots, l->curve_shift);
        } else if (l->curve_shift != 0) {
            return fail(FF_ERR_INVALID_ARG, "%s: curve_shift %d must be 0 on FF_GRADE_AXIS_LINEAR", who, l->curve_shift);
        }
        for (int i = 0; i < 3 * l->curve_size; ++i)
            if (!(std::fabs(l->curves[i]) <= kGradeMaxValue))
                return fail(FF_ERR_INVALID_ARG, "%s: curves: knot %d of channel %d is %g (knots are finite, at most FLT_MAX / 2 in magnitude)", who, i % l->curve_size,
                            i / l->curve_size, (double)l->curves[i]);
    }
    if (has_table) {
        if (!l->table) return fail(FF_ERR_INVALID_ARG, "%s: size %d without table", who, l->size);
        if (l->size < 2 || l->size > kGradeMaxSize) return fail(FF_ERR_INVALID_ARG, "%s: size %d is outside 2 .. %d", who, l->size, kGradeMaxSize);
        for (int c = 0; c < 3; ++c)
            if (!finite_f(l->domain_min[c]) || !finite_f(l->domain_max[c]) || !(l->domain_min[c] < l->domain_max[c]) || !finite_f(l->domain_max[c] - l->domain_min[c]))
                return fail(FF_ERR_INVALID_ARG, "%s: domain_min[%d] %g and domain_max[%d] %g must be finite, min < max, with a finite difference", who, c,
                            (double)l->domain_min[c], c, (double)l->domain_max[c]);
        const size_t n = (size_t)l->size * l->size * l->size * 3;
        for (size_t i = 0; i < n; ++i)
            if (!(std::fabs(l->table[i]) <= kGradeMaxValue))
                return fail(FF_ERR_INVALID_ARG, "%s: table: texel %zu channel %zu is %g (values are finite, at most FLT_MAX / 2 in magnitude)", who, i / 3, i % 3,
                            (double)l->table[i]);
    }
    return FF_OK;
}

// The parameter block and the image: everything but the LUT.
int check_grade(const FfGradeParams* p, int width, int height, const float* radiance_in, const void* rgb8, const float* radiance_out, const char* who)
{
    if (!p) return fail(FF_ERR_INVALID_ARG, "%s: params are null", who);
    if (check_image_size(width, height, who) != FF_OK) return FF_ERR_INVALID_ARG;
    if (p->flags & ~kGradeFlags) return fail(FF_ERR_INVALID_ARG, "%s: unknown flags 0x%x", who, p->flags);
    if (p->reserved != 0) return fail(FF_ERR_INVALID_ARG, "%s: reserved must be 0", who);
    for (int i = 0; i < 9; ++i)
        if (!finite_f(p->matrix[i])) return fail(FF_ERR_INVALID_ARG, "%s: matrix[%d] is not finite", who, i);
    for (int i = 0; i < 3; ++i)
        if (!finite_f(p->offset[i])) return fail(FF_ERR_INVALID_ARG, "%s: offset[%d] is not finite", who, i);
    if (!finite_f(p->saturation) || p->saturation < 0.f) return fail(FF_ERR_INVALID_ARG, "%s: saturation %g must be finite and >= 0", who, (double)p->saturation);
    if (!radiance_in) return fail(FF_ERR_INVALID_ARG, "%s: radiance_in is null", who);
    const size_t px = (size_t)width * (size_t)height;
    const Span in = { radiance_in, px * 12, "radiance_in" };
    // (in place: a pixel is read before it is written, and no pixel reads another)
    if (radiance_out == radiance_in) {
        if (rgb8 && overlaps({ rgb8, px * 3, "rgb8" }, in)) return fail(FF_ERR_INVALID_ARG, "%s: rgb8 overlaps radiance_in", who);
        return FF_OK;
    }
    return check_outputs_disjoint(rgb8, radiance_out, px, { in }, who);
}

// The halves the stage flags need, of a LUT that is there or not (desc null).
int check_halves(uint32_t flags, const FfGradeLut* desc, int lut_id, const char* who)
{
    if (!(flags & (FF_GRADE_CURVES | FF_GRADE_LUT3D))) return FF_OK;
    if (!desc) return lut_id >= -1 ? fail(FF_ERR_INVALID_ARG, "%s: FF_GRADE_CURVES / FF_GRADE_LUT3D need a lut (lut_id %d names none)", who, lut_id)
                                   : fail(FF_ERR_INVALID_ARG, "%s: FF_GRADE_CURVES / FF_GRADE_LUT3D need a lut (lut is null)", who);
    if ((flags & FF_GRADE_CURVES) && desc->curve_size == 0) return fail(FF_ERR_INVALID_ARG, "%s: FF_GRADE_CURVES: the lut has no curves", who);
    if ((flags & FF_GRADE_LUT3D) && desc->size == 0) return fail(FF_ERR_INVALID_ARG, "%s: FF_GRADE_LUT3D: the lut has no lattice (table)", who);
    return FF_OK;
}

// The kernel arguments of a call: the parameters and the descriptor's numbers (desc may be null when no stage needs it).
GradeArgs grade_args(const FfGradeParams* p, const FfGradeLut* desc)
{
    GradeArgs a;
    std::memset(&a, 0, sizeof a);
    a.flags = p->flags;
    for (int i = 0; i < 9; ++i) a.m[i] = p->matrix[i];
    for (int i = 0; i < 3; ++i) a.o[i] = p->offset[i];
    a.saturation = p->saturation;
    if (desc && desc->curve_size) {
        a.curve_size = desc->curve_size;
        a.curve_axis = desc->curve_axis;
        a.curve_shift = desc->curve_shift;
        a.curve_lo = desc->curve_lo;
        a.curve_hi = desc->curve_hi;
        a.curve_range = desc->curve_hi - desc->curve_lo;
        a.curve_scale = (float)(desc->curve_size - 1);
        a.curve_lo_bits = grade_bits(desc->curve_lo);
        a.curve_unit = (float)(1u << desc->curve_shift);
    }
    if (desc && desc->size) {
        a.size = desc->size;
        for (int c = 0; c < 3; ++c) {
            a.dmin[c] = desc->domain_min[c];
            a.dmax[c] = desc->domain_max[c];
            a.drange[c] = desc->domain_max[c] - desc->domain_min[c];
        }
        a.size_scale = (float)(desc->size - 1);
    }
    return a;
}

struct HostFetch {
    const float* table;
    FF_PIXEL_HD void operator()(int index, float* out) const
    {
        out[0] = table[3 * (size_t)index];
        out[1] = table[3 * (size_t)index + 1];
        out[2] = table[3 * (size_t)index + 2];
    }
};

template <bool PRIMARY, bool CURVES, int LUT>
void grade_host(const GradeArgs& a, const float* curves, const float* table, size_t px, const float* in, unsigned char* rgb8, float* out)
{
    const HostFetch fetch = { table };
    for (size_t i = 0; i < px; ++i) {
        float v[3];
        grade_pixel<PRIMARY, CURVES, LUT>(a, curves, fetch, in + 3 * i, v); // (reads the pixel before store_rgb writes it: in place is fine)
        store_rgb(i, v, rgb8, out);
    }
}

template <bool PRIMARY, bool CURVES>
void grade_host_lut(int lut, const GradeArgs& a, const float* curves, const float* table, size_t px, const float* in, unsigned char* rgb8, float* out)
{
    if (lut == 0) grade_host<PRIMARY, CURVES, 0>(a, curves, table, px, in, rgb8, out);
    else if (lut == 1) grade_host<PRIMARY, CURVES, 1>(a, curves, table, px, in, rgb8, out);
    else grade_host<PRIMARY, CURVES, 2>(a, curves, table, px, in, rgb8, out);
}

// ---- .cube ------------------------------------------------------------------------------------------------------------------

// Three floats and nothing else on a line: false if malformed; *finite false if one of them is not finite.
bool parse_three(const char* s, float* out, bool* finite)
{
    *finite = true;
    for (int i = 0; i < 3; ++i) {
        char* end = nullptr;
        errno = 0;
        out[i] = std::strtof(s, &end);
        if (end == s) return false;
        if (!std::isfinite(out[i])) *finite = false;
        s = end;
    }
    while (*s == ' ' || *s == '\t') ++s;
    return *s == '\0';
}

bool parse_size(const char* s, long* out)
{
    char* end = nullptr;
    *out = std::strtol(s, &end, 10);
    if (end == s) return false;
    while (*end == ' ' || *end == '\t') ++end;
    return *end == '\0';
}

void free_cube(FfCubeFile* f)
{
    std::free(const_cast<float*>(f->lut.curves));
    std::free(const_cast<float*>(f->lut.table));
    std::memset(f, 0, sizeof *f);
}

} // namespace

namespace ff {

void grade_release(FfState* s)
{
    for (FfState::GradeLut& l : s->grade_luts) {
        if (l.d_table) (void)hipFree(l.d_table);
        if (l.d_curves) (void)hipFree(l.d_curves);
    }
    s->grade_luts.clear();
}

} // namespace ff

extern "C" {

void ff_grade_params_init(FfGradeParams* p)
{
    if (!p) return;
    std::memset(p, 0, sizeof *p);
    p->matrix[0] = p->matrix[4] = p->matrix[8] = 1.f;
    p->saturation = 1.f;
    p->lut_id = -1;
}

int ff_grade_lut_create(FfState* s, const FfGradeLut* lut, int* out_id)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_grade_lut_create: state is null");
    if (!out_id) return fail(FF_ERR_INVALID_ARG, "ff_grade_lut_create: out_id is null");
    *out_id = -1;
    const int st = check_lut(lut, "ff_grade_lut_create");
    if (st != FF_OK) return st;
    size_t id = 0;
    while (id < s->grade_luts.size() && (s->grade_luts[id].d_table || s->grade_luts[id].d_curves)) ++id;
    if (id >= (size_t)kGradeMaxLuts) return fail(FF_ERR_INVALID_ARG, "ff_grade_lut_create: the state already holds %d luts", kGradeMaxLuts);
    FF_HIP(hipSetDevice(s->device));
    FfState::GradeLut made;
    made.desc = *lut;
    made.desc.curves = made.desc.table = nullptr;
    hipError_t e = hipSuccess;
    if (lut->curve_size) {
        const size_t bytes = (size_t)lut->curve_size * 12;
        e = hipMalloc((void**)&made.d_curves, bytes);
        if (e == hipSuccess) e = hipMemcpy(made.d_curves, lut->curves, bytes, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && lut->size) {
        const size_t n = (size_t)lut->size * lut->size * lut->size;
        std::vector<float4> texels(n);
        for (size_t k = 0; k < n; ++k) texels[k] = make_float4(lut->table[3 * k], lut->table[3 * k + 1], lut->table[3 * k + 2], 0.f);
        e = hipMalloc((void**)&made.d_table, n * sizeof(float4));
        if (e == hipSuccess) e = hipMemcpy(made.d_table, texels.data(), n * sizeof(float4), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        if (made.d_curves) (void)hipFree(made.d_curves);
        if (made.d_table) (void)hipFree(made.d_table);
        return fail(e == hipErrorOutOfMemory ? FF_ERR_OOM : FF_ERR_HIP, "ff_grade_lut_create: allocating or copying the lut failed: %s", hipGetErrorString(e));
    }
    if (id == s->grade_luts.size()) s->grade_luts.emplace_back();
    s->grade_luts[id] = made;
    *out_id = (int)id;
    return FF_OK;
}

int ff_grade_lut_destroy(FfState* s, int id)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_grade_lut_destroy: state is null");
    if (id < 0 || (size_t)id >= s->grade_luts.size() || !(s->grade_luts[(size_t)id].d_table || s->grade_luts[(size_t)id].d_curves))
        return fail(FF_ERR_INVALID_ARG, "ff_grade_lut_destroy: no lut %d", id);
    FF_HIP(hipSetDevice(s->device));
    FF_HIP(hipStreamSynchronize(s->stream));
    FfState::GradeLut& l = s->grade_luts[(size_t)id];
    if (l.d_table) (void)hipFree(l.d_table);
    if (l.d_curves) (void)hipFree(l.d_curves);
    l = FfState::GradeLut();
    return FF_OK;
}

int ff_color_grade(FfState* s, const FfGradeParams* p, int width, int height, const float* radiance_in, int input_on_device, void* rgb8, int rgb8_on_device,
                   float* radiance_out, int radiance_out_on_device)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_color_grade: state is null");
    int st = check_grade(p, width, height, radiance_in, rgb8, radiance_out, "ff_color_grade");
    if (st != FF_OK) return st;
    const FfState::GradeLut* lut = nullptr;
    if (p->lut_id >= 0 && (size_t)p->lut_id < s->grade_luts.size() && (s->grade_luts[(size_t)p->lut_id].d_table || s->grade_luts[(size_t)p->lut_id].d_curves))
        lut = &s->grade_luts[(size_t)p->lut_id];
    if (p->lut_id != -1 && !lut) return fail(FF_ERR_INVALID_ARG, "ff_color_grade: lut_id %d names no lut", p->lut_id);
    st = check_halves(p->flags, lut ? &lut->desc : nullptr, p->lut_id, "ff_color_grade");
    if (st != FF_OK) return st;
    FF_HIP(hipSetDevice(s->device));
    hipStream_t stream = s->stream;
    GradeArgs a = grade_args(p, lut ? &lut->desc : nullptr);
    const bool curves = (p->flags & FF_GRADE_CURVES) != 0, lattice = (p->flags & FF_GRADE_LUT3D) != 0;
    if (lut) {
        a.curves = lut->d_curves;
        a.table = lut->d_table;
    }
    // where the lattice lives: in LDS up to kGradeLdsMaxSize, with the curves beside it while they fit
    a.home = kGradeHomeGlobal;
    if (lattice && a.size <= kGradeLdsMaxSize && !s->sw.grade_no_lds)
        a.home = grade_lds_bytes(kGradeHomeLds, curves, a.curve_size, true, a.size) <= kGradeLdsBytes ? kGradeHomeLds : kGradeHomeLdsCurvesOut;
    const size_t px = (size_t)width * (size_t)height;
    const bool in_place = radiance_out == radiance_in;
    Staging stage(&s->d_img_work, &s->img_work_bytes);
    const float* d_in = radiance_in;
    if (!input_on_device) stage.in(&d_in, radiance_in, px * 12);
    // (in place on the host: the result is written over the staged input and copied back from there)
    StagedOutputs out(stage, px, rgb8, rgb8_on_device, in_place && !input_on_device ? nullptr : radiance_out, radiance_out_on_device);
    const int staged = stage.commit(stream, "ff_color_grade: staging the input failed");
    if (staged != FF_OK) return staged;
    float* d_out = out.radiance;
    if (in_place && !input_on_device) d_out = const_cast<float*>(d_in);
    a.vec_in = ((uintptr_t)d_in & 15) == 0;
    a.vec_out = ((uintptr_t)d_out & 15) == 0;
    a.vec_rgb8 = ((uintptr_t)out.rgb8 & 3) == 0;
    FF_HIP(launch_color_grade(a, px, d_in, out.rgb8, d_out, stream));
    if (in_place && !input_on_device) FF_HIP(hipMemcpyAsync(radiance_out, d_out, px * 12, hipMemcpyDeviceToHost, stream));
    FF_HIP(hipStreamSynchronize(stream));
    return stage.finish();
}

int ff_color_grade_host(const FfGradeParams* p, const FfGradeLut* lut, int width, int height, const float* radiance_in, unsigned char* rgb8, float* radiance_out)
{
    clear_error();
    int st = check_grade(p, width, height, radiance_in, rgb8, radiance_out, "ff_color_grade_host");
    if (st != FF_OK) return st;
    if (lut && (st = check_lut(lut, "ff_color_grade_host")) != FF_OK) return st;
    st = check_halves(p->flags, lut, -2, "ff_color_grade_host");
    if (st != FF_OK) return st;
    const GradeArgs a = grade_args(p, lut);
    const size_t px = (size_t)width * (size_t)height;
    const int l3 = !(p->flags & FF_GRADE_LUT3D) ? 0 : ((p->flags & FF_GRADE_TRILINEAR) ? 2 : 1);
    const float* curves = lut ? lut->curves : nullptr;
    const float* table = lut ? lut->table : nullptr;
    const bool primary = (p->flags & FF_GRADE_PRIMARY) != 0, cv = (p->flags & FF_GRADE_CURVES) != 0;
    if (primary && cv) grade_host_lut<true, true>(l3, a, curves, table, px, radiance_in, rgb8, radiance_out);
    else if (primary) grade_host_lut<true, false>(l3, a, curves, table, px, radiance_in, rgb8, radiance_out);
    else if (cv) grade_host_lut<false, true>(l3, a, curves, table, px, radiance_in, rgb8, radiance_out);
    else grade_host_lut<false, false>(l3, a, curves, table, px, radiance_in, rgb8, radiance_out);
    return FF_OK;
}

int ff_load_cube(const char* path, FfCubeFile* out)
{
    clear_error();
    if (!path || !out) return fail(FF_ERR_INVALID_ARG, "ff_load_cube: null argument");
    std::memset(out, 0, sizeof *out);
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return fail(FF_ERR_IO, "ff_load_cube: cannot open '%s': %s", path, std::strerror(errno));
    struct Closer {
        std::FILE* f;
        ~Closer() { std::fclose(f); }
    } closer = { f };
    float dmin[3] = { 0.f, 0.f, 0.f }, dmax[3] = { 1.f, 1.f, 1.f };
    long size1 = 0, size3 = 0;
    size_t rows = 0, got = 0;
    std::vector<float> data;
    std::string line;
    int line_no = 0;
    bool more = true;
    while (more) {
        line.clear();
        int c;
        while ((c = std::fgetc(f)) != EOF && c != '\n') line.push_back((char)c);
        more = c != EOF;
        if (!more && line.empty()) break;
        ++line_no;
        while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
        if (line.find('\0') != std::string::npos) return fail(FF_ERR_INVALID_ARG, "ff_load_cube: %s: line %d holds a NUL byte", path, line_no);
        const char* s = line.c_str();
        while (*s == ' ' || *s == '\t') ++s;
        if (*s == '\0' || *s == '#') continue;
        const bool keyword = (*s >= 'A' && *s <= 'Z') || (*s >= 'a' && *s <= 'z' && *s != 'n' && *s != 'i'); // (nan and inf are values, refused as such)
        if (keyword) {
            size_t n = 0;
            while (s[n] && s[n] != ' ' && s[n] != '\t') ++n;
            const std::string key(s, n);
            const char* rest = s + n;
            while (*rest == ' ' || *rest == '\t') ++rest;
            bool finite = true;
            if (key == "TITLE") {
                const size_t len = std::strlen(rest);
                if (len < 2 || rest[0] != '"' || rest[len - 1] != '"' || std::memchr(rest + 1, '"', len - 2))
                    return fail(FF_ERR_INVALID_ARG, "ff_load_cube: %s: line %d: TITLE wants one \"quoted\" text", path, line_no);
                if (len - 2 >= sizeof out->title) return fail(FF_ERR_INVALID_ARG, "ff_load_cube: %s: line %d: TITLE is longer than %zu bytes", path, line_no, sizeof out->title - 1);
                std::memcpy(out->title, rest + 1, len - 2);
                out->title[len - 2] = '\0';
            } else if (key == "DOMAIN_MIN" || key == "DOMAIN_MAX") {
                float* d = key == "DOMAIN_MIN" ? dmin : dmax;
                if (!parse_three(rest, d, &finite)) return fail(FF_ERR_INVALID_ARG, "ff_load_cube: %s: line %d: %s wants three numbers", path, line_no, key.c_str());
                if (!finite) return fail(FF_ERR_INVALID_ARG, "ff_load_cube: %s: line %d: %s holds a value that is not finite", path, line_no, key.c_str());
            } else if (key == "LUT_1D_SIZE" || key == "LUT_3D_SIZE") {
                if (size1 || size3) return fail(FF_ERR_INVALID_ARG, "ff_load_cube: %s: line %d: a second size (a file holds LUT_1D_SIZE or LUT_3D_SIZE, once)", path, line_no);
                long v = 0;
                if (!parse_size(rest, &v)) return fail(FF_ERR_INVALID_ARG, "ff_load_cube: %s: line %d: %s wants one integer", path, line_no, key.c_str());
                const bool is1 = key == "LUT_1D_SIZE";
                const long most = is1 ? kGradeMaxCurve : kGradeMaxSize;
                if (v < 2 || v > most) return fail(FF_ERR_INVALID_ARG, "ff_load_cube: %s: line %d: %s %ld is outside 2 .. %ld", path, line_no, key.c_str(), v, most);
                (is1 ? size1 : size3) = v;
                rows = is1 ? (size_t)v : (size_t)v * v * v;
                data.resize(rows * 3);
            } else {
                return fail(FF_ERR_INVALID_ARG, "ff_load_cube: %s: line %d: unknown keyword '%s'", path, line_no, key.c_str());
            }
            if (got > 0 && key != "TITLE") return fail(FF_ERR_INVALID_ARG, "ff_load_cube: %s: line %d: %s after the first data line", path, line_no, key.c_str());
            continue;
        }
        if (!rows) return fail(FF_ERR_INVALID_ARG, "ff_load_cube: %s: line %d: a data line before LUT_1D_SIZE or LUT_3D_SIZE", path, line_no);
        if (got == rows) return fail(FF_ERR_INVALID_ARG, "ff_load_cube: %s: line %d: more than the %zu data lines its size says", path, line_no, rows);
        bool finite = true;
        if (!parse_three(s, data.data() + 3 * got, &finite)) return fail(FF_ERR_INVALID_ARG, "ff_load_cube: %s: line %d: a data line wants three numbers", path, line_no);
        if (!finite) return fail(FF_ERR_INVALID_ARG, "ff_load_cube: %s: line %d: a value that is not finite", path, line_no);
        ++got;
    }
    if (!rows) return fail(FF_ERR_INVALID_ARG, "ff_load_cube: %s: neither LUT_1D_SIZE nor LUT_3D_SIZE", path);
    if (got < rows) return fail(FF_ERR_IO, "ff_load_cube: %s: the file ends after %zu of %zu data lines", path, got, rows);
    for (int c = 0; c < 3; ++c)
        if (!(dmin[c] < dmax[c])) return fail(FF_ERR_INVALID_ARG, "ff_load_cube: %s: DOMAIN_MIN %g is not below DOMAIN_MAX %g", path, (double)dmin[c], (double)dmax[c]);
    float* values = static_cast<float*>(std::malloc(data.size() * sizeof(float)));
    if (!values) return fail(FF_ERR_OOM, "ff_load_cube: %s: out of host memory", path);
    FfGradeLut& l = out->lut;
    if (size1) {
        if (dmin[0] != dmin[1] || dmin[0] != dmin[2] || dmax[0] != dmax[1] || dmax[0] != dmax[2]) {
            std::free(values);
            return fail(FF_ERR_INVALID_ARG, "ff_load_cube: %s: a 1D file's DOMAIN_MIN and DOMAIN_MAX must be the same for r, g and b", path);
        }
        for (size_t k = 0; k < rows; ++k)
            for (int c = 0; c < 3; ++c) values[(size_t)c * rows + k] = data[3 * k + c];
        l.curve_size = (int32_t)size1;
        l.curve_axis = FF_GRADE_AXIS_LINEAR;
        l.curve_lo = dmin[0];
        l.curve_hi = dmax[0];
        l.curves = values;
    } else {
        std::memcpy(values, data.data(), data.size() * sizeof(float));
        l.size = (int32_t)size3;
        l.table = values;
        // (the default domain a file without the keywords has; a 1D file's goes into curve_lo .. curve_hi)
        for (int c = 0; c < 3; ++c) {
            l.domain_min[c] = dmin[c];
            l.domain_max[c] = dmax[c];
        }
    }
    const int st = check_lut(&l, "ff_load_cube"); // (what ff_grade_lut_create would refuse: a value beyond FLT_MAX / 2, a domain whose difference overflows)
    if (st != FF_OK) free_cube(out);
    return st;
}

void ff_free_cube(FfCubeFile* file)
{
    if (file) free_cube(file);
}

int ff_save_cube(const char* path, const FfCubeFile* file)
{
    clear_error();
    if (!path || !file) return fail(FF_ERR_INVALID_ARG, "ff_save_cube: null argument");
    const FfGradeLut& l = file->lut;
    const int st = check_lut(&l, "ff_save_cube");
    if (st != FF_OK) return st;
    if (l.curve_size && l.size) return fail(FF_ERR_INVALID_ARG, "ff_save_cube: a file holds the curves or the lattice, not both");
    if (l.curve_size && l.curve_axis != FF_GRADE_AXIS_LINEAR) return fail(FF_ERR_INVALID_ARG, "ff_save_cube: a 1D file holds curves on FF_GRADE_AXIS_LINEAR (curve_axis is %d)", l.curve_axis);
    const size_t tl = strnlen(file->title, sizeof file->title);
    if (tl == sizeof file->title) return fail(FF_ERR_INVALID_ARG, "ff_save_cube: title is not NUL-terminated");
    for (size_t i = 0; i < tl; ++i)
        if (file->title[i] == '"' || file->title[i] == '\n' || file->title[i] == '\r') return fail(FF_ERR_INVALID_ARG, "ff_save_cube: title may not hold '\"' or a line end");
    std::FILE* f = std::fopen(path, "wb");
    if (!f) return fail(FF_ERR_IO, "ff_save_cube: cannot open '%s' for writing: %s", path, std::strerror(errno));
    bool ok = true;
    if (tl) ok = std::fprintf(f, "TITLE \"%s\"\n", file->title) > 0 && ok;
    if (l.curve_size) {
        ok = std::fprintf(f, "LUT_1D_SIZE %d\nDOMAIN_MIN %.9g %.9g %.9g\nDOMAIN_MAX %.9g %.9g %.9g\n", l.curve_size, (double)l.curve_lo, (double)l.curve_lo,
                          (double)l.curve_lo, (double)l.curve_hi, (double)l.curve_hi, (double)l.curve_hi) > 0 && ok;
        const size_t K = (size_t)l.curve_size;
        for (size_t k = 0; k < K && ok; ++k) ok = std::fprintf(f, "%.9g %.9g %.9g\n", (double)l.curves[k], (double)l.curves[K + k], (double)l.curves[2 * K + k]) > 0;
    } else {
        ok = std::fprintf(f, "LUT_3D_SIZE %d\nDOMAIN_MIN %.9g %.9g %.9g\nDOMAIN_MAX %.9g %.9g %.9g\n", l.size, (double)l.domain_min[0], (double)l.domain_min[1],
                          (double)l.domain_min[2], (double)l.domain_max[0], (double)l.domain_max[1], (double)l.domain_max[2]) > 0 && ok;
        const size_t n = (size_t)l.size * l.size * l.size;
        for (size_t k = 0; k < n && ok; ++k) ok = std::fprintf(f, "%.9g %.9g %.9g\n", (double)l.table[3 * k], (double)l.table[3 * k + 1], (double)l.table[3 * k + 2]) > 0;
    }
    ok = std::fclose(f) == 0 && ok;
    if (!ok) return fail(FF_ERR_IO, "ff_save_cube: writing '%s' failed", path);
    return FF_OK;
}

} // extern "C"
