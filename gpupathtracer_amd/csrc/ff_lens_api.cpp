// ff_lens_api.cpp — host side of ff_lens (include/firefly/ff_api.h): the argument checks, the radial model in double and the two
// tables it is folded into (cached on the device under their key), the staging of host buffers in the state's image work buffer
// (ff_image.h's helpers), the one launch (kernel in ff_lens.hip), the loops of the host-only twin ff_lens_host and of
// ff_lens_map_host over ff_lens.h's per-pixel functions, and ff_lens_fit_zoom.  A pure image operation: no scene, no G-buffer, no
// history.
#include <cmath>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "ff_lens.h"
#include "ff_state.h"

using namespace ff;

namespace {

// ---- the model, in double ----------------------------------------------------------------------------------------------------------

struct Poly {
    double k1, k2, k3;
};

// f(s) = s d(s^2): the lens's radius for the ideal radius s, and f'(s) as a cubic g in t = s^2.
double lens_f(const Poly& k, double s)
{
    const double t = s * s;
    return s * (1.0 + k.k1 * t + k.k2 * t * t + k.k3 * t * t * t);
}
double lens_g(const Poly& k, double t) { return 1.0 + 3.0 * k.k1 * t + 5.0 * k.k2 * t * t + 7.0 * k.k3 * t * t * t; }

// The smallest t in (0, limit] with g(t) <= 0, the square of the radius at which the image folds over; negative if there is none.
// g(0) = 1, and between two neighbours of {0, the roots of g', limit} g is monotone: the first piece that ends at or below 0 holds
// the first root, found by bisection.
double first_fold(const Poly& k, double limit)
{
    double cuts[4];
    int n = 0;
    const double a = 21.0 * k.k3, b = 10.0 * k.k2, c = 3.0 * k.k1; // g'(t) = a t^2 + b t + c
    if (a != 0.0) {
        const double disc = b * b - 4.0 * a * c;
        if (disc > 0.0) {
            const double q = -0.5 * (b + (b < 0.0 ? -std::sqrt(disc) : std::sqrt(disc)));
            const double t0 = q / a, t1 = q != 0.0 ? c / q : 0.0;
            cuts[n++] = t0 < t1 ? t0 : t1;
            cuts[n++] = t0 < t1 ? t1 : t0;
        }
    } else if (b != 0.0) {
        cuts[n++] = -c / b;
    }
    cuts[n++] = limit;
    double lo = 0.0;
    for (int i = 0; i < n; ++i) {
        const double hi = cuts[i] < limit ? cuts[i] : limit;
        if (!(hi > lo)) continue;
        if (lens_g(k, hi) <= 0.0) {
            double x0 = lo, x1 = hi;
            for (int it = 0; it < 200 && x0 < x1; ++it) {
                const double m = 0.5 * (x0 + x1);
                if (m <= x0 || m >= x1) break;
                if (lens_g(k, m) <= 0.0) x1 = m; else x0 = m;
            }
            return x1;
        }
        lo = hi;
    }
    return -1.0;
}

// The inverse of f at rho >= 0 on the rising branch [0, s_hi] (f(s_hi) >= rho): Newton from rho, kept inside a bracket that
// bisection shrinks.  f(rho) == rho (no distortion) returns rho itself.
double lens_f_inverse(const Poly& k, double rho, double s_hi)
{
    if (rho <= 0.0) return 0.0;
    double lo = 0.0, hi = s_hi, s = rho < s_hi ? rho : s_hi;
    for (int it = 0; it < 200; ++it) {
        const double r = lens_f(k, s) - rho;
        if (r == 0.0) return s;
        if (r > 0.0) hi = s; else lo = s;
        const double slope = lens_g(k, s * s);
        double next = slope > 0.0 ? s - r / slope : 0.5 * (lo + hi);
        if (!(next > lo && next < hi)) next = 0.5 * (lo + hi);
        if (next == s || !(hi > lo) || next <= lo || next >= hi) break;
        s = next;
    }
    return s;
}

// What the parameters and the size come to, once: the centre, the normalisation, the range of the tables and the rising branch.
struct LensModel {
    Poly k;
    int direction;
    double zoom, vignette, falloff;
    float cx, cy;      // as the kernel gets them
    double d2;         // (half the diagonal)^2
    double r2_max;     // the largest r^2 of a pixel centre (at least 2^-20)
    double s_hi;       // FF_LENS_DISTORT: the end of the bracket of f's inverse
    double fold;       // the radius at which f stops rising (negative: it never does)
};

// m(rho): the source radius of the unzoomed output radius rho.
double lens_m(const LensModel& m, double rho) { return m.direction == FF_LENS_UNDISTORT ? lens_f(m.k, rho) : lens_f_inverse(m.k, rho, m.s_hi); }

// The model for these parameters at this size with this zoom, or FF_ERR_INVALID_ARG when r d(r^2) does not rise strictly on the
// range the image needs (who: the prefix of the error's text).
int lens_model(const FfLensParams* p, int width, int height, double zoom, LensModel* m, const char* who)
{
    m->k = { (double)p->k1, (double)p->k2, (double)p->k3 };
    m->direction = p->direction;
    m->zoom = zoom;
    m->vignette = (double)p->vignette;
    m->falloff = (double)p->vignette_falloff;
    m->cx = 0.5f * (float)width + p->center_x;
    m->cy = 0.5f * (float)height + p->center_y;
    m->d2 = 0.25 * ((double)width * (double)width + (double)height * (double)height);
    double r2 = 0.0;
    for (int corner = 0; corner < 4; ++corner) {
        const double dx = ((corner & 1) ? (double)width - 0.5 : 0.5) - (double)m->cx;
        const double dy = ((corner & 2) ? (double)height - 0.5 : 0.5) - (double)m->cy;
        const double v = (dx * dx + dy * dy) / m->d2;
        r2 = v > r2 ? v : r2;
    }
    m->r2_max = r2 > 9.5367431640625e-07 ? r2 : 9.5367431640625e-07; // 2^-20: a 1 x 1 image on its own centre has r2 = 0
    const double rho_max = std::sqrt(m->r2_max) / zoom;
    m->s_hi = rho_max;
    if (p->direction == FF_LENS_UNDISTORT) {
        const double t = first_fold(m->k, rho_max * rho_max);
        m->fold = t < 0.0 ? -1.0 : std::sqrt(t);
        if (t >= 0.0)
            return fail(FF_ERR_INVALID_ARG, "%s: k1, k2, k3 fold the image over at radius %g (r d(r^2) must rise strictly up to radius %g)", who, std::sqrt(t),
                        rho_max);
    } else {
        const double t = first_fold(m->k, 1.0e6);
        m->fold = t < 0.0 ? -1.0 : std::sqrt(t);
        if (t >= 0.0) {
            const double s = std::sqrt(t);
            if (!(lens_f(m->k, s) > rho_max))
                return fail(FF_ERR_INVALID_ARG, "%s: k1, k2, k3 fold the image over at radius %g, where r d(r^2) = %g (it must rise strictly up to %g)", who,
                            s, lens_f(m->k, s), rho_max);
            m->s_hi = s;
        } else {
            double s = rho_max > 0.0 ? rho_max : 1.0;
            for (int it = 0; it < 64 && lens_f(m->k, s) < rho_max; ++it) s = 2.0 * s;
            m->s_hi = s;
        }
    }
    return FF_OK;
}

// The tables: e(r^2) = m(r / zoom) / r - 1 and the gain at FF_LENS_KNOTS + 1 equally spaced knots of r^2 over [0, r2_max].
void lens_fill_tables(const LensModel& m, LensKnot* table)
{
    for (int j = 0; j <= kLensKnots; ++j) {
        const double r2 = m.r2_max * (double)j / (double)kLensKnots;
        const double r = std::sqrt(r2);
        const double rho = r / m.zoom;
        const double src = lens_m(m, rho);                             // the source radius
        const double e = j == 0 ? 1.0 / m.zoom - 1.0 : src / r - 1.0;
        const double lens_r = m.direction == FF_LENS_DISTORT ? rho : src; // the radius in the lens's image
        const double fr = m.falloff * lens_r;
        const double c = 1.0 + fr * fr;
        const double v = 1.0 / (c * c);
        const double gain = (1.0 - m.vignette) + m.vignette * v;
        table[j].e = (float)e;
        table[j].gain = (float)(m.direction == FF_LENS_DISTORT ? gain : 1.0 / gain);
    }
}

// ---- checks ------------------------------------------------------------------------------------------------------------------------

bool in_range(float v, float lo, float hi) { return v >= lo && v <= hi; } // (false for NaN)

// The parameter block against the size: every field finite and in range, the enumerations, reserved, the flags.
int check_lens_params(const FfLensParams* p, int width, int height, const char* who)
{
    if (!p) return fail(FF_ERR_INVALID_ARG, "%s: params are null", who);
    if (check_image_size(width, height, who) != FF_OK) return FF_ERR_INVALID_ARG;
    const struct {
        const char* name;
        float v, lo, hi;
    } fields[] = { { "k1", p->k1, -10.f, 10.f }, { "k2", p->k2, -10.f, 10.f }, { "k3", p->k3, -10.f, 10.f },
                   { "center_x", p->center_x, -0.5f * (float)width, 0.5f * (float)width }, { "center_y", p->center_y, -0.5f * (float)height, 0.5f * (float)height },
                   { "zoom", p->zoom, 0.0625f, 16.f }, { "ca_red", p->ca_red, -0.25f, 0.25f }, { "ca_blue", p->ca_blue, -0.25f, 0.25f },
                   { "vignette", p->vignette, 0.f, 1.f }, { "vignette_falloff", p->vignette_falloff, 0.f, 8.f } };
    for (const auto& f : fields)
        if (!in_range(f.v, f.lo, f.hi)) return fail(FF_ERR_INVALID_ARG, "%s: %s must be %g .. %g and finite (got %g)", who, f.name, (double)f.lo, (double)f.hi, (double)f.v);
    if (p->direction != FF_LENS_UNDISTORT && p->direction != FF_LENS_DISTORT) return fail(FF_ERR_INVALID_ARG, "%s: unknown direction %d", who, p->direction);
    if (p->filter != FF_LENS_BILINEAR && p->filter != FF_LENS_CATMULL_ROM) return fail(FF_ERR_INVALID_ARG, "%s: unknown filter %d", who, p->filter);
    if (p->border != FF_LENS_BORDER_BLACK && p->border != FF_LENS_BORDER_CLAMP) return fail(FF_ERR_INVALID_ARG, "%s: unknown border %d", who, p->border);
    if (p->reserved != 0) return fail(FF_ERR_INVALID_ARG, "%s: reserved must be 0", who);
    if (p->flags & ~(uint32_t)FF_LENS_ANTI_RING) return fail(FF_ERR_INVALID_ARG, "%s: unknown flags 0x%x", who, p->flags);
    return FF_OK;
}

// The kernel arguments of a model.
void lens_args(const FfLensParams* p, int width, int height, const LensModel& m, LensArgs* a)
{
    a->width = width;
    a->height = height;
    a->cx = m.cx;
    a->cy = m.cy;
    a->inv_d2 = (float)(1.0 / m.d2);
    a->knot_scale = (float)((double)kLensKnots / m.r2_max);
    a->q_red = p->ca_red;
    a->q_blue = p->ca_blue;
    a->filter = p->filter == FF_LENS_BILINEAR ? kLensBilinear : ((p->flags & FF_LENS_ANTI_RING) ? kLensCatmullRomClamped : kLensCatmullRom);
    a->per_channel = (p->ca_red != 0.f || p->ca_blue != 0.f) ? 1 : 0;
    a->border = p->border;
}

// What both image entry points check, in this order: the parameter block, the size, the parameters (the fold-over last of them),
// the input, the outputs' places.  Fills the model and the kernel arguments.
int check_lens(int width, int height, const FfLensParams* p, const float* radiance_in, const void* rgb8, const float* radiance_out, LensModel* m,
               LensArgs* a, const char* who)
{
    if (check_lens_params(p, width, height, who) != FF_OK) return FF_ERR_INVALID_ARG;
    if (lens_model(p, width, height, (double)p->zoom, m, who) != FF_OK) return FF_ERR_INVALID_ARG;
    if (!radiance_in) return fail(FF_ERR_INVALID_ARG, "%s: radiance_in is null", who);
    const size_t px = (size_t)width * (size_t)height;
    if (check_outputs_disjoint(rgb8, radiance_out, px, { { radiance_in, px * 12, "radiance_in" } }, who) != FF_OK) return FF_ERR_INVALID_ARG;
    lens_args(p, width, height, *m, a);
    return FF_OK;
}

// What the device table is built from: the parameters that feed it, and the size.
FfState::LensTable::Key table_key(const FfLensParams* p, int width, int height)
{
    FfState::LensTable::Key k;
    const float f[8] = { p->k1, p->k2, p->k3, p->center_x, p->center_y, p->zoom, p->vignette, p->vignette_falloff };
    std::memcpy(k.f, f, sizeof f);
    k.direction = p->direction;
    k.width = width;
    k.height = height;
    return k;
}

// The state's device table for this call: rebuilt and uploaded only when its key changes.
int device_table(FfState* s, const FfLensParams* p, int width, int height, const LensModel& m, hipStream_t stream, const LensKnot** out)
{
    FfState::LensTable& t = s->lens_table;
    const FfState::LensTable::Key key = table_key(p, width, height);
    if (!(t.valid && std::memcmp(&t.key, &key, sizeof key) == 0)) {
        t.valid = false;
        std::vector<LensKnot> table(kLensKnots + 1);
        lens_fill_tables(m, table.data());
        const int st = ensure_bytes(&t.d_table, &t.bytes, table.size() * sizeof(LensKnot));
        if (st != FF_OK) return st;
        FF_HIP(hipMemcpyAsync(t.d_table, table.data(), table.size() * sizeof(LensKnot), hipMemcpyHostToDevice, stream));
        FF_HIP(hipStreamSynchronize(stream)); // (the host vector ends here, and a failed copy must not leave the key set)
        t.key = key;
        t.valid = true;
        ++t.builds;
    }
    *out = (const LensKnot*)t.d_table;
    return FF_OK;
}

template <int FILTER, bool PER_CHANNEL>
void lens_rows(const LensArgs& a, const LensKnot* table, const float* radiance_in, unsigned char* rgb8, float* radiance_out)
{
    for (int y = 0; y < a.height; ++y)
        for (int x = 0; x < a.width; ++x) {
            float v[3];
            lens_pixel<FILTER, PER_CHANNEL>(a, table, radiance_in, x, y, v);
            store_rgb((size_t)y * (size_t)a.width + (size_t)x, v, rgb8, radiance_out);
        }
}

template <int FILTER>
void lens_rows_filter(const LensArgs& a, const LensKnot* table, const float* radiance_in, unsigned char* rgb8, float* radiance_out)
{
    if (a.per_channel)
        lens_rows<FILTER, true>(a, table, radiance_in, rgb8, radiance_out);
    else
        lens_rows<FILTER, false>(a, table, radiance_in, rgb8, radiance_out);
}

// The distance from c along the unit direction (nx, ny) to the edge of [0, w] x [0, h] (c lies inside).
double edge_distance(double cx, double cy, double nx, double ny, double w, double h)
{
    double t = HUGE_VAL;
    if (nx > 0.0) t = std::fmin(t, (w - cx) / nx);
    if (nx < 0.0) t = std::fmin(t, (0.0 - cx) / nx);
    if (ny > 0.0) t = std::fmin(t, (h - cy) / ny);
    if (ny < 0.0) t = std::fmin(t, (0.0 - cy) / ny);
    return t;
}

} // namespace

namespace ff {

void lens_release(FfState* s)
{
    if (s->lens_table.d_table) (void)hipFree(s->lens_table.d_table);
    s->lens_table = FfState::LensTable();
}

} // namespace ff

extern "C" {

void ff_lens_params_init(FfLensParams* p)
{
    if (!p) return;
    // (DESIGN.md section 8 row 26): the identity
    std::memset(p, 0, sizeof *p);
    p->zoom = 1.f;
    p->direction = FF_LENS_UNDISTORT;
    p->filter = FF_LENS_CATMULL_ROM;
    p->border = FF_LENS_BORDER_BLACK;
    p->flags = FF_LENS_ANTI_RING;
}

int ff_lens_tables(const FfLensParams* p, int width, int height, float* out_e, float* out_gain, double* out_r2_max)
{
    clear_error();
    if (check_lens_params(p, width, height, "ff_lens_tables") != FF_OK) return FF_ERR_INVALID_ARG;
    LensModel m;
    if (lens_model(p, width, height, (double)p->zoom, &m, "ff_lens_tables") != FF_OK) return FF_ERR_INVALID_ARG;
    std::vector<LensKnot> table(kLensKnots + 1);
    lens_fill_tables(m, table.data());
    for (int j = 0; j <= kLensKnots; ++j) {
        if (out_e) out_e[j] = table[j].e;
        if (out_gain) out_gain[j] = table[j].gain;
    }
    if (out_r2_max) *out_r2_max = m.r2_max;
    return FF_OK;
}

int ff_lens_map_host(const FfLensParams* p, int width, int height, int channel, const float* xy_out, int n, float* xy_src)
{
    clear_error();
    if (check_lens_params(p, width, height, "ff_lens_map_host") != FF_OK) return FF_ERR_INVALID_ARG;
    LensModel m;
    if (lens_model(p, width, height, (double)p->zoom, &m, "ff_lens_map_host") != FF_OK) return FF_ERR_INVALID_ARG;
    if (channel < 0 || channel > 2) return fail(FF_ERR_INVALID_ARG, "ff_lens_map_host: channel %d is not 0, 1 or 2", channel);
    if (n < 0) return fail(FF_ERR_INVALID_ARG, "ff_lens_map_host: n is negative");
    if (n > 0 && !xy_out) return fail(FF_ERR_INVALID_ARG, "ff_lens_map_host: xy_out is null");
    if (n > 0 && !xy_src) return fail(FF_ERR_INVALID_ARG, "ff_lens_map_host: xy_src is null");
    for (int i = 0; i < 2 * n; ++i)
        if (!pixel_finite(xy_out[i])) return fail(FF_ERR_INVALID_ARG, "ff_lens_map_host: xy_out[%d] is not finite", i);
    LensArgs a;
    lens_args(p, width, height, m, &a);
    std::vector<LensKnot> table(kLensKnots + 1);
    lens_fill_tables(m, table.data());
    const float q = channel == 0 ? a.q_red : (channel == 2 ? a.q_blue : 0.f);
    for (int i = 0; i < n; ++i) {
        const float px = xy_out[2 * i], py = xy_out[2 * i + 1];
        float dx, dy, e, gain;
        lens_radial(a, table.data(), px, py, dx, dy, e, gain);
        lens_source(px, py, dx, dy, e, q, xy_src[2 * i], xy_src[2 * i + 1]);
    }
    return FF_OK;
}

int ff_lens_fit_zoom(const FfLensParams* p, int width, int height, int mode, float* out_zoom)
{
    clear_error();
    if (check_lens_params(p, width, height, "ff_lens_fit_zoom") != FF_OK) return FF_ERR_INVALID_ARG;
    if (mode != FF_LENS_FIT_FILL && mode != FF_LENS_FIT_ALL) return fail(FF_ERR_INVALID_ARG, "ff_lens_fit_zoom: unknown mode %d", mode);
    if (!out_zoom) return fail(FF_ERR_INVALID_ARG, "ff_lens_fit_zoom: out_zoom is null");
    // The polynomial's whole rising branch is in reach here: the zoom this call chooses decides how much of it an image uses.
    const Poly k = { (double)p->k1, (double)p->k2, (double)p->k3 };
    const double fold_t = first_fold(k, 1.0e6);
    const double fold = fold_t < 0.0 ? -1.0 : std::sqrt(fold_t);
    const double w = (double)width, h = (double)height;
    const double cx = (double)(0.5f * (float)width + p->center_x), cy = (double)(0.5f * (float)height + p->center_y);
    const double D = std::sqrt(0.25 * (w * w + h * h));
    // f's inverse at sigma on the rising branch; false where the branch ends below sigma
    auto f_inverse = [&](double sigma, double* out) {
        double hi;
        if (fold >= 0.0) {
            if (!(lens_f(k, fold) > sigma)) return false;
            hi = fold;
        } else {
            hi = sigma > 0.0 ? sigma : 1.0;
            for (int it = 0; it < 64 && lens_f(k, hi) < sigma; ++it) hi = 2.0 * hi;
        }
        *out = lens_f_inverse(k, sigma, hi);
        return true;
    };
    double zoom = mode == FF_LENS_FIT_FILL ? 0.0 : HUGE_VAL;
    const int steps_x = width, steps_y = height;
    // the border: for FILL the pixel centres of the output's outermost rows and columns, for ALL the points of the source's edge
    const int count = mode == FF_LENS_FIT_FILL ? 2 * (steps_x + steps_y) : 2 * (steps_x + steps_y) + 4;
    for (int i = 0; i < count; ++i) {
        double bx, by;
        const int side = i < 2 * steps_x ? (i < steps_x ? 0 : 1) : (i < 2 * (steps_x + steps_y) ? (i - 2 * steps_x < steps_y ? 2 : 3) : 4);
        if (mode == FF_LENS_FIT_FILL) {
            if (side < 2) { bx = (double)(i % steps_x) + 0.5; by = side == 0 ? 0.5 : h - 0.5; }
            else { by = (double)((i - 2 * steps_x) % steps_y) + 0.5; bx = side == 2 ? 0.5 : w - 0.5; }
        } else {
            if (side < 2) { bx = (double)(i % steps_x) + 0.5; by = side == 0 ? 0.0 : h; }
            else if (side < 4) { by = (double)((i - 2 * steps_x) % steps_y) + 0.5; bx = side == 2 ? 0.0 : w; }
            else { const int c = i - 2 * (steps_x + steps_y); bx = (c & 1) ? w : 0.0; by = (c & 2) ? h : 0.0; }
        }
        const double dx = bx - cx, dy = by - cy, dist = std::sqrt(dx * dx + dy * dy);
        if (!(dist > 0.0)) continue;
        const double r = dist / D;
        if (mode == FF_LENS_FIT_FILL) {
            // the output pixel at radius r may read the source up to the edge along its direction: m(r / zoom) D <= L
            const double sigma = edge_distance(cx, cy, dx / dist, dy / dist, w, h) / D;
            double rho_lim;
            if (p->direction == FF_LENS_UNDISTORT) {
                if (!f_inverse(sigma, &rho_lim)) rho_lim = fold * (1.0 - 1.0e-6); // (the source's edge is never reached: only the fold limits)
            } else {
                rho_lim = lens_f(k, sigma);
                if (fold >= 0.0 && sigma > fold) rho_lim = lens_f(k, fold) * (1.0 - 1.0e-6);
            }
            if (!(rho_lim > 0.0)) return fail(FF_ERR_INVALID_ARG, "ff_lens_fit_zoom: k1, k2, k3 leave no radius to fill the frame from");
            const double z = r / rho_lim;
            zoom = z > zoom ? z : zoom;
        } else {
            // the source's edge point at radius r appears in the output at zoom m^-1(r), which must stay inside the edge along its direction
            const double lim = edge_distance(cx, cy, dx / dist, dy / dist, w, h) / D;
            double rho;
            if (p->direction == FF_LENS_UNDISTORT) {
                if (!f_inverse(r, &rho))
                    return fail(FF_ERR_INVALID_ARG, "ff_lens_fit_zoom: k1, k2, k3 fold the image over at radius %g, before the source's edge at radius %g comes into view",
                                fold, r);
            } else {
                if (fold >= 0.0 && r >= fold)
                    return fail(FF_ERR_INVALID_ARG, "ff_lens_fit_zoom: k1, k2, k3 fold the image over at radius %g, inside the source's edge at radius %g", fold, r);
                rho = lens_f(k, r);
            }
            if (!(rho > 0.0)) continue;
            const double z = lim / rho;
            zoom = z < zoom ? z : zoom;
        }
    }
    if (mode == FF_LENS_FIT_FILL) {
        if (!(zoom > 0.0)) zoom = 1.0; // (a 1 x 1 image on its own centre)
        zoom = zoom * (1.0 + 1.0e-4);  // the margin that covers the kernel's float arithmetic and its table
    } else {
        if (!(zoom < HUGE_VAL)) zoom = 1.0;
        zoom = zoom * (1.0 - 1.0e-4);
    }
    if (!(zoom >= 0.0625 && zoom <= 16.0)) return fail(FF_ERR_INVALID_ARG, "ff_lens_fit_zoom: the zoom that fits, %g, is outside 1/16 .. 16", zoom);
    *out_zoom = (float)zoom;
    return FF_OK;
}

int ff_lens(FfState* s, int width, int height, const FfLensParams* p, const float* radiance_in, int input_on_device, void* rgb8, int rgb8_on_device,
            float* radiance_out, int radiance_out_on_device)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_lens: state is null");
    LensModel m;
    LensArgs a;
    const int st = check_lens(width, height, p, radiance_in, rgb8, radiance_out, &m, &a, "ff_lens");
    if (st != FF_OK) return st;
    FF_HIP(hipSetDevice(s->device));
    hipStream_t stream = s->stream;
    const LensKnot* table = nullptr;
    const int tst = device_table(s, p, width, height, m, stream, &table);
    if (tst != FF_OK) return tst;
    const size_t px = (size_t)width * (size_t)height;
    Staging stage(&s->d_img_work, &s->img_work_bytes);
    if (!input_on_device) stage.in(&radiance_in, radiance_in, px * 12);
    StagedOutputs out(stage, px, rgb8, rgb8_on_device, radiance_out, radiance_out_on_device);
    const int staged = stage.commit(stream, "ff_lens: staging the input failed");
    if (staged != FF_OK) return staged;
    const int max_blocks = (s->num_cus > 0 ? s->num_cus : 256) * 8;
    FF_HIP(launch_lens(a, table, radiance_in, out.rgb8, out.radiance, max_blocks, stream));
    FF_HIP(hipStreamSynchronize(stream));
    return stage.finish();
}

int ff_lens_host(int width, int height, const FfLensParams* p, const float* radiance_in, unsigned char* rgb8, float* radiance_out)
{
    clear_error();
    LensModel m;
    LensArgs a;
    const int st = check_lens(width, height, p, radiance_in, rgb8, radiance_out, &m, &a, "ff_lens_host");
    if (st != FF_OK) return st;
    std::vector<LensKnot> table(kLensKnots + 1);
    lens_fill_tables(m, table.data());
    if (a.filter == kLensBilinear)
        lens_rows_filter<kLensBilinear>(a, table.data(), radiance_in, rgb8, radiance_out);
    else if (a.filter == kLensCatmullRom)
        lens_rows_filter<kLensCatmullRom>(a, table.data(), radiance_in, rgb8, radiance_out);
    else
        lens_rows_filter<kLensCatmullRomClamped>(a, table.data(), radiance_in, rgb8, radiance_out);
    return FF_OK;
}

int ff_debug_lens_table_builds(FfState* s, uint64_t* out_builds)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_debug_lens_table_builds: state is null");
    if (!out_builds) return fail(FF_ERR_INVALID_ARG, "ff_debug_lens_table_builds: out_builds is null");
    *out_builds = s->lens_table.builds;
    return FF_OK;
}

} // extern "C"
