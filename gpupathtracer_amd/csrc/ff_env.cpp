// ff_env.cpp — the environment light: its sampling table on the host, the state's device copy, and the Radiance .hdr reader.
//
// A map is W x H linear RGB texels, row 0 at the top (+Y), looked up at the nearest texel, so its radiance is constant per texel
// and a texel's pdf in solid angle is exact.  Texels are chosen with probability luminance x solid angle / sum (a Vose alias table,
// built in double like the light table of ff_nee.cpp); a map of zero total luminance has an empty table and is never sampled.
// The estimator is in ff_api.h; the kernel is nee_path_kernel<..., ENV = 1> (ff_k_nee.h).
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ff_state.h"

using namespace ff;

namespace {

constexpr long long kMaxEnvTexels = 1ll << 26;
constexpr double kPiD = 3.14159265358979323846;

struct EnvTableD {
    std::vector<double> prob;       // p_k = w_k / sum (0 everywhere if the sum is 0)
    std::vector<double> alias_prob; // Vose: texel k = floor(u0 n) is kept if u1 < alias_prob_k, else alias_k
    std::vector<int> alias;
    std::vector<double> pdf;        // p_k / Omega_k per steradian
    std::vector<double> z;          // H + 1 row bounds cos(pi r / H)
    bool sampled = false;
};

int check_map(const float* rgb, int w, int h, const char* who)
{
    if (!rgb) return fail(FF_ERR_INVALID_ARG, "%s: texel array is null", who);
    if (w < 1 || h < 1) return fail(FF_ERR_INVALID_ARG, "%s: the map must be at least 1x1 (got %dx%d)", who, w, h);
    if ((long long)w * (long long)h > kMaxEnvTexels)
        return fail(FF_ERR_INVALID_ARG, "%s: %dx%d is more than 2^26 texels", who, w, h);
    const size_t n = (size_t)w * (size_t)h * 3;
    for (size_t i = 0; i < n; ++i)
        if (!(rgb[i] >= 0.f) || !std::isfinite(rgb[i]))
            return fail(FF_ERR_INVALID_ARG, "%s: texel %zu (row %zu, column %zu) has a negative or non-finite value %g", who, i / 3,
                        i / 3 / (size_t)w, i / 3 % (size_t)w, (double)rgb[i]);
    return FF_OK;
}

// The table of a checked map, in double.
void compute_env_table(const float* rgb, int w, int h, EnvTableD& t)
{
    const size_t n = (size_t)w * (size_t)h;
    t.z.resize((size_t)h + 1);
    for (int r = 0; r <= h; ++r) t.z[(size_t)r] = std::cos(kPiD * (double)r / (double)h);
    t.z[0] = 1.0;
    t.z[(size_t)h] = -1.0;
    std::vector<double> omega((size_t)h);
    for (int r = 0; r < h; ++r) omega[(size_t)r] = (2.0 * kPiD / (double)w) * (t.z[(size_t)r] - t.z[(size_t)r + 1]);
    t.prob.assign(n, 0.0);
    double sum = 0.0;
    for (size_t k = 0; k < n; ++k) {
        const double lum = 0.2126 * (double)rgb[3 * k] + 0.7152 * (double)rgb[3 * k + 1] + 0.0722 * (double)rgb[3 * k + 2];
        t.prob[k] = lum * omega[k / (size_t)w];
        sum += t.prob[k];
    }
    t.alias_prob.assign(n, 1.0);
    t.alias.resize(n);
    for (size_t k = 0; k < n; ++k) t.alias[k] = (int)k;
    t.pdf.assign(n, 0.0);
    t.sampled = sum > 0.0 && std::isfinite(sum);
    if (!t.sampled) {
        std::fill(t.prob.begin(), t.prob.end(), 0.0);
        return;
    }
    for (size_t k = 0; k < n; ++k) {
        t.prob[k] /= sum;
        t.pdf[k] = t.prob[k] / omega[k / (size_t)w];
    }
    // Vose's alias method (as ff_nee.cpp builds the light table)
    std::vector<double> q(n);
    std::vector<size_t> small, large;
    for (size_t k = 0; k < n; ++k) {
        q[k] = t.prob[k] * (double)n;
        (q[k] < 1.0 ? small : large).push_back(k);
    }
    while (!small.empty() && !large.empty()) {
        const size_t s = small.back(), l = large.back();
        small.pop_back();
        large.pop_back();
        t.alias_prob[s] = q[s];
        t.alias[s] = (int)l;
        q[l] = (q[l] + q[s]) - 1.0;
        (q[l] < 1.0 ? small : large).push_back(l);
    }
    for (size_t k : large) t.alias_prob[k] = 1.0;
    for (size_t k : small) t.alias_prob[k] = 1.0; // (rounding leftovers)
}

// ---- Radiance RGBE (.hdr) ---------------------------------------------------------------------------------------------------

struct HdrFile {
    FILE* f = nullptr;
    ~HdrFile()
    {
        if (f) std::fclose(f);
    }
};

// One header line without its newline; false at the end of the file.
bool read_line(FILE* f, std::string& line)
{
    line.clear();
    int c;
    while ((c = std::fgetc(f)) != EOF) {
        if (c == '\n') return true;
        line.push_back((char)c);
        if (line.size() > 4096) return true; // (the caller finds no valid header line this long)
    }
    return !line.empty();
}

// One scanline of w RGBE pixels (4 bytes each) into px: flat, or new-style run-length encoded (2, 2, w >> 8, w & 255, then the four
// channels one after another as runs: a count byte c > 128 repeats the next byte c - 128 times, 0 < c <= 128 copies c bytes).
int read_scanline(FILE* f, int w, unsigned char* px, const char* path, int row)
{
    unsigned char head[4];
    if (std::fread(head, 1, 4, f) != 4) return fail(FF_ERR_IO, "ff_load_hdr: %s: truncated at scanline %d", path, row);
    if (w < 8 || w > 0x7FFF || head[0] != 2 || head[1] != 2 || (head[2] & 0x80)) {
        std::memcpy(px, head, 4);
        if (w > 1 && std::fread(px + 4, 4, (size_t)w - 1, f) != (size_t)w - 1)
            return fail(FF_ERR_IO, "ff_load_hdr: %s: truncated at scanline %d", path, row);
        return FF_OK;
    }
    if (((int)head[2] << 8 | head[3]) != w)
        return fail(FF_ERR_INVALID_ARG, "ff_load_hdr: %s: scanline %d is encoded for width %d, not %d", path, row, (int)head[2] << 8 | head[3], w);
    for (int ch = 0; ch < 4; ++ch) {
        int x = 0;
        while (x < w) {
            const int c = std::fgetc(f);
            if (c == EOF) return fail(FF_ERR_IO, "ff_load_hdr: %s: truncated at scanline %d", path, row);
            if (c > 128) {
                const int run = c - 128, v = std::fgetc(f);
                if (v == EOF) return fail(FF_ERR_IO, "ff_load_hdr: %s: truncated at scanline %d", path, row);
                if (x + run > w) return fail(FF_ERR_INVALID_ARG, "ff_load_hdr: %s: a run overflows scanline %d", path, row);
                for (int i = 0; i < run; ++i) px[4 * (x + i) + ch] = (unsigned char)v;
                x += run;
            } else {
                if (c == 0 || x + c > w) return fail(FF_ERR_INVALID_ARG, "ff_load_hdr: %s: a bad run count in scanline %d", path, row);
                for (int i = 0; i < c; ++i) {
                    const int v = std::fgetc(f);
                    if (v == EOF) return fail(FF_ERR_IO, "ff_load_hdr: %s: truncated at scanline %d", path, row);
                    px[4 * (x + i) + ch] = (unsigned char)v;
                }
                x += c;
            }
        }
    }
    return FF_OK;
}

} // namespace

namespace ff {

void env_release(FfState* s)
{
    if (s->d_env_texels) (void)hipFree(s->d_env_texels);
    if (s->d_env_alias) (void)hipFree(s->d_env_alias);
    if (s->d_env_z) (void)hipFree(s->d_env_z);
    s->d_env_texels = nullptr;
    s->d_env_alias = nullptr;
    s->d_env_z = nullptr;
    s->env_texels_bytes = s->env_alias_bytes = s->env_z_bytes = 0;
    s->env_set = s->env_sampled = false;
}

} // namespace ff

extern "C" {

int ff_set_environment(FfState* s, const float* rgb, int width, int height, float intensity, float rotation_deg)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_set_environment: state is null");
    if (!rgb) {
        FF_HIP(hipSetDevice(s->device));
        FF_HIP(hipStreamSynchronize(s->stream)); // (a frame in flight may still read the table)
        env_release(s);
        return FF_OK;
    }
    int st = check_map(rgb, width, height, "ff_set_environment");
    if (st != FF_OK) return st;
    if (!(intensity >= 0.f) || !std::isfinite(intensity))
        return fail(FF_ERR_INVALID_ARG, "ff_set_environment: intensity must be finite and >= 0 (got %g)", (double)intensity);
    if (!std::isfinite(rotation_deg)) return fail(FF_ERR_INVALID_ARG, "ff_set_environment: rotation must be finite");
    EnvTableD t;
    compute_env_table(rgb, width, height, t);
    const size_t n = (size_t)width * (size_t)height;
    std::vector<float4> texels(n);
    std::vector<float2> alias(n);
    for (size_t k = 0; k < n; ++k) {
        // (radiance: intensity x texel in float, as a direct view of the map shows it)
        texels[k] = make_float4(intensity * rgb[3 * k], intensity * rgb[3 * k + 1], intensity * rgb[3 * k + 2], (float)t.pdf[k]);
        int a = t.alias[k];
        float af;
        std::memcpy(&af, &a, 4);
        alias[k] = make_float2((float)t.alias_prob[k], af);
    }
    std::vector<float> z(t.z.begin(), t.z.end());
    double rot = std::fmod((double)rotation_deg, 360.0);
    if (rot < 0.0) rot += 360.0;
    float rad = (float)(rot * kPiD / 180.0);
    if (!(rad < 6.28318530717958648f)) rad = 0.f;
    FF_HIP(hipSetDevice(s->device));
    FF_HIP(hipStreamSynchronize(s->stream));
    s->env_set = false; // (until the new table is in place)
    st = ensure_bytes((void**)&s->d_env_texels, &s->env_texels_bytes, n * sizeof(float4));
    if (st == FF_OK) st = ensure_bytes((void**)&s->d_env_alias, &s->env_alias_bytes, n * sizeof(float2));
    if (st == FF_OK) st = ensure_bytes((void**)&s->d_env_z, &s->env_z_bytes, z.size() * sizeof(float));
    if (st != FF_OK) {
        env_release(s);
        return st;
    }
    FF_HIP(hipMemcpy(s->d_env_texels, texels.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    FF_HIP(hipMemcpy(s->d_env_alias, alias.data(), n * sizeof(float2), hipMemcpyHostToDevice));
    FF_HIP(hipMemcpy(s->d_env_z, z.data(), z.size() * sizeof(float), hipMemcpyHostToDevice));
    s->env_w = width;
    s->env_h = height;
    s->env_rotation = rad;
    s->env_sampled = t.sampled;
    s->env_set = true;
    return FF_OK;
}

int ff_environment_table(const float* rgb, int width, int height, float* out_probability, float* out_alias_probability, int* out_alias,
                         float* out_pdf)
{
    clear_error();
    const int st = check_map(rgb, width, height, "ff_environment_table");
    if (st != FF_OK) return st;
    EnvTableD t;
    compute_env_table(rgb, width, height, t);
    const size_t n = (size_t)width * (size_t)height;
    for (size_t k = 0; k < n; ++k) {
        if (out_probability) out_probability[k] = (float)t.prob[k];
        if (out_alias_probability) out_alias_probability[k] = (float)t.alias_prob[k];
        if (out_alias) out_alias[k] = t.alias[k];
        if (out_pdf) out_pdf[k] = (float)t.pdf[k];
    }
    return FF_OK;
}

int ff_load_hdr(const char* path, float** out_rgb, int* out_width, int* out_height)
{
    clear_error();
    if (!path || !out_rgb || !out_width || !out_height) return fail(FF_ERR_INVALID_ARG, "ff_load_hdr: null argument");
    *out_rgb = nullptr;
    *out_width = *out_height = 0;
    HdrFile hf;
    hf.f = std::fopen(path, "rb");
    if (!hf.f) return fail(FF_ERR_IO, "ff_load_hdr: cannot open '%s': %s", path, std::strerror(errno));
    std::string line;
    if (!read_line(hf.f, line) || line.size() < 2 || line[0] != '#' || line[1] != '?')
        return fail(FF_ERR_INVALID_ARG, "ff_load_hdr: %s: not a Radiance file (no #? signature)", path);
    bool ended = false;
    while (read_line(hf.f, line)) {
        if (line.empty()) {
            ended = true;
            break;
        }
        if (line.compare(0, 7, "FORMAT=") == 0 && line != "FORMAT=32-bit_rle_rgbe")
            return fail(FF_ERR_INVALID_ARG, "ff_load_hdr: %s: unsupported %s (only 32-bit_rle_rgbe)", path, line.c_str());
    }
    if (!ended) return fail(FF_ERR_IO, "ff_load_hdr: %s: the header does not end", path);
    if (!read_line(hf.f, line)) return fail(FF_ERR_IO, "ff_load_hdr: %s: no resolution line", path);
    int w = 0, h = 0;
    char tail = 0;
    if (std::sscanf(line.c_str(), "-Y %d +X %d%c", &h, &w, &tail) != 2)
        return fail(FF_ERR_INVALID_ARG, "ff_load_hdr: %s: unsupported resolution line '%.64s' (only '-Y h +X w')", path, line.c_str());
    if (w < 1 || h < 1 || (long long)w * (long long)h > kMaxEnvTexels)
        return fail(FF_ERR_INVALID_ARG, "ff_load_hdr: %s: size %dx%d is not in 1 .. 2^26 texels", path, w, h);
    const size_t n = (size_t)w * (size_t)h;
    float* rgb = static_cast<float*>(std::malloc(n * 3 * sizeof(float)));
    if (!rgb) return fail(FF_ERR_OOM, "ff_load_hdr: %s: out of host memory for %dx%d", path, w, h);
    std::vector<unsigned char> px((size_t)w * 4);
    for (int y = 0; y < h; ++y) {
        const int st = read_scanline(hf.f, w, px.data(), path, y);
        if (st != FF_OK) {
            std::free(rgb);
            return st;
        }
        float* o = rgb + (size_t)y * (size_t)w * 3;
        for (int x = 0; x < w; ++x) {
            const unsigned char* p = &px[4 * (size_t)x];
            // m x 2^(e - 136) (exact in float); e = 0 is black
            const float f = p[3] == 0 ? 0.f : std::ldexp(1.0f, (int)p[3] - 136);
            o[3 * x] = (float)p[0] * f;
            o[3 * x + 1] = (float)p[1] * f;
            o[3 * x + 2] = (float)p[2] * f;
        }
    }
    *out_rgb = rgb;
    *out_width = w;
    *out_height = h;
    return FF_OK;
}

void ff_free_hdr(float* rgb) { std::free(rgb); }

} // extern "C"
