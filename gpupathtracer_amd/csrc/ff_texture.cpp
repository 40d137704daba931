// ff_texture.cpp — albedo textures (include/firefly/ff_api.h): the state's textures and the scene's bindings with their device
// tables, the host twins of the lookup (ff_texture_sample, ff_surface_uv: ff_texture.h's inline functions compiled for the host),
// and the PPM reader with the byte-to-linear table that turn an image file into texels.
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "ff_state.h"
#include "ff_texture.h"

using namespace ff;

namespace {

constexpr long long kMaxTexels = 1ll << 26; // ff_set_environment's bound

int check_image(const float* rgb, int width, int height, int flags, const char* who)
{
    if (!rgb) return fail(FF_ERR_INVALID_ARG, "%s: rgb is null", who);
    if (width < 1 || height < 1 || (long long)width * (long long)height > kMaxTexels)
        return fail(FF_ERR_INVALID_ARG, "%s: size %dx%d is not in 1 .. 2^26 texels", who, width, height);
    if (flags & ~(FF_TEX_CLAMP | FF_TEX_NEAREST)) return fail(FF_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x", who, flags);
    const size_t n = (size_t)width * (size_t)height * 3;
    for (size_t i = 0; i < n; ++i)
        if (!(rgb[i] >= 0.f) || !std::isfinite(rgb[i]))
            return fail(FF_ERR_INVALID_ARG, "%s: texel %zu channel %zu is %g (texels are finite and >= 0)", who, i / 3, i % 3, (double)rgb[i]);
    return FF_OK;
}

struct HostFetch {
    const float* rgb;
    int w;
    FF_TEX_HD void operator()(int x, int y, float* out) const
    {
        const float* t = rgb + ((size_t)y * (size_t)w + (size_t)x) * 3;
        out[0] = t[0];
        out[1] = t[1];
        out[2] = t[2];
    }
};

// Next token of a PPM header: skips white space and '#' comments.  -1 at the end of the file or for anything but digits.
long ppm_number(std::FILE* f)
{
    int c = std::fgetc(f);
    for (;;) {
        while (c == ' ' || c == '\t' || c == '\r' || c == '\n') c = std::fgetc(f);
        if (c != '#') break;
        while (c != '\n' && c != EOF) c = std::fgetc(f);
    }
    if (c < '0' || c > '9') return -1;
    long v = 0;
    while (c >= '0' && c <= '9') {
        v = v * 10 + (c - '0');
        if (v > (1l << 30)) return -1;
        c = std::fgetc(f);
    }
    // (the single white-space character behind the last header number - consumed here - is what separates it from P6's bytes)
    if (c != EOF && c != ' ' && c != '\t' && c != '\r' && c != '\n') return -1;
    return v;
}

} // namespace

namespace ff {

void tex_drop_bindings(FfState* s)
{
    s->tex_bindings.clear();
    s->tex_bound = 0;
}

// The device tables from the host's: one binding per record (processing order), one descriptor per texture id.
int tex_sync_tables(FfState* s)
{
    s->tex_bound = 0;
    for (const TexBinding& b : s->tex_bindings) s->tex_bound += b.tex >= 0 ? 1 : 0;
    if (s->tex_bound == 0 || !s->has_scene) {
        s->tex_bound = 0;
        return FF_OK;
    }
    std::vector<TexBinding> bind(std::max<size_t>(s->h_geoms.size(), 1));
    for (size_t r = 0; r < bind.size(); ++r) {
        std::memset(&bind[r], 0, sizeof(TexBinding));
        bind[r].tex = -1;
        const int o = r < s->h_geoms.size() ? s->h_geoms[r].orig_index : -1;
        if (o >= 0 && (size_t)o < s->tex_bindings.size()) bind[r] = s->tex_bindings[(size_t)o];
    }
    std::vector<TexDesc> desc(std::max<size_t>(s->textures.size(), 1));
    std::memset(desc.data(), 0, desc.size() * sizeof(TexDesc));
    for (size_t t = 0; t < s->textures.size(); ++t) {
        desc[t].texels = s->textures[t].d_texels;
        desc[t].w = s->textures[t].w;
        desc[t].h = s->textures[t].h;
        desc[t].flags = s->textures[t].flags;
    }
    FF_HIP(hipSetDevice(s->device));
    FF_HIP(hipStreamSynchronize(s->stream)); // (a frame in flight may still read the tables)
    int st = ensure_bytes((void**)&s->d_tex_bind, &s->tex_bind_bytes, bind.size() * sizeof(TexBinding));
    if (st == FF_OK) st = ensure_bytes((void**)&s->d_tex_desc, &s->tex_desc_bytes, desc.size() * sizeof(TexDesc));
    if (st != FF_OK) return st;
    FF_HIP(hipMemcpy(s->d_tex_bind, bind.data(), bind.size() * sizeof(TexBinding), hipMemcpyHostToDevice));
    FF_HIP(hipMemcpy(s->d_tex_desc, desc.data(), desc.size() * sizeof(TexDesc), hipMemcpyHostToDevice));
    return FF_OK;
}

void tex_release(FfState* s)
{
    for (FfState::Texture& t : s->textures)
        if (t.d_texels) (void)hipFree(t.d_texels);
    s->textures.clear();
    tex_drop_bindings(s);
    if (s->d_tex_bind) (void)hipFree(s->d_tex_bind);
    if (s->d_tex_desc) (void)hipFree(s->d_tex_desc);
    s->d_tex_bind = nullptr;
    s->d_tex_desc = nullptr;
    s->tex_bind_bytes = s->tex_desc_bytes = 0;
}

} // namespace ff

extern "C" {

int ff_texture_create(FfState* s, const float* rgb, int width, int height, int flags, int* out_id)
{
    clear_error();
    if (!s || !out_id) return fail(FF_ERR_INVALID_ARG, "ff_texture_create: null argument");
    *out_id = -1;
    int st = check_image(rgb, width, height, flags, "ff_texture_create");
    if (st != FF_OK) return st;
    const size_t n = (size_t)width * (size_t)height;
    std::vector<float4> texels(n);
    for (size_t k = 0; k < n; ++k) texels[k] = make_float4(rgb[3 * k], rgb[3 * k + 1], rgb[3 * k + 2], 0.f);
    FF_HIP(hipSetDevice(s->device));
    float4* d = nullptr;
    {
        const hipError_t e = hipMalloc((void**)&d, n * sizeof(float4));
        if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? FF_ERR_OOM : FF_ERR_HIP, "ff_texture_create: hipMalloc(%zu) failed: %s", n * sizeof(float4), hipGetErrorString(e));
    }
    {
        const hipError_t e = hipMemcpy(d, texels.data(), n * sizeof(float4), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d);
            return fail(FF_ERR_HIP, "ff_texture_create: copy failed: %s", hipGetErrorString(e));
        }
    }
    size_t id = 0;
    while (id < s->textures.size() && s->textures[id].d_texels) ++id;
    if (id == s->textures.size()) s->textures.emplace_back();
    FfState::Texture& t = s->textures[id];
    t.d_texels = d;
    t.w = width;
    t.h = height;
    t.flags = flags;
    *out_id = (int)id;
    return FF_OK; // (nothing is bound to a new id: the device tables stay as they are)
}

int ff_texture_destroy(FfState* s, int id)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_texture_destroy: state is null");
    if (id < 0 || (size_t)id >= s->textures.size() || !s->textures[(size_t)id].d_texels)
        return fail(FF_ERR_INVALID_ARG, "ff_texture_destroy: no texture %d", id);
    FF_HIP(hipSetDevice(s->device));
    FF_HIP(hipStreamSynchronize(s->stream)); // (a frame in flight may still read it)
    bool bound = false;
    for (TexBinding& b : s->tex_bindings)
        if (b.tex == id) {
            b.tex = -1;
            bound = true;
        }
    (void)hipFree(s->textures[(size_t)id].d_texels);
    s->textures[(size_t)id] = FfState::Texture();
    if (bound) {
        s->primary_valid = s->last_key_valid = false;
        return tex_sync_tables(s);
    }
    return FF_OK;
}

int ff_set_albedo_texture(FfState* s, int geometry_index, int texture_id, float scale_u, float scale_v, float offset_u, float offset_v)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_set_albedo_texture: state is null");
    if (!s->has_scene) return fail(FF_ERR_NO_SCENE, "ff_set_albedo_texture: no scene uploaded");
    const GeomRecord* rec = nullptr;
    for (const GeomRecord& g : s->h_geoms)
        if (g.orig_index == geometry_index) rec = &g;
    if (geometry_index < 0 || !rec) return fail(FF_ERR_INVALID_ARG, "ff_set_albedo_texture: geometry %d is not in the uploaded scene", geometry_index);
    if (texture_id < -1 || (texture_id >= 0 && ((size_t)texture_id >= s->textures.size() || !s->textures[(size_t)texture_id].d_texels)))
        return fail(FF_ERR_INVALID_ARG, "ff_set_albedo_texture: no texture %d", texture_id);
    if (texture_id >= 0) {
        if (!std::isfinite(scale_u) || !std::isfinite(scale_v) || !std::isfinite(offset_u) || !std::isfinite(offset_v))
            return fail(FF_ERR_INVALID_ARG, "ff_set_albedo_texture: scale and offset must be finite");
        if (rec->bxdf_type != FF_BXDF_DIFFUSE)
            return fail(FF_ERR_UNSUPPORTED, "ff_set_albedo_texture: geometry %d is not FF_BXDF_DIFFUSE (emission, specular and transmittance maps are not offered)",
                        geometry_index);
    }
    if (s->tex_bindings.size() <= (size_t)geometry_index) {
        TexBinding none;
        std::memset(&none, 0, sizeof none);
        none.tex = -1;
        s->tex_bindings.resize((size_t)geometry_index + 1, none);
    }
    TexBinding& b = s->tex_bindings[(size_t)geometry_index];
    std::memset(&b, 0, sizeof b);
    b.tex = texture_id;
    if (texture_id >= 0) {
        b.scale_u = scale_u;
        b.scale_v = scale_v;
        b.offset_u = offset_u;
        b.offset_v = offset_v;
    }
    s->primary_valid = s->last_key_valid = false; // (stored start records hold a first hit's albedo: the mega-kernels' frames start afresh)
    return tex_sync_tables(s);
}

int ff_texture_sample(const float* rgb, int width, int height, int flags, const float* uv, int n, float* out_rgb)
{
    clear_error();
    const int st = check_image(rgb, width, height, flags, "ff_texture_sample");
    if (st != FF_OK) return st;
    if (n < 0 || (n > 0 && (!uv || !out_rgb))) return fail(FF_ERR_INVALID_ARG, "ff_texture_sample: bad coordinate or output array");
    const HostFetch fetch = { rgb, width };
    for (int i = 0; i < n; ++i) tex_sample(fetch, width, height, flags, uv[2 * i], uv[2 * i + 1], out_rgb + 3 * (size_t)i);
    return FF_OK;
}

int ff_surface_uv(const FfGeometry* host_geometries, int n, int geometry_index, const int* triangle_indices, const float* world_points, int count,
                  float* out_uv)
{
    clear_error();
    if (!host_geometries || n <= 0) return fail(FF_ERR_INVALID_ARG, "ff_surface_uv: no geometries");
    if (geometry_index < 0 || geometry_index >= n) return fail(FF_ERR_INVALID_ARG, "ff_surface_uv: geometry %d is not in 0 .. %d", geometry_index, n - 1);
    if (count < 0 || (count > 0 && (!world_points || !out_uv))) return fail(FF_ERR_INVALID_ARG, "ff_surface_uv: bad point or output array");
    const FfGeometry& g = host_geometries[geometry_index];
    const float* m = g.m_inverseModelMatrix.m;
    const bool mesh = g.m_geometryType == FF_GEOM_TRIANGLEMESH;
    if (!mesh && g.m_geometryType != FF_GEOM_PLANE && g.m_geometryType != FF_GEOM_SPHERE)
        return fail(FF_ERR_INVALID_ARG, "ff_surface_uv: geometry %d has an unknown type", geometry_index);
    if (mesh && count > 0 && (!triangle_indices || !g.m_triangles)) return fail(FF_ERR_INVALID_ARG, "ff_surface_uv: a mesh needs triangle indices");
    for (int i = 0; i < count; ++i) {
        float px, py, pz;
        tex_object_point(m, m + 4, m + 8, m + 12, world_points[3 * i], world_points[3 * i + 1], world_points[3 * i + 2], px, py, pz);
        TexUV r;
        if (mesh) {
            const int ti = triangle_indices[i];
            if (ti < 0 || ti >= g.m_numberOfTriangles) return fail(FF_ERR_INVALID_ARG, "ff_surface_uv: triangle %d is not in 0 .. %d", ti, g.m_numberOfTriangles - 1);
            const FfTriangle& t = g.m_triangles[ti];
            // the record's edges: one fp32 subtraction per component (the scene compiler's)
            const float v0[3] = { t.m_v0.x, t.m_v0.y, t.m_v0.z };
            const float e1[3] = { t.m_v1.x - t.m_v0.x, t.m_v1.y - t.m_v0.y, t.m_v1.z - t.m_v0.z };
            const float e2[3] = { t.m_v2.x - t.m_v0.x, t.m_v2.y - t.m_v0.y, t.m_v2.z - t.m_v0.z };
            const float uv3[6] = { t.m_uv0.x, t.m_uv0.y, t.m_uv1.x, t.m_uv1.y, t.m_uv2.x, t.m_uv2.y };
            r = tex_triangle_uv(v0, e1, e2, uv3, px, py, pz);
        } else if (g.m_geometryType == FF_GEOM_PLANE) {
            r = tex_plane_uv(px, py);
        } else {
            r = tex_sphere_uv(px, py, pz);
        }
        out_uv[2 * i] = r.u;
        out_uv[2 * i + 1] = r.v;
    }
    return FF_OK;
}

int ff_load_ppm(const char* path, unsigned char** out_rgb8, int* out_width, int* out_height)
{
    clear_error();
    if (!path || !out_rgb8 || !out_width || !out_height) return fail(FF_ERR_INVALID_ARG, "ff_load_ppm: null argument");
    *out_rgb8 = nullptr;
    *out_width = *out_height = 0;
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return fail(FF_ERR_IO, "ff_load_ppm: cannot open '%s': %s", path, std::strerror(errno));
    struct Closer {
        std::FILE* f;
        ~Closer() { std::fclose(f); }
    } closer = { f };
    const int c0 = std::fgetc(f), c1 = std::fgetc(f);
    if (c0 != 'P' || (c1 != '3' && c1 != '6')) return fail(FF_ERR_INVALID_ARG, "ff_load_ppm: %s: not a P3 or P6 file", path);
    const long w = ppm_number(f), h = ppm_number(f), maxval = ppm_number(f);
    if (w < 1 || h < 1 || (long long)w * (long long)h > kMaxTexels) return fail(FF_ERR_INVALID_ARG, "ff_load_ppm: %s: size %ldx%ld is not in 1 .. 2^26 pixels", path, w, h);
    if (maxval != 255) return fail(FF_ERR_INVALID_ARG, "ff_load_ppm: %s: maxval %ld (only 8-bit files, maxval 255)", path, maxval);
    const size_t n = (size_t)w * (size_t)h * 3;
    unsigned char* px = static_cast<unsigned char*>(std::malloc(n));
    if (!px) return fail(FF_ERR_OOM, "ff_load_ppm: %s: out of host memory for %ldx%ld", path, w, h);
    bool ok = true;
    if (c1 == '6') {
        ok = std::fread(px, 1, n, f) == n;
    } else {
        for (size_t i = 0; i < n && ok; ++i) {
            const long v = ppm_number(f);
            if (v < 0 || v > 255) ok = false;
            else px[i] = (unsigned char)v;
        }
    }
    if (!ok) {
        std::free(px);
        return fail(FF_ERR_IO, "ff_load_ppm: %s: the pixel data ends early or holds a value outside 0 .. 255", path);
    }
    *out_rgb8 = px;
    *out_width = (int)w;
    *out_height = (int)h;
    return FF_OK;
}

void ff_free_ppm(unsigned char* rgb8) { std::free(rgb8); }

int ff_rgb8_to_linear(const unsigned char* bytes, int n, int srgb, float* out_floats)
{
    clear_error();
    if (n < 0 || (n > 0 && (!bytes || !out_floats))) return fail(FF_ERR_INVALID_ARG, "ff_rgb8_to_linear: bad argument");
    float table[256];
    for (int b = 0; b < 256; ++b) {
        const double v = (double)b / 255.0;
        table[b] = (float)(!srgb ? v : (v <= 0.04045 ? v / 12.92 : std::pow((v + 0.055) / 1.055, 2.4))); // ff_display's eotf
    }
    for (int i = 0; i < n; ++i) out_floats[i] = table[bytes[i]];
    return FF_OK;
}

} // extern "C"
