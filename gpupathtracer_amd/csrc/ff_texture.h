// ff_texture.h — albedo textures: the surface coordinate of a hit and the texel lookup, as inline functions compiled for the host and
// the device alike.  nee_path_kernel (ff_k_nee.h), gbuffer_resolve_kernel (ff_denoise.hip) and the host twins ff_surface_uv /
// ff_texture_sample (ff_texture.cpp) all call these, so the integrator, the G-buffer and the host agree on every operation.
//
// Arithmetic: float32 throughout, every expression evaluated exactly as parenthesised below, no fused multiply-add (the library is
// built with -ffp-contract=off), divisions correctly rounded.  Planes and triangles use only + - * / and floor, so host and device
// agree bit for bit; a sphere's coordinate goes through atan2f / acosf / sqrtf, whose host and device versions may differ by an ulp.
//
// Surface coordinate of the WORLD hit point x on a geometry (never a function of the ray):
//   object point   p_k = (I0_k x.x + I1_k x.y) + (I2_k x.z + I3_k), I0..I3 the columns of m_inverseModelMatrix, k = x, y, z
//   triangle       (v0, e1, e2) of the record, e1 = v1 - v0, e2 = v2 - v0;  d = p - v0;  dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z
//                  d00 = dot(e1, e1), d01 = dot(e1, e2), d11 = dot(e2, e2), d20 = dot(d, e1), d21 = dot(d, e2)
//                  den = d00 d11 - d01 d01;  u = (d11 d20 - d01 d21) / den;  v = (d00 d21 - d01 d20) / den
//                  uv = (uv0 + u (uv1 - uv0)) + v (uv2 - uv0) per component
//   plane          uv = (p.x + 0.5, p.y + 0.5) of the unit quad
//   sphere         u = atan2f(p.x, -p.z) * (1 / 2 pi), plus 1 if negative;  v = 1 - acosf(min(max(p.y / sqrtf(dot(p, p)), -1), 1)) * (1 / pi)
//                  (the environment map's orientation: +Y is the top row, u = 0 faces -Z)
// Lookup coordinate: c = uv * scale + offset per component (one multiplication, one addition).
//
// Texel lookup of (cu, cv) in a W x H texture, row 0 the top of the image (v = 1, the OBJ convention):
//   sanitise       a coordinate that is NaN or +-Inf reads as 0.  Then FF_TEX_REPEAT: c = c - floor(c), in [0, 1] (exact for c >= 0),
//                  which makes the lookup periodic bit for bit; FF_TEX_CLAMP: c = min(max(c, 0), 1).  Every index below is
//                  therefore in range before it becomes an integer, for any bit pattern of the coordinate.
//   bilinear       s = cu W - 0.5, t = (1 - cv) H - 0.5;  x0 = floor(s), fx = s - x0, y0 = floor(t), fy = t - y0;  taps x0, x0 + 1 and
//                  y0, y0 + 1: REPEAT adds W to a tap below 0 and subtracts W from one above W - 1, CLAMP clamps it into 0 .. W - 1
//                  a = T(x0, y0), b = T(x0 + 1, y0), c = T(x0, y0 + 1), d = T(x0 + 1, y0 + 1)
//                  top = a + fx (b - a), bot = c + fx (d - c), out = top + fy (bot - top): a constant texture returns its value exactly
//   nearest        x = floor(cu W), y = floor((1 - cv) H); REPEAT maps W to 0, CLAMP to W - 1 (the same in y)
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FF_TEX_HD __host__ __device__ __forceinline__
#else
#define FF_TEX_HD inline
#endif

namespace ff {

// flag bits (FfTextureFlags in ff_types.h)
constexpr int kTexClamp = 1, kTexNearest = 2;

struct TexUV {
    float u, v;
};

FF_TEX_HD float tex_dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

// p = inverseModel * (x, 1); i0 .. i3: the matrix's columns (three floats each are read)
FF_TEX_HD void tex_object_point(const float* i0, const float* i1, const float* i2, const float* i3, float x, float y, float z, float& px, float& py, float& pz)
{
    px = (i0[0] * x + i1[0] * y) + (i2[0] * z + i3[0]);
    py = (i0[1] * x + i1[1] * y) + (i2[1] * z + i3[1]);
    pz = (i0[2] * x + i1[2] * y) + (i2[2] * z + i3[2]);
}

// uv3: the triangle's {uv0, uv1, uv2} as six floats
FF_TEX_HD TexUV tex_triangle_uv(const float* v0, const float* e1, const float* e2, const float* uv3, float px, float py, float pz)
{
    const float dx = px - v0[0], dy = py - v0[1], dz = pz - v0[2];
    const float d00 = tex_dot3(e1[0], e1[1], e1[2], e1[0], e1[1], e1[2]);
    const float d01 = tex_dot3(e1[0], e1[1], e1[2], e2[0], e2[1], e2[2]);
    const float d11 = tex_dot3(e2[0], e2[1], e2[2], e2[0], e2[1], e2[2]);
    const float d20 = tex_dot3(dx, dy, dz, e1[0], e1[1], e1[2]);
    const float d21 = tex_dot3(dx, dy, dz, e2[0], e2[1], e2[2]);
    const float den = d00 * d11 - d01 * d01;
    const float u = (d11 * d20 - d01 * d21) / den;
    const float v = (d00 * d21 - d01 * d20) / den;
    TexUV r;
    r.u = (uv3[0] + u * (uv3[2] - uv3[0])) + v * (uv3[4] - uv3[0]);
    r.v = (uv3[1] + u * (uv3[3] - uv3[1])) + v * (uv3[5] - uv3[1]);
    return r;
}

FF_TEX_HD TexUV tex_plane_uv(float px, float py)
{
    TexUV r;
    r.u = px + 0.5f;
    r.v = py + 0.5f;
    return r;
}

FF_TEX_HD TexUV tex_sphere_uv(float px, float py, float pz)
{
    constexpr float kInvTwoPi = 0.15915494309189535f, kInvPi = 0.31830988618379067f;
    TexUV r;
    r.u = atan2f(px, -pz) * kInvTwoPi;
    if (r.u < 0.f) r.u = r.u + 1.0f;
    const float c = py / sqrtf(tex_dot3(px, py, pz, px, py, pz));
    r.v = 1.0f - acosf(fminf(fmaxf(c, -1.f), 1.f)) * kInvPi;
    return r;
}

// The sanitised coordinate, in [0, 1].
FF_TEX_HD float tex_wrap(float c, bool clamp)
{
    if (!(fabsf(c) <= 3.0e38f)) c = 0.f; // NaN, +-Inf
    if (clamp) return fminf(fmaxf(c, 0.f), 1.f);
    c = c - floorf(c);
    return fminf(fmaxf(c, 0.f), 1.f); // (already there; keeps the bound independent of the subtraction)
}

FF_TEX_HD int tex_tap(int i, int n, bool clamp)
{
    if (clamp) return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
    if (i < 0) i += n;
    if (i > n - 1) i -= n;
    return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); // (a 1-wide texture: -1 + 1 = 0, 1 - 1 = 0; the bound holds regardless)
}

// fetch(x, y, rgb): texel (x, y) of the texture, 0 <= x < W, 0 <= y < H, as three floats.
template <class Fetch>
FF_TEX_HD void tex_sample(const Fetch& fetch, int W, int H, int flags, float cu, float cv, float* out)
{
    const bool clamp = (flags & kTexClamp) != 0;
    const float u = tex_wrap(cu, clamp), v = tex_wrap(cv, clamp);
    if (flags & kTexNearest) {
        const int x = (int)floorf(u * (float)W), y = (int)floorf((1.0f - v) * (float)H);
        fetch(x > W - 1 ? (clamp ? W - 1 : 0) : x, y > H - 1 ? (clamp ? H - 1 : 0) : y, out);
        return;
    }
    const float s = u * (float)W - 0.5f, t = (1.0f - v) * (float)H - 0.5f;
    const float xf = floorf(s), yf = floorf(t);
    const float fx = s - xf, fy = t - yf;
    const int x0 = tex_tap((int)xf, W, clamp), x1 = tex_tap((int)xf + 1, W, clamp);
    const int y0 = tex_tap((int)yf, H, clamp), y1 = tex_tap((int)yf + 1, H, clamp);
    float a[3], b[3], c[3], d[3];
    fetch(x0, y0, a);
    fetch(x1, y0, b);
    fetch(x0, y1, c);
    fetch(x1, y1, d);
    for (int k = 0; k < 3; ++k) {
        const float top = a[k] + fx * (b[k] - a[k]);
        const float bot = c[k] + fx * (d[k] - c[k]);
        out[k] = top + fy * (bot - top);
    }
}

// ---- device tables (global memory) -------------------------------------------------------------------------------------------

// One per geometry record (processing order): the texture bound to its albedo, or tex < 0.
struct TexBinding {
    int tex;
    float scale_u, scale_v, offset_u, offset_v;
    int pad[3];
};
static_assert(sizeof(TexBinding) == 32, "32-byte binding");

// One per texture id: W x H texels of {r, g, b, 0}, row 0 the top (one tap is one 16-byte load); texels == null: a free id.
struct TexDesc {
    const void* texels;
    int w, h, flags, pad;
    long long pad2;
};
static_assert(sizeof(TexDesc) == 32, "32-byte descriptor");

// The three UV pairs of a triangle, parallel to the TriRecords (record order).
struct TriUVs {
    float uv[6];
};
static_assert(sizeof(TriUVs) == 24, "24-byte UV record");

#if defined(__HIPCC__)
struct TexFetch4 {
    const float4* texels;
    int w;
    FF_TEX_HD void operator()(int x, int y, float* out) const
    {
        const float4 t = texels[(size_t)y * (size_t)w + (size_t)x];
        out[0] = t.x;
        out[1] = t.y;
        out[2] = t.z;
    }
};

// The texel that multiplies the albedo of record g at the world point (x, y, z), or false if nothing is bound to it.  geom: the
// record's 72 leading floats are read as the four inverse-model columns (GeomRecord::inv_c0 .. inv_c3, four floats apart); type: its
// FfGeometryType; rec: the hit's triangle record (-1 for planes and spheres); tris: the TriRecord array as floats (12 per record:
// v0 at 0, e1 at 4, e2 at 8); uvs: the TriUVs array.
FF_TEX_HD bool tex_albedo(const TexBinding* __restrict__ bind, const TexDesc* __restrict__ desc, const TriUVs* __restrict__ uvs, int g, int rec, int type,
                          const float* __restrict__ geom, const float* __restrict__ tris, float x, float y, float z, float* out)
{
    const TexBinding b = bind[g];
    if (b.tex < 0) return false;
    float px, py, pz;
    tex_object_point(geom, geom + 4, geom + 8, geom + 12, x, y, z, px, py, pz);
    TexUV r;
    if (rec >= 0) {
        const float* t = tris + (size_t)rec * 12;
        const float v0[3] = { t[0], t[1], t[2] }, e1[3] = { t[4], t[5], t[6] }, e2[3] = { t[8], t[9], t[10] };
        const TriUVs u = uvs[rec];
        r = tex_triangle_uv(v0, e1, e2, u.uv, px, py, pz);
    } else if (type == 1 /* FF_GEOM_PLANE */) {
        r = tex_plane_uv(px, py);
    } else {
        r = tex_sphere_uv(px, py, pz);
    }
    const TexDesc d = desc[b.tex];
    const TexFetch4 fetch = { reinterpret_cast<const float4*>(d.texels), d.w };
    tex_sample(fetch, d.w, d.h, d.flags, r.u * b.scale_u + b.offset_u, r.v * b.scale_v + b.offset_v, out);
    return true;
}
#endif

} // namespace ff
