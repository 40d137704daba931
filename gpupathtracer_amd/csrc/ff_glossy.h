// ff_glossy.h — the rough-specular (GGX) conductor lobe: its value, its pdf and its sampler, as inline functions compiled for the
// host and the device alike.  nee_path_kernel<..., GLOSSY = 1> (ff_k_nee.h) and the host twins ff_glossy_eval / ff_glossy_sample
// (ff_glossy.cpp) call these, so the integrator and the host agree on every operation.  The estimator they serve is in ff_api.h.
//
// Arithmetic: float32 throughout, every expression evaluated exactly as parenthesised below, no fused multiply-add (the library is
// built with -ffp-contract=off).  Quotients are a * rcp(b) and roots sqrt(x), both correctly rounded: FF_GLOSSY_RCP / FF_GLOSSY_SQRT
// are the kernels' ieee_rcp / ieee_sqrt on the device (ff_k_core.h defines them before it includes this file) and 1.0f / x, sqrtf
// on the host - the same bits.  The sampler's sine and cosine are fixed-order polynomials on an exactly reduced octant (the scheme
// of the diffuse bounce's cosine_sample), so the sampled direction, too, is the same on the host and on the device bit for bit.
//
// Directions are in the local frame of the hit: z the unit normal flipped against the incoming ray, x and y the Duff basis scatter
// builds.  wo points to the viewer, wi to the light; alpha = roughness * roughness; every w.z in a quotient is clamped to >= 1e-6.
//   h         = (wo + wi) / |wo + wi|
//   D(h)      = alpha^2 / (pi q^2),  q = alpha^2 h.z^2 + (h.x^2 + h.y^2)       (no (h.z^2 (alpha^2 - 1) + 1): it loses all digits at small alpha)
//   Lambda(w) = (sqrt(1 + alpha^2 (w.x^2 + w.y^2) / w.z^2) - 1) / 2
//   G1(w)     = 1 / (1 + Lambda(w)),  G2(wo, wi) = 1 / (1 + Lambda(wo) + Lambda(wi))    (height-correlated Smith)
//   F(c)      = F0 + (1 - F0) m^5,  m = 1 - c,  c = max(dot(wo, h), 0),  m^5 = (m2 m2) m with m2 = m m        (Schlick)
//   f         = F D G2 / (4 wo.z wi.z)                                          (the BRDF, not times cosine; 0 for wi.z <= 0)
//   pdf_b     = G1(wo) D(h) / (4 wo.z)                                          (visible normals, over 4 dot(wo, h))
//   weight    = f wi.z / pdf_b = F G2 / G1 = F (1 + Lambda(wo)) / ((1 + Lambda(wo)) + Lambda(wi)), computed in that form
// Sampler (visible normals by spherical caps: Dupuy and Benyoub 2023), from k24 = the 24-bit integer of u1 and u2 in [0, 1):
//   v = unit(alpha wo.x, alpha wo.y, wo.z);  z = (1 - u2)(1 + v.z) - v.z;  r = sqrt(max(0, 1 - z^2))
//   c = (r cos(2 pi u1), r sin(2 pi u1), z);  h' = c + v;  h = unit(alpha h'.x, alpha h'.y, max(h'.z, 0));  wi = 2 dot(wo, h) h - wo
//   wi.z <= 0 (or h' = 0): the sample fails - weight and pdf 0.  Otherwise weight and pdf are the expressions above evaluated at
//   (wo, wi), with h recomputed from them: the pdf a sample carries is bit for bit the pdf glossy_eval gives its direction.
#pragma once

#include <math.h>

#if defined(FF_GLOSSY_HD)
// (ff_k_core.h: device only, with the kernels' own reciprocal and root)
#elif defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FF_GLOSSY_HD __host__ __device__ __forceinline__
#else
#define FF_GLOSSY_HD inline
#endif

#ifndef FF_GLOSSY_RCP
#define FF_GLOSSY_RCP(x) (1.0f / (x))
#define FF_GLOSSY_SQRT(x) sqrtf(x)
#endif

namespace ff {

constexpr float kGlossyMinAlpha = 1.0e-3f; // a binding below it shades as the perfect mirror
constexpr float kGlossyMinCos = 1.0e-6f;   // clamp of w.z in quotients

struct GlossyLobe {
    float fr, fg, fb; // F D G2 / (4 wo.z wi.z) per channel
    float pdf;        // pdf_b(wi), per steradian
    float wr, wg, wb; // F G2 / G1 per channel
};

FF_GLOSSY_HD float glossy_dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

FF_GLOSSY_HD float glossy_lambda(float a2, float wx, float wy, float wz)
{
    const float z = fmaxf(wz, kGlossyMinCos);
    const float t = (a2 * (wx * wx + wy * wy)) * FF_GLOSSY_RCP(z * z);
    return (FF_GLOSSY_SQRT(1.0f + t) - 1.0f) * 0.5f;
}

// The lobe at (wo, wi), both unit, wo.z already clamped to >= kGlossyMinCos; all zeros for wi.z <= 0.
FF_GLOSSY_HD GlossyLobe glossy_eval(float alpha, float f0r, float f0g, float f0b, float wox, float woy, float woz, float wix, float wiy, float wiz)
{
    GlossyLobe o = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
    if (!(wiz > 0.f)) return o;
    constexpr float kPi = 3.14159265358979324f;
    const float a2 = alpha * alpha;
    const float sx = wox + wix, sy = woy + wiy, sz = woz + wiz;
    const float sinv = FF_GLOSSY_RCP(FF_GLOSSY_SQRT(glossy_dot3(sx, sy, sz, sx, sy, sz)));
    const float hx = sx * sinv, hy = sy * sinv, hz = sz * sinv;
    const float q = a2 * (hz * hz) + (hx * hx + hy * hy);
    const float D = a2 * FF_GLOSSY_RCP(kPi * (q * q));
    const float lo = glossy_lambda(a2, wox, woy, woz), li = glossy_lambda(a2, wix, wiy, wiz);
    const float one_lo = 1.0f + lo;
    const float G1 = FF_GLOSSY_RCP(one_lo), G2 = FF_GLOSSY_RCP(one_lo + li);
    const float c = fmaxf(glossy_dot3(wox, woy, woz, hx, hy, hz), 0.f);
    const float m = 1.0f - c, m2 = m * m, m5 = (m2 * m2) * m;
    const float Fr = f0r + (1.0f - f0r) * m5, Fg = f0g + (1.0f - f0g) * m5, Fb = f0b + (1.0f - f0b) * m5;
    const float common = (D * G2) * FF_GLOSSY_RCP((4.0f * woz) * fmaxf(wiz, kGlossyMinCos));
    o.fr = Fr * common;
    o.fg = Fg * common;
    o.fb = Fb * common;
    o.pdf = (G1 * D) * FF_GLOSSY_RCP(4.0f * woz);
    const float g = one_lo * G2;
    o.wr = Fr * g;
    o.wg = Fg * g;
    o.wb = Fb * g;
    return o;
}

// sin and cos of 2 pi k24 / 2^24: the octant taken off the integer, fixed-order polynomials on [0, pi / 4] (cosine_sample's scheme)
FF_GLOSSY_HD void glossy_sincos_turn(unsigned k24, float& sn, float& cs)
{
    const unsigned oct = (k24 >> 21) & 7u, f = k24 & 0x1FFFFFu;
    const unsigned mm = (oct & 1u) ? (0x200000u - f) : f;
    const float a = (float)mm * 3.7450704e-07f; // 2 pi / 2^24
    const float a2 = a * a;
    float sp = -1.9841270e-04f + a2 * 2.7557319e-06f;
    sp = 8.3333333e-03f + a2 * sp;
    sp = -1.6666667e-01f + a2 * sp;
    const float s = a + (a * a2) * sp;
    float cp = -1.3888889e-03f + a2 * 2.4801587e-05f;
    cp = 4.1666667e-02f + a2 * cp;
    cp = -0.5f + a2 * cp;
    const float c = 1.0f + a2 * cp;
    if ((oct + 1u) & 2u) { sn = c; cs = s; } else { sn = s; cs = c; }
    if (oct >= 4u) sn = -sn;
    if (oct >= 2u && oct <= 5u) cs = -cs;
}

// Draws wi for wo (unit, wo.z >= kGlossyMinCos).  Returns the lobe at (wo, wi); a failed sample (wi.z <= 0) has weight and pdf 0.
FF_GLOSSY_HD GlossyLobe glossy_sample(float alpha, float f0r, float f0g, float f0b, float wox, float woy, float woz, unsigned k24, float u2, float& wix,
                                      float& wiy, float& wiz)
{
    const float vx0 = alpha * wox, vy0 = alpha * woy;
    const float vinv = FF_GLOSSY_RCP(FF_GLOSSY_SQRT(glossy_dot3(vx0, vy0, woz, vx0, vy0, woz)));
    const float vx = vx0 * vinv, vy = vy0 * vinv, vz = woz * vinv;
    const float z = (1.0f - u2) * (1.0f + vz) - vz;
    const float r = FF_GLOSSY_SQRT(fmaxf(0.f, 1.0f - z * z));
    float sn, cs;
    glossy_sincos_turn(k24, sn, cs);
    const float px = r * cs + vx, py = r * sn + vy, pz = z + vz;
    const float gx = alpha * px, gy = alpha * py, gz = fmaxf(pz, 0.f);
    const float len2 = glossy_dot3(gx, gy, gz, gx, gy, gz);
    if (!(len2 > 0.f)) { // h' = 0: the cap's one point opposite v
        wix = -wox;
        wiy = -woy;
        wiz = -woz;
        return glossy_eval(alpha, f0r, f0g, f0b, wox, woy, woz, wix, wiy, -1.0f);
    }
    const float ginv = FF_GLOSSY_RCP(FF_GLOSSY_SQRT(len2));
    const float hx = gx * ginv, hy = gy * ginv, hz = gz * ginv;
    const float k2 = 2.0f * glossy_dot3(wox, woy, woz, hx, hy, hz);
    wix = k2 * hx - wox;
    wiy = k2 * hy - woy;
    wiz = k2 * hz - woz;
    return glossy_eval(alpha, f0r, f0g, f0b, wox, woy, woz, wix, wiy, wiz);
}

} // namespace ff
