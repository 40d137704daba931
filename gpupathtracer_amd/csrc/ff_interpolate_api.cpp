// ff_interpolate_api.cpp — host side of ff_interpolate (include/firefly/ff_api.h): the argument checks, what is prepared in double on
// the host (the cameras' inverse ray matrices, the pixel size, the geometry table), its use of the state's image work buffer (the five
// counts, the {rgb, state} work image, then the staging of host buffers through ff_image.h's helpers), the two launches (kernels in
// ff_interpolate.hip), the loops of the host-only twin ff_interpolate_host over ff_interpolate.h's per-pixel functions, and
// ff_interpolate_geometry_maps.  A pure image operation: no scene, no history, nothing kept in the state.
#include <cmath>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>

#include "ff_interpolate.h"
#include "ff_state.h"

using namespace ff;

namespace {

constexpr size_t kCountBytes = 32; // the five counts at the head of the work buffer; the work image follows

const float kIdentityMap[12] = { 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f };

// The caller's buffers of one call.
struct InterpBuffers {
    const FfCamera* camera[3];   // mid, A, B
    const float* position[3];
    const int32_t* ids[3];
    const float* radiance[2];    // A, B
};

// What both entry points check, in this order: the parameter block, the size, the parameters, the required pointers, the geometry
// table, the outputs' places, the cameras.  Fills the kernel arguments (but for the device pointers) and the geometry table.
int check_interpolate(int width, int height, const FfInterpolateParams* p, const InterpBuffers& b, const float* geom_maps, int num_geometries,
                      const void* rgb8, const float* radiance_out, InterpArgs* a, std::vector<InterpMap>* table, const char* who)
{
    static const char* const kName[3] = { "mid", "a", "b" };
    if (!p) return fail(FF_ERR_INVALID_ARG, "%s: params are null", who);
    if (check_image_size(width, height, who) != FF_OK) return FF_ERR_INVALID_ARG;
    if (!(p->t >= 0.f && p->t <= 1.f)) return fail(FF_ERR_INVALID_ARG, "%s: t must be 0 .. 1 (got %g)", who, (double)p->t); // (false for NaN)
    if (!(p->surface_tolerance > 0.f) || !std::isfinite(p->surface_tolerance))
        return fail(FF_ERR_INVALID_ARG, "%s: surface_tolerance must be positive and finite (got %g)", who, (double)p->surface_tolerance);
    if (p->fill_radius < 0 || p->fill_radius > kInterpMaxFill)
        return fail(FF_ERR_INVALID_ARG, "%s: fill_radius must be 0 .. %d (got %d)", who, kInterpMaxFill, p->fill_radius);
    if (p->flags != 0) return fail(FF_ERR_INVALID_ARG, "%s: unknown flags 0x%x", who, (unsigned)p->flags);
    if (p->reserved != 0) return fail(FF_ERR_INVALID_ARG, "%s: reserved must be 0", who);
    for (int i = 0; i < 3; ++i) {
        if (!b.camera[i]) return fail(FF_ERR_INVALID_ARG, "%s: camera_%s is null", who, kName[i]);
        if (!b.position[i]) return fail(FF_ERR_INVALID_ARG, "%s: position%s%s is null", who, i ? "_" : "", i ? kName[i] : "");
        if (!b.ids[i]) return fail(FF_ERR_INVALID_ARG, "%s: ids%s%s is null", who, i ? "_" : "", i ? kName[i] : "");
        if (i && !b.radiance[i - 1]) return fail(FF_ERR_INVALID_ARG, "%s: radiance_%s is null", who, kName[i]);
    }
    if (geom_maps && num_geometries <= 0) return fail(FF_ERR_INVALID_ARG, "%s: geom_maps given with num_geometries %d", who, num_geometries);
    const size_t px = (size_t)width * (size_t)height;
    if (check_outputs_disjoint(rgb8, radiance_out, px,
                               { { b.position[0], px * 12, "position" },   { b.ids[0], px * 12, "ids" },
                                 { b.radiance[0], px * 12, "radiance_a" }, { b.position[1], px * 12, "position_a" },
                                 { b.ids[1], px * 12, "ids_a" },           { b.radiance[1], px * 12, "radiance_b" },
                                 { b.position[2], px * 12, "position_b" }, { b.ids[2], px * 12, "ids_b" } },
                               who) != FF_OK)
        return FF_ERR_INVALID_ARG;

    a->width = width;
    a->height = height;
    a->t = p->t;
    a->tol2 = p->surface_tolerance * p->surface_tolerance;
    a->fill_radius = p->fill_radius;
    a->num_geoms = geom_maps ? num_geometries : 0;
    a->maps = nullptr;
    FfMat4 ray;
    if (!inverse_ray_matrix(b.camera[0], a->inv_mid, &ray)) return fail(FF_ERR_INVALID_ARG, "%s: camera_mid's ray matrix is singular", who);
    std::memcpy(a->ray, ray.m, sizeof a->ray);
    a->far_clip = b.camera[0]->m_farClip;
    a->sw = b.camera[0]->m_screenWidth;
    a->sh = b.camera[0]->m_screenHeight;
    for (int S = 0; S < 2; ++S) {
        const FfCamera* c = b.camera[S + 1];
        InterpSource& s = a->src[S];
        FfMat4 unused;
        if (!inverse_ray_matrix(c, s.inv, &unused)) return fail(FF_ERR_INVALID_ARG, "%s: camera_%s's ray matrix is singular", who, kName[S + 1]);
        s.sw = c->m_screenWidth;
        s.sh = c->m_screenHeight;
        s.eye[0] = c->m_position.x;
        s.eye[1] = c->m_position.y;
        s.eye[2] = c->m_position.z;
        s.pix = (float)(2.0 * std::tan((double)c->m_fov * (3.14159265358979323846 / 180.0) * 0.5) / (double)c->m_screenHeight);
        s.cam_rest = std::memcmp(c, b.camera[0], sizeof(FfCamera)) == 0 ? 1 : 0;
    }
    table->clear();
    if (geom_maps) {
        table->resize((size_t)num_geometries * 2);
        for (size_t i = 0; i < table->size(); ++i) {
            const float* m = geom_maps + 12 * i;
            InterpMap& row = (*table)[i];
            for (int r = 0; r < 3; ++r) row.a[r] = make_float4(m[4 * r], m[4 * r + 1], m[4 * r + 2], m[4 * r + 3]);
            row.identity = std::memcmp(m, kIdentityMap, sizeof kIdentityMap) == 0 ? 1 : 0;
            row.pad[0] = row.pad[1] = row.pad[2] = 0;
        }
    }
    return FF_OK;
}

void set_buffers(InterpArgs* a, const InterpBuffers& b)
{
    a->position = b.position[0];
    a->ids = b.ids[0];
    for (int S = 0; S < 2; ++S) {
        a->src[S].radiance = b.radiance[S];
        a->src[S].position = b.position[S + 1];
        a->src[S].ids = b.ids[S + 1];
    }
}

} // namespace

extern "C" {

void ff_interpolate_params_init(FfInterpolateParams* p)
{
    if (!p) return;
    // 
    p->t = 0.5f;
    p->surface_tolerance = 4.f;
    p->fill_radius = 4;
    p->flags = 0;
    p->reserved = 0;
}

int ff_interpolate(FfState* s, int width, int height, const FfInterpolateParams* p, const FfCamera* camera_mid, const float* position, const int32_t* ids,
                   const FfCamera* camera_a, const float* radiance_a, const float* position_a, const int32_t* ids_a, const FfCamera* camera_b,
                   const float* radiance_b, const float* position_b, const int32_t* ids_b, const float* geom_maps, int num_geometries, int inputs_on_device,
                   void* rgb8, int rgb8_on_device, float* radiance_out, int radiance_out_on_device, uint32_t* counts)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_interpolate: state is null");
    InterpBuffers b = { { camera_mid, camera_a, camera_b }, { position, position_a, position_b }, { ids, ids_a, ids_b }, { radiance_a, radiance_b } };
    InterpArgs a;
    std::vector<InterpMap> table;
    const int st = check_interpolate(width, height, p, b, geom_maps, num_geometries, rgb8, radiance_out, &a, &table, "ff_interpolate");
    if (st != FF_OK) return st;
    FF_HIP(hipSetDevice(s->device));
    hipStream_t stream = s->stream;
    const size_t px = (size_t)width * (size_t)height;
    Staging stage(&s->d_img_work, &s->img_work_bytes, kCountBytes + px * sizeof(float4));
    if (!table.empty()) stage.in(&a.maps, table.data(), table.size() * sizeof(InterpMap));
    if (!inputs_on_device) {
        for (int i = 0; i < 3; ++i) {
            stage.in(&b.position[i], b.position[i], px * 12);
            stage.in(&b.ids[i], b.ids[i], px * 12);
        }
        for (int S = 0; S < 2; ++S) stage.in(&b.radiance[S], b.radiance[S], px * 12);
    }
    StagedOutputs out(stage, px, rgb8, rgb8_on_device, radiance_out, radiance_out_on_device);
    const int staged = stage.commit(stream, "ff_interpolate: staging the inputs failed");
    if (staged != FF_OK) return staged;
    set_buffers(&a, b);
    uint32_t* d_count = (uint32_t*)s->d_img_work;
    float4* d_work = (float4*)((char*)s->d_img_work + kCountBytes);
    FF_HIP(hipMemsetAsync(d_count, 0, kCountBytes, stream));
    FF_HIP(launch_interpolate(a, d_work, out.rgb8, out.radiance, d_count, stream));
    FF_HIP(hipStreamSynchronize(stream));
    if (counts) FF_HIP(hipMemcpy(counts, d_count, 5 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return stage.finish();
}

int ff_interpolate_host(int width, int height, const FfInterpolateParams* p, const FfCamera* camera_mid, const float* position, const int32_t* ids,
                        const FfCamera* camera_a, const float* radiance_a, const float* position_a, const int32_t* ids_a, const FfCamera* camera_b,
                        const float* radiance_b, const float* position_b, const int32_t* ids_b, const float* geom_maps, int num_geometries,
                        unsigned char* rgb8, float* radiance_out, uint32_t* counts)
{
    clear_error();
    const InterpBuffers b = { { camera_mid, camera_a, camera_b }, { position, position_a, position_b }, { ids, ids_a, ids_b }, { radiance_a, radiance_b } };
    InterpArgs a;
    std::vector<InterpMap> table;
    const int st = check_interpolate(width, height, p, b, geom_maps, num_geometries, rgb8, radiance_out, &a, &table, "ff_interpolate_host");
    if (st != FF_OK) return st;
    set_buffers(&a, b);
    a.maps = table.empty() ? nullptr : table.data();
    const size_t px = (size_t)width * (size_t)height;
    std::vector<float4> work(px);
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) work[(size_t)y * (size_t)width + (size_t)x] = interp_gather(a, x, y);
    uint32_t n[5] = { 0, 0, 0, 0, 0 };
    const int r = a.fill_radius;
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t i = (size_t)y * (size_t)width + (size_t)x;
            float v[3] = { work[i].x, work[i].y, work[i].z };
            int state = (int)work[i].w;
            if (work[i].w == kInterpHole) {
                UpscaleMean m;
                for (int dy = -r; dy <= r; ++dy)
                    for (int dx = -r; dx <= r; ++dx) {
                        const int qx = x + dx, qy = y + dy;
                        if (qx < 0 || qy < 0 || qx >= width || qy >= height) continue;
                        const size_t q = (size_t)qy * (size_t)width + (size_t)qx;
                        if (work[q].w == kInterpHole || ids[3 * q] != ids[3 * i] || ids[3 * q + 2] != ids[3 * i + 2]) continue;
                        m.add(interp_fill_weight(dx, dy), work[q].x, work[q].y, work[q].z);
                    }
                if (m.n > 0) {
                    m.get(v);
                    state = kInterpFilled;
                } else {
                    interp_fallback(a, i, v);
                    state = kInterpFallback;
                }
            }
            ++n[state];
            store_rgb(i, v, rgb8, radiance_out);
        }
    if (counts) std::memcpy(counts, n, sizeof n);
    return FF_OK;
}

int ff_interpolate_geometry_maps(const FfGeometry* mid, const FfGeometry* a, const FfGeometry* b, int n, float* out, int32_t* out_identity_flags)
{
    clear_error();
    if (!mid || !a || !b || !out) return fail(FF_ERR_INVALID_ARG, "ff_interpolate_geometry_maps: %s is null", !mid ? "mid" : (!a ? "a" : (!b ? "b" : "out")));
    if (n <= 0) return fail(FF_ERR_INVALID_ARG, "ff_interpolate_geometry_maps: n must be positive (got %d)", n);
    for (int g = 0; g < n; ++g) {
        double m[16], inv[16];
        for (int k = 0; k < 16; ++k) m[k] = mid[g].m_modelMatrix.m[k];
        bool inverted = false;
        for (int S = 0; S < 2; ++S) {
            const FfGeometry& src = (S == 0 ? a : b)[g];
            float* o = out + 12 * (2 * (size_t)g + S);
            const bool same = std::memcmp(src.m_modelMatrix.m, mid[g].m_modelMatrix.m, sizeof(FfMat4)) == 0;
            if (out_identity_flags) out_identity_flags[2 * (size_t)g + S] = same ? 1 : 0;
            if (same) {
                std::memcpy(o, kIdentityMap, sizeof kIdentityMap);
                continue;
            }
            if (!inverted && !invert4(m, inv)) return fail(FF_ERR_INVALID_ARG, "ff_interpolate_geometry_maps: geometry %d's model matrix at mid is singular", g);
            inverted = true;
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 4; ++c) {
                    double v = 0.0;
                    for (int k = 0; k < 4; ++k) v += (double)src.m_modelMatrix.m[k * 4 + r] * inv[c * 4 + k];
                    o[4 * r + c] = (float)v;
                }
        }
    }
    return FF_OK;
}

} // extern "C"
