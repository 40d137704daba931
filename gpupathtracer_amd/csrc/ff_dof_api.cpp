// ff_dof_api.cpp — host side of ff_depth_of_field (include/firefly/ff_api.h): the argument checks, the work buffer and the staging of
// host buffers, the three launches (kernels in ff_dof.hip), the parameters of a thin lens (ff_dof_params_from_camera), and the
// host-only twin ff_depth_of_field_host, which runs ff_dof.h's per-pixel functions in loops.  A pure image operation: no scene, no
// history, nothing kept in the state but the work buffer.
#include <algorithm>
#include <cmath>
#include <vector>

#include <hip/hip_runtime.h>

#include "ff_dof.h"
#include "ff_state.h"

using namespace ff;

namespace {

struct Span {
    const void* ptr;
    size_t bytes;
    const char* name;
};

bool overlaps(const Span& a, const Span& b)
{
    const char* p = (const char*)a.ptr;
    const char* q = (const char*)b.ptr;
    return p < q + b.bytes && q < p + a.bytes;
}

// What both entry points check, in this order: the camera and the parameter block, the size, the parameters, the camera's floats,
// the inputs, the outputs' places.  Fills the kernel arguments.
int check_dof(const FfCamera* camera, int width, int height, const FfDofParams* p, const float* radiance_in, const float* position, const float* depth,
              const void* rgb8, const float* radiance_out, DofArgs* a, const char* who)
{
    if (!camera) return fail(FF_ERR_INVALID_ARG, "%s: camera is null", who);
    if (!p) return fail(FF_ERR_INVALID_ARG, "%s: params are null", who);
    if (width < 1 || height < 1 || width > 65535 || height > 65535) return fail(FF_ERR_INVALID_ARG, "%s: image size %dx%d is invalid", who, width, height);
    // (a focus_distance so small that its reciprocal overflows would turn coc_scale 0 into 0 * Inf)
    if (!(p->focus_distance > 0.f) || !std::isfinite(p->focus_distance) || !std::isfinite(1.f / p->focus_distance))
        return fail(FF_ERR_INVALID_ARG, "%s: focus_distance must be positive and finite, and so must 1 / focus_distance (got %g)", who, (double)p->focus_distance);
    if (!(p->coc_scale >= 0.f) || !std::isfinite(p->coc_scale))
        return fail(FF_ERR_INVALID_ARG, "%s: coc_scale must be >= 0 and finite (got %g)", who, (double)p->coc_scale);
    if (p->max_radius < 1 || p->max_radius > 64) return fail(FF_ERR_INVALID_ARG, "%s: max_radius must be 1 .. 64 (got %d)", who, p->max_radius);
    if (p->grid < 1 || p->grid > kDofMaxGrid) return fail(FF_ERR_INVALID_ARG, "%s: grid must be 1 .. %d (got %d)", who, kDofMaxGrid, p->grid);
    if (!(p->depth_extent > 0.f) || !std::isfinite(p->depth_extent))
        return fail(FF_ERR_INVALID_ARG, "%s: depth_extent must be positive and finite (got %g)", who, (double)p->depth_extent);
    if (p->flags != 0) return fail(FF_ERR_INVALID_ARG, "%s: unknown flags 0x%x", who, p->flags);
    if (p->reserved[0] != 0 || p->reserved[1] != 0) return fail(FF_ERR_INVALID_ARG, "%s: reserved must be 0", who);
    const float pos[3] = { camera->m_position.x, camera->m_position.y, camera->m_position.z };
    const float fwd[3] = { camera->m_forward.x, camera->m_forward.y, camera->m_forward.z };
    for (int c = 0; c < 3; ++c) {
        if (!std::isfinite(pos[c])) return fail(FF_ERR_INVALID_ARG, "%s: the camera's m_position is not finite", who);
        if (!std::isfinite(fwd[c])) return fail(FF_ERR_INVALID_ARG, "%s: the camera's m_forward is not finite", who);
    }
    if (!radiance_in) return fail(FF_ERR_INVALID_ARG, "%s: radiance_in is null", who);
    if (!position) return fail(FF_ERR_INVALID_ARG, "%s: position is null", who);
    if (!depth) return fail(FF_ERR_INVALID_ARG, "%s: depth is null", who);
    // the gather reads neighbours: no output may lie on an input, and the two outputs are written by different lanes
    const size_t px = (size_t)width * (size_t)height;
    const Span in[3] = { { radiance_in, px * 12, "radiance_in" }, { position, px * 12, "position" }, { depth, px * 4, "depth" } };
    const Span out[2] = { { rgb8, px * 3, "rgb8" }, { radiance_out, px * 12, "radiance_out" } };
    for (const Span& o : out)
        for (const Span& i : in)
            if (o.ptr && overlaps(o, i)) return fail(FF_ERR_INVALID_ARG, "%s: %s overlaps %s", who, o.name, i.name);
    if (rgb8 && radiance_out && overlaps(out[0], out[1])) return fail(FF_ERR_INVALID_ARG, "%s: rgb8 overlaps radiance_out", who);
    a->width = width;
    a->height = height;
    a->k = p->max_radius;
    a->g = p->grid;
    a->tiles_x = (width + a->k - 1) / a->k;
    a->tiles_y = (height + a->k - 1) / a->k;
    a->fi = 1.f / p->focus_distance;
    a->coc_scale = p->coc_scale;
    a->depth_extent = p->depth_extent;
    for (int c = 0; c < 3; ++c) {
        a->origin[c] = pos[c];
        a->forward[c] = fwd[c];
    }
    return FF_OK;
}

} // namespace

namespace ff {

void dof_release(FfState* s)
{
    if (s->d_dof_work) (void)hipFree(s->d_dof_work);
    s->d_dof_work = nullptr;
    s->dof_work_bytes = 0;
}

} // namespace ff

extern "C" {

void ff_dof_params_init(FfDofParams* p)
{
    if (!p) return;
    // 
    p->focus_distance = 1.f;
    p->coc_scale = 0.f;
    p->max_radius = 16;
    p->grid = 4;
    p->depth_extent = 0.1f;
    p->flags = 0;
    p->reserved[0] = p->reserved[1] = 0;
}

int ff_dof_params_from_camera(const FfCamera* camera, const FfCameraSampling* cs, FfDofParams* p)
{
    clear_error();
    if (!camera) return fail(FF_ERR_INVALID_ARG, "ff_dof_params_from_camera: camera is null");
    if (!cs) return fail(FF_ERR_INVALID_ARG, "ff_dof_params_from_camera: camera sampling is null");
    if (!p) return fail(FF_ERR_INVALID_ARG, "ff_dof_params_from_camera: params are null");
    const int st = check_camera_sampling(cs, "ff_dof_params_from_camera");
    if (st != FF_OK) return st;
    if (!std::isfinite(camera->m_fov) || !(camera->m_fov > 0.f && camera->m_fov < 180.f))
        return fail(FF_ERR_INVALID_ARG, "ff_dof_params_from_camera: m_fov must be in (0, 180) degrees (got %g)", (double)camera->m_fov);
    if (!std::isfinite(camera->m_screenHeight) || !(camera->m_screenHeight > 0.f))
        return fail(FF_ERR_INVALID_ARG, "ff_dof_params_from_camera: m_screenHeight must be positive and finite (got %g)", (double)camera->m_screenHeight);
    // a lens of radius R focused at z_f spreads a point at axial depth z over R (H / 2) / tan(fov / 2) |1 / z_f - 1 / z| pixels
    // (m_fov is perspectiveFovRH_NO's vertical field of view, pixels are square); in double, rounded once
    const double half_fov = (double)camera->m_fov * (3.14159265358979323846 / 180.0) * 0.5;
    const float scale = (float)((double)cs->lens_radius * 0.5 * (double)camera->m_screenHeight / std::tan(half_fov));
    if (!std::isfinite(scale)) return fail(FF_ERR_INVALID_ARG, "ff_dof_params_from_camera: coc_scale of this lens and camera is not finite");
    p->focus_distance = cs->focus_distance;
    p->coc_scale = scale;
    return FF_OK;
}

int ff_depth_of_field(FfState* s, const FfCamera* camera, int width, int height, const FfDofParams* p, const float* radiance_in, const float* position,
                      const float* depth, int inputs_on_device, void* rgb8, int rgb8_on_device, float* radiance_out, int radiance_out_on_device)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_depth_of_field: state is null");
    DofArgs a;
    int st = check_dof(camera, width, height, p, radiance_in, position, depth, rgb8, radiance_out, &a, "ff_depth_of_field");
    if (st != FF_OK) return st;
    FF_HIP(hipSetDevice(s->device));
    hipStream_t stream = s->stream;
    const size_t px = (size_t)width * (size_t)height, tiles = (size_t)a.tiles_x * (size_t)a.tiles_y;
    // the work buffer: the packed plane, T and N, then (from a multiple of 16 bytes on) the staging of host buffers
    const size_t plane_bytes = px * sizeof(float2), tile_bytes = tiles * sizeof(float);
    const size_t own_bytes = (plane_bytes + 2 * tile_bytes + 15) & ~(size_t)15;
    unsigned char* d_rgb8 = (unsigned char*)rgb8;
    float* d_out = radiance_out;
    Staging stage(&s->d_dof_work, &s->dof_work_bytes, own_bytes);
    if (!inputs_on_device) {
        stage.in(&radiance_in, radiance_in, px * 12);
        stage.in(&position, position, px * 12);
        stage.in(&depth, depth, px * 4);
    }
    if (rgb8 && !rgb8_on_device) stage.out(&d_rgb8, rgb8, px * 3);
    if (radiance_out && !radiance_out_on_device) stage.out(&d_out, radiance_out, px * 12);
    st = stage.commit(stream, "ff_depth_of_field: staging the inputs failed");
    if (st != FF_OK) return st;
    float2* plane = (float2*)s->d_dof_work;
    float* tile_max = (float*)(plane + px);
    float* neighbour_max = tile_max + tiles;
    FF_HIP(launch_dof_pack_tile_max(a, position, depth, plane, tile_max, stream));
    FF_HIP(launch_dof_neighbour_max(a, tile_max, neighbour_max, stream));
    if (d_rgb8 || d_out) FF_HIP(launch_dof_gather(a, plane, neighbour_max, radiance_in, d_rgb8, d_out, stream));
    FF_HIP(hipStreamSynchronize(stream));
    return stage.finish();
}

int ff_depth_of_field_host(const FfCamera* camera, int width, int height, const FfDofParams* p, const float* radiance_in, const float* position,
                           const float* depth, unsigned char* rgb8, float* radiance_out)
{
    clear_error();
    DofArgs a;
    const int st = check_dof(camera, width, height, p, radiance_in, position, depth, rgb8, radiance_out, &a, "ff_depth_of_field_host");
    if (st != FF_OK) return st;
    const size_t px = (size_t)width * (size_t)height, tiles = (size_t)a.tiles_x * (size_t)a.tiles_y;
    std::vector<float2> plane(px);
    std::vector<float> tile_max(tiles), neighbour_max(tiles);
    // steps 1 and 2
    for (int ty = 0; ty < a.tiles_y; ++ty)
        for (int tx = 0; tx < a.tiles_x; ++tx) {
            const int x0 = tx * a.k, y0 = ty * a.k;
            const int tw = std::min(a.k, width - x0), th = std::min(a.k, height - y0);
            float best = 0.f;
            for (int i = 0; i < tw * th; ++i) {
                const size_t q = (size_t)(y0 + i / tw) * (size_t)width + (size_t)(x0 + i % tw);
                const float2 v = dof_pack(a, position[3 * q], position[3 * q + 1], position[3 * q + 2], depth[q]);
                plane[q] = v;
                best = v.x > best ? v.x : best;
            }
            tile_max[(size_t)ty * (size_t)a.tiles_x + (size_t)tx] = best;
        }
    for (int ty = 0; ty < a.tiles_y; ++ty)
        for (int tx = 0; tx < a.tiles_x; ++tx) neighbour_max[(size_t)ty * (size_t)a.tiles_x + (size_t)tx] = dof_neighbour_max(a, tile_max.data(), tx, ty);
    signed char dxs[kDofColumns];
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t i = (size_t)y * (size_t)width + (size_t)x;
            float v[3];
            dof_gather(a, x, y, plane.data(), radiance_in, neighbour_max[(size_t)(y / a.k) * (size_t)a.tiles_x + (size_t)(x / a.k)], dxs, 1, v);
            if (radiance_out) { radiance_out[3 * i] = v[0]; radiance_out[3 * i + 1] = v[1]; radiance_out[3 * i + 2] = v[2]; }
            if (rgb8) { rgb8[3 * i] = dof_u8(v[0]); rgb8[3 * i + 1] = dof_u8(v[1]); rgb8[3 * i + 2] = dof_u8(v[2]); }
        }
    return FF_OK;
}

} // extern "C"
