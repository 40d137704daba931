// ff_dof_api.cpp — host side of ff_depth_of_field (include/firefly/ff_api.h): the argument checks, the parameters of a thin lens
// (ff_dof_params_from_camera) and the entry points.  The use of the state's image work buffer, the staging of host buffers, the
// three launches (kernels in ff_dof.hip) and the loops of the host-only twin ff_depth_of_field_host are ff_tile_filter.h's, over
// ff_dof.h's per-pixel functions.  A pure image operation: no scene, no history, nothing kept in the state.
#include <cmath>

#include <hip/hip_runtime.h>

#include "ff_dof.h"
#include "ff_state.h"

using namespace ff;

namespace {

// What both entry points check, in this order: the camera and the parameter block, the size, the parameters, the camera's floats,
// the inputs, the outputs' places.  Fills the kernel arguments.
int check_dof(const FfCamera* camera, int width, int height, const FfDofParams* p, const float* radiance_in, const float* position, const float* depth,
              const void* rgb8, const float* radiance_out, DofArgs* a, const char* who)
{
    if (!camera) return fail(FF_ERR_INVALID_ARG, "%s: camera is null", who);
    if (!p) return fail(FF_ERR_INVALID_ARG, "%s: params are null", who);
    if (check_image_size(width, height, who) != FF_OK) return FF_ERR_INVALID_ARG;
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
    const size_t px = (size_t)width * (size_t)height;
    if (check_outputs_disjoint(rgb8, radiance_out, px, { { radiance_in, px * 12, "radiance_in" }, { position, px * 12, "position" }, { depth, px * 4, "depth" } }, who) != FF_OK)
        return FF_ERR_INVALID_ARG;
    a->grid = make_tile_grid(width, height, p->max_radius);
    a->g = p->grid;
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
    const int st = check_dof(camera, width, height, p, radiance_in, position, depth, rgb8, radiance_out, &a, "ff_depth_of_field");
    if (st != FF_OK) return st;
    return tile_filter_device<DofFilter>(s, a, radiance_in, position, depth, inputs_on_device, rgb8, rgb8_on_device, radiance_out, radiance_out_on_device,
                                         "ff_depth_of_field");
}

int ff_depth_of_field_host(const FfCamera* camera, int width, int height, const FfDofParams* p, const float* radiance_in, const float* position,
                           const float* depth, unsigned char* rgb8, float* radiance_out)
{
    clear_error();
    DofArgs a;
    const int st = check_dof(camera, width, height, p, radiance_in, position, depth, rgb8, radiance_out, &a, "ff_depth_of_field_host");
    if (st != FF_OK) return st;
    tile_filter_host<DofFilter>(a, radiance_in, position, depth, rgb8, radiance_out);
    return FF_OK;
}

} // extern "C"
