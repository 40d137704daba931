// ff_camera.cpp — per-sample camera rays (include/firefly/ff_api.h): the state's setting and the host twin of the kernel's camera ray
// (ff_camera_sample_rays: ff_camera.h's inline functions compiled for the host).
#include <cmath>
#include <cstring>

#include <hip/hip_runtime.h>

#include "ff_state.h"
#include "ff_camera.h"

using namespace ff;

namespace ff {

int check_camera_sampling(const FfCameraSampling* cs, const char* who)
{
    if (cs->pixel_filter != FF_PIXEL_CORNER && cs->pixel_filter != FF_PIXEL_BOX)
        return fail(FF_ERR_INVALID_ARG, "%s: pixel_filter %d is neither FF_PIXEL_CORNER nor FF_PIXEL_BOX", who, (int)cs->pixel_filter);
    if (!std::isfinite(cs->lens_radius) || cs->lens_radius < 0.f)
        return fail(FF_ERR_INVALID_ARG, "%s: lens_radius %g is not a finite number >= 0", who, (double)cs->lens_radius);
    if (!std::isfinite(cs->focus_distance)) return fail(FF_ERR_INVALID_ARG, "%s: focus_distance %g is not finite", who, (double)cs->focus_distance);
    if (cs->lens_radius > 0.f && !(cs->focus_distance > 0.f))
        return fail(FF_ERR_INVALID_ARG, "%s: focus_distance %g must be > 0 while lens_radius > 0", who, (double)cs->focus_distance);
    if (cs->reserved != 0) return fail(FF_ERR_INVALID_ARG, "%s: reserved must be 0 (got %d)", who, (int)cs->reserved);
    return FF_OK;
}

} // namespace ff

extern "C" {

void ff_camera_sampling_init(FfCameraSampling* cs)
{
    if (!cs) return;
    cs->pixel_filter = FF_PIXEL_CORNER;
    cs->lens_radius = 0.f;
    cs->focus_distance = 1.f;
    cs->reserved = 0;
}

int ff_set_camera_sampling(FfState* s, const FfCameraSampling* cs)
{
    clear_error();
    if (!s) return fail(FF_ERR_INVALID_ARG, "ff_set_camera_sampling: state is null");
    FfCameraSampling v;
    ff_camera_sampling_init(&v);
    if (cs) {
        const int st = check_camera_sampling(cs, "ff_set_camera_sampling");
        if (st != FF_OK) return st;
        v = *cs;
    }
    // (the mega-kernels' stored hits belong to the pinhole camera and stay valid: frames under an active setting never touch them)
    s->cam_sampling = v;
    return FF_OK;
}

int ff_camera_sample_rays(const FfCamera* camera, const FfCameraSampling* cs, float jitter_x, float jitter_y, int width, uint64_t seed, const int* xs,
                          const int* ys, const int* samples, int n, float* out_origins3, float* out_directions3)
{
    clear_error();
    if (!camera) return fail(FF_ERR_INVALID_ARG, "ff_camera_sample_rays: camera is null");
    FfCameraSampling v;
    ff_camera_sampling_init(&v);
    if (cs) {
        const int st = check_camera_sampling(cs, "ff_camera_sample_rays");
        if (st != FF_OK) return st;
        v = *cs;
    }
    if (!(jitter_x >= 0.f && jitter_x < 1.f && jitter_y >= 0.f && jitter_y < 1.f))
        return fail(FF_ERR_INVALID_ARG, "ff_camera_sample_rays: the jitter must be finite and in [0, 1) (got %g %g)", (double)jitter_x, (double)jitter_y);
    if (width < 1) return fail(FF_ERR_INVALID_ARG, "ff_camera_sample_rays: width must be at least 1 (got %d)", width);
    if (n < 0) return fail(FF_ERR_INVALID_ARG, "ff_camera_sample_rays: n must not be negative (got %d)", n);
    if (n > 0 && (!xs || !ys || !samples || !out_origins3 || !out_directions3))
        return fail(FF_ERR_INVALID_ARG, "ff_camera_sample_rays: null pixel, sample or output array");
    // the frame's camera as render_enqueue hands it to the kernel: the jittered matrix, or the unjittered one under FF_PIXEL_BOX
    FfMat4 cm;
    if (v.pixel_filter == FF_PIXEL_BOX) ff_camera_ray_matrix(camera, &cm);
    else ff_camera_ray_matrix_jittered(camera, jitter_x, jitter_y, &cm);
    const float pos[3] = { camera->m_position.x, camera->m_position.y, camera->m_position.z };
    const float fwd[3] = { camera->m_forward.x, camera->m_forward.y, camera->m_forward.z };
    const float right[3] = { camera->m_right.x, camera->m_right.y, camera->m_right.z };
    const float up[3] = { camera->m_up.x, camera->m_up.y, camera->m_up.z };
    const CameraRays C = { &cm.m[0], &cm.m[4], &cm.m[8], &cm.m[12], pos, camera->m_farClip, camera->m_screenWidth, camera->m_screenHeight,
                           v.pixel_filter == FF_PIXEL_BOX ? 1 : 0, v.lens_radius, v.focus_distance, fwd, right, up };
    const unsigned key = (unsigned)seed ^ (unsigned)(seed >> 32);
    for (int i = 0; i < n; ++i) {
        if (xs[i] < 0 || ys[i] < 0 || xs[i] > 0xFFFF || ys[i] > 0xFFFF || samples[i] < 0)
            return fail(FF_ERR_INVALID_ARG, "ff_camera_sample_rays: entry %d (pixel %d %d, sample %d) is out of range", i, xs[i], ys[i], samples[i]);
        float* o = out_origins3 + 3 * (size_t)i;
        float* d = out_directions3 + 3 * (size_t)i;
        camera_sample_ray(C, xs[i], ys[i], (unsigned)ys[i] * (unsigned)width + (unsigned)xs[i], (unsigned)samples[i], key, o[0], o[1], o[2], d[0], d[1], d[2]);
    }
    return FF_OK;
}

} // extern "C"
