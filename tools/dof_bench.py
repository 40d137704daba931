"""ff_depth_of_field timings on device buffers, with ff_motion_blur, ff_taa and ff_display as the same-run yardsticks, and what the
filter buys.

At the given size (default 1080p), in one process, ff_depth_of_field over --repeats windows of --reps calls, each after warm-up, timed
with device events around each window (median and spread of the windows reported; every call is synchronous, so the figure holds the
call's launches and wait, as a viewer pays it) and with the host clock per call (median): (a) everything in focus (coc_scale 0 on
the C2 G-buffer: the copy-through path), (b) the C2 G-buffer under the lens of the quality measurement (radius 0.08, focused on the
back wall, parameters from ff_dof_params_from_camera, defaults k 16, g 4), (c) every pixel at the full radius l = k = 16 for
g = 2, 4 and 8 (13, 49 and 197 grid points).  Beside them ff_motion_blur at rest and at its uniform worst case, ff_taa along
tools/taa_bench.py's sliding camera and ff_display (defaults), timed the same way.  Compulsory bytes per pixel: 16 read by the pack
pass and 8 written, 12 + 4 (N, from cache) read by the gather and 15 written: 55 B in focus.

Quality, at 480x270 on the C2 pose, NEE, 8 bounces: a thin-lens frame of 4096 spp (radius 0.08, focused on the back wall) as the
truth; against it (1) the 1-spp pipeline: a pinhole frame through ff_denoise, then ff_depth_of_field, beside the denoised frame
unfiltered; (2) a 64-spp pinhole frame filtered and unfiltered.  MSE of each and the ratios.  Prints human-readable lines, then one
JSON line.  The per-kernel split comes from a separate run under `rocprofv3 --kernel-trace --stats` with --no-quality.

    python tools/dof_bench.py [--width 1920 --height 1080 --reps 200 --warmup 20 --repeats 7]
"""
import argparse
import json
import os
import sys
import time

import torch  # (before the library: one HIP runtime per process, see tests/conftest.py)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpupathtracer_amd import lib, scenes  # noqa: E402
from gpupathtracer_amd import types as T  # noqa: E402

HBM_COPY_BYTES_PER_S = 6.29e12
LENS = dict(lens_radius=0.08, focus_distance=4.9)  # focused on the back wall of the C2 pose


def timed(fn, reps, warmup, repeats, before=None):
    """`repeats` windows of `reps` calls, each after `warmup` calls (before(): run ahead of every window) -> {event_ms: the median
    over the windows of device-event ms per call, event_ms_min / _max: the spread of the windows, host_median_ms: median host ms
    per call over all windows}."""
    windows, host = [], []
    for _ in range(repeats):
        if before:
            before()
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record()
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            host.append((time.perf_counter() - t0) * 1e3)
        end.record()
        torch.cuda.synchronize()
        windows.append(begin.elapsed_time(end) / reps)
    return {"event_ms": round(float(np.median(windows)), 5), "event_ms_min": round(min(windows), 5), "event_ms_max": round(max(windows), 5),
            "host_median_ms": round(float(np.median(host)), 5)}


def c2(w, h, x=0.0):
    return scenes.posed_camera(w, h, position=(x, 0.0, 2.4), yaw=-90.0, pitch=0.0)


def world_step(px, cam):
    """The camera slide that moves the back wall (4.9 away) by px pixels."""
    return px * 2 * 4.9 * np.tan(np.radians(cam.m_fov) / 2) / cam.m_screenHeight


def quality(t, w=480, h=270, truth_spp=4096):
    nee = T.SHADE_DIFFUSE_PATH_NEE
    cam = c2(w, h)
    cs = lib.camera_sampling(T.PIXEL_CORNER, **LENS)
    p = lib.dof_params_from_camera(cam, cs)
    try:
        t.set_camera_sampling(cs)
        truth = t.render(cam, lib.render_params(w, h, 8, truth_spp, 77, shade_mode=nee))[1].astype(np.float64)
    finally:
        t.set_camera_sampling(None)
    gb = t.gbuffer(cam, lib.render_params(w, h))
    mse = lambda a: float(np.mean((a.astype(np.float64) - truth) ** 2))  # noqa: E731
    res = {"lens": LENS, "truth_spp": truth_spp, "coc_scale": round(float(p.coc_scale), 4)}
    one = t.denoise(t.render(cam, lib.render_params(w, h, 8, 1, 4321, shade_mode=nee))[1], gb)[1]
    many = t.render(cam, lib.render_params(w, h, 8, 64, 4322, shade_mode=nee))[1]
    for name, frame in (("1spp_denoised", one), ("64spp", many)):
        out = t.depth_of_field(frame, gb, cam, p)[1]
        res[name] = {"mse_filtered": mse(out), "mse_unfiltered": mse(frame), "ratio": round(mse(out) / mse(frame), 4)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7, help="timed windows of --reps calls per case; the median and the spread are reported")
    ap.add_argument("--no-quality", action="store_true", help="skip the 480x270 MSE measurement")
    ap.add_argument("--no-taa", action="store_true", help="skip the ff_taa yardstick (it stores reps + warmup frames of inputs on the device)")
    args = ap.parse_args()
    W, H = args.width, args.height
    px = W * H
    res = {"scene": "cornell_wahoo C2 pose", "width": W, "height": H, "reps": args.reps, "repeats": args.repeats}
    with lib.Tracer(0) as t:
        t.set_stream(torch.cuda.current_stream().cuda_stream)
        t.upload_scene(scenes.cornell_wahoo_scene())
        dev = torch.device("cuda")
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
        rad, out, pos, depth, motion = f32(H, W, 3), f32(H, W, 3), f32(H, W, 3), f32(H, W), f32(H, W, 2)
        ids = torch.zeros((H, W, 3), dtype=torch.int32, device=dev)
        rgb8 = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
        flat = lib.render_params(W, H)
        cam = c2(W, H)
        t.gbuffer_device(cam, flat, depth.data_ptr(), pos.data_ptr(), None, None, ids.data_ptr())
        t.render_device(cam, lib.render_params(W, H, 8, 1, 1234), None, rad.data_ptr())
        torch.cuda.synchronize()

        def dof(q):
            t.depth_of_field_device(cam, W, H, rad.data_ptr(), pos.data_ptr(), depth.data_ptr(), q, rgb8.data_ptr(), out.data_ptr())

        def radii(q):
            """Step 1 on the device buffers, for the case's description only."""
            fwd = torch.tensor([cam.m_forward.x, cam.m_forward.y, cam.m_forward.z], device=dev)
            org = torch.tensor([cam.m_position.x, cam.m_position.y, cam.m_position.z], device=dev)
            z = ((pos - org) * fwd).sum(-1)
            hit = (depth > 0) & (z > 1e-6)
            iz = torch.where(hit, 1.0 / torch.where(hit, z, torch.ones_like(z)), torch.zeros_like(z))
            return (q.coc_scale * (1.0 / q.focus_distance - iz).abs()).clamp(max=float(q.max_radius))

        def case(name, q, nbytes=None):
            res[name] = timed(lambda: dof(q), args.reps, args.warmup, args.repeats)
            l = radii(q)
            res[name].update(params={f: getattr(q, f) for f in ("focus_distance", "coc_scale", "max_radius", "grid")},
                             share_of_pixels_with_l_over_half=round(float((l > 0.5).float().mean()), 4), largest_l_px=round(float(l.max()), 2),
                             mean_l_px=round(float(l.mean()), 2))
            if nbytes:
                res[name].update(bytes=nbytes, share_of_copy_rate=round(nbytes / (res[name]["event_ms"] * 1e-3) / HBM_COPY_BYTES_PER_S, 3))

        # (a) everything in focus, (b) the C2 G-buffer under the lens
        case("a_in_focus", lib.dof_params(focus_distance=LENS["focus_distance"], coc_scale=0.0), 55 * px)
        case("b_c2_lens", lib.dof_params_from_camera(cam, lib.camera_sampling(T.PIXEL_CORNER, **LENS)))
        # (c) every pixel at l = k: a wall half a unit in front of the camera, focus 2
        near = pos.clone()
        pos[...] = torch.tensor([cam.m_position.x, cam.m_position.y, cam.m_position.z], device=dev) + 0.5 * torch.tensor(
            [cam.m_forward.x, cam.m_forward.y, cam.m_forward.z], device=dev)
        depth_kept = depth.clone()
        depth[...] = 0.5
        torch.cuda.synchronize()
        for g in (2, 4, 8):
            case(f"c_full_radius_g{g}", lib.dof_params(focus_distance=2.0, coc_scale=20.0, max_radius=16, grid=g))
        pos.copy_(near)
        depth.copy_(depth_kept)
        del near, depth_kept
        # the yardsticks: ff_motion_blur (at rest and its uniform worst case), ff_display (defaults), ff_taa along the sliding camera
        mp = lib.motion_blur_params()

        def blur():
            t.motion_blur_device(W, H, rad.data_ptr(), motion.data_ptr(), depth.data_ptr(), mp, rgb8.data_ptr(), out.data_ptr())
        res["motion_blur_at_rest"] = timed(blur, args.reps, args.warmup, args.repeats)
        motion[..., 0] = 2.0 * mp.max_radius / mp.shutter
        torch.cuda.synchronize()
        res["motion_blur_worst_case"] = timed(blur, args.reps, args.warmup, args.repeats)
        dp = lib.display_params()
        res["display_defaults"] = timed(lambda: t.display_device(W, H, rad.data_ptr(), dp, rgb8.data_ptr(), None), args.reps, args.warmup, args.repeats)
        if not args.no_taa:
            tp = lib.taa_params()
            n = args.reps + args.warmup
            poses = [c2(W, H, world_step(2.0, cam) * j) for j in range(n)]
            frames = []
            for j, pose in enumerate(poses):
                t.set_pixel_jitter(*lib.jitter_sequence(j, 16))
                t.gbuffer_device(pose, flat, None, pos.data_ptr(), None, None, ids.data_ptr())
                t.render_device(pose, lib.render_params(W, H, 8, 1, 1234 + j), None, rad.data_ptr())
                torch.cuda.synchronize()
                frames.append([x.clone() for x in (rad, pos, ids)])
            t.set_pixel_jitter(0.0, 0.0)
            k = [-1]

            def restart():
                t.taa_reset()
                k[0] = -1

            def taa():
                k[0] += 1
                r_, p_, i_ = frames[k[0]]
                t.taa_device(poses[k[0]], W, H, r_.data_ptr(), p_.data_ptr(), i_.data_ptr(), tp, rgb8.data_ptr(), out.data_ptr())
            res["taa"] = timed(taa, args.reps, args.warmup, args.repeats, before=restart)
            del frames
        for name in [key for key in res if key[:2] in ("a_", "b_", "c_")]:
            res[name]["over_motion_blur_worst_case"] = round(res[name]["event_ms"] / res["motion_blur_worst_case"]["event_ms"], 3)
            if "taa" in res:
                res[name]["over_taa"] = round(res[name]["event_ms"] / res["taa"]["event_ms"], 3)
        if not args.no_quality:
            res["quality_480x270"] = quality(t)
    for key, val in res.items():
        print(f"{key:24s} {val}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
