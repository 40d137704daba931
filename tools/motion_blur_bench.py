"""ff_motion_blur timings on device buffers, with ff_taa and ff_display as the same-run yardsticks, and what the blur buys.

At the given size (default 1080p), in one process, ff_motion_blur with its default parameters over --repeats windows of --reps calls, each after warm-up, timed
with device events around each window (median and spread of the windows reported) (every call is synchronous, so the figure holds the call's launches and wait, as a
viewer pays it) and with the host clock per call (median): (a) a camera at rest (motion 0: the copy-through path), (b) the sliding C2
camera of tools/taa_bench.py (--slide-px per call at the back wall, default 2; the motion is ff_taa_history's, the depth
ff_gbuffer's, the input ff_taa's output), (c) the same slide at 16 px per call, (d) uniform worst-case motion: every pixel at
l = max_radius.  Beside them ff_taa along the sliding camera and ff_display (defaults), timed the same way.  Compulsory bytes per
pixel: 12 read by the pack pass and 16 written, 12 + 16 (N, from cache) read by the gather and 15 written: 55 B at rest.

Quality, at 320x180: a 64-spp frame of the sliding camera (8 px per frame, shutter 1) blurred with the motion ff_taa_history
reports, and the same frame unblurred, against the mean of 32 sub-frame renders across the shutter interval (camera positions spread
over the half frame interval either side of the frame's own); MSE of each and the ratio.  Prints human-readable lines, then one JSON
line.  The per-kernel split comes from a separate run under `rocprofv3 --kernel-trace --stats` with --no-quality.

    python tools/motion_blur_bench.py [--width 1920 --height 1080 --reps 200 --warmup 20 --repeats 7]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch  # (before the library: one HIP runtime per process, see tests/conftest.py)
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpupathtracer_amd import lib, scenes  # noqa: E402

HBM_COPY_BYTES_PER_S = 6.29e12


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


def world_step(px, h):
    """The camera slide that moves the back wall (4.9 away) by px pixels of an image h high."""
    return px * 2 * 4.9 * np.tan(np.radians(22.5)) / h


def quality(t, w=320, h=180, slide_px=8.0, subframes=32, spp=64):
    step = world_step(slide_px, h)
    prev, cur = c2(w, h, 0.0), c2(w, h, step)
    flat = lib.render_params(w, h)
    frame = lib.render_params(w, h, 8, spp, 4321)
    t.taa_reset()
    t.taa(t.render(prev, frame)[1], t.gbuffer(prev, flat), prev)
    gb = t.gbuffer(cur, flat)
    rad = t.render(cur, frame)[1]
    t.taa(rad, gb, cur)
    motion = t.taa_history()[0]
    p = lib.motion_blur_params(shutter=1.0)
    blurred = t.motion_blur(rad, motion, gb["depth"], p)[1]
    truth = np.zeros((h, w, 3))
    for i in range(subframes):
        x = step + ((i + 0.5) / subframes - 0.5) * step  # the shutter is open for one frame interval, centred on the frame
        truth += t.render(c2(w, h, x), lib.render_params(w, h, 8, spp, 9000 + i))[1]
    truth /= subframes
    mse = lambda a: float(np.mean((a.astype(np.float64) - truth) ** 2))  # noqa: E731
    return {"slide_px": slide_px, "shutter": 1.0, "subframes": subframes, "spp": spp, "largest_motion_px": round(float(np.abs(motion).max()), 2),
            "mse_blurred": mse(blurred), "mse_unblurred": mse(rad), "ratio": round(mse(blurred) / mse(rad), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7, help="timed windows of --reps calls per case; the median and the spread are reported")
    ap.add_argument("--slide-px", type=float, default=2.0)
    ap.add_argument("--no-quality", action="store_true", help="skip the 320x180 MSE measurement")
    args = ap.parse_args()
    W, H = args.width, args.height
    px = W * H
    p = lib.motion_blur_params()
    res = {"scene": "cornell_wahoo C2 pose, 8 bounces, 1 spp", "width": W, "height": H, "reps": args.reps, "repeats": args.repeats,
           "params": {f: getattr(p, f) for f, _ in p._fields_}}
    with lib.Tracer(0) as t:
        t.set_stream(torch.cuda.current_stream().cuda_stream)
        t.upload_scene(scenes.cornell_wahoo_scene())
        dev = torch.device("cuda")
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
        rad, resolved, out, pos, depth, motion = f32(H, W, 3), f32(H, W, 3), f32(H, W, 3), f32(H, W, 3), f32(H, W), f32(H, W, 2)
        ids = torch.zeros((H, W, 3), dtype=torch.int32, device=dev)
        rgb8 = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
        flat = lib.render_params(W, H)
        tp = lib.taa_params()

        def blur(q=p):
            t.motion_blur_device(W, H, resolved.data_ptr(), motion.data_ptr(), depth.data_ptr(), q, rgb8.data_ptr(), out.data_ptr())

        def case(name, nbytes=None, q=p):
            res[name] = timed(lambda: blur(q), args.reps, args.warmup, args.repeats)
            l = torch.linalg.vector_norm(motion, dim=-1) * (0.5 * q.shutter)
            res[name].update(share_of_pixels_with_l_over_half=round(float((l > 0.5).float().mean()), 4),
                             largest_l_px=round(float(l.max().clamp(max=q.max_radius)), 2))
            if nbytes:
                res[name].update(bytes=nbytes, share_of_copy_rate=round(nbytes / (res[name]["event_ms"] * 1e-3) / HBM_COPY_BYTES_PER_S, 3))

        def slide(step_px):
            """Two frames of the sliding camera through ff_gbuffer and ff_taa: resolved, motion and depth of the second."""
            t.taa_reset()
            for j in range(2):
                cam = c2(W, H, world_step(step_px, H) * j)
                t.gbuffer_device(cam, flat, depth.data_ptr(), pos.data_ptr(), None, None, ids.data_ptr())
                t.render_device(cam, lib.render_params(W, H, 8, 1, 1234 + j), None, rad.data_ptr())
                t.taa_device(cam, W, H, rad.data_ptr(), pos.data_ptr(), ids.data_ptr(), tp, rgb8.data_ptr(), resolved.data_ptr())
            lib.check(lib.load().ff_taa_history(t._state, C.c_void_p(motion.data_ptr()), None, 1))
            torch.cuda.synchronize()

        # (a) at rest: the resolved frame of a still camera, motion 0
        slide(0.0)
        case("a_at_rest", 55 * px)
        # (b), (c) the sliding camera
        slide(args.slide_px)
        case(f"b_sliding_{args.slide_px:g}px")
        slide(16.0)
        case("c_sliding_16px")
        # small tile edges on the same input (tiles of up to 8 x 8 pixels are packed by lane groups, several tiles per workgroup)
        for k in (1, 2, 4, 8):
            case(f"c_sliding_16px_k{k}", q=lib.motion_blur_params(max_radius=k))
        # (d) every pixel at l = max_radius
        motion[..., 0] = 2.0 * p.max_radius / p.shutter
        motion[..., 1] = 0.0
        torch.cuda.synchronize()
        case("d_uniform_worst_case")
        # the yardsticks: ff_display (defaults) and ff_taa along tools/taa_bench.py's sliding camera
        dp = lib.display_params()
        res["display_defaults"] = timed(lambda: t.display_device(W, H, resolved.data_ptr(), dp, rgb8.data_ptr(), None), args.reps, args.warmup, args.repeats)
        n = args.reps + args.warmup
        poses = [c2(W, H, world_step(2.0, H) * j) for j in range(n)]
        inputs = []
        for j, cam in enumerate(poses):
            t.set_pixel_jitter(*lib.jitter_sequence(j, 16))
            t.gbuffer_device(cam, flat, None, pos.data_ptr(), None, None, ids.data_ptr())
            t.render_device(cam, lib.render_params(W, H, 8, 1, 1234 + j), None, rad.data_ptr())
            torch.cuda.synchronize()
            inputs.append([x.clone() for x in (rad, pos, ids)])
        t.set_pixel_jitter(0.0, 0.0)
        k = [-1]

        def restart():
            t.taa_reset()
            k[0] = -1

        def taa():
            k[0] += 1
            r_, p_, i_ = inputs[k[0]]
            t.taa_device(poses[k[0]], W, H, r_.data_ptr(), p_.data_ptr(), i_.data_ptr(), tp, rgb8.data_ptr(), out.data_ptr())
        res["taa"] = timed(taa, args.reps, args.warmup, args.repeats, before=restart)
        del inputs
        for name in [key for key in res if key[:2] in ("a_", "b_", "c_", "d_")]:
            res[name]["over_taa"] = round(res[name]["event_ms"] / res["taa"]["event_ms"], 3)
            res[name]["over_display"] = round(res[name]["event_ms"] / res["display_defaults"]["event_ms"], 3)
        if not args.no_quality:
            res["quality_320x180"] = quality(t)
    for key, val in res.items():
        print(f"{key:24s} {val}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
