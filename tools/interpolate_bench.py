"""ff_interpolate timings on device buffers, with ff_taa and ff_display as the same-run yardsticks, and what frame generation buys:
the error of an in-between frame against a many-sample render of its pose, beside the plain blend, a repeated frame and a frame that
was really rendered.

(a) At the given size (default 1080p), in one process, ff_interpolate on 1-spp C2 frames with next-event estimation: at rest (three
equal cameras: nothing is projected), along taa_bench.py's sliding camera (A, mid and B one step of the path apart each), there with
fill_radius 0 and 8, over --repeats windows of --reps calls, each after warm-up, timed with device events around the window (the
median and the spread of the windows are reported) and per call on the host.  ff_taa (at rest) and ff_display (defaults) run beside
them.

(b) Reported, asserted nowhere.  On the sliding C2 camera at 480 x 270, the sources A and B are two 1-spp NEE frames two steps apart,
each the last of a run of the path through ff_denoise_temporal and ff_taa; the pose between them is compared, as MSE against a
--ref-spp render of that pose, for: ff_interpolate (surface_tolerance 1, 2, 4 and 8; fill_radius 0 and 4), the blend (A + B) / 2, A
repeated, and a frame really rendered at the mid pose and resolved through the same filters.  The host time of ff_gbuffer +
ff_interpolate stands beside that of the rendered and resolved frame.
Prints human-readable lines, then one JSON line.

    python tools/interpolate_bench.py [--width 1920 --height 1080 --reps 200 --warmup 20 --repeats 7 --ref-spp 1024 --no-quality]
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

NEE = T.SHADE_DIFFUSE_PATH_NEE
TOLERANCES = (1.0, 2.0, 4.0, 8.0)


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


def sliding(w, h, k):
    """Pose k of taa_bench.py's sliding path."""
    return scenes.posed_camera(w, h, position=(-0.24 + 0.03 * k, 0.0, 2.4), yaw=-90.0 + 0.2 * k, pitch=0.0)


def quality_sliding(t, ref_spp, w=480, h=270, last=14):
    """A = pose last - 2, mid = last - 1, B = last of the sliding path; every resolved frame is the end of its own run of the path."""
    t.upload_scene(scenes.cornell_wahoo_scene())
    flat = lib.render_params(w, h)

    def resolved(k_end, seed):
        """Poses 0 .. k_end at 1 spp through ff_denoise_temporal and ff_taa -> (the last output, its G-buffer, host ms of the last frame)."""
        t.temporal_reset()
        t.taa_reset()
        out = gb = None
        ms = 0.0
        for k in range(k_end + 1):
            cam = sliding(w, h, k)
            t0 = time.perf_counter()
            frame = t.render(cam, lib.render_params(w, h, 8, 1, seed + k, shade_mode=NEE))[1]
            gb = t.gbuffer(cam, flat)
            out = t.taa(t.denoise_temporal(frame, gb, cam)[1], gb, cam)[1]
            ms = (time.perf_counter() - t0) * 1e3
        return out, gb, ms

    cams = [sliding(w, h, k) for k in (last - 2, last - 1, last)]
    ra, ga, _ = resolved(last - 2, 3000)
    rb, gb_, _ = resolved(last, 3000)
    rm, gm, rendered_ms = resolved(last - 1, 3000)
    t.temporal_reset()
    t.taa_reset()
    truth = t.render(cams[1], lib.render_params(w, h, 8, ref_spp, 77, shade_mode=NEE))[1].astype(np.float64)
    mse = lambda a: float(np.mean((np.asarray(a, np.float64) - truth) ** 2))  # noqa: E731
    res = {"scene": f"cornell_wahoo, sliding C2 path, {w}x{h}, A / mid / B = poses {last - 2} / {last - 1} / {last}, 1-spp NEE through "
                    "ff_denoise_temporal and ff_taa (defaults)", "truth_spp": ref_spp,
           "mse_blend": mse((ra.astype(np.float64) + rb) / 2), "mse_repeat_a": mse(ra), "mse_rendered_mid_1spp": mse(rm),
           "rendered_mid_host_ms": round(rendered_ms, 3)}
    mid, a, b = (cams[1], gm), (cams[0], ra, ga), (cams[2], rb, gb_)
    for tol in TOLERANCES:
        for r in (0, 4):
            rgb8, out, counts = t.interpolate(mid, a, b, lib.interpolate_params(surface_tolerance=tol, fill_radius=r), want_rgb8=False)
            res[f"interpolated_tol{tol:g}_fill{r}"] = {"mse": mse(out), "over_blend": round(mse(out) / res["mse_blend"], 4),
                                                       "over_rendered": round(mse(out) / res["mse_rendered_mid_1spp"], 4), "counts": counts.tolist()}
    ts = []
    for _ in range(9):
        t0 = time.perf_counter()
        g = t.gbuffer(cams[1], flat)
        t.interpolate((cams[1], g), a, b, want_rgb8=False)
        ts.append((time.perf_counter() - t0) * 1e3)
    res["gbuffer_plus_interpolate_host_ms"] = round(float(np.median(ts)), 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7, help="timed windows of --reps calls per case; the median and the spread are reported")
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--no-quality", action="store_true", help="skip the MSE measurements")
    args = ap.parse_args()
    W, H = args.width, args.height
    res = {"scene": "cornell_wahoo, 1-spp NEE", "width": W, "height": H, "reps": args.reps, "repeats": args.repeats}
    with lib.Tracer(0) as t:
        t.set_stream(torch.cuda.current_stream().cuda_stream)
        t.upload_scene(scenes.cornell_wahoo_scene())
        dev = torch.device("cuda")
        f32 = lambda: torch.zeros((H, W, 3), dtype=torch.float32, device=dev)  # noqa: E731
        i32 = lambda: torch.zeros((H, W, 3), dtype=torch.int32, device=dev)  # noqa: E731
        out = f32()
        rgb8 = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
        flat = lib.render_params(W, H)

        def frame(cam, seed, want_radiance=True):
            rad, pos, ids = f32(), f32(), i32()
            t.gbuffer_device(cam, flat, None, pos.data_ptr(), None, None, ids.data_ptr())
            if want_radiance:
                t.render_device(cam, lib.render_params(W, H, 8, 1, seed, shade_mode=NEE), None, rad.data_ptr())
            return cam, rad, pos, ids

        def call(mid, a, b, p):
            ptrs = [x.data_ptr() for x in (mid[2], mid[3], a[1], a[2], a[3], b[1], b[2], b[3])]
            return lambda: t.interpolate_device(W, H, (mid[0], a[0], b[0]), ptrs, p, None, rgb8.data_ptr(), out.data_ptr(), want_counts=False)

        rest = frame(sliding(W, H, 8), 1234)
        rest_b = (rest[0], frame(rest[0], 1235)[1], rest[2], rest[3])
        a, mid, b = frame(sliding(W, H, 7), 1236), frame(sliding(W, H, 8), 0, False), frame(sliding(W, H, 9), 1237)
        torch.cuda.synchronize()
        res["interpolate_at_rest"] = timed(call(rest, rest, rest_b, lib.interpolate_params()), args.reps, args.warmup, args.repeats)
        for r in (4, 0, 8):
            p = lib.interpolate_params(fill_radius=r)
            name = f"interpolate_sliding_fill{r}"
            res[name] = timed(call(mid, a, b, p), args.reps, args.warmup, args.repeats)
            ptrs = [x.data_ptr() for x in (mid[2], mid[3], a[1], a[2], a[3], b[1], b[2], b[3])]
            res[name]["counts"] = t.interpolate_device(W, H, (mid[0], a[0], b[0]), ptrs, p, None, None, out.data_ptr()).tolist()
        res["gbuffer"] = timed(lambda: t.gbuffer_device(mid[0], flat, None, mid[2].data_ptr(), None, None, mid[3].data_ptr()), args.reps // 4, 5, 3)
        tp = lib.taa_params()
        res["taa_at_rest"] = timed(lambda: t.taa_device(rest[0], W, H, rest[1].data_ptr(), rest[2].data_ptr(), rest[3].data_ptr(), tp, rgb8.data_ptr(),
                                                        out.data_ptr()), args.reps, args.warmup, args.repeats, before=t.taa_reset)
        dp = lib.display_params()
        res["display_defaults"] = timed(lambda: t.display_device(W, H, rest[1].data_ptr(), dp, rgb8.data_ptr(), out.data_ptr()), args.reps, args.warmup,
                                        args.repeats)
        for name in [k for k in res if k.startswith("interpolate_")]:
            res[name]["over_taa"] = round(res[name]["event_ms"] / res["taa_at_rest"]["event_ms"], 3)
            res[name]["over_display"] = round(res[name]["event_ms"] / res["display_defaults"]["event_ms"], 3)
        # compulsory bytes per pixel: the mid G-buffer's position and ids (24), two sources' radiance, position and ids at one tap
        # each (72), the work image written and read (32), radiance and rgb8 out (15)
        res["compulsory_bytes"] = 143 * W * H
        res["floor_ms_at_8TBps"] = round(143 * W * H / 8.0e12 * 1e3, 5)
        if not args.no_quality:
            res["quality_sliding_480x270"] = quality_sliding(t, args.ref_spp)
    for key, val in res.items():
        if key.startswith("quality_"):
            print(key)
            for k2, v2 in val.items():
                print(f"  {k2:34s} {v2}")
        else:
            print(f"{key:36s} {val}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
