"""ff_sharpen timings on device buffers, with ff_taa and ff_display as the same-run yardsticks, and what the filter buys: the error of
a temporally resolved image against a many-sample frame with and without it.

(a) At the given size (default 1080p), in one process, ff_sharpen on a 1-spp C2 frame with next-event estimation, for both flag
settings, over --repeats windows of --reps calls, each after warm-up, timed with device events around the window (the median and the
spread of the windows are reported) and per call on the host.  ff_taa (camera at rest) and ff_display (defaults) run beside them.

(b) Reported, asserted nowhere.  MSE against a full-resolution --ref-spp frame, without ff_sharpen and with it at strength 0.25, 0.5
and 1 under both flag settings, of
  - the checker case of tests/test_gpu_taa_upscale.py: cornell_spheres with a checker of 64 squares across the back wall, 160 x 90
    from 16 jittered 80 x 45 frames of 16 spp through ff_taa_upscale (over the back wall and over the whole frame);
  - a C2 sequence at 480 x 270: 16 jittered 1-spp frames through ff_denoise_temporal and ff_taa, the last output.
Prints human-readable lines, then one JSON line.

    python tools/sharpen_bench.py [--width 1920 --height 1080 --reps 200 --warmup 20 --repeats 7 --ref-spp 1024 --no-quality]
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
BACK_WALL = 1  # geometry index in scenes.cornell_spheres_scene
STRENGTHS = (0.25, 0.5, 1.0)
FLAG_SETTINGS = ((T.SHARPEN_NOISE_AWARE, "noise_aware"), (0, "plain"))


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


def c2(w, h):
    return scenes.posed_camera(w, h, position=(0.0, 0.0, 2.4), yaw=-90.0, pitch=0.0)


def sharpened_errors(t, image, mses):
    """{case: {name: mse}} of `image` as it is and through ff_sharpen at every strength and flag setting; mses: {name: function}."""
    rows = {"unsharpened": {k: f(image) for k, f in mses.items()}}
    for flags, label in FLAG_SETTINGS:
        for s in STRENGTHS:
            out = t.sharpen(image, lib.sharpen_params(strength=s, flags=flags), want_rgb8=False)[1]
            row = {k: f(out) for k, f in mses.items()}
            for k in mses:
                row[k + "_ratio"] = round(row[k] / rows["unsharpened"][k], 4)
            rows[f"{label}_{s}"] = row
    return rows


def quality_checker(t, ref_spp, frames=16):
    W, H, w, h = 160, 90, 80, 45
    t.upload_scene(scenes.cornell_spheres_scene())
    t.set_albedo_texture(BACK_WALL, t.create_texture(scenes.checker_texture(128, 128, cells=64)))
    c_hi, c_lo = c2(W, H), c2(w, h)
    hi = t.gbuffer(c_hi, lib.render_params(W, H))
    ref = t.render(c_hi, lib.render_params(W, H, 8, ref_spp, 77, shade_mode=NEE))[1].astype(np.float64)
    t.taa_upscale_reset()
    out = None
    for i in range(frames):
        j = lib.jitter_sequence(i, 16)
        t.set_pixel_jitter(*j)
        frame = t.render(c_lo, lib.render_params(w, h, 8, 16, 1000 + i, shade_mode=NEE))[1]
        lo = t.gbuffer(c_lo, lib.render_params(w, h))
        t.set_pixel_jitter(0.0, 0.0)
        out = t.taa_upscale(frame, lo, hi, c_hi, lib.taa_upscale_params(lo_jitter=j))[1]
    t.taa_upscale_reset()
    wall = hi["ids"][..., 0] == BACK_WALL
    mse = lambda a, m: float(np.mean((np.asarray(a, np.float64)[m] - ref[m]) ** 2))  # noqa: E731
    res = {"scene": "cornell_spheres, checker of 64 squares on the back wall; 160x90 from 16 jittered 80x45 frames of 16 spp, ff_taa_upscale defaults",
           "truth_spp": ref_spp}
    res.update(sharpened_errors(t, out, {"mse_back_wall": lambda a: mse(a, wall), "mse_frame": lambda a: mse(a, np.ones((H, W), bool))}))
    return res


def quality_c2(t, ref_spp, w=480, h=270, frames=16):
    t.upload_scene(scenes.cornell_wahoo_scene())
    cam = c2(w, h)
    ref = t.render(cam, lib.render_params(w, h, 8, ref_spp, 77, shade_mode=NEE))[1].astype(np.float64)
    t.temporal_reset()
    t.taa_reset()
    out = None
    for i in range(frames):
        t.set_pixel_jitter(*lib.jitter_sequence(i, 16))
        frame = t.render(cam, lib.render_params(w, h, 8, 1, 2000 + i, shade_mode=NEE))[1]
        gb = t.gbuffer(cam, lib.render_params(w, h))
        clean = t.denoise_temporal(frame, gb, cam)[1]
        out = t.taa(clean, gb, cam)[1]
    t.set_pixel_jitter(0.0, 0.0)
    t.temporal_reset()
    t.taa_reset()
    res = {"scene": "cornell_wahoo C2 pose, 480x270, 16 jittered 1-spp NEE frames through ff_denoise_temporal and ff_taa (defaults)", "truth_spp": ref_spp}
    res.update(sharpened_errors(t, out, {"mse_frame": lambda a: float(np.mean((np.asarray(a, np.float64) - ref) ** 2))}))
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
    res = {"scene": "cornell_wahoo C2 pose, 1-spp NEE", "width": W, "height": H, "reps": args.reps, "repeats": args.repeats}
    with lib.Tracer(0) as t:
        t.set_stream(torch.cuda.current_stream().cuda_stream)
        t.upload_scene(scenes.cornell_wahoo_scene())
        dev = torch.device("cuda")
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
        rad, out, pos, nrm, alb = f32(H, W, 3), f32(H, W, 3), f32(H, W, 3), f32(H, W, 3), f32(H, W, 3)
        ids = torch.zeros((H, W, 3), dtype=torch.int32, device=dev)
        rgb8 = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
        cam = c2(W, H)
        t.gbuffer_device(cam, lib.render_params(W, H), None, pos.data_ptr(), nrm.data_ptr(), alb.data_ptr(), ids.data_ptr())
        t.render_device(cam, lib.render_params(W, H, 8, 1, 1234, shade_mode=NEE), None, rad.data_ptr())
        torch.cuda.synchronize()
        for flags, label in FLAG_SETTINGS:
            p = lib.sharpen_params(flags=flags)
            name = f"sharpen_{label}"
            res[name] = timed(lambda: t.sharpen_device(W, H, rad.data_ptr(), p, rgb8.data_ptr(), out.data_ptr()), args.reps, args.warmup, args.repeats)
            res[name]["changed_share"] = round(float((out != rad).any(dim=-1).float().mean().item()), 5)
        res["sharpen_noise_aware_radiance_only"] = timed(lambda: t.sharpen_device(W, H, rad.data_ptr(), None, None, out.data_ptr()), args.reps, args.warmup,
                                                         args.repeats)
        tp = lib.taa_params()
        res["taa_at_rest"] = timed(lambda: t.taa_device(cam, W, H, rad.data_ptr(), pos.data_ptr(), ids.data_ptr(), tp, rgb8.data_ptr(), out.data_ptr()),
                                   args.reps, args.warmup, args.repeats, before=t.taa_reset)
        dp = lib.display_params()
        res["display_defaults"] = timed(lambda: t.display_device(W, H, rad.data_ptr(), dp, rgb8.data_ptr(), out.data_ptr()), args.reps, args.warmup,
                                        args.repeats)
        for name in [k for k in res if k.startswith("sharpen_")]:
            res[name]["over_taa"] = round(res[name]["event_ms"] / res["taa_at_rest"]["event_ms"], 3)
            res[name]["over_display"] = round(res[name]["event_ms"] / res["display_defaults"]["event_ms"], 3)
        # compulsory bytes: radiance in (12), radiance and rgb8 out (15) per pixel
        res["compulsory_bytes"] = 27 * W * H
        res["floor_ms_at_8TBps"] = round(27 * W * H / 8.0e12 * 1e3, 5)
        if not args.no_quality:
            res["quality_checker_160x90"] = quality_checker(t, args.ref_spp)
            res["quality_c2_480x270"] = quality_c2(t, args.ref_spp)
    for key, val in res.items():
        if key.startswith("quality_"):
            print(key)
            for k2, v2 in val.items():
                print(f"  {k2:22s} {v2}")
        else:
            print(f"{key:36s} {val}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
