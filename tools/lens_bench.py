"""ff_lens timings on device buffers, with ff_display and ff_resize as the same-run yardsticks, and what the better filter buys: the
error of a distort / undistort round trip.

(a) At the given size (default 1080p), in one process, ff_lens on a 1-spp C2 frame with next-event estimation: bilinear, Catmull-Rom
with and without the anti-ring clamp, with and without chromatic aberration, mild (k1 = -0.05) and strong (k1 = -0.3) distortion
(UNDISTORT, the direction in which the strong one does not fold), the vignette alone; beside them ff_display (ACES + sRGB) and
ff_resize at equal size under Lanczos-3.  Medians of --repeats windows of --reps synchronous calls, device-event time per call, with
the windows' range.  The stage's byte floor is 27 bytes per pixel (12 in, 12 + 3 out) at 6.3 TB/s; the ratio is stated.
(b) Reported, asserted nowhere.  A 480 x 270 frame of the box with a checker on its back wall, 64 spp: DISTORT, then UNDISTORT with
the same coefficients, BLACK border, both at zoom 1 (the zoom magnifies a call's OUTPUT, so two zoomed calls do not compose to the
identity and a fitting zoom cannot be undone by the second call); the MSE against the original over the pixels whose way through both
maps stays two pixels inside the image, for bilinear against Catmull-Rom (with the clamp).

    python tools/lens_bench.py [--width 1920 --height 1080 --reps 200 --warmup 20 --repeats 7 --no-quality]
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
CR, BL, RING = T.LENS_CATMULL_ROM, T.LENS_BILINEAR, T.LENS_ANTI_RING
U = T.LENS_UNDISTORT
CASES = {
    "bilinear_mild": dict(k1=-0.05, direction=U, filter=BL, flags=0),
    "catmull_rom_mild": dict(k1=-0.05, direction=U, filter=CR, flags=0),
    "catmull_rom_clamped_mild": dict(k1=-0.05, direction=U, filter=CR, flags=RING),
    "catmull_rom_clamped_mild_ca": dict(k1=-0.05, direction=U, filter=CR, flags=RING, ca_red=0.003, ca_blue=-0.003),
    "bilinear_mild_ca": dict(k1=-0.05, direction=U, filter=BL, flags=0, ca_red=0.003, ca_blue=-0.003),
    "catmull_rom_clamped_strong": dict(k1=-0.3, direction=U, filter=CR, flags=RING),
    "catmull_rom_clamped_strong_ca": dict(k1=-0.3, direction=U, filter=CR, flags=RING, ca_red=0.003, ca_blue=-0.003),
    "vignette_alone": dict(filter=CR, flags=RING, vignette=0.7, vignette_falloff=1.0, direction=T.LENS_DISTORT),
    "identity": dict(),
}


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


def quality_round_trip(t, spp=64):
    W, H = 480, 270
    t.upload_scene(scenes.cornell_spheres_scene())
    t.set_albedo_texture(BACK_WALL, t.create_texture(scenes.checker_texture(128, 128, cells=64)))
    frame = t.render(c2(W, H), lib.render_params(W, H, 8, spp, 77, shade_mode=NEE))[1]
    y, x = np.mgrid[0:H, 0:W]
    xy = np.stack([x.ravel() + 0.5, y.ravel() + 0.5], axis=1)
    res = {"scene": f"cornell_spheres, checker of 64 squares on the back wall, {W}x{H}, {spp} spp"}
    for label, k in (("mild_k1_-0.05", dict(k1=-0.05)), ("strong_k1_-0.2_k2_0.03", dict(k1=-0.2, k2=0.03))):
        row = {}
        for name, filt in (("bilinear", dict(filter=BL, flags=0)), ("catmull_rom", dict(filter=CR, flags=RING))):
            there = lib.lens_params(direction=T.LENS_DISTORT, **k, **filt)
            back = lib.lens_params(direction=T.LENS_UNDISTORT, **k, **filt)
            out = t.lens(t.lens(frame, there, want_rgb8=False)[1], back, want_rgb8=False)[1]
            # the way of the returned image's pixels: first through `back`'s map, then through `there`'s
            mid = lib.lens_map(W, H, xy, back)
            src = lib.lens_map(W, H, mid, there)
            keep = np.ones(len(xy), bool)
            for pos in (mid, src):
                keep &= (pos[:, 0] >= 2) & (pos[:, 0] <= W - 2) & (pos[:, 1] >= 2) & (pos[:, 1] <= H - 2)
            keep = keep.reshape(H, W)
            row[name + "_mse"] = float(np.mean((np.asarray(out, np.float64)[keep] - np.asarray(frame, np.float64)[keep]) ** 2))
            row["kept_share"] = round(float(keep.mean()), 4)
            row[name + "_way_error_px"] = round(float(np.abs(src - xy)[keep.ravel()].max()), 6)
        row["bilinear_over_catmull_rom"] = round(row["bilinear_mse"] / row["catmull_rom_mse"], 3)
        res[label] = row
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7, help="timed windows of --reps calls per case; the median and the spread are reported")
    ap.add_argument("--no-quality", action="store_true", help="skip the round-trip MSE")
    args = ap.parse_args()
    W, H = args.width, args.height
    res = {"scene": "cornell_wahoo C2 pose, 1-spp NEE", "width": W, "height": H, "reps": args.reps, "repeats": args.repeats}
    with lib.Tracer(0) as t:
        t.set_stream(torch.cuda.current_stream().cuda_stream)
        t.upload_scene(scenes.cornell_wahoo_scene())
        dev = torch.device("cuda")
        rad = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
        out = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
        rgb8 = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
        t.render_device(c2(W, H), lib.render_params(W, H, 8, 1, 1234, shade_mode=NEE), None, rad.data_ptr())
        torch.cuda.synchronize()
        for name, fields in CASES.items():
            p = lib.lens_params(**fields)
            key = f"lens_{name}"
            res[key] = timed(lambda: t.lens_device(W, H, rad.data_ptr(), p, rgb8.data_ptr(), out.data_ptr()), args.reps, args.warmup, args.repeats)
            res[key]["changed_share"] = round(float((out != rad).any(dim=-1).float().mean().item()), 5)
        p = lib.lens_params(**CASES["catmull_rom_clamped_mild"])
        res["lens_catmull_rom_clamped_mild_radiance_only"] = timed(lambda: t.lens_device(W, H, rad.data_ptr(), p, None, out.data_ptr()), args.reps,
                                                                   args.warmup, args.repeats)
        dp = lib.display_params()
        res["display_defaults"] = timed(lambda: t.display_device(W, H, rad.data_ptr(), dp, rgb8.data_ptr(), out.data_ptr()), args.reps, args.warmup,
                                        args.repeats)
        rp = lib.resize_params(filter=T.RESIZE_LANCZOS3)
        res["resize_equal_size_lanczos3"] = timed(lambda: t.resize_device(W, H, rad.data_ptr(), W, H, rp, rgb8.data_ptr(), out.data_ptr()), args.reps,
                                                  args.warmup, args.repeats)
        # compulsory bytes: radiance in (12), radiance and rgb8 out (15) per pixel
        res["compulsory_bytes"] = 27 * W * H
        floor = 27 * W * H / 6.3e12 * 1e3
        res["floor_ms_at_6.3TBps"] = round(floor, 5)
        for name in [k for k in res if k.startswith("lens_")]:
            res[name]["over_display"] = round(res[name]["event_ms"] / res["display_defaults"]["event_ms"], 3)
            res[name]["over_resize"] = round(res[name]["event_ms"] / res["resize_equal_size_lanczos3"]["event_ms"], 3)
            res[name]["over_floor"] = round(res[name]["event_ms"] / floor, 2)
        if not args.no_quality:
            res["quality_round_trip_480x270"] = quality_round_trip(t)
    for key, val in res.items():
        if key.startswith("quality_"):
            print(key)
            for k2, v2 in val.items():
                print(f"  {k2:26s} {v2}")
        else:
            print(f"{key:46s} {val}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
