"""ff_local_tonemap timings on device buffers, with ff_taa and ff_display as the same-run yardsticks, and how far its piecewise-linear
log2 / exp2 take the result from the true ones.

(a) At the given size (default 1080p), in one process, ff_local_tonemap on a 1-spp C2 frame with next-event estimation for cell 8,
16, 32 and 64 (defaults otherwise), radiance and rgb8 out, over --repeats windows of --reps calls, each after warm-up, timed with
device events around the window (the median and the spread of the windows are reported) and per call on the host; the copy
(compression 1, detail 1) and the in-place call beside them.  ff_taa (camera at rest) and ff_display (defaults) run in the same
process.  The per-kernel split comes from a separate run under `rocprofv3 --kernel-trace --stats` with --no-quality.

(b) Reported, asserted nowhere.  The largest and the median relative deviation of the output from a float64 restatement with true
log2 / exp2 (tests/local_tonemap_ref.py true_log_tonemap), over the mapped pixels, at the defaults, on a 64-spp C2 frame and on
the wahoo-under-sun frame of tools/env_bench.py, both 480 x 270; and how much of each frame's range the call takes away (the
spread of log2 luminance between the 1st and the 99th percentile, before and after).
Prints human-readable lines, then one JSON line.

    python tools/local_tonemap_bench.py [--width 1920 --height 1080 --reps 200 --warmup 20 --repeats 7 --no-quality]
"""
import argparse
import json
import os
import sys
import time

import torch  # (before the library: one HIP runtime per process, see tests/conftest.py)
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gpupathtracer_amd import lib, scenes  # noqa: E402
from gpupathtracer_amd import types as T  # noqa: E402
import local_tonemap_ref as R  # noqa: E402

NEE = T.SHADE_DIFFUSE_PATH_NEE


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


def deviation(t, frame, what):
    """The call at its defaults on `frame` against the float64 true-log restatement."""
    p = lib.local_tonemap_params()
    out = t.local_tonemap(frame, p, want_rgb8=False)[1].astype(np.float64)
    true = R.true_log_tonemap(frame, p.compression, p.detail, p.pivot, p.cell)
    with np.errstate(all="ignore"):
        l = R.luminance(np.asarray(frame, np.float32))
    ok = R.mapped_mask(np.asarray(frame, np.float32), l)
    lum = lambda a: 0.2126 * a[..., 0] + 0.7152 * a[..., 1] + 0.0722 * a[..., 2]  # noqa: E731
    rel = np.abs(lum(out)[ok] / lum(true)[ok] - 1.0)
    spread = lambda a: float(np.subtract(*np.percentile(np.log2(lum(a)[ok]), [99, 1])))  # noqa: E731
    return {"frame": what, "mapped_share": round(float(ok.mean()), 4), "max_rel_deviation": round(float(rel.max()), 4),
            "median_rel_deviation": round(float(np.median(rel)), 4), "p99_rel_deviation": round(float(np.percentile(rel, 99)), 4),
            "stops_p1_to_p99_in": round(spread(np.asarray(frame, np.float64)), 3), "stops_p1_to_p99_out": round(spread(out), 3),
            "stops_p1_to_p99_true_log": round(spread(true), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7, help="timed windows of --reps calls per case; the median and the spread are reported")
    ap.add_argument("--no-quality", action="store_true", help="timings only (the run rocprofv3 watches)")
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
        for cell in T.LOCAL_TONEMAP_CELLS:
            p = lib.local_tonemap_params(cell=cell)
            name = f"local_tonemap_cell{cell}"
            res[name] = timed(lambda: t.local_tonemap_device(W, H, rad.data_ptr(), p, rgb8.data_ptr(), out.data_ptr()), args.reps, args.warmup, args.repeats)
            res[name]["changed_share"] = round(float((out != rad).any(dim=-1).float().mean().item()), 5)
            res[name]["grid_cells"] = -(-W // cell) * -(-H // cell) * T.LOCAL_TONEMAP_BINS
        res["local_tonemap_cell32_radiance_only"] = timed(lambda: t.local_tonemap_device(W, H, rad.data_ptr(), None, None, out.data_ptr()), args.reps,
                                                          args.warmup, args.repeats)
        ident = lib.local_tonemap_params(compression=1.0, detail=1.0)
        res["local_tonemap_copy"] = timed(lambda: t.local_tonemap_device(W, H, rad.data_ptr(), ident, rgb8.data_ptr(), out.data_ptr()), args.reps,
                                          args.warmup, args.repeats)
        scratch = rad.clone()  # (in place: the image drifts from call to call, the work per call does not)
        gentle = lib.local_tonemap_params(compression=0.99)
        res["local_tonemap_cell32_in_place"] = timed(lambda: t.local_tonemap_device(W, H, scratch.data_ptr(), gentle, rgb8.data_ptr(), scratch.data_ptr()),
                                                     args.reps, args.warmup, args.repeats)
        tp = lib.taa_params()
        res["taa_at_rest"] = timed(lambda: t.taa_device(cam, W, H, rad.data_ptr(), pos.data_ptr(), ids.data_ptr(), tp, rgb8.data_ptr(), out.data_ptr()),
                                   args.reps, args.warmup, args.repeats, before=t.taa_reset)
        dp = lib.display_params()
        res["display_defaults"] = timed(lambda: t.display_device(W, H, rad.data_ptr(), dp, rgb8.data_ptr(), out.data_ptr()), args.reps, args.warmup,
                                        args.repeats)
        for name in [k for k in res if k.startswith("local_tonemap_")]:
            res[name]["over_taa"] = round(res[name]["event_ms"] / res["taa_at_rest"]["event_ms"], 3)
            res[name]["over_display"] = round(res[name]["event_ms"] / res["display_defaults"]["event_ms"], 3)
        # compulsory bytes: radiance in twice (splat, slice: 24), radiance and rgb8 out (15) per pixel
        res["compulsory_bytes"] = 39 * W * H
        res["floor_ms_at_8TBps"] = round(39 * W * H / 8.0e12 * 1e3, 5)
        if not args.no_quality:
            w, h = 480, 270
            frame = t.render(c2(w, h), lib.render_params(w, h, 8, 64, 77, shade_mode=NEE))[1]
            res["true_log_c2_480x270"] = deviation(t, frame, "cornell_wahoo C2 pose, 64-spp NEE")
            t.upload_scene(scenes.open_floor_scene())
            t.set_environment(scenes.sun_sky_map(2048, 1024))
            sun_cam = scenes.posed_camera(w, h, position=(0.0, -1.2, 3.0), yaw=-90.0, pitch=0.0)
            frame = t.render(sun_cam, lib.render_params(w, h, 8, 64, 77, shade_mode=NEE))[1]
            res["true_log_wahoo_under_sun_480x270"] = deviation(t, frame, "wahoo on a floor under sun_sky_map 2048x1024, 64-spp NEE")
    for key, val in res.items():
        print(f"{key:40s} {val}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
