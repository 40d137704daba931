"""ff_despeckle timings on device buffers, with ff_denoise and ff_taa as the same-run yardsticks, and what the filter is for: the error
of a denoised 1-spp frame with and without it, and the energy it removes.

(a) At the given size (default 1080p), in one process, ff_despeckle on the C2 G-buffer and a 1-spp frame with next-event estimation
over --repeats windows of --reps calls, each after warm-up, timed with device events around the window (the median and the spread of
the windows are reported) and per call on the host: radius 1, 2 and 3 at rank 2, and rank 1 and 4 at radius 3.  ff_denoise (defaults)
and ff_taa (camera at rest) run beside them.

(b) At 480x270: C2 with its floor a rough mirror (tools/glossy_bench.py's scene, roughness 0.3), a --ref-spp frame with next-event
estimation as the truth.  MSE against it of the raw 1-spp frame through ff_denoise, of the despeckled frame through ff_denoise, and of
each of the two through 16 frames of ff_denoise_temporal (camera at rest, a new seed per frame, the last output).  The mean luminance
of the raw and of the despeckled frame over the truth's: the energy the clamp removes.  Then a sweep of threshold x rank (radius 1
and 2) through the spatial pipeline.  Prints human-readable lines, then one JSON line.

    python tools/despeckle_bench.py [--width 1920 --height 1080 --reps 200 --warmup 20 --repeats 7 --ref-spp 4096 --no-quality]
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
C2_FLOOR = 3
LUMA = np.array([0.2126, 0.7152, 0.0722])


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


def rough_floor_scene():
    scene = scenes.cornell_wahoo_scene()
    s = scenes.Scene()
    s._specs = list(scene._specs)
    s._specs[C2_FLOOR] = s._specs[C2_FLOOR][:5] + (scenes.make_bxdf(T.BXDF_MIRROR, specular=(0.9, 0.85, 0.75)),)
    return s.finalize()


def quality(t, ref_spp, w=480, h=270, frames=16):
    t.upload_scene(rough_floor_scene())
    t.set_roughness(C2_FLOOR, 0.3)
    cam = c2(w, h)
    t0 = time.perf_counter()
    truth = t.render(cam, lib.render_params(w, h, 8, ref_spp, 77, shade_mode=NEE))[1].astype(np.float64)
    res = {"scene": "C2, floor a mirror of roughness 0.3", "width": w, "height": h, "truth_spp": ref_spp, "truth_s": round(time.perf_counter() - t0, 2)}
    gb = t.gbuffer(cam, lib.render_params(w, h))
    mse = lambda a: float(np.mean((a.astype(np.float64) - truth) ** 2))  # noqa: E731
    mean_l = lambda a: float((a.astype(np.float64) @ LUMA).mean())  # noqa: E731
    raws = [t.render(cam, lib.render_params(w, h, 8, 1, 4321 + j, shade_mode=NEE))[1] for j in range(frames)]
    raw = raws[0]

    def spatial(p):
        rgb8, clean, n = t.despeckle(raw, gb, p, want_rgb8=False)
        return {"mse_denoised": mse(t.denoise(clean, gb)[1]), "mse_frame": mse(clean), "clamped_share": round(n / (w * h), 5),
                "mean_luminance_over_truth": round(mean_l(clean) / mean_l(truth), 5)}

    def temporal(p):
        t.temporal_reset()
        out = None
        for frame in raws:
            if p is not None:
                frame = t.despeckle(frame, gb, p, want_rgb8=False)[1]
            out = t.denoise_temporal(frame, gb, cam)[1]
        t.temporal_reset()
        return mse(out)

    defaults = lib.despeckle_params()
    res["raw"] = {"mse_denoised": mse(t.denoise(raw, gb)[1]), "mse_frame": mse(raw), "mean_luminance_over_truth": round(mean_l(raw) / mean_l(truth), 5),
                  "mse_temporal_16": temporal(None)}
    res["defaults"] = dict(spatial(defaults), mse_temporal_16=temporal(defaults))
    res["defaults"]["denoised_ratio"] = round(res["defaults"]["mse_denoised"] / res["raw"]["mse_denoised"], 4)
    res["defaults"]["temporal_ratio"] = round(res["defaults"]["mse_temporal_16"] / res["raw"]["mse_temporal_16"], 4)
    sweep = {}
    for radius in (1, 2):
        for rank in (1, 2, 3, 4):
            for threshold in (1.5, 2.0, 3.0, 4.0, 8.0):
                row = spatial(lib.despeckle_params(radius=radius, rank=rank, min_neighbours=max(rank, 3), threshold=threshold))
                row["denoised_ratio"] = round(row["mse_denoised"] / res["raw"]["mse_denoised"], 4)
                sweep[f"r{radius}_rank{rank}_t{threshold}"] = row
    res["sweep"] = sweep
    best = min(sweep, key=lambda k: sweep[k]["mse_denoised"])
    res["best_of_sweep"] = {"case": best, **sweep[best]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7, help="timed windows of --reps calls per case; the median and the spread are reported")
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--no-quality", action="store_true", help="skip the 480x270 MSE measurement")
    args = ap.parse_args()
    W, H = args.width, args.height
    res = {"scene": "cornell_wahoo C2 pose", "width": W, "height": H, "reps": args.reps, "repeats": args.repeats}
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
        for radius, rank in ((1, 2), (2, 2), (3, 2), (3, 1), (3, 4)):
            p = lib.despeckle_params(radius=radius, rank=rank, min_neighbours=max(rank, 3))
            clamped = t.despeckle_device(W, H, rad.data_ptr(), alb.data_ptr(), ids.data_ptr(), p, rgb8.data_ptr(), out.data_ptr())
            name = f"despeckle_r{radius}_rank{rank}"
            res[name] = timed(lambda: t.despeckle_device(W, H, rad.data_ptr(), alb.data_ptr(), ids.data_ptr(), p, rgb8.data_ptr(), out.data_ptr()),
                              args.reps, args.warmup, args.repeats)
            res[name]["clamped_share"] = round(clamped / (W * H), 5)
        dn = lib.denoise_params()
        res["denoise_defaults"] = timed(lambda: t.denoise_device(W, H, rad.data_ptr(), pos.data_ptr(), nrm.data_ptr(), alb.data_ptr(), ids.data_ptr(), dn,
                                                                 rgb8.data_ptr(), out.data_ptr()), args.reps, args.warmup, args.repeats)
        tp = lib.taa_params()
        res["taa_at_rest"] = timed(lambda: t.taa_device(cam, W, H, rad.data_ptr(), pos.data_ptr(), ids.data_ptr(), tp, rgb8.data_ptr(), out.data_ptr()),
                                   args.reps, args.warmup, args.repeats, before=t.taa_reset)
        for name in [k for k in res if k.startswith("despeckle_")]:
            res[name]["over_denoise"] = round(res[name]["event_ms"] / res["denoise_defaults"]["event_ms"], 3)
            res[name]["over_taa"] = round(res[name]["event_ms"] / res["taa_at_rest"]["event_ms"], 3)
        if not args.no_quality:
            res["quality_480x270"] = quality(t, args.ref_spp)
    for key, val in res.items():
        if key == "quality_480x270":
            for k2, v2 in val.items():
                if k2 == "sweep":
                    for k3, v3 in v2.items():
                        print(f"  sweep {k3:20s} {v3}")
                else:
                    print(f"  {k2:22s} {v2}")
        else:
            print(f"{key:24s} {val}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
