"""ff_render_adaptive measured on C2 (the Cornell box with wahoo and the cube, the benchmark's pose), 8 bounces, in both path modes.

(a) Driver overhead at the given size (default 1080p): threshold 0 over --passes passes of --spp samples - every tile runs to the end,
so the call does the work of --passes progressive frames plus its own: a launch and a render_finish per rectangle, the accumulate,
the error pass and its read-back at every second pass, the resolve - against --passes frames of ff_render_progressive and against
one ff_render of passes * spp samples, wall time, best of --repeats.  The progressive frames of a camera at rest start from the
primary hits the state keeps; so do the adaptive call's whole-frame passes, and its partial rectangles cannot.

(b) Adaptive against uniform at 480x270: a sweep of threshold x tile at max_passes * spp = --budget (default 1024) against the
uniform frame of --budget samples: wall time, info.samples over the uniform count, info.rectangles, and the MSE of both against a
--ref-spp frame (default 16384).  Reported as equal-time MSE (the uniform frame whose sample count takes the adaptive call's time,
rendered and measured) and as equal-quality time (the time of the uniform frame that reaches the adaptive frame's MSE, from the
uniform frames' measured MSE-over-time curve, interpolated in log-log).  Prints human-readable lines, then one JSON line.

    python tools/adaptive_bench.py [--width 1920 --height 1080 --passes 16 --spp 64 --repeats 3 --budget 1024 --ref-spp 16384 --no-quality]
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
from gpupathtracer_amd import types as T  # noqa: E402

MODES = {"path": T.SHADE_DIFFUSE_PATH, "nee": T.SHADE_DIFFUSE_PATH_NEE}


def c2(w, h):
    return scenes.posed_camera(w, h, position=(0.0, 0.0, 2.4), yaw=-90.0, pitch=0.0)


def best_of(fn, repeats):
    """The shortest wall time of `repeats` runs of fn (seconds), after one run to warm up, and the last result."""
    out = fn()
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return min(times), out


def overhead(t, w, h, shade, passes, spp, repeats, rad_ptr):
    cam = c2(w, h)
    frame = lib.render_params(w, h, 8, spp, 1234, shade_mode=shade)
    whole = lib.render_params(w, h, 8, spp * passes, 1234, shade_mode=shade)
    res = {}
    for tile in (32, 64, 128):
        ap = lib.adaptive_params(tile=tile, min_passes=2, max_passes=passes, threshold=0.0)
        sec, info = best_of(lambda: t.render_adaptive_device(cam, frame, ap, None, rad_ptr, None), repeats)
        assert info.passes_run == passes and info.rectangles == passes
        res[f"adaptive_t{tile}_s"] = round(sec, 4)

    def prog():
        for k in range(passes):
            lib.check(t._lib.ff_render_progressive(t._state, C.byref(cam), C.byref(frame), k, None, 1, C.c_void_p(rad_ptr), 1))

    res["progressive_s"] = round(best_of(prog, repeats)[0], 4)
    res["one_frame_s"] = round(best_of(lambda: t.render_device(cam, whole, None, rad_ptr), repeats)[0], 4)
    for tile in (32, 64, 128):
        res[f"adaptive_t{tile}_over_progressive"] = round(res[f"adaptive_t{tile}_s"] / res["progressive_s"], 4)
    res["progressive_over_one_frame"] = round(res["progressive_s"] / res["one_frame_s"], 4)
    return res


def quality(t, shade, budget, ref_spp, repeats, w=480, h=270):
    cam = c2(w, h)
    params = lambda spp, seed=1234: lib.render_params(w, h, 8, spp, seed, shade_mode=shade)  # noqa: E731
    t0 = time.perf_counter()
    truth = t.render(cam, params(ref_spp, 777), want_rgb8=False)[1].astype(np.float64)
    res = {"width": w, "height": h, "truth_spp": ref_spp, "truth_s": round(time.perf_counter() - t0, 2), "budget_spp": budget}
    mse = lambda a: float(np.mean((a.astype(np.float64) - truth) ** 2))  # noqa: E731
    # the uniform frames' curve: spp -> (seconds, MSE)
    curve = {}
    spp = budget
    while spp >= max(8, budget // 64):
        sec, out = best_of(lambda: t.render(cam, params(spp), want_rgb8=False), repeats)
        curve[spp] = (sec, mse(out[1]))
        spp //= 2
    res["uniform"] = {str(k): {"s": round(v[0], 4), "mse": v[1]} for k, v in curve.items()}
    xs = sorted(curve)
    log_t = np.log([curve[k][0] for k in xs])
    log_m = np.log([curve[k][1] for k in xs])
    log_s = np.log(xs)
    uniform_s, uniform_mse = curve[budget]
    sweep = {}
    for tile in (32, 64, 128):
        for threshold in (0.0, 5e-5, 1e-4, 2e-4, 4e-4, 8e-4, 1.6e-3, 3.2e-3):
            for pass_spp in (16, 64):
                ap = lib.adaptive_params(tile=tile, min_passes=2, max_passes=budget // pass_spp, threshold=threshold)
                sec, out = best_of(lambda: t.render_adaptive(cam, params(pass_spp), ap), repeats)
                info = out[3]
                m = mse(out[1])
                # equal time: the uniform frame of the sample count that takes this call's time (interpolated), rendered and measured
                eq_spp = int(round(float(np.exp(np.interp(np.log(sec), log_t, log_s)))))
                eq_spp = max(1, min(budget, eq_spp))
                eq_mse = mse(t.render(cam, params(eq_spp), want_rgb8=False)[1])
                # equal quality: the time of the uniform frame that reaches this MSE (the MSE falls as time grows: interpolate on -log mse)
                eq_time = float(np.exp(np.interp(-np.log(m), -log_m, log_t))) if m > 0 else None
                sweep[f"t{tile}_thr{threshold:g}_spp{pass_spp}"] = {
                    "s": round(sec, 4), "s_over_uniform": round(sec / uniform_s, 4), "samples_over_uniform": round(info.samples / (w * h * budget), 4),
                    "rectangles": info.rectangles, "passes_run": info.passes_run, "stopped_early": info.tiles_stopped_early, "tiles": info.tiles,
                    "mse": m, "mse_over_uniform": round(m / uniform_mse, 4), "equal_time_uniform_spp": eq_spp, "equal_time_uniform_mse": eq_mse,
                    "equal_time_mse_ratio": round(m / eq_mse, 4), "equal_quality_uniform_s": None if eq_time is None else round(eq_time, 4),
                    "equal_quality_time_ratio": None if eq_time is None else round(sec / eq_time, 4)}
    res["sweep"] = sweep
    best = min(sweep, key=lambda k: sweep[k]["equal_time_mse_ratio"])
    res["best_equal_time"] = {"case": best, **sweep[best]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--passes", type=int, default=16)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--budget", type=int, default=1024)
    ap.add_argument("--ref-spp", type=int, default=16384)
    ap.add_argument("--modes", default="path,nee")
    ap.add_argument("--no-overhead", action="store_true")
    ap.add_argument("--no-quality", action="store_true", help="skip the 480x270 sweep")
    args = ap.parse_args()
    W, H = args.width, args.height
    res = {"scene": "cornell_wahoo C2 pose, 8 bounces", "width": W, "height": H, "passes": args.passes, "spp": args.spp, "repeats": args.repeats}
    with lib.Tracer(0) as t:
        t.set_stream(torch.cuda.current_stream().cuda_stream)
        t.upload_scene(scenes.cornell_wahoo_scene())
        rad = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        for name in args.modes.split(","):
            shade = MODES[name]
            if not args.no_overhead:
                res[f"overhead_{name}"] = overhead(t, W, H, shade, args.passes, args.spp, args.repeats, rad.data_ptr())
                print(f"overhead_{name}", res[f"overhead_{name}"], flush=True)
            if not args.no_quality:
                q = quality(t, shade, args.budget, args.ref_spp, args.repeats)
                res[f"quality_{name}"] = q
                for key, val in q.items():
                    if key == "sweep":
                        for k2, v2 in val.items():
                            print(f"  {name} sweep {k2:24s} {v2}", flush=True)
                    else:
                        print(f"  {name} {key:20s} {val}", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
