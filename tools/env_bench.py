"""Environment lighting on an open scene: wahoo on a floor plane (scenes.open_floor_scene) under a 2048x1024 scenes.sun_sky_map,
8 bounces, FF_SHADE_DIFFUSE_PATH + environment against FF_SHADE_DIFFUSE_PATH_NEE + environment.

Reports, at the given size (default 1080p): ms per 1-spp frame of both modes (device buffers, camera at rest, median over --reps),
the MSE of 1-spp frames (mean over --seeds seeds) against a --ref-spp FF_SHADE_DIFFUSE_PATH_NEE frame, the MSE x time products and
their ratio (the gain at equal time of an unbiased estimator).  Prints human-readable lines, then one JSON line.

    python tools/env_bench.py [--width 1920 --height 1080 --reps 20 --warmup 3 --seeds 4 --ref-spp 4096]
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

PATH, NEE = T.SHADE_DIFFUSE_PATH, T.SHADE_DIFFUSE_PATH_NEE


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seeds", type=int, default=4)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--no-quality", action="store_true", help="timings only")
    args = ap.parse_args()
    W, H = args.width, args.height
    res = {"scene": "wahoo on a floor, sun_sky_map 2048x1024", "width": W, "height": H, "bounces": 8}
    with lib.Tracer(0) as t:
        t.upload_scene(scenes.open_floor_scene())
        t.set_environment(scenes.sun_sky_map(2048, 1024))
        cam = scenes.posed_camera(W, H, position=(0.0, -1.2, 3.0), yaw=-90.0, pitch=0.0)
        rad = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for name, mode in (("path_env", PATH), ("nee_env", NEE)):
            p = lib.render_params(W, H, 8, 1, 1234, shade_mode=mode)
            res[f"ms_1spp_{name}"], res[f"min_ms_1spp_{name}"] = timed(lambda: t.render_device(cam, p, None, rad.data_ptr()), args.reps, args.warmup)
            st = t.stats()
            res[f"rays_1spp_{name}"] = int(st.rays_traced)
            res[f"kernel_ms_1spp_{name}"] = round(float(st.kernel_ms), 4)
        res["kernel"] = t.kernel_name()
        if not args.no_quality:
            t0 = time.perf_counter()
            _, ref = t.render(cam, lib.render_params(W, H, 8, args.ref_spp, 77, shade_mode=NEE))
            res["ref_spp"] = args.ref_spp
            res["ref_s"] = round(time.perf_counter() - t0, 2)
            ref = ref.astype(np.float64)
            mse = lambda a: float(np.mean((a.astype(np.float64) - ref) ** 2))  # noqa: E731
            for name, mode in (("path_env", PATH), ("nee_env", NEE)):
                res[f"mse_1spp_{name}"] = float(np.mean([mse(t.render(cam, lib.render_params(W, H, 8, 1, 500 + s, shade_mode=mode))[1])
                                                         for s in range(args.seeds)]))
                res[f"mse_x_ms_{name}"] = res[f"mse_1spp_{name}"] * res[f"ms_1spp_{name}"]
            res["mse_ratio_nee_vs_path"] = round(res["mse_1spp_nee_env"] / res["mse_1spp_path_env"], 4)
            res["equal_time_gain"] = round(res["mse_x_ms_path_env"] / res["mse_x_ms_nee_env"], 3)
    for key, val in res.items():
        print(f"{key:28s} {val}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
