"""Next-event estimation (FF_SHADE_DIFFUSE_PATH_NEE) against FF_SHADE_DIFFUSE_PATH on the C2 scene (cornell_wahoo at the C2 pose),
8 bounces.

Reports, at the given size (default 1080p): ms per 1-spp frame of both modes (device buffers, camera at rest, median over --reps);
the MSE of 1-spp frames (mean over --seeds seeds) against a 4 096-spp FF_SHADE_DIFFUSE_PATH frame, the MSE x time products (the
efficiency of an unbiased estimator: equal time means equal MSE x ms) and a measured equal-time pair (FF_SHADE_DIFFUSE_PATH at the
spp that takes as long as one NEE sample); and, at 320x180, the MSE of ff_denoise_temporal (SVGF) after 16 sliding 1-spp frames
(tools/temporal_bench.py's path) fed by either mode, against 4 096 spp of the final pose.  Prints human-readable lines, then one
JSON line.  The per-kernel split comes from a separate run under `rocprofv3 --kernel-trace --stats` with --no-quality.

    python tools/nee_bench.py [--width 1920 --height 1080 --reps 20 --warmup 3 --seeds 4]
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


def c2(w, h):
    return scenes.posed_camera(w, h, position=(0.0, 0.0, 2.4), yaw=-90.0, pitch=0.0)


def svgf_quality(t):
    """MSE against 4 096 spp after 16 sliding 1-spp frames at 320x180 through ff_denoise_temporal, fed by each mode."""
    w, h = 320, 180
    t.upload_scene(scenes.cornell_wahoo_scene())
    poses = [scenes.posed_camera(w, h, position=(-0.24 + 0.03 * k, 0.0, 2.4), yaw=-90.0 + 0.2 * k, pitch=0.0) for k in range(16)]
    _, ref = t.render(poses[-1], lib.render_params(w, h, 8, 4096, 77))
    mse = lambda a: float(np.mean((a.astype(np.float64) - ref) ** 2))  # noqa: E731
    tp = lib.temporal_params()
    res = {}
    for name, mode in (("path", PATH), ("nee", NEE)):
        t.temporal_reset()
        for k, c in enumerate(poses):
            gb = t.gbuffer(c, lib.render_params(w, h))
            _, noisy = t.render(c, lib.render_params(w, h, 8, 1, 1000 + k, shade_mode=mode))
            _, out = t.denoise_temporal(noisy, gb, c, tp)
        res[f"mse_raw_last_{name}"] = mse(noisy)
        res[f"mse_svgf_{name}"] = mse(out)
    res["svgf_factor_nee_vs_path"] = round(res["mse_svgf_nee"] / res["mse_svgf_path"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seeds", type=int, default=4)
    ap.add_argument("--no-quality", action="store_true", help="timings only (the run rocprofv3 watches)")
    args = ap.parse_args()
    W, H = args.width, args.height
    res = {"scene": "cornell_wahoo C2 pose", "width": W, "height": H, "bounces": 8}
    with lib.Tracer(0) as t:
        t.upload_scene(scenes.cornell_wahoo_scene())
        cam = c2(W, H)
        rad = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for name, mode in (("path", PATH), ("nee", NEE)):
            p = lib.render_params(W, H, 8, 1, 1234, shade_mode=mode)
            res[f"ms_1spp_{name}"], res[f"min_ms_1spp_{name}"] = timed(lambda: t.render_device(cam, p, None, rad.data_ptr()), args.reps, args.warmup)
            st = t.stats()
            res[f"rays_1spp_{name}"] = int(st.rays_traced)
            res[f"kernel_ms_1spp_{name}"] = round(float(st.kernel_ms), 4)
        if not args.no_quality:
            _, ref = t.render(cam, lib.render_params(W, H, 8, 4096, 77))
            ref = ref.astype(np.float64)
            mse = lambda a: float(np.mean((a.astype(np.float64) - ref) ** 2))  # noqa: E731
            for name, mode in (("path", PATH), ("nee", NEE)):
                res[f"mse_1spp_{name}"] = float(np.mean([mse(t.render(cam, lib.render_params(W, H, 8, 1, 500 + s, shade_mode=mode))[1])
                                                         for s in range(args.seeds)]))
                res[f"mse_x_ms_{name}"] = res[f"mse_1spp_{name}"] * res[f"ms_1spp_{name}"]
            res["equal_time_gain"] = round(res["mse_x_ms_path"] / res["mse_x_ms_nee"], 3)
            # measured equal time: the path mode at the spp one NEE sample's time buys
            k = max(1, int(round(res["ms_1spp_nee"] / res["ms_1spp_path"])))
            p = lib.render_params(W, H, 8, k, 1234, shade_mode=PATH)
            res["equal_time_path_spp"] = k
            res["equal_time_path_ms"], _ = timed(lambda: t.render_device(cam, p, None, rad.data_ptr()), max(3, args.reps // 4), 1)
            res["equal_time_path_mse"] = float(np.mean([mse(t.render(cam, lib.render_params(W, H, 8, k, 900 + s, shade_mode=PATH))[1])
                                                        for s in range(args.seeds)]))
            res["svgf_320x180"] = svgf_quality(t)
    for key, val in res.items():
        print(f"{key:28s} {val}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
