"""Rough-specular (GGX) mirrors: what a glossy floor costs a 1-spp frame of 8 bounces and what next-event estimation buys on it.

Scene A: C2 (scenes.cornell_wahoo_scene) with its floor a mirror, unbound (the perfect mirror: the mega-kernels' frame) and bound at
roughness 0.1 / 0.3 / 0.6: ms per frame in FF_SHADE_DIFFUSE_PATH and FF_SHADE_DIFFUSE_PATH_NEE (device buffers, camera at rest, median
over --reps), and the MSE of a 16-spp frame against --ref-spp samples of the NEE mode, for both modes.  Plain C2, untouched, is timed
next to it: the frame a scene without bindings launches.  Scene B: tools/env_bench.py's scene (wahoo on a floor under a 2048x1024
sun_sky_map) with the mesh a rough conductor at 0.3.  Prints human-readable lines, then one JSON line.

    python tools/glossy_bench.py [--width 1920 --height 1080 --reps 20 --warmup 3 --ref-spp 4096 --no-quality]

FF_LIB_PATH=<another build of the library> runs the plain-C2 rows against that build (--plain-only), for a same-box comparison.
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

NEE, PATH = T.SHADE_DIFFUSE_PATH_NEE, T.SHADE_DIFFUSE_PATH
C2_FLOOR = 3


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def with_bxdf(scene, index, bxdf):
    s = scenes.Scene()
    s._specs = list(scene._specs)
    s._specs[index] = s._specs[index][:5] + (bxdf,)
    return s.finalize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ref-spp", type=int, default=4096)
    ap.add_argument("--no-quality", action="store_true", help="timings only")
    ap.add_argument("--plain-only", action="store_true", help="only the frames of the untouched C2 (works with an older library)")
    args = ap.parse_args()
    W, H = args.width, args.height
    res = {"width": W, "height": H, "bounces": 8}
    cam = scenes.posed_camera(W, H, position=(0.0, 0.0, 2.4), yaw=-90.0, pitch=0.0)
    with lib.Tracer(0) as t:
        rad = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        def frames(tag, camera=cam):
            for name, mode in (("path", PATH), ("nee", NEE)):
                p = lib.render_params(W, H, 8, 1, 1234, shade_mode=mode)
                res[f"ms_1spp_{name}_{tag}"], res[f"min_ms_1spp_{name}_{tag}"] = timed(lambda: t.render_device(camera, p, None, rad.data_ptr()), args.reps, args.warmup)
                res[f"kernel_{name}_{tag}"] = t.kernel_name()

        t.upload_scene(scenes.cornell_wahoo_scene())
        frames("plain_c2")
        if not args.plain_only:
            floor = scenes.make_bxdf(T.BXDF_MIRROR, specular=(0.9, 0.85, 0.75))
            t.upload_scene(with_bxdf(scenes.cornell_wahoo_scene(), C2_FLOOR, floor))
            frames("mirror_floor")
            for rough in (0.1, 0.3, 0.6):
                t.set_roughness(C2_FLOOR, rough)
                tag = f"rough_{rough}"
                frames(tag)
                if args.no_quality:
                    continue
                t0 = time.perf_counter()
                ref = t.render(cam, lib.render_params(W, H, 8, args.ref_spp, 77, shade_mode=NEE))[1].astype(np.float64)
                res[f"ref_s_{tag}"] = round(time.perf_counter() - t0, 2)
                for name, mode in (("path", PATH), ("nee", NEE)):
                    img = t.render(cam, lib.render_params(W, H, 8, 16, 7, shade_mode=mode))[1].astype(np.float64)
                    res[f"mse_16spp_{name}_{tag}"] = float(np.mean((img - ref) ** 2))
            t.set_roughness(C2_FLOOR, 0.0)
            # scene B
            mesh = scenes.make_bxdf(T.BXDF_MIRROR, specular=(0.95, 0.64, 0.54))
            t.upload_scene(with_bxdf(scenes.open_floor_scene(), 0, mesh))
            t.set_environment(scenes.sun_sky_map(2048, 1024))
            cam_b = scenes.posed_camera(W, H, position=(0.0, -1.2, 3.0), yaw=-90.0, pitch=0.0)
            frames("env_mirror_mesh", cam_b)
            t.set_roughness(0, 0.3)
            frames("env_rough_0.3", cam_b)
            t.clear_environment()
            t.upload_scene(scenes.cornell_wahoo_scene())
            frames("plain_c2_again")
    for key, val in res.items():
        print(f"{key:40s} {val}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
