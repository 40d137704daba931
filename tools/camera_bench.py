"""Per-sample camera rays (ff_set_camera_sampling): what a box pixel filter and a thin lens cost a frame of C2 at 8 bounces.

C2 (scenes.cornell_wahoo_scene) without a setting, then with FF_PIXEL_BOX, with a lens (radius 0.05, focused on the back wall's
distance) and with both: ms per 1-spp frame in FF_SHADE_DIFFUSE_PATH and FF_SHADE_DIFFUSE_PATH_NEE (device buffers, camera at rest,
median and minimum over --reps), the kernel each frame launched and a checksum of its radiance; then a 64-spp NEE frame with and
without both - the camera ray's share of an offline render.  FF_SHADE_DIFFUSE_PATH frames move from the mega-kernel to the NEE kernel
under a setting, as they do under a glossy binding: that price is the `path` rows'.  Prints human-readable lines, then one JSON line.

    python tools/camera_bench.py [--width 1920 --height 1080 --reps 20 --warmup 3]

FF_LIB_PATH=<another build of the library> runs the rows without a setting against that build (--plain-only), for a same-box comparison.
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
    ap.add_argument("--plain-only", action="store_true", help="only the frames without a setting (works with an older library)")
    args = ap.parse_args()
    W, H = args.width, args.height
    res = {"width": W, "height": H, "bounces": 8}
    cam = scenes.posed_camera(W, H, position=(0.0, 0.0, 2.4), yaw=-90.0, pitch=0.0)
    with lib.Tracer(0) as t:
        rad = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        def frames(tag, spp=1, modes=(("path", PATH), ("nee", NEE)), reps=args.reps):
            for name, mode in modes:
                p = lib.render_params(W, H, 8, spp, 1234, shade_mode=mode)
                key = f"{spp}spp_{name}_{tag}"
                res[f"ms_{key}"], res[f"min_ms_{key}"] = timed(lambda: t.render_device(cam, p, None, rad.data_ptr()), reps, args.warmup)
                res[f"kernel_{key}"] = t.kernel_name()
                res[f"checksum_{key}"] = float(rad.double().sum().item())

        t.upload_scene(scenes.cornell_wahoo_scene())
        frames("plain")
        if not args.plain_only:
            settings = (("box", lib.camera_sampling(T.PIXEL_BOX)), ("lens", lib.camera_sampling(T.PIXEL_CORNER, 0.05, 4.9)),
                        ("lens_box", lib.camera_sampling(T.PIXEL_BOX, 0.05, 4.9)))
            for tag, cs in settings:
                t.set_camera_sampling(cs)
                frames(tag)
            t.set_camera_sampling(None)
            frames("plain_again")
            few = max(3, args.reps // 4)
            frames("plain", spp=64, modes=(("nee", NEE),), reps=few)
            t.set_camera_sampling(settings[2][1])
            frames("lens_box", spp=64, modes=(("nee", NEE),), reps=few)
            t.set_camera_sampling(None)
    for key, val in res.items():
        print(f"{key:40s} {val}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
