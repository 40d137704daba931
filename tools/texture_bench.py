"""Albedo textures on C2 (scenes.cornell_wahoo_scene): what the lookup costs a 1-spp FF_SHADE_DIFFUSE_PATH_NEE frame of 8 bounces
and ff_gbuffer.

Three variants of the frame at the given size (default 1080p), device buffers, camera at rest, median over --reps: untextured;
every diffuse geometry bound to a 1024x1024 bilinear texture (scenes.gradient_texture); the same with FF_TEX_NEAREST.  Then
ff_gbuffer with and without the bindings.  Prints human-readable lines, then one JSON line.

    python tools/texture_bench.py [--width 1920 --height 1080 --reps 20 --warmup 3 --texture 1024]
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
    ap.add_argument("--texture", type=int, default=1024, help="side of the square texture")
    args = ap.parse_args()
    W, H = args.width, args.height
    res = {"scene": "C2 cornell_wahoo", "width": W, "height": H, "bounces": 8, "texture": args.texture}
    scene = scenes.cornell_wahoo_scene()
    diffuse = [i for i in range(len(scene)) if scene.geometries[i].m_bxdf.contents.m_type == T.BXDF_DIFFUSE]
    texels = scenes.gradient_texture(args.texture, args.texture)
    with lib.Tracer(0) as t:
        t.upload_scene(scene)
        cam = scenes.posed_camera(W, H, position=(0.0, 0.0, 2.4), yaw=-90.0, pitch=0.0)
        rad = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        gb = {name: torch.zeros((H, W) + shape, dtype=torch.float32 if dt == np.float32 else torch.int32, device="cuda")
              for name, dt, shape in lib.GBUFFER_CHANNELS}
        torch.cuda.synchronize()
        p = lib.render_params(W, H, 8, 1, 1234, shade_mode=NEE)
        render = lambda: t.render_device(cam, p, None, rad.data_ptr())  # noqa: E731
        gbuffer = lambda: t.gbuffer_device(cam, p, *(gb[name].data_ptr() for name, _, _ in lib.GBUFFER_CHANNELS))  # noqa: E731
        textures = {"bilinear": t.create_texture(texels, T.TEX_BILINEAR), "nearest": t.create_texture(texels, T.TEX_NEAREST)}
        for name in ("untextured", "bilinear", "nearest", "untextured_again"):
            for gi in diffuse:
                t.set_albedo_texture(gi, textures.get(name), (4.0, 4.0))
            res[f"ms_1spp_nee_{name}"], res[f"min_ms_1spp_nee_{name}"] = timed(render, args.reps, args.warmup)
            st = t.stats()
            res[f"kernel_ms_1spp_nee_{name}"] = round(float(st.kernel_ms), 4)
            res[f"rays_1spp_nee_{name}"] = int(st.rays_traced)
            res[f"kernel_{name}"] = t.kernel_name()
            res[f"ms_gbuffer_{name}"], res[f"min_ms_gbuffer_{name}"] = timed(gbuffer, args.reps, args.warmup)
    for key, val in res.items():
        print(f"{key:34s} {val}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
