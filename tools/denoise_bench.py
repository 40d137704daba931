"""G-buffer and denoiser timings on the C2 scene (cornell_wahoo at the C2 pose) and the error the filter removes.

Reports, at the given size (default 1080p): ff_gbuffer resolving the stored primary hits of a frame at rest and tracing its own
pre-pass; ff_denoise at the default passes on device buffers; one 1-spp 8-bounce frame at rest for scale; the compulsory bytes
of an à-trous pass (32 B of guides, 16 B of colour read and 16 B written per pixel) against 8 TB/s; and the MSE of a 16-spp frame
before and after the filter against a 4 096-spp frame at 320x180.  Every call is synchronous; times are host clock around
single calls after warm-up (median over --reps).  Prints human-readable lines, then one JSON line.

    python tools/denoise_bench.py [--width 1920 --height 1080 --reps 30 --warmup 5]
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

HBM_BYTES_PER_S = 8.0e12


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def c2(w, h, yaw=-90.0):
    return scenes.posed_camera(w, h, position=(0.0, 0.0, 2.4), yaw=yaw, pitch=0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=None, help="à-trous passes (default: ff_denoise_params_init's)")
    ap.add_argument("--no-quality", action="store_true", help="skip the 320x180 MSE measurement")
    args = ap.parse_args()
    W, H = args.width, args.height
    dn = lib.denoise_params() if args.iterations is None else lib.denoise_params(iterations=args.iterations)
    scene = scenes.cornell_wahoo_scene()
    cam = c2(W, H)
    res = {"scene": "cornell_wahoo C2 pose", "width": W, "height": H, "iterations": dn.iterations, "sigma_color": dn.sigma_color,
           "sigma_normal": dn.sigma_normal, "sigma_plane": dn.sigma_plane}
    with lib.Tracer(0) as t:
        t.upload_scene(scene)
        dev = torch.device("cuda")
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
        depth, pos, nrm, alb = f32(H, W), f32(H, W, 3), f32(H, W, 3), f32(H, W, 3)
        ids = torch.zeros((H, W, 3), dtype=torch.int32, device=dev)
        rgb8 = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
        rad, out = f32(H, W, 3), f32(H, W, 3)
        torch.cuda.synchronize()
        frame = lib.render_params(W, H, 8, 1, 1234)
        # the 1-spp frame with the camera at rest (its primary hits stored and kept from frame to frame)
        res["frame_1spp_at_rest_ms"], _ = timed(lambda: t.render_device(cam, frame, rgb8.data_ptr(), rad.data_ptr()), args.reps, args.warmup)
        gbuf = lambda c: t.gbuffer_device(c, frame, depth.data_ptr(), pos.data_ptr(), nrm.data_ptr(), alb.data_ptr(), ids.data_ptr())  # noqa: E731
        res["gbuffer_kept_hits_ms"], res["gbuffer_kept_hits_min_ms"] = timed(lambda: gbuf(cam), args.reps, args.warmup)
        # from scratch: two cameras that no frame has stored hits for, alternately (each call runs its own pre-pass)
        others = [c2(W, H, -90.001), c2(W, H, -89.999)]
        k = [0]

        def fresh():
            k[0] ^= 1
            gbuf(others[k[0]])
        res["gbuffer_from_scratch_ms"], res["gbuffer_from_scratch_min_ms"] = timed(fresh, args.reps, args.warmup)
        gbuf(cam)
        den = lambda: t.denoise_device(W, H, rad.data_ptr(), pos.data_ptr(), nrm.data_ptr(), alb.data_ptr(), ids.data_ptr(), dn,  # noqa: E731
                                       rgb8.data_ptr(), out.data_ptr())
        res["denoise_ms"], res["denoise_min_ms"] = timed(den, args.reps, args.warmup)
        px = W * H
        res["pass_compulsory_bytes"] = 64 * px
        res["pass_floor_ms_at_8TBps"] = round(64 * px / HBM_BYTES_PER_S * 1e3, 4)
        res["denoise_floor_ms_at_8TBps"] = round(dn.iterations * 64 * px / HBM_BYTES_PER_S * 1e3 + (60 + 16 + 15) * px / HBM_BYTES_PER_S * 1e3, 4)
        res["gbuffer_resolve_bytes"] = (48 + 52) * px
        if not args.no_quality:
            w, h = 320, 180
            qc = c2(w, h)
            gb = t.gbuffer(qc, lib.render_params(w, h))
            _, ref = t.render(qc, lib.render_params(w, h, 8, 4096, 77))
            _, noisy = t.render(qc, lib.render_params(w, h, 8, 16, 5))
            _, d = t.denoise(noisy, gb, dn)
            mse = lambda a: float(np.mean((a.astype(np.float64) - ref) ** 2))  # noqa: E731
            res["mse_raw_16spp"], res["mse_denoised_16spp"] = mse(noisy), mse(d)
            res["mse_factor"] = round(mse(d) / mse(noisy), 4)
    for key, v in res.items():
        print(f"{key:32s} {v}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
