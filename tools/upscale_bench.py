"""Guided upsampling timings on the C2 scene (cornell_wahoo at the C2 pose, 8 bounces, 1-spp FF_SHADE_DIFFUSE_PATH_NEE frames) and
what tracing at half resolution buys and costs.

Reports, for a low frame of half the given size (default 960x540 -> 1920x1080):
(a) ff_upscale alone on device buffers, with ff_taa's time from the same run beside it, and the call's compulsory bytes against
    8 TB/s;
(b) the full-resolution pipeline (1-spp frame, ff_gbuffer, ff_denoise) against the half-resolution one (1-spp frame at low
    resolution, both G-buffers, ff_denoise at low resolution, ff_upscale): total ms of each, stage by stage, and the MSE of both
    results - and of the same low image upsampled bilinearly - against a --ref-spp (default 4 096) full-resolution frame.
Every call is synchronous; times are host clock around single calls after warm-up (median over --reps).  Prints human-readable
lines, then one JSON line.

    python tools/upscale_bench.py [--width 1920 --height 1080 --reps 30 --warmup 5 --ref-spp 4096]
"""
import argparse
import json
import os
import sys
import time

import torch  # (before the library: one HIP runtime per process, see tests/conftest.py)
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from gpupathtracer_amd import lib, scenes  # noqa: E402
from gpupathtracer_amd import types as T  # noqa: E402
from upscale_ref import bilinear_ref  # noqa: E402  (the tests' plain bilinear upsampling on ff_upscale's grid)

HBM_BYTES_PER_S = 8.0e12


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def c2(w, h):
    return scenes.posed_camera(w, h, position=(0.0, 0.0, 2.4), yaw=-90.0, pitch=0.0)


class Buffers:
    """Device images of one size: a G-buffer, radiance in and out."""

    def __init__(self, w, h):
        dev = torch.device("cuda")
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
        self.w, self.h = w, h
        self.depth, self.pos, self.nrm, self.alb = f32(h, w), f32(h, w, 3), f32(h, w, 3), f32(h, w, 3)
        self.ids = torch.zeros((h, w, 3), dtype=torch.int32, device=dev)
        self.rad, self.out = f32(h, w, 3), f32(h, w, 3)
        self.cam = c2(w, h)

    def guides(self):
        return self.pos.data_ptr(), self.nrm.data_ptr(), self.alb.data_ptr(), self.ids.data_ptr()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ref-spp", type=int, default=4096)
    args = ap.parse_args()
    W, H = args.width, args.height
    w, h = W // 2, H // 2
    up, dn, taa = lib.upscale_params(), lib.denoise_params(), lib.taa_params()
    res = {"scene": "cornell_wahoo C2 pose, 8 bounces, 1-spp NEE", "width": W, "height": H, "lo_width": w, "lo_height": h,
           "params": {"sigma_normal": up.sigma_normal, "sigma_plane": up.sigma_plane, "flags": up.flags}}
    with lib.Tracer(0) as t:
        t.upload_scene(scenes.cornell_wahoo_scene())
        hi, lo = Buffers(W, H), Buffers(w, h)
        rgb8 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        frame = lambda b, spp=1, seed=1234: lib.render_params(b.w, b.h, 8, spp, seed, shade_mode=T.SHADE_DIFFUSE_PATH_NEE)  # noqa: E731
        render = lambda b: t.render_device(b.cam, frame(b), None, b.rad.data_ptr())  # noqa: E731
        gbuf = lambda b: t.gbuffer_device(b.cam, frame(b), b.depth.data_ptr(), *b.guides())  # noqa: E731
        denoise = lambda b: t.denoise_device(b.w, b.h, b.rad.data_ptr(), *b.guides(), dn, None, b.out.data_ptr())  # noqa: E731
        upscale = lambda: t.upscale_device(w, h, lo.out.data_ptr(), *lo.guides(), W, H, *hi.guides(), up, rgb8.data_ptr(), hi.out.data_ptr())  # noqa: E731
        for b in (hi, lo):
            render(b)
            gbuf(b)
            denoise(b)
        # (a) the call alone, and ff_taa on the same full-resolution buffers beside it
        res["upscale_ms"] = timed(upscale, args.reps, args.warmup)
        t.taa_reset()
        res["taa_ms"] = timed(lambda: t.taa_device(hi.cam, W, H, hi.rad.data_ptr(), hi.pos.data_ptr(), hi.ids.data_ptr(), taa, rgb8.data_ptr(),
                                                   hi.out.data_ptr()), args.reps, args.warmup)
        # compulsory bytes: per high pixel position, normal, albedo, ids in (48) and radiance, rgb8 out (15); per low pixel the five images once (60)
        nbytes = (48 + 15) * W * H + 60 * w * h
        res["compulsory_bytes"] = nbytes
        res["floor_ms_at_8TBps"] = round(nbytes / HBM_BYTES_PER_S * 1e3, 4)
        # (b) the two pipelines, stage by stage (a camera at rest: ff_gbuffer resolves the stored hits of the frame before it where
        # the sizes match, and traces its own primary rays otherwise - the half-resolution pipeline's full-resolution G-buffer)
        stages = {}
        for name, fn in (("full_frame_ms", lambda: render(hi)), ("full_gbuffer_ms", lambda: gbuf(hi)), ("full_denoise_ms", lambda: denoise(hi)),
                         ("half_frame_ms", lambda: render(lo)), ("half_gbuffer_lo_ms", lambda: gbuf(lo)), ("half_denoise_lo_ms", lambda: denoise(lo))):
            stages[name] = timed(fn, args.reps, args.warmup)
        res.update(stages)

        def full():
            render(hi)
            gbuf(hi)
            denoise(hi)

        def half():
            render(lo)
            gbuf(lo)
            gbuf(hi)
            denoise(lo)
            upscale()
        res["full_pipeline_ms"] = timed(full, args.reps, args.warmup)
        res["half_pipeline_ms"] = timed(half, args.reps, args.warmup)
        res["half_over_full"] = round(res["half_pipeline_ms"] / res["full_pipeline_ms"], 4)
        # quality against a converged full-resolution frame (the last `full` and `half` results are in hi.out; run each once more)
        ref = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        t.render_device(hi.cam, frame(hi, args.ref_spp, 77), None, ref.data_ptr())
        ref = ref.cpu().numpy().astype(np.float64)
        mse = lambda a: float(np.mean((np.asarray(a, np.float64) - ref) ** 2))  # noqa: E731
        full()
        res["mse_full_raw"] = mse(hi.rad.cpu().numpy())
        res["mse_full_denoised"] = mse(hi.out.cpu().numpy())
        half()
        res["mse_half_upscaled"] = mse(hi.out.cpu().numpy())
        res["mse_half_bilinear"] = mse(bilinear_ref(lo.out.cpu().numpy(), H, W))
        res["mse_half_upscaled_over_full_denoised"] = round(res["mse_half_upscaled"] / res["mse_full_denoised"], 4)
        res["mse_half_upscaled_over_bilinear"] = round(res["mse_half_upscaled"] / res["mse_half_bilinear"], 4)
    for key, val in res.items():
        print(f"{key:40s} {val}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
