"""Temporal upsampling timings and quality on the C2 scene (cornell_wahoo at the C2 pose, 8 bounces, 1-spp FF_SHADE_DIFFUSE_PATH_NEE
frames), after tools/upscale_bench.py's method.

Reports, for a low frame of half the given size (default 960x540 -> 1920x1080):
(a) ff_taa_upscale alone on device buffers (history in place, camera at rest), with ff_taa's and ff_upscale's times from the same run
    beside it, and the call's compulsory bytes against 8 TB/s;
(b) a --frames (default 32) sequence at rest, three ways, each result's MSE against a --ref-spp (default 4 096) full-resolution
    frame: half-resolution frames under ff_jitter_sequence(i, 16) through ff_taa_upscale (defaults, and FF_TAA_NO_CLAMP); the
    per-frame ff_upscale pipeline (unjittered half-resolution frame, ff_denoise at low resolution, ff_upscale: the last frame's
    image); full-resolution jittered frames through ff_taa.
Every call is synchronous; times are host clock around single calls after warm-up (median over --reps).  Prints human-readable
lines, then one JSON line.

    python tools/taa_upscale_bench.py [--width 1920 --height 1080 --reps 30 --warmup 5 --frames 32 --ref-spp 4096]
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
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--ref-spp", type=int, default=4096)
    args = ap.parse_args()
    W, H = args.width, args.height
    w, h = W // 2, H // 2
    up, dn, taa = lib.upscale_params(), lib.denoise_params(), lib.taa_params()
    res = {"scene": "cornell_wahoo C2 pose, 8 bounces, 1-spp NEE", "width": W, "height": H, "lo_width": w, "lo_height": h, "frames": args.frames}
    with lib.Tracer(0) as t:
        t.upload_scene(scenes.cornell_wahoo_scene())
        hi, lo, hi_j = Buffers(W, H), Buffers(w, h), Buffers(W, H)  # hi: the unjittered high G-buffer; hi_j: jittered full-resolution frames
        rgb8 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        frame = lambda b, spp=1, seed=1234: lib.render_params(b.w, b.h, 8, spp, seed, shade_mode=T.SHADE_DIFFUSE_PATH_NEE)  # noqa: E731
        render = lambda b, seed=1234: t.render_device(b.cam, frame(b, 1, seed), None, b.rad.data_ptr())  # noqa: E731
        gbuf = lambda b: t.gbuffer_device(b.cam, frame(b), b.depth.data_ptr(), *b.guides())  # noqa: E731
        denoise = lambda b: t.denoise_device(b.w, b.h, b.rad.data_ptr(), *b.guides(), dn, None, b.out.data_ptr())  # noqa: E731
        upscale = lambda: t.upscale_device(w, h, lo.out.data_ptr(), *lo.guides(), W, H, *hi.guides(), up, rgb8.data_ptr(), hi.out.data_ptr())  # noqa: E731

        def taa_upscale(p):
            t.taa_upscale_device(hi.cam, w, h, lo.rad.data_ptr(), lo.ids.data_ptr(), W, H, hi.pos.data_ptr(), hi.ids.data_ptr(), p, rgb8.data_ptr(),
                                 hi.out.data_ptr())

        for b in (hi, lo):
            render(b)
            gbuf(b)
            denoise(b)
        # (a) the call alone, with ff_taa and ff_upscale on the same buffers beside it
        t.taa_upscale_reset()
        res["taa_upscale_ms"] = timed(lambda: taa_upscale(lib.taa_upscale_params()), args.reps, args.warmup)
        res["taa_upscale_bilinear_ms"] = timed(lambda: taa_upscale(lib.taa_upscale_params(flags=T.TAA_BILINEAR)), args.reps, args.warmup)
        t.taa_reset()
        res["taa_ms"] = timed(lambda: t.taa_device(hi.cam, W, H, hi.rad.data_ptr(), hi.pos.data_ptr(), hi.ids.data_ptr(), taa, rgb8.data_ptr(),
                                                   hi.out.data_ptr()), args.reps, args.warmup)
        res["upscale_ms"] = timed(upscale, args.reps, args.warmup)
        # compulsory bytes: per high pixel position and ids in (24), the history in and out (32), the motion (8), radiance and rgb8 out (15);
        # per low pixel radiance and ids once (24)
        nbytes = (24 + 32 + 8 + 15) * W * H + 24 * w * h
        res["compulsory_bytes"] = nbytes
        res["floor_ms_at_8TBps"] = round(nbytes / HBM_BYTES_PER_S * 1e3, 4)
        # (b) quality of a sequence at rest against a converged full-resolution frame
        ref = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        t.render_device(hi.cam, frame(hi, args.ref_spp, 77), None, ref.data_ptr())
        ref = ref.cpu().numpy().astype(np.float64)
        mse = lambda a: float(np.mean((a.cpu().numpy().astype(np.float64) - ref) ** 2))  # noqa: E731
        gbuf(hi)
        for name, flags in (("mse_taa_upscale", 0), ("mse_taa_upscale_no_clamp", T.TAA_NO_CLAMP)):
            t.taa_upscale_reset()
            for i in range(args.frames):
                j = lib.jitter_sequence(i, 16)
                t.set_pixel_jitter(*j)
                render(lo, 2000 + i)
                gbuf(lo)
                t.set_pixel_jitter(0.0, 0.0)
                taa_upscale(lib.taa_upscale_params(flags=flags, lo_jitter=j))
            res[name] = mse(hi.out)
        for i in range(args.frames):  # the per-frame spatial pipeline: every frame stands alone, the last one is measured
            render(lo, 2000 + i)
            gbuf(lo)
            denoise(lo)
            upscale()
        res["mse_upscale_pipeline"] = mse(hi.out)
        t.taa_reset()
        for i in range(args.frames):
            t.set_pixel_jitter(*lib.jitter_sequence(i, 16))
            render(hi_j, 2000 + i)
            gbuf(hi_j)
            t.taa_device(hi_j.cam, W, H, hi_j.rad.data_ptr(), hi_j.pos.data_ptr(), hi_j.ids.data_ptr(), taa, None, hi_j.out.data_ptr())
        t.set_pixel_jitter(0.0, 0.0)
        res["mse_full_taa"] = mse(hi_j.out)
        res["mse_taa_upscale_over_upscale_pipeline"] = round(res["mse_taa_upscale"] / res["mse_upscale_pipeline"], 4)
        res["mse_taa_upscale_over_full_taa"] = round(res["mse_taa_upscale"] / res["mse_full_taa"], 4)
        res["mse_taa_upscale_no_clamp_over_upscale_pipeline"] = round(res["mse_taa_upscale_no_clamp"] / res["mse_upscale_pipeline"], 4)
        res["mse_taa_upscale_no_clamp_over_full_taa"] = round(res["mse_taa_upscale_no_clamp"] / res["mse_full_taa"], 4)
    for key, val in res.items():
        print(f"{key:50s} {val}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
