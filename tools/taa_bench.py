"""Temporal anti-aliasing timings on the C2 scene (cornell_wahoo at the C2 pose) and the aliasing it removes.

Reports, at the given size (default 1080p): ff_taa on device buffers along a sliding camera (2 px per call, a new jitter every
call; every pose has its own 1-spp frame and jittered G-buffer, made before the timed region); the compulsory bytes of the call
against 8 TB/s; the cost of a 1-spp frame at rest with a new jitter every frame (the stored primary hits are re-traced) against
one without jitter; and one moving-camera viewer frame end to end (1-spp ff_render, ff_gbuffer, ff_denoise_temporal, ff_taa).
Quality, at 320x180: at rest, NORMAL_DEBUG frames against the mean over a 16x16 jitter grid (32 frames through ff_taa, and the
progressive mean of 16 jittered frames, against the unjittered frame); along temporal_bench.py's 16-frame sliding path, the MSE
of SVGF + TAA and of SVGF alone against an anti-aliased reference (the progressive mean over a 16x16 jitter grid at 16 spp per
jitter).  Every call is synchronous; times are host clock around single calls after warm-up (median over --reps).  Prints
human-readable lines, then one JSON line.  The per-kernel split comes from a separate run under
`rocprofv3 --kernel-trace --stats` with --no-quality.

    python tools/taa_bench.py [--width 1920 --height 1080 --reps 30 --warmup 5]
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


def c2(w, h, x=0.0, yaw=-90.0):
    return scenes.posed_camera(w, h, position=(x, 0.0, 2.4), yaw=yaw, pitch=0.0)


def grid_jitters(n=16):
    return [((i + 0.5) / n, (j + 0.5) / n) for j in range(n) for i in range(n)]


def quality_at_rest(t, w=320, h=180):
    c = c2(w, h)
    dbg = lib.render_params(w, h, 1, 1, 1, shade_mode=T.SHADE_NORMAL_DEBUG)
    S = np.zeros((h, w, 3))
    for j in grid_jitters():
        t.set_pixel_jitter(*j)
        S += t.render(c, dbg)[1]
    S /= 256
    t.set_pixel_jitter(0.0, 0.0)
    plain = t.render(c, dbg)[1]
    t.taa_reset()
    acc = np.zeros((h, w, 3))
    for f in range(32):
        t.set_pixel_jitter(*lib.jitter_sequence(f, 16))
        frame = t.render(c, dbg)[1]
        gb = t.gbuffer(c, lib.render_params(w, h))
        if f < 16:
            acc += frame
        out = t.taa(frame, gb, c)[1]
    t.set_pixel_jitter(0.0, 0.0)
    mse = lambda a: float(np.mean((a.astype(np.float64) - S) ** 2))  # noqa: E731
    return {"mse_unjittered": mse(plain), "mse_taa_32": mse(out), "factor_taa": round(mse(out) / mse(plain), 4),
            "mse_mean_16": mse(acc / 16), "factor_mean_16": round(mse(acc / 16) / mse(plain), 4)}


def quality_sliding(t, w=320, h=180):
    poses = [scenes.posed_camera(w, h, position=(-0.24 + 0.03 * k, 0.0, 2.4), yaw=-90.0 + 0.2 * k, pitch=0.0) for k in range(16)]
    t.temporal_reset()
    t.taa_reset()
    svgf_only = lib.Tracer(0)
    svgf_only.upload_scene(scenes.cornell_wahoo_scene())
    try:
        for k, c in enumerate(poses):
            # SVGF alone: unjittered frames
            gb0 = svgf_only.gbuffer(c, lib.render_params(w, h))
            _, noisy0 = svgf_only.render(c, lib.render_params(w, h, 8, 1, 1000 + k))
            _, svgf = svgf_only.denoise_temporal(noisy0, gb0, c)
            # SVGF + TAA: jittered frames
            t.set_pixel_jitter(*lib.jitter_sequence(k, 16))
            gb = t.gbuffer(c, lib.render_params(w, h))
            _, noisy = t.render(c, lib.render_params(w, h, 8, 1, 1000 + k))
            _, den = t.denoise_temporal(noisy, gb, c)
            _, taa = t.taa(den, gb, c)
    finally:
        svgf_only.close()
    ref = np.zeros((h, w, 3))
    for j in grid_jitters():
        t.set_pixel_jitter(*j)
        ref += t.render(poses[-1], lib.render_params(w, h, 8, 16, 77))[1]
    ref /= 256
    t.set_pixel_jitter(0.0, 0.0)
    mse = lambda a: float(np.mean((a.astype(np.float64) - ref) ** 2))  # noqa: E731
    return {"mse_svgf": mse(svgf), "mse_svgf_taa": mse(taa), "factor_svgf_taa_vs_svgf": round(mse(taa) / mse(svgf), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-quality", action="store_true", help="skip the 320x180 MSE measurements")
    args = ap.parse_args()
    W, H = args.width, args.height
    p = lib.taa_params()
    res = {"scene": "cornell_wahoo C2 pose", "width": W, "height": H, "params": {f: getattr(p, f) for f, _ in p._fields_}}
    with lib.Tracer(0) as t:
        t.upload_scene(scenes.cornell_wahoo_scene())
        dev = torch.device("cuda")
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
        depth, pos, nrm, alb = f32(H, W), f32(H, W, 3), f32(H, W, 3), f32(H, W, 3)
        ids = torch.zeros((H, W, 3), dtype=torch.int32, device=dev)
        rgb8 = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
        rad, out = f32(H, W, 3), f32(H, W, 3)
        torch.cuda.synchronize()
        frame = lib.render_params(W, H, 8, 1, 1234)
        step = 2 * 2 * 4.9 * np.tan(np.radians(22.5)) / H
        poses = [c2(W, H, x=step * j) for j in range(args.warmup + args.reps)]
        gbuf = lambda c: t.gbuffer_device(c, frame, depth.data_ptr(), pos.data_ptr(), nrm.data_ptr(), alb.data_ptr(), ids.data_ptr())  # noqa: E731
        inputs = []
        for j, c in enumerate(poses):
            t.set_pixel_jitter(*lib.jitter_sequence(j, 16))
            gbuf(c)
            t.render_device(c, lib.render_params(W, H, 8, 1, 1234 + j), None, rad.data_ptr())
            torch.cuda.synchronize()
            inputs.append([x.clone() for x in (rad, pos, ids)])
        torch.cuda.synchronize()
        t.taa_reset()
        k = [-1]

        def taa():
            k[0] += 1
            r_, p_, i_ = inputs[k[0]]
            t.taa_device(poses[k[0]], W, H, r_.data_ptr(), p_.data_ptr(), i_.data_ptr(), p, rgb8.data_ptr(), out.data_ptr())
        res["taa_ms"], res["taa_min_ms"] = timed(taa, args.reps, args.warmup)
        _, length = t.taa_history()
        res["last_call_valid_history_share"] = round(float((length > 1).mean()), 4)
        del inputs
        # 1-spp frames at rest: a new jitter every frame (the stored hits are re-traced) against no jitter (they are kept)
        c = poses[0]
        t.set_pixel_jitter(0.0, 0.0)
        res["frame_at_rest_no_jitter_ms"], _ = timed(lambda: t.render_device(c, frame, None, rad.data_ptr()), args.reps, args.warmup)
        jn = [0]

        def jittered_frame():
            jn[0] += 1
            t.set_pixel_jitter(*lib.jitter_sequence(jn[0], 16))
            t.render_device(c, frame, None, rad.data_ptr())
        res["frame_at_rest_new_jitter_ms"], _ = timed(jittered_frame, args.reps, args.warmup)
        # one moving-camera viewer frame: jitter, 1-spp frame, G-buffer, SVGF, TAA
        vposes = [c2(W, H, x=step * j) for j in range(1, 4)]
        v = [0]
        tp = lib.temporal_params()

        def viewer():
            v[0] += 1
            c_ = vposes[v[0] % len(vposes)]
            t.set_pixel_jitter(*lib.jitter_sequence(v[0], 16))
            t.render_device(c_, frame, None, rad.data_ptr())
            gbuf(c_)
            t.denoise_temporal_device(c_, W, H, rad.data_ptr(), pos.data_ptr(), nrm.data_ptr(), alb.data_ptr(), ids.data_ptr(), tp, None,
                                      rad.data_ptr())
            t.taa_device(c_, W, H, rad.data_ptr(), pos.data_ptr(), ids.data_ptr(), p, rgb8.data_ptr(), out.data_ptr())
        res["viewer_frame_ms"], res["viewer_frame_min_ms"] = timed(viewer, args.reps, args.warmup)
        t.set_pixel_jitter(0.0, 0.0)
        # compulsory bytes per pixel: reads radiance 12, position 12, ids 12, history 16; writes history 16, motion 8, radiance 12,
        # rgb8 3 (the issue's 83 B leaves out the motion buffer)
        b = 12 + 12 + 12 + 16 + 16 + 8 + 12 + 3
        res["compulsory_bytes_per_pixel"] = b
        res["floor_ms_at_8TBps"] = round(b * W * H / HBM_BYTES_PER_S * 1e3, 4)
        if not args.no_quality:
            res["quality_at_rest_320x180"] = quality_at_rest(t)
            res["quality_sliding_320x180"] = quality_sliding(t)
    for key, val in res.items():
        print(f"{key:30s} {val}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
