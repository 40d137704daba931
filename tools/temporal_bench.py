"""Temporal denoiser timings on the C2 scene (cornell_wahoo at the C2 pose) and the error it removes from a moving camera's 1-spp
frames.

Reports, at the given size (default 1080p): ff_denoise_temporal on device buffers along a sliding camera (2 px per call; every
pose has its own 1-spp frame and G-buffer, rendered before the timed region, so reprojection, tap validity and the share of
short histories are those of a real moving camera); one moving-camera viewer frame (a 1-spp 8-bounce ff_render, ff_gbuffer
with its own pre-pass, ff_denoise_temporal); the compulsory bytes of each kernel against 8 TB/s; and, at 320x180, the MSE of 16
sliding 1-spp frames against a 4 096-spp frame of the final pose for ff_denoise of the last frame and for the temporal filter
over a max_history sweep.  Every call is synchronous; times are host clock around single calls after warm-up (median over
--reps).  Prints human-readable lines, then one JSON line.  The per-kernel split comes from a separate run under
`rocprofv3 --kernel-trace --stats` with --no-quality.

    python tools/temporal_bench.py [--width 1920 --height 1080 --reps 30 --warmup 5]
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


def c2(w, h, x=0.0, yaw=-90.0):
    return scenes.posed_camera(w, h, position=(x, 0.0, 2.4), yaw=yaw, pitch=0.0)


def quality(t, sweep):
    """MSE against 4 096 spp after 16 sliding 1-spp frames at 320x180: ff_denoise of the last frame and the temporal filter."""
    w, h = 320, 180
    t.upload_scene(scenes.cornell_wahoo_scene())
    poses = [scenes.posed_camera(w, h, position=(-0.24 + 0.03 * k, 0.0, 2.4), yaw=-90.0 + 0.2 * k, pitch=0.0) for k in range(16)]
    frames = []
    for k, c in enumerate(poses):
        gb = t.gbuffer(c, lib.render_params(w, h))
        _, noisy = t.render(c, lib.render_params(w, h, 8, 1, 1000 + k))
        frames.append((c, gb, noisy))
    _, ref = t.render(poses[-1], lib.render_params(w, h, 8, 4096, 77))
    mse = lambda a: float(np.mean((a.astype(np.float64) - ref) ** 2))  # noqa: E731
    _, den = t.denoise(frames[-1][2], frames[-1][1])
    res = {"mse_raw_1spp": mse(frames[-1][2]), "mse_denoise_1spp": mse(den), "sweep": []}
    for over in sweep:
        tp = lib.temporal_params(**over)
        t.temporal_reset()
        for c, gb, noisy in frames:
            _, out = t.denoise_temporal(noisy, gb, c, tp)
        res["sweep"].append(dict(over, mse=mse(out), factor_vs_denoise=round(mse(out) / mse(den), 4)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-quality", action="store_true", help="skip the 320x180 MSE measurement")
    args = ap.parse_args()
    W, H = args.width, args.height
    tp = lib.temporal_params()
    res = {"scene": "cornell_wahoo C2 pose", "width": W, "height": H,
           "params": {f: getattr(tp, f) for f, _ in tp._fields_}}
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
        # a camera sliding ~2 px per frame at the back wall: every pose's frame and G-buffer is made before the timed calls
        step = 2 * 2 * 4.9 * np.tan(np.radians(22.5)) / H
        poses = [c2(W, H, x=step * j) for j in range(args.warmup + args.reps)]
        gbuf = lambda c: t.gbuffer_device(c, frame, depth.data_ptr(), pos.data_ptr(), nrm.data_ptr(), alb.data_ptr(), ids.data_ptr())  # noqa: E731
        inputs = []
        for j, c in enumerate(poses):
            gbuf(c)
            t.render_device(c, lib.render_params(W, H, 8, 1, 1234 + j), None, rad.data_ptr())
            torch.cuda.synchronize()
            inputs.append([x.clone() for x in (rad, pos, nrm, alb, ids)])
        torch.cuda.synchronize()
        t.temporal_reset()
        k = [-1]

        def temporal():
            k[0] += 1
            r_, p_, n_, a_, i_ = inputs[k[0]]
            t.denoise_temporal_device(poses[k[0]], W, H, r_.data_ptr(), p_.data_ptr(), n_.data_ptr(), a_.data_ptr(), i_.data_ptr(), tp,
                                      rgb8.data_ptr(), out.data_ptr())
        res["temporal_ms"], res["temporal_min_ms"] = timed(temporal, args.reps, args.warmup)
        _, length = t.temporal_history()
        res["last_call_short_history_share"] = round(float(((length > 0) & (length < tp.variance_history)).sum() / max(1, (length > 0).sum())), 4)
        del inputs
        gbuf(poses[0])
        t.render_device(poses[0], frame, None, rad.data_ptr())
        dn = lib.denoise_params()
        res["denoise_ms"], _ = timed(lambda: t.denoise_device(W, H, rad.data_ptr(), pos.data_ptr(), nrm.data_ptr(), alb.data_ptr(), ids.data_ptr(),
                                                              dn, rgb8.data_ptr(), out.data_ptr()), args.reps, args.warmup)
        # one moving-camera viewer frame: 1-spp frame, G-buffer (its own pre-pass: the camera moved), temporal filter
        vposes = [c2(W, H, x=step * j) for j in range(1, 4)]
        v = [0]

        def viewer():
            v[0] = (v[0] + 1) % len(vposes)
            c = vposes[v[0]]
            t.render_device(c, frame, None, rad.data_ptr())
            gbuf(c)
            t.denoise_temporal_device(c, W, H, rad.data_ptr(), pos.data_ptr(), nrm.data_ptr(), alb.data_ptr(), ids.data_ptr(), tp,
                                      rgb8.data_ptr(), out.data_ptr())
        res["viewer_frame_ms"], res["viewer_frame_min_ms"] = timed(viewer, args.reps, args.warmup)
        px = W * H
        # compulsory bytes per pixel: inputs 60 (radiance, position, normal, albedo, ids), previous history 64, writes 72
        # (guides 32, moments 16, colour 16, motion 8) [+16 colour history for feedback_pass -1]; a pass reads 32 of guides and
        # 16 of colour and writes 16 [+16 feedback]; the finish reads 12 + 12 + 16 + 16 and writes 12 + 3
        kb = {"reproject": 60 + 64 + 72, "pass": 64, "pass_with_feedback": 80, "finish": 71}
        res["compulsory_bytes_per_pixel"] = kb
        res["floor_ms_at_8TBps"] = {k_: round(b * px / HBM_BYTES_PER_S * 1e3, 4) for k_, b in kb.items()}
        res["call_floor_ms_at_8TBps"] = round((kb["reproject"] + kb["pass_with_feedback"] + (tp.iterations - 1) * kb["pass"] + kb["finish"]) * px
                                              / HBM_BYTES_PER_S * 1e3, 4)
        if not args.no_quality:
            res["quality_320x180"] = quality(t, [{"max_history": m} for m in (4, 8, 16, 32, 64)] +
                                             [{"feedback_pass": -1}, {"iterations": 4}, {"sigma_luminance": 2.0}, {"sigma_luminance": 8.0}])
    for key, val in res.items():
        print(f"{key:28s} {val}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
