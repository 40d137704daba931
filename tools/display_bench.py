"""ff_display timings on device buffers, with ff_taa as the same-run yardstick.

At the given size (default 1080p), in one process: (a) CLAMP + LINEAR without flags, (b) the default ACES + SRGB, (c) (b) with
automatic exposure, (d) (c) with bloom, 5 levels; each over --reps calls after warm-up, timed with device events around the whole
run of calls (every call is synchronous, so the figure holds the call's launch and wait, as a viewer pays it) and with the host
clock per call (median).  Beside them ff_taa along tools/taa_bench.py's sliding camera, timed the same way.  The input is a
rendered 8-bounce 1-spp frame of the C2 scene.  Reports the compulsory bytes of each variant and bytes / time against the HBM rate
a float4 copy reaches on this part (6.29 TB/s).  Prints human-readable lines, then one JSON line.  The per-kernel split comes from
a separate run under `rocprofv3 --kernel-trace --stats`.

    python tools/display_bench.py [--width 1920 --height 1080 --reps 200 --warmup 20]
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

HBM_COPY_BYTES_PER_S = 6.29e12


def timed(fn, reps, warmup):
    """-> (device-event ms per call over the run, median host ms per call)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    host = []
    begin.record()
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        host.append((time.perf_counter() - t0) * 1e3)
    end.record()
    torch.cuda.synchronize()
    return begin.elapsed_time(end) / reps, float(np.median(host))


def bloom_bytes(w, h, levels):
    """Compulsory traffic of the pyramid: the bright pass reads the frame once; every level is written once going down and read
    once by the next; going up every level but the last is read and written once more and read once by the finer one."""
    sizes = []
    for _ in range(levels):
        w, h = (w + 1) // 2, (h + 1) // 2
        sizes.append(16 * w * h)
    down = sum(sizes) + sum(sizes[:-1])
    up = sum(2 * s for s in sizes[:-1]) + sum(sizes[1:])
    return down + up + sizes[0]  # (+ the display kernel's read of level 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-taa", action="store_true", help="skip the ff_taa yardstick")
    args = ap.parse_args()
    W, H = args.width, args.height
    px = W * H
    res = {"scene": "cornell_wahoo C2 pose, 8 bounces, 1 spp", "width": W, "height": H, "reps": args.reps}
    with lib.Tracer(0) as t:
        t.set_stream(torch.cuda.current_stream().cuda_stream)
        t.upload_scene(scenes.cornell_wahoo_scene())
        dev = torch.device("cuda")
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)  # noqa: E731
        rad, out = f32(H, W, 3), f32(H, W, 3)
        rgb8 = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
        cam = lambda x=0.0: scenes.posed_camera(W, H, position=(x, 0.0, 2.4), yaw=-90.0, pitch=0.0)  # noqa: E731
        frame = lib.render_params(W, H, 8, 1, 1234)
        t.render_device(cam(), frame, None, rad.data_ptr())
        torch.cuda.synchronize()
        auto, bloom = T.DISPLAY_AUTO_EXPOSURE, T.DISPLAY_BLOOM
        variants = [
            ("a_clamp_linear", lib.display_params(curve=T.CURVE_CLAMP, encoding=T.ENCODE_LINEAR), 15 * px),
            ("b_aces_srgb", lib.display_params(), 15 * px),
            ("c_auto_exposure", lib.display_params(flags=auto, dt=1 / 60), 27 * px + 1024),
            ("d_auto_bloom5", lib.display_params(flags=auto | bloom, dt=1 / 60, bloom_levels=5), 39 * px + 1024 + bloom_bytes(W, H, 5)),
        ]
        for name, p, nbytes in variants:
            t.display_reset()
            call = lambda p=p: t.display_device(W, H, rad.data_ptr(), p, rgb8.data_ptr(), None)  # noqa: E731
            ev, host = timed(call, args.reps, args.warmup)
            res[name] = {"event_ms": round(ev, 5), "host_median_ms": round(host, 5), "bytes": nbytes,
                         "TBps": round(nbytes / (ev * 1e-3) / 1e12, 3), "share_of_copy_rate": round(nbytes / (ev * 1e-3) / HBM_COPY_BYTES_PER_S, 3)}
        # (b) with display_out as well: 27 bytes per pixel
        p = lib.display_params()
        ev, host = timed(lambda: t.display_device(W, H, rad.data_ptr(), p, rgb8.data_ptr(), out.data_ptr()), args.reps, args.warmup)
        res["b_with_display_out"] = {"event_ms": round(ev, 5), "host_median_ms": round(host, 5), "bytes": 27 * px,
                                     "TBps": round(27 * px / (ev * 1e-3) / 1e12, 3)}
        res["b_over_a"] = round(res["b_aces_srgb"]["event_ms"] / res["a_clamp_linear"]["event_ms"], 3)
        if not args.no_taa:
            # tools/taa_bench.py's sliding camera: 2 px per call, a new jitter every call, inputs made before the timed region
            n = args.reps + args.warmup
            pos = f32(H, W, 3)
            ids = torch.zeros((H, W, 3), dtype=torch.int32, device=dev)
            step = 2 * 2 * 4.9 * np.tan(np.radians(22.5)) / H
            poses = [cam(step * j) for j in range(n)]
            inputs = []
            for j, c in enumerate(poses):
                t.set_pixel_jitter(*lib.jitter_sequence(j, 16))
                t.gbuffer_device(c, frame, None, pos.data_ptr(), None, None, ids.data_ptr())
                t.render_device(c, lib.render_params(W, H, 8, 1, 1234 + j), None, rad.data_ptr())
                torch.cuda.synchronize()
                inputs.append([x.clone() for x in (rad, pos, ids)])
            t.set_pixel_jitter(0.0, 0.0)
            t.taa_reset()
            tp = lib.taa_params()
            k = [-1]

            def taa():
                k[0] += 1
                r_, p_, i_ = inputs[k[0]]
                t.taa_device(poses[k[0]], W, H, r_.data_ptr(), p_.data_ptr(), i_.data_ptr(), tp, rgb8.data_ptr(), out.data_ptr())
            ev, host = timed(taa, args.reps, args.warmup)
            res["taa"] = {"event_ms": round(ev, 5), "host_median_ms": round(host, 5), "bytes": 91 * px, "TBps": round(91 * px / (ev * 1e-3) / 1e12, 3)}
            for name, _, _ in variants:
                res[name]["over_taa"] = round(res[name]["event_ms"] / ev, 3)
    for key, val in res.items():
        print(f"{key:22s} {val}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
