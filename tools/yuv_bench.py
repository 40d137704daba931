"""ff_encode_yuv timings on device buffers, with ff_display (ACES + sRGB) as the same-run yardstick.

At the given size (default 1080p), in one process: a 1-spp C2 frame with next-event estimation is rendered, ff_display writes its
display_out (ACES, linear semantics), and ff_encode_yuv turns that into NV12 / BT.709 / LIMITED / LEFT and the radiance itself into
P010 / PQ / BT.2020 / LIMITED / LEFT; NV12 with CENTER siting runs beside them.  Each figure is the median of --repeats windows of
--reps calls, each after warm-up, timed with device events around the window (the spread of the windows is reported) and per call
on the host.  ff_display at its defaults (ACES + sRGB, rgb8 and display_out) runs in the same process, and every figure is also
given as its ratio to that.
Prints human-readable lines, then one JSON line.

    python tools/yuv_bench.py [--width 1920 --height 1080 --reps 200 --warmup 20 --repeats 7]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch  # (before the library: one HIP runtime per process, see tests/conftest.py)
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpupathtracer_amd import lib, scenes  # noqa: E402
from gpupathtracer_amd import types as T  # noqa: E402


def timed(fn, reps, warmup, repeats):
    """`repeats` windows of `reps` calls, each after `warmup` calls -> {event_ms: the median over the windows of device-event ms per
    call, event_ms_min / _max: the spread of the windows, host_median_ms: median host ms per call over all windows}."""
    windows, host = [], []
    for _ in range(repeats):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        begin.record()
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            host.append((time.perf_counter() - t0) * 1e3)
        end.record()
        torch.cuda.synchronize()
        windows.append(begin.elapsed_time(end) / reps)
    return {"event_ms": round(float(np.median(windows)), 5), "event_ms_min": round(min(windows), 5), "event_ms_max": round(max(windows), 5),
            "host_median_ms": round(float(np.median(host)), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7, help="timed windows of --reps calls per case; the median and the spread are reported")
    args = ap.parse_args()
    W, H = args.width, args.height
    res = {"scene": "cornell_wahoo C2 pose, 1-spp NEE", "width": W, "height": H, "reps": args.reps, "repeats": args.repeats}
    with lib.Tracer(0) as t:
        t.set_stream(torch.cuda.current_stream().cuda_stream)
        t.upload_scene(scenes.cornell_wahoo_scene())
        dev = torch.device("cuda")
        rad = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
        shown = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
        rgb8 = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
        cam = scenes.posed_camera(W, H, position=(0.0, 0.0, 2.4), yaw=-90.0, pitch=0.0)
        t.render_device(cam, lib.render_params(W, H, 8, 1, 1234, shade_mode=T.SHADE_DIFFUSE_PATH_NEE), None, rad.data_ptr())
        t.display_device(W, H, rad.data_ptr(), lib.display_params(encoding=T.ENCODE_LINEAR), None, shown.data_ptr())
        torch.cuda.synchronize()
        cases = {
            "encode_yuv_nv12_bt709_left": (shown, lib.yuv_params()),
            "encode_yuv_nv12_bt709_center": (shown, lib.yuv_params(siting=T.YUV_SITING_CENTER)),
            "encode_yuv_p010_pq_bt2020_left": (rad, lib.yuv_params(transfer=T.YUV_TRANSFER_PQ, matrix=T.YUV_MATRIX_BT2020, depth=10)),
        }
        for name, (src, p) in cases.items():
            luma, chroma = t.encode_yuv_device(src, p)
            lb, cb = lib.yuv_plane_bytes(W, H, p)
            call = (t._state, W, H, C.byref(p), C.c_void_p(src.data_ptr()), 1, C.c_void_p(luma.data_ptr()), C.c_void_p(chroma.data_ptr()), 1)
            fn = lambda: lib.check(t._lib.ff_encode_yuv(*call))  # noqa: E731,B023  (the raw call, as the other stages' *_device methods make it)
            res[name] = timed(fn, args.reps, args.warmup, args.repeats)
            res[name]["luma_codes"] = int(torch.unique(luma).numel())
            # compulsory bytes: the float3 image in, the two planes out
            res[name]["floor_ms_at_8TBps"] = round((12 * W * H + lb + cb) / 8.0e12 * 1e3, 5)
        dp = lib.display_params()
        res["display_defaults"] = timed(lambda: t.display_device(W, H, rad.data_ptr(), dp, rgb8.data_ptr(), shown.data_ptr()), args.reps, args.warmup,
                                        args.repeats)
        for name in cases:
            res[name]["over_display"] = round(res[name]["event_ms"] / res["display_defaults"]["event_ms"], 3)
    for key, val in res.items():
        print(f"{key:40s} {val}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
