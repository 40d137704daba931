"""ff_resize timings on device buffers, with ff_display (ACES + sRGB) as the same-run yardstick.

In one process, on seeded noise images: 3840 x 2160 -> 1920 x 1080 under LANCZOS3 + ANTI_RING and under BOX, 1280 x 720 ->
1920 x 1080 under MITCHELL, and 1920 x 1080 -> 1920 x 1080 under LANCZOS3, each writing the radiance output only.  Each figure is
the median of --repeats windows of --reps calls, each after warm-up, timed with device events around the window (the spread of the
windows is reported) and per call on the host.  Every case is also given as its ratio to its byte floor - the input read and the
intermediate written, the intermediate read and the output written, at --floor-tbps (6.3 TB/s, what a float4 copy reaches) - and
to ff_display at its defaults (rgb8 and display_out) on 1920 x 1080 in the same process.
Prints human-readable lines, then one JSON line.

    python tools/resize_bench.py [--reps 200 --warmup 20 --repeats 7]
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
from gpupathtracer_amd import lib  # noqa: E402
from gpupathtracer_amd import types as T  # noqa: E402

CASES = {
    "resize_2160p_to_1080p_lanczos3_antiring": ((3840, 2160), (1920, 1080), dict(filter=T.RESIZE_LANCZOS3, flags=T.RESIZE_ANTI_RING)),
    "resize_2160p_to_1080p_box": ((3840, 2160), (1920, 1080), dict(filter=T.RESIZE_BOX, flags=T.RESIZE_ANTI_RING)),
    "resize_720p_to_1080p_mitchell": ((1280, 720), (1920, 1080), dict(filter=T.RESIZE_MITCHELL, flags=T.RESIZE_ANTI_RING)),
    "resize_1080p_to_1080p_lanczos3": ((1920, 1080), (1920, 1080), dict(filter=T.RESIZE_LANCZOS3, flags=T.RESIZE_ANTI_RING)),
}


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


def floor_bytes(in_size, out_size):
    """The bytes both passes must move: W x H read and W' x H written, then W' x H read and W' x H' written, 12 bytes a pixel."""
    (w, h), (ow, oh) = in_size, out_size
    return 12 * (w * h + ow * h + ow * h + ow * oh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7, help="timed windows of --reps calls per case; the median and the spread are reported")
    ap.add_argument("--floor-tbps", type=float, default=6.3, help="the bandwidth the byte floor is taken at")
    args = ap.parse_args()
    res = {"input": "seeded noise", "reps": args.reps, "repeats": args.repeats, "floor_tbps": args.floor_tbps}
    with lib.Tracer(0) as t:
        t.set_stream(torch.cuda.current_stream().cuda_stream)
        dev = torch.device("cuda")
        gen = torch.Generator(device=dev).manual_seed(1234)
        for name, (in_size, out_size, fields) in CASES.items():
            (w, h), (ow, oh) = in_size, out_size
            src = torch.rand((h, w, 3), dtype=torch.float32, device=dev, generator=gen) * 2.0
            dst = torch.zeros((oh, ow, 3), dtype=torch.float32, device=dev)
            p = lib.resize_params(**fields)
            torch.cuda.synchronize()
            call = (t._state, C.byref(p), w, h, C.c_void_p(src.data_ptr()), 1, ow, oh, None, 1, C.c_void_p(dst.data_ptr()), 1)
            fn = lambda: lib.check(t._lib.ff_resize(*call))  # noqa: E731,B023  (the raw call, as the other stages' *_device methods make it)
            res[name] = timed(fn, args.reps, args.warmup, args.repeats)
            res[name]["taps"] = [lib.resize_taps(w, ow, p.filter), lib.resize_taps(h, oh, p.filter)]
            res[name]["out_mean"] = round(float(dst.mean()), 6)
            res[name]["floor_mb"] = round(floor_bytes(in_size, out_size) / 1.0e6, 2)
            res[name]["floor_ms"] = round(floor_bytes(in_size, out_size) / (args.floor_tbps * 1.0e12) * 1e3, 5)
            res[name]["over_floor"] = round(res[name]["event_ms"] / res[name]["floor_ms"], 2)
            del src, dst
        W, H = 1920, 1080
        rad = torch.rand((H, W, 3), dtype=torch.float32, device=dev, generator=gen)
        shown = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
        rgb8 = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
        dp = lib.display_params()
        torch.cuda.synchronize()
        res["display_defaults_1080p"] = timed(lambda: t.display_device(W, H, rad.data_ptr(), dp, rgb8.data_ptr(), shown.data_ptr()), args.reps, args.warmup,
                                              args.repeats)
        for name in CASES:
            res[name]["over_display"] = round(res[name]["event_ms"] / res["display_defaults_1080p"]["event_ms"], 3)
    for key, val in res.items():
        print(f"{key:44s} {val}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
