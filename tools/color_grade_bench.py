"""ff_color_grade timings on device buffers, with ff_display (ACES + sRGB) as the same-run yardstick.

In one process, on a seeded 1920 x 1080 noise image, writing both outputs (24.9 MB in, 24.9 + 6.2 MB out): the primary grade alone;
with the curves (K = 1024 on the LOG axis); with the lattice at N = 17 from LDS and - on a second state created under
FF_GRADE_NO_LDS - from global memory, at N = 33 and N = 65, tetrahedral and trilinear.  Each figure is the median of --repeats windows
of --reps calls, each after warm-up, timed with device events around the window (the spread of the windows is reported) and per call
on the host.  Every case is also given as its ratio to the byte floor - 56 MB at --floor-tbps (6.3 TB/s, what a float4 copy reaches)
- and to ff_display at its defaults on the same image.  Prints human-readable lines, then one JSON line.

    python tools/color_grade_bench.py [--reps 200 --warmup 20 --repeats 7]
"""
import argparse
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

W, H = 1920, 1080
P, C, L, TRI = T.GRADE_PRIMARY, T.GRADE_CURVES, T.GRADE_LUT3D, T.GRADE_TRILINEAR
PRIMARY = dict(matrix=(1.1, -0.05, 0.02, 0.03, 0.9, -0.01, -0.02, 0.04, 1.25), offset=(-0.02, 0.01, 0.03), saturation=0.7)


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


def make_lut(N, K=1024):
    """A shaper of K knots on the LOG axis (128 to a binade from 2^-4) and an N^3 lattice that desaturates half-way."""
    lo = np.float32(2.0 ** -4)
    hi = (np.array([lo]).view(np.uint32) + np.uint32((K - 1) << 16)).view(np.float32)[0]
    y = np.linspace(0.0, 1.0, K)
    g = np.linspace(0.0, 1.0, N)
    b, gg, r = np.meshgrid(g, g, g, indexing="ij")
    lum = 0.2126 * r + 0.7152 * gg + 0.0722 * b
    table = np.stack([0.5 * (c + lum) for c in (r, gg, b)], axis=-1)
    return lib.grade_lut(curves=np.stack([y, y * y, np.sqrt(y)]), curve_lo=float(lo), curve_hi=float(hi), curve_axis=T.GRADE_AXIS_LOG, curve_shift=16, table=table)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7, help="timed windows of --reps calls per case; the median and the spread are reported")
    ap.add_argument("--floor-tbps", type=float, default=6.3, help="the bandwidth the byte floor is taken at")
    args = ap.parse_args()
    floor_bytes = W * H * (12 + 12 + 3)
    floor_ms = floor_bytes / (args.floor_tbps * 1.0e12) * 1e3
    res = {"input": "seeded noise 1920x1080", "reps": args.reps, "repeats": args.repeats, "floor_tbps": args.floor_tbps, "floor_mb": round(floor_bytes / 1.0e6, 2),
           "floor_ms": round(floor_ms, 5)}
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(1234)
    src = torch.rand((H, W, 3), dtype=torch.float32, device=dev, generator=gen) * 1.5
    dst = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    rgb8 = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    cases = []

    def run(t, name, flags, N):
        lut_id = t.grade_lut_create(make_lut(N)) if N else -1
        p = lib.grade_params(flags=flags, lut_id=lut_id, **PRIMARY)
        res[name] = timed(lambda: t.color_grade_device(W, H, src.data_ptr(), p, rgb8.data_ptr(), dst.data_ptr()), args.reps, args.warmup, args.repeats)
        res[name]["out_mean"] = round(float(dst.mean()), 6)
        res[name]["over_floor"] = round(res[name]["event_ms"] / floor_ms, 2)
        cases.append(name)
        if N:
            t.grade_lut_destroy(lut_id)

    with lib.Tracer(0) as t:
        t.set_stream(torch.cuda.current_stream().cuda_stream)
        run(t, "copy", 0, 0)
        run(t, "primary", P, 0)
        run(t, "primary_curves", P | C, 17)
        for N in (17, 33, 65):
            home = "lds" if N <= T.GRADE_LDS_MAX_SIZE else "global"
            run(t, f"primary_curves_lut{N}_{home}_tetrahedral", P | C | L, N)
            run(t, f"primary_curves_lut{N}_{home}_trilinear", P | C | L | TRI, N)
        run(t, "lut17_lds_tetrahedral", L, 17)
        dp = lib.display_params()
        shown = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        res["display_defaults_1080p"] = timed(lambda: t.display_device(W, H, src.data_ptr(), dp, rgb8.data_ptr(), shown.data_ptr()), args.reps, args.warmup,
                                              args.repeats)
    os.environ["FF_GRADE_NO_LDS"] = "1"   # (read once, at ff_create)
    with lib.Tracer(0) as t:
        t.set_stream(torch.cuda.current_stream().cuda_stream)
        run(t, "primary_curves_lut17_global_tetrahedral", P | C | L, 17)
        run(t, "primary_curves_lut17_global_trilinear", P | C | L | TRI, 17)
        run(t, "lut17_global_tetrahedral", L, 17)
    del os.environ["FF_GRADE_NO_LDS"]
    for name in cases:
        res[name]["over_display"] = round(res[name]["event_ms"] / res["display_defaults_1080p"]["event_ms"], 3)
    for kind in ("primary_curves_lut17_{}_tetrahedral", "primary_curves_lut17_{}_trilinear", "lut17_{}_tetrahedral"):
        res[kind.format("lds_over_global")] = round(res[kind.format("lds")]["event_ms"] / res[kind.format("global")]["event_ms"], 3)
    for key, val in res.items():
        print(f"{key:48s} {val}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
