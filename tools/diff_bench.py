#!/usr/bin/env python3
"""What a motion-tracker step costs (oatgpu_diff_batch_dev / oatgpu_diff_sequence_dev, kernels_diff.hip) against the way the
same work had to be done before it: per camera stream `oatgpu_cvt_color` BGR -> GREY (BGR cameras only) followed by
`oatgpu_detect_diff`, both on host frames.

    python tools/diff_bench.py [--steps 200] [--warmup 20] [--quick]
    python tools/diff_bench.py --bayer [--steps 200] [--warmup 20] [--quick]      # the RAW8 leg: tools/tracker_bayer_legs.py
    python tools/diff_bench.py --undistort [--steps 200] [--warmup 20] [--quick]  # the lens leg: tools/tracker_undistort_legs.py
    python tools/diff_bench.py --filters [--steps 200] [--warmup 20] [--quick]    # the filter chain: tools/tracker_filters_legs.py

Shapes: 1 x 4K, 16 x 1080p and 1 x 640x480, each with BGR and with GREY frames; diff_threshold 10, blur 2, three moving discs a
camera.  Legs, us a frame set:
  sync      oatgpu_diff_batch_dev, frames in device memory: the median of `steps` calls after `warmup` calls;
  sequence  oatgpu_diff_sequence_dev over `steps` frame sets in one call, divided by `steps`: the median of 5 calls after one
            warm-up call;
  parent    n_streams x (oatgpu_cvt_color + oatgpu_detect_diff) on host frames: the median of `steps` frame sets after
            `warmup`.
Every timed call ends in a device synchronisation, so a host clock around it is the step (the events of a HIP stream would
miss the host's share of 2 n synchronous calls).  The ratio parent / sync is reported, not promised.  Prints one JSON line; the
recipe and the figures' place are in profiles/diff_bench.txt.  Without a GPU the tool fails (no fallback)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("1x4K", 1, 2160, 3840), ("16x1080p", 16, 1080, 1920), ("1x640x480", 1, 480, 640)]
AREA = (20.0, 1e6)


def grey(bgr):
    import numpy as np
    f = bgr.astype(np.uint32)
    return ((1868 * f[..., 0] + 9617 * f[..., 1] + 4899 * f[..., 2] + 8192) >> 14).astype(np.uint8)


def median_us(call, steps, warmup):
    for t in range(warmup):
        call(t)
    d = []
    for t in range(steps):
        t0 = time.perf_counter()
        call(warmup + t)
        d.append(time.perf_counter() - t0)
    return round(statistics.median(d) * 1e6, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="few steps (a rehearsal or a profiler run)")
    ap.add_argument("--bayer", action="store_true", help="the RAW8 leg: demosaic inside the front kernel against oatgpu_debayer_dev + BGR")
    ap.add_argument("--undistort", action="store_true",
                    help="the lens leg: remap inside the front kernel against oatgpu_undistort_dev + the packed call")
    ap.add_argument("--filters", action="store_true", help="the filter chain behind the tracker (kalman, homography, regions) on and off")
    a = ap.parse_args()
    if a.quick:
        a.steps, a.warmup = 16, 4
    import numpy as np
    import torch
    import oat_amd
    if a.filters:
        if not torch.cuda.is_available():
            raise SystemExit("diff_bench: no GPU (nothing is measured without one)")
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import tracker_filters_legs
        make = lambda rows, cols, n: oat_amd.MotionTracker(rows, cols, n_streams=n, channels=3, diff_threshold=10, blur=2, area=AREA)  # noqa: E731
        shapes = tracker_filters_legs.run([({}, make)], a.steps, a.warmup)
        print(json.dumps({"tool": "diff_bench --filters", "unit": "us a frame set, host clock around synchronous calls, median",
                          "library": os.path.relpath(oat_amd.lib_path(), ROOT), "shapes": shapes, "device": torch.cuda.get_device_name(0)}))
        return
    if a.bayer:
        if not torch.cuda.is_available():
            raise SystemExit("diff_bench: no GPU (nothing is measured without one)")
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import tracker_bayer_legs
        shapes = tracker_bayer_legs.run(lambda rows, cols, n: oat_amd.MotionTracker(rows, cols, n_streams=n, channels=3, diff_threshold=10,
                                                                                   blur=2, area=AREA), a.steps, a.warmup)
        print(json.dumps({"tool": "diff_bench --bayer", "unit": "us a frame set, host clock around synchronous calls, median",
                          "library": os.path.relpath(oat_amd.lib_path(), ROOT), "shapes": shapes, "device": torch.cuda.get_device_name(0)}))
        return
    if a.undistort:
        if not torch.cuda.is_available():
            raise SystemExit("diff_bench: no GPU (nothing is measured without one)")
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import tracker_undistort_legs
        make = lambda rows, cols, n: oat_amd.MotionTracker(rows, cols, n_streams=n, channels=3, diff_threshold=10, blur=2, area=AREA)  # noqa: E731
        shapes = tracker_undistort_legs.run([({}, make)], a.steps, a.warmup)
        print(json.dumps({"tool": "diff_bench --undistort", "unit": "us a frame set, host clock around synchronous calls, median",
                          "library": os.path.relpath(oat_amd.lib_path(), ROOT), "shapes": shapes, "device": torch.cuda.get_device_name(0)}))
        return
    from oat_amd import ffi
    from oat_amd.components import PIX_BGR, PIX_GREY
    from oat_amd.synth import make_pool
    if not torch.cuda.is_available():
        raise SystemExit("diff_bench: no GPU (nothing is measured without one)")

    out = []
    for name, n, rows, cols in SHAPES:
        frames = 8
        bgr_pool = np.stack(make_pool(rows, cols, n, frames, n_discs=3))                 # [frames][n][rows][cols][3]
        for ch in (3, 1):
            host = bgr_pool if ch == 3 else grey(bgr_pool)
            dev = torch.from_numpy(host).cuda()
            torch.cuda.synchronize()
            ptrs = [dev[t].data_ptr() for t in range(frames)]
            rec = {"shape": name, "streams": n, "rows": rows, "cols": cols, "channels": ch, "steps": a.steps, "warmup": a.warmup}
            mt = oat_amd.MotionTracker(rows, cols, n_streams=n, channels=ch, diff_threshold=10, blur=2, area=AREA)
            rec["sync_us"] = median_us(lambda t: mt.track_dev(ptrs[t % frames]), a.steps, a.warmup)
            seq = [ptrs[t % frames] for t in range(a.steps)]
            rec["sequence_us"] = round(median_us(lambda t: mt.track_sequence_dev(seq), 5, 1) / a.steps, 1)
            mt.close()
            det = oat_amd.DifferenceDetector(rows, cols, diff_threshold=10, blur=2, area=AREA, n_streams=n)
            tmp = np.empty((rows, cols), np.uint8)
            pos = ffi.Position()

            def parent(t):
                for s in range(n):
                    f = host[t % frames, s]
                    if ch == 3:
                        det._chk(det.lib.oatgpu_cvt_color(det.ctx, PIX_BGR, PIX_GREY, ffi.u8(f), ffi.u8(tmp)))
                        f = tmp
                    det._chk(det.lib.oatgpu_detect_diff(det.ctx, s, ffi.u8(f), C.byref(pos)))
            rec["parent_us"] = median_us(parent, a.steps, a.warmup)
            det.close()
            rec["parent_over_sync"] = round(rec["parent_us"] / rec["sync_us"], 2)
            rec["parent_over_sequence"] = round(rec["parent_us"] / rec["sequence_us"], 2)
            out.append(rec)
            del dev
            torch.cuda.empty_cache()
    print(json.dumps({"tool": "diff_bench", "unit": "us a frame set, host clock around synchronous calls, median",
                      "library": os.path.relpath(oat_amd.lib_path(), ROOT), "shapes": out, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
