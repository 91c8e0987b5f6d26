#!/usr/bin/env python3
"""Frame rate of the fused tracker with `framefilt undistort` in front (oatgpu_set_track_undistort), switch off and on.

    python tools/track_undistort_bench.py [--frames N] [--reps R] [--quick]
    python tools/track_undistort_bench.py --stats KERNEL_STATS.csv     # the remap's share of a step, from a
                                                                       # rocprofv3 --kernel-trace --stats run of --quick

Shapes: 1 x 4K (bench.py's headline: erode 7, dilate 7), 16 x 1080p and 1 x 640x480 (erode 3, dilate 7), bench.py's
detector window, learning rate, area limits and ring depth.  Each shape gets ONE context; its models are aged on the frame
pool first, then oatgpu_track_sequence_dev runs the pool R times with the switch off and R times with it on, alternating;
the median of each is reported.  Prints one JSON line."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [("1x4K", 1, 2160, 3840, 7, 7), ("16x1080p", 16, 1080, 1920, 3, 7), ("1x640x480", 1, 480, 640, 3, 7)]


def remap_share(path):
    """kernel time of the tracker's remap (k_undistort_frames) / all kernel time, from rocprofv3's kernel_stats.csv"""
    total = remap = 0.0
    with open(path) as f:
        for row in csv.DictReader(f):
            ns = float(row["TotalDurationNs"])
            total += ns
            if "k_undistort_frames" in row["Name"]:
                remap += ns
    return {"tool": "track_undistort_bench", "stats": os.path.basename(path), "remap_ns": remap, "all_kernels_ns": total,
            "remap_share": round(remap / total, 4) if total else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64, help="frame sets in the pool (one sequence call)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="few frames (a profiler run)")
    ap.add_argument("--stats", help="print the remap's share of the kernel time in this rocprofv3 stats file and exit")
    a = ap.parse_args()
    if a.stats:
        print(json.dumps(remap_share(a.stats)))
        return
    if a.quick:
        a.frames, a.reps = 16, 1
    import torch
    import oat_amd
    import undistort_ref as R
    from oat_amd.synth import disc_hsv_window, make_pool

    out = []
    for name, n, rows, cols, ero, dil in SHAPES:
        hp = oat_amd.HotPath(rows, cols, n_streams=n, adaptation_coeff=0.01, erode=ero, dilate=dil, area=(20.0, 1e5),
                             ring_depth=8, mog_restore_nmodes=1, **disc_hsv_window())
        for s in range(n):
            hp.set_undistort(s, *R.cases(rows, cols)["mild5"])
        frames = min(a.frames, max(8, 1024 * 1024 * 1024 // (n * rows * cols * 3)))     # (at most ~1 GB of pool)
        pool = torch.from_numpy(__import__("numpy").stack(make_pool(rows, cols, n, frames))).cuda()
        ptrs = [pool[t].data_ptr() for t in range(frames)]
        torch.cuda.synchronize()
        hp.track_sequence_dev(ptrs)                               # age the models and warm both forms up
        hp.undistort(True)
        hp.track_sequence_dev(ptrs)
        fps = {0: [], 1: []}
        for _ in range(a.reps):
            for on in (0, 1):
                hp.undistort(bool(on))
                t0 = time.perf_counter()
                hp.track_sequence_dev(ptrs)
                fps[on].append(frames * n / (time.perf_counter() - t0))
        off, on = statistics.median(fps[0]), statistics.median(fps[1])
        out.append({"shape": name, "streams": n, "rows": rows, "cols": cols, "frames": frames, "reps": a.reps,
                    "fps_off": round(off, 1), "fps_on": round(on, 1), "on_over_off": round(on / off, 3)})
        hp.close()
        del pool
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "track_undistort_bench", "entry": "oatgpu_track_sequence_dev", "unit": "frames/s aggregate",
                      "calibration": "mild5", "shapes": out, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
