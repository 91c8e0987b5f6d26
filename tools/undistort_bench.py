#!/usr/bin/env python3
"""Throughput of `framefilt undistort` on the device entry (oatgpu_undistort_dev: every stream's frame in ONE launch).

    python tools/undistort_bench.py [--iters N] [--quick]

Shapes: 4 x 4K (the headline: about 400 MB of maps and frames a launch, more than the 256 MiB Infinity Cache), 1 x 4K
(its map and frame stay resident in the Infinity Cache: reported beside the headline, labelled), 16 x 1080p, 1 x 640x480.
Every shape is created and warmed up first; each is then timed with HIP events around N back-to-back launches on the
context's own stream.  Bytes by the byte model of DESIGN.md section 9: per output pixel 6 B of map (sx, sy shorts + the
fraction ushort) + channels B written + channels B of source read at least once (the 2x2 gather is reused through
L1 / L2).  Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ACHIEVABLE_TBPS = 6.3      # MI355X HBM, achievable by a streaming kernel
PEAK_TBPS = 8.0

SHAPES = [("4x4K", 4, 2160, 3840), ("1x4K", 1, 2160, 3840), ("16x1080p", 16, 1080, 1920), ("1x640x480", 1, 480, 640)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="few launches (a profiler run)")
    a = ap.parse_args()
    if a.quick:
        a.iters, a.warmup = 20, 5
    import torch
    import oat_amd
    import undistort_ref as R

    runs = []
    for name, n, rows, cols in SHAPES:            # create + warm every shape first
        K, D = R.cases(rows, cols)["mild5"]
        ud = oat_amd.Undistorter(rows, cols, K, D, channels=3, n_streams=n)
        fin = torch.randint(0, 256, (n, rows, cols, 3), dtype=torch.uint8, device="cuda")
        fout = torch.empty_like(fin)
        torch.cuda.synchronize()
        for _ in range(a.warmup):
            ud.filter_dev(fin.data_ptr(), fout.data_ptr())
        ud.synchronize()
        runs.append((name, n, rows, cols, ud, fin, fout))

    out = []
    for name, n, rows, cols, ud, fin, fout in runs:
        st = torch.cuda.ExternalStream(ud.get_stream())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(a.iters):
            ud.filter_dev(fin.data_ptr(), fout.data_ptr())
        e1.record(st)
        e1.synchronize()
        us = e0.elapsed_time(e1) * 1000.0 / a.iters
        npx = n * rows * cols
        nbytes = npx * (6 + 3 + 3)
        tbps = nbytes / (us * 1e-6) / 1e12
        out.append({"shape": name, "streams": n, "rows": rows, "cols": cols, "channels": 3, "calibration": "mild5",
                    "us_per_launch": round(us, 2), "frames_per_s": round(n * 1e6 / us, 1),
                    "stream_fps": round(1e6 / us, 1), "model_bytes": nbytes, "model_TBps": round(tbps, 3),
                    "of_achievable_6p3": round(tbps / ACHIEVABLE_TBPS, 3), "of_peak_8": round(tbps / PEAK_TBPS, 3),
                    "note": "map and frame resident in the 256 MiB Infinity Cache" if name == "1x4K" else ""})
    for r in runs:
        r[4].close()
    head = next(o for o in out if o["shape"] == "4x4K")
    print(json.dumps({"tool": "undistort_bench", "iters": a.iters, "headline": head, "shapes": out,
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
