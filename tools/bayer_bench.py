#!/usr/bin/env python3
"""What Bayer RAW8 ingest (oatgpu_set_track_bayer) costs on the device and what it gains where the PCIe link binds.

    python tools/bayer_bench.py [--calls N] [--steps K] [--quick] [--skip-link]
    python tools/bayer_bench.py --stats KERNEL_STATS.csv     # the demosaic kernels' share of the kernel time, from a
                                                             # rocprofv3 --kernel-trace --stats run of --quick

1. Cost of the stage: oatgpu_track_sequence_dev on device-resident frames, switch off (BGR frames) against on (the RAW8
   frames whose demosaic those BGR frames are, so both legs see the same pixels), 1 x 4K (erode 7, dilate 7), 16 x 1080p and
   1 x 640x480 (erode 3, dilate 7); bench.py's detector window, learning rate, area limits and ring depth.  One context a
   shape, its models aged on the pool first; N sequence calls a leg (default 200), alternating; microseconds a frame set:
   median and 10th / 90th percentile.
2. Gain where the link binds: page-locked host frames through enqueue / collect with the ring kept full, BGR against RAW8,
   8 x 1080p and 16 x 1080p; K steps a run (default 200), three runs a leg, alternating; frames/s and GB/s of frames.
Prints one JSON line."""
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
LINK_SHAPES = [("8x1080p", 8, 1080, 1920), ("16x1080p", 16, 1080, 1920)]
PATTERN = "RGGB"


def demosaic_share(path):
    total = own = 0.0
    with open(path) as f:
        for row in csv.DictReader(f):
            ns = float(row["TotalDurationNs"])
            total += ns
            if "k_debayer" in row["Name"]:
                own += ns
    return {"tool": "bayer_bench", "stats": os.path.basename(path), "debayer_ns": own, "all_kernels_ns": total,
            "debayer_share": round(own / total, 4) if total else None}


def pools(rows, cols, n, frames):
    """(raw [frames][n, rows, cols], bgr [frames][n, rows, cols, 3]) on the device: the mosaic of the synthetic pool and its
    demosaic by the library"""
    import numpy as np
    import torch
    import oat_amd
    import debayer_ref as D
    from oat_amd.synth import make_pool
    raw = torch.from_numpy(np.stack([np.stack([D.mosaic(f, D.RGGB) for f in fs]) for fs in make_pool(rows, cols, n, frames)])).cuda()
    bgr = torch.empty((frames, n, rows, cols, 3), dtype=torch.uint8, device="cuda")
    db = oat_amd.Debayer(rows, cols, n_streams=n, ring_depth=1)
    torch.cuda.synchronize()
    for t in range(frames):
        db.filter_dev(raw[t].data_ptr(), bgr[t].data_ptr(), PATTERN)
    db.synchronize()
    db.close()
    return raw, bgr


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(round(q * (len(v) - 1))))]


def stage_cost(a):
    import torch
    import oat_amd
    from oat_amd.synth import disc_hsv_window
    out = []
    for name, n, rows, cols, ero, dil in SHAPES:
        frames = min(a.frames, max(4, 768 * 1024 * 1024 // (n * rows * cols * 4)))       # (at most ~0.75 GB of pools)
        raw, bgr = pools(rows, cols, n, frames)
        hp = oat_amd.HotPath(rows, cols, n_streams=n, adaptation_coeff=0.01, erode=ero, dilate=dil, area=(20.0, 1e5),
                             ring_depth=8, mog_restore_nmodes=1, **disc_hsv_window())
        ptrs = {0: [bgr[t].data_ptr() for t in range(frames)], 1: [raw[t].data_ptr() for t in range(frames)]}
        for _ in range(3):                                        # age the models and warm both forms up
            for on in (0, 1):
                hp.bayer(PATTERN if on else None)
                hp.track_sequence_dev(ptrs[on])
        us = {0: [], 1: []}
        for _ in range(a.calls):
            for on in (0, 1):
                hp.bayer(PATTERN if on else None)
                t0 = time.perf_counter()
                hp.track_sequence_dev(ptrs[on])
                us[on].append((time.perf_counter() - t0) * 1e6 / frames)
        leg = lambda v: {"median": round(statistics.median(v), 2), "p10": round(pct(v, 0.1), 2), "p90": round(pct(v, 0.9), 2)}
        out.append({"shape": name, "streams": n, "rows": rows, "cols": cols, "frames_a_call": frames, "calls": a.calls,
                    "us_per_set_bgr": leg(us[0]), "us_per_set_raw8": leg(us[1]),
                    "raw8_minus_bgr_us": round(statistics.median(us[1]) - statistics.median(us[0]), 2)})
        hp.close()
        del raw, bgr
        torch.cuda.empty_cache()
    return out


def link_gain(a):
    import numpy as np
    import torch
    import oat_amd
    import debayer_ref as D
    from oat_amd.synth import disc_hsv_window, make_pool
    out = []
    for name, n, rows, cols in LINK_SHAPES:
        sets = 4
        pool = make_pool(rows, cols, n, sets)
        host = {0: [[torch.from_numpy(np.ascontiguousarray(f)).pin_memory().numpy() for f in fs] for fs in pool],
                1: [[torch.from_numpy(D.mosaic(f, D.RGGB)).pin_memory().numpy() for f in fs] for fs in pool]}
        hp = oat_amd.HotPath(rows, cols, n_streams=n, adaptation_coeff=0.01, erode=3, dilate=7, area=(20.0, 1e5), ring_depth=4,
                             mog_restore_nmodes=1, **disc_hsv_window())
        depth = 4

        def run(on, steps):
            hp.bayer(PATTERN if on else None)
            t0 = time.perf_counter()
            for t in range(steps):
                if hp.outstanding() == depth:
                    hp.collect()
                hp.enqueue(host[on][t % sets])
            while hp.outstanding():
                hp.collect()
            return steps * n / (time.perf_counter() - t0)

        for on in (0, 1):
            run(on, 16)
        fps = {0: [], 1: []}
        for _ in range(3):
            for on in (0, 1):
                fps[on].append(run(on, a.steps))
        b, r = statistics.median(fps[0]), statistics.median(fps[1])
        px = rows * cols
        out.append({"shape": name, "streams": n, "steps": a.steps, "runs": 3,
                    "fps_bgr": [round(v, 1) for v in fps[0]], "fps_raw8": [round(v, 1) for v in fps[1]],
                    "GBps_frames_bgr": round(b * px * 3 / 1e9, 2), "GBps_frames_raw8": round(r * px / 1e9, 2),
                    "raw8_over_bgr": round(r / b, 3)})
        hp.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16, help="frame sets in a sequence call")
    ap.add_argument("--calls", type=int, default=200, help="sequence calls a leg")
    ap.add_argument("--steps", type=int, default=200, help="enqueue steps a run of the link legs")
    ap.add_argument("--quick", action="store_true", help="few calls (a profiler run)")
    ap.add_argument("--skip-link", action="store_true")
    ap.add_argument("--stats", help="print the demosaic kernels' share of the kernel time in this rocprofv3 stats file and exit")
    a = ap.parse_args()
    if a.stats:
        print(json.dumps(demosaic_share(a.stats)))
        return
    if a.quick:
        a.calls, a.steps = 2, 16
    import torch
    res = {"tool": "bayer_bench", "pattern": PATTERN, "stage_cost": {"entry": "oatgpu_track_sequence_dev", "unit": "us a frame set", "shapes": stage_cost(a)}}
    if not a.skip_link:
        res["link"] = {"entry": "oatgpu_track_enqueue / _collect, page-locked host frames, ring 4", "shapes": link_gain(a)}
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
