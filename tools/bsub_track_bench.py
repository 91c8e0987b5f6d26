#!/usr/bin/env python3
"""What a subtraction-tracker step costs (oatgpu_bsub_track_batch_dev / oatgpu_bsub_track_sequence_dev, kernels_bsubtrack.hip)
against the way the same work had to be done before it -- per camera stream `oatgpu_bsub_filter` + `oatgpu_bgr2hsv` +
`oatgpu_detect_hsv`, all on host frames -- and, beside them, the MOG2 chain (`oatgpu_track_sequence_dev`) on the same frames.

    python tools/bsub_track_bench.py [--steps 200] [--warmup 20] [--quick]
    python tools/bsub_track_bench.py --ktrace RESULTS.db      # the kernels of a rocprofv3 --kernel-trace run of --quick
    python tools/bsub_track_bench.py --bayer [--steps 200] [--warmup 20] [--quick]      # the RAW8 leg: tools/tracker_bayer_legs.py
    python tools/bsub_track_bench.py --undistort [--steps 200] [--warmup 20] [--quick]  # the lens leg: tools/tracker_undistort_legs.py
    python tools/bsub_track_bench.py --filters [--steps 200] [--warmup 20] [--quick]    # the filter chain: tools/tracker_filters_legs.py

Shapes: 1 x 4K, 16 x 1080p and 1 x 640x480, BGR frames, alpha 0 and 0.01; the window is V >= 60 on the difference image,
erode 0, dilate 10 (the reference's default), three moving discs a camera.  Legs, us a frame set:
  sync      oatgpu_bsub_track_batch_dev, frames in device memory: median (and 10th / 90th percentile) of `steps` calls after
            `warmup` calls;
  sequence  oatgpu_bsub_track_sequence_dev over `steps` frame sets in one call, divided by `steps`: the median of 5 calls after
            one warm-up call;
  parent    n_streams x (oatgpu_bsub_filter + oatgpu_bgr2hsv + oatgpu_detect_hsv) on host frames: the median of `steps`
            frame sets after `warmup`;
  mog       oatgpu_track_sequence_dev (MOG2 at learning rate 0.01, the same window on the masked frame) over `steps` frame
            sets in one call, divided by `steps`: the median of 5 calls after one.
Every timed call ends in a device synchronisation, so a host clock around it is the step.  The ratios are reported, not
promised.  Prints one JSON line; the recipe and the figures' place are in profiles/bsub_track_bench.txt.  Without a GPU the tool
fails (no fallback)."""
import argparse
import ctypes as C
import json
import os
import re
import sqlite3
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("1x4K", 1, 2160, 3840), ("16x1080p", 16, 1080, 1920), ("1x640x480", 1, 480, 640)]
AREA = (20.0, 1e6)
WINDOW = dict(h_thresh=(0, 256), s_thresh=(0, 256), v_thresh=(60, 256))
ALPHAS = (0.0, 0.01)


def bytes_a_pixel(ch, roi, pair, learn):
    """DESIGN.md 9d's byte model of the front kernel, per pixel and FRAME: frame, background, accumulator, mask words, ROI."""
    nf = 2 if pair else 1
    state = ch * (4 + 4 + 1) if learn else ch            # acc read and written, bg written; or bg read
    return (nf * (ch + 1 / 8) + state + (1 / 8 if roi else 0)) / nf


def ktrace(path):
    """Every kernel of a rocpd database grouped by name and grid; the front kernel against its byte model."""
    db = sqlite3.connect(path)
    rows = db.execute("select s.kernel_name, d.start, d.end, d.grid_size_x, d.grid_size_y from rocpd_kernel_dispatch d "
                      "join rocpd_info_kernel_symbol s on d.kernel_id = s.id order by d.start").fetchall()
    groups = {}
    for name, st, en, gx, gy in rows:
        short = re.sub(r"\(anonymous namespace\)::|oatgpu::|^void |\(.*$", "", name)
        groups.setdefault((short, gx, gy), []).append((en - st) / 1e3)
    out = []
    for (name, gx, gy), d in sorted(groups.items()):
        rec = {"kernel": name, "grid_x_threads": gx, "grid_y": gy, "calls": len(d), "median_us": round(statistics.median(d), 2),
               "min_us": round(min(d), 2), "max_us": round(max(d), 2)}
        m = (re.match(r"k_bsubtrack_(wide|narrow)<(\d), (\w+), (\w+), (\w+)>", name)
             or re.search(r"k_bsubtrack_(wide|narrow)ILi(\d)ELb(\d)ELb(\d)ELb(\d)EE", name))      # (a trace may keep the mangled name)
        raw = (re.match(r"k_bsubtrack_raw_(wide|narrow)<(\w+), (\w+), (\w+)>", name)   # RAW8 frames: 1 byte a pixel in, BGR state
               or re.search(r"k_bsubtrack_raw_(wide|narrow)ILb(\d)ELb(\d)ELb(\d)EE", name))
        if raw:
            roi, pair, learn = (raw.group(i) in ("true", "1") for i in (2, 3, 4))
            px = gx * (4 if raw.group(1) == "wide" else 1) * gy
            mb = px * (bytes_a_pixel(3, roi, pair, learn) - 2) * (2 if pair else 1) / 1e6
            rec.update(model_MB=round(mb, 2), model_TBps=round(mb / rec["median_us"], 3))
        if m:
            ch, roi, pair, learn = int(m.group(2)), m.group(3) in ("true", "1"), m.group(4) in ("true", "1"), m.group(5) in ("true", "1")
            px = gx * (4 if m.group(1) == "wide" else 1) * gy                   # padded pixels of the launch
            mb = px * bytes_a_pixel(ch, roi, pair, learn) * (2 if pair else 1) / 1e6
            rec.update(model_MB=round(mb, 2), model_TBps=round(mb / rec["median_us"], 3))
        out.append(rec)
    return {"tool": "bsub_track_bench", "ktrace": os.path.basename(path), "kernels": out}


def timed_us(call, steps, warmup):
    for t in range(warmup):
        call(t)
    d = []
    for t in range(steps):
        t0 = time.perf_counter()
        call(warmup + t)
        d.append((time.perf_counter() - t0) * 1e6)
    d.sort()
    return round(statistics.median(d), 1), round(d[len(d) // 10], 1), round(d[(9 * len(d)) // 10], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="few steps (a rehearsal or a profiler run)")
    ap.add_argument("--ktrace", help="print the kernels of this rocprofv3 database and exit")
    ap.add_argument("--bayer", action="store_true", help="the RAW8 leg: demosaic inside the front kernel against oatgpu_debayer_dev + BGR")
    ap.add_argument("--undistort", action="store_true",
                    help="the lens leg: remap inside the front kernel against oatgpu_undistort_dev + the packed call")
    ap.add_argument("--filters", action="store_true", help="the filter chain behind the tracker (kalman, homography, regions) on and off")
    a = ap.parse_args()
    if a.ktrace:
        print(json.dumps(ktrace(a.ktrace)))
        return
    if a.quick:
        a.steps, a.warmup = 16, 4
    import numpy as np
    import torch
    import oat_amd
    from oat_amd import ffi
    from oat_amd.synth import make_pool
    if not torch.cuda.is_available():
        raise SystemExit("bsub_track_bench: no GPU (nothing is measured without one)")
    if a.bayer:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import tracker_bayer_legs
        shapes = []
        for alpha in ALPHAS:
            shapes += tracker_bayer_legs.run(lambda rows, cols, n: oat_amd.SubtractionTracker(
                rows, cols, n_streams=n, channels=3, alpha=alpha, erode=0, dilate=10, area=AREA, **WINDOW), a.steps, a.warmup, {"alpha": alpha})
        print(json.dumps({"tool": "bsub_track_bench --bayer", "unit": "us a frame set, host clock around synchronous calls, median",
                          "library": os.path.relpath(oat_amd.lib_path(), ROOT), "shapes": shapes, "device": torch.cuda.get_device_name(0)}))
        return
    if a.filters:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import tracker_filters_legs
        maker = lambda alpha: lambda rows, cols, n: oat_amd.SubtractionTracker(  # noqa: E731
            rows, cols, n_streams=n, channels=3, alpha=alpha, erode=0, dilate=10, area=AREA, **WINDOW)
        shapes = tracker_filters_legs.run([({"alpha": alpha}, maker(alpha)) for alpha in ALPHAS], a.steps, a.warmup)
        print(json.dumps({"tool": "bsub_track_bench --filters", "unit": "us a frame set, host clock around synchronous calls, median",
                          "library": os.path.relpath(oat_amd.lib_path(), ROOT), "shapes": shapes, "device": torch.cuda.get_device_name(0)}))
        return
    if a.undistort:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import tracker_undistort_legs
        maker = lambda alpha: lambda rows, cols, n: oat_amd.SubtractionTracker(  # noqa: E731
            rows, cols, n_streams=n, channels=3, alpha=alpha, erode=0, dilate=10, area=AREA, **WINDOW)
        shapes = tracker_undistort_legs.run([({"alpha": alpha}, maker(alpha)) for alpha in ALPHAS], a.steps, a.warmup)
        print(json.dumps({"tool": "bsub_track_bench --undistort", "unit": "us a frame set, host clock around synchronous calls, median",
                          "library": os.path.relpath(oat_amd.lib_path(), ROOT), "shapes": shapes, "device": torch.cuda.get_device_name(0)}))
        return

    out = []
    for name, n, rows, cols in SHAPES:
        frames = 8
        host = np.stack(make_pool(rows, cols, n, frames, n_discs=3))                     # [frames][n][rows][cols][3]
        dev = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        ptrs = [dev[t].data_ptr() for t in range(frames)]
        seq = [ptrs[t % frames] for t in range(a.steps)]
        hp = oat_amd.HotPath(rows, cols, n_streams=n, adaptation_coeff=0.01, erode=0, dilate=10, area=AREA, **WINDOW)
        mog_us = round(timed_us(lambda t: hp.track_sequence_dev(seq), 5, 1)[0] / a.steps, 1)
        hp.close()
        for alpha in ALPHAS:
            rec = {"shape": name, "streams": n, "rows": rows, "cols": cols, "channels": 3, "alpha": alpha, "steps": a.steps,
                   "warmup": a.warmup, "mog_sequence_us": mog_us}
            st = oat_amd.SubtractionTracker(rows, cols, n_streams=n, channels=3, alpha=alpha, erode=0, dilate=10, area=AREA, **WINDOW)
            rec["sync_us"], rec["sync_p10_us"], rec["sync_p90_us"] = timed_us(lambda t: st.track_dev(ptrs[t % frames]), a.steps, a.warmup)
            s_med, s_lo, s_hi = timed_us(lambda t: st.track_sequence_dev(seq), 5, 1)
            rec["sequence_us"], rec["sequence_min_us"], rec["sequence_max_us"] = (round(x / a.steps, 1) for x in (s_med, s_lo, s_hi))
            st.close()
            det = oat_amd.HSVDetector(rows, cols, erode=0, dilate=10, area=AREA, n_streams=n, **WINDOW)
            sub, hsv = np.empty((rows, cols, 3), np.uint8), np.empty((rows, cols, 3), np.uint8)
            pos = ffi.Position()

            def parent(t):
                for s in range(n):
                    det._chk(det.lib.oatgpu_bsub_filter(det.ctx, s, ffi.u8(host[t % frames, s]), ffi.u8(sub), alpha))
                    det._chk(det.lib.oatgpu_bgr2hsv(det.ctx, ffi.u8(sub), ffi.u8(hsv)))
                    det._chk(det.lib.oatgpu_detect_hsv(det.ctx, s, ffi.u8(hsv), C.byref(pos)))
            rec["parent_us"], rec["parent_p10_us"], rec["parent_p90_us"] = timed_us(parent, a.steps, a.warmup)
            det.close()
            rec["parent_over_sync"] = round(rec["parent_us"] / rec["sync_us"], 2)
            rec["parent_over_sequence"] = round(rec["parent_us"] / rec["sequence_us"], 2)
            rec["mog_over_sequence"] = round(mog_us / rec["sequence_us"], 2)
            out.append(rec)
        del dev
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "bsub_track_bench", "unit": "us a frame set, host clock around synchronous calls, median",
                      "library": os.path.relpath(oat_amd.lib_path(), ROOT), "shapes": out, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
