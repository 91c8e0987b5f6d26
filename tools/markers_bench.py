#!/usr/bin/env python3
"""What a marker step costs (oatgpu_track_markers_dev): M = 1, 2, 3 markers in ONE context against
  * `plain`: oatgpu_track_batch_dev on the same frames with one marker's window as the context's own -- one marker, no
    marker machinery (for the PARENT COMMIT's own number run this tool on a built checkout of the parent:
    python tools/markers_bench.py --baseline-only --tree PARENT_CHECKOUT);
  * `contexts`: M separate contexts, each with its own MOG2 model and its own window, stepped one after the other -- what a
    user had to do before marker sets.

    python tools/markers_bench.py [--steps N] [--warmup W] [--quick] [--baseline-only]
    python tools/markers_bench.py --ktrace RESULTS.db      # k_marker_bits from a rocprofv3 --kernel-trace run of --quick
                                                           # against its byte model (C + 1/8 B read, M/8 B written a pixel)

Shapes: 1 x 4K (bench.py's headline morphology: erode 7, dilate 7), 16 x 1080p and 1 x 640x480 (erode 3, dilate 7), three
discs a camera, learning rate 0.01.  Every call is synchronous (one frame set in, its results out); a step is timed with a
pair of HIP events on the context's stream around the call, after the warm-up; medians are reported, with the wall-clock
median beside them.  Prints one JSON line.

    python tools/markers_bench.py --pipelined [--rounds R] [--sets N] [--tree CHECKOUT --parent]
The PIPELINED legs (oatgpu_set_marker_pipeline), a host clock around calls that end in a synchronisation, us a frame set, N
(>= 200) frame sets a call after a warm-up call that ages the models, R rounds of every leg, every round's figure reported:
  (b) the synchronous marker step;  (c) oatgpu_track_markers_sequence_dev;  (d) M plain contexts, each through
  oatgpu_track_sequence_dev, summed;  (e) ONE plain context through oatgpu_track_sequence_dev -- the floor, the marker work
  fully hidden.  With --parent (a library without the pipelined path, e.g. --tree PARENT_CHECKOUT) only the legs it has: the
  synchronous marker step -- leg (a) -- and (e); its own repeats are the noise floor.

    python tools/markers_bench.py --filters [--pipelined ...]
The filter chain behind the combined record (oatgpu_set_marker_filters) on every marker leg, synchronous and pipelined: all
three members on -- posifilt kalman, posifilt homography, posifilt region with two regions (the left and the right half of
the frame).  The same command without --filters is the chain-off step; profiles/markers_filters_bench.txt has the recipe."""
import argparse
import json
import os
import sqlite3
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("1x4K", 1, 2160, 3840, 7, 7), ("16x1080p", 16, 1080, 1920, 3, 7), ("1x640x480", 1, 480, 640, 3, 7)]
WINDOWS = [dict(h=(100, 125), s=(150, 256), v=(100, 256)), dict(h=(0, 20), s=(150, 256), v=(100, 256)),
           dict(h=(50, 70), s=(150, 256), v=(100, 256))]
AREA = (20.0, 1e6)


def filters(rows, cols):
    """HotPath.set_marker_filters keywords of --filters: all three members, two regions"""
    half = cols // 2
    return dict(kalman=dict(dt=0.02, timeout=0.2, sigma_accel=5.0, sigma_noise=1.0),
                homography=[[0.01, 0, -0.005 * cols], [0, 0.01, -0.005 * rows], [0, 0, 1]],
                regions=[("left", [(0, 0), (half, 0), (half, rows), (0, rows)]),
                         ("right", [(half, 0), (cols, 0), (cols, rows), (half, rows)])])


def ktrace(path, steps_hint=None):
    """k_marker_bits in a rocpd database: dispatches grouped by grid (= shape), each group split into the three consecutive
    runs of the tool (M = 1, 2, 3); median duration against the byte model."""
    db = sqlite3.connect(path)
    rows = db.execute("select s.kernel_name, d.start, d.end, d.grid_size_x, d.grid_size_y from rocpd_kernel_dispatch d "
                      "join rocpd_info_kernel_symbol s on d.kernel_id = s.id order by d.start").fetchall()
    groups = {}
    for name, st, en, gx, gy in rows:
        if "k_marker_bits" in name:
            groups.setdefault((gx, gy), []).append(en - st)
    out = []
    for (gx, gy), d in groups.items():
        px = gx * 4 * gy                                  # 256 threads a 1024-pixel workgroup, grid y = streams
        third = len(d) // 3
        for i, M in enumerate((1, 2, 3)):
            run = d[i * third:(i + 1) * third]
            run = run[len(run) // 4:]                     # the warm-up quarter
            if not run:
                continue
            us = statistics.median(run) / 1e3
            model = px * (3 + 1 / 8 + M / 8)
            out.append({"padded_pixels": px, "streams": gy, "markers": M, "dispatches": len(run), "median_us": round(us, 2),
                        "model_MB": round(model / 1e6, 2), "model_TBps": round(model / us / 1e6, 3)})
    return {"tool": "markers_bench", "ktrace": os.path.basename(path), "kernel": "k_marker_bits", "rows": out}


def timed(torch, stream, step, steps, warmup):
    """median over `steps` calls of step(t): (HIP-event us, wall-clock us)"""
    for t in range(warmup):
        step(t)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    wall = []
    for t in range(steps):
        ev[t][0].record(stream)
        t0 = time.perf_counter()
        step(warmup + t)
        wall.append(time.perf_counter() - t0)
        ev[t][1].record(stream)
    torch.cuda.synchronize()
    return (round(statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3, 1), round(statistics.median(wall) * 1e6, 1))


def pipelined(a):
    import numpy as np
    import torch
    import oat_amd
    from oat_amd.synth import make_pool
    out = []
    for name, n, rows, cols, ero, dil in SHAPES:
        frames = min(32, max(8, 1024 * 1024 * 1024 // (n * rows * cols * 3)))
        pool = torch.from_numpy(np.stack(make_pool(rows, cols, n, frames, n_discs=3))).cuda()
        ptrs = [pool[t % frames].data_ptr() for t in range(a.sets)]
        torch.cuda.synchronize()
        kw = dict(n_streams=n, adaptation_coeff=0.01, erode=ero, dilate=dil, area=AREA, ring_depth=4)

        def ctx(w):
            return oat_amd.HotPath(rows, cols, h_thresh=w["h"], s_thresh=w["s"], v_thresh=w["v"], **kw)

        def clock(call):
            """us a frame set of call() over a.sets frame sets, once per round, after one warm-up call"""
            call()
            res = []
            for _ in range(a.rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                res.append(round((time.perf_counter() - t0) / a.sets * 1e6, 1))
            return res

        rec = {"shape": name, "streams": n, "rows": rows, "cols": cols, "sets": a.sets, "rounds": a.rounds}
        one = ctx(WINDOWS[0])
        rec["e_plain_pipelined_us"] = clock(lambda: one.track_sequence_dev(ptrs))
        one.close()
        for M in (1, 2, 3):
            markers = [dict(w, erode=ero, dilate=dil, area=AREA) for w in WINDOWS[:M]]
            hp = ctx(dict(h=(0, 256), s=(0, 256), v=(1, 256)))
            hp.set_markers(markers, heading_anchor=0)
            if a.filters:
                hp.set_marker_filters(**filters(rows, cols))

            def sync_steps():
                for p_ in ptrs:
                    hp.track_markers_dev(p_)
            r = {"a_parent_sync_us" if a.parent else "b_sync_us": clock(sync_steps)}
            if not a.parent:
                hp.marker_pipeline(True)
                r["c_markers_sequence_us"] = clock(lambda: hp.track_markers_sequence_dev(ptrs))
                r["last_step_shape"] = list(hp.last_step_shape())
            hp.close()
            if not a.parent:
                many = [ctx(w) for w in WINDOWS[:M]]

                def each():
                    for c in many:
                        c.track_sequence_dev(ptrs)
                r["d_contexts_pipelined_sum_us"] = clock(each)
                for c in many:
                    c.close()
            rec[f"M{M}"] = r
        out.append(rec)
        del pool
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "markers_bench", "mode": "pipelined", "unit": "us a frame set, host clock, one figure a round",
                      "parent": a.parent, "filters": a.filters, "library": os.path.relpath(oat_amd.lib_path(), os.path.abspath(a.tree)), "shapes": out,
                      "device": torch.cuda.get_device_name(0)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pipelined", action="store_true", help="the pipelined legs (see the module's text)")
    ap.add_argument("--parent", action="store_true", help="with --pipelined: a library without the pipelined marker path")
    ap.add_argument("--filters", action="store_true", help="the filter chain (kalman, homography, two regions) on every marker leg")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sets", type=int, default=256, help="frame sets a timed call (--pipelined)")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--quick", action="store_true", help="few steps (a profiler run)")
    ap.add_argument("--baseline-only", action="store_true", help="only `plain` (works with a library that has no marker sets)")
    ap.add_argument("--tree", default=ROOT, help="import oat_amd (and its library) from this built checkout instead of this one")
    ap.add_argument("--ktrace", help="print k_marker_bits' medians from this rocprofv3 database and exit")
    a = ap.parse_args()
    if a.ktrace:
        print(json.dumps(ktrace(a.ktrace)))
        return
    if a.quick:
        a.steps, a.warmup = 24, 8
    sys.path.insert(0, os.path.abspath(a.tree))
    if a.pipelined:
        return pipelined(a)
    import numpy as np
    import torch
    import oat_amd
    from oat_amd.synth import make_pool

    out = []
    for name, n, rows, cols, ero, dil in SHAPES:
        frames = min(32, max(8, 1024 * 1024 * 1024 // (n * rows * cols * 3)))           # (at most ~1 GB of pool)
        pool = torch.from_numpy(np.stack(make_pool(rows, cols, n, frames, n_discs=3))).cuda()
        ptrs = [pool[t].data_ptr() for t in range(frames)]
        torch.cuda.synchronize()
        kw = dict(n_streams=n, adaptation_coeff=0.01, erode=ero, dilate=dil, area=AREA, ring_depth=2)

        def ctx(w):
            return oat_amd.HotPath(rows, cols, h_thresh=w["h"], s_thresh=w["s"], v_thresh=w["v"], **kw)

        rec = {"shape": name, "streams": n, "rows": rows, "cols": cols, "pool": frames, "steps": a.steps}
        plain = ctx(WINDOWS[0])
        st = torch.cuda.ExternalStream(plain.get_stream())
        rec["plain_us"], rec["plain_wall_us"] = timed(torch, st, lambda t: plain.track_dev(ptrs[t % frames]), a.steps, a.warmup)
        plain.close()
        for M in (() if a.baseline_only else (1, 2, 3)):
            hp = ctx(dict(h=(0, 256), s=(0, 256), v=(1, 256)))                         # the non-zero window
            hp.set_markers([dict(w, erode=ero, dilate=dil, area=AREA) for w in WINDOWS[:M]], heading_anchor=0)
            if a.filters:
                hp.set_marker_filters(**filters(rows, cols))
            st = torch.cuda.ExternalStream(hp.get_stream())
            ev, wall = timed(torch, st, lambda t: hp.track_markers_dev(ptrs[t % frames]), a.steps, a.warmup)
            hp.close()
            many = [ctx(w) for w in WINDOWS[:M]]
            st = torch.cuda.ExternalStream(many[0].get_stream())                        # (the contexts of a process share their streams)

            def step_many(t):
                for c in many:
                    c.track_dev(ptrs[t % frames])
            ev_c, wall_c = timed(torch, st, step_many, a.steps, a.warmup)
            for c in many:
                c.close()
            rec[f"M{M}"] = {"markers_us": ev, "markers_wall_us": wall, "contexts_us": ev_c, "contexts_wall_us": wall_c,
                            "markers_over_contexts": round(ev / ev_c, 3), "markers_over_plain": round(ev / rec["plain_us"], 3)}
        out.append(rec)
        del pool
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "markers_bench", "entry": "oatgpu_track_markers_dev | oatgpu_track_batch_dev", "unit": "us a step, median",
                      "library": os.path.relpath(oat_amd.lib_path(), os.path.abspath(a.tree)), "baseline_only": a.baseline_only, "filters": a.filters, "shapes": out, "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
