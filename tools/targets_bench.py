#!/usr/bin/env python3
"""What multi-target detection costs (oatgpu_set_targets): a step with targets on gives up the single-workgroup LDS
blob kernel and, in the fused tracker, the early / paired launch orders, for the global blob kernels with k_blob_rank behind them.

    python tools/targets_bench.py [--steps 200] [--warmup 20] [--quick]
    python tools/targets_bench.py --off-only --tree DIR      # the off legs alone with the package of another checkout (the parent)
    python tools/targets_bench.py --tracks [--off-only --tree DIR]      # what target tracks cost on top of targets
    python tools/targets_bench.py --target-shapes [--off-only --tree DIR]      # what target shapes cost on top of targets

Shapes: 1 x 4K, 16 x 1080p and 1 x 640x480, BGR frames in device memory; the fused tracker (HotPath, bench.py's detector) and the
motion tracker (diff_threshold 16, blur 2); frames with ONE blob a camera and with TWELVE (squares of the disc colour, 8 .. 30
pixels wide, moving a few pixels a frame over synth.py's gradient with its +-6 noise and WITHOUT its flickering pixels: every
64th pixel flickering by 110 levels is a foreground dot of the motion tracker on every frame, 130 k of them at 4K, far over the
LDS blob kernel's capacity -- the step would take the global kernels with targets off as well and there would be nothing to
compare).  --shapes / --trackers / --blobs pick a part.  Legs, us a frame set:
  sync      track_dev: the median of `steps` calls after `warmup` calls;
  sequence  track_sequence_dev over the 8 frame sets of the pool in one call, divided by 8: the median of `steps` calls after 2.
Each with targets off, off once more (the same process, a new context: the run-to-run spread beside the differences), then K =
1, 4, 8.  Every timed call ends in a device synchronisation, so a host clock around it is the step.  --off-only runs the two off
legs and nothing that needs the new entry points, so that the same file measures the parent commit's step from its own tree
(--tree): the off legs of the two trees should differ by no more than the two off legs of one tree do.  Prints one JSON line;
the recipe and the figures' place are in profiles/targets_bench.txt.

--tracks measures target tracks (oatgpu_set_tracks) instead: the motion and the subtraction tracker (alpha 0, a window on the
brightness of the difference), the same shapes and legs; per K = 4 and 8: targets on with tracks off, off once more (a new
context), then tracks on (kalman dt 0.02 timeout 0.1 sigma-accel 300 sigma-noise 0.5, gate 40 pixels).  The added us a frame
set is tracks minus off.  With --off-only the tracks-off legs alone: they need nothing newer than oatgpu_set_targets, so the
parent commit's tree (--tree) runs them.  The recipe and the figures' place are in profiles/tracks_bench.txt.

--target-shapes measures target shapes (oatgpu_set_target_shapes) instead: the fused and the motion tracker, the same shapes,
blobs and legs; per K = 4 and 8: targets on with shapes off, off once more (a new context), then shapes on.  The added us a frame
set is shapes minus off.  With --off-only the shapes-off legs alone, which the parent commit's tree (--tree) runs too.  (--shapes
is the list of frame shapes.)  The recipe and the figures' place are in profiles/shapes_bench.txt.

Without a GPU the tool fails (no fallback)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [("1x4K", 1, 2160, 3840), ("16x1080p", 16, 1080, 1920), ("1x640x480", 1, 480, 640)]
AREA = (20.0, 1e6)
BLOCK = (255, 64, 0)                 # synth.DISC_BGR[0]: inside disc_hsv_window()
POOL = 8


def median_us(call, steps, warmup):
    for t in range(warmup):
        call(t)
    d = []
    for t in range(steps):
        t0 = time.perf_counter()
        call(warmup + t)
        d.append(time.perf_counter() - t0)
    return round(statistics.median(d) * 1e6, 1)


def paint(pool, blobs):
    """a copy of the pool [POOL][n, rows, cols, 3] with `blobs` squares a camera, each on its own cell of a 4 x 3 grid"""
    import numpy as np                      # (here and not at the top: --help needs nothing)
    out = np.stack(pool).copy()
    _, n, rows, cols, _ = out.shape
    ch, cw = rows // 3, cols // 4
    for t in range(out.shape[0]):
        for s in range(n):
            for b in range(blobs):
                side = min(8 + 2 * b, ch // 3, cw // 3)
                y = (b // 4) * ch + ch // 4 + (3 * t + s) % (ch // 4)
                x = (b % 4) * cw + cw // 4 + (5 * t + 2 * s) % (cw // 4)
                out[t, s, y:y + side, x:x + side] = BLOCK
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="few steps (a rehearsal)")
    ap.add_argument("--off-only", action="store_true", help="the two off legs alone: nothing that needs oatgpu_set_targets")
    ap.add_argument("--tracks", action="store_true", help="target tracks on top of targets K = 4, 8 (motion and subtraction tracker)")
    ap.add_argument("--target-shapes", action="store_true", help="target shapes on top of targets K = 4, 8 (fused and motion tracker)")
    ap.add_argument("--shapes", default="", help="comma list of shape names (default: all)")
    ap.add_argument("--trackers", default="", help="fused, motion or both (default)")
    ap.add_argument("--blobs", default="1,12", help="blobs a camera, comma list")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose oat_amd package and library are measured (default: this one)")
    a = ap.parse_args()
    if a.quick:
        a.steps, a.warmup = 16, 4
    tree = os.path.abspath(a.tree)
    sys.path.insert(0, tree)
    import torch
    import oat_amd
    import numpy as np
    from oat_amd.synth import SyntheticStream, disc_hsv_window
    if not torch.cuda.is_available():
        raise SystemExit("targets_bench: no GPU (nothing is measured without one)")
    assert os.path.abspath(oat_amd.__file__).startswith(tree + os.sep), (oat_amd.__file__, tree)

    def fused(rows, cols, n):
        return oat_amd.HotPath(rows, cols, n_streams=n, adaptation_coeff=0.01, erode=3, dilate=7, area=AREA, ring_depth=8,
                               **disc_hsv_window())

    def motion(rows, cols, n):
        return oat_amd.MotionTracker(rows, cols, n_streams=n, channels=3, diff_threshold=16, blur=2, area=AREA)

    def subtraction(rows, cols, n):
        return oat_amd.SubtractionTracker(rows, cols, n_streams=n, channels=3, alpha=0.0, v_thresh=(60, 256), erode=0, dilate=3, area=AREA)

    # (leg, K, tracks or shapes on)
    legs = [("off", 0, False), ("off_again", 0, False)] + ([] if a.off_only else [("k1", 1, False), ("k4", 4, False), ("k8", 8, False)])
    trackers = (("fused", fused), ("motion", motion))
    if a.tracks:
        legs = [(f"k{k}_{leg}", k, leg == "tracks") for k in (4, 8) for leg in ("off", "off_again") + (() if a.off_only else ("tracks",))]
        trackers = (("motion", motion), ("subtraction", subtraction))
    if a.target_shapes:
        legs = [(f"k{k}_{leg}", k, leg == "shapes") for k in (4, 8) for leg in ("off", "off_again") + (() if a.off_only else ("shapes",))]
    out = []
    for name, n, rows, cols in SHAPES:
        if a.shapes and name not in a.shapes.split(","):
            continue
        streams = [SyntheticStream(rows, cols, s, n_discs=0, flicker=False) for s in range(n)]
        bare = [np.stack([st.frame(t) for st in streams]) for t in range(POOL)]
        for blobs in [int(b) for b in a.blobs.split(",")]:
            dev = torch.from_numpy(paint(bare, blobs)).cuda()
            torch.cuda.synchronize()
            ptrs = [dev[t].data_ptr() for t in range(POOL)]
            for tracker, make in trackers:
                if a.trackers and tracker not in a.trackers.split(","):
                    continue
                rec = {"shape": name, "streams": n, "rows": rows, "cols": cols, "tracker": tracker, "blobs": blobs,
                       "steps": a.steps, "warmup": a.warmup}
                for leg, k, extra in legs:
                    tracks, shapes = extra and a.tracks, extra and a.target_shapes
                    tr = make(rows, cols, n)
                    if k:
                        tr.set_targets(k)
                    if shapes:
                        tr.set_target_shapes()
                    if tracks:
                        tr.set_tracks(kalman=dict(dt=0.02, timeout=0.1, sigma_accel=300.0, sigma_noise=0.5), gate=40.0)
                    for t in range(POOL):                                   # the model and the last images settle on the pool
                        tr.track_dev(ptrs[t])
                    rec[f"sync_us_{leg}"] = median_us(lambda t: tr.track_dev(ptrs[t % POOL]), a.steps, a.warmup)
                    rec[f"sequence_us_{leg}"] = round(median_us(lambda t: tr.track_sequence_dev(ptrs), a.steps, 2) / POOL, 1)
                    if k:
                        (tset,) = tr.targets()[-1:]
                        rec[f"n_found_{leg}"] = [f for _, f in tset][:4]
                    if shapes:
                        rec[f"axes_{leg}"] = [sum(r.axis_valid for r in cam) for cam in tr.target_shapes()[-1]][:4]
                    if tracks:
                        rec[f"ids_{leg}"] = [[r.id for r in cam] for cam in tr.tracks()[-1]][:2]
                    tr.close()
                out.append(rec)
            del dev
            torch.cuda.empty_cache()
    print(json.dumps({"tool": "targets_bench" + (" --tracks" if a.tracks else "") + (" --target-shapes" if a.target_shapes else "") + (" --off-only" if a.off_only else ""),
                      "unit": "us a frame set, host clock around synchronous calls, median",
                      "tree": os.path.relpath(tree, ROOT), "library": os.path.relpath(oat_amd.lib_path(), tree), "shapes": out,
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
