#!/usr/bin/env python3
"""What target crops cost (oatgpu_set_target_crops) on top of targets and target shapes: one more kernel
(k_target_crops) behind the frame's ranking and shapes, its windows written into host-mapped memory, and the call's copy of the
delivered crop set.

    python tools/crops_bench.py [--steps 200] [--warmup 20] [--quick]
    python tools/crops_bench.py --off-only --tree DIR      # the off legs alone with the package of another checkout (the parent)
    python tools/crops_bench.py --tensor                   # crop tensors against the host-mapped crops, see below
    python tools/crops_bench.py --mask                     # target masks beside crop tensors, see below

The shape of tools/targets_bench.py --target-shapes: 1 x 4K, 16 x 1080p and 1 x 640x480, BGR frames in device memory; the motion
tracker (diff_threshold 16, blur 2) and the subtraction tracker (alpha 0, a window on the brightness of the difference); frames with
ONE blob a camera and with TWELVE (targets_bench.paint); targets K = 4 and 8 with shapes on.  Legs, us a frame set:
  sync      track_dev: the median of `steps` calls after `warmup` calls;
  sequence  track_sequence_dev over the 8 frame sets of the pool in one call, divided by 8: the median of `steps` calls after 2.
Each with crops off, off once more (the same process, a new context: the run-to-run spread beside the differences), then 64 x 64
upright, 64 x 64 along the body axis and 128 x 128 along the body axis.  fetch_us is target_crops() behind a synchronous step: the
copy of one crop set out of the library.  windows_us is oatgpu_crop_windows_dev alone, K windows a camera at the frame's centre,
64 x 64, turned by 30 degrees.  Every timed call ends in a device synchronisation, so a host clock around it is the step.
--off-only runs the two off legs and nothing that needs the new entry points, so that the same file measures the parent commit's
step from its own tree (--tree).  Prints one JSON line; the recipe and the figures' place are in profiles/crops_bench.txt.

--tensor measures crop tensors (oatgpu_set_target_crop_tensor; profiles/crop_tensor_bench.txt) instead: the same
shapes and trackers, twelve blobs a camera, K = 4 and 8 with shapes on, windows of 64 x 64 and 128 x 128 along the body axis.  Legs,
each a new context in one process: off, off_again; crops -- the host-mapped crop sets of oatgpu_set_target_crops; u8 -- the tensor in
bytes, left on the device; u8_copy -- the same followed by ONE copy_ of the delivered entries into a pinned host tensor and a device
synchronisation ("a device set plus one async copy"); f16 -- the tensor in half, scale 1/255, zoom 1; f16_zoom2 -- the same at zoom 2.

--mask measures target masks (oatgpu_set_target_mask_tensor; profiles/mask_tensor_bench.txt) the same way: off,
off_again; tensor_u8 -- the crop tensor in bytes; mask_u8 -- the mask in bytes; both -- the two beside each other; mask_f16_zoom2 --
the mask in half at zoom 2.

Without a GPU the tool fails (no fallback)."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from targets_bench import AREA, POOL, SHAPES, median_us, paint      # noqa: E402

CROPS = (("up64", 64, 64, False), ("ax64", 64, 64, True), ("ax128", 128, 128, True))


TENSOR_SIZES = (64, 128)
TENSOR_LEGS = ("off", "off_again", "crops", "u8", "u8_copy", "f16", "f16_zoom2")
MASK_LEGS = ("off", "off_again", "tensor_u8", "mask_u8", "both", "mask_f16_zoom2")


def tensor_main(a, torch, oat_amd, np, makers, tree, legs=TENSOR_LEGS, tool="--tensor"):
    from oat_amd.synth import SyntheticStream
    out = []
    for name, n, rows, cols in SHAPES:
        if a.shapes and name not in a.shapes.split(","):
            continue
        streams = [SyntheticStream(rows, cols, s, n_discs=0, flicker=False) for s in range(n)]
        bare = [np.stack([st.frame(t) for st in streams]) for t in range(POOL)]
        dev = torch.from_numpy(paint(bare, 12)).cuda()
        torch.cuda.synchronize()
        ptrs = [dev[t].data_ptr() for t in range(POOL)]
        for tracker, make in makers:
            if a.trackers and tracker not in a.trackers.split(","):
                continue
            for k in [int(v) for v in a.ks.split(",")]:
                for side in TENSOR_SIZES:
                    rec = {"shape": name, "streams": n, "rows": rows, "cols": cols, "tracker": tracker, "blobs": 12, "k": k, "side": side,
                           "steps": a.steps, "warmup": a.warmup}
                    for leg in legs:
                        tr = make(rows, cols, n)
                        tr.set_targets(k)
                        tr.set_target_shapes()
                        tensor = pinned = mask = None
                        if leg in ("tensor_u8", "both"):
                            tensor = tr.set_target_crop_tensor(side, side, axis=True, dtype="uint8", capacity=POOL)
                        if leg in ("mask_u8", "both"):
                            mask = tr.set_target_mask_tensor(side, side, axis=True, dtype="uint8", capacity=POOL)
                        elif leg == "mask_f16_zoom2":
                            mask = tr.set_target_mask_tensor(side, side, axis=True, zoom=2.0, dtype="float16", capacity=POOL)
                        if leg == "crops":
                            tr.set_target_crops(side, side, axis=True)
                        elif leg in ("u8", "u8_copy"):
                            tensor = tr.set_target_crop_tensor(side, side, axis=True, dtype="uint8", capacity=POOL)
                        elif leg in ("f16", "f16_zoom2"):
                            tensor = tr.set_target_crop_tensor(side, side, axis=True, zoom=2.0 if leg == "f16_zoom2" else 1.0, dtype="float16",
                                                               scale=1.0 / 255.0, capacity=POOL)
                        if leg == "u8_copy":
                            pinned = torch.empty(tuple(tensor.shape), dtype=torch.uint8).pin_memory()

                        def sync_step(t):
                            tr.track_dev(ptrs[t % POOL])
                            if pinned is not None:
                                pinned[:1].copy_(tr.target_crop_tensor(), non_blocking=True)
                                torch.cuda.synchronize()

                        def sequence(t):
                            tr.track_sequence_dev(ptrs)
                            if pinned is not None:
                                pinned.copy_(tr.target_crop_tensor(), non_blocking=True)
                                torch.cuda.synchronize()
                        for t in range(POOL):                               # the last images and the background settle on the pool
                            tr.track_dev(ptrs[t])
                        rec[f"sync_us_{leg}"] = median_us(sync_step, a.steps, a.warmup)
                        rec[f"sequence_us_{leg}"] = round(median_us(sequence, a.steps, 2) / POOL, 1)
                        if tensor is not None:
                            torch.cuda.synchronize()
                            rec[f"entry_bytes_{leg}"] = int(tensor[0].numel() * tensor.element_size())
                            rec[f"nonzero_windows_{leg}"] = int((tensor[0].reshape(n * k, -1) != 0).any(dim=1).sum().item())
                        if mask is not None:
                            torch.cuda.synchronize()
                            rec[f"mask_entry_bytes_{leg}"] = int(mask[0].numel() * mask.element_size())
                            rec[f"mask_nonzero_windows_{leg}"] = int((mask[0].reshape(n * k, -1) != 0).any(dim=1).sum().item())
                            rec[f"mask_on_fraction_{leg}"] = round(float((mask[0] != 0).float().mean().item()), 4)
                        tr.close()
                        del tensor, pinned, mask
                    out.append(rec)
        del dev
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "crops_bench " + tool, "unit": "us a frame set, host clock around synchronous calls, median",
                      "tree": os.path.relpath(tree, ROOT), "library": os.path.relpath(oat_amd.lib_path(), tree), "shapes": out,
                      "device": torch.cuda.get_device_name(0)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="few steps (a rehearsal)")
    ap.add_argument("--off-only", action="store_true", help="the two off legs alone: nothing that needs oatgpu_set_target_crops")
    ap.add_argument("--tensor", action="store_true", help="crop tensors against the host-mapped crops (DESIGN.md 9m)")
    ap.add_argument("--mask", action="store_true", help="target masks beside crop tensors (DESIGN.md 9o)")
    ap.add_argument("--shapes", default="", help="comma list of shape names (default: all)")
    ap.add_argument("--trackers", default="", help="motion, subtraction or both (default)")
    ap.add_argument("--blobs", default="1,12", help="blobs a camera, comma list")
    ap.add_argument("--ks", default="4,8", help="K of oatgpu_set_targets, comma list")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose oat_amd package and library are measured (default: this one)")
    a = ap.parse_args()
    if a.quick:
        a.steps, a.warmup = 16, 4
    tree = os.path.abspath(a.tree)
    sys.path.insert(0, tree)
    import torch
    import oat_amd
    import numpy as np
    from oat_amd.synth import SyntheticStream
    if not torch.cuda.is_available():
        raise SystemExit("crops_bench: no GPU (nothing is measured without one)")
    assert os.path.abspath(oat_amd.__file__).startswith(tree + os.sep), (oat_amd.__file__, tree)

    def motion(rows, cols, n):
        return oat_amd.MotionTracker(rows, cols, n_streams=n, channels=3, diff_threshold=16, blur=2, area=AREA)

    def subtraction(rows, cols, n):
        return oat_amd.SubtractionTracker(rows, cols, n_streams=n, channels=3, alpha=0.0, v_thresh=(60, 256), erode=0, dilate=3, area=AREA)

    if a.tensor:
        return tensor_main(a, torch, oat_amd, np, (("motion", motion), ("subtraction", subtraction)), tree)
    if a.mask:
        return tensor_main(a, torch, oat_amd, np, (("motion", motion), ("subtraction", subtraction)), tree, MASK_LEGS, "--mask")
    legs = [("off", None), ("off_again", None)] + ([] if a.off_only else [(name, (h, w, axis)) for name, h, w, axis in CROPS])
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
            for tracker, make in (("motion", motion), ("subtraction", subtraction)):
                if a.trackers and tracker not in a.trackers.split(","):
                    continue
                for k in [int(v) for v in a.ks.split(",")]:
                    rec = {"shape": name, "streams": n, "rows": rows, "cols": cols, "tracker": tracker, "blobs": blobs, "k": k,
                           "steps": a.steps, "warmup": a.warmup}
                    for leg, crop in legs:
                        tr = make(rows, cols, n)
                        tr.set_targets(k)
                        tr.set_target_shapes()
                        if crop:
                            tr.set_target_crops(crop[0], crop[1], axis=crop[2])
                        for t in range(POOL):                               # the last images and the background settle on the pool
                            tr.track_dev(ptrs[t])
                        rec[f"sync_us_{leg}"] = median_us(lambda t: tr.track_dev(ptrs[t % POOL]), a.steps, a.warmup)
                        rec[f"sequence_us_{leg}"] = round(median_us(lambda t: tr.track_sequence_dev(ptrs), a.steps, 2) / POOL, 1)
                        if crop:
                            tr.track_dev(ptrs[0])
                            rec[f"fetch_us_{leg}"] = median_us(lambda t: tr.target_crops(), a.steps, 2)
                            c = tr.target_crops()
                            rec[f"nonzero_windows_{leg}"] = int(c.reshape(c.shape[0] * n * k, -1).any(axis=1).sum())
                        elif not a.off_only and leg == "off":
                            ang = math.radians(30.0)
                            wins = [[(1, 0, cols / 2 + 3.25 * q, rows / 2 - 1.5 * q, math.cos(ang), math.sin(ang)) for q in range(k)]] * n
                            rec["windows_us"] = median_us(lambda t: tr.crop_windows(ptrs[t % POOL], wins, 64, 64), a.steps, a.warmup)
                        tr.close()
                    out.append(rec)
            del dev
            torch.cuda.empty_cache()
    print(json.dumps({"tool": "crops_bench" + (" --off-only" if a.off_only else ""),
                      "unit": "us a frame set, host clock around synchronous calls, median",
                      "tree": os.path.relpath(tree, ROOT), "library": os.path.relpath(oat_amd.lib_path(), tree), "shapes": out,
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
