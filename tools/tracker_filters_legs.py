"""The `--filters` leg of tools/diff_bench.py and tools/bsub_track_bench.py: what the filter chain `posifilt kalman` -> `posifilt
homography` -> `posifilt region` behind a batched tracker costs (oatgpu_set_tracker_filters): one more launch a
frame -- one lane a camera -- behind the blob analysis, and inside the sequence calls one event wait and one event record a frame
that order the launches of consecutive frames.

Shapes: 1 x 4K, 16 x 1080p, 1 x 640x480, BGR frames of the tools' pool, QUIET: one frame set repeated -- nothing moves, the masks
are empty and the back half is at its cheapest, so the extra launch's share of the step is at its largest.  All three members
are on: the Kalman filter with a timeout of 0.1 s, a projective matrix, three regions.  Legs, us a frame set:
  off   no chain configured -- the code path without the feature: sync = the tracker's synchronous call on device frames, the
        median of `steps` calls after `warmup`; sequence = `steps` frame sets in one call, the median of 5 calls after one,
        divided by `steps`;
  on    the same two calls with the chain configured, on the same context, measured right behind.
Every timed call ends in a device synchronisation, so a host clock around it is the step."""
import statistics
import time

SHAPES = [("1x4K", 1, 2160, 3840), ("16x1080p", 16, 1080, 1920), ("1x640x480", 1, 480, 640)]
CHAIN = dict(kalman=dict(dt=0.02, timeout=0.1, sigma_accel=5.0, sigma_noise=1.0),
             homography=[0.02, 0.001, -1.5, -0.002, 0.025, 0.75, 1e-4, -2e-4, 1.0],
             regions=[("north", [(-10, -10), (30, -10), (30, 10), (-10, 10)]), ("south", [(-10, 10), (30, 10), (30, 40), (-10, 40)]),
                      ("east", [(30, -10), (90, -10), (90, 40), (30, 40)])])


def _median_us(call, steps, warmup):
    for t in range(warmup):
        call(t)
    d = []
    for t in range(steps):
        t0 = time.perf_counter()
        call(warmup + t)
        d.append(time.perf_counter() - t0)
    return round(statistics.median(d) * 1e6, 1)


def run(makers, steps, warmup):
    """makers: [(extra fields of the record, make_tracker(rows, cols, n) -> a MotionTracker / SubtractionTracker, BGR)]; every
    maker runs on one pool a shape.  -> one record a shape and maker"""
    import numpy as np
    import torch
    from oat_amd.synth import make_pool
    out = []
    for name, n, rows, cols in SHAPES:
        pool = torch.from_numpy(np.stack(make_pool(rows, cols, n, 1, n_discs=3))).cuda()      # [1][n][rows][cols][3]
        torch.cuda.synchronize()
        quiet = pool[0].data_ptr()
        seq = [quiet] * steps
        for extra, make_tracker in makers:
            tr = make_tracker(rows, cols, n)
            tr.track_dev(quiet)                                    # (the first frame of a context: the last image, the background)
            rec = {"shape": name, "streams": n, "rows": rows, "cols": cols, "frames": "quiet", "steps": steps, "warmup": warmup}
            rec.update(extra)
            for leg in ("off", "on"):
                if leg == "on":
                    tr.set_filters(**CHAIN)
                rec[f"{leg}_sync_us"] = _median_us(lambda t: tr.track_dev(quiet), steps, warmup)
                rec[f"{leg}_sequence_us"] = round(_median_us(lambda t: tr.track_sequence_dev(seq), 5, 1) / steps, 1)
            assert len(tr.filtered()) == steps
            for call in ("sync", "sequence"):
                rec[f"on_minus_off_{call}_us"] = round(rec[f"on_{call}_us"] - rec[f"off_{call}_us"], 1)
            tr.close()
            out.append(rec)
        del pool
        torch.cuda.empty_cache()
    return out
