"""The `--undistort` leg of tools/diff_bench.py and tools/bsub_track_bench.py: what a batched tracker's step costs on distorted
frames with the remap inside the front kernel (oatgpu_set_tracker_undistort) against the way the same work had to
be done before it, on the same frames, and against the packed step alone.

Shapes: 1 x 4K, 16 x 1080p, 1 x 640x480, BGR frames of the tools' pool; the calibration is tests/undistort_ref.py's `mild5` for
the shape (inside the frame almost everywhere); the frames of leg (c) are oatgpu_undistort_dev's output of the pool.  Legs, us a
frame set, median of `steps` after `warmup` (sequence: `steps` frame sets in one call, the median of 5 calls after one, divided
by `steps`):
  fused     (a) the given frames through the tracker's own call, switch on: sync (device frames), sequence;
  undistort (b) oatgpu_undistort_dev into a buffer followed by the packed call, switch off, one context: sync, sequence (every
            frame set is remapped again, into the pool's second set of buffers, in front of the sequence call);
  packed    (c) the packed call alone on the undistorted frames: sync, sequence -- the floor.
`quiet`: the same legs on one frame set repeated: nothing moves, the masks are empty and the back half is at its cheapest, so
the front kernel's share of the step is at its largest.
Every timed call ends in a device synchronisation, so a host clock around it is the step."""
import ctypes as C
import statistics
import time

SHAPES = [("1x4K", 1, 2160, 3840), ("16x1080p", 16, 1080, 1920), ("1x640x480", 1, 480, 640)]
MILD5 = [-0.21, 0.07, 0.0013, -0.0009, -0.011]


def mild5(rows, cols):
    """(camera matrix, distortion coefficients): focal length 0.8 * cols, the principal point near the centre"""
    f = 0.8 * cols
    return [f, 0.0, cols / 2.0 - 0.37, 0.0, f * 1.01, rows / 2.0 + 0.29, 0.0, 0.0, 1.0], MILD5


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
    """makers: [(extra fields of the record, make_tracker(rows, cols, n) -> a MotionTracker / SubtractionTracker, BGR, switch
    off)]; every maker runs on one pool a shape.  -> one record a shape, maker and variant"""
    import numpy as np
    import torch
    from oat_amd.synth import make_pool
    out = []
    for name, n, rows, cols in SHAPES:
        frames = 8
        given = torch.from_numpy(np.stack(make_pool(rows, cols, n, frames, n_discs=3))).cuda()     # [frames][n][rows][cols][3]
        und = torch.empty_like(given)
        torch.cuda.synchronize()
        for extra, make_tracker in makers:
            tr = make_tracker(rows, cols, n)
            for s in range(n):
                tr.set_undistort(s, *mild5(rows, cols))
            remap = lambda i, o: tr._chk(tr.lib.oatgpu_undistort_dev(tr.ctx, C.c_void_p(i), C.c_void_p(o)))   # noqa: E731  (the tracker's own context and stream)
            for t in range(frames):
                remap(given[t].data_ptr(), und[t].data_ptr())
            tr._chk(tr.lib.oatgpu_synchronize(tr.ctx))
            for variant in ("moving", "quiet"):
                ix = (lambda t: t % frames) if variant == "moving" else (lambda t: 0)
                gp, up = [given[ix(t)].data_ptr() for t in range(steps)], [und[ix(t)].data_ptr() for t in range(steps)]
                rec = {"shape": name, "streams": n, "rows": rows, "cols": cols, "frames": variant, "steps": steps, "warmup": warmup}
                rec.update(extra)
                # (c) the floor
                tr.undistort(False)
                rec["packed_sync_us"] = _median_us(lambda t: tr.track_dev(up[t % steps]), steps, warmup)
                rec["packed_sequence_us"] = round(_median_us(lambda t: tr.track_sequence_dev(up), 5, 1) / steps, 1)

                # (b) the parent's way
                def parent_sync(t):
                    remap(gp[t % steps], up[t % steps])
                    tr.track_dev(up[t % steps])

                def parent_seq(_):
                    for t in range(steps):
                        remap(gp[t], up[t])
                    tr.track_sequence_dev(up)
                rec["undistort_sync_us"] = _median_us(parent_sync, steps, warmup)
                rec["undistort_sequence_us"] = round(_median_us(parent_seq, 5, 1) / steps, 1)
                # (a) the remap inside the front kernel
                tr.undistort(True)
                rec["fused_sync_us"] = _median_us(lambda t: tr.track_dev(gp[t % steps]), steps, warmup)
                rec["fused_sequence_us"] = round(_median_us(lambda t: tr.track_sequence_dev(gp), 5, 1) / steps, 1)
                for leg in ("sync", "sequence"):
                    rec[f"undistort_over_fused_{leg}"] = round(rec[f"undistort_{leg}_us"] / rec[f"fused_{leg}_us"], 2)
                out.append(rec)
            tr.close()
        del given, und
        torch.cuda.empty_cache()
    return out
