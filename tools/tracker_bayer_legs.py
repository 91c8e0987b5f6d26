"""The `--bayer` leg of tools/diff_bench.py and tools/bsub_track_bench.py: what a batched tracker's step costs on Bayer RAW8
frames with the demosaic inside the front kernel (oatgpu_set_tracker_bayer) against the way the same work had to
be done before it, on the same raw frames, and against the BGR step alone.

Shapes: 1 x 4K, 16 x 1080p, 1 x 640x480; the raw frames are the RGGB mosaic of the tools' BGR pool, the BGR frames of legs (b)
and (c) are oatgpu_debayer_dev's output of them.  Legs, us a frame set, median of `steps` after `warmup` (sequence: `steps`
frame sets in one call, the median of 5 calls after one, divided by `steps`):
  fused     (a) RAW8 through the tracker's own call, switch on: sync (device frames), sequence, host (host frames: rows*cols
            bytes a stream are uploaded);
  debayer   (b) oatgpu_debayer_dev into a BGR buffer followed by the BGR call, switch off, one context: sync, sequence (every
            frame set is demosaiced again, into the pool's BGR buffers, in front of the sequence call), host (the raw frames
            are copied to the device first, camera by camera from pageable memory as the tracker's own host call does);
  bgr       (c) the BGR call alone on the demosaiced frames: sync, sequence -- the floor.
`quiet`: the same legs on one frame set repeated: nothing moves, the masks are empty and the back half is at its cheapest, so
the front kernel's share of the step is at its largest.
Every timed call ends in a device synchronisation, so a host clock around it is the step."""
import statistics
import time

SHAPES = [("1x4K", 1, 2160, 3840), ("16x1080p", 16, 1080, 1920), ("1x640x480", 1, 480, 640)]
PATTERN = "RGGB"


def mosaic_rggb(bgr):
    """[..., rows, cols, 3] BGR -> [..., rows, cols] RGGB samples"""
    raw = bgr[..., 1].copy()
    raw[..., 0::2, 0::2] = bgr[..., 0::2, 0::2, 2]
    raw[..., 1::2, 1::2] = bgr[..., 1::2, 1::2, 0]
    return raw


def _median_us(call, steps, warmup):
    for t in range(warmup):
        call(t)
    d = []
    for t in range(steps):
        t0 = time.perf_counter()
        call(warmup + t)
        d.append(time.perf_counter() - t0)
    return round(statistics.median(d) * 1e6, 1)


def run(make_tracker, steps, warmup, extra=None):
    """make_tracker(rows, cols, n) -> a MotionTracker / SubtractionTracker (BGR, switch off).  -> one record a shape and variant"""
    import numpy as np
    import torch
    import oat_amd
    from oat_amd.synth import make_pool
    out = []
    for name, n, rows, cols in SHAPES:
        frames = 8
        raw_host = mosaic_rggb(np.stack(make_pool(rows, cols, n, frames, n_discs=3)))   # [frames][n][rows][cols]
        raw = torch.from_numpy(raw_host).cuda()
        bgr = torch.empty((frames, n, rows, cols, 3), dtype=torch.uint8, device="cuda")
        stage = torch.empty((n, rows, cols), dtype=torch.uint8, device="cuda")          # leg (b) on host frames: the raw set
        torch.cuda.synchronize()
        tr = make_tracker(rows, cols, n)
        deb = lambda i, o: oat_amd.Debayer.filter_dev(tr, i, o, PATTERN)                # noqa: E731  (the tracker's own context and stream)
        for t in range(frames):
            deb(raw[t].data_ptr(), bgr[t].data_ptr())
        tr._chk(tr.lib.oatgpu_synchronize(tr.ctx))
        for variant in ("moving", "quiet"):
            ix = (lambda t: t % frames) if variant == "moving" else (lambda t: 0)
            rp, bp = [raw[ix(t)].data_ptr() for t in range(steps)], [bgr[ix(t)].data_ptr() for t in range(steps)]
            rec = {"shape": name, "streams": n, "rows": rows, "cols": cols, "frames": variant, "steps": steps, "warmup": warmup}
            if extra:
                rec.update(extra)
            # (c) the floor
            tr.bayer(None)
            rec["bgr_sync_us"] = _median_us(lambda t: tr.track_dev(bp[t % steps]), steps, warmup)
            rec["bgr_sequence_us"] = round(_median_us(lambda t: tr.track_sequence_dev(bp), 5, 1) / steps, 1)

            # (b) the parent's way
            def parent_sync(t):
                deb(rp[t % steps], bp[t % steps])
                tr.track_dev(bp[t % steps])

            def parent_seq(_):
                for t in range(steps):
                    deb(rp[t], bp[t])
                tr.track_sequence_dev(bp)

            def parent_host(t):
                for s in range(n):                      # camera by camera, as the tracker's own host call copies them
                    stage[s].copy_(torch.from_numpy(raw_host[ix(t), s]), non_blocking=True)
                torch.cuda.synchronize()
                deb(stage.data_ptr(), bp[t % steps])
                tr.track_dev(bp[t % steps])
            rec["debayer_sync_us"] = _median_us(parent_sync, steps, warmup)
            rec["debayer_sequence_us"] = round(_median_us(parent_seq, 5, 1) / steps, 1)
            rec["debayer_host_us"] = _median_us(parent_host, steps, warmup)
            # (a) the demosaic inside the front kernel
            tr.bayer(PATTERN)
            rec["fused_sync_us"] = _median_us(lambda t: tr.track_dev(rp[t % steps]), steps, warmup)
            rec["fused_sequence_us"] = round(_median_us(lambda t: tr.track_sequence_dev(rp), 5, 1) / steps, 1)
            rec["fused_host_us"] = _median_us(lambda t: tr.track(list(raw_host[ix(t)])), steps, warmup)
            for leg in ("sync", "sequence", "host"):
                rec[f"debayer_over_fused_{leg}"] = round(rec[f"debayer_{leg}_us"] / rec[f"fused_{leg}_us"], 2)
            out.append(rec)
        tr.close()
        del raw, bgr, stage
        torch.cuda.empty_cache()
    return out
