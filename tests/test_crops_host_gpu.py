"""GPU tests of `--crop-sinks` of oat-posidet-hip (target crops) in process pipelines on 37 x 61 frames:
oat-frameserve-raw -> oat-posidet-hip diff --bgr --target-sinks .. --crop-sinks .. -> oat-posi-cout and oat-frame-dump readers; the
same through hsv --bsub with --target-shape --crop-axis and the options in a -c table; and diff --track-sinks .. --crop-sinks ..,
where crop sink i carries the window of the rank track slot i took.  Every byte of every crop token is compared with the model
of tests/crops_ref.py, every token carries its frame's Sample, and the position sinks carry what they carry without the option."""
import json
import os
import subprocess
import uuid

import numpy as np
import pytest

import crops_cases as CC
import crops_ref as R
import targets_cases as T
import test_targets_host_gpu as TH
import tracks_cases as TC
import tracks_ref as TR
from test_targets_host_gpu import host_bins  # noqa: F401  (the fixture builds the binaries)

pytestmark = pytest.mark.gpu

FPS = 200


def _run(bins, tmp_path, component, source, frames, color, position_sinks, crop_sinks):
    """-> ({position sink: tokens}, {crop sink: (lines, bytes)})"""
    B = lambda b: os.path.join(bins, b)      # noqa: E731
    rows, cols = frames[0].shape[:2]
    files = {a: open(tmp_path / f"{a}.out", "w+") for a in position_sinks + crop_sinks}
    readers = [subprocess.Popen([B("oat-posi-cout"), a], stdout=files[a], stderr=subprocess.DEVNULL, text=True) for a in position_sinks]
    readers += [subprocess.Popen([B("oat-frame-dump"), a, str(tmp_path / f"{a}.raw")], stdout=files[a], stderr=subprocess.DEVNULL, text=True)
                for a in crop_sinks]
    proc = subprocess.Popen([B(component[0])] + component[1:])
    TH._consumers_ready(source, *position_sinks, *crop_sinks)
    raw = tmp_path / "frames.raw"
    np.stack(frames).tofile(raw)
    feeder = subprocess.Popen([B("oat-frameserve-raw"), source, "-f", str(raw), "--rows", str(rows), "--cols", str(cols), "-C", color,
                               "-n", str(len(frames)), "-r", str(FPS)])
    pos, crops = {}, {}
    try:
        for r, a in zip(readers, position_sinks + crop_sinks):
            r.wait(timeout=120)
            files[a].seek(0)
            lines = [l for l in files[a].read().splitlines() if l.strip()]
            if a in position_sinks:
                pos[a] = [json.loads(l) for l in lines]
            else:
                crops[a] = (lines, np.fromfile(tmp_path / f"{a}.raw", np.uint8))
        feeder.wait(timeout=60)
        proc.wait(timeout=60)
    finally:
        for p in readers + [feeder, proc]:
            if p.poll() is None:
                p.kill()
        subprocess.run([B("oat-clean-hip"), source] + position_sinks + crop_sinks, capture_output=True)
    assert proc.returncode == 0
    return pos, crops


def _check_crop_sink(got, want, h, w, color, tag):
    """got: (oat-frame-dump's lines, its dump); want[t]: the frame's window"""
    lines, data = got
    assert len(lines) == len(want), (tag, len(lines))
    assert lines == [f"{h} {w} {color} {t + 1}" for t in range(len(want))], (tag, lines[:3])       # the size, the colour, the frame's Sample
    data = data.reshape((len(want),) + want[0].shape)
    for t, x in enumerate(want):
        assert np.array_equal(data[t], x), (tag, t)


def test_posidet_diff_bgr_crop_sinks(host_bins, tmp_path):  # noqa: F811
    rows, cols, k, h, w = 37, 61, 4, 16, 12
    frames = CC.sequence("motion", rows, cols, 0)
    ranks = CC.sequence_targets("motion", rows, cols, 0, 0.0, k)
    want = CC.sequence_crops("motion", rows, cols, 0, 0.0, k, False, h, w)
    tag = "oat_c_" + uuid.uuid4().hex[:8]
    src, snk = tag + "raw", tag + "pos"
    tsinks, csinks = [tag + f"t{j}" for j in range(k)], [tag + f"c{j}" for j in range(3)]          # fewer crop sinks than K
    base = ["oat-posidet-hip", "diff", src, snk, "--bgr", "-d", str(T.DIFF["diff_threshold"]), "-b", str(T.DIFF["blur"]), "-a",
            "[2,1000000]", "--target-sinks", ",".join(tsinks)]
    pos, crops = _run(host_bins, tmp_path, base + ["--crop-sinks", ",".join(csinks), "--crop-size", f"{h}x{w}"], src, frames, "BGR",
                      [snk] + tsinks, csinks)
    for j, a in enumerate(csinks):
        _check_crop_sink(crops[a], [c[j] for c in want], h, w, "BGR", j)
    assert any(not r["valid"] for rs, _ in ranks[2:] for r in rs[:3]) and any(c[:3].any() for c in want)
    for t, (rs, _) in enumerate(ranks):
        TH._check_token(pos[snk][t], t, rs[0], ("sink", t))
        for j in range(k):
            TH._check_token(pos[tsinks[j]][t], t, rs[j], (j, t))
    plain, _ = _run(host_bins, tmp_path, base, src, frames, "BGR", [snk] + tsinks, [])
    assert plain == pos                                                # the position sinks carry what they carry without the option


def test_posidet_hsv_bsub_crop_axis_from_a_config_table(host_bins, tmp_path):  # noqa: F811
    rows, cols, k, h, w, alpha = 37, 61, 4, 8, 8, 0.05
    frames = CC.sequence("subtraction", rows, cols, 1)
    ranks = CC.sequence_targets("subtraction", rows, cols, 1, alpha, k)
    shapes = CC.sequence_shapes("subtraction", rows, cols, 1, alpha, k)
    want = CC.sequence_crops("subtraction", rows, cols, 1, alpha, k, True, h, w)
    assert any(s["valid"] and s["axis_valid"] for ss in shapes for s in ss) and any(s["valid"] and not s["axis_valid"] for ss in shapes for s in ss)
    tag = "oat_c_" + uuid.uuid4().hex[:8]
    src, snk = tag + "raw", tag + "pos"
    tsinks, csinks = [tag + f"t{j}" for j in range(k)], [tag + f"c{j}" for j in range(k)]
    cfg = tmp_path / "det.toml"
    cfg.write_text('[det]\ntarget-sinks = "%s"\ntarget-shape = true\ncrop-sinks = "%s"\ncrop-size = "%dx%d"\ncrop-axis = true\n'
                   % (",".join(tsinks), ",".join(csinks), h, w))
    win = T.sub_window()
    argv = ["oat-posidet-hip", "hsv", src, snk, "--bsub", "--bsub-alpha", repr(alpha), "-H", "[%d,%d]" % tuple(win["h"]),
            "-S", "[%d,%d]" % tuple(win["s"]), "-V", "[%d,%d]" % tuple(win["v"]), "-e", str(T.SUB_MORPH[0]), "-d", str(T.SUB_MORPH[1]),
            "-a", "[2,1000000]", "-c", str(cfg), "det"]
    pos, crops = _run(host_bins, tmp_path, argv, src, frames, "BGR", [snk], csinks)
    for j, a in enumerate(csinks):
        _check_crop_sink(crops[a], [c[j] for c in want], h, w, "BGR", j)
    for t, (rs, _) in enumerate(ranks):
        TH._check_token(pos[snk][t], t, rs[0], ("sink", t))


def test_posidet_diff_track_sinks_crop_sinks(host_bins, tmp_path):  # noqa: F811
    """Identity is the sink: crop sink i carries the window of the rank slot i took, zeros while the slot has none."""
    rows, cols, channels = TC.GEOMETRIES[1]
    assert (rows, cols, channels) == (37, 61, 1)
    k, h, w = TC.IMG_K, 16, 12
    frames = TC.sequence("motion", rows, cols, channels, 0)
    targets = TC.image_targets("motion", rows, cols, channels, 0, 0.0, k)
    slots, _ = TR.run([TC.triples(r) for r, _ in targets], k, kalman=TC.IMG_KALMAN, gate=TC.IMG_GATE)
    want = []
    for t, f in enumerate(frames):
        wins = [R.window(True, True, targets[t][0][s["rank"]]["x"], targets[t][0][s["rank"]]["y"]) if s["id"] and s["rank"] >= 0
                else R.INVALID for s in slots[t]]
        want.append([R.crop(f, win, h, w) for win in wins])
    assert len({s["rank"] for ss in slots for s in ss if s["id"] and s["rank"] >= 0 and s is ss[0]}) > 1, "slot 0 never changes its rank"
    assert any(s["id"] and s["rank"] < 0 for ss in slots for s in ss), "no live slot without a rank"
    tag = "oat_c_" + uuid.uuid4().hex[:8]
    src, snk = tag + "raw", tag + "pos"
    ksinks, csinks = [tag + f"k{i}" for i in range(k)], [tag + f"c{i}" for i in range(k)]
    kp = TC.IMG_KALMAN
    argv = ["oat-posidet-hip", "diff", src, snk, "-d", str(TC.DIFF["diff_threshold"]), "-b", str(TC.DIFF["blur"]), "-a", "[%d,%d]" % TC.DC.AREA,
            "--track-sinks", ",".join(ksinks), "--track-gate", repr(TC.IMG_GATE), "--kalman", "--dt", repr(kp["dt"]), "--timeout",
            repr(kp["timeout"]), "--sigma-accel", repr(kp["sigma_accel"]), "--sigma-noise", repr(kp["sigma_noise"]),
            "--crop-sinks", ",".join(csinks), "--crop-size", f"{h}x{w}"]
    pos, crops = _run(host_bins, tmp_path, argv, src, frames, "GREY", [snk] + ksinks, csinks)
    for i, a in enumerate(csinks):
        _check_crop_sink(crops[a], [c[i] for c in want], h, w, "GREY", i)
    for a in [snk] + ksinks:
        assert len(pos[a]) == len(frames), a
