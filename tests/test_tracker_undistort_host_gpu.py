"""GPU tests of `oat-posidet-hip --camera-matrix --distortion-coeffs` in process pipelines: oat-frameserve-raw -> oat-posidet-hip diff
--bgr --camera-matrix K --distortion-coeffs D -> oat-posi-cout gives, token by token (tick, validity, position), what the chain
that needs no calibration in the detector gives on the same source: oat-framefilt-hip undistort -> oat-posidet-hip diff --bgr.  The
same for hsv --bsub with --bsub-alpha 0.05, for the GREY chains (diff, thresh --bsub), and with the calibration read from the -c
FILE KEY table.  (The start-up refusals need no device: tests/test_tracker_undistort_cpu.py.)"""
import json
import os
import subprocess
import uuid

import numpy as np
import pytest

import bsub_cases as B
import diff_cases as D
import undistort_ref as R
from test_host_pipeline import _consumers_ready, host_bins  # noqa: F401  (the fixture builds the binaries)

pytestmark = pytest.mark.gpu

ROWS, COLS, N = 90, 200, 24
K, DIST = R.cases(ROWS, COLS)["mild5"]
_arr = lambda v: "[" + ",".join(repr(float(x)) for x in v) + "]"       # noqa: E731
CAL = ["--camera-matrix", _arr(K), "--distortion-coeffs", _arr(DIST)]


def _pipeline(host_bins, tmp_path, name, frames, det_args, undistort):  # noqa: F811
    """feeder -> [framefilt undistort ->] posidet -> posi-cout; -> [(tick, pos_ok, pos_xy)]"""
    src = tmp_path / f"{name}.raw"
    np.stack(frames).tofile(src)
    color = "BGR" if frames[0].ndim == 3 else "GREY"
    tag = "oat_t_" + uuid.uuid4().hex[:8]
    a_raw, a_und, a_pos = tag + "raw", tag + "und", tag + "pos"
    bin_ = lambda n: os.path.join(host_bins, n)       # noqa: E731
    reader = subprocess.Popen([bin_("oat-posi-cout"), a_pos], stdout=subprocess.PIPE, text=True)
    procs, det_src, consumers = [reader], a_raw, [a_pos, a_raw]
    if undistort:
        det_src = a_und
        consumers.append(a_und)
    det = subprocess.Popen([bin_("oat-posidet-hip"), det_args[0], det_src, a_pos] + det_args[1:], stderr=subprocess.PIPE, text=True)
    procs.append(det)
    if undistort:
        procs.append(subprocess.Popen([bin_("oat-framefilt-hip"), "undistort", a_raw, a_und] + CAL, stderr=subprocess.DEVNULL))
    _consumers_ready(*consumers)
    feeder = subprocess.Popen([bin_("oat-frameserve-raw"), a_raw, "-f", str(src), "--rows", str(ROWS), "--cols", str(COLS), "-C", color,
                               "-n", str(len(frames)), "-r", "200"])
    procs.append(feeder)
    try:
        out, _ = reader.communicate(timeout=120)
        feeder.wait(timeout=60)
        _, err = det.communicate(timeout=60)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
        subprocess.run([bin_("oat-clean-hip"), a_raw, a_und, a_pos], capture_output=True)
    assert det.returncode == 0, err
    return [(g["tick"], g["pos_ok"], g.get("pos_xy")) for g in (json.loads(l) for l in out.splitlines() if l.strip())]


def _diff_frames(channels):
    c = D.make_case("host-und", ROWS, COLS, channels, 1, n_frames=12, seed=7)
    return [fs[0] for fs in c.frames] * 2                      # (the second round starts with a jump back: motion all the same)


def _bsub_frames(channels):
    c = B.make_case("host-und", ROWS, COLS, channels, 1, alpha=0.05, erode=0, dilate=10, n_frames=N, seed=7)
    return [fs[0] for fs in c.frames]


def _table(tmp_path):
    cfg = tmp_path / "cal.toml"
    cfg.write_text("[lens]\ncamera-matrix = " + _arr(K) + "\ndistortion-coeffs = " + _arr(DIST) + "\n")
    return ["-c", str(cfg), "lens"]


@pytest.mark.parametrize("form", ["options", "table"])
def test_posidet_diff_bgr_with_a_calibration_equals_undistort_in_front(host_bins, tmp_path, form):  # noqa: F811
    frames = _diff_frames(3)
    common = ["-d", "12", "-b", "2", "-a", "[2,1000000]"]
    want = _pipeline(host_bins, tmp_path, "two", frames, ["diff", "--bgr"] + common, undistort=True)
    got = _pipeline(host_bins, tmp_path, "one", frames, ["diff", "--bgr"] + common + (CAL if form == "options" else _table(tmp_path)),
                    undistort=False)
    assert len(want) == N and got == want
    assert sum(ok for _, ok, _ in want) >= N // 2


def test_posidet_diff_on_a_grey_source_with_a_calibration(host_bins, tmp_path):  # noqa: F811
    frames = _diff_frames(1)
    common = ["-d", "12", "-b", "2", "-a", "[2,1000000]"]
    want = _pipeline(host_bins, tmp_path, "two", frames, ["diff"] + common, undistort=True)
    got = _pipeline(host_bins, tmp_path, "one", frames, ["diff"] + common + CAL, undistort=False)
    assert len(want) == N and got == want
    assert sum(ok for _, ok, _ in want) >= N // 2


@pytest.mark.parametrize("form", ["options", "table"])
def test_posidet_hsv_bsub_with_a_calibration_equals_undistort_in_front(host_bins, tmp_path, form):  # noqa: F811
    frames = _bsub_frames(3)
    w = B.HSV_WIN
    common = ["--bsub", "--bsub-alpha", "0.05", "-H", "[%d,%d]" % w["h"], "-S", "[%d,%d]" % w["s"], "-V", "[%d,%d]" % w["v"],
              "-a", "[2,1000000]"]
    want = _pipeline(host_bins, tmp_path, "two", frames, ["hsv"] + common, undistort=True)
    got = _pipeline(host_bins, tmp_path, "one", frames, ["hsv"] + common + (CAL if form == "options" else _table(tmp_path)),
                    undistort=False)
    assert len(want) == N and got == want
    assert sum(ok for _, ok, _ in want) >= N // 2


def test_posidet_thresh_bsub_with_a_calibration_equals_undistort_in_front(host_bins, tmp_path):  # noqa: F811
    frames = _bsub_frames(1)
    common = ["--bsub", "--bsub-alpha", "0.05", "-T", "[%d,%d]" % B.GREY_WIN, "-a", "[2,1000000]"]
    want = _pipeline(host_bins, tmp_path, "two", frames, ["thresh"] + common, undistort=True)
    got = _pipeline(host_bins, tmp_path, "one", frames, ["thresh"] + common + CAL, undistort=False)
    assert len(want) == N and got == want
    assert sum(ok for _, ok, _ in want) >= N // 2
