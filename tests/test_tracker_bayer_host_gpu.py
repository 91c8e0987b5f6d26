"""GPU tests of `oat-posidet-hip --bayer` in process pipelines: oat-frameserve-raw -C GREY (RAW8 frames) -> oat-posidet-hip diff
--bayer GRBG -> oat-posi-cout gives, token by token (tick, validity, position), what the chain that needs no --bayer gives on
the same source: oat-framefilt-hip debayer --pattern GRBG -> oat-posidet-hip diff --bgr.  The same for hsv --bsub --bayer with
--bsub-alpha 0.05.  (The start-up refusals need no device: tests/test_tracker_bayer_cpu.py.)"""
import json
import os
import subprocess
import uuid

import numpy as np
import pytest

import bsub_cases as B
import debayer_ref as R
import diff_cases as D
from test_host_pipeline import _consumers_ready, host_bins  # noqa: F401  (the fixture builds the binaries)

pytestmark = pytest.mark.gpu

ROWS, COLS, N = R.TRACK_ROWS, R.TRACK_COLS, 12
PATTERN = R.GRBG


def _pipeline(host_bins, tmp_path, name, raw_frames, det_args, debayer):  # noqa: F811
    """feeder (RAW8, GREY-tagged) -> [framefilt debayer ->] posidet -> posi-cout; -> [(tick, pos_ok, pos_xy)]"""
    src = tmp_path / f"{name}.raw"
    np.stack(raw_frames).tofile(src)
    tag = "oat_t_" + uuid.uuid4().hex[:8]
    a_raw, a_bgr, a_pos = tag + "raw", tag + "bgr", tag + "pos"
    bin_ = lambda n: os.path.join(host_bins, n)       # noqa: E731
    reader = subprocess.Popen([bin_("oat-posi-cout"), a_pos], stdout=subprocess.PIPE, text=True)
    procs, det_src, consumers = [reader], a_raw, [a_pos, a_raw]
    if debayer:
        det_src = a_bgr
        consumers.append(a_bgr)
    det = subprocess.Popen([bin_("oat-posidet-hip"), det_args[0], det_src, a_pos] + det_args[1:], stderr=subprocess.PIPE, text=True)
    procs.append(det)
    if debayer:
        procs.append(subprocess.Popen([bin_("oat-framefilt-hip"), "debayer", a_raw, a_bgr, "--pattern", R.NAMES[PATTERN]],
                                      stderr=subprocess.DEVNULL))
    _consumers_ready(*consumers)
    feeder = subprocess.Popen([bin_("oat-frameserve-raw"), a_raw, "-f", str(src), "--rows", str(ROWS), "--cols", str(COLS), "-C", "GREY",
                               "-n", str(len(raw_frames)), "-r", "200"])
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
        subprocess.run([bin_("oat-clean-hip"), a_raw, a_bgr, a_pos], capture_output=True)
    assert det.returncode == 0, err
    return [(g["tick"], g["pos_ok"], g.get("pos_xy")) for g in (json.loads(l) for l in out.splitlines() if l.strip())]


def test_posidet_diff_bayer_equals_debayer_in_front_of_diff_bgr(host_bins, tmp_path):  # noqa: F811
    c = D.make_case("host-raw", ROWS, COLS, 3, 1, n_frames=N, seed=7)
    raw = [R.mosaic(fs[0], PATTERN) for fs in c.frames]
    common = ["-d", "12", "-b", "2", "-a", "[2,1000000]"]
    want = _pipeline(host_bins, tmp_path, "bgr", raw, ["diff", "--bgr"] + common, debayer=True)
    got = _pipeline(host_bins, tmp_path, "raw", raw, ["diff", "--bayer", R.NAMES[PATTERN]] + common, debayer=False)
    assert len(want) == N and got == want
    assert sum(ok for _, ok, _ in want) >= N // 2


def test_posidet_hsv_bsub_bayer_equals_debayer_in_front_of_hsv_bsub(host_bins, tmp_path):  # noqa: F811
    c = B.make_case("host-raw", ROWS, COLS, 3, 1, alpha=0.05, erode=0, dilate=10, n_frames=N, seed=7)
    raw = [R.mosaic(fs[0], PATTERN) for fs in c.frames]
    w = B.HSV_WIN
    common = ["--bsub", "--bsub-alpha", "0.05", "-H", "[%d,%d]" % w["h"], "-S", "[%d,%d]" % w["s"], "-V", "[%d,%d]" % w["v"],
              "-a", "[2,1000000]"]
    want = _pipeline(host_bins, tmp_path, "bgr", raw, ["hsv"] + common, debayer=True)
    got = _pipeline(host_bins, tmp_path, "raw", raw, ["hsv", "--bayer", R.NAMES[PATTERN]] + common, debayer=False)
    assert len(want) == N and got == want
    assert sum(ok for _, ok, _ in want) >= N // 2
