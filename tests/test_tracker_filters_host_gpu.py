"""GPU tests of `oat-posidet-hip --kalman --homography --region` in process pipelines: oat-frameserve-raw -> oat-posidet-hip diff
--bgr --kalman .. --homography .. --region .. -> oat-posi-cout publishes, token by token, the filtered Position2D of the reference
chain (tests/tracker_filters_cases.py): flags, WORLD unit, position, velocity, region name.  The same for hsv --bsub, once with
the chain read from the -c FILE KEY table and its [[KEY.region]] tables.  Without the options the pipeline publishes the
detector's token as before.  oat-posi-cout prints numbers cut to 5 places.  (The start-up refusals need no device:
tests/test_tracker_filters_cpu.py.)"""
import json
import os
import subprocess
import uuid

import numpy as np
import pytest

import bsub_cases as B
import diff_cases as D
import tracker_filters_cases as K
from test_host_pipeline import _consumers_ready, host_bins  # noqa: F401  (the fixture builds the binaries)

pytestmark = pytest.mark.gpu

ROWS, COLS, CH = K.GEOMETRIES[0]
CUT = 1e-5 * (1 + 1e-9)             # a number printed cut to 5 places is less than 1e-5 below its value


def _pipeline(host_bins, tmp_path, name, frames, det_args):  # noqa: F811
    """feeder -> posidet -> posi-cout; -> the JSON records"""
    src = tmp_path / f"{name}.raw"
    np.stack(frames).tofile(src)
    rows, cols = frames[0].shape[:2]
    color = "BGR" if frames[0].ndim == 3 else "GREY"
    tag = "oat_t_" + uuid.uuid4().hex[:8]
    a_raw, a_pos = tag + "raw", tag + "pos"
    bin_ = lambda n: os.path.join(host_bins, n)       # noqa: E731
    reader = subprocess.Popen([bin_("oat-posi-cout"), a_pos], stdout=subprocess.PIPE, text=True)
    det = subprocess.Popen([bin_("oat-posidet-hip"), det_args[0], a_raw, a_pos] + det_args[1:], stderr=subprocess.PIPE, text=True)
    procs = [reader, det]
    _consumers_ready(a_pos, a_raw)
    feeder = subprocess.Popen([bin_("oat-frameserve-raw"), a_raw, "-f", str(src), "--rows", str(rows), "--cols", str(cols), "-C", color,
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
        subprocess.run([bin_("oat-clean-hip"), a_raw, a_pos], capture_output=True)
    assert det.returncode == 0, err
    return [json.loads(l) for l in out.splitlines() if l.strip()]


def _num(v):
    return repr(float(v))


def _options(cfg):
    k, out = cfg["kalman"], []
    if k:
        out += ["--kalman", "--dt", _num(k["dt"]), "--timeout", _num(k["timeout"]), "--sigma-accel", _num(k["sigma_accel"]),
                "--sigma-noise", _num(k["sigma_noise"])]
    if cfg["homography"]:
        out += ["--homography", "[" + ",".join(_num(v) for v in cfg["homography"]) + "]"]
    for name, pts in cfg["regions"] or []:
        out += ["--region", name + "=[" + ",".join(f"[{x},{y}]" for x, y in pts) + "]"]
    return out


def _table(tmp_path, cfg, own):
    k = cfg["kalman"]
    text = "[det]\n" + "".join(f"{key} = {val}\n" for key, val in own)
    text += f"kalman = true\ndt = {_num(k['dt'])}\ntimeout = {_num(k['timeout'])}\nsigma-accel = {_num(k['sigma_accel'])}\n"
    text += f"sigma-noise = {_num(k['sigma_noise'])}\nhomography = [" + ", ".join(_num(v) for v in cfg["homography"]) + "]\n"
    for name, pts in cfg["regions"]:                  # points over several lines, as a hand-written file has them
        text += f'\n[[det.region]]\nname = "{name}"\npoints = [\n' + ",\n".join(f"  [{x}, {y}]" for x, y in pts) + "\n]\n"
    f = tmp_path / "rig.toml"
    f.write_text(text)
    return ["-c", str(f), "det"]


def _near(g, w):
    return all(abs(a - b) <= CUT for a, b in zip(g, w))


def _check_filtered(recs, want, unit=1, regions_hit=3):
    assert len(recs) == len(want)
    regions = set()
    for t, (g, ws) in enumerate(zip(recs, want)):
        w = ws[0]
        assert (g["tick"], g["unit"], g["pos_ok"], g["vel_ok"], g["head_ok"], g["reg_ok"]) == \
            (recs[0]["tick"] + t, unit, w["position_valid"], w["velocity_valid"], False, w["region_valid"]), (t, g, w)
        if w["position_valid"]:
            assert _near(g["pos_xy"], (w["x"], w["y"])) and _near(g["vel_xy"], (w["vx"], w["vy"])), (t, g, w)
        assert g.get("reg") == w["region"], (t, g, w)
        regions.add(w["region"])
    assert len(regions) >= regions_hit                # no region and two named ones


def _check_plain(recs, det):
    assert len(recs) == len(det)
    for t, (g, ds) in enumerate(zip(recs, det)):
        d = ds[0]
        assert (g["tick"], g["unit"], g["pos_ok"], g["vel_ok"], g["head_ok"], g["reg_ok"]) == \
            (recs[0]["tick"] + t, 0, bool(d["valid"]), False, False, False), (t, g, d)
        if d["valid"]:
            assert _near(g["pos_xy"], (d["x"], d["y"])), (t, g, d)
    assert sum(d[0]["valid"] for d in det) >= 6


DIFF_ARGS = ["-d", str(K.DIFF["diff_threshold"]), "-b", str(K.DIFF["blur"]), "-a", "[%d,%d]" % D.AREA]
_W = B.HSV_WIN
BSUB_ARGS = ["--bsub", "--bsub-alpha", "0", "-H", "[%d,%d]" % _W["h"], "-S", "[%d,%d]" % _W["s"], "-V", "[%d,%d]" % _W["v"],
             "-e", str(K.BSUB["erode"]), "-d", str(K.BSUB["dilate"]), "-a", "[%d,%d]" % B.AREA]


def _case(kind, name="all", geometry=(ROWS, COLS, CH)):
    frames = [fs[0] for fs in K.frames(kind, *geometry, 1)]
    return frames, K.detections(kind, *geometry, 1), K.config(name, kind, *geometry, 1), K.want(name, kind, *geometry, 1)


def test_posidet_diff_bgr_publishes_the_filtered_position(host_bins, tmp_path):  # noqa: F811
    frames, det, cfg, want = _case("diff")
    _check_plain(_pipeline(host_bins, tmp_path, "plain", frames, ["diff", "--bgr"] + DIFF_ARGS), det)
    _check_filtered(_pipeline(host_bins, tmp_path, "chain", frames, ["diff", "--bgr"] + DIFF_ARGS + _options(cfg)), want)


@pytest.mark.parametrize("form", ["options", "table"])
def test_posidet_hsv_bsub_publishes_the_filtered_position(host_bins, tmp_path, form):  # noqa: F811
    frames, det, cfg, want = _case("bsub")
    if form == "options":
        _check_plain(_pipeline(host_bins, tmp_path, "plain", frames, ["hsv"] + BSUB_ARGS), det)
        args = ["hsv"] + BSUB_ARGS + _options(cfg)
    else:
        args = ["hsv"] + BSUB_ARGS + _table(tmp_path, cfg, [])
    _check_filtered(_pipeline(host_bins, tmp_path, "chain", frames, args), want)


def test_plain_posidet_diff_with_a_filter_runs_the_motion_tracker_on_its_grey_source(host_bins, tmp_path):  # noqa: F811
    """--kalman alone on a GREY source: pixel units, position and velocity of the filter, the gap bridged"""
    frames, det, cfg, want = _case("diff", "k_long", K.GEOMETRIES[1])
    assert any(w[0]["position_valid"] and not d[0]["valid"] for w, d in zip(want, det))
    _check_filtered(_pipeline(host_bins, tmp_path, "chain", frames, ["diff"] + DIFF_ARGS + _options(cfg)), want, unit=0, regions_hit=1)
