"""GPU test of `oat-posidet-hip diff --bgr` in a process pipeline: oat-frameserve-raw (BGR) -> oat-posidet-hip diff --bgr ->
oat-posi-cout equals the oracle chain `framefilt col -C GREY -> posidet diff`; without --bgr the same BGR source is refused
with the reference's words (Source.h:300-313), as before."""
import json
import os
import subprocess
import uuid

import numpy as np
import pytest

import diff_cases as D
import oracle_lib as O
from test_host_pipeline import _consumers_ready, host_bins  # noqa: F401  (the fixture builds the binaries)

pytestmark = pytest.mark.gpu

ROWS, COLS, N = 90, 200, 20


def _frames():
    return [fs[0] for fs in D.make_case("host", ROWS, COLS, 3, 1, n_frames=N, seed=7).frames]


def _start(host_bins, tmp_path, frames, det_args):
    raw = tmp_path / "frames.raw"
    np.stack(frames).tofile(raw)
    tag = "oat_t_" + uuid.uuid4().hex[:8]
    a_raw, a_pos = tag + "raw", tag + "pos"
    B = lambda n: os.path.join(host_bins, n)
    reader = subprocess.Popen([B("oat-posi-cout"), a_pos], stdout=subprocess.PIPE, text=True)
    det = subprocess.Popen([B("oat-posidet-hip"), "diff", a_raw, a_pos, "-d", "12", "-b", "2", "-a", "[2,1000000]"] + det_args,
                           stderr=subprocess.PIPE, text=True)
    _consumers_ready(a_pos, a_raw)
    feeder = subprocess.Popen([B("oat-frameserve-raw"), a_raw, "-f", str(raw), "--rows", str(ROWS), "--cols", str(COLS),
                               "-n", str(len(frames)), "-r", "200"])
    return reader, det, feeder, (a_raw, a_pos)


def _stop(host_bins, procs, addresses):
    for p in procs:
        if p.poll() is None:
            p.kill()
            p.wait()
    subprocess.run([os.path.join(host_bins, "oat-clean-hip"), *addresses], capture_output=True)


def test_posidet_diff_bgr_pipeline_matches_the_oracle_chain(host_bins, tmp_path):  # noqa: F811
    frames = _frames()
    reader, det, feeder, addr = _start(host_bins, tmp_path, frames, ["--bgr"])
    try:
        out, _ = reader.communicate(timeout=120)
        feeder.wait(timeout=60)
        _, err = det.communicate(timeout=60)
    finally:
        _stop(host_bins, [reader, det, feeder], addr)
    assert det.returncode == 0, err
    got = [json.loads(l) for l in out.splitlines() if l.strip()]
    assert len(got) == N
    orc = O.Diff(ROWS, COLS, 12, 2, 2.0, 1e6)
    hits = 0
    for t, (f, g) in enumerate(zip(frames, got)):
        want, _ = orc.detect(O.bgr2grey(f))
        assert g["tick"] == t + 1 and g["pos_ok"] == want["valid"], t
        if want["valid"]:
            hits += 1
            assert abs(g["pos_xy"][0] - want["x"]) < 1e-4 and abs(g["pos_xy"][1] - want["y"]) < 1e-4, t
    assert hits >= N // 2


def test_posidet_diff_without_bgr_still_refuses_a_bgr_source(host_bins, tmp_path):  # noqa: F811
    frames = _frames()[:4]
    reader, det, feeder, addr = _start(host_bins, tmp_path, frames, [])
    try:
        _, err = det.communicate(timeout=60)
    finally:
        _stop(host_bins, [reader, det, feeder], addr)
    assert det.returncode == 255
    assert "Component requires frame source with pixels of type GREY" in err and "oat-framefilt col" in err
