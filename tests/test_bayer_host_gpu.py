"""GPU tests of the Bayer stage in process pipelines: oat-frameserve-raw -C GREY -> oat-framefilt-hip debayer publishes the
model's frames (read back by oat-frame-dump), and oat-track-hip --bayer on two cameras gives, token by token, what the BGR
pipeline gives on the model's frames (tests/debayer_ref.py) -- with END on one camera in the middle of a round."""
import json
import os
import subprocess
import uuid

import numpy as np
import pytest

import debayer_ref as D
from test_host_pipeline import _consumers_ready, host_bins  # noqa: F401  (the fixture builds the binaries)

pytestmark = pytest.mark.gpu

ROWS, COLS = D.TRACK_ROWS, D.TRACK_COLS


def _stop(host_bins, procs, addresses):
    for p in procs:
        if p.poll() is None:
            p.kill()
            p.wait()
    subprocess.run([os.path.join(host_bins, "oat-clean-hip"), *addresses], capture_output=True)


@pytest.mark.parametrize("pattern", [D.RGGB, D.GBRG])
def test_framefilt_debayer_publishes_the_models_frames(host_bins, tmp_path, pattern):  # noqa: F811
    raw, model = D.track_sequence(7, pattern)
    src = tmp_path / "raw8.raw"
    np.stack(raw).tofile(src)
    dump = tmp_path / "bgr.raw"
    tag = "oat_t_" + uuid.uuid4().hex[:8]
    a_raw, a_bgr = tag + "raw", tag + "bgr"
    B = lambda b: os.path.join(host_bins, b)
    reader = subprocess.Popen([B("oat-frame-dump"), a_bgr, str(dump)], stdout=subprocess.PIPE, text=True)
    filt = subprocess.Popen([B("oat-framefilt-hip"), "debayer", a_raw, a_bgr, "--pattern", D.NAMES[pattern]],
                            stderr=subprocess.PIPE, text=True)
    _consumers_ready(a_bgr, a_raw)
    feeder = subprocess.Popen([B("oat-frameserve-raw"), a_raw, "-f", str(src), "--rows", str(ROWS), "--cols", str(COLS), "-C", "GREY",
                               "-n", str(len(raw)), "-r", "200"])
    try:
        out, _ = reader.communicate(timeout=120)
        feeder.wait(timeout=60)
        _, err = filt.communicate(timeout=60)
    finally:
        _stop(host_bins, [reader, filt, feeder], (a_raw, a_bgr))
    assert filt.returncode == 0, err
    lines = out.split("\n")[:-1]
    assert lines == [f"{ROWS} {COLS} BGR {t + 1}" for t in range(len(raw))]
    got = np.fromfile(dump, np.uint8).reshape(len(raw), ROWS, COLS, 3)
    for t in range(len(raw)):
        assert np.array_equal(got[t], model[t]), t


def test_framefilt_debayer_refusals(host_bins, tmp_path):  # noqa: F811
    B = lambda b: os.path.join(host_bins, b)
    r = subprocess.run([B("oat-framefilt-hip"), "debayer", "a", "b"], capture_output=True, text=True)
    assert r.returncode == 255 and "'pattern'" in r.stderr
    r = subprocess.run([B("oat-framefilt-hip"), "debayer", "a", "b", "--pattern", "RGBG"], capture_output=True, text=True)
    assert r.returncode == 255 and "Invalid Bayer pattern" in r.stderr
    r = subprocess.run([B("oat-track-hip"), "a", "b", "--bayer", "RGGB", "--thresh", "[1,256]"], capture_output=True, text=True)
    assert r.returncode == 255 and "--thresh" in r.stderr
    r = subprocess.run([B("oat-track-hip"), "a,b,c", "x,y,z", "--bayer", "RGGB,BGGR"], capture_output=True, text=True)
    assert r.returncode == 255 and "2 patterns for 3 SOURCEs" in r.stderr
    r = subprocess.run([B("oat-track-hip"), "a", "b", "--bayer", "XYZW"], capture_output=True, text=True)
    assert r.returncode == 255 and "Invalid Bayer pattern" in r.stderr


def _track(host_bins, tmp_path, name, streams_frames, color, extra):
    """n feeders -> ONE oat-track-hip -> n readers; nothing is waited for longer than the pipeline lives.  Tokens per camera."""
    n = len(streams_frames)
    tag = "oat_t_" + uuid.uuid4().hex[:8]
    srcs = [f"{tag}raw{s}" for s in range(n)]
    snks = [f"{tag}pos{s}" for s in range(n)]
    B = lambda b: os.path.join(host_bins, b)
    files = [open(tmp_path / f"{name}{s}.out", "w+") for s in range(n)]
    readers = [subprocess.Popen([B("oat-posi-cout"), a], stdout=f, stderr=subprocess.DEVNULL, text=True) for a, f in zip(snks, files)]
    tracker = subprocess.Popen([B("oat-track-hip"), ",".join(srcs), ",".join(snks), "-a", str(D.LR), "--area", "[10,1000000]",
                                "-H", "[100,125]", "-S", "[150,256]", "-V", "[100,256]", "-e", "0", "-d", "3", "--ring", "2"] + list(extra),
                               stderr=subprocess.PIPE, text=True)
    _consumers_ready(*srcs, *snks)
    feeders = []
    for s in range(n):
        raw = tmp_path / f"{name}{s}.raw"
        np.stack(streams_frames[s]).tofile(raw)
        feeders.append(subprocess.Popen([B("oat-frameserve-raw"), srcs[s], "-f", str(raw), "--rows", str(ROWS), "--cols", str(COLS),
                                         "-C", color, "-n", str(len(streams_frames[s])), "-r", "100"]))
    try:
        for r in readers:
            r.wait(timeout=120)
        _, err = tracker.communicate(timeout=60)
    finally:
        _stop(host_bins, readers + feeders + [tracker], srcs + snks)     # (a camera may still hold frames nobody will take)
    assert tracker.returncode == 0, err[-500:]
    out = []
    for fl in files:
        fl.seek(0)
        out.append([(g["tick"], g["pos_ok"], g.get("pos_xy")) for g in (json.loads(l) for l in fl.read().splitlines() if l.strip())])
    return out


def test_track_bayer_equals_the_bgr_pipeline_on_the_models_frames(host_bins, tmp_path):  # noqa: F811
    """Two cameras, one pattern (--bayer RGGB); camera 1's frame server stops 3 frames early: END in the middle of a round."""
    seqs = [D.track_sequence(1, D.RGGB), D.track_sequence(5, D.RGGB)]
    short = D.TRACK_T - 3
    raw = [seqs[0][0], seqs[1][0][:short]]
    model = [seqs[0][1], seqs[1][1][:short]]
    want = _track(host_bins, tmp_path, "bgr", model, "BGR", [])
    got = _track(host_bins, tmp_path, "raw", raw, "GREY", ["--bayer", "RGGB"])
    assert [len(w) for w in want] == [short, short]
    assert got == want
    assert sum(ok for cam in want for _, ok, _ in cam) >= short


def test_track_bayer_one_pattern_per_source(host_bins, tmp_path):  # noqa: F811
    seqs = [D.track_sequence(2, D.BGGR), D.track_sequence(3, D.GRBG)]
    want = _track(host_bins, tmp_path, "bgr", [s[1] for s in seqs], "BGR", [])
    got = _track(host_bins, tmp_path, "raw", [s[0] for s in seqs], "GREY", ["--bayer", "BGGR,GRBG"])
    assert [len(w) for w in want] == [D.TRACK_T] * 2 and got == want
    assert sum(ok for cam in want for _, ok, _ in cam) >= D.TRACK_T
