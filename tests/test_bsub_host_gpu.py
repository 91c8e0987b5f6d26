"""GPU test of `oat-posidet-hip hsv|thresh --bsub` in a process pipeline: oat-frameserve-raw -> oat-posidet-hip hsv --bsub
--bsub-alpha 0.05 -> oat-posi-cout equals the oracle chain `framefilt bsub -> col -C HSV -> posidet hsv` on a BGR source, and
thresh --bsub --bsub-background FILE.pgm (the keys from a -c table) the chain `framefilt bsub -f FILE -> posidet thresh` on a GREY
one, token by token; the --bsub-* options without --bsub, or on TYPE diff, are errors."""
import json
import os
import subprocess
import uuid

import numpy as np
import pytest

import bsub_cases as B
from test_host_pipeline import _consumers_ready, host_bins  # noqa: F401  (the fixture builds the binaries)

pytestmark = pytest.mark.gpu

ROWS, COLS, N = 48, 64, 20
AREA_ARG = "[2,1000000]"


def _run(host_bins, tmp_path, frames, color, det_args):
    raw = tmp_path / "frames.raw"
    np.stack(frames).tofile(raw)
    tag = "oat_t_" + uuid.uuid4().hex[:8]
    a_raw, a_pos = tag + "raw", tag + "pos"
    bin_ = lambda n: os.path.join(host_bins, n)
    reader = subprocess.Popen([bin_("oat-posi-cout"), a_pos], stdout=subprocess.PIPE, text=True)
    det = subprocess.Popen([bin_("oat-posidet-hip"), det_args[0], a_raw, a_pos] + det_args[1:], stderr=subprocess.PIPE, text=True)
    _consumers_ready(a_pos, a_raw)
    feeder = subprocess.Popen([bin_("oat-frameserve-raw"), a_raw, "-f", str(raw), "--rows", str(ROWS), "--cols", str(COLS),
                               "-C", color, "-n", str(len(frames)), "-r", "200"])
    try:
        out, _ = reader.communicate(timeout=120)
        feeder.wait(timeout=60)
        _, err = det.communicate(timeout=60)
    finally:
        for p in (reader, det, feeder):
            if p.poll() is None:
                p.kill()
                p.wait()
        subprocess.run([bin_("oat-clean-hip"), a_raw, a_pos], capture_output=True)
    assert det.returncode == 0, err
    return [json.loads(l) for l in out.splitlines() if l.strip()]


def _compare(got, case, orc):
    assert len(got) == N
    hits = 0
    for t, g in enumerate(got):
        want = orc.step(case.frames[t][0])[0]
        assert g["tick"] == t + 1 and g["pos_ok"] == want["valid"], t
        if want["valid"]:
            hits += 1
            # (the token is JSON text truncated to five decimal places (datatypes.hpp: jsonNumber, the reference's serializer):
            # 1e-4 covers the printed precision, as in tests/test_diff_host_gpu.py; it is no tolerance on the arithmetic --
            # tests/test_bsub_tracker_gpu.py compares the integer sums and the centroid exactly)
            assert abs(g["pos_xy"][0] - want["x"]) < 1e-4 and abs(g["pos_xy"][1] - want["y"]) < 1e-4, t
    assert hits >= N // 2


def test_posidet_hsv_bsub_pipeline_matches_the_oracle_chain(host_bins, tmp_path):  # noqa: F811
    c = B.make_case("host-bgr", ROWS, COLS, 3, 1, alpha=0.05, erode=0, dilate=10, n_frames=N, seed=7)
    w = B.HSV_WIN
    got = _run(host_bins, tmp_path, [fs[0] for fs in c.frames], "BGR",
               ["hsv", "--bsub", "--bsub-alpha", "0.05", "-H", "[%d,%d]" % w["h"], "-S", "[%d,%d]" % w["s"], "-V", "[%d,%d]" % w["v"],
                "-a", AREA_ARG])
    _compare(got, c, B.Oracle(c))


def test_posidet_thresh_bsub_background_pipeline_matches_the_oracle_chain(host_bins, tmp_path):  # noqa: F811
    c = B.make_case("host-grey", ROWS, COLS, 1, 1, alpha=0.0, erode=0, dilate=0, background=True, n_frames=N, seed=8)
    pgm = tmp_path / "bg.pgm"
    with open(pgm, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (COLS, ROWS))
        f.write(c.background[0].tobytes())
    toml = tmp_path / "det.toml"
    toml.write_text('[det]\nbsub = true\nbsub-background = "%s"\nthresh = [%d, %d]\n' % (pgm, *B.GREY_WIN))
    got = _run(host_bins, tmp_path, [fs[0] for fs in c.frames], "GREY", ["thresh", "-c", str(toml), "det", "-a", AREA_ARG])
    _compare(got, c, B.Oracle(c, c.background[0]))


@pytest.mark.parametrize("args,needle", [
    (["hsv", "--bsub-alpha", "0.05"], "need --bsub"),
    (["thresh", "--bsub-background", "bg.pgm"], "need --bsub"),
    (["diff", "--bsub"], "hsv or thresh only"),
    (["diff", "--bsub-alpha", "0.1"], "hsv or thresh only"),
    (["hsv", "--bsub", "--bsub-alpha", "1.5"], "out of range"),
    (["thresh", "--bsub", "--bsub-alpha", "0.1", "--bsub-background", "bg.pgm"], "cannot adapt"),
])
def test_option_errors(host_bins, args, needle):  # noqa: F811
    r = subprocess.run([os.path.join(host_bins, "oat-posidet-hip"), args[0], "oat_t_nosrc", "oat_t_nosnk"] + args[1:],
                       capture_output=True, text=True, timeout=30)
    assert r.returncode == 255 and needle in r.stderr, r.stderr


def test_a_config_table_with_bsub_keys_but_no_bsub_is_an_error(host_bins, tmp_path):  # noqa: F811
    toml = tmp_path / "det.toml"
    toml.write_text("[det]\nbsub-alpha = 0.05\n")
    r = subprocess.run([os.path.join(host_bins, "oat-posidet-hip"), "hsv", "oat_t_nosrc", "oat_t_nosnk", "-c", str(toml), "det"],
                       capture_output=True, text=True, timeout=30)
    assert r.returncode == 255 and "need --bsub" in r.stderr, r.stderr
