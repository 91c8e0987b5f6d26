"""GPU test of `--track-sinks` of oat-posidet-hip (target tracks) in a process pipeline: oat-frameserve-raw ->
oat-posidet-hip diff --bgr --track-sinks a,b,c --track-gate G --kalman .. --homography .. -> four oat-posi-cout.  Every token of
every track sink is compared with the model of tests/tracks_ref.py on the oracle's detections (tests/tracks_cases.py): the
frame's Sample, the flags, WORLD units, position and velocity as oat-posi-cout prints them (cut to 5 places); the SINK carries
the filtered ordinary result, as without the option.  (The start-up refusals need no device: tests/test_tracks_cpu.py.)"""
import pytest

import marker_filters_ref as R
import oracle_lib as O
import posfilt_cases as P
import tracks_cases as TC
import tracks_ref as TR
from test_targets_host_gpu import _run, host_bins  # noqa: F401  (the fixture builds the binaries)

pytestmark = pytest.mark.gpu

CUT = 1e-5 * (1 + 1e-9)             # a number printed cut to 5 places is less than 1e-5 below its value
FPS = 200


def _near(g, w):
    return all(abs(a - b) <= CUT for a, b in zip(g, w))


def _check_token(g, t, w, tag):
    assert g["tick"] == t + 1 and g["usec"] == (t + 1) * (1000000 // FPS), (tag, g)          # the frame's Sample
    assert (g["unit"], g["pos_ok"], g["vel_ok"], g["head_ok"], g["reg_ok"]) == (1, w["position_valid"], w["velocity_valid"], False, False), (tag, g, w)
    if w["position_valid"]:
        assert _near(g["pos_xy"], (w["x"], w["y"])) and _near(g["vel_xy"], (w["vx"], w["vy"])), (tag, g, w)


def test_posidet_diff_bgr_track_sinks(host_bins, tmp_path):  # noqa: F811
    import uuid
    rows, cols, channels, k = 48, 64, 3, TC.IMG_K
    frames = TC.sequence("motion", rows, cols, channels, 0)
    h = P.HOMOGRAPHIES["affine"]
    dets = [TC.triples(r) for r, _ in TC.image_targets("motion", rows, cols, channels, 0, 0.0, k)]
    want, _ = TR.run(dets, k, kalman=TC.IMG_KALMAN, gate=TC.IMG_GATE, homography=h)
    assert len({r["id"] for rs in want for r in rs}) >= 4 and any(not r["position_valid"] for rs in want for r in rs)
    kal = O.Kalman(**TC.IMG_KALMAN)                   # the SINK: the trackers' own chain on the ordinary result (rank 0)
    sink = [R.chain(dict(position_valid=d[0][0], x=d[0][1], y=d[0][2], heading_valid=False, hx=0.0, hy=0.0), kalman=kal, homography=h)
            for d in dets]
    tag = "oat_t_" + uuid.uuid4().hex[:8]
    src, snk, tsinks = tag + "raw", tag + "pos", [tag + f"k{i}" for i in range(k)]
    kp = TC.IMG_KALMAN
    argv = ["oat-posidet-hip", "diff", src, snk, "--bgr", "-d", str(TC.DIFF["diff_threshold"]), "-b", str(TC.DIFF["blur"]),
            "-a", "[%d,%d]" % TC.DC.AREA, "--track-sinks", ",".join(tsinks), "--track-gate", repr(TC.IMG_GATE), "--kalman",
            "--dt", repr(kp["dt"]), "--timeout", repr(kp["timeout"]), "--sigma-accel", repr(kp["sigma_accel"]),
            "--sigma-noise", repr(kp["sigma_noise"]), "--homography", "[" + ",".join(repr(float(v)) for v in h) + "]"]
    got = _run(host_bins, tmp_path, argv, [src], [frames], "BGR", [snk] + tsinks, fps=FPS)
    for a in [snk] + tsinks:
        assert len(got[a]) == len(frames), (a, len(got[a]))             # one token a frame on every sink: consumers stay in step
    for t in range(len(frames)):
        _check_token(got[snk][t], t, sink[t], ("sink", t))
        for i in range(k):
            _check_token(got[tsinks[i]][t], t, want[t][i], (i, t))
