"""GPU tests of `--target-shape` of the host binaries (target shapes): oat-frameserve-raw -> oat-posidet-hip thresh
--target-sinks a,b,c,d --target-shape -> five oat-posi-cout, and the same through oat-track-hip with two cameras, --ring 2 and the
options in a -c table.  The heading of every token on every target sink is the model's body axis (tests/shapes_ref.py) as
oat-posi-cout prints it; the SINK carries what it carries without the option; and without --target-shape every token is what it
was (no heading anywhere)."""
import os
import subprocess
import uuid

import numpy as np
import pytest

import oracle_lib as O
import shapes_cases as S
import shapes_ref as R
import targets_cases as T
import test_targets_host_gpu as TH

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin")


@pytest.fixture(scope="module")
def host_bins():
    if not all(os.path.exists(os.path.join(BIN, b)) for b in ("oat-posidet-hip", "oat-track-hip", "oat-posi-cout", "oat-frameserve-raw")):
        subprocess.check_call(["make", "-s", "-j4", "-C", ROOT, "host"])
    return BIN


def _check_token(g, t, rank, shape, tag, fps=200):
    """a target sink's token: the rank's position and, where the blob has one, its axis as the heading"""
    assert g["tick"] == t + 1 and g["usec"] == (t + 1) * (1000000 // fps), (tag, g)
    assert g["pos_ok"] == rank["valid"], (tag, g, rank)
    if rank["valid"]:
        assert g["pos_xy"] == [TH._printed(rank["x"]), TH._printed(rank["y"])], (tag, g, rank)
    else:
        assert "pos_xy" not in g, (tag, g)
    assert g["head_ok"] == (shape["valid"] and shape["axis_valid"]), (tag, g, shape)
    if g["head_ok"]:
        assert g["head_xy"] == [TH._printed(shape["axis_x"]), TH._printed(shape["axis_y"])], (tag, g, shape)
    else:
        assert "head_xy" not in g, (tag, g)
    assert g["vel_ok"] is False and g["reg_ok"] is False, (tag, g)


def test_posidet_thresh_target_shape(host_bins, tmp_path):
    cases = {c.name: c for c in S.all_planted()}
    names = ["hole-48x64", "groups-48x64", "ties-48x64", None, "ring-48x64", "groups-48x64"]
    imgs = [cases[n].img if n else np.zeros((48, 64), np.uint8) for n in names]
    area, k = (0.5, T.BIG), 4
    p = O.hsv_params(h_lo=255, h_hi=256, erode=0, dilate=0, min_area=area[0], max_area=area[1])
    masks = [O.detect_thresh(im, p)[1] for im in imgs]
    ranks = [T.reference(m, area, k)[0] for m in masks]
    shapes = [R.reference(m, area, k) for m in masks]
    assert any(s["valid"] and not s["axis_valid"] for ss in shapes for s in ss), "no blob without an axis"
    assert sum(s["axis_valid"] for ss in shapes for s in ss) >= 10
    seen = {}
    for flag in (True, False):
        tag = "oat_s_" + uuid.uuid4().hex[:8]
        src, snk, tsinks = tag + "raw", tag + "pos", [tag + f"t{j}" for j in range(k)]
        argv = ["oat-posidet-hip", "thresh", src, snk, "-T", "[255,256]", "-e", "0", "-d", "0", "-a", "[0.5,1000000]", "--target-sinks",
                ",".join(tsinks)] + (["--target-shape"] if flag else [])
        got = TH._run(host_bins, tmp_path, argv, [src], [imgs], "GREY", [snk] + tsinks)
        for a in [snk] + tsinks:
            assert len(got[a]) == len(imgs), (a, len(got[a]))
        for t in range(len(imgs)):
            TH._check_token(got[snk][t], t, ranks[t][0], ("sink", flag, t))          # SINK unchanged: no heading
            for j in range(k):
                if flag:
                    _check_token(got[tsinks[j]][t], t, ranks[t][j], shapes[t][j], (j, t))
                else:
                    TH._check_token(got[tsinks[j]][t], t, ranks[t][j], (j, t))       # without the flag: today's tokens
        seen[flag] = [got[snk]] + [got[a] for a in tsinks]
    # ... and the flag changes nothing but the heading
    strip = lambda g: {key: v for key, v in g.items() if key not in ("head_ok", "head_xy")}      # noqa: E731
    assert [[strip(g) for g in sink] for sink in seen[True]] == [[strip(g) for g in sink] for sink in seen[False]]
    assert seen[True][0] == seen[False][0]


def test_track_target_shape_two_cameras_ring_2_from_a_config_table(host_bins, tmp_path):
    rows, cols, ncam, k = 48, 64, 2, S.TRACKER_K
    frames = [S.sequence("fused", rows, cols, s) for s in range(ncam)]
    ranks = [S.sequence_targets("fused", rows, cols, s, 0.0, k) for s in range(ncam)]
    shapes = [S.sequence_reference("fused", rows, cols, s, 0.0, k) for s in range(ncam)]
    tag = "oat_s_" + uuid.uuid4().hex[:8]
    srcs = [f"{tag}raw{s}" for s in range(ncam)]
    snks = [f"{tag}pos{s}" for s in range(ncam)]
    tsinks = [[f"{tag}c{s}t{j}" for j in range(k)] for s in range(ncam)]
    cfg = tmp_path / "track.toml"
    cfg.write_text("[rig]\ntarget-shape = true\ntarget-sinks = [%s]\n" % ", ".join('"%s"' % ",".join(l) for l in tsinks))
    w = T.FUSED_WIN
    argv = ["oat-track-hip", ",".join(srcs), ",".join(snks), "-a", str(T.FUSED_LR), "--area", "[2,1000000]",
            "-H", "[%d,%d]" % w["h_thresh"], "-S", "[%d,%d]" % w["s_thresh"], "-V", "[%d,%d]" % w["v_thresh"],
            "-e", str(T.FUSED_MORPH[0]), "-d", str(T.FUSED_MORPH[1]), "--ring", "2", "-c", str(cfg), "rig"]
    readers = snks + [a for l in tsinks for a in l]
    got = TH._run(host_bins, tmp_path, argv, srcs, frames, "BGR", readers)
    n = len(frames[0])
    assert sum(s["axis_valid"] for ss in shapes[0] for s in ss) >= 2 * (n - S.WARM["fused"])
    for s in range(ncam):
        for a in [snks[s]] + tsinks[s]:
            assert len(got[a]) == n, (a, len(got[a]))
        for t in range(n):
            TH._check_token(got[snks[s]][t], t, ranks[s][t][0][0], ("sink", s, t))
            for j in range(k):
                _check_token(got[tsinks[s][j]][t], t, ranks[s][t][0][j], shapes[s][t][j], (s, j, t))
