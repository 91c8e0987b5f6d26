"""GPU tests of `--target-sinks` of the host binaries (multi-target detection): oat-frameserve-raw ->
oat-posidet-hip thresh --target-sinks a,b,c -> three oat-posi-cout, and the same through oat-track-hip with two cameras and
--ring 2.  Every token of every sink is compared with the reference ranking of tests/targets_cases.py: the frame's Sample, the
valid flag, and the position as oat-posi-cout prints it (serializePosition truncates to 5 decimal places)."""
import json
import os
import subprocess
import time
import uuid

import numpy as np
import pytest

import targets_cases as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin")


@pytest.fixture(scope="module")
def host_bins():
    if not all(os.path.exists(os.path.join(BIN, b)) for b in ("oat-posidet-hip", "oat-track-hip", "oat-posi-cout", "oat-frameserve-raw")):
        subprocess.check_call(["make", "-s", "-j4", "-C", ROOT, "host"])
    return BIN


def _printed(v):
    """jsonNumber of host/datatypes.hpp: nine places, cut to five"""
    s = "%.9f" % v
    return float(s[:s.index(".") + 6])


def _check_token(g, t, want, tag, fps=200):
    assert g["tick"] == t + 1 and g["usec"] == (t + 1) * (1000000 // fps), (tag, g)          # the frame's Sample
    assert g["pos_ok"] == want["valid"], (tag, g, want)
    if want["valid"]:
        assert g["pos_xy"] == [_printed(want["x"]), _printed(want["y"])], (tag, g, want)
    else:
        assert "pos_xy" not in g, (tag, g)
    assert g["vel_ok"] is False and g["head_ok"] is False and g["reg_ok"] is False, (tag, g)


def _consumers_ready(*addresses, timeout=30.0, settle=1.0):
    t_end = time.monotonic() + timeout
    while time.monotonic() < t_end and not all(os.path.exists(f"/dev/shm/{a}_node") for a in addresses):
        time.sleep(0.05)
    time.sleep(settle)


def _run(host_bins, tmp_path, component, sources, frames, color, reader_addresses, fps=200):
    """component: the argv of the one GPU process; sources[s] is fed frames[s]; -> {address: tokens}"""
    B = lambda b: os.path.join(host_bins, b)      # noqa: E731
    rows, cols = frames[0][0].shape[:2]
    files = {a: open(tmp_path / f"{a}.out", "w+") for a in reader_addresses}
    readers = [subprocess.Popen([B("oat-posi-cout"), a], stdout=files[a], stderr=subprocess.DEVNULL, text=True) for a in reader_addresses]
    proc = subprocess.Popen([B(component[0])] + component[1:])
    _consumers_ready(*sources, *reader_addresses)
    feeders = []
    for s, a in enumerate(sources):
        raw = tmp_path / f"frames{s}.raw"
        np.stack(frames[s]).tofile(raw)
        feeders.append(subprocess.Popen([B("oat-frameserve-raw"), a, "-f", str(raw), "--rows", str(rows), "--cols", str(cols), "-C", color,
                                         "-n", str(len(frames[s])), "-r", str(fps)]))
    out = {}
    try:
        for r, a in zip(readers, reader_addresses):
            r.wait(timeout=120)
            files[a].seek(0)
            out[a] = [json.loads(l) for l in files[a].read().splitlines() if l.strip()]
        for f in feeders:
            f.wait(timeout=60)
        proc.wait(timeout=60)
    finally:
        for p in readers + feeders + [proc]:
            if p.poll() is None:
                p.kill()
        subprocess.run([B("oat-clean-hip")] + list(sources) + list(reader_addresses), capture_output=True)
    assert proc.returncode == 0
    return out


def test_posidet_thresh_target_sinks(host_bins, tmp_path):
    cases = {c.name: c for c in T.planted_cases()}
    names = ["ties-48x64", "ring-48x64", "window-48x64", None, "ties-48x64", "ring-48x64"]
    imgs = [cases[n].img if n else np.zeros((48, 64), np.uint8) for n in names]
    area, k = (0.5, T.BIG), 3
    import oracle_lib as O
    p = O.hsv_params(h_lo=255, h_hi=256, erode=0, dilate=0, min_area=area[0], max_area=area[1])
    refs = [T.reference(O.detect_thresh(im, p)[1], area, k) for im in imgs]
    assert [r[1] for r in refs] == [10, 3, 6, 0, 10, 3]
    tag = "oat_t_" + uuid.uuid4().hex[:8]
    src, snk, tsinks = tag + "raw", tag + "pos", [tag + f"t{j}" for j in range(k)]
    got = _run(host_bins, tmp_path,
               ["oat-posidet-hip", "thresh", src, snk, "-T", "[255,256]", "-e", "0", "-d", "0", "-a", "[0.5,1000000]", "--target-sinks",
                ",".join(tsinks)], [src], [imgs], "GREY", [snk] + tsinks)
    for a in [snk] + tsinks:
        assert len(got[a]) == len(imgs), (a, len(got[a]))               # one token a frame on every sink: consumers stay in step
    for t, (ranks, _) in enumerate(refs):
        _check_token(got[snk][t], t, ranks[0], ("sink", t))             # the SINK carries what it carries without the option
        for j in range(k):
            _check_token(got[tsinks[j]][t], t, ranks[j], (j, t))


def test_track_target_sinks_two_cameras_ring_2(host_bins, tmp_path):
    rows, cols, ncam, k = 48, 64, 2, T.TRACKER_K
    frames = [T.sequence("fused", rows, cols, s) for s in range(ncam)]
    refs = [T.sequence_reference("fused", rows, cols, s, 0.0, k) for s in range(ncam)]
    tag = "oat_t_" + uuid.uuid4().hex[:8]
    srcs = [f"{tag}raw{s}" for s in range(ncam)]
    snks = [f"{tag}pos{s}" for s in range(ncam)]
    tsinks = [[f"{tag}c{s}t{j}" for j in range(k)] for s in range(ncam)]
    w = T.FUSED_WIN
    argv = ["oat-track-hip", ",".join(srcs), ",".join(snks), "-a", str(T.FUSED_LR), "--area", "[2,1000000]",
            "-H", "[%d,%d]" % w["h_thresh"], "-S", "[%d,%d]" % w["s_thresh"], "-V", "[%d,%d]" % w["v_thresh"],
            "-e", str(T.FUSED_MORPH[0]), "-d", str(T.FUSED_MORPH[1]), "--ring", "2"]
    for s in range(ncam):
        argv += ["--target-sinks", ",".join(tsinks[s])]
    readers = snks + [a for l in tsinks for a in l]
    got = _run(host_bins, tmp_path, argv, srcs, frames, "BGR", readers)
    n = len(frames[0])
    assert any(r[1] > k for r in refs[0]) and any(r[1] < k for r in refs[0])
    for s in range(ncam):
        for a in [snks[s]] + tsinks[s]:
            assert len(got[a]) == n, (a, len(got[a]))
        for t, (ranks, _) in enumerate(refs[s]):
            _check_token(got[snks[s]][t], t, ranks[0], ("sink", s, t))
            for j in range(k):
                _check_token(got[tsinks[s][j]][t], t, ranks[j], (s, j, t))
