"""GPU tests of marker sets on the pipelined path (oatgpu_set_marker_pipeline, oatgpu_track_collect_markers,
oatgpu_track_markers_sequence_dev; HotPath.marker_pipeline / .collect_markers / .track_markers_sequence_dev): the marker work
as a citizen of the result ring, two frames a launch, one back half for all markers.

Expected values are those of tests/test_markers_gpu.py: the oracle chain run once per marker (markers_ref.MarkerOracle),
markers_ref.combine for the combined record -- never the library's own synchronous step.  Comparisons are exact as there:
valid, first_pixel and the contour sums as integers, x / y within 1e-4 px, the combined x / y / hx / hy bit for bit, masks
byte for byte, the model bit for bit against a plain context fed the same frames."""
import json
import os
import subprocess
import uuid

import numpy as np
import pytest

import blob_load as B
import markers_ref as MR
import oracle_lib as O
from test_markers_gpu import (BIN, BLUE, GREEN, LR, MORPH, RED, ROOT, _Rig, _hp, _mk_arg, _same_combined, _same_detection,
                              _streams)

pytestmark = pytest.mark.gpu

THREE = [BLUE, RED, GREEN]
_CACHE = {}


def _expected(key, rows, cols, n, markers, frames, ch=3, threads=1):
    """The oracle's answer for a frame sequence, once per distinct input: [t] -> (want[s][m], planes[s][m], fg[s])."""
    if key not in _CACHE:
        rig = _Rig(rows, cols, n, markers, ch=ch, threads=threads)
        _CACHE[key] = [rig.step(fs) for fs in frames]
    return _CACHE[key]


def _compare(got, exp, anchor, tag):
    fg, markers, mean = got
    want, _, want_fg = exp
    for s in range(len(fg)):
        _same_detection(fg[s], want_fg[s], (tag, s, "fg"))
        for m in range(len(want[s])):
            _same_detection(markers[s][m], want[s][m], (tag, s, m))
        _same_combined(mean[s], markers[s], anchor, (tag, s))


def _cap(exps, gots, n, M):
    """The cap against vacuous passes: the oracle alone finds every marker on >= 90 % of the compared frames (the first has
    no discs) of each stream, and a unit heading comes out exactly where all markers were found."""
    valid = np.zeros((n, M), int)
    all_valid = np.zeros(n, int)
    headings = 0
    for t in range(1, len(exps)):
        want = exps[t][0]
        for s in range(n):
            valid[s] += [int(want[s][m]["valid"]) for m in range(M)]
            all_valid[s] += int(all(want[s][m]["valid"] for m in range(M)))
        headings += sum(int(c.heading_valid and abs(c.hx * c.hx + c.hy * c.hy - 1.0) < 1e-9) for c in gots[t][2])
    steps = len(exps) - 1
    print("oracle: frames with the marker valid, per stream and marker:", valid.tolist(), "all:", all_valid.tolist(), "of", steps)
    assert (valid >= 0.9 * steps).all(), valid
    assert headings == all_valid.sum() > 0, (headings, all_valid)


def _pinned(frames):
    import torch
    return [[torch.from_numpy(f).pin_memory().numpy() for f in fs] for fs in frames]


def _run_ring(hp, frames, form, depth):
    """Every frame set through the given enqueue form, results collected as late as the ring allows -> [t] results."""
    import torch
    gots, keep = [], []
    if form == "stage_kernel":
        hp.set_stage_copy(1)
        frames = _pinned(frames)
    for fs in frames:
        if hp.outstanding() == depth:
            gots.append(hp.collect_markers())
        if form.startswith("dev"):
            dev = torch.from_numpy(np.stack(fs)).cuda()
            torch.cuda.synchronize()
            keep.append(dev)
            hp.enqueue_dev(dev.data_ptr(), keepalive=dev)
        elif form == "host":
            hp.enqueue(fs)
        else:
            for s in reversed(range(len(fs))):
                hp.stage(s, fs[s])
            hp.enqueue_staged()
    while hp.outstanding():
        gots.append(hp.collect_markers())
    return gots


# ------------------------------------------------------------------------- 1: the ring, host and device frames ---

@pytest.mark.parametrize("seed", [0, 100])
@pytest.mark.parametrize("depth", [2, 3, 4])
@pytest.mark.parametrize("form", ["dev", "dev_fuse2", "host", "stage_dma", "stage_kernel"])
def test_ring_host_and_device_frames(form, depth, seed):
    rows, cols, n, T = 270, 480, 3, 41
    frames = _streams(rows, cols, n, T, seed=seed)
    exps = _expected(("ring", seed), rows, cols, n, THREE, frames)
    hp = _hp(rows, cols, n, ring_depth=depth)
    try:
        hp.set_markers(THREE, heading_anchor=0)
        hp.marker_pipeline(True)
        if form == "dev_fuse2":
            hp.set_fusion(2)
        gots = _run_ring(hp, frames, form, depth)
        assert len(gots) == T
        for t in range(T):
            _compare(gots[t], exps[t], 0, (form, depth, seed, t))
    finally:
        hp.close()
    _cap(exps, gots, n, 3)


# --------------------------------------------- 2: the sequence call at the sizes where the launch order changes ---

@pytest.mark.parametrize("n,rows,cols,T,seed", [(2, 1080, 1920, 25, 20), (1, 2160, 3840, 13, 40), (1, 480, 640, 41, 7)])
def test_sequence_call_where_the_launch_order_changes(n, rows, cols, T, seed):
    import torch
    frames = _streams(rows, cols, n, T, seed=seed)
    exps = _expected(("seq", rows, seed), rows, cols, n, THREE, frames, threads=4 if rows > 500 else 1)
    dev = [torch.from_numpy(np.stack(fs)).cuda() for fs in frames]
    torch.cuda.synchronize()
    records = {}
    for fusion in (1, 2):
        hp = _hp(rows, cols, n)
        try:
            hp.set_markers(THREE, heading_anchor=0)
            hp.marker_pipeline(True)
            hp.set_fusion(fusion)
            gots = hp.track_markers_sequence_dev([d.data_ptr() for d in dev])
            print("last step shape (K1 workgroup, early blob):", (rows, cols, n), "fusion", fusion, hp.last_step_shape())
            assert not hp.last_step_shape()[1]              # marker steps never take the early order
            assert len(gots) == T
            for t in range(T):
                _compare(gots[t], exps[t], 0, (rows, fusion, t))
            records[fusion] = [[tuple(vars(p).values()) for p in fg] + [tuple(vars(p).values()) for cam in mk for p in cam] +
                               [repr(tuple(vars(c).values())) for c in mean] for fg, mk, mean in gots]
        finally:
            hp.close()
    assert records[1] == records[2]
    _cap(exps, gots, n, 3)


# ------------------------------------------------------------------ 3: per-marker parameters through the table ---

def _params_case(name):
    if name == "morph":
        return 3, [dict(BLUE, erode=0, dilate=10, area=(0.0, 1e7)), dict(RED, erode=3, dilate=7), dict(GREEN, erode=5, dilate=0),
                   dict(BLUE, erode=4, dilate=6),                                             # even sizes
                   dict(BLUE, area=(1e5, 1e6)),                                               # an area window that excludes the disc
                   dict(h=(0, 256), s=(0, 256), v=(0, 50), erode=0, dilate=0, area=(1000.0, 1e9)),   # holds (0,0,0)
                   dict(h=(30, 20), s=(0, 256), v=(0, 256), erode=0, dilate=0)]               # lo > hi: the empty window
    if name == "one":
        return 3, [BLUE]
    if name == "eight":
        return 3, [BLUE, RED, GREEN, dict(BLUE, erode=0, dilate=3), dict(RED, erode=2, dilate=0), dict(GREEN, erode=7, dilate=9),
                   dict(RED, erode=0, dilate=0, area=(5.0, 1e6)), dict(BLUE, erode=6, dilate=2)]
    return 1, [dict(h=(55, 80), **MORPH), dict(h=(105, 125), erode=0, dilate=5, area=(20.0, 1e6))]     # grey: discs 0 and 1


@pytest.mark.parametrize("name", ["morph", "one", "eight", "grey"])
def test_per_marker_parameters_through_the_table(name):
    import torch
    ch, markers = _params_case(name)
    rows, cols, n, T = 270, 480, 2, 15
    M = len(markers)
    anchor = None if name == "morph" else 0
    frames = _streams(rows, cols, n, T, ch=ch, seed=2)
    rig = _Rig(rows, cols, n, markers, ch=ch)
    if name == "morph":                                       # per-camera colour windows: camera 1's marker 1 looks for green
        rig.cams[1].set_window(1, dict(GREEN, erode=3, dilate=7))
    hp = _hp(rows, cols, n, ch=ch, ring_depth=3)
    try:
        hp.set_markers(markers, heading_anchor=anchor)
        if name == "morph":
            hp.set_marker_window(1, 1, h=GREEN["h"], s=GREEN["s"], v=GREEN["v"])
        hp.marker_pipeline(True)
        dev = [torch.from_numpy(np.stack(fs)).cuda() for fs in frames]
        torch.cuda.synchronize()
        gots = hp.track_markers_sequence_dev([d.data_ptr() for d in dev])
        found = np.zeros(M, int)
        for t in range(T):
            want, _ = rig.check(gots[t], frames[t], anchor, (name, t), count=t > 0)
            found += [int(all(want[s][m]["valid"] for s in range(n))) for m in range(M)]
            if name == "morph":
                for s in range(n):
                    assert not want[s][4]["valid"] and not want[s][6]["valid"]
                    if t > 0:
                        assert want[s][5]["valid"] and want[s][5]["area"] > 0.5 * rows * cols
        print("frames on which every camera found the marker:", found.tolist(), "of", T)
        # (against a vacuous pass: the plain disc markers are found; heavy erosions may legitimately lose theirs)
        live = [m for m, mk in enumerate(markers) if mk.get("erode", 0) <= 3 and not (name == "morph" and m in (4, 6))]
        assert len(live) >= min(M, 2) and all(found[m] >= (T - 1) // 2 for m in live), found
    finally:
        hp.close()


# ------------------------------------------------------------------------------------------- 4: taps and model ---

def test_taps_after_a_collect_and_the_model():
    from oat_amd import ffi
    import oat_amd
    rows, cols, n, T = 270, 480, 2, 12
    frames = _streams(rows, cols, n, T, seed=4)
    markers = [BLUE, dict(RED, erode=0, dilate=5), dict(GREEN, erode=2, dilate=0)]
    filt = [O.Mog2(rows, cols, 3) for _ in range(n)]
    rig = _Rig(rows, cols, n, markers)
    hp = _hp(rows, cols, n, ring_depth=3)
    plain = oat_amd.HotPath(rows, cols, n_streams=n, adaptation_coeff=LR, erode=3, dilate=7, area=(20.0, 1e6),
                            h_thresh=(100, 125), s_thresh=(150, 256), v_thresh=(100, 256))
    try:
        hp.set_markers(markers, heading_anchor=2)
        hp.marker_pipeline(True)

        def check_taps(t, fs, planes, z_too):
            for s in range(n):
                masked, _ = filt[s].filter(fs[s], LR)
                if z_too:                                 # (the Z tap is the latest LAUNCHED frame's: compared when that is this one)
                    assert (hp.read_mask(ffi.TAP_THRESHOLD, s) == np.where(masked.max(-1) != 0, 255, 0)).all(), (t, s)
                hsv = O.bgr2hsv(masked)
                for m, mk in enumerate(markers):
                    thr = O.inrange3(hsv, (mk["h"][0], mk["s"][0], mk["v"][0]), (mk["h"][1], mk["s"][1], mk["v"][1]))
                    assert (hp.read_marker_mask(m, ffi.TAP_THRESHOLD, s) == thr).all(), (t, s, m)
                    mor = planes[s][m]
                    assert (hp.read_marker_mask(m, ffi.TAP_MORPH, s) == mor).all(), (t, s, m)
                    assert (hp.read_marker_mask(m, ffi.TAP_FINAL, s) == B.frame_zeroed(mor) * 255).all(), (t, s, m)

        # two frame sets in flight, the older one collected: the taps are ITS planes, not the newer set's
        for t in range(0, T, 2):
            hp.enqueue(frames[t])
            hp.enqueue(frames[t + 1])
            for k in (t, t + 1):
                plain.track(frames[k])
                got = hp.collect_markers()
                _, planes = rig.check(got, frames[k], 2, ("taps", k))
                check_taps(k, frames[k], planes, z_too=k == t + 1)
        for s in range(n):
            for a, b in zip(hp.mog_state(s), plain.mog_state(s)):
                assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), s
    finally:
        hp.close()
        plain.close()


# --------------------------------------------------------------------------------------------- 5: a busy frame ---

@pytest.mark.parametrize("which", ["one", "all"])
def test_busy_frame_in_the_middle_of_a_pipelined_run(which):
    rows, cols, n, T = 270, 480, 1, 14
    rng = np.random.default_rng(11)
    frames = _streams(rows, cols, n, T, n_discs=2, seed=3)
    open_ = dict(erode=0, dilate=0, area=(0.0, 1e9))
    markers = [dict(BLUE, **open_), RED] if which == "one" else [dict(BLUE, **open_), dict(RED, **open_)]
    from oat_amd.synth import DISC_BGR
    busy = (6, 7, 9)
    for t in busy:                                            # 50 % noise in the open markers' windows
        f = frames[t][0].copy()
        hit = rng.random((rows, cols)) < 0.5
        if which == "one":
            f[hit] = DISC_BGR[0]
        else:
            f[hit] = np.where(rng.random((int(hit.sum()), 1)) < 0.5, DISC_BGR[0], DISC_BGR[1])
        frames[t] = [f]
    rig = _Rig(rows, cols, n, markers)
    hp = _hp(rows, cols, n, ring_depth=4)
    try:
        hp.set_markers(markers, heading_anchor=1)
        hp.marker_pipeline(True)
        gots = _run_ring(hp, frames, "host", 4)
        paths = []
        for t in range(T):
            _, planes = rig.check(gots[t], frames[t], 1, ("busy", which, t))
            paths.append([B.blob_load(planes[0][m])["path"] for m in range(2)])
        print("paths:", paths)
        for t in range(T):
            if t not in busy:
                assert paths[t] == ["lds", "lds"], (t, paths[t])
            else:                                             # (one: marker 1's plane on a busy frame is whatever the noise left of its disc)
                assert paths[t][0] == "global" and (which == "one" or paths[t][1] == "global"), (t, paths[t])
    finally:
        hp.close()


# ------------------------------------------------------- 6: undistort + ROI, device buffers refilled at once ---

def test_undistort_roi_and_buffers_refilled_after_input_consumed():
    """Two device buffers reused in turn; each is refilled -- with a frame whose discs sit elsewhere -- the moment
    input_consumed returns.  The marker kernel reads the frames after the per-pixel kernel has: input_consumed covers it."""
    import torch
    import undistort_ref as R
    rows, cols, n, T = 480, 640, 2, 16
    cals = [R.cases(rows, cols)[k] for k in ("barrel", "mild5")]
    maps = [R.undistort_map(rows, cols, K, D) for K, D in cals]
    yy, xx = np.mgrid[0:rows, 0:cols]
    roi = (((xx - 330) ** 2 + (yy - 230) ** 2) < 200 ** 2).astype(np.uint8) * 255
    frames = _streams(rows, cols, n, T, seed=13)
    decoys = _streams(rows, cols, n, T + 40, seed=13)[40:]                 # the same cameras much later: discs elsewhere
    for fusion in (1, 2):
        hp = _hp(rows, cols, n, undistort=cals, ring_depth=4)
        rig = _Rig(rows, cols, n, THREE)
        try:
            hp.set_roi_mask(roi, stream=0)
            hp.set_markers(THREE, heading_anchor=0)
            hp.marker_pipeline(True)
            hp.set_fusion(fusion)
            bufs = [torch.empty((n, rows, cols, 3), dtype=torch.uint8, device="cuda") for _ in range(2)]
            gots = []
            for t, fs in enumerate(frames):
                if hp.outstanding() == 4:
                    gots.append(hp.collect_markers())
                buf = bufs[t & 1]
                buf.copy_(torch.from_numpy(np.stack(fs)))
                torch.cuda.synchronize()
                hp.enqueue_dev(buf.data_ptr(), keepalive=buf)
                if t & 1:                                     # both buffers are in the library's hands: get them back, refill both
                    hp.input_consumed()
                    for k in (0, 1):
                        bufs[k].copy_(torch.from_numpy(np.stack(decoys[t - k])))
                    torch.cuda.synchronize()
            while hp.outstanding():
                gots.append(hp.collect_markers())
            for t, fs in enumerate(frames):
                seen = [R.remap(fs[s], *maps[s]) for s in range(n)]
                seen[0] = seen[0].copy()
                seen[0][roi == 0] = 0
                rig.check(gots[t], seen, 0, ("roi+ud", fusion, t), count=t > 0)
            assert rig.valid.sum() >= rig.steps * n, rig.valid
        finally:
            hp.close()


# ------------------------------------------------------------------------------- 7: interleaving and refusals ---

def test_interleaving_and_refusals():
    from oat_amd import ffi
    rows, cols, n = 270, 480, 2
    frames = _streams(rows, cols, n, 30, seed=6)
    rig = _Rig(rows, cols, n, [BLUE, RED])
    plain_ctx = _hp(rows, cols, n)
    it = iter(frames)
    hp = _hp(rows, cols, n, ring_depth=3)

    def step(how):
        """one frame set through `how`; every way must still match the oracle, and the plain context sees the same frames"""
        fs = next(it)
        plain_ctx.track(fs)
        want, _, want_fg = rig.step(fs)
        if how == "plain":
            got = hp.track(fs)
            for s in range(n):
                _same_detection(got[s], want_fg[s], ("plain", s))
            return
        if how == "sync":
            got = hp.track_markers(fs)
        elif how == "plain_collect":                      # plain collect on a switched-on context: fg only, the slot retired
            hp.enqueue(fs)
            fg = hp.collect()
            assert hp.outstanding() == 0
            for s in range(n):
                _same_detection(fg[s], want_fg[s], ("plain_collect", s))
            return
        else:
            hp.enqueue(fs)
            got = hp.collect_markers()
        for s in range(n):
            _same_detection(got[0][s], want_fg[s], (how, s, "fg"))
            for m in range(2):
                _same_detection(got[1][s][m], want[s][m], (how, s, m))
            _same_combined(got[2][s], got[1][s], 0, (how, s))

    def refused(fn, word):
        with pytest.raises(ffi.OatGpuError) as e:
            fn()
        assert word in str(e.value), str(e.value)

    try:
        step("plain")
        refused(lambda: hp.marker_pipeline(True), "not configured")
        refused(lambda: hp.collect_markers(), "marker pipeline is off")
        step("plain")
        hp.set_markers([BLUE, RED], heading_anchor=0)
        fs = next(it)
        plain_ctx.track(fs)
        want_fg = rig.step(fs)[2]
        hp.enqueue(fs)                                                               # results outstanding
        refused(lambda: hp.marker_pipeline(True), "outstanding")
        got = hp.collect()
        for s in range(n):
            _same_detection(got[s], want_fg[s], ("ring", s))
        hp.set_kalman(True, dt=0.02, timeout=1.0)
        refused(lambda: hp.marker_pipeline(True), "oatgpu_set_kalman")
        hp.set_kalman(False)
        step("plain")
        hp.set_homography([1, 0, 0, 0, 1, 0, 0, 0, 1])
        refused(lambda: hp.marker_pipeline(True), "homography")
        hp.set_homography(None)
        step("sync")
        hp._chk(hp.lib.oatgpu_set_detector(hp.ctx, 100, 125, 150, 256, 100, 256, 3, 7, 20.0, 1e6))    # the wrong own window
        refused(lambda: hp.marker_pipeline(True), "non-zero window")
        hp._chk(hp.lib.oatgpu_set_detector(hp.ctx, 0, 256, 0, 256, 1, 256, 3, 7, 20.0, 1e6))
        step("plain")
        hp.marker_pipeline(True)
        refused(lambda: hp.collect_markers(), "nothing outstanding")
        step("pipe")
        step("pipe")
        # what would pull the path's memory or its premises from under it is refused while the switch is on
        refused(lambda: hp.set_markers([BLUE]), "marker pipeline is on")
        refused(lambda: hp.set_markers([]), "marker pipeline is on")
        refused(lambda: hp.set_kalman(True), "marker pipeline is on")
        refused(lambda: hp.set_homography([1, 0, 0, 0, 1, 0, 0, 0, 1]), "marker pipeline is on")
        refused(lambda: hp._chk(hp.lib.oatgpu_set_detector(hp.ctx, 100, 125, 150, 256, 100, 256, 3, 7, 20.0, 1e6)), "marker pipeline is on")
        step("pipe")
        step("plain")                                       # track() on a switched-on context: enqueue + collect, fg only
        step("plain_collect")
        step("sync")                                        # the synchronous step between drained pipelined runs
        step("pipe")
        fs = next(it)
        hp.enqueue(fs)
        refused(lambda: hp.track_markers(fs), "outstanding")
        refused(lambda: hp.marker_pipeline(False), "outstanding")
        plain_ctx.track(fs)
        want = rig.step(fs)
        _compare(hp.collect_markers(), want, 0, "after refusals")
        # switch off again: an ordinary context (the checks of test_markers_off_again_is_an_ordinary_context)
        hp.marker_pipeline(False)
        refused(lambda: hp.collect_markers(), "marker pipeline is off")
        step("sync")
        hp.set_markers([])
        for _ in range(4):
            fs = next(it)
            rig.step(fs)
            got, want = hp.track(fs), plain_ctx.track(fs)
            assert [tuple(vars(p).values()) for p in got] == [tuple(vars(p).values()) for p in want]
        for s in range(n):
            for x, y in zip(hp.mog_state(s), plain_ctx.mog_state(s)):
                assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True), s
            assert (hp.read_mask(ffi.TAP_FINAL, s) == plain_ctx.read_mask(ffi.TAP_FINAL, s)).all()
    finally:
        hp.close()
        plain_ctx.close()


# ------------------------------------------------------------------------------------ 8: the process pipeline ---

@pytest.mark.parametrize("ncam,stop_mid_round", [(1, False), (2, False), (2, True)])
def test_process_pipeline_marker_ring(tmp_path, ncam, stop_mid_round):
    """oat-frameserve-raw -> oat-track-hip --marker x3 --heading-anchor 0 --marker-ring 3 -> 4 x oat-posi-cout per camera: every
    token against the oracle, in order, one out per frame in.  stop_mid_round: camera 1 delivers three frames fewer -- END
    arrives in the middle of a round, the owed results still leave and nothing is published for the dropped rounds."""
    from test_host_pipeline import _consumers_ready
    subprocess.check_call(["make", "-s", "-j4", "-C", ROOT, "host"])
    rows, cols, T = 270, 480, 20
    sets = _streams(rows, cols, ncam, T, seed=21)
    counts = [T - (3 if stop_mid_round and c == 1 else 0) for c in range(ncam)]
    tag = "oat_mr_" + uuid.uuid4().hex[:8]
    exe = lambda b: os.path.join(BIN, b)
    srcs = [f"{tag}src{c}" for c in range(ncam)]
    poss = [f"{tag}pos{c}" for c in range(ncam)]
    msinks = [[f"{tag}m{c}_{m}" for m in range(3)] for c in range(ncam)]
    for c in range(ncam):
        np.stack([fs[c] for fs in sets[:counts[c]]]).tofile(tmp_path / f"frames{c}.raw")
    addrs = [a for c in range(ncam) for a in msinks[c] + [poss[c]]]
    readers = [subprocess.Popen([exe("oat-posi-cout"), a], stdout=subprocess.PIPE, text=True) for a in addrs]
    args = [exe("oat-track-hip"), ",".join(srcs), ",".join(poss), "-a", str(LR), "-e", "3", "-d", "7", "--area", "[20,1000000]"]
    for m in THREE:
        args += ["--marker", _mk_arg(m)]
    for c in range(ncam):
        args += ["--marker-sinks", ",".join(msinks[c])]
    args += ["--heading-anchor", "0", "--marker-ring", "3"]
    track = subprocess.Popen(args)
    _consumers_ready(*srcs, *addrs)
    feeders = [subprocess.Popen([exe("oat-frameserve-raw"), srcs[c], "-f", str(tmp_path / f"frames{c}.raw"), "--rows", str(rows),
                                 "--cols", str(cols), "-n", str(counts[c]), "-r", "200"]) for c in range(ncam)]
    try:
        outs = [r.communicate(timeout=180)[0] for r in readers]
        track.wait(timeout=60)
        for c, f in enumerate(feeders):                       # (a camera that outlives the shorter one holds frames nobody will take)
            if counts[c] == min(counts):
                f.wait(timeout=60)
    finally:
        for p in readers + [track] + feeders:
            if p.poll() is None:
                p.kill()
        subprocess.run([exe("oat-clean-hip"), *srcs, *addrs], capture_output=True)
    assert track.returncode == 0
    recs = [[json.loads(l) for l in o.splitlines() if l.strip()] for o in outs]
    rounds = min(counts)
    print("tokens per sink:", [len(r) for r in recs], "rounds", rounds)
    assert [len(r) for r in recs] == [rounds] * len(addrs)
    headings = 0
    for c in range(ncam):
        rig = MR.MarkerOracle(rows, cols, 3, THREE)
        for t in range(rounds):
            want, _ = rig.step(sets[t][c], LR)
            for m in range(3):
                g = recs[c * 4 + m][t]
                assert g["tick"] == t + 1 and g["pos_ok"] == want[m]["valid"] and g["head_ok"] is False, (c, t, m, g)
                if want[m]["valid"]:
                    assert abs(g["pos_xy"][0] - want[m]["x"]) <= 1e-4 and abs(g["pos_xy"][1] - want[m]["y"]) <= 1e-4, (c, t, m, g)
            k = MR.combine([(w["valid"], w["x"] if w["valid"] else 0.0, w["y"] if w["valid"] else 0.0) for w in want], 0)
            g = recs[c * 4 + 3][t]
            assert (g["tick"], g["pos_ok"], g["head_ok"], g["vel_ok"]) == (t + 1, k["position_valid"], k["heading_valid"], False), (c, t, g, k)
            if k["position_valid"]:
                assert abs(g["pos_xy"][0] - k["x"]) <= 1e-4 and abs(g["pos_xy"][1] - k["y"]) <= 1e-4, (c, t, g, k)
            if k["heading_valid"]:
                assert abs(g["head_xy"][0] - k["hx"]) <= 1e-5 and abs(g["head_xy"][1] - k["hy"]) <= 1e-5, (c, t, g, k)
                headings += 1
    assert headings >= rounds * ncam // 2
