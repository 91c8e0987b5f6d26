"""GPU tests of the marker sets (oatgpu_set_markers, oatgpu_track_markers[_dev], HotPath.track_markers): several colour
windows per camera behind ONE MOG2 pass, and `posicom mean` behind them.

Expected values: marker m of a camera is the existing oracle chain (O.Mog2 + O.chain_step) run with marker m's parameters on
the same frames -- MOG2 does not depend on the detector -- and the combined record is MeanPosition::combine restated in
tests/markers_ref.py, computed from the library's own marker centroids.  All comparisons are exact: valid, first_pixel and
the contour sums as integers, x / y to the project's 1e-4 px bar, the combined x / y / hx / hy bit for bit."""
import os
import struct
import subprocess
import uuid
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import blob_load as B
import markers_ref as MR
import oracle_lib as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin")
LR = 0.01
NZ = dict(h_thresh=(0, 256), s_thresh=(0, 256), v_thresh=(1, 256))          # the non-zero window: the threshold plane is Z
NZ_P = dict(h_lo=0, h_hi=256, s_lo=0, s_hi=256, v_lo=1, v_hi=256)
MORPH = dict(erode=3, dilate=7, area=(20.0, 1e6))
BLUE = dict(h=(100, 125), s=(150, 256), v=(100, 256), **MORPH)               # DISC_BGR[0]
RED = dict(h=(0, 20), s=(150, 256), v=(100, 256), **MORPH)                   # DISC_BGR[1]
GREEN = dict(h=(50, 70), s=(150, 256), v=(100, 256), **MORPH)                # DISC_BGR[2]


def _hp(rows, cols, n, ch=3, **kw):
    import oat_amd
    if ch == 1:
        return oat_amd.HotPath(rows, cols, n_streams=n, channels=1, adaptation_coeff=LR, h_thresh=(1, 256), erode=3, dilate=7,
                               area=(20.0, 1e6), **kw)
    return oat_amd.HotPath(rows, cols, n_streams=n, adaptation_coeff=LR, erode=3, dilate=7, area=(20.0, 1e6), **NZ, **kw)


def _fg_params(ch=3):
    if ch == 1:
        return O.hsv_params(h_lo=1, h_hi=256, erode=3, dilate=7, min_area=20.0, max_area=1e6)
    return O.hsv_params(**NZ_P, erode=3, dilate=7, min_area=20.0, max_area=1e6)


def _streams(rows, cols, n, T, n_discs=3, ch=3, seed=0):
    """[T][n] frames, the first without discs."""
    from oat_amd.synth import SyntheticStream
    sts = [SyntheticStream(rows, cols, seed + s, n_discs=n_discs) for s in range(n)]
    out = []
    for t in range(T):
        fs = [st.frame(t, with_discs=t > 0) for st in sts]
        out.append([O.bgr2grey(f) if ch == 1 else f for f in fs])
    return out


def _same_detection(got, want, tag):
    print("   ", tag, "got", (got.position_valid, got.first_pixel, got.a00, got.a10, got.a01, got.x, got.y), "want",
          (want["valid"], want["first_pixel"], want["a00"], want["a10"], want["a01"], want["x"], want["y"]))
    assert got.position_valid == want["valid"], tag
    if want["valid"]:
        assert (got.first_pixel, got.a00, got.a10, got.a01) == (want["first_pixel"], want["a00"], want["a10"], want["a01"]), tag
        assert abs(got.x - want["x"]) <= 1e-4 and abs(got.y - want["y"]) <= 1e-4, tag


def _bits(x):
    return struct.pack("<d", x)


def _same_combined(got, markers, anchor, tag):
    """bit-equal to the restatement, computed from the library's own marker centroids"""
    want = MR.combine([(p.position_valid, p.x, p.y) for p in markers], anchor)
    print("   ", tag, "combined got", got, "want", want)
    assert (got.position_valid, got.heading_valid, got.velocity_valid, got.n_valid) == \
        (want["position_valid"], want["heading_valid"], want["velocity_valid"], want["n_valid"]), tag
    for k in ("x", "y", "hx", "hy"):
        assert _bits(getattr(got, k)) == _bits(want[k]) or (np.isnan(getattr(got, k)) and np.isnan(want[k])), (tag, k)


class _Rig:
    """n cameras x M markers of oracle chains (+ one chain per camera for the context's own, non-zero window)."""

    def __init__(self, rows, cols, n, markers, ch=3, threads=1):
        self.n, self.M, self.ch = n, len(markers), ch
        self.cams = [MR.MarkerOracle(rows, cols, ch, markers, nthreads=threads) for _ in range(n)]
        self.fg = [O.Mog2(rows, cols, ch) for _ in range(n)]
        self.fg_p = _fg_params(ch)
        self.pool = ThreadPoolExecutor(8)
        self.valid = np.zeros((n, self.M), int)
        self.all_valid = np.zeros(n, int)
        self.steps = 0

    def step(self, frames):
        """-> ([n][M] detections, [n][M] planes after erode / dilate, [n] own-window detections)"""
        jobs = [self.pool.submit(self.cams[s].step, frames[s], LR) for s in range(self.n)]
        fgj = [self.pool.submit(O.chain_step, self.fg[s], frames[s], LR, self.fg_p) for s in range(self.n)]
        res = [j.result() for j in jobs]
        return [r[0] for r in res], [r[1] for r in res], [j.result()[0] for j in fgj]

    def check(self, got, frames, anchor, tag, count=True):
        fg, markers, mean = got
        want, planes, want_fg = self.step(frames)
        for s in range(self.n):
            _same_detection(fg[s], want_fg[s], (tag, s, "fg"))
            for m in range(self.M):
                _same_detection(markers[s][m], want[s][m], (tag, s, m))
            _same_combined(mean[s], markers[s], anchor, (tag, s))
            if count:
                self.valid[s] += [int(want[s][m]["valid"]) for m in range(self.M)]
                self.all_valid[s] += int(all(want[s][m]["valid"] for m in range(self.M)))
        self.steps += int(count)
        return want, planes


# ------------------------------------------------------------------- 1: three markers, three cameras, 40 frames ---

@pytest.mark.parametrize("rows,cols", [(270, 480), (1080, 1920)])
def test_three_markers_three_cameras(rows, cols):
    """Windows H [100,125] / [0,20] / [50,70], S [150,256], V [100,256], erode 3, dilate 7, area [20, 1e6], lr 0.01; 3 streams,
    40 frames, the first without discs; anchor 0.  The oracle alone must find every marker on >= 90 % of the compared frames,
    so that the test cannot pass on empty results."""
    import torch
    n, T = 3, 40
    frames = _streams(rows, cols, n, T)
    rig = _Rig(rows, cols, n, [BLUE, RED, GREEN], threads=2 if rows > 500 else 1)
    hp = _hp(rows, cols, n)
    try:
        hp.set_markers([BLUE, RED, GREEN], heading_anchor=0)
        headings = 0
        for t, fs in enumerate(frames):
            if t % 2:                                    # device frames and host frames alternately
                dev = torch.from_numpy(np.stack(fs)).cuda()
                torch.cuda.synchronize()
                got = hp.track_markers_dev(dev.data_ptr())
            else:
                got = hp.track_markers(fs)
            rig.check(got, fs, 0, (rows, t), count=t > 0)
            headings += sum(int(c.heading_valid and abs(c.hx * c.hx + c.hy * c.hy - 1.0) < 1e-9) for c in got[2])
    finally:
        hp.close()
    print("oracle: frames with the marker valid, per stream and marker:", rig.valid.tolist(), "all three:", rig.all_valid.tolist(),
          "of", rig.steps)
    assert rig.steps == T - 1
    assert (rig.valid >= 0.9 * rig.steps).all(), rig.valid
    assert headings == rig.all_valid.sum() > 0, (headings, rig.all_valid)     # a unit heading exactly where all three markers were found


# --------------------------------------------------------------------- 2: the masks at all three taps, the model ---

def test_marker_masks_at_all_taps_and_the_model_is_undisturbed():
    from oat_amd import ffi
    import oat_amd
    rows, cols, n, T = 270, 480, 2, 12
    frames = _streams(rows, cols, n, T, seed=4)
    markers = [BLUE, dict(RED, erode=0, dilate=5), dict(GREEN, erode=2, dilate=0)]
    filt = [O.Mog2(rows, cols, 3) for _ in range(n)]
    rig = _Rig(rows, cols, n, markers)
    hp = _hp(rows, cols, n)
    plain = oat_amd.HotPath(rows, cols, n_streams=n, adaptation_coeff=LR, erode=3, dilate=7, area=(20.0, 1e6),
                            h_thresh=(100, 125), s_thresh=(150, 256), v_thresh=(100, 256))
    try:
        hp.set_markers(markers, heading_anchor=2)
        for t, fs in enumerate(frames):
            got = hp.track_markers(fs)
            plain.track(fs)
            _, planes = rig.check(got, fs, 2, ("taps", t))
            for s in range(n):
                masked, _ = filt[s].filter(fs[s], LR)
                assert (hp.read_mask(ffi.TAP_THRESHOLD, s) == np.where(masked.max(-1) != 0, 255, 0)).all(), (t, s)   # Z
                hsv = O.bgr2hsv(masked)
                for m, mk in enumerate(markers):
                    thr = O.inrange3(hsv, (mk["h"][0], mk["s"][0], mk["v"][0]), (mk["h"][1], mk["s"][1], mk["v"][1]))
                    assert (hp.read_marker_mask(m, ffi.TAP_THRESHOLD, s) == thr).all(), (t, s, m)
                    mor = thr
                    if mk["erode"] > 1:
                        mor = O.erode(mor, mk["erode"])
                    if mk["dilate"] > 1:
                        mor = O.dilate(mor, mk["dilate"])
                    assert (mor == planes[s][m]).all(), (t, s, m)                   # the oracle chain's own threshold_frame_
                    assert (hp.read_marker_mask(m, ffi.TAP_MORPH, s) == mor).all(), (t, s, m)
                    assert (hp.read_marker_mask(m, ffi.TAP_FINAL, s) == B.frame_zeroed(mor) * 255).all(), (t, s, m)
        for s in range(n):                     # markers do not disturb the model: bit-equal to a plain context's
            for a, b in zip(hp.mog_state(s), plain.mog_state(s)):
                assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), s
    finally:
        hp.close()
        plain.close()


# ------------------------------------------------------------------------------------- 3: per-camera windows ---

def test_per_camera_windows():
    """Stream 1's marker 0 moved to the red window: stream 1 gets the red disc there, the others the blue."""
    rows, cols, n, T = 270, 480, 3, 16
    frames = _streams(rows, cols, n, T, seed=1)
    rig = _Rig(rows, cols, n, [BLUE, RED])
    rig.cams[1].set_window(0, RED)
    hp = _hp(rows, cols, n)
    try:
        hp.set_markers([BLUE, RED], heading_anchor=1)
        hp.set_marker_window(1, 0, h=RED["h"], s=RED["s"], v=RED["v"])
        found = 0
        for t, fs in enumerate(frames):
            fg, mk, mean = hp.track_markers(fs)
            want, _ = rig.check((fg, mk, mean), fs, 1, ("percam", t))
            if t > 0 and want[1][1]["valid"]:
                a, b = mk[1]
                assert (a.position_valid, a.first_pixel, a.a00, a.a10, a.a01) == (b.position_valid, b.first_pixel, b.a00, b.a10, b.a01)
                assert mk[0][0].position_valid and mk[0][0].first_pixel != mk[0][1].first_pixel      # stream 0: blue is not red
                found += 1
        assert found >= T // 2
    finally:
        hp.close()


# ---------------------------------------------------------------------- 4: per-marker morphology and area ---

def test_per_marker_morphology_and_area():
    rows, cols, n, T = 270, 480, 2, 14
    frames = _streams(rows, cols, n, T, seed=2)
    markers = [BLUE,
               dict(BLUE, area=(1e5, 1e6)),                                       # an area window that excludes the disc
               dict(h=(0, 256), s=(0, 256), v=(0, 50), erode=0, dilate=0, area=(1000.0, 1e9)),   # holds (0,0,0): the background is the blob
               dict(h=(30, 20), s=(0, 256), v=(0, 256), erode=0, dilate=0),      # lo > hi: the empty window
               dict(BLUE, erode=0, dilate=10, area=(0.0, 1e7)),
               dict(RED, erode=5, dilate=3)]
    rig = _Rig(rows, cols, n, markers)
    hp = _hp(rows, cols, n)
    try:
        hp.set_markers(markers, heading_anchor=None)
        for t, fs in enumerate(frames):
            got = hp.track_markers(fs)
            want, _ = rig.check(got, fs, None, ("morph", t), count=t > 0)
            for s in range(n):
                assert not want[s][1]["valid"] and not want[s][3]["valid"]
                assert not got[2][s].position_valid and not got[2][s].heading_valid
                if t > 0:
                    assert want[s][2]["valid"] and want[s][2]["area"] > 0.5 * rows * cols
        assert (rig.valid[:, 0] >= 0.9 * rig.steps).all() and (rig.valid[:, 4] >= 0.9 * rig.steps).all(), rig.valid
    finally:
        hp.close()


# ----------------------------------------------------------------------------------------- 5: the GREY chain ---

def test_grey_chain_two_intensity_windows():
    rows, cols, n, T = 270, 480, 2, 16
    frames = _streams(rows, cols, n, T, ch=1, seed=5)
    markers = [dict(h=(55, 80), **MORPH), dict(h=(105, 125), **MORPH)]            # discs 0 and 1 in grey levels: 67 and 114
    rig = _Rig(rows, cols, n, markers, ch=1)
    hp = _hp(rows, cols, n, ch=1)
    try:
        hp.set_markers(markers, heading_anchor=0)
        for t, fs in enumerate(frames):
            rig.check(hp.track_markers(fs), fs, 0, ("grey", t), count=t > 0)
        assert (rig.valid >= rig.steps // 2).all(), rig.valid
    finally:
        hp.close()


# --------------------------------------------------------------------------- 6: ROI mask and undistort ---

def test_with_roi_mask_and_undistort():
    """The markers see what the model sees: the undistorted frame with the ROI applied.  Expected values from the oracle
    chain fed undistort_ref's frames with the ROI zeroed."""
    import undistort_ref as R
    rows, cols, n, T = 480, 640, 2, 12
    names = ("barrel", "mild5")
    cals = [R.cases(rows, cols)[k] for k in names]
    maps = [R.undistort_map(rows, cols, K, D) for K, D in cals]
    yy, xx = np.mgrid[0:rows, 0:cols]
    roi = (((xx - 330) ** 2 + (yy - 230) ** 2) < 200 ** 2).astype(np.uint8) * 255
    frames = _streams(rows, cols, n, T, seed=13)
    rig = _Rig(rows, cols, n, [BLUE, RED, GREEN])
    hp = _hp(rows, cols, n, undistort=cals)
    try:
        hp.set_roi_mask(roi, stream=0)
        hp.set_markers([BLUE, RED, GREEN], heading_anchor=0)
        for t, fs in enumerate(frames):
            seen = [R.remap(fs[s], *maps[s]) for s in range(n)]
            seen[0] = seen[0].copy()
            seen[0][roi == 0] = 0
            rig.check(hp.track_markers(fs), seen, 0, ("roi+ud", t), count=t > 0)
        assert rig.valid.sum() >= rig.steps * n, rig.valid            # discs were found
    finally:
        hp.close()


# ------------------------------------------------------- 7: a frame too busy for the single-workgroup kernel ---

def test_busy_frame_takes_the_global_fallback():
    rows, cols, n = 270, 480, 1
    rng = np.random.default_rng(11)
    frames = _streams(rows, cols, n, 10, n_discs=2, seed=3)
    markers = [dict(BLUE, erode=0, dilate=0, area=(0.0, 1e9)), RED]
    rig = _Rig(rows, cols, n, markers)
    hp = _hp(rows, cols, n)
    try:
        hp.set_markers(markers, heading_anchor=1)
        paths = []
        for t, fs in enumerate(frames):
            if t >= 6:                                   # 50 % noise in marker 0's window
                f = fs[0].copy()
                f[rng.random((rows, cols)) < 0.5] = (255, 64, 0)
                fs = [f]
            _, planes = rig.check(hp.track_markers(fs), fs, 1, ("busy", t))
            paths.append(B.blob_load(planes[0][0])["path"])
        print("paths of marker 0:", paths)
        assert paths[:6] == ["lds"] * 6 and paths[6:] == ["global"] * 4, paths
    finally:
        hp.close()


# ------------------------------------------------------------------------------------------------- 8: refusals ---

def test_refusals_leave_the_context_as_it_was():
    from oat_amd import ffi
    rows, cols, n = 270, 480, 2
    frames = _streams(rows, cols, n, 14, seed=6)
    mogs = [O.Mog2(rows, cols, 3) for _ in range(n)]
    it = iter(frames)
    hp = _hp(rows, cols, n)

    def plain_step(p=None):
        """an ordinary step on the same context still matches the oracle"""
        fs = next(it)
        got = hp.track(fs)
        for s in range(n):
            want, _ = O.chain_step(mogs[s], fs[s], LR, p or _fg_params())
            _same_detection(got[s], want, ("plain", s))

    def refused(fn, word):
        with pytest.raises(ffi.OatGpuError) as e:
            fn()
        assert e.value.code == -1 and word in str(e.value), str(e.value)

    try:
        plain_step()
        fs = next(it)
        refused(lambda: hp.track_markers(fs), "not configured")                      # markers off
        plain_step()
        refused(lambda: hp.set_markers([BLUE] * 9), "n_markers")
        refused(lambda: hp.set_markers([BLUE, RED], heading_anchor=2), "anchor")
        refused(lambda: hp.set_markers([dict(BLUE, erode=64)]), "erode")
        hp.set_markers([BLUE, RED], heading_anchor=0)
        hp.enqueue(fs)                                                               # results outstanding in the ring
        refused(lambda: hp.track_markers(fs), "outstanding")
        got = hp.collect()
        for s in range(n):
            want, _ = O.chain_step(mogs[s], fs[s], LR, _fg_params())
            _same_detection(got[s], want, ("ring", s))
        plain_step()
        hp.set_kalman(True, dt=0.02, timeout=1.0)                                    # the position filter
        refused(lambda: hp.track_markers(fs), "oatgpu_set_kalman")
        hp.set_kalman(False)
        plain_step()
        hp.set_homography([1, 0, 0, 0, 1, 0, 0, 0, 1])
        refused(lambda: hp.track_markers(fs), "homography")
        hp.set_homography(None)
        plain_step()
        disc = dict(h_lo=100, h_hi=125, s_lo=150, s_hi=256, v_lo=100, v_hi=256)
        hp._chk(hp.lib.oatgpu_set_detector(hp.ctx, 100, 125, 150, 256, 100, 256, 3, 7, 20.0, 1e6))    # the wrong own window
        refused(lambda: hp.track_markers(fs), "non-zero window")
        plain_step(O.hsv_params(**disc, erode=3, dilate=7, min_area=20.0, max_area=1e6))
        hp._chk(hp.lib.oatgpu_set_detector(hp.ctx, 0, 256, 0, 256, 1, 256, 3, 7, 20.0, 1e6))
        refused(lambda: hp.set_marker_window(0, 2, h=(0, 20)), "marker index")       # marker index out of range
        refused(lambda: hp.set_marker_window(2, 0, h=(0, 20)), "stream index")
        refused(lambda: hp.read_marker_mask(2), "marker index")
        refused(lambda: hp.set_marker_window(0, 0, h=(0, 300)), "between 0 and 256")
        plain_step()
        # ... and after all that a marker step is still right (one model, the masked frame through each marker's detector)
        fs = next(it)
        fg, mk, mean = hp.track_markers(fs)
        for s in range(n):
            masked, _ = mogs[s].filter(fs[s], LR)
            hsv = O.bgr2hsv(masked)
            _same_detection(fg[s], O.detect_hsv(hsv, _fg_params())[0], ("after", s, "fg"))
            for m, mk_m in enumerate((BLUE, RED)):
                _same_detection(mk[s][m], O.detect_hsv(hsv, MR.hsv_params_of(mk_m))[0], ("after", s, m))
            _same_combined(mean[s], mk[s], 0, ("after", s))
            assert mk[s][0].position_valid or mk[s][1].position_valid
    finally:
        hp.close()


# ----------------------------------------------------------------------------------- 9: n_markers back to 0 ---

def test_markers_off_again_is_an_ordinary_context():
    import oat_amd
    from oat_amd import ffi
    rows, cols, n = 270, 480, 2
    frames = _streams(rows, cols, n, 16, seed=8)
    a, b = _hp(rows, cols, n), _hp(rows, cols, n)
    try:
        a.set_markers([BLUE, RED, GREEN], heading_anchor=0)
        for t, fs in enumerate(frames):
            if t == 8:
                a.set_markers([])
                with pytest.raises(ffi.OatGpuError):
                    a.track_markers(fs)
            got = a.track_markers(fs)[0] if t < 8 else a.track(fs)
            want = b.track(fs)                           # a context that never heard of markers, same frames
            assert [tuple(vars(p).values()) for p in got] == [tuple(vars(p).values()) for p in want], t
        for s in range(n):
            for x, y in zip(a.mog_state(s), b.mog_state(s)):
                assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True), s
            assert (a.read_mask(ffi.TAP_FINAL, s) == b.read_mask(ffi.TAP_FINAL, s)).all()
        assert any(p.position_valid for p in want)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------ 10: the process pipeline ---

def _mk_arg(m):
    return "H=[%d,%d] S=[%d,%d] V=[%d,%d] e=%d d=%d area=[%r,%r]" % (*m["h"], *m["s"], *m["v"], m["erode"], m["dilate"], *m["area"])


def test_process_pipeline_markers_and_heading(tmp_path):
    """oat-frameserve-raw -> oat-track-hip --marker .. --marker .. --heading-anchor 0: one oat-posi-cout on each marker's sink
    and one on the camera's SINK receive the per-marker and the combined records, heading included."""
    import json
    from test_host_pipeline import _consumers_ready
    subprocess.check_call(["make", "-s", "-j4", "-C", ROOT, "host"])
    rows, cols, T = 270, 480, 20
    frames = [fs[0] for fs in _streams(rows, cols, 1, T, seed=21)]
    raw = tmp_path / "frames.raw"
    np.stack(frames).tofile(raw)
    tag = "oat_m_" + uuid.uuid4().hex[:8]
    src, pos, ma, mb = (tag + x for x in ("src", "pos", "blue", "red"))
    exe = lambda b: os.path.join(BIN, b)
    readers = [subprocess.Popen([exe("oat-posi-cout"), a], stdout=subprocess.PIPE, text=True) for a in (ma, mb, pos)]
    track = subprocess.Popen([exe("oat-track-hip"), src, pos, "-a", str(LR), "-e", "3", "-d", "7", "--area", "[20,1000000]",
                              "--marker", _mk_arg(BLUE), "--marker", _mk_arg(RED), "--marker-sinks", f"{ma},{mb}",
                              "--heading-anchor", "0"])
    _consumers_ready(src, ma, mb, pos)
    feeder = subprocess.Popen([exe("oat-frameserve-raw"), src, "-f", str(raw), "--rows", str(rows), "--cols", str(cols),
                               "-n", str(T), "-r", "200"])
    try:
        outs = [r.communicate(timeout=180)[0] for r in readers]
        feeder.wait(timeout=60)
        track.wait(timeout=60)
    finally:
        for p in readers + [track, feeder]:
            if p.poll() is None:
                p.kill()
        subprocess.run([exe("oat-clean-hip"), src, pos, ma, mb], capture_output=True)
    assert track.returncode == 0
    recs = [[json.loads(l) for l in o.splitlines() if l.strip()] for o in outs]
    assert [len(r) for r in recs] == [T, T, T]
    rig = MR.MarkerOracle(rows, cols, 3, [BLUE, RED])
    both = 0
    for t, f in enumerate(frames):
        want, _ = rig.step(f, LR)
        for m in range(2):
            g = recs[m][t]
            assert g["tick"] == t + 1 and g["pos_ok"] == want[m]["valid"] and g["head_ok"] is False, (t, m, g)   # Sample propagated
            if want[m]["valid"]:
                assert abs(g["pos_xy"][0] - want[m]["x"]) <= 1e-4 and abs(g["pos_xy"][1] - want[m]["y"]) <= 1e-4, (t, m, g)
        c = MR.combine([(w["valid"], w["x"] if w["valid"] else 0.0, w["y"] if w["valid"] else 0.0) for w in want], 0)
        g = recs[2][t]
        assert (g["tick"], g["pos_ok"], g["head_ok"], g["vel_ok"]) == (t + 1, c["position_valid"], c["heading_valid"], False), (t, g, c)
        if c["position_valid"]:
            assert abs(g["pos_xy"][0] - c["x"]) <= 1e-4 and abs(g["pos_xy"][1] - c["y"]) <= 1e-4, (t, g, c)
        if c["heading_valid"]:
            assert abs(g["head_xy"][0] - c["hx"]) <= 1e-5 and abs(g["head_xy"][1] - c["hy"]) <= 1e-5, (t, g, c)
            both += 1
    assert both >= T - 3, both
