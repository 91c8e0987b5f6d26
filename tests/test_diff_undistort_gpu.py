"""GPU tests of the motion tracker with lens undistortion inside its front kernel (oatgpu_set_tracker_undistort;
MotionTracker.undistort; k_diff_remap_wide / k_diff_remap_narrow).  The reference for a run with the switch on is
the packed tracker fed undistort_ref.remap(frame, the stream's map) -- positions field for field, every tap byte for byte --, and
beside it the oracle chain and the numpy front end on the same undistorted frames (tests/tracker_undistort_cases.py;
tests/test_tracker_undistort_cpu.py holds that case list to non-vacuity and to the planted wrong front ends).  Every comparison
is bit for bit.  Every frame is under 0.1 MP.

The lane mapping under the switch follows the frame width alone (W % 4 == 0: wide): the frames are gathered with unaligned
loads and the last grey image is the context's own, aligned allocation, so the geometry list is what selects the mapping -- the
narrow one at (37, 91) and (3, 3), the wide one at the seven others -- and a frame pointer one byte off must change nothing."""
import ctypes as C

import numpy as np
import pytest

import diff_cases as D
import tracker_undistort_cases as T
from parity_asserts import _same_detection

pytestmark = pytest.mark.gpu

E_INVALID = -1
THR, MORPH, FIN = 0, 1, 2
FIELDS = ("position_valid", "x", "y", "area", "a00", "a10", "a01", "first_pixel")


@pytest.fixture(scope="module")
def A():
    import oat_amd
    return oat_amd


def _dev(frames):
    """[n_streams] host frames -> a stream-major device tensor (kept by the caller while the library reads it)."""
    import torch
    t = torch.from_numpy(np.stack(frames)).cuda()
    torch.cuda.synchronize()
    return t


def _calibrate(mt, uc, cals=None):
    for s, k in enumerate(cals or uc.cals):
        mt.set_undistort(s, *T.calibration(uc.c.rows, uc.c.cols, k))


def _tracker(A, uc, on=False, cals=None):
    c = uc.c
    mt = A.MotionTracker(c.rows, c.cols, n_streams=c.n_streams, channels=c.channels, diff_threshold=c.diff_threshold, blur=c.blur,
                         area=D.AREA)
    if on:
        _calibrate(mt, uc, cals)
        mt.undistort(True)
    return mt


def _taps(mt, s, read=None):
    read = read or mt.read_mask
    return [read(w, s) for w in (THR, MORPH, FIN)]


def _same_as(got, ref, tag):
    """positions of a step with the switch on against the packed tracker's on the undistorted frames: every field"""
    for s, (g, r) in enumerate(zip(got, ref)):
        for f in FIELDS:
            a, b = getattr(g, f), getattr(r, f)
            assert a == b or (a != a and b != b), (tag, s, f, a, b)


def _same_taps(mt, ref, n, tag, read=None, ref_read=None):
    for s in range(n):
        for p, q in zip(_taps(mt, s, read), _taps(ref, s, ref_read)):
            assert p.tobytes() == q.tobytes(), (tag, s)


def _check_want(mt, got, want_t, tag, read=None):
    """... and against the oracle chain and the numpy front end"""
    for s, (det, bits, omask, first) in enumerate(want_t):
        _same_detection(got[s], det, (tag, s))
        thr, morph, _ = _taps(mt, s, read)
        assert ((thr > 0) == bits).all(), ("threshold tap", tag, s)
        if first:
            assert ((morph > 0) == omask).all(), ("morph tap of a first frame", tag, s)
        else:
            assert ((morph > 0)[1:-1, 1:-1] == omask[1:-1, 1:-1]).all(), ("morph tap", tag, s)


def _roi_to(trackers, c, t, on):
    now = c.roi_at(t, c.roi_stream) is not None
    if now != on:
        for mt in trackers:
            mt.set_roi_mask(c.roi if now else None, stream=c.roi_stream)
    return now


def _probe(last, thr, k):
    """A grey frame whose difference from `last` is thr + k (k 0 / 1 per pixel), upwards where that fits into a byte"""
    L = last.astype(np.int32)
    return np.where(L + thr + 1 <= 255, L + thr + k, L - thr - k).astype(np.uint8)


def _context_mask(mt, which, s):
    """oatgpu_read_mask (the single-stage calls' planes), not the tracker's own taps"""
    from oat_amd import ffi
    out = np.empty((mt.rows, mt.cols), np.uint8)
    mt._chk(mt.lib.oatgpu_read_mask(mt.ctx, s, which, ffi.u8(out)))
    return out


def _check_last_grey(mt_a, mt_b, s, last, thr):
    """The last grey image of stream s, read by advancing with oatgpu_detect_diff: two trackers in the same state take two
    probes with complementary checkerboards of |difference| = thr and thr + 1.  A pixel of the state that is off its model
    flips a bit of one of the two; the threshold plane of either must be its checkerboard exactly."""
    from oat_amd import ffi
    yy, xx = np.mgrid[0:last.shape[0], 0:last.shape[1]]
    for mt, k in ((mt_a, (yy + xx) & 1), (mt_b, (yy + xx + 1) & 1)):
        p = ffi.Position()
        mt._chk(mt.lib.oatgpu_detect_diff(mt.ctx, s, ffi.u8(_probe(last, thr, k)), C.byref(p)))
        got = _context_mask(mt, THR, s) > 0
        assert (got == (k == 1)).all(), ("last grey", s, int((got != (k == 1)).sum()))


# ------------------------------------------------------------------------------------------ the synchronous step ----

@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("cal", T.CALS)
@pytest.mark.parametrize("rows,cols", T.GEOMETRIES)
def test_every_geometry_and_calibration_on_device_and_host_frames(A, rows, cols, cal, channels):
    uc, want = T.diff_want(rows, cols, channels, (cal,))
    dev, ref = _tracker(A, uc, on=True), _tracker(A, uc)
    c = uc.c
    host = A.MotionTracker(rows, cols, n_streams=1, channels=channels, diff_threshold=c.diff_threshold, blur=c.blur, area=D.AREA,
                           undistort=uc.calibration(0))          # (the constructor's keyword)
    for t in range(len(uc.given)):
        und, given = _dev(uc.und[t]), _dev(uc.given[t])
        want_pos = ref.track_dev(und.data_ptr())
        for mt, got, tag in ((dev, dev.track_dev(given.data_ptr()), "dev"), (host, host.track(uc.given[t]), "host")):
            _same_as(got, want_pos, (tag, t))
            _same_taps(mt, ref, 1, (tag, t))
            _check_want(mt, got, want[t], (tag, t))
    # the state behind the last frame: the grey of the last undistorted frame
    _check_last_grey(dev, host, 0, D.grey_of(uc.und[-1][0]), c.diff_threshold)


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("rows,cols", [(90, 200), (37, 91)])      # wide and narrow
def test_three_streams_three_calibrations_and_a_roi_set_and_removed(A, rows, cols, channels):
    """... and the swapped assignment of the calibrations gives other planes: the map is per stream"""
    uc, want = T.diff_want(rows, cols, channels, T.THREE, roi=True)
    und, ref, swapped = _tracker(A, uc, on=True), _tracker(A, uc), _tracker(A, uc, on=True, cals=T.THREE_SWAPPED)
    on, differs, with_roi = False, 0, 0
    for t in range(len(uc.given)):
        on = _roi_to((und, ref, swapped), uc.c, t, on)
        with_roi += on
        u, g = _dev(uc.und[t]), _dev(uc.given[t])
        want_pos = ref.track_dev(u.data_ptr())
        got = und.track_dev(g.data_ptr())
        _same_as(got, want_pos, (rows, t))
        _same_taps(und, ref, 3, (rows, t))
        _check_want(und, got, want[t], (rows, t))
        swapped.track_dev(g.data_ptr())
        differs += [(swapped.read_mask(THR, s) != und.read_mask(THR, s)).any() for s in range(3)] == [True, True, False]
    assert 0 < with_roi < len(uc.given)
    assert differs >= len(uc.given) // 2                         # streams 0 and 1 differ, stream 2 (the same calibration) never


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("rows,cols", [(33, 128), (90, 200), (37, 91)])
def test_a_device_pointer_one_byte_off(A, rows, cols, channels):
    import torch
    uc, want = T.diff_want(rows, cols, channels, T.THREE)
    und, ref = _tracker(A, uc, on=True), _tracker(A, uc)
    size = 3 * rows * cols * channels
    store = torch.zeros(size + 8, dtype=torch.uint8, device="cuda")
    view = store[1:1 + size]
    assert view.data_ptr() % 4 == 1
    for t in range(6):
        view.copy_(torch.from_numpy(np.stack(uc.given[t]).reshape(-1)))
        u = _dev(uc.und[t])
        want_pos = ref.track_dev(u.data_ptr())
        got = und.track_dev(view.data_ptr())
        _same_as(got, want_pos, t)
        _same_taps(und, ref, 3, t)
        _check_want(und, got, want[t], t)
    view.copy_(torch.from_numpy(np.stack(uc.given[6]).reshape(-1)))        # ... and as the second frame of a paired launch
    g5 = _dev(uc.given[5])
    und.reset()
    ref.reset()
    got = und.track_sequence_dev([g5.data_ptr(), g5.data_ptr(), view.data_ptr()])
    for i, t in enumerate((5, 5, 6)):
        u = _dev(uc.und[t])
        _same_as(got[i], ref.track_dev(u.data_ptr()), ("pair", t))
    _same_taps(und, ref, 3, "pair")


def test_sixty_six_streams_cross_the_launch_split(A):
    """5 x 4 frames; the streams behind the split carry other calibrations than streams 0 and 1"""
    cals = tuple(T.CALS[(s + s // 64) % 3] for s in range(66))
    assert cals[64] != cals[0] and cals[65] != cals[1]
    for channels in (3, 1):
        uc, want = T.diff_want(5, 4, channels, cals, n_frames=5)
        und, ref = _tracker(A, uc, on=True), _tracker(A, uc)
        bufs = [_dev(fs) for fs in uc.given]
        for t in range(3):
            u = _dev(uc.und[t])
            want_pos = ref.track_dev(u.data_ptr())
            got = und.track_dev(bufs[t].data_ptr())
            _same_as(got, want_pos, t)
            _same_taps(und, ref, 66, t)
            _check_want(und, got, want[t], t)
        got = und.track_sequence_dev([bufs[3].data_ptr(), bufs[4].data_ptr()])              # ... and a paired launch across it
        for i, t in enumerate((3, 4)):
            u = _dev(uc.und[t])
            _same_as(got[i], ref.track_dev(u.data_ptr()), ("pair", t))
        _same_taps(und, ref, 66, "pair")
        _check_want(und, got[1], want[4], "pair")


# ----------------------------------------------------------------------------------------------- the sequence call ----

@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("rows,cols", [(90, 200), (37, 91), (12, 1040), (5, 4)])
def test_sequence_with_paired_launches_and_a_first_frame_inside(A, rows, cols, channels):
    """A fresh sequence (a lone first frame, then pairs), a sequence from a mixed state after reset(1) (single launches until
    every stream has a last image), a synchronous step behind it: the packed tracker takes the undistorted frames in
    synchronous steps, and a second tracker with the switch on takes the given frames in single launches."""
    uc, want = T.diff_want(rows, cols, channels, T.THREE, roi=True)
    und, single, ref = _tracker(A, uc, on=True), _tracker(A, uc, on=True), _tracker(A, uc)
    for mt in (und, single, ref):                               # (one ROI on stream 1 for the whole run)
        mt.set_roi_mask(uc.c.roi, stream=uc.c.roi_stream)
    bufs = [_dev(fs) for fs in uc.given]
    unds = [_dev(fs) for fs in uc.und]

    def run(ts, tag):
        got = und.track_sequence_dev([bufs[t].data_ptr() for t in ts])
        for i, t in enumerate(ts):
            want_pos = ref.track_dev(unds[t].data_ptr())
            _same_as(got[i], want_pos, (tag, t))
            _same_as(single.track_dev(bufs[t].data_ptr()), want_pos, (tag, "single", t))
        _same_taps(und, ref, 3, tag)
        _same_taps(und, single, 3, (tag, "single"))

    run([0, 1, 2, 3, 4, 5], "fresh")
    for mt in (und, single, ref):
        mt.reset(1)
    run([6, 7, 8, 9, 10], "after reset(1)")
    for mt in (und, single, ref):
        mt.reset()
    run([3, 4, 5, 6], "after reset()")
    _same_as(und.track_dev(bufs[11].data_ptr()), ref.track_dev(unds[11].data_ptr()), "next")
    _same_taps(und, ref, 3, "next")
    single.track_dev(bufs[11].data_ptr())
    for s in range(3):                                          # the state: the grey of the undistorted frame, 0 outside the ROI
        g = D.grey_of(uc.und[11][s])
        if s == uc.c.roi_stream:
            g = np.where(uc.c.roi != 0, g, 0).astype(np.uint8)
        _check_last_grey(und, single, s, g, uc.c.diff_threshold)


@pytest.mark.parametrize("channels", [3, 1])
def test_a_sequence_equals_the_oracle(A, channels):
    uc, want = T.diff_want(90, 200, channels, T.THREE)
    und = _tracker(A, uc, on=True)
    bufs = [_dev(fs) for fs in uc.given]
    got = und.track_sequence_dev([b.data_ptr() for b in bufs])
    for t in range(len(bufs)):
        for s in range(3):
            _same_detection(got[t][s], want[t][s][0], (t, s))
    _check_want(und, got[-1], want[-1], "last")
    twin = _tracker(A, uc, on=True)
    twin.track_sequence_dev([b.data_ptr() for b in bufs])
    for s in range(3):                                          # the state behind a sequence that ended in a paired launch
        _check_last_grey(und, twin, s, D.grey_of(uc.und[-1][s]), uc.c.diff_threshold)


# -------------------------------------------------------------------------------------------------------- state ----

@pytest.mark.parametrize("channels", [3, 1])
def test_steps_with_the_switch_on_off_and_detect_diff_continue_one_stream(A, channels):
    """Steps with the switch on (given frames), off (undistorted frames) and oatgpu_detect_diff on undistorted grey frames in
    turn: every stream equals a reference that saw the undistorted frames one after the other -- the state lives in the
    undistorted domain."""
    from oat_amd import ffi
    uc, _ = T.diff_want(90, 200, channels, T.THREE)
    c = uc.c
    mt, ref = _tracker(A, uc), _tracker(A, uc)
    _calibrate(mt, uc)
    refs = [T.DiffRef(c) for _ in range(3)]
    for t in range(len(uc.given)):
        u = _dev(uc.und[t])
        kind = ("on", "off", "single")[t % 3]
        if kind == "single":
            for s in range(3):
                g, p, q = D.grey_of(uc.und[t][s]), ffi.Position(), ffi.Position()
                mt._chk(mt.lib.oatgpu_detect_diff(mt.ctx, s, ffi.u8(g), C.byref(p)))
                ref._chk(ref.lib.oatgpu_detect_diff(ref.ctx, s, ffi.u8(g), C.byref(q)))
                _same_detection(A.Position2D.from_c(p), refs[s].step(g)[0], (t, s))
            continue
        want_pos = ref.track_dev(u.data_ptr())
        if kind == "on":
            mt.undistort(True)
            buf = _dev(uc.given[t])
            got = mt.track_dev(buf.data_ptr())
            mt.undistort(False)
        else:
            got = mt.track_dev(u.data_ptr())
        _same_as(got, want_pos, (kind, t))
        _same_taps(mt, ref, 3, (kind, t))
        _check_want(mt, got, [refs[s].step(uc.und[t][s]) for s in range(3)], (kind, t))


def test_a_recalibration_between_steps_takes_effect_from_the_next_frame(A):
    import undistort_ref as R
    uc, _ = T.diff_want(90, 200, 3, T.THREE)
    c = uc.c
    und, ref = _tracker(A, uc, on=True), _tracker(A, uc)
    cals = list(T.THREE)
    changed = 0
    for t in range(8):
        if t == 3:                                              # stream 1 from pincushion to skew, the switch staying on
            cals[1] = "skew"
            und.set_undistort(1, *T.calibration(c.rows, c.cols, "skew"))
        frames = [R.remap(uc.given[t][s], *T.maps(c.rows, c.cols, cals[s])) for s in range(3)]
        changed += t >= 3 and (frames[1] != uc.und[t][1]).any()
        u, g = _dev(frames), _dev(uc.given[t])
        _same_as(und.track_dev(g.data_ptr()), ref.track_dev(u.data_ptr()), t)
        _same_taps(und, ref, 3, t)
    assert changed == 5


# ------------------------------------------------------------------------------------ refusals, the context's other calls ----

def _both(A, c):
    """A context with the fused tracker's detector AND the motion tracker (MotionTracker's methods serve any context)."""
    hp = A.HotPath(c.rows, c.cols, n_streams=c.n_streams, adaptation_coeff=0.01, erode=0, dilate=3, area=D.AREA,
                   diff_threshold=c.diff_threshold, blur=c.blur, h_thresh=(0, 256), s_thresh=(0, 256), v_thresh=(60, 256))
    hp._chk(hp.lib.oatgpu_set_diff_tracker(hp.ctx, 1))
    return hp


def test_refusals_leave_the_context_usable_and_unchanged(A):
    from oat_amd import ffi
    uc, want = T.diff_want(90, 200, 3, T.THREE)
    _, plain = T.diff_want(90, 200, 3, T.THREE, plain=True)
    c, n = uc.c, 3
    hp = _both(A, c)
    lib, ctx = hp.lib, hp.ctx
    rd = lambda which, s: A.MotionTracker.read_mask(hp, which, s)          # noqa: E731
    bufs = [_dev(fs) for fs in uc.given]
    out = (ffi.Position * n)()
    K, Dc = uc.calibration(0)
    Kc, Dd = (C.c_double * 9)(*K), (C.c_double * len(Dc))(*Dc)

    def refused(rc, *needles):
        assert rc == E_INVALID
        msg = lib.oatgpu_last_error(ctx).decode()
        assert all(k in msg for k in needles), msg

    # no stream has a map, then only streams 0 and 2: on = 1 names the first stream without one
    refused(lib.oatgpu_set_tracker_undistort(ctx, 1), "stream 0", "no undistortion map")
    hp.set_undistort(0, *uc.calibration(0))
    hp.set_undistort(2, *uc.calibration(2))
    refused(lib.oatgpu_set_tracker_undistort(ctx, 1), "stream 1", "no undistortion map")
    hp.set_undistort(1, *uc.calibration(1))
    refused(lib.oatgpu_set_tracker_undistort(ctx, 2), "0 (off) or 1 (on)")
    refused(lib.oatgpu_set_tracker_undistort(ctx, -1), "0 (off) or 1 (on)")
    hp.enqueue_dev(bufs[0].data_ptr(), keepalive=bufs[0])
    refused(lib.oatgpu_set_tracker_undistort(ctx, 1), "outstanding")
    hp.collect()
    hp.stage(0, uc.given[0][0])
    refused(lib.oatgpu_set_tracker_undistort(ctx, 1), "staged")
    hp.stage_abort()
    pat = (C.c_int32 * 1)(1)
    assert lib.oatgpu_set_tracker_bayer(ctx, pat, 1) == 0
    refused(lib.oatgpu_set_tracker_undistort(ctx, 1), "oatgpu_set_tracker_bayer")
    assert lib.oatgpu_set_tracker_bayer(ctx, None, 0) == 0
    # the switch is off and stayed off through every refusal: a step on the given frames is the oracle's WITHOUT undistortion
    got = A.MotionTracker.track_dev(hp, bufs[0].data_ptr())
    _check_want(hp, got, plain[0], "off after refusals", read=rd)
    A.MotionTracker.reset(hp)
    # the switch is on and stays on through every refusal
    assert lib.oatgpu_set_tracker_undistort(ctx, 1) == 0
    refused(lib.oatgpu_set_tracker_undistort(ctx, 3), "0 (off) or 1 (on)")
    refused(lib.oatgpu_set_tracker_bayer(ctx, pat, 1), "oatgpu_set_tracker_undistort")
    refused(lib.oatgpu_set_undistort(ctx, 1, Kc, Dd, 0), "stream 1", "oatgpu_set_tracker_undistort")
    hp.enqueue_dev(bufs[0].data_ptr(), keepalive=bufs[0])
    refused(lib.oatgpu_set_tracker_undistort(ctx, 0), "outstanding")
    hp.collect()
    got = A.MotionTracker.track_dev(hp, bufs[0].data_ptr())
    _check_want(hp, got, want[0], "on after refusals", read=rd)
    # oatgpu_set_track_undistort is another switch: while it is on the diff calls are refused as before
    hp.undistort(True)
    refused(lib.oatgpu_diff_batch_dev(ctx, C.c_void_p(bufs[1].data_ptr()), out), "oatgpu_set_track_undistort")
    arr = (C.c_void_p * 1)(bufs[1].data_ptr())
    refused(lib.oatgpu_diff_sequence_dev(ctx, arr, 1, out), "oatgpu_set_track_undistort")
    hp.undistort(False)
    hp.set_kalman(True)
    refused(lib.oatgpu_diff_batch_dev(ctx, C.c_void_p(bufs[1].data_ptr()), out), "oatgpu_set_kalman")
    hp.set_kalman(False)
    got = A.MotionTracker.track_dev(hp, bufs[1].data_ptr())
    _check_want(hp, got, want[1], "on after the other switches", read=rd)
    # off again: the map of a stream may go, and on = 1 is refused once more
    assert lib.oatgpu_set_tracker_undistort(ctx, 0) == 0
    assert lib.oatgpu_set_undistort(ctx, 1, Kc, Dd, 0) == 0
    refused(lib.oatgpu_set_tracker_undistort(ctx, 1), "stream 1")
    und2 = _dev(uc.und[2])
    got = A.MotionTracker.track_dev(hp, und2.data_ptr())
    _check_want(hp, got, want[2], "packed again", read=rd)


def test_the_contexts_other_calls_work_beside_the_switch(A):
    """A fused track_batch and oatgpu_undistort_dev on a context whose motion tracker undistorts"""
    import oracle_lib as O
    import torch
    uc, want = T.diff_want(90, 200, 3, T.THREE)
    c, n = uc.c, 3
    hp = _both(A, c)
    _calibrate(hp, uc)
    hp._chk(hp.lib.oatgpu_set_tracker_undistort(hp.ctx, 1))
    rd = lambda which, s: A.MotionTracker.read_mask(hp, which, s)          # noqa: E731
    p = O.hsv_params(h_lo=0, h_hi=256, s_lo=0, s_hi=256, v_lo=60, v_hi=256, erode=0, dilate=3, min_area=D.AREA[0], max_area=D.AREA[1])
    mogs = [O.Mog2(c.rows, c.cols, 3) for _ in range(n)]
    out = torch.zeros(n * c.rows * c.cols * 3, dtype=torch.uint8, device="cuda")
    for t in range(4):
        g = _dev(uc.given[t])
        got = A.MotionTracker.track_dev(hp, g.data_ptr())
        _check_want(hp, got, want[t], ("on", t), read=rd)
        pos = hp.track(uc.given[t])                             # the fused tracker does not look at this switch
        for s in range(n):
            w, mask = O.chain_step(mogs[s], uc.given[t][s], 0.01, p)
            _same_detection(pos[s], w, ("track", t, s))
            assert (hp.read_mask(MORPH, s) == mask).all(), ("track", t, s)
        hp._chk(hp.lib.oatgpu_undistort_dev(hp.ctx, C.c_void_p(g.data_ptr()), C.c_void_p(out.data_ptr())))
        hp.synchronize()
        assert np.array_equal(out.cpu().numpy().reshape(n, c.rows, c.cols, 3), np.stack(uc.und[t])), t
