"""GPU tests of the motion tracker on Bayer RAW8 frames (oatgpu_set_tracker_bayer; MotionTracker.bayer; k_diff_raw_wide /
k_diff_raw_narrow).  The reference for a RAW8 run is the BGR tracker fed debayer_ref.demosaic(raw, pattern) --
positions field for field, every tap byte for byte --, and beside it the oracle chain and the numpy front end on the same
demosaiced frames (tests/tracker_bayer_cases.py; tests/test_tracker_bayer_cpu.py holds that case list to non-vacuity and to the
planted wrong front ends).  Every comparison is bit for bit.  Every frame is under 0.1 MP."""
import ctypes as C

import numpy as np
import pytest

import debayer_ref as R
import diff_cases as D
import tracker_bayer_cases as T
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


def _tracker(A, rc, bayer=None):
    c = rc.c
    return A.MotionTracker(c.rows, c.cols, n_streams=c.n_streams, channels=3, diff_threshold=c.diff_threshold, blur=c.blur,
                           area=D.AREA, bayer=bayer)


def _taps(mt, s, read=None):
    read = read or mt.read_mask
    return [read(w, s) for w in (THR, MORPH, FIN)]


def _same_as(got, ref, tag):
    """positions of a RAW8 step against the BGR tracker's on the demosaiced frames: every field"""
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
    mt._chk(mt.lib.oatgpu_read_mask(mt.ctx, which, s, ffi.u8(out)))
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

@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("rows,cols", T.GEOMETRIES)
def test_every_geometry_and_pattern_on_device_and_host_frames(A, rows, cols, pattern):
    rc, want = T.diff_want(rows, cols, (pattern,))
    dev, host, ref = _tracker(A, rc, bayer=R.NAMES[pattern]), _tracker(A, rc, bayer=pattern), _tracker(A, rc)
    assert dev.frame_shape == (rows, cols) and ref.frame_shape == (rows, cols, 3)
    for t in range(len(rc.raw)):
        bgr, raw = _dev(rc.bgr[t]), _dev(rc.raw[t])
        want_pos = ref.track_dev(bgr.data_ptr())
        for mt, got, tag in ((dev, dev.track_dev(raw.data_ptr()), "dev"), (host, host.track(rc.raw[t]), "host")):
            _same_as(got, want_pos, (tag, t))
            _same_taps(mt, ref, 1, (tag, t))
            _check_want(mt, got, want[t], (tag, t))
    # the state behind the last frame: the grey of the last demosaiced frame
    _check_last_grey(dev, host, 0, D.grey_of(rc.bgr[-1][0]), rc.c.diff_threshold)


def test_three_streams_three_patterns_and_a_roi_set_and_removed(A):
    """... and the swapped assignment of the patterns gives other planes: the pattern table is per stream"""
    for rows, cols in ((90, 200), (37, 91)):                    # wide and narrow
        rc, want = T.diff_want(rows, cols, T.THREE, roi=True)
        raw, ref, swapped = _tracker(A, rc, bayer=list(T.THREE)), _tracker(A, rc), _tracker(A, rc, bayer=list(T.THREE_SWAPPED))
        on, differs, with_roi = False, 0, 0
        for t in range(len(rc.raw)):
            on = _roi_to((raw, ref, swapped), rc.c, t, on)
            with_roi += on
            bgr, rw = _dev(rc.bgr[t]), _dev(rc.raw[t])
            want_pos = ref.track_dev(bgr.data_ptr())
            got = raw.track_dev(rw.data_ptr())
            _same_as(got, want_pos, (rows, t))
            _same_taps(raw, ref, 3, (rows, t))
            _check_want(raw, got, want[t], (rows, t))
            swapped.track_dev(rw.data_ptr())
            differs += [(swapped.read_mask(THR, s) != raw.read_mask(THR, s)).any() for s in range(3)] == [True, True, False]
        assert 0 < with_roi < len(rc.raw)
        assert differs >= len(rc.raw) // 2                       # streams 0 and 1 differ, stream 2 (the same pattern) never


@pytest.mark.parametrize("rows,cols", [(33, 128), (90, 200)])
def test_a_device_pointer_one_byte_off_takes_the_narrow_form(A, rows, cols):
    import torch
    rc, want = T.diff_want(rows, cols, T.THREE)
    raw, ref = _tracker(A, rc, bayer=list(T.THREE)), _tracker(A, rc)
    size = 3 * rows * cols
    store = torch.zeros(size + 8, dtype=torch.uint8, device="cuda")
    view = store[1:1 + size]
    assert view.data_ptr() % 4 == 1
    for t in range(6):
        view.copy_(torch.from_numpy(np.stack(rc.raw[t]).reshape(-1)))
        bgr = _dev(rc.bgr[t])
        want_pos = ref.track_dev(bgr.data_ptr())
        got = raw.track_dev(view.data_ptr())
        _same_as(got, want_pos, t)
        _same_taps(raw, ref, 3, t)
        _check_want(raw, got, want[t], t)


def test_sixty_six_streams_cross_the_launch_split(A):
    """6 x 8 frames; the streams behind the split carry other patterns than the streams their parity bits would alias"""
    pats = tuple(R.PATTERNS[(s + s // 64) % 4] for s in range(66))
    assert pats[64] != pats[0] and pats[65] != pats[1]
    rc, want = T.diff_want(6, 8, pats, n_frames=5)
    raw, ref = _tracker(A, rc, bayer=list(pats)), _tracker(A, rc)
    bufs = [_dev(fs) for fs in rc.raw]
    for t in range(3):
        bgr = _dev(rc.bgr[t])
        want_pos = ref.track_dev(bgr.data_ptr())
        got = raw.track_dev(bufs[t].data_ptr())
        _same_as(got, want_pos, t)
        _same_taps(raw, ref, 66, t)
        _check_want(raw, got, want[t], t)
    got = raw.track_sequence_dev([bufs[3].data_ptr(), bufs[4].data_ptr()])              # ... and a paired launch across it
    for i, t in enumerate((3, 4)):
        bgr = _dev(rc.bgr[t])
        _same_as(got[i], ref.track_dev(bgr.data_ptr()), ("pair", t))
    _same_taps(raw, ref, 66, "pair")
    _check_want(raw, got[1], want[4], "pair")


# ----------------------------------------------------------------------------------------------- the sequence call ----

@pytest.mark.parametrize("rows,cols", [(90, 200), (37, 91), (12, 1040), (5, 4)])
def test_sequence_with_paired_launches_and_a_first_frame_inside(A, rows, cols):
    """A fresh sequence (a lone first frame, then pairs), a sequence from a mixed state after reset(1) (single launches until
    every stream has a last image), a synchronous step behind it: the BGR tracker takes the same frames in synchronous steps."""
    rc, want = T.diff_want(rows, cols, T.THREE, roi=True)
    raw, ref = _tracker(A, rc, bayer=list(T.THREE)), _tracker(A, rc)
    for mt in (raw, ref):                                       # (one ROI on stream 1 for the whole run)
        mt.set_roi_mask(rc.c.roi, stream=rc.c.roi_stream)
    bufs = [_dev(fs) for fs in rc.raw]
    bgrs = [_dev(fs) for fs in rc.bgr]

    def run(ts, tag):
        got = raw.track_sequence_dev([bufs[t].data_ptr() for t in ts])
        for i, t in enumerate(ts):
            _same_as(got[i], ref.track_dev(bgrs[t].data_ptr()), (tag, t))
        _same_taps(raw, ref, 3, tag)

    run([0, 1, 2, 3, 4, 5], "fresh")
    for mt in (raw, ref):
        mt.reset(1)
    run([6, 7, 8, 9, 10], "after reset(1)")
    _same_as(raw.track_dev(bufs[11].data_ptr()), ref.track_dev(bgrs[11].data_ptr()), "next")
    _same_taps(raw, ref, 3, "next")


def test_a_sequence_equals_the_oracle(A):
    rc, want = T.diff_want(90, 200, T.THREE)
    raw = _tracker(A, rc, bayer=list(T.THREE))
    bufs = [_dev(fs) for fs in rc.raw]
    got = raw.track_sequence_dev([b.data_ptr() for b in bufs])
    for t in range(len(bufs)):
        for s in range(3):
            _same_detection(got[t][s], want[t][s][0], (t, s))
    _check_want(raw, got[-1], want[-1], "last")


# -------------------------------------------------------------------------------------------------------- state ----

def test_raw_steps_bgr_steps_and_detect_diff_continue_one_stream(A):
    """RAW8 steps (switch on), BGR steps (switch off) and oatgpu_detect_diff on grey frames in turn: every stream equals a
    reference that saw the demosaiced (or grey) frames one after the other -- the state lives in the demosaiced domain."""
    from oat_amd import ffi
    rc, _ = T.diff_want(90, 200, T.THREE)
    c = rc.c
    mt, ref = _tracker(A, rc), _tracker(A, rc)
    refs = [T.DiffRef(c) for _ in range(3)]
    for t in range(len(rc.raw)):
        bgr = _dev(rc.bgr[t])
        kind = ("raw", "bgr", "single")[t % 3]
        if kind == "single":
            for s in range(3):
                g, p, q = D.grey_of(rc.bgr[t][s]), ffi.Position(), ffi.Position()
                mt._chk(mt.lib.oatgpu_detect_diff(mt.ctx, s, ffi.u8(g), C.byref(p)))
                ref._chk(ref.lib.oatgpu_detect_diff(ref.ctx, s, ffi.u8(g), C.byref(q)))
                _same_detection(A.Position2D.from_c(p), refs[s].step(g)[0], (t, s))
            continue
        want_pos = ref.track_dev(bgr.data_ptr())
        if kind == "raw":
            mt.bayer(list(T.THREE))
            buf = _dev(rc.raw[t])
            got = mt.track_dev(buf.data_ptr())
            mt.bayer(None)
        else:
            got = mt.track_dev(bgr.data_ptr())
        _same_as(got, want_pos, (kind, t))
        _same_taps(mt, ref, 3, (kind, t))
        _check_want(mt, got, [refs[s].step(rc.bgr[t][s]) for s in range(3)], (kind, t))


# ------------------------------------------------------------------------------------ refusals, the context's other calls ----

def _both(A, c):
    """A context with the fused tracker's detector AND the motion tracker (MotionTracker's methods serve any context)."""
    hp = A.HotPath(c.rows, c.cols, n_streams=c.n_streams, adaptation_coeff=0.01, erode=0, dilate=3, area=D.AREA,
                   diff_threshold=c.diff_threshold, blur=c.blur, h_thresh=(0, 256), s_thresh=(0, 256), v_thresh=(60, 256))
    hp._chk(hp.lib.oatgpu_set_diff_tracker(hp.ctx, 1))
    return hp


def _switch(hp, patterns):
    arr = (C.c_int32 * max(len(patterns), 1))(*patterns)
    return hp.lib.oatgpu_set_tracker_bayer(hp.ctx, arr if patterns else None, len(patterns))


def test_refusals_leave_the_context_usable_and_unchanged(A):
    rc, want = T.diff_want(90, 200, T.THREE)
    c, n = rc.c, 3
    hp = _both(A, c)
    lib, ctx = hp.lib, hp.ctx
    rd = lambda which, s: A.MotionTracker.read_mask(hp, which, s)          # noqa: E731
    bufs = [_dev(fs) for fs in rc.raw]
    bgrs = [_dev(fs) for fs in rc.bgr]

    def refused(patterns, *needles):
        assert _switch(hp, patterns) == E_INVALID
        msg = lib.oatgpu_last_error(ctx).decode()
        assert any(k in msg for k in needles), msg

    # the switch is off and stays off through every refusal: a BGR step is the oracle's
    refused([0], "Bayer pattern 0")
    refused([1, 2, 5], "Bayer pattern 5")
    refused([1, 2], "2 Bayer patterns for 3 streams")
    refused([1, 2, 3, 4], "4 Bayer patterns for 3 streams")
    hp.enqueue_dev(bgrs[0].data_ptr(), keepalive=bgrs[0])
    refused([1], "outstanding")
    hp.collect()
    hp.stage(0, rc.bgr[0][0])
    refused([1], "staged")
    hp.stage_abort()
    got = A.MotionTracker.track_dev(hp, bgrs[0].data_ptr())
    _check_want(hp, got, want[0], "bgr after refusals", read=rd)
    # the switch is on and stays as it was through every refusal: the next RAW8 step is the oracle's
    assert _switch(hp, list(T.THREE)) == 0
    refused([7], "Bayer pattern 7")
    refused([1, 2], "2 Bayer patterns")
    got = A.MotionTracker.track_dev(hp, bufs[1].data_ptr())
    _check_want(hp, got, want[1], "raw after refusals", read=rd)
    # oatgpu_set_track_bayer is another switch: while it is on the diff calls are refused as before
    from oat_amd import ffi
    out = (ffi.Position * n)()
    hp.bayer("RGGB")
    assert lib.oatgpu_diff_batch_dev(ctx, C.c_void_p(bufs[2].data_ptr()), out) == E_INVALID
    assert "oatgpu_set_track_bayer" in lib.oatgpu_last_error(ctx).decode()
    hp.bayer(None)
    hp.set_kalman(True)
    assert lib.oatgpu_diff_batch_dev(ctx, C.c_void_p(bufs[2].data_ptr()), out) == E_INVALID
    assert "oatgpu_set_kalman" in lib.oatgpu_last_error(ctx).decode()
    hp.set_kalman(False)
    got = A.MotionTracker.track_dev(hp, bufs[2].data_ptr())
    _check_want(hp, got, want[2], "raw after the other switch", read=rd)
    assert _switch(hp, []) == 0
    got = A.MotionTracker.track_dev(hp, bgrs[3].data_ptr())
    _check_want(hp, got, want[3], "bgr again", read=rd)


def test_contexts_that_cannot_take_raw_frames(A):
    grey = A.MotionTracker(37, 91, n_streams=1, channels=1, diff_threshold=12, blur=2, area=D.AREA)
    assert _switch(grey, [1]) == E_INVALID and "channels = 3" in grey.lib.oatgpu_last_error(grey.ctx).decode()
    g = D.make_case("grey", 37, 91, 1, 1, seed=3)
    first = grey.track(g.frames[0])                              # ... and goes on as a GREY tracker
    assert first[0].position_valid == D.Model(12, 2).detect(g.frames[0][0])[0]["valid"]
    with pytest.raises(A.OatGpuError, match="3 x 3"):
        A.MotionTracker(2, 8, n_streams=1, channels=3, bayer="RGGB")
    with pytest.raises(A.OatGpuError, match="3 x 3"):
        A.MotionTracker(8, 2, n_streams=1, channels=3, bayer="RGGB")
    with pytest.raises(ValueError):
        A.MotionTracker(8, 8, bayer="RGBG")


def test_the_contexts_other_calls_work_beside_the_switch(A):
    """A fused track_batch on BGR frames and oatgpu_debayer_dev on a context whose motion tracker takes RAW8"""
    import oracle_lib as O
    import torch
    rc, want = T.diff_want(90, 200, T.THREE)
    c, n = rc.c, 3
    hp = _both(A, c)
    assert _switch(hp, list(T.THREE)) == 0
    rd = lambda which, s: A.MotionTracker.read_mask(hp, which, s)          # noqa: E731
    p = O.hsv_params(h_lo=0, h_hi=256, s_lo=0, s_hi=256, v_lo=60, v_hi=256, erode=0, dilate=3, min_area=D.AREA[0], max_area=D.AREA[1])
    mogs = [O.Mog2(c.rows, c.cols, 3) for _ in range(n)]
    out = torch.zeros(n * c.rows * c.cols * 3, dtype=torch.uint8, device="cuda")
    for t in range(4):
        raw = _dev(rc.raw[t])
        got = A.MotionTracker.track_dev(hp, raw.data_ptr())
        _check_want(hp, got, want[t], ("raw", t), read=rd)
        pos = hp.track(rc.bgr[t])                               # the fused tracker still takes BGR
        for s in range(n):
            w, mask = O.chain_step(mogs[s], rc.bgr[t][s], 0.01, p)
            _same_detection(pos[s], w, ("track", t, s))
            assert (hp.read_mask(MORPH, s) == mask).all(), ("track", t, s)
        A.Debayer.filter_dev(hp, raw.data_ptr(), out.data_ptr(), list(T.THREE))
        hp.synchronize()
        assert np.array_equal(out.cpu().numpy().reshape(n, c.rows, c.cols, 3), np.stack(rc.bgr[t])), t
