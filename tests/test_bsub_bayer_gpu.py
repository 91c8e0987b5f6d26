"""GPU tests of the subtraction tracker on Bayer RAW8 frames (oatgpu_set_tracker_bayer; SubtractionTracker.bayer;
k_bsubtrack_raw_wide / k_bsubtrack_raw_narrow).  The reference for a RAW8 run is the BGR tracker fed
debayer_ref.demosaic(raw, pattern) -- positions field for field, every tap and the state (background bytes, accumulator bit
patterns) byte for byte --, and beside it bsub_cases.Ref (the oracle chain with the numpy model) on the same demosaiced frames
(tests/tracker_bayer_cases.py; tests/test_tracker_bayer_cpu.py holds that case list to non-vacuity and to the planted wrong
front ends).  Every comparison is bit for bit.  Every frame is under 0.1 MP."""
import ctypes as C

import numpy as np
import pytest

import bsub_cases as B
import debayer_ref as R
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
    st = A.SubtractionTracker(rc.c.rows, rc.c.cols, bayer=bayer, **rc.c.tracker_args())
    for s, img in rc.c.background.items():                      # (a BGR image, whatever the track calls take)
        st.set_background(img, stream=s)
    return st


def _taps(st, s, read=None):
    read = read or st.read_mask
    return [read(w, s) for w in (THR, MORPH, FIN)]


def _same_as(got, ref, tag):
    """positions of a RAW8 step against the BGR tracker's on the demosaiced frames: every field"""
    for s, (g, r) in enumerate(zip(got, ref)):
        for f in FIELDS:
            a, b = getattr(g, f), getattr(r, f)
            assert a == b or (a != a and b != b), (tag, s, f, a, b)


def _same_taps(st, ref, n, tag):
    for s in range(n):
        for p, q in zip(_taps(st, s), _taps(ref, s)):
            assert p.tobytes() == q.tobytes(), (tag, s)


def _same_state(st, ref, n, tag, acc=True):
    for s in range(n):
        (bg1, acc1), (bg2, acc2) = st.state(s, acc=acc), ref.state(s, acc=acc)
        assert bg1.tobytes() == bg2.tobytes(), ("background", tag, s)
        assert not acc or acc1.tobytes() == acc2.tobytes(), ("accumulator", tag, s)


def _check_want(st, got, want_t, tag, read=None):
    """... and against the oracle chain and the numpy model"""
    for s, (det, bits, omorph, _, _) in enumerate(want_t):
        _same_detection(got[s], det, (tag, s))
        thr, morph, fin = _taps(st, s, read)
        assert ((thr > 0) == bits).all(), ("threshold tap", tag, s)
        assert ((morph > 0) == omorph).all(), ("morph tap", tag, s)
        ring = np.ones(fin.shape, bool)
        ring[1:-1, 1:-1] = False
        assert (fin[1:-1, 1:-1] == morph[1:-1, 1:-1]).all() and not fin[ring].any(), ("final tap", tag, s)


def _check_state(st, want_t, tag):
    """oatgpu_bsub_get_state against the model: the background bytes and the accumulator's bit patterns"""
    for s, w in enumerate(want_t):
        bg, acc = st.state(s, acc=w[4] is not None)
        assert bg.tobytes() == w[3].tobytes(), ("background", tag, s, int((bg != w[3]).sum()))
        if w[4] is not None:
            assert acc.tobytes() == w[4].tobytes(), ("accumulator", tag, s)


def _roi_to(trackers, c, t, on):
    now = c.roi_at(t, c.roi_stream) is not None
    if now != on:
        for st in trackers:
            st.set_roi_mask(c.roi if now else None, stream=c.roi_stream)
    return now


# ------------------------------------------------------------------------------------------ the synchronous step ----

@pytest.mark.parametrize("alpha", [0.0, 0.05])
@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("rows,cols", T.GEOMETRIES)
def test_every_geometry_and_pattern_on_device_and_host_frames(A, rows, cols, pattern, alpha):
    rc, want = T.bsub_want(rows, cols, (pattern,), alpha=alpha)
    dev, host, ref = _tracker(A, rc, bayer=R.NAMES[pattern]), _tracker(A, rc, bayer=pattern), _tracker(A, rc)
    assert dev.frame_shape == (rows, cols) and ref.frame_shape == (rows, cols, 3)
    for t in range(len(rc.raw)):
        bgr, raw = _dev(rc.bgr[t]), _dev(rc.raw[t])
        want_pos = ref.track_dev(bgr.data_ptr())
        for st, got, tag in ((dev, dev.track_dev(raw.data_ptr()), "dev"), (host, host.track(rc.raw[t]), "host")):
            _same_as(got, want_pos, (tag, t))
            _same_taps(st, ref, 1, (tag, t))
            _check_want(st, got, want[t], (tag, t))
    for st, tag in ((dev, "dev"), (host, "host")):
        _same_state(st, ref, 1, tag)
        _check_state(st, want[-1], tag)


@pytest.mark.parametrize("rows,cols", [(90, 200), (37, 91), (4, 8)])
def test_alpha_one_leaves_the_models_state(A, rows, cols):
    rc, want = T.bsub_want(rows, cols, (R.GBRG,), alpha=1.0)
    raw, ref = _tracker(A, rc, bayer="GBRG"), _tracker(A, rc)
    for t in range(len(rc.raw)):
        bgr, rw = _dev(rc.bgr[t]), _dev(rc.raw[t])
        want_pos = ref.track_dev(bgr.data_ptr())
        got = raw.track_dev(rw.data_ptr())
        _same_as(got, want_pos, t)
        _check_want(raw, got, want[t], t)
    _same_state(raw, ref, 1, "alpha 1")
    _check_state(raw, want[-1], "alpha 1")


@pytest.mark.parametrize("alpha", [0.0, 0.05])
def test_three_streams_three_patterns_and_a_roi_set_and_removed(A, alpha):
    """... and the swapped assignment of the patterns gives another state: the pattern table is per stream"""
    for rows, cols in ((90, 200), (37, 91)):                    # wide and narrow
        rc, want = T.bsub_want(rows, cols, T.THREE, alpha=alpha, roi=True)
        raw, ref, swapped = _tracker(A, rc, bayer=list(T.THREE)), _tracker(A, rc), _tracker(A, rc, bayer=list(T.THREE_SWAPPED))
        on, with_roi = False, 0
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
        assert 0 < with_roi < len(rc.raw)
        _same_state(raw, ref, 3, rows)
        _check_state(raw, want[-1], rows)
        other = [swapped.state(s)[0].tobytes() != raw.state(s)[0].tobytes() for s in range(3)]
        assert other == [True, True, False]                     # streams 0 and 1 differ, stream 2 (the same pattern) does not


@pytest.mark.parametrize("alpha", [0.0, 0.05])
@pytest.mark.parametrize("rows,cols", [(33, 128), (90, 200)])
def test_a_device_pointer_one_byte_off_takes_the_narrow_form(A, rows, cols, alpha):
    import torch
    rc, want = T.bsub_want(rows, cols, T.THREE, alpha=alpha)
    raw, ref = _tracker(A, rc, bayer=list(T.THREE)), _tracker(A, rc)
    size = 3 * rows * cols
    store = torch.zeros(size + 8, dtype=torch.uint8, device="cuda")
    view = store[1:1 + size]
    assert view.data_ptr() % 4 == 1
    for t in range(5):
        view.copy_(torch.from_numpy(np.stack(rc.raw[t]).reshape(-1)))
        bgr = _dev(rc.bgr[t])
        want_pos = ref.track_dev(bgr.data_ptr())
        got = raw.track_dev(view.data_ptr())
        _same_as(got, want_pos, t)
        _same_taps(raw, ref, 3, t)
        _check_want(raw, got, want[t], t)
    _same_state(raw, ref, 3, "offset 1")
    _check_state(raw, want[4], "offset 1")


def test_sixty_six_streams_cross_the_launch_split(A):
    """6 x 8 frames; the streams behind the split carry other patterns than the streams their parity bits would alias"""
    pats = tuple(R.PATTERNS[(s + s // 64) % 4] for s in range(66))
    assert pats[64] != pats[0] and pats[65] != pats[1]
    rc, want = T.bsub_want(6, 8, pats, n_frames=5)
    raw, ref = _tracker(A, rc, bayer=list(pats)), _tracker(A, rc)
    bufs = [_dev(fs) for fs in rc.raw]
    for t in range(3):
        bgr = _dev(rc.bgr[t])
        want_pos = ref.track_dev(bgr.data_ptr())
        _same_as(raw.track_dev(bufs[t].data_ptr()), want_pos, t)
        _same_taps(raw, ref, 66, t)
    got = raw.track_sequence_dev([bufs[3].data_ptr(), bufs[4].data_ptr()])              # ... and a paired launch across it
    for i, t in enumerate((3, 4)):
        bgr = _dev(rc.bgr[t])
        _same_as(got[i], ref.track_dev(bgr.data_ptr()), ("pair", t))
    _same_taps(raw, ref, 66, "pair")
    _same_state(raw, ref, 66, "pair")
    _check_state(raw, want[4], "pair")


# ----------------------------------------------------------------------------------------------- the sequence call ----

@pytest.mark.parametrize("alpha", [0.0, 0.05])
@pytest.mark.parametrize("rows,cols", [(90, 200), (37, 91), (12, 1040), (5, 4)])
def test_sequence_with_paired_launches_and_a_first_frame_inside(A, rows, cols, alpha):
    """A fresh sequence (the first frame is the first of a pair), a sequence from a mixed state after reset(1) (stream 1's first
    frame inside a pair), a synchronous step behind it: the BGR tracker takes the same frames in synchronous steps."""
    rc, want = T.bsub_want(rows, cols, T.THREE, alpha=alpha, roi=True, n_frames=12)
    raw, ref = _tracker(A, rc, bayer=list(T.THREE)), _tracker(A, rc)
    for st in (raw, ref):                                       # (one ROI on stream 1 for the whole run)
        st.set_roi_mask(rc.c.roi, stream=rc.c.roi_stream)
    bufs = [_dev(fs) for fs in rc.raw]
    bgrs = [_dev(fs) for fs in rc.bgr]

    def run(ts, tag):
        got = raw.track_sequence_dev([bufs[t].data_ptr() for t in ts])
        for i, t in enumerate(ts):
            _same_as(got[i], ref.track_dev(bgrs[t].data_ptr()), (tag, t))
        _same_taps(raw, ref, 3, tag)
        _same_state(raw, ref, 3, tag)

    run([0, 1, 2, 3, 4, 5], "fresh")
    for st in (raw, ref):
        st.reset(1)
    run([6, 7, 8, 9, 10], "after reset(1)")
    _same_as(raw.track_dev(bufs[11].data_ptr()), ref.track_dev(bgrs[11].data_ptr()), "next")
    _same_taps(raw, ref, 3, "next")
    _same_state(raw, ref, 3, "next")


@pytest.mark.parametrize("alpha", [0.0, 0.05])
def test_a_sequence_equals_the_oracle(A, alpha):
    rc, want = T.bsub_want(90, 200, T.THREE, alpha=alpha)
    raw = _tracker(A, rc, bayer=list(T.THREE))
    bufs = [_dev(fs) for fs in rc.raw]
    got = raw.track_sequence_dev([b.data_ptr() for b in bufs])
    for t in range(len(bufs)):
        for s in range(3):
            _same_detection(got[t][s], want[t][s][0], (t, s))
    _check_want(raw, got[-1], want[-1], "last")
    _check_state(raw, want[-1], "last")


# -------------------------------------------------------------------------------------------------------- state ----

@pytest.mark.parametrize("alpha", [0.0, 0.05])
def test_raw_steps_bgr_steps_and_bsub_filter_continue_one_stream(A, alpha):
    """RAW8 steps (switch on), BGR steps (switch off) and oatgpu_bsub_filter on BGR frames in turn: every stream equals a
    reference that saw the demosaiced frames one after the other -- the state lives in the demosaiced domain."""
    from oat_amd import ffi
    rc, want = T.bsub_want(90, 200, T.THREE, alpha=alpha)
    st, ref = _tracker(A, rc), _tracker(A, rc)
    for t in range(len(rc.raw)):
        bgr = _dev(rc.bgr[t])
        kind = ("raw", "bgr", "single")[t % 3]
        if kind == "single":
            for s in range(3):
                a, b = np.empty(rc.c.shape, np.uint8), np.empty(rc.c.shape, np.uint8)
                st._chk(st.lib.oatgpu_bsub_filter(st.ctx, s, ffi.u8(rc.bgr[t][s]), ffi.u8(a), alpha))
                ref._chk(ref.lib.oatgpu_bsub_filter(ref.ctx, s, ffi.u8(rc.bgr[t][s]), ffi.u8(b), alpha))
                assert a.tobytes() == b.tobytes(), (t, s)
        else:
            want_pos = ref.track_dev(bgr.data_ptr())
            if kind == "raw":
                st.bayer(list(T.THREE))
                buf = _dev(rc.raw[t])
                got = st.track_dev(buf.data_ptr())
                st.bayer(None)
            else:
                got = st.track_dev(bgr.data_ptr())
            _same_as(got, want_pos, (kind, t))
            _same_taps(st, ref, 3, (kind, t))
            _check_want(st, got, want[t], (kind, t))
        _same_state(st, ref, 3, (kind, t))
        _check_state(st, want[t], (kind, t))


def test_a_background_from_a_file_stays_bgr(A):
    """oatgpu_bsub_set_background takes a BGR image while the switch is on (streams 0 and 2; stream 1 makes its own)"""
    rc, want = T.bsub_want(48, 64, T.THREE, alpha=0.0, background=True)
    assert sorted(rc.c.background) == [0, 2]
    raw, ref = _tracker(A, rc, bayer=list(T.THREE)), _tracker(A, rc)
    hits = 0
    for t in range(len(rc.raw)):
        bgr, rw = _dev(rc.bgr[t]), _dev(rc.raw[t])
        want_pos = ref.track_dev(bgr.data_ptr())
        got = raw.track_dev(rw.data_ptr())
        _same_as(got, want_pos, t)
        _same_taps(raw, ref, 3, t)
        _check_want(raw, got, want[t], t)
        hits += sum(w[0]["valid"] for w in want[t])
    assert hits >= len(rc.raw)
    for s in range(3):
        bg, _ = raw.state(s, acc=False)
        assert bg.tobytes() == want[-1][s][3].tobytes(), s
    with pytest.raises(A.OatGpuError, match="no accumulator"):
        raw.state(0)


# ------------------------------------------------------------------------------------ refusals, the context's other calls ----

def _both(A, c):
    """A context with the fused tracker's detector AND the subtraction tracker (SubtractionTracker's methods serve any context)."""
    kw = c.tracker_args()
    kw.pop("channels"), kw.pop("alpha")
    hp = A.HotPath(c.rows, c.cols, adaptation_coeff=0.01, **kw)
    hp._chk(hp.lib.oatgpu_set_bsub_tracker(hp.ctx, 1))
    return hp


def _switch(hp, patterns):
    arr = (C.c_int32 * max(len(patterns), 1))(*patterns)
    return hp.lib.oatgpu_set_tracker_bayer(hp.ctx, arr if patterns else None, len(patterns))


def test_refusals_and_the_contexts_other_calls(A):
    """The setter's refusals leave the switch as it was; oatgpu_set_track_bayer still refuses the bsub calls; a fused
    track_batch on BGR frames and oatgpu_debayer_dev work beside the switch."""
    import oracle_lib as O
    import torch
    from oat_amd import ffi
    rc, want = T.bsub_want(90, 200, T.THREE)
    c, n, alpha = rc.c, 3, rc.c.alpha
    hp = _both(A, c)
    lib, ctx = hp.lib, hp.ctx
    rd = lambda which, s: A.SubtractionTracker.read_mask(hp, which, s)     # noqa: E731
    track = lambda buf: A.SubtractionTracker.track_dev(hp, buf.data_ptr(), alpha=alpha)     # noqa: E731
    bufs = [_dev(fs) for fs in rc.raw]
    bgrs = [_dev(fs) for fs in rc.bgr]
    out = (ffi.Position * n)()

    def refused(patterns, *needles):
        assert _switch(hp, patterns) == E_INVALID
        msg = lib.oatgpu_last_error(ctx).decode()
        assert any(k in msg for k in needles), msg

    refused([0], "Bayer pattern 0")
    refused([1, 2], "2 Bayer patterns for 3 streams")
    hp.enqueue_dev(bgrs[0].data_ptr(), keepalive=bgrs[0])
    refused([1], "outstanding")
    hp.collect()
    hp.stage(0, rc.bgr[0][0])
    refused([1], "staged")
    hp.stage_abort()
    _check_want(hp, track(bgrs[0]), want[0], "bgr after refusals", read=rd)
    assert _switch(hp, list(T.THREE)) == 0
    refused([5], "Bayer pattern 5")
    refused([1, 2, 3, 4], "4 Bayer patterns")
    _check_want(hp, track(bufs[1]), want[1], "raw after refusals", read=rd)
    hp.bayer("RGGB")                                            # the fused tracker's switch: another one
    assert lib.oatgpu_bsub_track_batch_dev(ctx, C.c_void_p(bufs[2].data_ptr()), alpha, out) == E_INVALID
    assert "oatgpu_set_track_bayer" in lib.oatgpu_last_error(ctx).decode()
    hp.bayer(None)
    hp.set_homography([1, 0, 2, 0, 1, 3, 0, 0, 1])
    assert lib.oatgpu_bsub_track_batch_dev(ctx, C.c_void_p(bufs[2].data_ptr()), alpha, out) == E_INVALID
    assert "oatgpu_set_homography" in lib.oatgpu_last_error(ctx).decode()
    hp.set_homography(None)
    _check_want(hp, track(bufs[2]), want[2], "raw after the other switch", read=rd)
    # beside the switch
    w = B.HSV_WIN
    p = O.hsv_params(h_lo=w["h"][0], h_hi=w["h"][1], s_lo=w["s"][0], s_hi=w["s"][1], v_lo=w["v"][0], v_hi=w["v"][1], erode=c.erode,
                     dilate=c.dilate, min_area=B.AREA[0], max_area=B.AREA[1])
    mogs = [O.Mog2(c.rows, c.cols, 3) for _ in range(n)]
    for s in range(n):                                          # (the enqueued frame 0 above moved the model)
        O.chain_step(mogs[s], rc.bgr[0][s], 0.01, p)
    pos = hp.track(rc.bgr[3])
    for s in range(n):
        wnt, mask = O.chain_step(mogs[s], rc.bgr[3][s], 0.01, p)
        _same_detection(pos[s], wnt, ("track", s))
        assert (hp.read_mask(MORPH, s) == mask).all(), ("track", s)
    bgr_out = torch.zeros(n * c.rows * c.cols * 3, dtype=torch.uint8, device="cuda")
    A.Debayer.filter_dev(hp, bufs[3].data_ptr(), bgr_out.data_ptr(), list(T.THREE))
    hp.synchronize()
    assert np.array_equal(bgr_out.cpu().numpy().reshape(n, c.rows, c.cols, 3), np.stack(rc.bgr[3]))
    _check_want(hp, track(bufs[3]), want[3], "raw behind the other calls", read=rd)
    assert _switch(hp, []) == 0
    _check_want(hp, track(bgrs[4]), want[4], "bgr again", read=rd)
    for s in range(n):
        bg, acc = A.SubtractionTracker.state(hp, s)
        assert bg.tobytes() == want[4][s][3].tobytes() and acc.tobytes() == want[4][s][4].tobytes(), s
