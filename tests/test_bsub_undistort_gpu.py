"""GPU tests of the subtraction tracker with lens undistortion inside its front kernel (oatgpu_set_tracker_undistort;
SubtractionTracker.undistort; k_bsubtrack_remap_wide / k_bsubtrack_remap_narrow).  The reference for a run with the
switch on is the packed tracker fed undistort_ref.remap(frame, the stream's map) -- positions field for field, every tap and
the state (background bytes, accumulator bit patterns) byte for byte --, and beside it bsub_cases.Ref (the oracle chain with the
numpy model) on the same undistorted frames (tests/tracker_undistort_cases.py; tests/test_tracker_undistort_cpu.py holds that case
list to non-vacuity and to the planted wrong front ends).  Every comparison is bit for bit.  Every frame is under 0.1 MP.

The lane mapping under the switch follows the frame width alone (W % 4 == 0: wide): the frames are gathered with unaligned
loads, the background and the accumulator are the context's own, aligned allocations, so the geometry list is what selects the
mapping -- the narrow one at (37, 91) and (3, 3), the wide one at the seven others -- and a frame pointer one byte off must change
nothing."""
import ctypes as C

import numpy as np
import pytest

import bsub_cases as B
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


def _calibrate(st, uc, cals=None):
    for s, k in enumerate(cals or uc.cals):
        st.set_undistort(s, *T.calibration(uc.c.rows, uc.c.cols, k))


def _tracker(A, uc, on=False, cals=None):
    st = A.SubtractionTracker(uc.c.rows, uc.c.cols, **uc.c.tracker_args())
    for s, img in uc.c.background.items():                      # (an image in undistorted coordinates, switch or none)
        st.set_background(img, stream=s)
    if on:
        _calibrate(st, uc, cals)
        st.undistort(True)
    return st


def _taps(st, s, read=None):
    read = read or st.read_mask
    return [read(w, s) for w in (THR, MORPH, FIN)]


def _same_as(got, ref, tag):
    """positions of a step with the switch on against the packed tracker's on the undistorted frames: every field"""
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

@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("alpha", [0.0, 0.05])
@pytest.mark.parametrize("cal", T.CALS)
@pytest.mark.parametrize("rows,cols", T.GEOMETRIES)
def test_every_geometry_and_calibration_on_device_and_host_frames(A, rows, cols, cal, alpha, channels):
    uc, want = T.bsub_want(rows, cols, channels, (cal,), alpha=alpha)
    dev, ref = _tracker(A, uc, on=True), _tracker(A, uc)
    host = A.SubtractionTracker(rows, cols, undistort=uc.calibration(0), **uc.c.tracker_args())     # (the constructor's keyword)
    for t in range(len(uc.given)):
        und, given = _dev(uc.und[t]), _dev(uc.given[t])
        want_pos = ref.track_dev(und.data_ptr())
        for st, got, tag in ((dev, dev.track_dev(given.data_ptr()), "dev"), (host, host.track(uc.given[t]), "host")):
            _same_as(got, want_pos, (tag, t))
            _same_taps(st, ref, 1, (tag, t))
            _check_want(st, got, want[t], (tag, t))
    for st, tag in ((dev, "dev"), (host, "host")):
        _same_state(st, ref, 1, tag)
        _check_state(st, want[-1], tag)


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("rows,cols", [(90, 200), (37, 91), (4, 8)])
def test_alpha_one_leaves_the_models_state(A, rows, cols, channels):
    uc, want = T.bsub_want(rows, cols, channels, ("pincushion",), alpha=1.0)
    und, ref = _tracker(A, uc, on=True), _tracker(A, uc)
    for t in range(len(uc.given)):
        u, g = _dev(uc.und[t]), _dev(uc.given[t])
        want_pos = ref.track_dev(u.data_ptr())
        got = und.track_dev(g.data_ptr())
        _same_as(got, want_pos, t)
        _check_want(und, got, want[t], t)
    _same_state(und, ref, 1, "alpha 1")
    _check_state(und, want[-1], "alpha 1")


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("alpha", [0.0, 0.05])
@pytest.mark.parametrize("rows,cols", [(90, 200), (37, 91)])      # wide and narrow
def test_three_streams_three_calibrations_and_a_roi_set_and_removed(A, rows, cols, alpha, channels):
    """... and the swapped assignment of the calibrations gives another state: the map is per stream"""
    uc, want = T.bsub_want(rows, cols, channels, T.THREE, alpha=alpha, roi=True)
    und, ref, swapped = _tracker(A, uc, on=True), _tracker(A, uc), _tracker(A, uc, on=True, cals=T.THREE_SWAPPED)
    on, with_roi = False, 0
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
    assert 0 < with_roi < len(uc.given)
    _same_state(und, ref, 3, rows)
    _check_state(und, want[-1], rows)
    other = [swapped.state(s)[0].tobytes() != und.state(s)[0].tobytes() for s in range(3)]
    assert other == [True, True, False]                         # streams 0 and 1 differ, stream 2 (the same calibration) does not


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("alpha", [0.0, 0.05])
@pytest.mark.parametrize("rows,cols", [(33, 128), (90, 200), (37, 91)])
def test_a_device_pointer_one_byte_off(A, rows, cols, alpha, channels):
    import torch
    uc, want = T.bsub_want(rows, cols, channels, T.THREE, alpha=alpha)
    und, ref = _tracker(A, uc, on=True), _tracker(A, uc)
    size = 3 * rows * cols * channels
    store = torch.zeros(size + 8, dtype=torch.uint8, device="cuda")
    view = store[1:1 + size]
    assert view.data_ptr() % 4 == 1
    for t in range(5):
        view.copy_(torch.from_numpy(np.stack(uc.given[t]).reshape(-1)))
        u = _dev(uc.und[t])
        want_pos = ref.track_dev(u.data_ptr())
        got = und.track_dev(view.data_ptr())
        _same_as(got, want_pos, t)
        _same_taps(und, ref, 3, t)
        _check_want(und, got, want[t], t)
    _same_state(und, ref, 3, "offset 1")
    _check_state(und, want[4], "offset 1")
    view.copy_(torch.from_numpy(np.stack(uc.given[6]).reshape(-1)))        # ... and as the second frame of a paired launch
    g5 = _dev(uc.given[5])
    got = und.track_sequence_dev([g5.data_ptr(), view.data_ptr()])
    for i, t in enumerate((5, 6)):
        u = _dev(uc.und[t])
        _same_as(got[i], ref.track_dev(u.data_ptr()), ("pair", t))
    _same_taps(und, ref, 3, "pair")
    _same_state(und, ref, 3, "pair")
    _check_state(und, want[6], "pair")


@pytest.mark.parametrize("channels", [3, 1])
def test_sixty_six_streams_cross_the_launch_split(A, channels):
    """5 x 4 frames; the streams behind the split carry other calibrations than streams 0 and 1"""
    cals = tuple(T.CALS[(s + s // 64) % 3] for s in range(66))
    assert cals[64] != cals[0] and cals[65] != cals[1]
    uc, want = T.bsub_want(5, 4, channels, cals, n_frames=5)
    und, ref = _tracker(A, uc, on=True), _tracker(A, uc)
    bufs = [_dev(fs) for fs in uc.given]
    for t in range(3):
        u = _dev(uc.und[t])
        want_pos = ref.track_dev(u.data_ptr())
        _same_as(und.track_dev(bufs[t].data_ptr()), want_pos, t)
        _same_taps(und, ref, 66, t)
    got = und.track_sequence_dev([bufs[3].data_ptr(), bufs[4].data_ptr()])              # ... and a paired launch across it
    for i, t in enumerate((3, 4)):
        u = _dev(uc.und[t])
        _same_as(got[i], ref.track_dev(u.data_ptr()), ("pair", t))
    _same_taps(und, ref, 66, "pair")
    _same_state(und, ref, 66, "pair")
    _check_state(und, want[4], "pair")


# ----------------------------------------------------------------------------------------------- the sequence call ----

@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("alpha", [0.0, 0.05])
@pytest.mark.parametrize("rows,cols", [(90, 200), (37, 91), (12, 1040), (5, 4)])
def test_sequences_of_even_and_odd_length_with_a_first_frame_inside(A, rows, cols, alpha, channels):
    """A fresh sequence of even length (pairs, the first frame the first of a pair), one of odd length from a mixed state after
    reset(1) (stream 1's first frame inside a pair, a lone launch at the end), a synchronous step behind it: the packed tracker
    takes the undistorted frames in synchronous steps, and a second tracker with the switch on takes the given frames in single
    launches."""
    uc, want = T.bsub_want(rows, cols, channels, T.THREE, alpha=alpha, roi=True, n_frames=12)
    und, single, ref = _tracker(A, uc, on=True), _tracker(A, uc, on=True), _tracker(A, uc)
    for st in (und, single, ref):                               # (one ROI on stream 1 for the whole run)
        st.set_roi_mask(uc.c.roi, stream=uc.c.roi_stream)
    bufs = [_dev(fs) for fs in uc.given]
    unds = [_dev(fs) for fs in uc.und]

    def run(ts, tag):
        got = und.track_sequence_dev([bufs[t].data_ptr() for t in ts])
        for i, t in enumerate(ts):
            want_pos = ref.track_dev(unds[t].data_ptr())
            _same_as(got[i], want_pos, (tag, t))
            _same_as(single.track_dev(bufs[t].data_ptr()), want_pos, (tag, "single", t))
        _same_taps(und, ref, 3, tag)
        _same_state(und, ref, 3, tag)
        _same_state(und, single, 3, (tag, "single"))

    run([0, 1, 2, 3, 4, 5], "fresh, even")
    for st in (und, single, ref):
        st.reset(1)
    run([6, 7, 8, 9, 10], "after reset(1), odd")
    _same_as(und.track_dev(bufs[11].data_ptr()), ref.track_dev(unds[11].data_ptr()), "next")
    _same_taps(und, ref, 3, "next")
    _same_state(und, ref, 3, "next")


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("alpha", [0.0, 0.05, 1.0])
def test_a_sequence_equals_the_oracle(A, alpha, channels):
    uc, want = T.bsub_want(90, 200, channels, T.THREE, alpha=alpha)
    und = _tracker(A, uc, on=True)
    bufs = [_dev(fs) for fs in uc.given]
    got = und.track_sequence_dev([b.data_ptr() for b in bufs])
    for t in range(len(bufs)):
        for s in range(3):
            _same_detection(got[t][s], want[t][s][0], (t, s))
    _check_want(und, got[-1], want[-1], "last")
    _check_state(und, want[-1], "last")


# -------------------------------------------------------------------------------------------------------- state ----

@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("alpha", [0.0, 0.05])
def test_steps_with_the_switch_on_off_and_bsub_filter_continue_one_stream(A, alpha, channels):
    """Steps with the switch on (given frames), off (undistorted frames) and oatgpu_bsub_filter on undistorted frames in turn:
    every stream equals a reference that saw the undistorted frames one after the other -- the state lives in the undistorted
    domain."""
    from oat_amd import ffi
    uc, want = T.bsub_want(90, 200, channels, T.THREE, alpha=alpha)
    st, ref = _tracker(A, uc), _tracker(A, uc)
    _calibrate(st, uc)
    for t in range(len(uc.given)):
        u = _dev(uc.und[t])
        kind = ("on", "off", "single")[t % 3]
        if kind == "single":
            for s in range(3):
                a, b = np.empty(uc.c.shape, np.uint8), np.empty(uc.c.shape, np.uint8)
                st._chk(st.lib.oatgpu_bsub_filter(st.ctx, s, ffi.u8(uc.und[t][s]), ffi.u8(a), alpha))
                ref._chk(ref.lib.oatgpu_bsub_filter(ref.ctx, s, ffi.u8(uc.und[t][s]), ffi.u8(b), alpha))
                assert a.tobytes() == b.tobytes(), (t, s)
        else:
            want_pos = ref.track_dev(u.data_ptr())
            if kind == "on":
                st.undistort(True)
                buf = _dev(uc.given[t])
                got = st.track_dev(buf.data_ptr())
                st.undistort(False)
            else:
                got = st.track_dev(u.data_ptr())
            _same_as(got, want_pos, (kind, t))
            _same_taps(st, ref, 3, (kind, t))
            _check_want(st, got, want[t], (kind, t))
        _same_state(st, ref, 3, (kind, t))
        _check_state(st, want[t], (kind, t))


def test_a_recalibration_between_steps_takes_effect_from_the_next_frame(A):
    import undistort_ref as R
    uc, _ = T.bsub_want(90, 200, 3, T.THREE, alpha=0.05)
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
        _same_state(und, ref, 3, t)
    assert changed == 5


@pytest.mark.parametrize("channels", [3, 1])
def test_a_background_from_a_file_is_an_undistorted_image(A, channels):
    """oatgpu_bsub_set_background takes its image as it is while the switch is on (streams 0 and 2; stream 1 makes its own)"""
    uc, want = T.bsub_want(48, 64, channels, T.THREE, alpha=0.0, background=True)
    assert sorted(uc.c.background) == [0, 2]
    und, ref = _tracker(A, uc, on=True), _tracker(A, uc)
    hits = 0
    for t in range(len(uc.given)):
        u, g = _dev(uc.und[t]), _dev(uc.given[t])
        want_pos = ref.track_dev(u.data_ptr())
        got = und.track_dev(g.data_ptr())
        _same_as(got, want_pos, t)
        _same_taps(und, ref, 3, t)
        _check_want(und, got, want[t], t)
        hits += sum(w[0]["valid"] for w in want[t])
    assert hits >= len(uc.given)
    for s in range(3):
        bg, _ = und.state(s, acc=False)
        assert bg.tobytes() == want[-1][s][3].tobytes(), s
    with pytest.raises(A.OatGpuError, match="no accumulator"):
        und.state(0)


# ------------------------------------------------------------------------------------ refusals, the context's other calls ----

def _both(A, c):
    """A context with the fused tracker's detector AND the subtraction tracker (SubtractionTracker's methods serve any context)."""
    kw = c.tracker_args()
    kw.pop("channels"), kw.pop("alpha")
    hp = A.HotPath(c.rows, c.cols, adaptation_coeff=0.01, **kw)
    hp._chk(hp.lib.oatgpu_set_bsub_tracker(hp.ctx, 1))
    return hp


def test_refusals_and_the_contexts_other_calls(A):
    """The setter's refusals leave the switch and the state as they were; oatgpu_set_track_undistort still refuses the bsub
    calls; a fused track_batch and oatgpu_undistort_dev work beside the switch."""
    import oracle_lib as O
    import torch
    from oat_amd import ffi
    uc, want = T.bsub_want(90, 200, 3, T.THREE)
    _, plain = T.bsub_want(90, 200, 3, T.THREE, plain=True)
    c, n, alpha = uc.c, 3, uc.c.alpha
    hp = _both(A, c)
    lib, ctx = hp.lib, hp.ctx
    rd = lambda which, s: A.SubtractionTracker.read_mask(hp, which, s)     # noqa: E731
    track = lambda buf: A.SubtractionTracker.track_dev(hp, buf.data_ptr(), alpha=alpha)     # noqa: E731
    bufs = [_dev(fs) for fs in uc.given]
    out = (ffi.Position * n)()
    K, Dc = uc.calibration(0)
    Kc, Dd = (C.c_double * 9)(*K), (C.c_double * len(Dc))(*Dc)

    def refused(rc, *needles):
        assert rc == E_INVALID
        msg = lib.oatgpu_last_error(ctx).decode()
        assert all(k in msg for k in needles), msg

    refused(lib.oatgpu_set_tracker_undistort(ctx, 1), "stream 0", "no undistortion map")
    hp.set_undistort(0, *uc.calibration(0))
    hp.set_undistort(1, *uc.calibration(1))
    refused(lib.oatgpu_set_tracker_undistort(ctx, 1), "stream 2", "no undistortion map")
    hp.set_undistort(2, *uc.calibration(2))
    refused(lib.oatgpu_set_tracker_undistort(ctx, 2), "0 (off) or 1 (on)")
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
    # off through every refusal: a step on the given frames is the oracle's WITHOUT undistortion
    _check_want(hp, track(bufs[0]), plain[0], "off after refusals", read=rd)
    A.SubtractionTracker.reset(hp)
    assert lib.oatgpu_set_tracker_undistort(ctx, 1) == 0
    refused(lib.oatgpu_set_tracker_undistort(ctx, 7), "0 (off) or 1 (on)")
    refused(lib.oatgpu_set_tracker_bayer(ctx, pat, 1), "oatgpu_set_tracker_undistort")
    refused(lib.oatgpu_set_undistort(ctx, 2, Kc, Dd, 0), "stream 2", "oatgpu_set_tracker_undistort")
    _check_want(hp, track(bufs[0]), want[0], "on after refusals", read=rd)
    hp.undistort(True)                                          # the fused tracker's switch: another one
    refused(lib.oatgpu_bsub_track_batch_dev(ctx, C.c_void_p(bufs[1].data_ptr()), alpha, out), "oatgpu_set_track_undistort")
    arr = (C.c_void_p * 1)(bufs[1].data_ptr())
    refused(lib.oatgpu_bsub_track_sequence_dev(ctx, arr, 1, alpha, out), "oatgpu_set_track_undistort")
    hp.undistort(False)
    hp.set_homography([1, 0, 2, 0, 1, 3, 0, 0, 1])
    refused(lib.oatgpu_bsub_track_batch_dev(ctx, C.c_void_p(bufs[1].data_ptr()), alpha, out), "oatgpu_set_homography")
    hp.set_homography(None)
    _check_want(hp, track(bufs[1]), want[1], "on after the other switches", read=rd)
    # beside the switch
    w = B.HSV_WIN
    p = O.hsv_params(h_lo=w["h"][0], h_hi=w["h"][1], s_lo=w["s"][0], s_hi=w["s"][1], v_lo=w["v"][0], v_hi=w["v"][1], erode=c.erode,
                     dilate=c.dilate, min_area=B.AREA[0], max_area=B.AREA[1])
    mogs = [O.Mog2(c.rows, c.cols, 3) for _ in range(n)]
    for s in range(n):                                          # (the enqueued frame 0 above moved the model)
        O.chain_step(mogs[s], uc.given[0][s], 0.01, p)
    pos = hp.track(uc.given[2])                                 # the fused tracker does not look at this switch
    for s in range(n):
        wnt, mask = O.chain_step(mogs[s], uc.given[2][s], 0.01, p)
        _same_detection(pos[s], wnt, ("track", s))
        assert (hp.read_mask(MORPH, s) == mask).all(), ("track", s)
    und_out = torch.zeros(n * c.rows * c.cols * 3, dtype=torch.uint8, device="cuda")
    hp._chk(lib.oatgpu_undistort_dev(ctx, C.c_void_p(bufs[2].data_ptr()), C.c_void_p(und_out.data_ptr())))
    hp.synchronize()
    assert np.array_equal(und_out.cpu().numpy().reshape(n, c.rows, c.cols, 3), np.stack(uc.und[2]))
    _check_want(hp, track(bufs[2]), want[2], "on behind the other calls", read=rd)
    assert lib.oatgpu_set_tracker_undistort(ctx, 0) == 0
    u3 = _dev(uc.und[3])
    _check_want(hp, track(u3), want[3], "packed again", read=rd)
    for s in range(n):
        bg, acc = A.SubtractionTracker.state(hp, s)
        assert bg.tobytes() == want[3][s][3].tobytes() and acc.tobytes() == want[3][s][4].tobytes(), s
