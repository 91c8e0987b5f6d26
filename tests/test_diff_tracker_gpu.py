"""GPU tests of the motion tracker (oatgpu_set_diff_tracker / oatgpu_diff_*; MotionTracker; kernels_diff.hip): `framefilt mask
-> col -C GREY -> posidet diff` for every camera of a context, against the oracle chain per stream (O.bgr2grey on the frame,
after frame[roi == 0] = 0 where a ROI is set, then O.Diff.detect).  Detections as tests/parity_asserts.py compares them; the
THRESHOLD tap bit for bit against the numpy front end of tests/diff_cases.py, the MORPH tap against the oracle's `thr > 0`
on [1:-1, 1:-1] (the outer ring is where blur and dilation differ, and findContours zeroes it), the FINAL tap = MORPH with
that ring zeroed.  These cases are about the FRONT kernel: their masks are nearly empty (noise under a third of the threshold),
so the back half takes its single-workgroup LDS kernel on every frame here and the global union-find never runs.  The back half
on frames over that kernel's capacity is tested in tests/test_busy_trackers_gpu.py.  Every frame is under 0.1 MP."""
import ctypes as C
import functools

import numpy as np
import pytest

import diff_cases as D
import oracle_lib as O
from parity_asserts import _same_detection

pytestmark = pytest.mark.gpu

E_INVALID = -1
THR, MORPH, FIN = 0, 1, 2


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


class Ref:
    """One stream of the reference, with the numpy front end beside it for the THRESHOLD tap."""

    def __init__(self, c):
        self.c = c
        self.reset()

    def reset(self):
        self.o = O.Diff(self.c.rows, self.c.cols, self.c.diff_threshold, self.c.blur, *D.AREA)
        self.m = D.Model(self.c.diff_threshold, self.c.blur)

    def step(self, frame, roi=None):
        """-> (detection, threshold bits, oracle mask > 0, first frame?)"""
        first = self.m.last is None
        bits, _ = self.m.front(frame, roi)
        det, thr = self.o.detect(D.oracle_frame(frame, roi))
        return det, bits, thr > 0, first


@functools.lru_cache(maxsize=None)
def _case(rows, cols, ch, n, thr=12, blur=2, roi=False, n_frames=12):
    c = D.make_case(f"{rows}x{cols}-ch{ch}-n{n}-t{thr}-b{blur}", rows, cols, ch, n, diff_threshold=thr, blur=blur, roi=roi,
                    n_frames=n_frames, seed=rows + n)
    refs = [Ref(c) for _ in range(n)]
    want = [[refs[s].step(f, c.roi_at(t, s)) for s, f in enumerate(fs)] for t, fs in enumerate(c.frames)]
    return c, want


def _tracker(A, c, **kw):
    return A.MotionTracker(c.rows, c.cols, n_streams=c.n_streams, channels=c.channels, diff_threshold=c.diff_threshold,
                           blur=c.blur, area=D.AREA, **kw)


def _check_taps(mt, s, want, tag, read=None):
    _, bits, omask, first = want
    read = read or mt.read_mask
    thr, morph, fin = read(THR, s), read(MORPH, s), read(FIN, s)
    for m in (thr, morph, fin):
        assert set(np.unique(m)) <= {0, 255}, tag
    assert ((thr > 0) == bits).all(), ("threshold tap", tag)
    if first:
        assert ((morph > 0) == omask).all(), ("morph tap of a first frame", tag)
    else:
        assert ((morph > 0)[1:-1, 1:-1] == omask[1:-1, 1:-1]).all(), ("morph tap", tag)
    ring = np.ones(fin.shape, bool)
    ring[1:-1, 1:-1] = False
    assert (fin[1:-1, 1:-1] == morph[1:-1, 1:-1]).all() and not fin[ring].any(), ("final tap", tag)


def _check(mt, got, want_t, tag, taps=True, read=None):
    for s, w in enumerate(want_t):
        _same_detection(got[s], w[0], (tag, s))
        if taps:
            _check_taps(mt, s, w, (tag, s), read)


# ------------------------------------------------------------------------------------------ the synchronous step ----

@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("ch", [3, 1])
@pytest.mark.parametrize("rows,cols", D.GEOMETRIES)
def test_synchronous_step_on_device_and_host_frames(A, rows, cols, ch, n):
    c, want = _case(rows, cols, ch, n)
    dev, host = _tracker(A, c), _tracker(A, c)
    hits = 0
    for t, fs in enumerate(c.frames):
        buf = _dev(fs)
        _check(dev, dev.track_dev(buf.data_ptr()), want[t], ("dev", t))
        _check(host, host.track(fs), want[t], ("host", t))
        hits += sum(w[0]["valid"] for w in want[t])
    assert hits >= 6 * n


@pytest.mark.parametrize("blur", [0, 2, 5, 22])
@pytest.mark.parametrize("thr", [0, 12, 254, 255])
def test_parameters(A, thr, blur):
    for rows, cols, ch in ((37, 91, 3), (33, 128, 1)):          # the narrow and the wide instantiation
        c, want = _case(rows, cols, ch, 2, thr=thr, blur=blur)
        mt = _tracker(A, c)
        for t, fs in enumerate(c.frames):
            buf = _dev(fs)
            _check(mt, mt.track_dev(buf.data_ptr()), want[t], (rows, cols, t))


@pytest.mark.parametrize("offset", [1, 4])
@pytest.mark.parametrize("ch", [3, 1])
@pytest.mark.parametrize("rows,cols", [(90, 200), (33, 128)])
def test_misaligned_device_frames(A, rows, cols, ch, offset):
    """A frame buffer 1 byte off a dword takes the one-pixel-a-lane kernel (chosen per launch on the host); 4 bytes off is
    still aligned and stays on the wide one.  Either way the results are the oracle's."""
    import torch
    c, want = _case(rows, cols, ch, 3)
    mt = _tracker(A, c)
    size = c.n_streams * rows * cols * ch
    store = torch.zeros(size + 8, dtype=torch.uint8, device="cuda")
    view = store[offset:offset + size]
    assert view.data_ptr() % 4 == offset % 4
    for t, fs in enumerate(c.frames):
        view.copy_(torch.from_numpy(np.stack(fs).reshape(-1)))
        torch.cuda.synchronize()
        _check(mt, mt.track_dev(view.data_ptr()), want[t], (offset, t))


# ----------------------------------------------------------------------------------------------- the sequence call ----

def _taps(mt, n):
    return [[mt.read_mask(w, s) for w in (THR, MORPH, FIN)] for s in range(n)]


@pytest.mark.parametrize("before", [0, 3], ids=["fresh", "continuing"])
@pytest.mark.parametrize("n_frames", [0, 1, 2, 5, 8])
@pytest.mark.parametrize("rows,cols,ch", [(90, 200, 3), (37, 91, 1)])
def test_sequence_equals_synchronous_steps(A, rows, cols, ch, n_frames, before):
    c, _ = _case(rows, cols, ch, 3, roi=True)
    seq, one = _tracker(A, c), _tracker(A, c)
    for mt in (seq, one):                                       # (one ROI on stream 1 for the whole run)
        mt.set_roi_mask(c.roi, stream=c.roi_stream)
    bufs = [_dev(fs) for fs in c.frames]
    for t in range(before):
        a, b = seq.track_dev(bufs[t].data_ptr()), one.track_dev(bufs[t].data_ptr())
        assert a == b
    span = range(before, before + n_frames)
    got = seq.track_sequence_dev([bufs[t].data_ptr() for t in span])
    ref = [one.track_dev(bufs[t].data_ptr()) for t in span]
    assert got == ref
    assert len(got) == n_frames
    if before + n_frames:
        for x, y in zip(_taps(seq, 3), _taps(one, 3)):
            for p, q in zip(x, y):
                assert (p == q).all()
    nxt = before + n_frames
    assert seq.track_dev(bufs[nxt].data_ptr()) == one.track_dev(bufs[nxt].data_ptr())       # ... which proves `last`
    for x, y in zip(_taps(seq, 3), _taps(one, 3)):
        for p, q in zip(x, y):
            assert (p == q).all()


@pytest.mark.parametrize("n_frames", [1, 2, 5, 8])
def test_sequence_against_the_oracle(A, n_frames):
    c, want = _case(90, 200, 3, 3)
    mt = _tracker(A, c)
    bufs = [_dev(fs) for fs in c.frames[:n_frames + 1]]
    got = mt.track_sequence_dev([b.data_ptr() for b in bufs[:n_frames]])
    for t in range(n_frames):
        _check(mt, got[t], want[t], ("seq", t), taps=t == n_frames - 1)
    _check(mt, mt.track_dev(bufs[n_frames].data_ptr()), want[n_frames], "next")


def test_sequence_with_streams_in_mixed_first_frame_state(A):
    """Stream 1 is primed by oatgpu_detect_diff, the others are not: the first frame set of the sequence is a first frame
    for streams 0 and 2 and a second one for stream 1 (two runs of the back half, a single-frame front launch)."""
    from oat_amd import ffi
    c, _ = _case(90, 200, 3, 3)
    mt = _tracker(A, c)
    refs = [Ref(c) for _ in range(3)]
    p = ffi.Position()
    g0 = O.bgr2grey(c.frames[0][1])
    mt._chk(mt.lib.oatgpu_detect_diff(mt.ctx, 1, ffi.u8(g0), C.byref(p)))
    _same_detection(A.Position2D.from_c(p), refs[1].o.detect(g0)[0], "prime")
    refs[1].m.front(g0)
    bufs = [_dev(fs) for fs in c.frames[1:7]]
    got = mt.track_sequence_dev([b.data_ptr() for b in bufs[:5]])
    for t in range(5):
        want = [refs[s].step(c.frames[1 + t][s]) for s in range(3)]
        _check(mt, got[t], want, ("mixed", t), taps=t == 4)
    _check(mt, mt.track_dev(bufs[5].data_ptr()), [refs[s].step(c.frames[6][s]) for s in range(3)], "next")


# ------------------------------------------------------------------------------------------------ state and ROI ----

def test_state_is_shared_with_detect_diff_and_reset(A):
    """oatgpu_detect_diff (one stream), oatgpu_diff_batch_dev (all) and oatgpu_diff_reset interleaved over 10 frames: every
    stream equals an oracle that saw exactly the frames that stream was given; a reset oracle is a new one."""
    from oat_amd import ffi
    c, _ = _case(90, 200, 1, 3, n_frames=10)
    mt = _tracker(A, c)
    refs = [Ref(c) for _ in range(3)]
    plan = ["batch", ("single", 1), "batch", ("reset", 0), "batch", ("single", 0), ("single", 2), ("reset", None), "batch", "batch"]
    for t, op in enumerate(plan):
        fs = c.frames[t]
        if op == "batch":
            buf = _dev(fs)
            _check(mt, mt.track_dev(buf.data_ptr()), [refs[s].step(fs[s]) for s in range(3)], (t, op))
        elif op[0] == "single":
            s, p = op[1], ffi.Position()
            mt._chk(mt.lib.oatgpu_detect_diff(mt.ctx, s, ffi.u8(fs[s]), C.byref(p)))
            _same_detection(A.Position2D.from_c(p), refs[s].step(fs[s])[0], (t, op))
        else:
            mt.reset(op[1])
            for s in range(3):
                if op[1] in (None, s):
                    refs[s].reset()


@pytest.mark.parametrize("rows,cols,ch", [(90, 200, 3), (37, 91, 1)])
def test_roi_on_one_stream_set_and_removed_between_frames(A, rows, cols, ch):
    c, want = _case(rows, cols, ch, 3, roi=True)
    mt = _tracker(A, c)
    on = False
    for t, fs in enumerate(c.frames):
        now = c.roi_at(t, c.roi_stream) is not None
        if now != on:
            mt.set_roi_mask(c.roi if now else None, stream=c.roi_stream)
            on = now
        buf = _dev(fs)
        _check(mt, mt.track_dev(buf.data_ptr()), want[t], ("roi", t))


# ------------------------------------------------------------------------------------ refusals, the context's other calls ----

HSV_WIN = dict(h_thresh=(0, 256), s_thresh=(0, 256), v_thresh=(60, 256))
LR = 0.01


def _both(A, c, tracker=True):
    """A context with the fused tracker's detector AND the motion tracker (MotionTracker's methods serve any context)."""
    hp = A.HotPath(c.rows, c.cols, n_streams=c.n_streams, adaptation_coeff=LR, erode=0, dilate=3, area=D.AREA,
                   diff_threshold=c.diff_threshold, blur=c.blur, **HSV_WIN)
    if tracker:
        hp._chk(hp.lib.oatgpu_set_diff_tracker(hp.ctx, 1))
    return hp


def _diff_dev(A, hp, ptr):
    return A.MotionTracker.track_dev(hp, ptr)


def _read_diff(A, hp):
    return lambda which, s: A.MotionTracker.read_mask(hp, which, s)


def test_refusals_leave_the_context_as_it_was(A):
    import undistort_ref as R
    from oat_amd import ffi
    c, want = _case(90, 200, 3, 3)
    n = c.n_streams
    bufs = [_dev(fs) for fs in c.frames]
    out = (ffi.Position * (4 * n))()
    seq = (C.c_void_p * 2)(bufs[0].data_ptr(), bufs[1].data_ptr())
    hostp = (ffi._u8p * n)(*[ffi.u8(f) for f in c.frames[0]])

    def refused(hp, *needles):
        lib, ctx = hp.lib, hp.ctx
        for rc in (lib.oatgpu_diff_batch_dev(ctx, C.c_void_p(bufs[0].data_ptr()), out),
                   lib.oatgpu_diff_batch(ctx, hostp, n, out),
                   lib.oatgpu_diff_sequence_dev(ctx, seq, 2, out)):
            assert rc == E_INVALID
            msg = lib.oatgpu_last_error(ctx).decode()
            assert any(k in msg for k in needles), msg

    off = _both(A, c, tracker=False)
    refused(off, "oatgpu_set_diff_tracker")
    assert off.lib.oatgpu_read_diff_mask(off.ctx, 0, MORPH, ffi.u8(np.empty((c.rows, c.cols), np.uint8))) == E_INVALID

    hp = _both(A, c)
    lib, ctx = hp.lib, hp.ctx
    assert lib.oatgpu_read_diff_mask(ctx, 0, MORPH, ffi.u8(np.empty((c.rows, c.cols), np.uint8))) == E_INVALID   # no step yet
    hp.enqueue_dev(bufs[0].data_ptr(), keepalive=bufs[0])
    refused(hp, "outstanding")
    hp.collect()
    hp.stage(0, c.frames[0][0])
    refused(hp, "outstanding")
    hp.stage_abort()
    hp.set_kalman(True)
    refused(hp, "oatgpu_set_kalman")
    hp.set_kalman(False)
    hp.set_homography([1, 0, 2, 0, 1, 3, 0, 0, 1])
    refused(hp, "oatgpu_set_homography")
    hp.set_homography(None)
    K, Dc = next(iter(R.cases(c.rows, c.cols).values()))
    for s in range(n):
        hp.set_undistort(s, K, Dc)
    hp.undistort(True)
    refused(hp, "oatgpu_set_track_undistort")
    hp.undistort(False)
    # arguments
    assert lib.oatgpu_diff_batch_dev(ctx, None, out) == E_INVALID
    assert lib.oatgpu_diff_batch_dev(ctx, C.c_void_p(bufs[0].data_ptr()), None) == E_INVALID
    assert lib.oatgpu_diff_batch(ctx, None, n, out) == E_INVALID
    assert lib.oatgpu_diff_batch(ctx, hostp, n, None) == E_INVALID
    assert lib.oatgpu_diff_batch(ctx, hostp, n - 1, out) == E_INVALID
    assert lib.oatgpu_diff_batch(ctx, hostp, n + 1, out) == E_INVALID
    assert lib.oatgpu_diff_sequence_dev(ctx, None, 2, out) == E_INVALID
    assert lib.oatgpu_diff_sequence_dev(ctx, seq, 2, None) == E_INVALID
    assert lib.oatgpu_diff_sequence_dev(ctx, seq, -1, out) == E_INVALID
    assert "n_frames" in lib.oatgpu_last_error(ctx).decode()
    assert lib.oatgpu_diff_sequence_dev(ctx, seq, 0, out) == 0
    assert lib.oatgpu_diff_reset(ctx, n) == E_INVALID
    assert lib.oatgpu_read_diff_mask(ctx, 0, MORPH, None) == E_INVALID
    assert lib.oatgpu_read_diff_mask(ctx, n, MORPH, ffi.u8(np.empty((c.rows, c.cols), np.uint8))) == E_INVALID
    # nothing of all that moved the tracker: the frames still meet a fresh state
    for t in range(4):
        _check(hp, _diff_dev(A, hp, bufs[t].data_ptr()), want[t], ("after refusals", t), read=_read_diff(A, hp))
    assert lib.oatgpu_read_diff_mask(ctx, 0, 7, ffi.u8(np.empty((c.rows, c.cols), np.uint8))) == E_INVALID


def test_the_context_stays_good_for_its_other_calls(A):
    """Diff steps and the fused tracker's calls interleaved on ONE context: each side equals its oracle, oatgpu_read_mask
    shows the fused tracker's planes and oatgpu_read_diff_mask the motion tracker's, whatever ran in between."""
    c, want = _case(90, 200, 3, 3)
    n = c.n_streams
    hp = _both(A, c)
    p = O.hsv_params(h_lo=0, h_hi=256, s_lo=0, s_hi=256, v_lo=60, v_hi=256, erode=0, dilate=3, min_area=D.AREA[0], max_area=D.AREA[1])
    mogs = [O.Mog2(c.rows, c.cols, 3) for _ in range(n)]
    bufs = [_dev(fs) for fs in c.frames]
    rd = _read_diff(A, hp)
    dt = [0]                                    # the next frame of the diff side

    def diff_steps(k, seq=False):
        ts = list(range(dt[0], dt[0] + k))
        got = (A.MotionTracker.track_sequence_dev(hp, [bufs[t].data_ptr() for t in ts]) if seq
               else [_diff_dev(A, hp, bufs[t].data_ptr()) for t in ts])
        for i, t in enumerate(ts):
            _check(hp, got[i], want[t], ("diff", t), taps=i == k - 1, read=rd)
        dt[0] += k

    masks = [None] * n                          # the fused tracker's latest MORPH planes, from the oracle

    def track_steps(ts, seq=False):
        got = hp.track_sequence_dev([bufs[t].data_ptr() for t in ts]) if seq else [hp.track_dev(bufs[t].data_ptr()) for t in ts]
        for i, t in enumerate(ts):
            for s in range(n):
                w, masks[s] = O.chain_step(mogs[s], c.frames[t][s], LR, p)
                _same_detection(got[i][s], w, ("track", t, s))
        track_planes("track")

    def track_planes(tag):
        for s in range(n):
            assert (hp.read_mask(MORPH, s) == masks[s]).all(), (tag, s)

    def diff_planes(tag):
        for s in range(n):
            _check_taps(hp, s, want[dt[0] - 1][s], (tag, s), read=rd)

    diff_steps(2)
    track_steps([0, 1])
    diff_planes("behind synchronous track steps")
    diff_steps(3, seq=True)
    track_planes("behind a diff sequence")
    track_steps([2, 3, 4, 5], seq=True)
    diff_planes("behind a track sequence")
    diff_steps(1)
    track_planes("behind a diff step")
    track_steps([6])
    diff_steps(4, seq=True)
    track_planes("behind the last diff sequence")
