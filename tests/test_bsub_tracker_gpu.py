"""GPU tests of the subtraction tracker (oatgpu_set_bsub_tracker / oatgpu_bsub_track_*; SubtractionTracker; kernels_bsubtrack.hip):
`framefilt mask -> bsub -> col -C HSV -> posidet hsv` (GREY: `bsub -> posidet thresh`) for every camera of a context, against
the oracle chain per stream (tests/bsub_cases.py: Oracle).  Detections as tests/parity_asserts.py compares them, the integer
Green sums included; the THRESHOLD tap bit for bit against the oracle's inRange, the MORPH tap against its erode / dilate, the
FINAL tap = MORPH with the outer ring zeroed; the background and its fp32 accumulator (oatgpu_bsub_get_state) bit for bit
against the numpy model.  tests/test_bsub_tracker_cpu.py holds that model to the oracle through the subtracted image; the oracle
does not show its accumulator, so for `acc` the model (independent of the kernel, separate roundings) is the only reference.
Everything is exact: no tolerance anywhere.
These cases are about the FRONT kernel and the state: their masks hold a handful of planted pixels and one rectangle, so the back
half takes its single-workgroup LDS kernel on every frame here and the global union-find never runs.  The back half on frames over
that kernel's capacity is tested in tests/test_busy_trackers_gpu.py.
Every frame is under 0.1 MP."""
import ctypes as C
import functools

import numpy as np
import pytest

import bsub_cases as B
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


CASES = {c.name: c for c in B.cpu_cases()}


@functools.lru_cache(maxsize=None)
def _named(name):
    return _expect(CASES[name])


@functools.lru_cache(maxsize=None)
def _case(rows, cols, ch, n, alpha=0.05, erode=0, dilate=10, roi=False, n_frames=B.N_FRAMES):
    return _expect(B.make_case(f"{rows}x{cols}-ch{ch}-n{n}-a{alpha}", rows, cols, ch, n, alpha=alpha, erode=erode, dilate=dilate,
                               roi=roi, n_frames=n_frames, seed=rows + n))


def _expect(c):
    """-> (case, want[t][s] = (detection, bits, morph > 0, bg, acc)), computed once and shared"""
    refs = [B.Ref(c, s) for s in range(c.n_streams)]
    return c, [[refs[s].step(f, c.roi_at(t, s)) for s, f in enumerate(fs)] for t, fs in enumerate(c.frames)]


def _tracker(A, c):
    st = A.SubtractionTracker(c.rows, c.cols, **c.tracker_args())
    for s, img in c.background.items():
        st.set_background(img, stream=s)
    return st


def _check_taps(st, s, want, tag, read=None):
    _, bits, omorph, _, _ = want
    read = read or st.read_mask
    thr, morph, fin = read(THR, s), read(MORPH, s), read(FIN, s)
    for m in (thr, morph, fin):
        assert set(np.unique(m)) <= {0, 255}, tag
    assert ((thr > 0) == bits).all(), ("threshold tap", tag)
    assert ((morph > 0) == omorph).all(), ("morph tap", tag)
    ring = np.ones(fin.shape, bool)
    ring[1:-1, 1:-1] = False
    assert (fin[1:-1, 1:-1] == morph[1:-1, 1:-1]).all() and not fin[ring].any(), ("final tap", tag)


def _check(st, got, want_t, tag, taps=True, read=None):
    for s, w in enumerate(want_t):
        _same_detection(got[s], w[0], (tag, s))
        if taps:
            _check_taps(st, s, w, (tag, s), read)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _get_state(A, st, s, acc=True):
    return A.SubtractionTracker.state(st, s, acc=acc)


def _check_state(A, st, want_t, tag, streams=None):
    """oatgpu_bsub_get_state against the model: the background bytes and the accumulator's bit patterns"""
    for s, w in enumerate(want_t):
        if streams is not None and s not in streams:
            continue
        bg, acc = _get_state(A, st, s, acc=w[4] is not None)
        assert _same_bits(bg, w[3]), ("background", tag, s, int((bg != w[3]).sum()))
        if w[4] is not None:
            assert _same_bits(acc, w[4]), ("accumulator", tag, s, int((acc.view(np.uint32) != w[4].view(np.uint32)).sum()))


def _roi_to(st, c, t, on):
    now = c.roi_at(t, c.roi_stream) is not None
    if now != on:
        st.set_roi_mask(c.roi if now else None, stream=c.roi_stream)
    return now


# ------------------------------------------------------------------------------------------ the synchronous step ----

@pytest.mark.parametrize("name", list(CASES))
def test_every_case_on_device_and_host_frames(A, name):
    c, want = _named(name)
    dev, host = _tracker(A, c), _tracker(A, c)
    on = False
    hits = 0
    for t, fs in enumerate(c.frames):
        for st in (dev, host):
            now = _roi_to(st, c, t, on)
        on = now
        buf = _dev(fs)
        _check(dev, dev.track_dev(buf.data_ptr()), want[t], ("dev", t))
        _check(host, host.track(fs), want[t], ("host", t))
        hits += sum(w[0]["valid"] for w in want[t])
    if c.alpha <= 0.05:
        assert 2 * hits >= len(c.frames) * c.n_streams
    _check_state(A, dev, want[-1], "dev")
    _check_state(A, host, want[-1], "host")


def test_sixty_frames_of_adaptation_leave_the_models_state(A):
    c, want = _case(37, 91, 3, 2, alpha=0.05, n_frames=60)
    st = _tracker(A, c)
    for t, fs in enumerate(c.frames):
        buf = _dev(fs)
        got = st.track_dev(buf.data_ptr())
        for s, w in enumerate(want[t]):
            _same_detection(got[s], w[0], (t, s))
    _check_taps(st, 0, want[-1][0], "last")
    _check_state(A, st, want[-1], "60 frames")


@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("ch", [3, 1])
@pytest.mark.parametrize("rows,cols", [(90, 200), (33, 128)])
def test_misaligned_device_frames(A, rows, cols, ch, offset):
    """A frame buffer 1 to 3 bytes off a dword takes the one-pixel-a-lane kernel (chosen per launch on the host) on a width the
    aligned frames take four pixels a lane; results and state are the same."""
    import torch
    c, want = _case(rows, cols, ch, 3)
    st = _tracker(A, c)
    size = c.n_streams * rows * cols * ch
    store = torch.zeros(size + 8, dtype=torch.uint8, device="cuda")
    view = store[offset:offset + size]
    assert view.data_ptr() % 4 == offset
    for t, fs in enumerate(c.frames):
        view.copy_(torch.from_numpy(np.stack(fs).reshape(-1)))
        torch.cuda.synchronize()
        _check(st, st.track_dev(view.data_ptr()), want[t], (offset, t))
    _check_state(A, st, want[-1], offset)


# ----------------------------------------------------------------------------------------------- the sequence call ----

def _taps(st, n):
    return [[st.read_mask(w, s) for w in (THR, MORPH, FIN)] for s in range(n)]


def _same_everything(A, a, b, n, tag):
    for x, y in zip(_taps(a, n), _taps(b, n)):
        for p, q in zip(x, y):
            assert (p == q).all(), tag
    for s in range(n):
        (bg1, acc1), (bg2, acc2) = _get_state(A, a, s), _get_state(A, b, s)
        assert _same_bits(bg1, bg2) and _same_bits(acc1, acc2), (tag, s)


# the paired launch in every lane mapping and colour: wide BGR, narrow GREY, wide GREY, narrow BGR
PAIR_SHAPES = [(90, 200, 3), (37, 91, 1), (33, 128, 1), (37, 91, 3)]


@pytest.mark.parametrize("alpha", [0.0, 0.05])
@pytest.mark.parametrize("start", ["fresh", "mixed"])
@pytest.mark.parametrize("n_frames", [1, 2, 5, 8])
@pytest.mark.parametrize("rows,cols,ch", PAIR_SHAPES)
def test_sequence_equals_synchronous_steps(A, rows, cols, ch, n_frames, start, alpha):
    """Results, taps and state; from a fresh state (the first frame is the first of a pair) and from a mixed one: streams 0 and
    2 have a background, stream 1 was reset.  alpha 0: the paired kernels that do not learn -- a first frame of a pair stores the
    state once, from the first frame only; a later pair reads the background and stores nothing."""
    c, _ = _case(rows, cols, ch, 3, alpha=alpha, roi=True, n_frames=12)
    seq, one = _tracker(A, c), _tracker(A, c)
    for st in (seq, one):                                       # (one ROI on stream 1 for the whole run)
        st.set_roi_mask(c.roi, stream=c.roi_stream)
    bufs = [_dev(fs) for fs in c.frames]
    before = 0
    if start == "mixed":
        before = 2
        for t in range(before):
            assert seq.track_dev(bufs[t].data_ptr()) == one.track_dev(bufs[t].data_ptr())
        seq.reset(1)
        one.reset(1)
    span = range(before, before + n_frames)
    got = seq.track_sequence_dev([bufs[t].data_ptr() for t in span])
    ref = [one.track_dev(bufs[t].data_ptr()) for t in span]
    assert got == ref and len(got) == n_frames
    _same_everything(A, seq, one, 3, "behind the sequence")
    nxt = before + n_frames
    assert seq.track_dev(bufs[nxt].data_ptr()) == one.track_dev(bufs[nxt].data_ptr())
    _same_everything(A, seq, one, 3, "one step later")


@pytest.mark.parametrize("alpha", [0.0, 0.05])
@pytest.mark.parametrize("rows,cols,ch", PAIR_SHAPES)
@pytest.mark.parametrize("n_frames", [1, 2, 5, 8])
def test_sequence_against_the_oracle(A, n_frames, rows, cols, ch, alpha):
    c, want = _case(rows, cols, ch, 3, alpha=alpha, n_frames=12)
    st = _tracker(A, c)
    bufs = [_dev(fs) for fs in c.frames[:n_frames + 1]]
    got = st.track_sequence_dev([b.data_ptr() for b in bufs[:n_frames]])
    for t in range(n_frames):
        _check(st, got[t], want[t], ("seq", t), taps=t == n_frames - 1)
    _check_state(A, st, want[n_frames - 1], "seq")
    _check(st, st.track_dev(bufs[n_frames].data_ptr()), want[n_frames], "next")


@pytest.mark.parametrize("name", ["file-bgr", "file-grey"])
def test_sequence_over_backgrounds_from_a_file(A, name):
    """Every second stream's background came from a file (it has no accumulator and is never written), the others make theirs
    from the sequence's first frame, which is the first of a pair: one sequence call over all frames but the last, then a step."""
    c, want = _named(name)
    st = _tracker(A, c)
    bufs = [_dev(fs) for fs in c.frames]
    n = len(bufs) - 1
    got = st.track_sequence_dev([b.data_ptr() for b in bufs[:n]])
    for t in range(n):
        _check(st, got[t], want[t], (name, t), taps=t == n - 1)
    _check_state(A, st, want[n - 1], name)
    _check(st, st.track_dev(bufs[n].data_ptr()), want[n], "next")
    _check_state(A, st, want[n], "next")


@pytest.mark.parametrize("alpha", [0.0, 0.05])
@pytest.mark.parametrize("ch", [3, 1])
def test_sequence_on_misaligned_device_frames(A, ch, alpha):
    """Frame sets 1 byte off a dword: the paired launch takes the one-pixel-a-lane kernel on a width that is wide when aligned."""
    import torch
    c, want = _case(33, 128, ch, 3, alpha=alpha, n_frames=12)
    st = _tracker(A, c)
    size = c.n_streams * c.rows * c.cols * ch
    stores = []
    for fs in c.frames[:5]:
        store = torch.zeros(size + 8, dtype=torch.uint8, device="cuda")
        store[1:1 + size].copy_(torch.from_numpy(np.stack(fs).reshape(-1)))
        stores.append(store)
    torch.cuda.synchronize()
    ptrs = [s.data_ptr() + 1 for s in stores]
    assert all(p % 4 == 1 for p in ptrs)
    got = st.track_sequence_dev(ptrs)
    for t in range(5):
        _check(st, got[t], want[t], ("misaligned", t), taps=t == 4)
    _check_state(A, st, want[4], "misaligned")


@pytest.mark.parametrize("alpha", [0.0, 0.05])
def test_sixty_six_streams_split_the_first_frame_flags(A, alpha):
    """The first-frame flags of a launch are one 64-bit argument: 66 streams take two launches.  Streams 0 and 64 meet the
    frame as their first, 63 and 65 (and all others) as a later one; once as a synchronous step, once as the first of a pair."""
    c = B.make_case("66", 6, 8, 3, 66, alpha=alpha, dilate=3, n_frames=5, seed=9)
    for paired in (False, True):
        refs = [B.Ref(c, s) for s in range(66)]
        st = _tracker(A, c)
        bufs = [_dev(fs) for fs in c.frames]
        for t in range(2):
            want = [refs[s].step(c.frames[t][s]) for s in range(66)]
            _check(st, st.track_dev(bufs[t].data_ptr()), want, ("warm", t), taps=False)
        for s in (0, 64):
            st.reset(s)
            refs[s].reset()
        if paired:
            got = st.track_sequence_dev([bufs[2].data_ptr(), bufs[3].data_ptr()])
        else:
            got = [st.track_dev(bufs[t].data_ptr()) for t in (2, 3)]
        for i, t in enumerate((2, 3)):
            want = [refs[s].step(c.frames[t][s]) for s in range(66)]
            _check(st, got[i], want, ("split", paired, t), taps=False)
        for s in (0, 63, 64, 65):
            _check_taps(st, s, want[s], ("split", paired, s))
        _check_state(A, st, want, ("split", paired), streams=(0, 1, 62, 63, 64, 65))


# ------------------------------------------------------------------------------------------------ shared state ----

class _Side:
    """The model of one stream with the detector behind it (erode / dilate / siftContours of the oracle): for the tests that
    change alpha between steps, which oracle_lib.Bsub cannot.  The model is held to the oracle by the CPU file."""

    def __init__(self, c):
        self.c, self.m = c, B.Model(c.alpha)

    def step(self, frame, alpha=None):
        c = self.c
        self.m.alpha = c.alpha if alpha is None else alpha
        bits, bg, acc, d = self.m.front(frame)
        img = np.where(bits, 255, 0).astype(np.uint8)
        if c.erode > 0:
            img = O.erode(img, c.erode)
        if c.dilate > 0:
            img = O.dilate(img, c.dilate)
        return (O.sift_contours(img, *B.AREA), bits, img > 0, bg, acc), d


@pytest.mark.parametrize("rows,cols,ch", [(90, 200, 3), (37, 91, 1)])
def test_state_is_shared_with_bsub_filter_and_set_background(A, rows, cols, ch):
    from oat_amd import ffi
    c, _ = _case(rows, cols, ch, 2, n_frames=12)
    st = _tracker(A, c)
    sides = [_Side(c) for _ in range(2)]

    def batch(t, alpha=None):
        buf = _dev(c.frames[t])
        want = [sides[s].step(c.frames[t][s], alpha)[0] for s in range(2)]
        _check(st, st.track_dev(buf.data_ptr(), alpha=alpha), want, ("batch", t))
        return want

    def single(t, s, alpha):
        out = np.empty(c.shape, np.uint8)
        st._chk(st.lib.oatgpu_bsub_filter(st.ctx, s, ffi.u8(c.frames[t][s]), ffi.u8(out), alpha))
        assert (out == sides[s].step(c.frames[t][s], alpha)[1]).all(), ("bsub_filter", t, s)

    single(0, 1, 0.05)                      # oatgpu_bsub_filter makes stream 1's background, the tracker stream 0's
    batch(1)
    single(2, 0, 0.05)                      # ... and each continues the other's
    want = batch(3)
    _check_state(A, st, want, "mixed forms")
    single(4, 0, 0.0)
    want = batch(5, alpha=0.0)              # a frozen background: bg and acc stay
    _check_state(A, st, want, "alpha 0")
    # a background from a file on stream 1: alpha > 0 is refused naming the stream, and nothing has changed
    img = np.full(c.shape, 60, np.uint8)
    st.set_background(img, stream=1)
    sides[1].m.set_background(img)
    buf = _dev(c.frames[6])
    pos = (ffi.Position * 2)()
    seq = (C.c_void_p * 1)(buf.data_ptr())
    hostp = (ffi._u8p * 2)(*[ffi.u8(f) for f in c.frames[6]])
    for rc in (st.lib.oatgpu_bsub_track_batch_dev(st.ctx, C.c_void_p(buf.data_ptr()), 0.05, pos),
               st.lib.oatgpu_bsub_track_batch(st.ctx, hostp, 2, 0.05, pos),
               st.lib.oatgpu_bsub_track_sequence_dev(st.ctx, seq, 1, 0.05, pos)):
        assert rc == E_INVALID
        assert "stream 1" in st.lib.oatgpu_last_error(st.ctx).decode()
    bg0, acc0 = _get_state(A, st, 0)
    assert _same_bits(bg0, want[0][3]) and _same_bits(acc0, want[0][4])
    assert _same_bits(_get_state(A, st, 1, acc=False)[0], img)
    assert st.lib.oatgpu_bsub_get_state(st.ctx, 1, None, ffi.f32(np.empty(c.shape, np.float32))) == E_INVALID
    want = batch(6, alpha=0.0)
    _check_state(A, st, want, "file background")
    st.reset(1)                             # forgotten: the next frame is the background, and it can adapt again
    sides[1].m.reset()
    want = batch(7)
    _check_state(A, st, want, "after the reset")


# ------------------------------------------------------------------------------------ refusals, the context's other calls ----

LR = 0.01


def _both(A, c, tracker=True):
    """A context with the fused tracker's detector, the motion tracker AND the subtraction tracker (SubtractionTracker's methods
    serve any context)."""
    w = B.HSV_WIN
    hp = A.HotPath(c.rows, c.cols, n_streams=c.n_streams, adaptation_coeff=LR, erode=c.erode, dilate=c.dilate, area=B.AREA,
                   h_thresh=w["h"], s_thresh=w["s"], v_thresh=w["v"], diff_threshold=12, blur=2)
    hp._chk(hp.lib.oatgpu_set_diff_tracker(hp.ctx, 1))
    if tracker:
        hp._chk(hp.lib.oatgpu_set_bsub_tracker(hp.ctx, 1))
    return hp


def _read_bsub(A, hp):
    return lambda which, s: A.SubtractionTracker.read_mask(hp, which, s)


def test_refusals_leave_the_context_as_it_was(A):
    import undistort_ref as R
    from oat_amd import ffi
    c, want = _case(90, 200, 3, 3)
    n, a = c.n_streams, c.alpha
    bufs = [_dev(fs) for fs in c.frames]
    out = (ffi.Position * (4 * n))()
    seq = (C.c_void_p * 2)(bufs[2].data_ptr(), bufs[3].data_ptr())
    hostp = (ffi._u8p * n)(*[ffi.u8(f) for f in c.frames[2]])
    plane = lambda: ffi.u8(np.empty((c.rows, c.cols), np.uint8))

    def refused(hp, *needles, alpha=a):
        lib, ctx = hp.lib, hp.ctx
        for rc in (lib.oatgpu_bsub_track_batch_dev(ctx, C.c_void_p(bufs[2].data_ptr()), alpha, out),
                   lib.oatgpu_bsub_track_batch(ctx, hostp, n, alpha, out),
                   lib.oatgpu_bsub_track_sequence_dev(ctx, seq, 2, alpha, out)):
            assert rc == E_INVALID
            msg = lib.oatgpu_last_error(ctx).decode()
            assert any(k in msg for k in needles), msg

    off = _both(A, c, tracker=False)
    refused(off, "oatgpu_set_bsub_tracker")
    assert off.lib.oatgpu_read_bsub_mask(off.ctx, 0, MORPH, plane()) == E_INVALID
    assert off.lib.oatgpu_bsub_get_state(off.ctx, 0, plane(), None) == E_INVALID          # no background yet

    hp = _both(A, c)
    lib, ctx = hp.lib, hp.ctx
    rd = _read_bsub(A, hp)
    assert lib.oatgpu_read_bsub_mask(ctx, 0, MORPH, plane()) == E_INVALID                 # no step yet
    for t in range(2):
        _check(hp, A.SubtractionTracker.track_dev(hp, bufs[t].data_ptr(), alpha=a), want[t], ("before", t), read=rd)
    hp.enqueue_dev(bufs[0].data_ptr(), keepalive=bufs[0])
    refused(hp, "outstanding")
    assert lib.oatgpu_set_bsub_tracker(ctx, 0) == E_INVALID
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
    refused(hp, "adaptation-coeff", alpha=-0.01)
    refused(hp, "adaptation-coeff", alpha=1.5)
    refused(hp, "adaptation-coeff", alpha=float("nan"))
    # arguments
    ptr = C.c_void_p(bufs[2].data_ptr())
    assert lib.oatgpu_bsub_track_batch_dev(ctx, None, a, out) == E_INVALID
    assert lib.oatgpu_bsub_track_batch_dev(ctx, ptr, a, None) == E_INVALID
    assert lib.oatgpu_bsub_track_batch(ctx, None, n, a, out) == E_INVALID
    assert lib.oatgpu_bsub_track_batch(ctx, hostp, n, a, None) == E_INVALID
    assert lib.oatgpu_bsub_track_batch(ctx, hostp, n - 1, a, out) == E_INVALID
    assert lib.oatgpu_bsub_track_batch(ctx, hostp, n + 1, a, out) == E_INVALID
    assert lib.oatgpu_bsub_track_sequence_dev(ctx, None, 2, a, out) == E_INVALID
    assert lib.oatgpu_bsub_track_sequence_dev(ctx, seq, 2, a, None) == E_INVALID
    assert lib.oatgpu_bsub_track_sequence_dev(ctx, seq, -1, a, out) == E_INVALID
    assert "n_frames" in lib.oatgpu_last_error(ctx).decode()
    assert lib.oatgpu_bsub_track_sequence_dev(ctx, seq, 0, a, out) == 0
    assert lib.oatgpu_bsub_reset(ctx, n) == E_INVALID
    assert lib.oatgpu_bsub_get_state(ctx, n, plane(), None) == E_INVALID
    assert lib.oatgpu_read_bsub_mask(ctx, 0, MORPH, None) == E_INVALID
    assert lib.oatgpu_read_bsub_mask(ctx, n, MORPH, plane()) == E_INVALID
    assert lib.oatgpu_read_bsub_mask(ctx, 0, 7, plane()) == E_INVALID
    assert "unknown tap" in lib.oatgpu_last_error(ctx).decode()                            # last_error still speaks of this context
    # nothing of all that moved the tracker: the latest frame's planes and the state are frame 1's, and the frames go on
    for s in range(n):
        _check_taps(hp, s, want[1][s], ("after refusals", s), read=rd)
    _check_state(A, hp, want[1], "after refusals")
    for t in range(2, 5):
        _check(hp, A.SubtractionTracker.track_dev(hp, bufs[t].data_ptr(), alpha=a), want[t], ("after refusals", t), read=rd)
    _check_state(A, hp, want[4], "at the end")


@pytest.mark.parametrize("alpha", [0.0, 0.05])
def test_the_context_stays_good_for_its_other_calls(A, alpha):
    """Subtraction steps, the fused tracker's calls, oatgpu_detect_hsv and motion-tracker steps interleaved on ONE context:
    each side equals its oracle, oatgpu_read_mask shows the fused tracker's planes and oatgpu_read_bsub_mask the subtraction
    tracker's, whatever ran in between."""
    from oat_amd import ffi
    c, want = _case(90, 200, 3, 3, alpha=alpha, n_frames=12)
    n, w = c.n_streams, B.HSV_WIN
    hp = _both(A, c)
    p = O.hsv_params(h_lo=w["h"][0], h_hi=w["h"][1], s_lo=w["s"][0], s_hi=w["s"][1], v_lo=w["v"][0], v_hi=w["v"][1],
                     erode=c.erode, dilate=c.dilate, min_area=B.AREA[0], max_area=B.AREA[1])
    mogs = [O.Mog2(c.rows, c.cols, 3) for _ in range(n)]
    diffs = [O.Diff(c.rows, c.cols, 12, 2, *B.AREA) for _ in range(n)]
    bufs = [_dev(fs) for fs in c.frames]
    rd = _read_bsub(A, hp)
    bt = [0]                                    # the next frame of the subtraction side
    dt = [0]                                    # ... and of the motion tracker

    def bsub_steps(k, seq=False):
        ts = list(range(bt[0], bt[0] + k))
        got = (A.SubtractionTracker.track_sequence_dev(hp, [bufs[t].data_ptr() for t in ts], alpha=c.alpha) if seq
               else [A.SubtractionTracker.track_dev(hp, bufs[t].data_ptr(), alpha=c.alpha) for t in ts])
        for i, t in enumerate(ts):
            _check(hp, got[i], want[t], ("bsub", t), taps=i == k - 1, read=rd)
        bt[0] += k

    masks = [None] * n                          # the fused tracker's latest MORPH planes, from the oracle

    def track_steps(ts, seq=False):
        got = hp.track_sequence_dev([bufs[t].data_ptr() for t in ts]) if seq else [hp.track_dev(bufs[t].data_ptr()) for t in ts]
        for i, t in enumerate(ts):
            for s in range(n):
                wd, masks[s] = O.chain_step(mogs[s], c.frames[t][s], LR, p)
                _same_detection(got[i][s], wd, ("track", t, s))
        track_planes("track")

    def track_planes(tag):
        for s in range(n):
            assert (hp.read_mask(MORPH, s) == masks[s]).all(), (tag, s)

    def bsub_planes(tag):
        for s in range(n):
            _check_taps(hp, s, want[bt[0] - 1][s], (tag, s), read=rd)
        _check_state(A, hp, want[bt[0] - 1], tag)

    def detect_hsv(t, s):
        hsv = O.bgr2hsv(c.frames[t][s])
        pos = ffi.Position()
        hp._chk(hp.lib.oatgpu_detect_hsv(hp.ctx, s, ffi.u8(hsv), C.byref(pos)))
        _same_detection(A.Position2D.from_c(pos), O.detect_hsv(hsv, p)[0], ("detect_hsv", t, s))

    def diff_steps(k):
        for t in range(dt[0], dt[0] + k):
            got = A.MotionTracker.track_dev(hp, bufs[t].data_ptr())
            for s in range(n):
                _same_detection(got[s], diffs[s].detect(D.oracle_frame(c.frames[t][s]))[0], ("diff", t, s))
        dt[0] += k

    bsub_steps(2)
    track_steps([0, 1])
    bsub_planes("behind synchronous track steps")
    diff_steps(2)
    bsub_steps(3, seq=True)
    track_planes("behind a bsub sequence")
    track_steps([2, 3, 4, 5], seq=True)
    detect_hsv(3, 1)
    bsub_planes("behind a track sequence and a detector call")
    bsub_steps(1)
    diff_steps(1)
    track_steps([6])
    bsub_steps(4, seq=True)
    track_planes("behind the last bsub sequence")
    bsub_planes("at the end")
