"""GPU tests of the two batched trackers' BACK half on frames over the capacity of the blob stage's LDS kernel: the motion
tracker (oatgpu_diff_*; MotionTracker) and the subtraction tracker (oatgpu_bsub_track_*; SubtractionTracker) on the frame
sequences of tests/busy_tracker_cases.py, whose final masks sit at k_blob_lds' capacity or one over it, so that the global
union-find (k_merge + k_green_select) runs at these call sites: launches with first_stream != 0 (diff_back), planes of the
trackers' own in place of the scratch set's, slots of the in-flight sequence that alternate between the two routes, and
scratch set 0 shared with the context's ordinary calls.

Everything is exact: detections as parity_asserts._same_detection compares them (a00, a10, a01, first_pixel, valid and the
position), and on every frame whose planes can be read the FINAL tap equals the expected final mask bit for bit and
blob_load OF THE TAP THAT CAME BACK names the scheduled route (_check) -- a test cannot pass while staying on `lds`.
tests/test_busy_trackers_cpu.py holds the cases to the models and the oracle.  Every frame is under 0.1 MP but the area cases'
(blob_load.edge_cases(): 160 x 1000 and 40 x 1000, one stream)."""
import collections

import numpy as np
import pytest

import bsub_cases as B
import busy_tracker_cases as K
import oracle_lib as O
from parity_asserts import _same_detection

pytestmark = pytest.mark.gpu

THR, MORPH, FIN = 0, 1, 2
ROUTES = collections.defaultdict(collections.Counter)      # group -> frames checked on each route


@pytest.fixture(scope="module")
def A():
    import oat_amd
    yield oat_amd
    for group, c in sorted(ROUTES.items()):
        print(f"\n[busy trackers] {group}: {c['global']} frames global, {c['lds']} frames lds", end="")
    print()


def _dev(frames):
    """[n_streams] host frames -> a stream-major device tensor (kept by the caller while the library reads it)."""
    import torch
    t = torch.from_numpy(np.stack(frames)).cuda()
    torch.cuda.synchronize()
    return t


def _check(tr, got, st, tag, group, taps=True, read=None):
    """One frame set against the oracle; with taps, the FINAL tap read back from the library against the expected final mask,
    and blob_load of THAT TAP against the scheduled route."""
    read = read or tr.read_mask
    assert len(got) == len(st.want)
    for s, want in enumerate(st.want):
        _same_detection(got[s], want, (tag, s, st.kinds[s]))
        if taps:
            fin = read(FIN, s)
            assert set(np.unique(fin)) <= {0, 255}, (tag, s)
            assert ((fin != 0) == st.final[s]).all(), ("final tap", tag, s, st.kinds[s])
            route = K.load_of(fin)["path"]
            assert route == st.path[s], ("route of the tap that came back", tag, s, st.kinds[s], route)
        ROUTES[group][st.path[s]] += 1


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _check_state(A, tr, st, tag):
    """oatgpu_bsub_get_state against the model behind the frame: background bytes and accumulator bit patterns"""
    if st.state is None:
        return
    for s, (bg, acc) in enumerate(st.state):
        gbg, gacc = A.SubtractionTracker.state(tr, s, acc=acc is not None)
        assert _same_bits(gbg, bg), ("background", tag, s)
        if acc is not None:
            assert _same_bits(gacc, acc), ("accumulator", tag, s)


def _motion(A, rows, cols, ch, n, blur=0, area=K.AREA, bayer=None):
    return A.MotionTracker(rows, cols, n_streams=n, channels=ch, diff_threshold=K.THR, blur=blur, area=area,
                           bayer=None if bayer is None else list(bayer))


def _subtraction(A, run):
    st = A.SubtractionTracker(run.rows, run.cols, bayer=None if run.patterns is None else list(run.patterns), **run.tracker_args())
    if run.preset:
        for s in range(run.n):
            st.set_background(run.background, stream=s)
    return st


def _standard(A, tracker, rows, cols, ch, n, alpha=0.0):
    """-> (steps, a function that makes a fresh tracker for them)"""
    if tracker == "diff":
        return K.diff_standard(rows, cols, ch, n), lambda: _motion(A, rows, cols, ch, n)
    run, steps = K.bsub_standard(rows, cols, ch, n, alpha)
    return steps, lambda: _subtraction(A, run)


# ------------------------------------------------------------------------------------------ the synchronous step ----

@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("ch", [3, 1])
@pytest.mark.parametrize("rows,cols", K.SHAPES)
@pytest.mark.parametrize("tracker", ["diff", "bsub"])
def test_synchronous_steps_on_device_and_host_frames(A, tracker, rows, cols, ch, n):
    steps, make = _standard(A, tracker, rows, cols, ch, n)
    dev, host = make(), make()
    assert len(steps) >= 16
    for st in steps:
        buf = _dev(st.frames)
        _check(dev, dev.track_dev(buf.data_ptr()), st, ("dev", st.t), f"synchronous {tracker}")
        _check(host, host.track(st.frames), st, ("host", st.t), f"synchronous {tracker}")
    _check_state(A, dev, steps[-1], "dev")


# ------------------------------------------------------------ mixed first-frame state on the global route (motion) ----

@pytest.mark.parametrize("blur", [0, 2])
@pytest.mark.parametrize("n", [3, 5])
def test_motion_tracker_launches_behind_the_first_on_the_global_route(A, n, blur):
    """Busy masks on every stream; streams reset before a step, so that diff_back issues two to four launches with
    first_stream 0, 1, 2, ... -- the pattern with only the last stream fresh among them.  blur 2: the two kinds of launch
    differ in their dilation."""
    mt = _motion(A, *K.MANY, 3, n, blur)
    launches = set()
    for resets, st in K.diff_mixed(n, blur):
        for s in resets:
            mt.reset(s)
        assert st.path == ["global"] * n
        launches |= set(K.launches(st.first))
        buf = _dev(st.frames)
        _check(mt, mt.track_dev(buf.data_ptr()), st, ("mixed", n, blur, st.t, resets), "mixed first-frame state (diff)")
    assert {s0 for s0, _ in launches} == set(range(n))


# ----------------------------------------------------------------------------------------------- the sequence call ----

def _sequence(A, steps, make, before, n_frames, group):
    """`before` synchronous steps, then n_frames in one sequence call: every result against the oracle, the planes and the
    state behind the call the last frame's; the same frames one by one through a second tracker -- against the oracle, with
    every frame's tap and route -- and the two trackers against each other; one more step on both."""
    seq, one = make(), make()
    last = before + n_frames
    assert last < len(steps)
    bufs = [_dev(st.frames) for st in steps[:last + 1]]
    for t in range(before):
        _check(seq, seq.track_dev(bufs[t].data_ptr()), steps[t], ("before", t), group)
        one.track_dev(bufs[t].data_ptr())
    got = seq.track_sequence_dev([bufs[t].data_ptr() for t in range(before, last)])
    assert len(got) == n_frames
    for i, t in enumerate(range(before, last)):
        _check(seq, got[i], steps[t], ("sequence", t), group, taps=t == last - 1)     # read_*_mask shows the last frame
    _check_state(A, seq, steps[last - 1], "behind the sequence")
    ref = []
    for t in range(before, last):
        ref.append(one.track_dev(bufs[t].data_ptr()))
        _check(one, ref[-1], steps[t], ("one by one", t), group)
    assert got == ref
    for s in range(len(steps[0].want)):
        for which in (THR, MORPH, FIN):
            assert (seq.read_mask(which, s) == one.read_mask(which, s)).all(), (which, s)
    _check(seq, seq.track_dev(bufs[last].data_ptr()), steps[last], "next", group)
    _check(one, one.track_dev(bufs[last].data_ptr()), steps[last], "next, one by one", group)
    _check_state(A, seq, steps[last], "next")


@pytest.mark.parametrize("before", [0, 3], ids=["fresh", "continuing"])
@pytest.mark.parametrize("n_frames", [5, 8, 12, 13])
@pytest.mark.parametrize("ch", [3, 1])
@pytest.mark.parametrize("tracker,alpha", [("diff", 0.0), ("bsub", 0.0), ("bsub", 0.05)])
def test_sequences_on_the_standard_schedule(A, tracker, alpha, ch, n_frames, before):
    """Four frames in flight in slots t % 4, back halves on three streams, paired front launches: a slot alternates between
    the two routes while its neighbours run.  bsub at alpha 0.05 is the noise form (busy frames of 50 % salt)."""
    rows, cols = K.SHAPES[0] if ch == 3 else K.SHAPES[1]
    steps, make = _standard(A, tracker, rows, cols, ch, 3, alpha)
    _sequence(A, steps, make, before, n_frames, f"sequences {tracker}" + (" (noise form)" if alpha else ""))


@pytest.mark.parametrize("tracker", ["diff", "bsub"])
def test_sequence_with_a_stream_reset_in_front(A, tracker):
    """Stream 1 is reset ahead of the sequence: an unpaired first launch (motion tracker: two runs of the back half, launches
    with first_stream 0, 1 and 2) precedes the paired ones."""
    r = K.RESET_FRONT
    if tracker == "diff":
        steps, make = K.diff_reset_in_front(3), lambda: _motion(A, *K.SHAPES[0], 3, 3)
    else:
        run, steps = K.bsub_reset_in_front(3)
        make = lambda: _subtraction(A, run)                                                     # noqa: E731
    seq, one = make(), make()
    bufs = [_dev(st.frames) for st in steps]
    group = f"reset in front ({tracker})"
    for t in range(r["before"]):
        _check(seq, seq.track_dev(bufs[t].data_ptr()), steps[t], ("before", t), group)
        one.track_dev(bufs[t].data_ptr())
    seq.reset(r["reset"])
    one.reset(r["reset"])
    span = range(r["before"], r["before"] + r["n_frames"])
    assert steps[span[0]].first == [False, True, False]
    got = seq.track_sequence_dev([bufs[t].data_ptr() for t in span])
    ref = []
    for i, t in enumerate(span):
        _check(seq, got[i], steps[t], ("sequence", t), group, taps=t == span[-1])
        ref.append(one.track_dev(bufs[t].data_ptr()))
        _check(one, ref[-1], steps[t], ("one by one", t), group)
    assert got == ref
    _check_state(A, seq, steps[span[-1]], "behind the sequence")


@pytest.mark.parametrize("tracker", ["diff", "bsub"])
def test_raw8_sequence_puts_the_paired_front_launch_ahead_of_global_back_halves(A, tracker):
    """The noise form behind the demosaic (bit-identity of the RAW8 front end has tests of its own): a synchronous step, then
    a sequence whose launches are paired."""
    if tracker == "diff":
        run, steps = K.diff_raw()
        make = lambda: _motion(A, run.rows, run.cols, 3, run.n, run.blur, bayer=run.patterns)   # noqa: E731
    else:
        run, steps = K.bsub_raw()
        make = lambda: _subtraction(A, run)                                                     # noqa: E731
    assert sum(p == "global" for st in steps[1:-1] for p in st.path) >= 10
    _sequence(A, steps, make, 1, len(steps) - 2, f"RAW8 ({tracker})")


# --------------------------------------------------------------------------------------------------- 66 streams ----

@pytest.mark.parametrize("tracker", ["diff", "bsub"])
def test_sixty_six_streams_with_the_busy_ones_around_the_front_kernels_split(A, tracker):
    """The front kernel's first-frame flags split a launch at 64 streams, the back half covers all 66 in one grid: streams 0,
    63, 64 and 65 are over capacity (runs and roots), 1 and 62 at capacity, the others carry a rectangle each.  One synchronous
    step, then a 6-frame sequence."""
    if tracker == "diff":
        steps, mt = K.diff_many(), _motion(A, *K.MANY, 3, K.N_MANY)
    else:
        run, steps = K.bsub_many()
        mt = _subtraction(A, run)
    group = f"66 streams ({tracker})"
    bufs = [_dev(st.frames) for st in steps]
    _check(mt, mt.track_dev(bufs[0].data_ptr()), steps[0], "step", group)
    got = mt.track_sequence_dev([b.data_ptr() for b in bufs[1:]])
    assert len(got) == 6
    for i, st in enumerate(steps[1:]):
        _check(mt, got[i], st, ("sequence", st.t), group, taps=i == 5)
    _check_state(A, mt, steps[-1], group)


# ------------------------------------------------------------------------- ties and the area window over capacity ----

@pytest.mark.parametrize("ch", [3, 1])
@pytest.mark.parametrize("name", ["ties", "max_area_equal", "max_area_under", "min_area_equal"])
@pytest.mark.parametrize("tracker", ["diff", "bsub"])
def test_ties_and_the_area_window_on_the_global_route(A, tracker, name, ch):
    """769 components: the tie between hundreds of equal areas goes to the later first pixel; the one real blob shut out by
    max_area (strict) leaves the empty answer.  One synchronous step of each tracker."""
    mask, area = K.area_cases()[name]
    if tracker == "diff":
        st, tr = K.diff_area(name, ch), _motion(A, *mask.shape, ch, 1, area=area)
    else:
        run, st = K.bsub_area(name, ch)
        tr = _subtraction(A, run)
    assert st.path == ["global"] and st.want[0]["valid"] == (name in ("ties", "min_area_equal"))
    buf = _dev(st.frames)
    _check(tr, tr.track_dev(buf.data_ptr()), st, (name, "dev"), f"area window ({tracker})")
    tr2 = _motion(A, *mask.shape, ch, 1, area=area) if tracker == "diff" else _subtraction(A, run)
    _check(tr2, tr2.track(st.frames), st, (name, "host"), f"area window ({tracker})")


# ---------------------------------------------------------------------- one context, every user of scratch set 0 ----

LR = 0.001      # a painted pixel stays foreground for ~100 frames: the fused tracker's masks are exactly the painted masks


def test_one_context_and_every_user_of_scratch_set_zero(A):
    """The fused tracker (oatgpu_track_batch), oatgpu_detect_thresh, oatgpu_detect_hsv and the two batched trackers in turn on
    ONE context, busy calls of one form beside quiet ones of another (busy_tracker_cases.SHARED_OPS): each equals its own
    oracle, and no tracker step changes a bit of what oatgpu_read_mask shows."""
    rows, cols = K.SHARED_SHAPE
    n, w = K.SHARED_N, B.HSV_WIN
    hp = A.HotPath(rows, cols, n_streams=n, adaptation_coeff=LR, erode=0, dilate=0, area=K.AREA, h_thresh=w["h"], s_thresh=w["s"],
                   v_thresh=w["v"], diff_threshold=K.THR, blur=0)
    hp._chk(hp.lib.oatgpu_set_diff_tracker(hp.ctx, 1))
    hp._chk(hp.lib.oatgpu_set_bsub_tracker(hp.ctx, 1))
    run, steps = K.shared_steps()
    for s in range(n):
        A.SubtractionTracker.set_background(hp, run.background, stream=s)
    p = O.hsv_params(h_lo=w["h"][0], h_hi=w["h"][1], s_lo=w["s"][0], s_hi=w["s"][1], v_lo=w["v"][0], v_hi=w["v"][1],
                     erode=0, dilate=0, min_area=K.AREA[0], max_area=K.AREA[1])
    mogs = [O.Mog2(rows, cols, 3) for _ in range(n)]
    rng = np.random.default_rng(5)
    base = rng.integers(90, 150, (n, rows, cols, 3)).astype(np.int16)
    masks = K.shared_masks()
    colour = B.INSIDE_BGR                        # inside the window as a difference and as a colour of its own
    group = "shared scratch set 0"

    def ordinary(i, s, got, want, thr):
        mask = masks[i][s]
        assert ((thr != 0) == mask).all(), (i, s)
        _same_detection(got, want, (i, K.SHARED_OPS[i], s))
        fin = hp.read_mask(FIN, s)
        assert ((fin != 0) == mask).all(), ("final tap", i, s)
        route = K.load_of(fin)["path"]
        assert route == K.DECLARED[K.SHARED_OPS[i][1][s]], (i, s, route)
        ROUTES[group + ", ordinary calls"][route] += 1

    def planes():
        return [hp.read_mask(which, s) for s in range(n) for which in (THR, MORPH, FIN)]

    for i, (op, kinds) in enumerate(K.SHARED_OPS):
        if op == "track":
            f = np.clip(base + rng.integers(-5, 6, base.shape), 0, 255).astype(np.uint8)
            for s in range(n):
                f[s][masks[i][s]] = colour
            got = hp.track(list(f))
            for s in range(n):
                want, thr = O.chain_step(mogs[s], f[s], LR, p)
                ordinary(i, s, got[s], want, thr)
        elif op == "detect_thresh":
            s = next(s for s, k in enumerate(kinds) if k is not None)
            grey = np.where(masks[i][s], 50, 0).astype(np.uint8)       # -T is the context's h window
            want, thr = O.detect_thresh(grey, p)
            ordinary(i, s, hp.detect_thresh(grey, s), want, thr)
        elif op == "detect_hsv":
            s = next(s for s, k in enumerate(kinds) if k is not None)
            bgr = np.zeros((rows, cols, 3), np.uint8)
            bgr[masks[i][s]] = colour
            hsv = O.bgr2hsv(bgr)
            want, thr = O.detect_hsv(hsv, p)
            ordinary(i, s, hp.detect_hsv(hsv, s), want, thr)
        else:
            T = A.MotionTracker if op == "diff" else A.SubtractionTracker
            before = planes()
            buf = _dev(steps[i].frames)
            got = T.track_dev(hp, buf.data_ptr())
            _check(hp, got, steps[i], (i, op), group, read=lambda which, s: T.read_mask(hp, which, s))
            for x, y in zip(before, planes()):
                assert _same_bits(x, y), ("oatgpu_read_mask behind a tracker step", i, op)
    hp.close()
