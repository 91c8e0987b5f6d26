"""GPU tests of the filter chain behind the motion and the subtraction tracker (oatgpu_set_tracker_filters,
oatgpu_tracker_filtered; MotionTracker / SubtractionTracker .set_filters / .filtered; k_tracker_filters in kernels_trackfilt.hip):
`posifilt kalman` -> `posifilt homography` -> `posifilt region` on the trackers' own result records, in frame order across the
four frames in flight of the sequence calls.

Expected values come from the oracle alone (tests/tracker_filters_cases.py): the oracle detection per stream and frame, then
marker_filters_ref.chain with one oracle_lib.Kalman per stream.  Every filtered record is compared on every frame, valid or not:
flags and region name equal, x / y / vx / vy equal as doubles (==), hx = hy = 0; the sign of a zero is not pinned.  The detections
in front of the chain are held to the oracle too.  Every frame is under 0.01 MP."""
import ctypes as C

import numpy as np
import pytest

import bsub_cases as BC
import debayer_ref as DR
import diff_cases as DC
import tracker_filters_cases as K
import undistort_ref as UR
from parity_asserts import _same_detection, _same_double

pytestmark = pytest.mark.gpu

E_INVALID = -1
KINDS = ("diff", "bsub")


@pytest.fixture(scope="module")
def A():
    import oat_amd
    return oat_amd


def _dev(frames):
    import torch
    t = torch.from_numpy(np.stack(frames)).cuda()
    torch.cuda.synchronize()
    return t


def _tracker(A, kind, rows, cols, ch, n, **kw):
    if kind == "diff":
        return A.MotionTracker(rows, cols, n_streams=n, channels=ch, area=DC.AREA, **K.DIFF, **kw)
    return A.SubtractionTracker(rows, cols, **K.bsub_case(rows, cols, ch, n).tracker_args(), **kw)


def _same_filtered(got, want, tag):
    """(Not test_marker_filters_gpu's: a detector publishes no heading, so heading_valid, hx and hy are held to False, 0, 0
    whatever the expected record says, where the marker chain's are compared with it.)"""
    assert (got.position_valid, got.velocity_valid, got.heading_valid, got.region_valid, got.region) == \
        (want["position_valid"], want["velocity_valid"], False, want["region_valid"], want["region"]), (tag, got, want)
    for k in ("x", "y", "vx", "vy"):
        assert _same_double(getattr(got, k), want[k]), (tag, k, got, want)
    assert got.hx == 0.0 and got.hy == 0.0, (tag, got)


def _same_set(got, want_t, tag):
    assert len(got) == len(want_t)
    for s, (g, w) in enumerate(zip(got, want_t)):
        _same_filtered(g, w, (tag, s))


def _same_front(got, det_t, tag):
    for s, (g, w) in enumerate(zip(got, det_t)):
        _same_detection(g, w, (tag, s))


def _run(tr, fr, det, want, calls, tag):
    """fr[t][s] through the calls [(form, t0, t1)]: "host" / "dev" one frame a call, "seq" one sequence call; every record checked"""
    for form, t0, t1 in calls:
        if form == "seq":
            bufs = [_dev(fr[t]) for t in range(t0, t1)]
            pos = tr.track_sequence_dev([b.data_ptr() for b in bufs])
            sets = tr.filtered()
            assert len(sets) == len(pos) == t1 - t0
            for i, t in enumerate(range(t0, t1)):
                _same_front(pos[i], det[t], (tag, form, t))
                _same_set(sets[i], want[t], (tag, form, t))
            continue
        for t in range(t0, t1):
            if form == "dev":
                buf = _dev(fr[t])
                pos = tr.track_dev(buf.data_ptr())
            else:
                pos = tr.track(fr[t])
            sets = tr.filtered()
            assert len(sets) == 1 and sets == tr.filtered()                  # nothing is consumed
            _same_front(pos, det[t], (tag, form, t))
            _same_set(sets[0], want[t], (tag, form, t))


def _batch(form, n_frames=K.T):
    return [(form, 0, n_frames)]


# sequence calls of 1, 2, 5 and 11 frames (11 wraps the four slots more than twice, with an odd tail; single and paired front
# launches), batch calls and sequence calls continuing one filter
SPLITS = {
    "host": _batch("host"),
    "dev": _batch("dev"),
    "seq-1-2-11": [("seq", 0, 1), ("seq", 1, 3), ("seq", 3, 14)],
    "seq-5-dev-host-seq": [("seq", 0, 5), ("dev", 5, 6), ("host", 6, 7), ("seq", 7, 9), ("seq", 9, 14)],
    "seq-11-3": [("seq", 0, 11), ("seq", 11, 14)],
}


@pytest.mark.parametrize("name", K.CONFIGS)
@pytest.mark.parametrize("rows, cols, ch", K.GEOMETRIES)
@pytest.mark.parametrize("kind", KINDS)
def test_every_member_on_every_form(A, kind, rows, cols, ch, name):
    n = 3
    fr, det = K.frames(kind, rows, cols, ch, n), K.detections(kind, rows, cols, ch, n)
    cfg, want = K.config(name, kind, rows, cols, ch, n), K.want(name, kind, rows, cols, ch, n)
    for split, calls in SPLITS.items():
        tr = _tracker(A, kind, rows, cols, ch, n)
        try:
            tr.set_filters(**cfg)
            _run(tr, fr, det, want, calls, (name, split))
        finally:
            tr.close()


@pytest.mark.parametrize("n", [1, 66])
@pytest.mark.parametrize("kind", KINDS)
def test_one_stream_and_two_workgroups_of_streams(A, kind, n):
    rows, cols, ch = K.MANY if n == 66 else K.GEOMETRIES[0]
    T = 12
    fr, det = K.frames(kind, rows, cols, ch, n, T), K.detections(kind, rows, cols, ch, n, T)
    for name in ("all", "k_short"):
        cfg, want = K.config(name, kind, rows, cols, ch, n, T), K.want(name, kind, rows, cols, ch, n, T)
        for calls in ([("seq", 0, 1), ("seq", 1, 12)], [("dev", 0, 2), ("seq", 2, 7), ("host", 7, 8), ("seq", 8, 12)]):
            tr = _tracker(A, kind, rows, cols, ch, n)
            try:
                tr.set_filters(**cfg)
                _run(tr, fr, det, want, calls, (name, n))
            finally:
                tr.close()


@pytest.mark.parametrize("kind", KINDS)
def test_the_setter_restarts_the_filter_in_the_middle(A, kind):
    rows, cols, ch = K.GEOMETRIES[0]
    n, cut = 3, 6
    fr, det = K.frames(kind, rows, cols, ch, n), K.detections(kind, rows, cols, ch, n)
    cfg = K.config("all", kind, rows, cols, ch, n)
    other = dict(kalman=K.P.kw("below_3"), homography=K.HOMOGRAPHIES["h_projective"], regions=None)
    first = K.chain_run(det[:cut], kind=kind, **cfg)
    second = K.chain_run(det[cut:], kind=kind, **cfg)                        # the detector goes on, the filter starts again
    third = K.chain_run(det[cut:], kind=kind, **other)
    assert K.differs(second, K.chain_run(det, kind=kind, **cfg)[cut:])
    for tail_cfg, tail in ((cfg, second), (other, third)):
        tr = _tracker(A, kind, rows, cols, ch, n)
        try:
            tr.set_filters(**cfg)
            _run(tr, fr, det, first + [None] * (K.T - cut), [("seq", 0, 4), ("dev", 4, cut)], "before")
            tr.set_filters(**tail_cfg)
            with pytest.raises(A.OatGpuError):                               # nothing delivered since it was configured
                tr.filtered()
            _run(tr, fr, det, [None] * cut + tail, [("dev", cut, cut + 1), ("seq", cut + 1, K.T)], "after")
        finally:
            tr.close()


@pytest.mark.parametrize("kind", KINDS)
def test_chain_through_reset_raw8_and_undistorted_steps(A, kind):
    """reset, oatgpu_set_tracker_bayer and oatgpu_set_tracker_undistort change what the detector sees, never the filter state"""
    rows, cols, ch = K.GEOMETRIES[0]
    n = 3
    fr = K.frames(kind, rows, cols, ch, n)
    cal = UR.cases(rows, cols)["mild5"]
    maps = UR.undistort_map(rows, cols, *cal)
    pats = (DR.RGGB, DR.GRBG, DR.BGGR)
    raw8, und = (4, 5, 10), (6, 7, 8, 12)
    refs = [K.DetRef(kind, rows, cols, ch) for _ in range(n)]
    given, det = [], []
    for t in range(K.T):
        if t == 3:
            for r in refs:
                r.reset()
        if t in raw8:
            given.append([DR.mosaic(f, pats[s]) for s, f in enumerate(fr[t])])
            seen = [DR.demosaic(g, pats[s]) for s, g in enumerate(given[t])]
        else:
            given.append(fr[t])
            seen = [UR.remap(f, *maps) for f in fr[t]] if t in und else fr[t]
        det.append([refs[s].step(seen[s]) for s in range(n)])
    cfg = dict(kalman=K.P.kw(K.ALL_ROW), homography=K.HOMOGRAPHIES["h_affine"], regions=K.regions_for(
        K.chain_run(det, kalman=K.P.kw(K.ALL_ROW), homography=K.HOMOGRAPHIES["h_affine"])))
    want = K.chain_run(det, kind=kind, **cfg)
    assert sum(w["position_valid"] and not d["valid"] for ws, ds in zip(want, det) for w, d in zip(ws, ds)) >= 3
    assert sum(d["valid"] for ds in det[3:] for d in ds) >= 12
    tr = _tracker(A, kind, rows, cols, ch, n)
    try:
        tr.set_filters(**cfg)
        for s in range(n):
            tr.set_undistort(s, *cal)
        for t in range(K.T):
            if t == 3:
                tr.reset()
            tr.bayer(pats if t in raw8 else None)
            tr.undistort(t in und)
            form = ("dev", "host", "seq")[t % 3]
            _run(tr, given, det, want, [(form, t, t + 1)], "in turn")
    finally:
        tr.close()


@pytest.mark.parametrize("kind", KINDS)
def test_positions_and_taps_are_the_same_with_the_chain_on_and_off(A, kind):
    rows, cols, ch = K.GEOMETRIES[1]
    n = 3
    fr = K.frames(kind, rows, cols, ch, n)
    on, off = _tracker(A, kind, rows, cols, ch, n), _tracker(A, kind, rows, cols, ch, n)
    try:
        on.set_filters(**K.config("all", kind, rows, cols, ch, n))

        def both(t0, t1, seq):
            bufs = [_dev(fr[t]) for t in range(t0, t1)]
            if seq:
                a, b = (x.track_sequence_dev([u.data_ptr() for u in bufs]) for x in (on, off))
            else:
                a, b = (x.track_dev(bufs[0].data_ptr()) for x in (on, off))
            assert a == b, (t0, t1)
            for which in (0, 1, 2):
                for s in range(n):
                    assert (on.read_mask(which, s) == off.read_mask(which, s)).all(), (t0, which, s)

        both(0, 1, False)
        both(1, 6, True)
        both(6, 7, False)
        both(7, K.T, True)
        with pytest.raises(A.OatGpuError):
            off.filtered()
    finally:
        on.close()
        off.close()


def _hotpath(A, rows, cols, n):
    """A context with the fused tracker, a marker set and both batched trackers (their methods serve any context); its own
    window is the non-zero window a marker step asks for."""
    hp = A.HotPath(rows, cols, n_streams=n, adaptation_coeff=0.01, erode=0, dilate=3, area=DC.AREA, h_thresh=(0, 256),
                   s_thresh=(0, 256), v_thresh=(1, 256), **K.DIFF)
    hp._chk(hp.lib.oatgpu_set_diff_tracker(hp.ctx, 1))
    hp._chk(hp.lib.oatgpu_set_bsub_tracker(hp.ctx, 1))
    hp.set_markers([dict(h=(0, 256), s=(0, 256), v=(100, 256), dilate=3, area=DC.AREA)])
    return hp


def test_refusals_leave_the_context_and_the_chain_as_they_were(A):
    from oat_amd import ffi
    rows, cols, ch = K.GEOMETRIES[0]
    n = 3
    fr, det = K.frames("diff", rows, cols, ch, n), K.detections("diff", rows, cols, ch, n)
    cfg, want = K.config("all", "diff", rows, cols, ch, n), K.want("all", "diff", rows, cols, ch, n)
    hp = _hotpath(A, rows, cols, n)
    lib, ctx = hp.lib, hp.ctx
    M = A.MotionTracker
    bufs = [_dev(f) for f in fr]
    out, filt = (ffi.Position * n)(), (ffi.Filtered * (4 * n))()

    def refused(rc, text, whole=True):
        """whole: the complete message, as the source before the setters and getters had one body printed it"""
        assert rc == E_INVALID
        msg = lib.oatgpu_last_error(ctx).decode()
        assert msg == text if whole else text in msg, msg

    def chain(**kw):
        return C.byref(A.components._filter_chain(kw.get("kalman"), kw.get("homography"), kw.get("regions"))[0])

    sq = [(0, 0), (10, 0), (10, 10), (0, 10)]
    try:
        refused(lib.oatgpu_tracker_filtered(ctx, filt, 4), "no filter chain is configured (oatgpu_set_tracker_filters)")
        M.set_filters(hp, **cfg)
        refused(lib.oatgpu_tracker_filtered(ctx, filt, 4), "no tracker call has run since the filter chain was configured")
        for t in range(3):
            _same_front(M.track_dev(hp, bufs[t].data_ptr()), det[t], t)
            _same_set(M.filtered(hp)[0], want[t], t)
        # the limits, a bad parameter, results outstanding, a partly staged set: nothing changes
        for bad in (dict(kalman=dict(dt=0.0)), dict(kalman=dict(dt=0.02, timeout=-1.0)), dict(kalman=dict(sigma_accel=-1.0)),
                    dict(kalman=dict(sigma_noise=float("nan")))):
            f, _, keep = A.components._filter_chain(bad["kalman"], None, None)
            refused(lib.oatgpu_set_tracker_filters(ctx, C.byref(f)), "kalman: dt must be > 0, timeout / sigma-accel / sigma-noise >= 0")
        for regions, text in (([(f"r{i}", sq) for i in range(17)], "at most 16 regions (got 17)"),
                              ([("a", [(i, i * i % 7) for i in range(65)])], "region 0 (a): at most 64 points (got 65)"),
                              ([("tenletters", sq)], "region 0: a name takes at most 9 bytes"),
                              ([("a", [(0, 0), (40000, 0), (10, 10)])], "region 0 (a): point 1 is beyond +-32767")):
            f, _, keep = A.components._filter_chain(None, None, regions)
            refused(lib.oatgpu_set_tracker_filters(ctx, C.byref(f)), text)
        f, _, keep = A.components._filter_chain(cfg["kalman"], None, None)
        hp.enqueue_dev(bufs[0].data_ptr(), keepalive=bufs[0])
        refused(lib.oatgpu_set_tracker_filters(ctx, C.byref(f)), "set_tracker_filters while enqueued results are outstanding")
        refused(lib.oatgpu_set_tracker_filters(ctx, None), "set_tracker_filters while enqueued results are outstanding")
        hp.collect()
        hp.stage(0, fr[0][0])
        refused(lib.oatgpu_set_tracker_filters(ctx, C.byref(f)), "set_tracker_filters while enqueued results are outstanding")
        hp.stage_abort()
        # oatgpu_set_kalman / oatgpu_set_homography keep their meaning: the tracker calls stay refused while they are on
        arr = (C.c_void_p * 1)(bufs[3].data_ptr())
        hp.set_kalman(True)
        refused(lib.oatgpu_diff_batch_dev(ctx, C.c_void_p(bufs[3].data_ptr()), out), "oatgpu_set_kalman", whole=False)
        refused(lib.oatgpu_diff_sequence_dev(ctx, arr, 1, out), "oatgpu_set_kalman", whole=False)
        refused(lib.oatgpu_bsub_track_batch_dev(ctx, C.c_void_p(bufs[3].data_ptr()), 0.0, out), "oatgpu_set_kalman", whole=False)
        hp.set_kalman(False)
        hp.set_homography(K.HOMOGRAPHIES["h_affine"])
        refused(lib.oatgpu_diff_batch_dev(ctx, C.c_void_p(bufs[3].data_ptr()), out), "oatgpu_set_homography", whole=False)
        hp.set_homography(None)
        # the latest sets are still frame 2's; too little room is refused, nothing is consumed
        assert lib.oatgpu_tracker_filtered(ctx, filt, 1) == 1
        hp._tf_sets = 1
        _same_set(M.filtered(hp)[0], want[2], "kept")
        seq = M.track_sequence_dev(hp, [b.data_ptr() for b in bufs[3:7]])
        _same_front(seq[3], det[6], 6)
        refused(lib.oatgpu_tracker_filtered(ctx, filt, 3), "room for 3 frame sets, the latest call delivered 4")
        sets = M.filtered(hp)
        for i in range(4):
            _same_set(sets[i], want[3 + i], ("through the refusals", 3 + i))  # the chain went through every refusal untouched
        # switched off: freed, and the getter says so; the tracker goes on
        M.set_filters(hp)
        refused(lib.oatgpu_tracker_filtered(ctx, filt, 4), "no filter chain is configured (oatgpu_set_tracker_filters)")
        assert lib.oatgpu_set_tracker_filters(ctx, None) == 0
        _same_front(M.track_dev(hp, bufs[7].data_ptr()), det[7], 7)
    finally:
        hp.close()


@pytest.mark.parametrize("kind", KINDS)
def test_the_other_calls_of_the_context_never_look_at_the_chain(A, kind):
    """twin contexts, one with a chain: the MOG2 track call and a marker step before, between and after tracker steps are the same"""
    rows, cols, ch = K.GEOMETRIES[0]
    n = 3
    fr = K.frames(kind, rows, cols, ch, n)
    a, b = _hotpath(A, rows, cols, n), _hotpath(A, rows, cols, n)
    Tr = A.MotionTracker if kind == "diff" else A.SubtractionTracker
    try:
        Tr.set_filters(a, **K.config("all", kind, rows, cols, ch, n))
        valid = 0
        for t in range(K.T):
            assert a.track(fr[t]) == b.track(fr[t]), t
            if t % 3 == 0:
                assert a.track_markers(fr[t]) == b.track_markers(fr[t]), t
            if t % 2:
                buf = _dev(fr[t])
                pa, pb = (Tr.track_dev(x, buf.data_ptr(), *((0.0,) if kind == "bsub" else ())) for x in (a, b))
            else:
                pa, pb = (Tr.track(x, fr[t], *((0.0,) if kind == "bsub" else ())) for x in (a, b))
            assert pa == pb, t
            got = Tr.filtered(a)[0]
            valid += sum(g.position_valid for g in got)
            for g, p in zip(got, pa):                                         # no Kalman bridge yet: a valid detection is tracked
                assert g.position_valid or not p.position_valid
        assert valid >= 2 * n
    finally:
        a.close()
        b.close()
