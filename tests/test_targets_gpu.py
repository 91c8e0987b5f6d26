"""GPU tests of multi-target detection (oatgpu_set_targets / oatgpu_targets; _Detector.set_targets / .targets; k_blob_rank in
kernels_blob.hip).  Every rank of every frame and every n_found is compared, bit for bit, with the reference ranking
of tests/targets_cases.py (the oracle's contours of the oracle's own mask); rank 0 with the call's ordinary result; and the
ordinary results, taps, models, states and filtered records with those of a second context that never had targets on.  Every frame
is under 0.02 MP except the launch-order test (3 x 1080p, no oracle)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import targets_cases as T
from diff_cases import same_dict

pytestmark = pytest.mark.gpu

E_INVALID = -1
THR, MORPH, FIN = 0, 1, 2


@pytest.fixture(scope="module")
def A():
    import oat_amd
    import oat_amd.components as comp
    for name in ("SimpleThreshold", "HSVDetector", "DifferenceDetector"):
        if not hasattr(oat_amd, name):
            setattr(oat_amd, name, getattr(comp, name))
    return oat_amd


def _dev(frames):
    import torch
    t = torch.from_numpy(np.stack(frames)).cuda()
    torch.cuda.synchronize()
    return t


def _as_dict(p):
    return dict(valid=p.position_valid, area=p.area, a00=p.a00, a10=p.a10, a01=p.a01, first_pixel=p.first_pixel, x=p.x, y=p.y)


def _check_stream(got, ref, tag, ordinary=None):
    """got = (ranks, n_found) of one camera of one set; ref likewise, as dicts"""
    ranks, n_found = got
    assert n_found == ref[1], (tag, n_found, ref[1])
    assert len(ranks) == len(ref[0]), tag
    for j, (g, w) in enumerate(zip(ranks, ref[0])):
        assert same_dict(_as_dict(g), w), (tag, j, g, w)
        if not w["valid"]:
            assert not g.position_valid and g.first_pixel == -1, (tag, j, g)
        assert not g.velocity_valid, (tag, j)
    if ordinary is not None:                      # rank 0 is the call's ordinary result (no Kalman filter, no homography here)
        assert ranks[0] == ordinary, (tag, ranks[0], ordinary)


def _refused(fn, *a):
    from oat_amd.ffi import OatGpuError
    with pytest.raises(OatGpuError) as e:
        fn(*a)
    assert e.value.code == E_INVALID, e.value
    return str(e.value)


# ------------------------------------------------------------------------ planted masks through the single-stage detectors ----

PLANTED = T.planted_cases()


def _detector(A, kind, case, morph, n_streams=1):
    if kind == "thresh":
        return A.SimpleThreshold(case.rows, case.cols, thresh=(255, 256), erode=morph[0], dilate=morph[1], area=case.area, n_streams=n_streams)
    if kind == "hsv":
        return A.HSVDetector(case.rows, case.cols, h_thresh=(255, 256), s_thresh=(255, 256), v_thresh=(255, 256), erode=morph[0],
                             dilate=morph[1], area=case.area, n_streams=n_streams)
    return A.DifferenceDetector(case.rows, case.cols, diff_threshold=100, blur=morph[1], area=case.area, n_streams=n_streams)


def _planted_frames(kind, case, morph):
    """[(frame, mask the oracle analyses)]: thresh / hsv one frame; diff a first frame (analysed as it is) and the empty frame
    behind it (the same difference, blurred)"""
    if kind == "thresh":
        return [(case.img, T.planted_mask(case, morph)[1])]
    if kind == "hsv":
        hsv = np.repeat(case.img[..., None], 3, axis=2)
        p = O.hsv_params(h_lo=255, h_hi=256, s_lo=255, s_hi=256, v_lo=255, v_hi=256, erode=morph[0], dilate=morph[1],
                         min_area=case.area[0], max_area=case.area[1])
        return [(hsv, O.detect_hsv(hsv, p)[1])]
    d = O.Diff(case.rows, case.cols, 100, morph[1], *case.area)
    return [(f, d.detect(f)[1]) for f in (case.img, np.zeros_like(case.img))]


@pytest.mark.parametrize("kind", ["thresh", "hsv", "diff"])
@pytest.mark.parametrize("case", PLANTED, ids=[c.name for c in PLANTED])
def test_planted_masks_through_the_single_stage_detectors(A, case, kind):
    for morph in T.MORPHS:
        frames = _planted_frames(kind, case, morph)
        plain = _detector(A, kind, case, morph)
        want_plain = [plain.detectPosition(f) for f, _ in frames]
        taps = [plain.read_mask(w) for w in (THR, MORPH, FIN)]
        for k in T.KS:
            det = _detector(A, kind, case, morph)
            _refused(det.targets)                                        # targets off
            det.set_targets(k)
            _refused(det.targets)                                        # on, and no call has delivered yet
            for t, (f, mask) in enumerate(frames):
                got = det.detectPosition(f)
                assert got == want_plain[t], (morph, k, t)               # the ordinary result does not move
                sets = det.targets()
                assert len(sets) == 1 and len(sets[0]) == 1
                _check_stream(sets[0][0], T.reference(mask, case.area, k), (case.name, kind, morph, k, t), ordinary=got)
                assert det.targets() == sets                             # nothing is consumed
            for w, tap in zip((THR, MORPH, FIN), taps):
                assert (det.read_mask(w) == tap).all(), (morph, k, w)
            det.close()
        plain.close()


def test_a_single_stage_detector_fills_its_stream_only(A):
    case, morph, k = PLANTED[0], T.MORPHS[0], 3
    det = _detector(A, "thresh", case, morph, n_streams=3)
    det.set_targets(k)
    ref = T.planted_reference(case.name, morph, k)
    for s in (1, 2, 0):
        got = det.detectPosition(case.img, stream=s)
        (sets,) = det.targets()
        assert len(sets) == 3
        for q in range(3):
            _check_stream(sets[q], ref if q == s else ([dict(T.INVALID)] * k, 0), (s, q), ordinary=got if q == s else None)
    det.close()


def test_two_runs_rank_alike(A):
    """The order of the root list differs from run to run (atomics); the ranking does not depend on it: ~1300 candidates of one
    area, ranked by first pixel alone."""
    case = next(c for c in PLANTED if c.name.startswith("dots"))
    seen = []
    for _ in range(2):
        det = _detector(A, "thresh", case, (0, 0))
        det.set_targets(8)
        for _ in range(3):
            det.detectPosition(case.img)
            seen.append(det.targets())
        det.close()
    assert all(s == seen[0] for s in seen[1:])
    _check_stream(seen[0][0][0], T.planted_reference(case.name, (0, 0), 8), "dots")


# ------------------------------------------------------------------------------------------------- the batched trackers ----

def _frames_at(family, rows, cols, n, t):
    return [T.sequence(family, rows, cols, T.variant_of(s))[t] for s in range(n)]


def _refs_at(family, rows, cols, n, t, alpha=0.0, k=T.TRACKER_K):
    return [T.sequence_reference(family, rows, cols, T.variant_of(s), alpha, k)[t] for s in range(n)]


def _check_set(got_set, got_pos, family, rows, cols, n, t, alpha=0.0, k=T.TRACKER_K):
    refs = _refs_at(family, rows, cols, n, t, alpha, k)
    assert len(got_set) == n
    for s in range(n):
        _check_stream(got_set[s], refs[s], (family, rows, cols, n, t, s), ordinary=got_pos[s])


def _make_tracker(A, family, rows, cols, n, alpha=0.0):
    if family == "motion":
        return A.MotionTracker(rows, cols, n_streams=n, channels=3, area=T.AREA, **T.DIFF)
    w = T.sub_window()
    return A.SubtractionTracker(rows, cols, n_streams=n, channels=3, alpha=alpha, h_thresh=w["h"], s_thresh=w["s"], v_thresh=w["v"],
                                erode=T.SUB_MORPH[0], dilate=T.SUB_MORPH[1], area=T.AREA)


# frames 0 .. 9: a host step, a device step, sequence calls of 1, 2 and 5 frames
PLAN = (("track", 1), ("track_dev", 1), ("seq", 1), ("seq", 2), ("seq", 5))
KALMAN = dict(kalman=dict(dt=0.02, timeout=0.1, sigma_accel=5.0, sigma_noise=0.5))


def _run_tracker(A, family, rows, cols, n, alpha, k, filters):
    """-> per frame: (positions, target set or None, filtered set or None); then the taps and the state behind the last frame"""
    tr = _make_tracker(A, family, rows, cols, n, alpha)
    if filters:
        tr.set_filters(**KALMAN)
    if k:
        tr.set_targets(k)
    out, t = [], 0
    for how, count in PLAN:
        frames = [_frames_at(family, rows, cols, n, t + i) for i in range(count)]
        if how == "track":
            pos = [tr.track(frames[0])]
        else:
            bufs = [_dev(f) for f in frames]
            pos = [tr.track_dev(bufs[0].data_ptr())] if how == "track_dev" else tr.track_sequence_dev([b.data_ptr() for b in bufs])
        sets = tr.targets() if k else [None] * count
        filt = tr.filtered() if filters else [None] * count
        assert len(pos) == len(sets) == len(filt) == count, (how, count, len(sets))
        if k:
            assert tr.targets() == sets
        out += list(zip(pos, sets, filt))
        t += count
    assert t == T.N_FRAMES
    taps = [[tr.read_mask(w, s) for w in (THR, MORPH, FIN)] for s in range(min(n, 4))]
    state = [tr.state(s) for s in range(min(n, 4))] if family == "subtraction" else None
    tr.close()
    return out, taps, state


@pytest.mark.parametrize("n", [1, 3, 66])
@pytest.mark.parametrize("rows,cols", T.GEOMETRIES)
@pytest.mark.parametrize("family,alpha", [("motion", 0.0), ("subtraction", 0.0), ("subtraction", 0.05)])
def test_batched_trackers(A, family, alpha, rows, cols, n):
    k = T.TRACKER_K
    filters = n == 3
    got, taps, state = _run_tracker(A, family, rows, cols, n, alpha, k, filters)
    plain, ptaps, pstate = _run_tracker(A, family, rows, cols, n, alpha, 0, filters)
    for t, ((pos, tset, filt), (ppos, _, pfilt)) in enumerate(zip(got, plain)):
        assert pos == ppos, (t, "the ordinary results move with targets on")
        assert filt == pfilt, (t, "the filtered records move with targets on")
        _check_set(tset, pos, family, rows, cols, n, t, alpha, k)
    for a, b in zip(taps, ptaps):
        for x, y in zip(a, b):
            assert (x == y).all()
    if state is not None:
        for (bg, acc), (pbg, pacc) in zip(state, pstate):
            assert (bg == pbg).all() and (acc == pacc).all()
    if n == 1:                                    # ... and two runs give identical target sets
        again, _, _ = _run_tracker(A, family, rows, cols, n, alpha, k, filters)
        assert [g[1] for g in again] == [g[1] for g in got]


@pytest.mark.parametrize("k", [1, 8])
def test_batched_trackers_other_k(A, k):
    rows, cols, n = 37, 61, 3
    for family in ("motion", "subtraction"):
        got, _, _ = _run_tracker(A, family, rows, cols, n, 0.0, k, False)
        for t, (pos, tset, _) in enumerate(got):
            _check_set(tset, pos, family, rows, cols, n, t, 0.0, k)


def test_a_tracker_switched_on_behind_targets_has_its_sets(A):
    """oatgpu_set_targets before oatgpu_set_diff_tracker / _bsub_tracker: the tracker allocates its own target sets."""
    rows, cols, n, k = 48, 64, 3, T.TRACKER_K
    for family, sw in (("motion", "oatgpu_set_diff_tracker"), ("subtraction", "oatgpu_set_bsub_tracker")):
        tr = _make_tracker(A, family, rows, cols, n)
        tr._chk(getattr(tr.lib, sw)(tr.ctx, 0))
        tr.set_targets(k)
        tr._chk(getattr(tr.lib, sw)(tr.ctx, 1))
        for t in range(5):
            pos = tr.track(_frames_at(family, rows, cols, n, t))
            _check_set(tr.targets()[0], pos, family, rows, cols, n, t)
        tr.set_targets(0)
        _refused(tr.targets)
        pos = tr.track(_frames_at(family, rows, cols, n, 5))
        for s in range(n):
            assert same_dict(_as_dict(pos[s]), _refs_at(family, rows, cols, n, 5)[s][0][0])
        tr.close()


# ----------------------------------------------------------------------------------------------------- the fused tracker ----

def _hotpath(A, rows, cols, n, ring=4):
    return A.HotPath(rows, cols, n_streams=n, adaptation_coeff=T.FUSED_LR, erode=T.FUSED_MORPH[0], dilate=T.FUSED_MORPH[1],
                     area=T.AREA, ring_depth=ring, **T.FUSED_WIN)


def _run_fused(A, rows, cols, n, how, k, ring=4):
    """-> per frame (positions, target set or None); then the taps and the models behind the last frame"""
    hp = _hotpath(A, rows, cols, n, ring)
    n_frames = len(T.sequence("fused", rows, cols, 0))
    frames = [_frames_at("fused", rows, cols, n, t) for t in range(n_frames)]
    if k:
        hp.set_targets(k)
    out = []

    def sets():
        return hp.targets() if k else [None]
    if how == "track":
        for f in frames:
            out.append((hp.track(f), sets()[0]))
    elif how == "track_dev":
        for f in frames:
            b = _dev(f)
            out.append((hp.track_dev(b.data_ptr()), sets()[0]))
    elif how == "ring":
        pending = 0
        for f in frames:
            hp.enqueue(f)
            pending += 1
            if pending == ring:
                out.append((hp.collect(), sets()[0]))
                pending -= 1
        while pending:
            out.append((hp.collect(), sets()[0]))
            pending -= 1
    else:                                         # sequence calls of 5 frames, two frames a launch, then the rest
        hp.set_fusion(2)
        t = 0
        while t < n_frames:
            count = min(5, n_frames - t)
            bufs = [_dev(f) for f in frames[t:t + count]]
            pos = hp.track_sequence_dev([b.data_ptr() for b in bufs])
            ts = hp.targets() if k else [None] * count
            assert len(ts) == count
            out += list(zip(pos, ts))
            t += count
    taps = [[hp.read_mask(w, s) for w in (THR, MORPH, FIN)] for s in range(n)]
    models = [hp.mog_state(s) for s in range(n)]
    assert hp.last_step_shape()[1] is False
    hp.close()
    return out, taps, models


@pytest.mark.parametrize("how,ring", [("track", 4), ("track_dev", 4), ("ring", 2), ("ring", 4), ("sequence", 4)])
@pytest.mark.parametrize("rows,cols", T.GEOMETRIES)
def test_fused_tracker(A, rows, cols, how, ring):
    n, k = 3, T.TRACKER_K
    got, taps, models = _run_fused(A, rows, cols, n, how, k, ring)
    plain, ptaps, pmodels = _run_fused(A, rows, cols, n, how, 0, ring)
    assert len(got) == len(plain) == len(T.sequence("fused", rows, cols, 0))
    for t, ((pos, tset), (ppos, _)) in enumerate(zip(got, plain)):
        assert pos == ppos, (t, "the ordinary results move with targets on")
        _check_set(tset, pos, "fused", rows, cols, n, t, 0.0, k)
    for a, b in zip(taps, ptaps):
        for x, y in zip(a, b):
            assert (x == y).all()
    for a, b in zip(models, pmodels):
        for x, y in zip(a[:4], b[:4]):
            assert np.array_equal(x, y)
        assert a[4] == b[4]


def test_fused_tracker_filters_stay_on_the_ordinary_result(A):
    """Targets are raw detections: with oatgpu_set_kalman and oatgpu_set_homography on, the ordinary result is the filtered one,
    its raw_x / raw_y is rank 0, and every rank is the reference's."""
    rows, cols, n, k = 48, 64, 3, T.TRACKER_K
    hp, plain = _hotpath(A, rows, cols, n), _hotpath(A, rows, cols, n)
    for h in (hp, plain):
        h.set_kalman(True, dt=0.02, timeout=0.1, sigma_accel=5.0, sigma_noise=0.5)
        h.set_homography([2.0, 0.0, 1.0, 0.0, 2.0, -1.0, 0.0, 0.0, 1.0])
    hp.set_targets(k)
    for t in range(len(T.sequence("fused", rows, cols, 0))):
        f = _frames_at("fused", rows, cols, n, t)
        pos, ppos = hp.track(f), plain.track(f)
        assert pos == ppos, t
        (tset,) = hp.targets()
        _check_set(tset, [None] * n, "fused", rows, cols, n, t, 0.0, k)
        for s in range(n):
            r0 = tset[s][0][0]
            assert r0.position_valid == pos[s].raw_valid and (not r0.position_valid or (r0.x, r0.y) == (pos[s].raw_x, pos[s].raw_y))
    hp.close()
    plain.close()


def test_targets_off_again_restores_the_launch_order(A):
    """3 x 1080p on device frames is where the early order is the default.  A step with targets on takes the plain order (early_blob
    0); with targets off again the very next pipelined step is early again, and every result is what a context that never had
    targets on delivers."""
    rows, cols, n, k = 1080, 1920, 3, 4
    rng = np.random.default_rng(5)
    bg = rng.integers(40, 91, (rows, cols, 3)).astype(np.uint8)
    blocks = [(100 + 150 * i, 200 + 250 * i, 20 + 6 * i, 30 + 4 * i) for i in range(6)]

    def frame(t, s):
        f = bg.copy()
        for i, (y, x, h, w) in enumerate(blocks[: 2 + (t + s) % 5]):
            f[y + 7 * t:y + 7 * t + h, x + 11 * t + 40 * s:x + 11 * t + 40 * s + w] = T.BLOCK_BGR
        return f
    frames = [_dev([frame(t, s) for s in range(n)]) for t in range(8)]
    kw = dict(n_streams=n, adaptation_coeff=T.FUSED_LR, erode=0, dilate=3, area=(20.0, T.BIG), ring_depth=4, **T.FUSED_WIN)
    hp, plain = A.HotPath(rows, cols, **kw), A.HotPath(rows, cols, **kw)

    def pair(h, t):
        """two frames in flight: the second is not alone -> (results, was the second step early?)"""
        h.enqueue_dev(frames[t].data_ptr(), keepalive=frames[t])
        h.enqueue_dev(frames[t + 1].data_ptr(), keepalive=frames[t + 1])
        early = h.last_step_shape()[1]
        return [h.collect(), h.collect()], early

    want = [pair(plain, t) for t in (0, 2, 4, 6)]
    assert all(e for _, e in want), "the shape no longer takes the early order by default: pick another"
    got, early = pair(hp, 0)
    assert early and got == want[0][0]
    hp.set_targets(k)
    hp.enqueue_dev(frames[2].data_ptr(), keepalive=frames[2])
    hp.enqueue_dev(frames[3].data_ptr(), keepalive=frames[3])
    assert hp.last_step_shape()[1] is False
    for t in (2, 3):
        pos = hp.collect()
        assert pos == want[1][0][t - 2]
        (tset,) = hp.targets()
        for s in range(n):
            ranks, n_found = tset[s]
            assert ranks[0] == pos[s] and n_found >= sum(r.position_valid for r in ranks) >= 2
            keys = [(r.area, r.first_pixel) for r in ranks if r.position_valid]
            assert keys == sorted(keys, reverse=True)
    hp.set_targets(0)
    for i, t in enumerate((4, 6)):
        got, early = pair(hp, t)
        assert early, "targets off again: the early order is back at once"
        assert got == want[2 + i][0]
    assert hp.early_blob_timeouts() == 0
    hp.close()
    plain.close()


# ------------------------------------------------------------------------------------------------------------ refusals ----

def test_refusals_and_room(A):
    rows, cols, n, k = 48, 64, 2, T.TRACKER_K
    hp = _hotpath(A, rows, cols, n)
    f = [_frames_at("fused", rows, cols, n, t) for t in range(8)]
    assert "0..8" in _refused(hp.set_targets, -1)
    _refused(hp.set_targets, 9)
    _refused(hp.targets)                                               # off
    hp.enqueue(f[0])                                                   # results outstanding
    assert "outstanding" in _refused(hp.set_targets, k)
    hp.collect()
    hp.stage(0, f[1][0])                                               # a frame set partly staged
    _refused(hp.set_targets, k)
    hp.stage_abort()
    hp._chk(hp.lib.oatgpu_set_deferred(hp.ctx, 1))                     # deferred completion on
    assert "deferred" in _refused(hp.set_targets, k)
    hp._chk(hp.lib.oatgpu_set_deferred(hp.ctx, 0))
    hp.set_markers([dict(h=(100, 125), s=(150, 256), v=(100, 256), dilate=3)])      # marker sets configured
    assert "marker" in _refused(hp.set_targets, k)
    hp.set_markers([])
    _refused(hp.targets)                                               # still off: nothing above changed anything
    hp.set_targets(k)
    _refused(hp.targets)                                               # on, before any step
    assert "targets" in _refused(hp.set_markers, [dict(h=(100, 125))])
    assert hp.lib.oatgpu_set_deferred(hp.ctx, 1) == E_INVALID
    assert hp.lib.oatgpu_set_deferred(hp.ctx, 0) == 0
    # a step behind all of that still matches, and the room of oatgpu_targets is checked
    hp2 = _hotpath(A, rows, cols, n)
    for t in range(4):
        assert hp.track(f[t]) == hp2.track(f[t])
    bufs = [_dev(x) for x in f[4:7]]
    pos = hp.track_sequence_dev([b.data_ptr() for b in bufs])
    from oat_amd import ffi
    out = (ffi.Position * (3 * n * k))()
    found = (C.c_int32 * (3 * n))()
    assert hp.lib.oatgpu_targets(hp.ctx, out, found, 2) == E_INVALID   # one too small
    assert hp.lib.oatgpu_targets(hp.ctx, None, found, 3) == E_INVALID
    assert hp.lib.oatgpu_targets(hp.ctx, out, found, 3) == 3
    sets = hp.targets()
    assert len(sets) == 3
    for i in range(3):
        _check_set(sets[i], pos[i], "fused", rows, cols, n, 4 + i)
    hp.set_targets(k)                                                  # the setter starts the list over
    _refused(hp.targets)
    hp.close()
    hp2.close()
