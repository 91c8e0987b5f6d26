"""GPU tests of target tracks (oatgpu_set_tracks / oatgpu_tracks / oatgpu_tracks_update; _Detector.set_tracks / .tracks /
.update_tracks; k_target_tracks in kernels_tracks.hip).  Every record of every slot, frame and stream is compared,
bit for bit, with the model of tests/tracks_ref.py on the cases of tests/tracks_cases.py: the fed cases through
oatgpu_tracks_update, the image sequences through the motion and the subtraction tracker's batch and sequence calls, and
update_tracks(targets()) behind the fused tracker and a single-stage detector.  Everything else a context computes is compared
with a second context that never had tracks on.  Every frame is under 0.004 MP."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import targets_cases as T
import tracks_cases as TC
import tracks_ref as TR

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


def _as_dict(t):
    return dict(position_valid=t.position_valid, velocity_valid=t.velocity_valid, heading_valid=t.heading_valid,
                region_valid=t.region_valid, region=t.region, x=t.x, y=t.y, vx=t.vx, vy=t.vy, hx=t.hx, hy=t.hy, id=t.id, rank=t.rank,
                age=t.age, missed=t.missed)


def _check_camera(got, want, tag):
    """got: k Track of one camera and frame, want: the model's k records"""
    assert len(got) == len(want), tag
    for i, (g, w) in enumerate(zip(got, want)):
        assert TR.same(_as_dict(g), w), (tag, i, g, w)
        if not w["id"]:
            assert (g.id, g.rank, g.age, g.missed) == (0, -1, 0, 0), (tag, i, g)


def _refused(fn, *a, **kw):
    from oat_amd.ffi import OatGpuError
    with pytest.raises(OatGpuError) as e:
        fn(*a, **kw)
    assert e.value.code == E_INVALID, e.value
    return str(e.value)


def _feeder(A, n, k, **config):
    """a context whose only job is oatgpu_tracks_update"""
    d = A.SimpleThreshold(8, 8, n_streams=n)
    d.set_targets(k)
    d.set_tracks(**config)
    return d


# ---------------------------------------------------------------------------------- the fed cases through tracks_update ----

FED = TC.fed_cases()


@functools.lru_cache(maxsize=None)
def _fed_want(name, stream):
    return TC.fed(name).want(stream)[0]


@pytest.mark.parametrize("n", [1, 3, 66])
@pytest.mark.parametrize("case", FED, ids=[c.name for c in FED])
def test_fed_cases_through_tracks_update(A, case, n):
    d = _feeder(A, n, case.k, **case.config())
    _refused(d.tracks)                                               # on, and nothing delivered yet
    rows = [case.frames(s) for s in range(n)]
    for t in range(len(case.scene)):
        got = d.update_tracks([rows[s][t] for s in range(n)])
        assert len(got) == n
        for s in range(n):
            _check_camera(got[s], _fed_want(case.name, s)[t], (case.name, n, t, s))
        assert d.tracks() == [got]                                   # the update is a delivering call; nothing is consumed
    d.close()


def test_set_tracks_again_restarts_slots_and_ids(A):
    case = TC.fed("miss-k3")
    d = _feeder(A, 3, case.k, **case.config())
    for rerun in range(2):
        for t in range(9):
            got = d.update_tracks([case.frames(s)[t] for s in range(3)])
            for s in range(3):
                _check_camera(got[s], _fed_want(case.name, s)[t], (rerun, t, s))
        assert max(r.id for cam in got for r in cam) == 4
        d.set_tracks(**case.config())
        _refused(d.tracks)
    d.close()


def test_two_runs_give_the_same_records(A):
    case = TC.fed("many-k8")
    seen = []
    for _ in range(2):
        d = _feeder(A, 66, case.k, **case.config())
        seen.append([d.update_tracks([case.frames(s)[t] for s in range(66)]) for t in range(len(case.scene))])
        d.close()
    assert seen[0] == seen[1]


# --------------------------------------------------------------------------------- the motion and the subtraction tracker ----

# frames 0 .. 20: a host step, a device step, sequence calls of 1, 2 and 5 frames, the detector's reset, a sequence call of 11
PLAN = (("track", 1), ("track_dev", 1), ("seq", 1), ("seq", 2), ("seq", 5), ("reset", 0), ("seq", 11))
RESETS = (TC.RESET_AT,)
FILTERS = dict(kalman=dict(dt=0.02, timeout=0.1, sigma_accel=5.0, sigma_noise=0.5))


def _make_tracker(A, family, rows, cols, channels, n, alpha):
    if family == "motion":
        return A.MotionTracker(rows, cols, n_streams=n, channels=channels, area=TC.DC.AREA, **TC.DIFF)
    return A.SubtractionTracker(rows, cols, **TC.sub_case(rows, cols, channels, n, alpha).tracker_args())


def _frames_at(family, rows, cols, channels, n, t):
    return [TC.sequence(family, rows, cols, channels, TC.variant_of(s))[t] for s in range(n)]


def _run_tracker(A, family, rows, cols, channels, n, alpha, tracks, k=TC.IMG_K):
    """-> per frame (positions, target set, filtered set, track set or None); then the taps and the state behind the last frame"""
    tr = _make_tracker(A, family, rows, cols, channels, n, alpha)
    tr.set_filters(**FILTERS)
    tr.set_targets(k)
    if tracks:
        tr.set_tracks(**TC.image_config())
    out, t = [], 0
    for how, count in PLAN:
        if how == "reset":
            assert t == TC.RESET_AT
            tr.reset()
            continue
        frames = [_frames_at(family, rows, cols, channels, n, t + i) for i in range(count)]
        if how == "track":
            pos = [tr.track(frames[0])]
        else:
            bufs = [_dev(f) for f in frames]
            pos = [tr.track_dev(bufs[0].data_ptr())] if how == "track_dev" else tr.track_sequence_dev([b.data_ptr() for b in bufs])
        sets, filt = tr.targets(), tr.filtered()
        trk = tr.tracks() if tracks else [None] * count
        assert len(pos) == len(sets) == len(filt) == len(trk) == count, (how, count, len(trk))
        if tracks:
            assert tr.tracks() == trk                                # nothing is consumed
        out += list(zip(pos, sets, filt, trk))
        t += count
    assert t == TC.IMG_T
    taps = [[tr.read_mask(w, s) for w in (THR, MORPH, FIN)] for s in range(min(n, 4))]
    state = [tr.state(s) for s in range(min(n, 4))] if family == "subtraction" else None
    tr.close()
    return out, taps, state


SHAPES = [g + (n,) for g in TC.GEOMETRIES for n in (1, 3)] + [TC.MANY + (66,)]


@pytest.mark.parametrize("rows,cols,channels,n", SHAPES, ids=[f"{r}x{c}x{ch}-n{n}" for r, c, ch, n in SHAPES])
@pytest.mark.parametrize("family,alpha", TC.FAMILIES)
def test_batched_trackers(A, family, alpha, rows, cols, channels, n):
    k = TC.IMG_K
    got, taps, state = _run_tracker(A, family, rows, cols, channels, n, alpha, True)
    plain, ptaps, pstate = _run_tracker(A, family, rows, cols, channels, n, alpha, False)
    want = [TC.image_want(family, rows, cols, channels, v, alpha, k, None, RESETS)[0] for v in range(3)]
    feeder = _feeder(A, n, k, **TC.image_config())
    for t, ((pos, tset, filt, trk), (ppos, ptset, pfilt, _)) in enumerate(zip(got, plain)):
        assert pos == ppos, (t, "the ordinary results move with tracks on")
        assert tset == ptset, (t, "the target sets move with tracks on")
        assert filt == pfilt, (t, "the trackers' own filtered records move with tracks on")
        assert len(trk) == n
        for s in range(n):
            _check_camera(trk[s], want[TC.variant_of(s)][t], (family, alpha, rows, cols, n, t, s))
        assert feeder.update_tracks(tset) == trk, (t, "in-step tracks differ from the same targets fed to tracks_update")
    feeder.close()
    for a, b in zip(taps, ptaps):
        for x, y in zip(a, b):
            assert (x == y).all()
    if state is not None:
        for (bg, acc), (pbg, pacc) in zip(state, pstate):
            assert (bg == pbg).all() and (acc == pacc).all()
    if n == 1:                                        # ... and two runs give identical track sets
        again, _, _ = _run_tracker(A, family, rows, cols, channels, n, alpha, True)
        assert [g[3] for g in again] == [g[3] for g in got]


@pytest.mark.parametrize("k", [1, 8])
def test_batched_trackers_other_k(A, k):
    rows, cols, channels, n = 37, 61, 1, 3
    for family, alpha in TC.FAMILIES[:2]:
        got, _, _ = _run_tracker(A, family, rows, cols, channels, n, alpha, True, k)
        want = [TC.image_want(family, rows, cols, channels, v, alpha, k, None, RESETS)[0] for v in range(3)]
        for t, (_, _, _, trk) in enumerate(got):
            for s in range(n):
                _check_camera(trk[s], want[TC.variant_of(s)][t], (family, k, t, s))


def test_the_two_trackers_and_the_update_continue_one_another(A):
    """One context, one track state: a motion step, an update from outside, a subtraction step, and again -- the model sees one
    stream of detections (each call's own targets(), checked elsewhere, or the rows that were fed)."""
    from oat_amd import ffi
    rows, cols, channels, n, k = 48, 64, 3, 3, TC.IMG_K
    tr = _make_tracker(A, "motion", rows, cols, channels, n, 0.0)
    tr._chk(tr.lib.oatgpu_set_bsub_tracker(tr.ctx, 1))
    tr.set_targets(k)
    tr.set_tracks(**TC.image_config())
    cams = [TR.Camera(k, TC.IMG_KALMAN, TC.IMG_GATE) for _ in range(n)]
    fed_rows = [TC.fed("swap-k3-inf").frames(s) for s in range(n)]
    pos = (ffi.Position * n)()
    for t in range(9):
        frames = _frames_at("motion", rows, cols, channels, n, t)
        if t % 3 == 1:
            dets = [fed_rows[s][t] for s in range(n)]
            trk = tr.update_tracks(dets)
        else:
            if t % 3 == 0:
                tr.track(frames)
            else:
                ptrs = (ffi._u8p * n)(*[ffi.u8(f) for f in frames])
                tr._chk(tr.lib.oatgpu_bsub_track_batch(tr.ctx, ptrs, n, 0.0, pos))
            (trk,), (tset,) = tr.tracks(), tr.targets()
            dets = [[(p.position_valid, p.x, p.y) for p in tset[s][0]] for s in range(n)]
        for s in range(n):
            _check_camera(trk[s], cams[s].step(dets[s]), (t, s))
    assert max(r.id for cam in trk for r in cam) >= 2
    tr.close()


def test_a_tracker_switched_on_behind_tracks_has_its_sets(A):
    rows, cols, channels, n, k = 37, 61, 1, 3, TC.IMG_K
    for family, sw in (("motion", "oatgpu_set_diff_tracker"), ("subtraction", "oatgpu_set_bsub_tracker")):
        tr = _make_tracker(A, family, rows, cols, channels, n, 0.0)
        tr._chk(getattr(tr.lib, sw)(tr.ctx, 0))
        tr.set_targets(k)
        tr.set_tracks(**TC.image_config())
        tr._chk(getattr(tr.lib, sw)(tr.ctx, 1))
        want = [TC.image_want(family, rows, cols, channels, v, 0.0)[0] for v in range(3)]
        for t in range(6):
            tr.track(_frames_at(family, rows, cols, channels, n, t))
            (trk,) = tr.tracks()
            for s in range(n):
                _check_camera(trk[s], want[TC.variant_of(s)][t], (family, t, s))
        tr.set_tracks(None)
        _refused(tr.tracks)
        tr.set_targets(0)                             # ... allowed again with tracks off
        tr.close()


# ------------------------------------------------------------------- the fused tracker and a single-stage detector ----

def test_update_tracks_behind_the_fused_tracker(A):
    rows, cols, n, k = 48, 64, 3, T.TRACKER_K
    hp = A.HotPath(rows, cols, n_streams=n, adaptation_coeff=T.FUSED_LR, erode=T.FUSED_MORPH[0], dilate=T.FUSED_MORPH[1],
                   area=T.AREA, **T.FUSED_WIN)
    plain = A.HotPath(rows, cols, n_streams=n, adaptation_coeff=T.FUSED_LR, erode=T.FUSED_MORPH[0], dilate=T.FUSED_MORPH[1],
                      area=T.AREA, **T.FUSED_WIN)
    for h in (hp, plain):
        h.set_targets(k)
    hp.set_tracks(**TC.image_config())
    cams = [TR.Camera(k, TC.IMG_KALMAN, TC.IMG_GATE) for _ in range(n)]
    for t in range(len(T.sequence("fused", rows, cols, 0))):
        frames = [T.sequence("fused", rows, cols, T.variant_of(s))[t] for s in range(n)]
        assert hp.track(frames) == plain.track(frames), t            # the fused tracker's own calls do not look at tracks
        (tset,) = hp.targets()
        assert tset == plain.targets()[0]
        if t == 0:
            _refused(hp.tracks)                                      # ... and deliver no track set
        trk = hp.update_tracks(tset)
        for s in range(n):
            ref = T.sequence_reference("fused", rows, cols, T.variant_of(s), 0.0, k)[t][0]
            _check_camera(trk[s], cams[s].step(TC.triples(ref)), (t, s))
    for s in range(n):
        for a, b in zip(hp.mog_state(s)[:4], plain.mog_state(s)[:4]):
            assert np.array_equal(a, b)
    hp.close()
    plain.close()


@pytest.mark.parametrize("k", [3, 8])
def test_update_tracks_behind_detect_thresh(A, k):
    cases = [c for c in T.planted_cases() if (c.rows, c.cols) == (48, 64) and c.area == (0.5, T.BIG)]
    assert len(cases) >= 2
    det = A.SimpleThreshold(48, 64, thresh=(255, 256), area=cases[0].area)
    det.set_targets(k)
    det.set_tracks(kalman=TC.KALMAN, gate=25.0)
    cam = TR.Camera(k, TC.KALMAN, 25.0)
    for t in range(8):
        case = cases[(t // 2) % len(cases)]
        pos = det.detectPosition(case.img)
        (tset,) = det.targets()
        (trk,) = det.update_tracks(tset)
        ref = T.planted_reference(case.name, (0, 0), k)[0]
        _check_camera(trk, cam.step(TC.triples(ref)), (k, t))
        assert pos.position_valid == ref[0]["valid"]
    det.close()


# ------------------------------------------------------------------------------------------------------- the refusals ----

def test_refusals(A):
    from oat_amd import ffi
    kal = dict(kalman=TC.KALMAN)
    d = A.SimpleThreshold(8, 8, n_streams=2)
    _refused(d.tracks)                                               # tracks off
    _refused(d.update_tracks, [[], []])
    assert "targets are off" in _refused(d.set_tracks, **kal)
    d.set_targets(2)
    f = ffi.MarkerFilters()
    f.homography = 1
    f.h = (C.c_double * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    assert d.lib.oatgpu_set_tracks(d.ctx, C.byref(f), 1.0) == E_INVALID and b"kalman" in d.lib.oatgpu_last_error(d.ctx)
    for gate in (float("nan"), -1.0, -math.inf):
        assert "gate" in _refused(d.set_tracks, gate=gate, **kal)
    _refused(d.set_tracks, kalman=dict(TC.KALMAN, dt=0.0))           # a Kalman parameter out of range
    square = [(0, 0), (4, 0), (4, 4), (0, 4)]
    _refused(d.set_tracks, regions=[(f"r{i}", square) for i in range(17)], **kal)      # a limit exceeded
    _refused(d.set_tracks, regions=[("a-name-of-10", square)], **kal)
    _refused(d.tracks)                                               # ... and nothing has changed: still off
    d.set_tracks(gate=math.inf, **kal)
    d.set_tracks(gate=0.0, **kal)
    assert "switch tracks off first" in _refused(d.set_targets, 3)
    assert "switch tracks off first" in _refused(d.set_targets, 0)
    _refused(d.tracks)                                               # on, nothing delivered yet
    dets = [[(True, 1.0, 2.0), (False, 0.0, 0.0)]] * 2
    got = d.update_tracks(dets)
    assert [r.id for r in got[0]] == [1, 0] and d.tracks() == [got]
    out = (ffi.Track * 4)()
    assert d.lib.oatgpu_tracks(d.ctx, out, 0) == E_INVALID           # the room check
    assert b"room for 0 frame sets, the latest call delivered 1" in d.lib.oatgpu_last_error(d.ctx)
    assert d.lib.oatgpu_tracks(d.ctx, None, 1) == E_INVALID and d.lib.oatgpu_tracks_update(d.ctx, None, out) == E_INVALID
    d.set_tracks(None)
    _refused(d.tracks)
    d.set_targets(0)
    d.close()


def test_the_room_check_behind_a_sequence_call(A):
    from oat_amd import ffi
    rows, cols, channels, n, k = 37, 61, 1, 1, TC.IMG_K
    tr = _make_tracker(A, "motion", rows, cols, channels, n, 0.0)
    tr.set_targets(k)
    tr.set_tracks(**TC.image_config())
    bufs = [_dev(_frames_at("motion", rows, cols, channels, n, t)) for t in range(3)]
    tr.track_sequence_dev([b.data_ptr() for b in bufs])
    out = (ffi.Track * (3 * k))()
    assert tr.lib.oatgpu_tracks(tr.ctx, out, 2) == E_INVALID
    assert b"room for 2 frame sets, the latest call delivered 3" in tr.lib.oatgpu_last_error(tr.ctx)
    assert tr.lib.oatgpu_tracks(tr.ctx, out, 3) == 3 and len(tr.tracks()) == 3
    tr.close()


def test_refused_while_results_are_outstanding(A):
    rows, cols, n, k = 48, 64, 1, 3
    hp = A.HotPath(rows, cols, n_streams=n, area=T.AREA)
    hp.set_targets(k)
    hp.set_tracks(kalman=TC.KALMAN)
    frame = [T.sequence("fused", rows, cols, 0)[3]]
    hp.enqueue(frame)
    assert "outstanding" in _refused(hp.set_tracks, kalman=TC.KALMAN)
    assert "outstanding" in _refused(hp.set_tracks, None)
    assert "outstanding" in _refused(hp.update_tracks, [[(False, 0.0, 0.0)] * k])
    hp.collect()
    (tset,) = hp.targets()
    hp.update_tracks(tset)
    hp.close()
