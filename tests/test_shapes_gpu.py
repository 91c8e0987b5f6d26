"""GPU tests of target shapes (oatgpu_set_target_shapes / oatgpu_target_shapes; _Detector.set_target_shapes / .target_shapes;
k_blob_shape in kernels_blob.hip).  Every field of every rank, stream and frame is compared, bit for bit (integers
exact, doubles by bit pattern), with the model of tests/shapes_ref.py on the oracle's own mask; and the ordinary results, targets(),
tracks(), filtered(), the taps and the states with those of a second context that has targets on and shapes off.  Every frame is
under 0.08 MP."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import shapes_cases as S
import shapes_ref as R
import targets_cases as T
import tracks_cases as TC

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


def _as_dict(s):
    return {f: getattr(s, f) for f in R.FIELDS}


def _check_ranks(got, want, tag):
    """got: k Shape of one camera of one set; want: the model's k dicts"""
    assert len(got) == len(want), tag
    for j, (g, w) in enumerate(zip(got, want)):
        assert R.same(_as_dict(g), w), (tag, j, g, w)


def _refused(fn, *a):
    from oat_amd.ffi import OatGpuError
    with pytest.raises(OatGpuError) as e:
        fn(*a)
    assert e.value.code == E_INVALID, e.value
    return str(e.value)


# ------------------------------------------------------------------------ planted masks through the single-stage detectors ----

PLANTED = S.all_planted()


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
        return [(case.img, S.planted_mask(case.name, morph))]
    if kind == "hsv":
        hsv = np.repeat(case.img[..., None], 3, axis=2)
        return [(hsv, O.detect_hsv(hsv, S.planted_params(case, morph, "hsv"))[1])]
    d = O.Diff(case.rows, case.cols, 100, morph[1], *case.area)
    return [(f, d.detect(f)[1]) for f in (case.img, np.zeros_like(case.img))]


@pytest.mark.parametrize("kind", ["thresh", "hsv", "diff"])
@pytest.mark.parametrize("case", PLANTED, ids=[c.name for c in PLANTED])
def test_planted_masks_through_the_single_stage_detectors(A, case, kind):
    for morph in S.MORPHS:
        frames = _planted_frames(kind, case, morph)
        for k in S.KS:
            det, plain = _detector(A, kind, case, morph), _detector(A, kind, case, morph)
            det.set_targets(k)
            plain.set_targets(k)
            _refused(det.target_shapes)                                  # shapes off
            det.set_target_shapes()
            _refused(det.target_shapes)                                  # on, and no call has delivered yet
            _refused(det.targets)                                        # (the setter starts the lists over)
            for t, (f, mask) in enumerate(frames):
                assert det.detectPosition(f) == plain.detectPosition(f), (morph, k, t)
                assert det.targets() == plain.targets(), (morph, k, t)
                sets = det.target_shapes()
                assert len(sets) == 1 and len(sets[0]) == 1
                _check_ranks(sets[0][0], R.reference(mask, case.area, k), (case.name, kind, morph, k, t))
                assert det.target_shapes() == sets                       # nothing is consumed
            for w in (THR, MORPH, FIN):
                assert (det.read_mask(w) == plain.read_mask(w)).all(), (morph, k, w)
            det.close()
            plain.close()


def test_a_single_stage_detector_fills_its_stream_only(A):
    case, morph, k = next(c for c in PLANTED if c.name == "axes-24x32"), (0, 0), 4
    det = _detector(A, "thresh", case, morph, n_streams=3)
    det.set_targets(k)
    det.set_target_shapes()
    ref = S.planted_reference(case.name, morph, k)
    for s in (1, 2, 0):
        det.detectPosition(case.img, stream=s)
        (sets,) = det.target_shapes()
        assert len(sets) == 3
        for q in range(3):
            _check_ranks(sets[q], ref if q == s else [dict(R.INVALID)] * k, (s, q))
    det.close()


def test_two_runs_are_alike(A):
    """Integer sums and maxima: the result does not depend on the order in which workgroups arrive (three and five of them a
    stream here)."""
    for name in ("arrival-140x200", "far-64x1100"):
        case = next(c for c in PLANTED if c.name == name)
        seen = []
        for _ in range(2):
            det = _detector(A, "thresh", case, (0, 0))
            det.set_targets(8)
            det.set_target_shapes()
            for _ in range(3):
                det.detectPosition(case.img)
                seen.append(det.target_shapes())
            det.close()
        assert all(s == seen[0] for s in seen[1:])
        _check_ranks(seen[0][0][0], S.planted_reference(name, (0, 0), 8), name)


def test_shapes_switched_on_off_and_on_again_between_steps(A):
    cases = [next(c for c in PLANTED if c.name == n) for n in ("hole-48x64", "groups-48x64", "ties-48x64")]
    det, plain = _detector(A, "thresh", cases[0], (0, 0)), _detector(A, "thresh", cases[0], (0, 0))
    k = 4
    det.set_targets(k)
    plain.set_targets(k)
    for step in range(9):
        case = cases[step % 3]
        on = step % 3 != 1
        if step % 3 == 1:
            det.set_target_shapes(False)
        elif step % 3 == 2 or step == 0:
            det.set_target_shapes(True)
        assert det.detectPosition(case.img) == plain.detectPosition(case.img), step
        assert det.targets() == plain.targets(), step
        if on:
            _check_ranks(det.target_shapes()[0][0], S.planted_reference(case.name, (0, 0), k), (step, case.name))
        else:
            assert "off" in _refused(det.target_shapes)
    det.close()
    plain.close()


# ------------------------------------------------------------------------------------------------- the batched trackers ----

def _frames_at(family, rows, cols, n, t, source="shapes"):
    return [S.frames_of(family, rows, cols, S.variant_of(s), source)[t] for s in range(n)]


def _check_set(got_set, family, rows, cols, n, t, alpha=0.0, k=S.TRACKER_K, source="shapes"):
    assert len(got_set) == n
    for s in range(n):
        want = S.sequence_reference(family, rows, cols, S.variant_of(s), alpha, k, source)[t]
        _check_ranks(got_set[s], want, (family, rows, cols, n, t, s))


def _make_tracker(A, family, rows, cols, n, alpha=0.0):
    if family == "motion":
        return A.MotionTracker(rows, cols, n_streams=n, channels=3, area=T.AREA, **T.DIFF)
    w = T.sub_window()
    return A.SubtractionTracker(rows, cols, n_streams=n, channels=3, alpha=alpha, h_thresh=w["h"], s_thresh=w["s"], v_thresh=w["v"],
                                erode=T.SUB_MORPH[0], dilate=T.SUB_MORPH[1], area=T.AREA)


# frames 0 .. 9: a host step, a device step, sequence calls of 1, 2 and 5 frames; or one sequence call of all 11
PLAN = (("track", 1), ("track_dev", 1), ("seq", 1), ("seq", 2), ("seq", 5))
PLAN_LONG = (("seq", 11),)
KALMAN = dict(kalman=dict(dt=0.02, timeout=0.1, sigma_accel=5.0, sigma_noise=0.5))


def _run_tracker(A, family, rows, cols, n, alpha, k, shapes, extras, plan=PLAN, source="shapes"):
    """-> per frame: (positions, target set, shape set or None, filtered set or None, track set or None); then the taps and the
    state behind the last frame"""
    tr = _make_tracker(A, family, rows, cols, n, alpha)
    if extras:
        tr.set_filters(**KALMAN)
    tr.set_targets(k)
    if extras:
        tr.set_tracks(**TC.image_config())
    if shapes:
        tr.set_target_shapes()
    out, t = [], 0
    for how, count in plan:
        frames = [_frames_at(family, rows, cols, n, t + i, source) for i in range(count)]
        if how == "track":
            pos = [tr.track(frames[0])]
        else:
            bufs = [_dev(f) for f in frames]
            pos = [tr.track_dev(bufs[0].data_ptr())] if how == "track_dev" else tr.track_sequence_dev([b.data_ptr() for b in bufs])
        tgt = tr.targets()
        shp = tr.target_shapes() if shapes else [None] * count
        filt = tr.filtered() if extras else [None] * count
        trk = tr.tracks() if extras else [None] * count
        assert len(pos) == len(tgt) == len(shp) == len(filt) == len(trk) == count, (how, count, len(shp))
        if shapes:
            assert tr.target_shapes() == shp
        out += list(zip(pos, tgt, shp, filt, trk))
        t += count
    taps = [[tr.read_mask(w, s) for w in (THR, MORPH, FIN)] for s in range(min(n, 4))]
    state = [tr.state(s) for s in range(min(n, 4))] if family == "subtraction" else None
    tr.close()
    return out, taps, state


TRACKER_RUNS = [(f, a, r, c, n) for (f, a) in (("motion", 0.0), ("subtraction", 0.0), ("subtraction", 0.05))
                for (r, c) in S.GEOMETRIES for n in (1, 3)] + \
               [("motion", 0.0, 24, 32, 66), ("subtraction", 0.05, 24, 32, 66), ("motion", 0.0, 37, 61, 66)]


@pytest.mark.parametrize("family,alpha,rows,cols,n", TRACKER_RUNS)
def test_batched_trackers(A, family, alpha, rows, cols, n):
    k = S.TRACKER_K
    extras = n == 3                                # the trackers' filter chain and target tracks ride along
    got, taps, state = _run_tracker(A, family, rows, cols, n, alpha, k, True, extras)
    plain, ptaps, pstate = _run_tracker(A, family, rows, cols, n, alpha, k, False, extras)
    assert len(got) == 10
    for t, ((pos, tgt, shp, filt, trk), (ppos, ptgt, _, pfilt, ptrk)) in enumerate(zip(got, plain)):
        assert pos == ppos, (t, "the ordinary results move with shapes on")
        assert tgt == ptgt, (t, "the target sets move with shapes on")
        assert filt == pfilt and trk == ptrk, (t, "the filtered records or the tracks move with shapes on")
        _check_set(shp, family, rows, cols, n, t, alpha, k)
    for a, b in zip(taps, ptaps):
        for x, y in zip(a, b):
            assert (x == y).all()
    if state is not None:
        for (bg, acc), (pbg, pacc) in zip(state, pstate):
            assert (bg == pbg).all() and (acc == pacc).all()
    if n == 1:                                     # ... and two runs give identical shape sets
        again, _, _ = _run_tracker(A, family, rows, cols, n, alpha, k, True, extras)
        assert [g[2] for g in again] == [g[2] for g in got]


@pytest.mark.parametrize("family,alpha", [("motion", 0.0), ("subtraction", 0.05)])
def test_batched_trackers_one_long_sequence_call(A, family, alpha):
    """11 frames in one call: every one of the tracker's four slots is taken again and again"""
    rows, cols, n, k = 37, 61, 3, S.TRACKER_K
    got, _, _ = _run_tracker(A, family, rows, cols, n, alpha, k, True, False, plan=PLAN_LONG)
    assert len(got) == 11
    for t, (_, _, shp, _, _) in enumerate(got):
        _check_set(shp, family, rows, cols, n, t, alpha, k)


@pytest.mark.parametrize("k", [1, 8])
def test_batched_trackers_other_k_on_the_targets_sequences(A, k):
    """targets_cases' own sequences (frames without a blob, one blob, up to six), K = 1 and 8"""
    rows, cols, n = 37, 61, 3
    for family in ("motion", "subtraction"):
        got, _, _ = _run_tracker(A, family, rows, cols, n, 0.0, k, True, False, source="targets")
        for t, (_, _, shp, _, _) in enumerate(got):
            _check_set(shp, family, rows, cols, n, t, 0.0, k, source="targets")


def test_a_tracker_switched_on_behind_shapes_has_its_sets(A):
    """oatgpu_set_target_shapes before oatgpu_set_diff_tracker / _bsub_tracker: the tracker allocates its own shape sets."""
    rows, cols, n, k = 48, 64, 3, S.TRACKER_K
    for family, sw in (("motion", "oatgpu_set_diff_tracker"), ("subtraction", "oatgpu_set_bsub_tracker")):
        tr = _make_tracker(A, family, rows, cols, n)
        tr._chk(getattr(tr.lib, sw)(tr.ctx, 0))
        tr.set_targets(k)
        tr.set_target_shapes()
        tr._chk(getattr(tr.lib, sw)(tr.ctx, 1))
        for t in range(5):
            tr.track(_frames_at(family, rows, cols, n, t))
            _check_set(tr.target_shapes()[0], family, rows, cols, n, t)
        assert "switch them off first" in _refused(tr.set_targets, 0)
        tr.set_target_shapes(False)
        _refused(tr.target_shapes)
        tr.set_targets(0)
        tr.close()


def test_the_shape_of_a_track_follows_it_across_a_rank_swap(A):
    """tracks_cases' image sequence: three blocks of equal area whose ranks cross.  shapes[track.rank] is the shape of the track's
    blob: the model's record for that rank, and the track's raw detection lies inside its bounding box."""
    rows, cols, channels = TC.GEOMETRIES[0]
    k = TC.IMG_K
    tr = A.MotionTracker(rows, cols, n_streams=1, channels=channels, area=TC.DC.AREA, **TC.DIFF)
    tr.set_targets(k)
    tr.set_tracks(**TC.image_config())
    tr.set_target_shapes()
    d = O.Diff(rows, cols, TC.DIFF["diff_threshold"], TC.DIFF["blur"], *TC.DC.AREA)
    ranks_of = {}
    for t, f in enumerate(TC.sequence("motion", rows, cols, channels, 0)):
        mask = d.detect(TC.DC.oracle_frame(f))[1]
        tr.track([f])
        ((tgt, _),), (trk,), (shp,) = tr.targets()[0], tr.tracks()[0], tr.target_shapes()[0]
        want = R.reference(mask, TC.DC.AREA, k)
        _check_ranks(shp, want, t)
        for slot in trk:
            if slot.id and slot.rank >= 0:
                s, p = shp[slot.rank], tgt[slot.rank]
                assert s.valid and p.position_valid, (t, slot)
                assert s.x_min <= p.x <= s.x_max and s.y_min <= p.y <= s.y_max, (t, slot, s, p)
                ranks_of.setdefault(slot.id, set()).add(slot.rank)
    tr.close()
    assert any(len(r) > 1 for r in ranks_of.values()), ("no track changed its rank: pick another sequence", ranks_of)


# ----------------------------------------------------------------------------------------------------- the fused tracker ----

def _hotpath(A, rows, cols, n, ring=4):
    return A.HotPath(rows, cols, n_streams=n, adaptation_coeff=T.FUSED_LR, erode=T.FUSED_MORPH[0], dilate=T.FUSED_MORPH[1],
                     area=T.AREA, ring_depth=ring, **T.FUSED_WIN)


def _run_fused(A, rows, cols, n, how, k, shapes, ring=4):
    """-> per frame (positions, target set, shape set or None); then the taps and the models behind the last frame"""
    hp = _hotpath(A, rows, cols, n, ring)
    n_frames = len(S.sequence("fused", rows, cols, 0))
    frames = [_frames_at("fused", rows, cols, n, t) for t in range(n_frames)]
    hp.set_targets(k)
    if shapes:
        hp.set_target_shapes()
    out = []

    def sets():
        return hp.targets()[0], (hp.target_shapes()[0] if shapes else None)
    if how == "track":
        for f in frames:
            out.append((hp.track(f),) + sets())
    elif how == "track_dev":
        for f in frames:
            b = _dev(f)
            out.append((hp.track_dev(b.data_ptr()),) + sets())
    elif how in ("ring", "staged"):
        pending = 0
        for f in frames:
            if how == "ring":
                hp.enqueue(f)
            else:
                for s in range(n):
                    hp.stage(s, f[s])
                hp.enqueue_staged()
            pending += 1
            if pending == ring:
                out.append((hp.collect(),) + sets())
                pending -= 1
        while pending:
            out.append((hp.collect(),) + sets())
            pending -= 1
    else:                                         # sequence calls of 5 frames, two frames a launch, then the rest
        hp.set_fusion(2)
        t = 0
        while t < n_frames:
            count = min(5, n_frames - t)
            bufs = [_dev(f) for f in frames[t:t + count]]
            pos = hp.track_sequence_dev([b.data_ptr() for b in bufs])
            tg = hp.targets()
            sh = hp.target_shapes() if shapes else [None] * count
            assert len(tg) == len(sh) == count
            out += list(zip(pos, tg, sh))
            t += count
    taps = [[hp.read_mask(w, s) for w in (THR, MORPH, FIN)] for s in range(min(n, 4))]
    models = [hp.mog_state(s) for s in range(min(n, 4))]
    hp.close()
    return out, taps, models


FUSED_RUNS = [(r, c, 3, how, ring) for (r, c) in S.GEOMETRIES
              for how, ring in (("track", 4), ("track_dev", 4), ("ring", 2), ("ring", 4), ("staged", 3), ("sequence", 4))] + \
             [(24, 32, 1, "track", 4), (24, 32, 66, "ring", 4), (37, 61, 66, "sequence", 4)]


@pytest.mark.parametrize("rows,cols,n,how,ring", FUSED_RUNS)
def test_fused_tracker(A, rows, cols, n, how, ring):
    k = S.TRACKER_K
    got, taps, models = _run_fused(A, rows, cols, n, how, k, True, ring)
    plain, ptaps, pmodels = _run_fused(A, rows, cols, n, how, k, False, ring)
    assert len(got) == len(plain) == len(S.sequence("fused", rows, cols, 0))
    for t, ((pos, tgt, shp), (ppos, ptgt, _)) in enumerate(zip(got, plain)):
        assert pos == ppos, (t, "the ordinary results move with shapes on")
        assert tgt == ptgt, (t, "the target sets move with shapes on")
        _check_set(shp, "fused", rows, cols, n, t, 0.0, k)
    for a, b in zip(taps, ptaps):
        for x, y in zip(a, b):
            assert (x == y).all()
    for a, b in zip(models, pmodels):
        for x, y in zip(a[:4], b[:4]):
            assert np.array_equal(x, y)
        assert a[4] == b[4]


# ------------------------------------------------------------------------------------------------------------ refusals ----

def test_refusals_and_room(A):
    rows, cols, n, k = 48, 64, 2, S.TRACKER_K
    hp = _hotpath(A, rows, cols, n)
    f = [_frames_at("fused", rows, cols, n, t) for t in range(8)]
    assert "targets are off" in _refused(hp.set_target_shapes)         # targets off
    assert "targets are off" in _refused(hp.set_target_shapes, False)
    _refused(hp.target_shapes)
    hp.set_targets(k)
    hp.enqueue(f[0])                                                   # results outstanding
    assert "outstanding" in _refused(hp.set_target_shapes)
    hp.collect()
    assert len(hp.targets()) == 1                                      # ... and nothing changed: the list is still there
    hp.stage(0, f[1][0])                                               # a frame set partly staged
    _refused(hp.set_target_shapes)
    hp.stage_abort()
    assert "off" in _refused(hp.target_shapes)
    hp.set_target_shapes()
    _refused(hp.target_shapes)                                         # on, before any step
    assert "switch them off first" in _refused(hp.set_targets, k)
    assert "switch them off first" in _refused(hp.set_targets, 0)
    hp.enqueue(f[1])
    assert "outstanding" in _refused(hp.set_target_shapes, False)
    hp.collect()
    # a step behind all of that still matches, and the room of oatgpu_target_shapes is checked
    hp2 = _hotpath(A, rows, cols, n)
    hp2.track(f[0])
    hp2.track(f[1])
    for t in range(2, 4):
        assert hp.track(f[t]) == hp2.track(f[t])
        _check_set(hp.target_shapes()[0], "fused", rows, cols, n, t)
    bufs = [_dev(x) for x in f[4:7]]
    assert hp.track_sequence_dev([b.data_ptr() for b in bufs]) == hp2.track_sequence_dev([b.data_ptr() for b in bufs])
    from oat_amd import ffi
    out = (ffi.Shape * (3 * n * k))()
    assert hp.lib.oatgpu_target_shapes(hp.ctx, out, 2) == E_INVALID    # one too small
    assert b"room for 2 frame sets, the latest call delivered 3" in hp.lib.oatgpu_last_error(hp.ctx)
    assert hp.lib.oatgpu_target_shapes(hp.ctx, None, 3) == E_INVALID
    assert hp.lib.oatgpu_target_shapes(hp.ctx, out, 3) == 3
    sets = hp.target_shapes()
    assert len(sets) == 3
    for i in range(3):
        _check_set(sets[i], "fused", rows, cols, n, 4 + i)
    hp.set_target_shapes()                                             # the setter starts the list over
    _refused(hp.target_shapes)
    hp.set_target_shapes(False)
    hp.set_targets(0)                                                  # ... allowed again with shapes off
    hp.close()
    hp2.close()


def test_tracks_update_delivers_no_shapes(A):
    case = next(c for c in PLANTED if c.name == "axes-24x32")
    det = _detector(A, "thresh", case, (0, 0))
    det.set_targets(4)
    det.set_tracks(kalman=TC.KALMAN, gate=25.0)
    det.set_target_shapes()
    det.detectPosition(case.img)
    before = det.target_shapes()
    (tset,) = det.targets()
    det.update_tracks([tset[0][0]])
    assert det.target_shapes() == before and len(det.tracks()) == 1
    det.close()
