"""GPU tests of target crops (oatgpu_set_target_crops / oatgpu_target_crops / oatgpu_crop_windows_dev; _Detector.set_target_crops /
.target_crops / .crop_windows; k_target_crops in kernels_crops.hip).  Every byte of every window is compared with the
model of tests/crops_ref.py -- integers: bit for bit, no tolerance anywhere -- fed with the oracle chain's own targets and shapes;
and the ordinary results, targets(), target_shapes(), tracks(), filtered(), the taps and the states with those of a second context
that has crops off.  Every frame is under 0.004 MP."""
import numpy as np
import pytest

import crops_cases as CC
import crops_ref as R
import oracle_lib as O
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


def _dev(frames, offset=0):
    """frames of one set, stream-major, in device memory `offset` bytes behind an allocation's start -> (tensor kept alive, address)"""
    import torch
    flat = np.concatenate([np.ascontiguousarray(f).reshape(-1) for f in frames])
    buf = torch.zeros(flat.size + offset, dtype=torch.uint8, device="cuda")
    buf[offset:] = torch.from_numpy(flat).cuda()
    torch.cuda.synchronize()
    return buf, buf.data_ptr() + offset


def _refused(fn, *a, **kw):
    from oat_amd.ffi import OatGpuError
    with pytest.raises(OatGpuError) as e:
        fn(*a, **kw)
    assert e.value.code == E_INVALID, e.value
    return str(e.value)


def _same(got, want, tag):
    assert got.shape == want.shape and got.dtype == np.uint8, (tag, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError((tag, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


# ------------------------------------------------------------------------------------------------- oatgpu_crop_windows_dev ----

EXPLICIT = [(rows, cols, h, w, ch) for rows, cols in CC.GEOMETRIES for h, w in CC.CROP_SIZES for ch in (1, 3)]


def _cropper(A, rows, cols, n, channels):
    """any detector will do: the call needs no switch"""
    return A.MotionTracker(rows, cols, n_streams=n, channels=channels, area=T.AREA, **T.DIFF)


@pytest.mark.parametrize("rows,cols,h,w,channels", EXPLICIT)
def test_explicit_windows_against_the_model(A, rows, cols, h, w, channels):
    gs = [g for kind in CC.explicit_windows(rows, cols, h, w) for g in CC.groups(kind)]
    model = {}

    def want(variant, g):
        if (variant, g) not in model:
            model[(variant, g)] = np.stack([R.crop(CC.pattern(rows, cols, channels, variant), win, h, w) for win in gs[g]])
        return model[(variant, g)]
    for n in CC.STREAMS:
        det = _cropper(A, rows, cols, n, channels)
        frames = [CC.pattern(rows, cols, channels, CC.variant_of(s)) for s in range(n)]
        calls = len(gs) if n == 1 else 2
        for call in range(calls):
            offset = (call + n) % 2                                    # the frame set one byte off a 256-byte boundary, and on it
            keep, ptr = _dev(frames, offset)
            pick = [(call + 5 * s) % len(gs) for s in range(n)]
            got = det.crop_windows(ptr, [gs[g] for g in pick], h, w)
            for s in range(n):
                _same(got[s], want(CC.variant_of(s), pick[s]), (n, call, s, pick[s]))
            del keep
        det.close()


def test_fewer_windows_a_stream_and_window_structs(A):
    from oat_amd import ffi
    rows, cols, h, w = 37, 61, 16, 12
    det = _cropper(A, rows, cols, 3, 3)
    frames = [CC.pattern(rows, cols, 3, s) for s in range(3)]
    keep, ptr = _dev(frames, 1)
    turned = CC.explicit_windows(rows, cols, h, w)[1]
    for per in (1, 3):
        wins = [[turned[(7 * s + q) % len(turned)] for q in range(per)] for s in range(3)]
        asc = [[ffi.CropWindow(int(v), int(u), cx, cy, ax, ay) for v, u, cx, cy, ax, ay in cam] for cam in wins]
        got = det.crop_windows(ptr, asc, h, w)
        _same(got, R.crop_set(frames, wins, h, w), per)
    # a larger window behind a smaller one: the call grows its buffers
    got = det.crop_windows(ptr, [[turned[0]]] * 3, 256, 256)
    _same(got, R.crop_set(frames, [[turned[0]]] * 3, 256, 256), "256")
    det.close()


# ------------------------------------------------------------------------------------------------- the batched trackers ----

KALMAN = dict(kalman=dict(dt=0.02, timeout=0.1, sigma_accel=5.0, sigma_noise=0.5))


def _make_tracker(A, family, rows, cols, n, alpha=0.0, channels=3):
    if family == "motion":
        return A.MotionTracker(rows, cols, n_streams=n, channels=channels, area=T.AREA, **T.DIFF)
    win = T.sub_window()
    return A.SubtractionTracker(rows, cols, n_streams=n, channels=3, alpha=alpha, h_thresh=win["h"], s_thresh=win["s"], v_thresh=win["v"],
                                erode=T.SUB_MORPH[0], dilate=T.SUB_MORPH[1], area=T.AREA)


def _frames_at(family, rows, cols, n, t, channels=3):
    return [CC.sequence(family, rows, cols, CC.variant_of(s), channels)[t] for s in range(n)]


def _run_tracker(A, family, rows, cols, n, alpha, k, crops, extras, plan=CC.PLAN, channels=3, single=False):
    """crops: None, or (h, w, axis).  -> per frame: (positions, target set, shape set, crop set or None, filtered set or None, track set
    or None); then the taps and the state behind the last frame.  single: every frame of a sequence call as a device step instead."""
    tr = _make_tracker(A, family, rows, cols, n, alpha, channels)
    if extras:
        tr.set_filters(**KALMAN)
    tr.set_targets(k)
    if extras:
        tr.set_tracks(**TC.image_config())
    tr.set_target_shapes()
    if crops:
        tr.set_target_crops(crops[0], crops[1], axis=crops[2])
    out, t = [], 0
    for how, count in plan:
        frames = [_frames_at(family, rows, cols, n, t + i, channels) for i in range(count)]
        steps = [(how, frames)] if not (single and how == "seq") else [("track_dev", [f]) for f in frames]
        for how_, fs in steps:
            if how_ == "track":
                pos = [tr.track(fs[0])]
            else:
                bufs = [_dev(f, 1 if crops else 0) for f in fs]
                pos = [tr.track_dev(bufs[0][1])] if how_ == "track_dev" else tr.track_sequence_dev([b[1] for b in bufs])
            m = len(fs)
            tgt, shp = tr.targets(), tr.target_shapes()
            crp = tr.target_crops() if crops else [None] * m
            filt = tr.filtered() if extras else [None] * m
            trk = tr.tracks() if extras else [None] * m
            assert len(pos) == len(tgt) == len(shp) == len(crp) == len(filt) == len(trk) == m, (how_, m, len(crp))
            if crops:
                assert np.array_equal(tr.target_crops(), crp)                 # nothing is consumed
            out += list(zip(pos, tgt, shp, crp, filt, trk))
        t += count
    taps = [[tr.read_mask(w, s) for w in (THR, MORPH, FIN)] for s in range(min(n, 4))]
    state = [tr.state(s) for s in range(min(n, 4))] if family == "subtraction" else None
    tr.close()
    return out, taps, state


def _check_crops(crp, family, rows, cols, n, t, alpha, k, axis, h, w, channels=3):
    """one frame's crop set [n, k, h, w(, 3)] against the model"""
    assert crp.shape[:2] == (n, k)
    for s in range(n):
        want = CC.sequence_crops(family, rows, cols, CC.variant_of(s), alpha, k, axis, h, w, channels)[t]
        _same(crp[s], want, (family, rows, cols, n, t, s, axis))


def _check_model_inputs(tgt, shp, family, rows, cols, n, t, alpha, k):
    """the model is fed the oracle chain's targets and shapes: the device's are the same"""
    import shapes_ref as SR
    from diff_cases import same_dict
    for s in range(n):
        v = CC.variant_of(s)
        ranks, found = CC.sequence_targets(family, rows, cols, v, alpha, k)[t]
        got_ranks, got_found = tgt[s]
        as_dict = lambda p: dict(valid=p.position_valid, area=p.area, a00=p.a00, a10=p.a10, a01=p.a01, first_pixel=p.first_pixel,     # noqa: E731
                                 x=p.x, y=p.y)
        assert got_found == found and all(same_dict(as_dict(g), r) for g, r in zip(got_ranks, ranks)), (t, s)
        for g, r in zip(shp[s], CC.sequence_shapes(family, rows, cols, v, alpha, k)[t]):
            assert SR.same({f: getattr(g, f) for f in SR.FIELDS}, r), (t, s)


@pytest.mark.parametrize("axis", [False, True], ids=["upright", "axis"])
@pytest.mark.parametrize("family,alpha,rows,cols,n,k,h,w", CC.TRACKER_RUNS)
def test_batched_trackers(A, family, alpha, rows, cols, n, k, h, w, axis):
    extras = n == 3                                # the trackers' filter chain and target tracks ride along
    got, taps, state = _run_tracker(A, family, rows, cols, n, alpha, k, (h, w, axis), extras)
    plain, ptaps, pstate = _run_tracker(A, family, rows, cols, n, alpha, k, None, extras)
    assert len(got) == 10
    for t, ((pos, tgt, shp, crp, filt, trk), (ppos, ptgt, pshp, _, pfilt, ptrk)) in enumerate(zip(got, plain)):
        assert pos == ppos, (t, "the ordinary results move with crops on")
        assert tgt == ptgt and shp == pshp, (t, "the target or shape sets move with crops on")
        assert filt == pfilt and trk == ptrk, (t, "the filtered records or the tracks move with crops on")
        if n <= 3:
            _check_model_inputs(tgt, shp, family, rows, cols, n, t, alpha, k)
        _check_crops(crp, family, rows, cols, n, t, alpha, k, axis, h, w)
    for a, b in zip(taps, ptaps):
        for x, y in zip(a, b):
            assert (x == y).all()
    if state is not None:
        for (bg, acc), (pbg, pacc) in zip(state, pstate):
            assert (bg == pbg).all() and (acc == pacc).all()


@pytest.mark.parametrize("family,alpha", [("motion", 0.0), ("subtraction", 0.05)])
def test_batched_trackers_one_long_sequence_call(A, family, alpha):
    """11 frames in one call: every one of the tracker's four slots is taken again and again"""
    rows, cols, n, k, h, w = 37, 61, 3, 4, 16, 12
    for axis in (False, True):
        got, _, _ = _run_tracker(A, family, rows, cols, n, alpha, k, (h, w, axis), False, plan=CC.PLAN_LONG)
        assert len(got) == 11
        for t, (_, _, _, crp, _, _) in enumerate(got):
            _check_crops(crp, family, rows, cols, n, t, alpha, k, axis, h, w)


def test_grey_frames(A):
    family, alpha, rows, cols, n, k, h, w = "motion", 0.0, 37, 61, 3, 4, 16, 12
    for axis in (False, True):
        got, _, _ = _run_tracker(A, family, rows, cols, n, alpha, k, (h, w, axis), False, channels=1)
        for t, (_, _, _, crp, _, _) in enumerate(got):
            assert crp.shape == (n, k, h, w)
            _check_crops(crp, family, rows, cols, n, t, alpha, k, axis, h, w, channels=1)


@pytest.mark.parametrize("family,alpha", [("motion", 0.0), ("subtraction", 0.05)])
def test_a_paired_launch_against_single_launches(A, family, alpha):
    """The second frame of a paired front launch is cut from ITS frame set: sequence calls against one device step a frame."""
    rows, cols, n, k, h, w = 48, 64, 3, 4, 16, 12
    assert CC.paired_second(family, CC.PLAN_LONG)
    for axis in (False, True):
        paired, _, _ = _run_tracker(A, family, rows, cols, n, alpha, k, (h, w, axis), False, plan=CC.PLAN_LONG)
        single, _, _ = _run_tracker(A, family, rows, cols, n, alpha, k, (h, w, axis), False, plan=CC.PLAN_LONG, single=True)
        assert len(paired) == len(single) == 11
        for t, (a, b) in enumerate(zip(paired, single)):
            assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2], t
            _same(a[3], b[3], (family, axis, t))


def test_a_tracker_switched_on_behind_crops_has_its_sets(A):
    rows, cols, n, k, h, w = 48, 64, 3, 4, 8, 8
    for family, sw in (("motion", "oatgpu_set_diff_tracker"), ("subtraction", "oatgpu_set_bsub_tracker")):
        tr = _make_tracker(A, family, rows, cols, n)
        tr._chk(getattr(tr.lib, sw)(tr.ctx, 0))
        tr.set_targets(k)
        tr.set_target_shapes()
        tr.set_target_crops(h, w, axis=True)
        tr._chk(getattr(tr.lib, sw)(tr.ctx, 1))
        for t in range(5):
            tr.track(_frames_at(family, rows, cols, n, t))
            _check_crops(tr.target_crops()[0], family, rows, cols, n, t, 0.0, k, True, h, w)
        tr.close()


def test_the_crop_of_a_track_follows_it_across_a_rank_swap(A):
    """tracks_cases' image sequence: three blocks of equal area whose ranks cross.  crops[track.rank] is the window of the track's
    blob: the upright window at the track's raw detection."""
    rows, cols, channels = TC.GEOMETRIES[0]
    k, h, w = TC.IMG_K, 16, 12
    tr = A.MotionTracker(rows, cols, n_streams=1, channels=channels, area=TC.DC.AREA, **TC.DIFF)
    tr.set_targets(k)
    tr.set_tracks(**TC.image_config())
    tr.set_target_crops(h, w)
    ranks_of, seen = {}, 0
    for t, f in enumerate(TC.sequence("motion", rows, cols, channels, 0)):
        tr.track([f])
        ((tgt, _),), (trk,), crp = tr.targets()[0], tr.tracks()[0], tr.target_crops()[0, 0]
        for slot in trk:
            if slot.id and slot.rank >= 0:
                p = tgt[slot.rank]
                assert p.position_valid, (t, slot)
                _same(crp[slot.rank], R.crop(f, R.window(True, True, p.x, p.y), h, w), (t, slot.id))
                assert crp[slot.rank].any()
                ranks_of.setdefault(slot.id, set()).add(slot.rank)
                seen += 1
        for j in range(k):
            if not tgt[j].position_valid:
                assert not crp[j].any(), (t, j)
    tr.close()
    assert seen > 20 and any(len(r) > 1 for r in ranks_of.values()), ("no track changed its rank: pick another sequence", ranks_of)


# ------------------------------------------------------------------------------------------------------------ refusals ----

def test_refusals_each_leaving_a_working_context(A):
    from oat_amd import ffi
    family, alpha, rows, cols, n, k, h, w = "subtraction", 0.0, 37, 61, 3, 4, 16, 12
    tr = _make_tracker(A, family, rows, cols, n)
    frames = [_frames_at(family, rows, cols, n, t) for t in range(CC.N_FRAMES)]
    assert "off" in _refused(tr.target_crops)                                   # crops off
    assert "targets are off" in _refused(tr.set_target_crops, h, w)             # targets off
    tr.set_target_crops(None)                                                   # ... off is always allowed
    tr.set_targets(k)
    assert "shapes" in _refused(tr.set_target_crops, h, w, axis=True)           # axis without shapes
    for bad in ((0, 8), (257, 8), (8, 0), (8, 2), (8, 6), (8, 260), (-1, -4)):
        assert "a window is" in _refused(tr.set_target_crops, *bad)
    assert tr.lib.oatgpu_set_target_crops(tr.ctx, 3, h, w) == E_INVALID
    assert tr.lib.oatgpu_set_target_crops(tr.ctx, -1, h, w) == E_INVALID
    tr.bayer("RGGB")                                                            # RAW8 front end
    assert "Bayer" in _refused(tr.set_target_crops, h, w)
    tr.bayer(None)
    K = [60.0, 0, cols / 2, 0, 60.0, rows / 2, 0, 0, 1]
    for s in range(n):
        tr.set_undistort(s, K, [0.1, 0.0, 0.0, 0.0, 0.0])
    tr.undistort(True)                                                          # undistorting front end
    assert "undistortion" in _refused(tr.set_target_crops, h, w)
    tr.undistort(False)
    assert "off" in _refused(tr.target_crops)                                   # nothing of all that switched crops on
    tr.set_target_crops(h, w)
    assert "no call has delivered" in _refused(tr.target_crops)                 # on, before any step
    _refused(tr.targets)                                                        # (the setter starts the lists over)
    assert "target crops" in _refused(tr.bayer, "RGGB")                         # while crops are on
    assert "target crops" in _refused(tr.undistort, True)
    assert "switch them off first" in _refused(tr.set_targets, k)
    assert "switch them off first" in _refused(tr.set_targets, 0)
    tr.set_target_shapes()
    tr.set_target_shapes(False)                                                 # upright crops do not need shapes
    tr.set_target_shapes()
    tr.set_target_crops(h, w, axis=True)
    assert "switch them off first" in _refused(tr.set_target_shapes, False)     # axis crops do
    # oatgpu_crop_windows_dev's own
    keep, ptr = _dev(frames[0])
    wins = [[R.window(True, True, 10, 10)]] * n
    assert "windows a stream" in _refused(tr.crop_windows, ptr, [[R.INVALID] * 9] * n, h, w)
    assert "windows a stream" in _refused(tr.crop_windows, ptr, [[]] * n, h, w)
    assert "a window is" in _refused(tr.crop_windows, ptr, wins, 8, 6)
    assert "null" in _refused(tr.crop_windows, 0, wins, h, w)
    # a step behind all of that matches, and the room of oatgpu_target_crops is checked
    for t in range(2):
        tr.track(frames[t])
        _check_crops(tr.target_crops()[0], family, rows, cols, n, t, alpha, k, True, h, w)
    bufs = [_dev(f) for f in frames[2:5]]
    tr.track_sequence_dev([b[1] for b in bufs])
    out = np.zeros((3, n, k, h, w, 3), np.uint8)
    assert tr.lib.oatgpu_target_crops(tr.ctx, ffi.u8(out), 2) == E_INVALID      # one too small
    assert b"room for 2 frame sets, the latest call delivered 3" in tr.lib.oatgpu_last_error(tr.ctx)
    assert not out.any()
    assert tr.lib.oatgpu_target_crops(tr.ctx, None, 3) == E_INVALID
    assert tr.lib.oatgpu_target_crops(tr.ctx, ffi.u8(out), 3) == 3
    sets = tr.target_crops()
    assert np.array_equal(sets, out)
    for i in range(3):
        _check_crops(sets[i], family, rows, cols, n, 2 + i, alpha, k, True, h, w)
    tr.set_target_crops(h, w, axis=True)                                        # the setter starts the list over
    _refused(tr.target_crops)
    tr.set_target_crops(None)
    assert "off" in _refused(tr.target_crops)
    tr.set_target_shapes(False)
    tr.set_targets(0)                                                           # ... allowed again with crops off
    tr.close()


def test_results_outstanding_and_calls_that_deliver_no_crops(A):
    """The fused tracker's own calls deliver no crops and behave as with crops off; its outstanding results refuse the switch and
    oatgpu_crop_windows_dev."""
    import shapes_cases as S
    rows, cols, n, k, h, w = 48, 64, 2, 4, 8, 8
    mk = lambda: A.HotPath(rows, cols, n_streams=n, adaptation_coeff=T.FUSED_LR, erode=T.FUSED_MORPH[0], dilate=T.FUSED_MORPH[1],     # noqa: E731
                           area=T.AREA, ring_depth=4, **T.FUSED_WIN)
    hp, plain = mk(), mk()
    f = [[S.frames_of("fused", rows, cols, S.variant_of(s))[t] for s in range(n)] for t in range(6)]
    for x in (hp, plain):
        x.set_targets(k)
    hp.enqueue(f[0])
    plain.enqueue(f[0])
    assert "outstanding" in _refused(hp.set_target_crops, h, w)
    keep, ptr = _dev(f[0])
    assert "outstanding" in _refused(hp.crop_windows, ptr, [[R.window(True, True, 5, 5)]] * n, h, w)
    assert hp.collect() == plain.collect()
    hp.stage(0, f[1][0])                                                        # a frame set partly staged
    _refused(hp.set_target_crops, h, w)
    hp.stage_abort()
    hp.set_target_crops(h, w)
    for t in range(1, 6):
        assert hp.track(f[t]) == plain.track(f[t]), t
        assert hp.targets() == plain.targets(), t
        assert "no call has delivered" in _refused(hp.target_crops)
    got = hp.crop_windows(ptr, [[R.window(True, True, 30.5, 20.5)]] * n, h, w)   # ... and the stand-alone call is how it reaches crops
    _same(got, R.crop_set(f[0], [[R.window(True, True, 30.5, 20.5)]] * n, h, w), "hotpath")
    hp.close()
    plain.close()


def test_steps_with_crops_on_off_and_other_calls_in_turn(A):
    family, alpha, rows, cols, n, k = "motion", 0.0, 37, 61, 3, 4
    tr, plain = _make_tracker(A, family, rows, cols, n), _make_tracker(A, family, rows, cols, n)
    for x in (tr, plain):
        x.set_targets(k)
        x.set_target_shapes()
    modes = [None, (16, 12, False), (16, 12, True), None, (5, 4, True), (33, 64, False), (8, 8, True), (8, 8, False), None, (64, 128, True)]
    pat = [CC.pattern(rows, cols, 3, s) for s in range(n)]
    keep, ptr = _dev(pat, 1)
    wins = [CC.groups(CC.explicit_windows(rows, cols, 8, 8)[1])[s] for s in range(n)]
    for t, mode in enumerate(modes):
        frames = _frames_at(family, rows, cols, n, t)
        if mode is None:
            tr.set_target_crops(None)
        else:
            tr.set_target_crops(mode[0], mode[1], axis=mode[2])
        if t % 3 == 1:                                                          # another call of the context in between
            _same(tr.crop_windows(ptr, wins, 8, 8), R.crop_set(pat, wins, 8, 8), t)
        buf = _dev(frames, 1)
        pos = tr.track(frames) if t % 2 else tr.track_dev(buf[1])
        assert pos == (plain.track(frames) if t % 2 else plain.track_dev(buf[1])), t
        assert tr.targets() == plain.targets() and tr.target_shapes() == plain.target_shapes(), t
        if mode is None:
            assert "off" in _refused(tr.target_crops)
        else:
            _check_crops(tr.target_crops()[0], family, rows, cols, n, t, alpha, k, mode[2], mode[0], mode[1])
        if t % 3 == 2:
            tr.read_mask(MORPH, 1)
            _same(tr.crop_windows(ptr, wins, 8, 8), R.crop_set(pat, wins, 8, 8), t)
            if mode is not None:                                                # the stand-alone call touches nothing a switch owns
                _check_crops(tr.target_crops()[0], family, rows, cols, n, t, alpha, k, mode[2], mode[0], mode[1])
    tr.close()
    plain.close()
