"""GPU tests of target masks (oatgpu_set_target_mask_tensor / oatgpu_target_mask_tensor_sets; _Detector.set_target_mask_tensor /
.target_mask_tensor; k_target_mask in kernels_targetmask.hip).  Every element of every window is compared with the model
of tests/target_masks_ref.py -- integers, or fp32 / fp16 bit patterns: bit for bit, no tolerance anywhere -- fed with the oracle
chain's own masks, targets and shapes; at zoom 1 upright with the model on the context's own FINAL tap; and the ordinary results,
targets(), target_shapes(), target_crops(), the crop tensor, tracks(), filtered(), the taps and the states with those of a second
context that has the switch off.  Every frame is under 0.004 MP."""
import ctypes as C
import math

import numpy as np
import pytest

import crop_tensor_cases as TC
import crops_cases as CC
import target_masks_cases as MC
import target_masks_ref as MR
import targets_cases as T
import tracks_cases as TK

pytestmark = pytest.mark.gpu

E_INVALID = -1
THR, MORPH, FIN = 0, 1, 2


@pytest.fixture(scope="module")
def A():
    import oat_amd
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


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _same(got, want, tag):
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    if not MR.same_bits(got, want):
        as_int = {1: np.uint8, 2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
        bad = np.argwhere(np.ascontiguousarray(got).view(as_int) != np.ascontiguousarray(want).view(as_int))
        raise AssertionError((tag, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


def _make_tracker(A, kind, family, rows, cols, n, alpha=0.0, channels=3, **kw):
    """the tracker of a run: crops_cases' parameters for its sequences, no morphology for the designed ones"""
    if family == "motion":
        diff = T.DIFF if kind == "mix" else MC.DESIGNED_DIFF
        return A.MotionTracker(rows, cols, n_streams=n, channels=channels, area=MC.AREA, **diff, **kw)
    win, morph = T.sub_window(), T.SUB_MORPH if kind == "mix" else MC.DESIGNED_MORPH
    return A.SubtractionTracker(rows, cols, n_streams=n, channels=3, alpha=alpha, h_thresh=win["h"], s_thresh=win["s"], v_thresh=win["v"],
                                erode=morph[0], dilate=morph[1], area=MC.AREA, **kw)


class _Sequence:
    """the 11 frame sets of a run on the host and, one byte off an allocation's start, on the device"""

    def __init__(self, kind, family, rows, cols, n, channels=3):
        self.host = [[MC.sequence(kind, family, rows, cols, MC.variant_of(s), channels)[t] for s in range(n)] for t in range(MC.N_FRAMES)]
        self.bufs = [_dev(f, 1) for f in self.host]

    def ptr(self, t):
        return self.bufs[t][1]


def _call(tr, seq, how, t0, count, single=False):
    """one call of a run -> the positions of its frames"""
    if how == "track":
        return [tr.track(seq.host[t0])]
    if how == "track_dev":
        return [tr.track_dev(seq.ptr(t0))]
    if single:
        return [tr.track_dev(seq.ptr(t0 + i)) for i in range(count)]
    return tr.track_sequence_dev([seq.ptr(t0 + i) for i in range(count)])


def _run_setting(tr, seq, run, axis, zoom, dtype):
    """One setting of the switch on a tracker through MC.RUN_CALLS into one tensor of MC.CAPACITY entries: every element of the WHOLE
    tensor against the model behind every call -- the entries the call delivered, and those it must not touch."""
    kind, family, alpha, rows, cols, n, k, h, w = run
    tensor = tr.set_target_mask_tensor(h, w, axis=axis, zoom=zoom, dtype=dtype, capacity=MC.CAPACITY)
    want = [MC.entry(run, t, axis, zoom, dtype) for t in range(MC.N_FRAMES)]
    assert tuple(tensor.shape) == (MC.CAPACITY, n, k, h, w) and not _host(tensor).any()
    mirror = np.zeros((MC.CAPACITY,) + want[0].shape, want[0].dtype)
    assert "no call has delivered" in _refused(tr.target_mask_tensor)
    on = 0
    for i, (how, t0, count) in enumerate(MC.RUN_CALLS):
        if i in (0, MC.RESET_BEFORE):
            tr.reset()
        pos = _call(tr, seq, how, t0, count)
        view = tr.target_mask_tensor()
        assert len(pos) == count == len(view) and view.data_ptr() == tensor.data_ptr()            # zero-copy
        mirror[:count] = np.stack(want[t0:t0 + count])
        _same(_host(tensor), mirror, (kind, family, axis, zoom, dtype, how, t0, count))
        on += int((mirror[:count] != 0).sum())
    assert on > 0                                                                                  # (not a run of empty masks)
    return tensor


@pytest.mark.parametrize("axis", [False, True], ids=["upright", "axis"])
@pytest.mark.parametrize("case", range(len(MC.RUNS)))
def test_batched_trackers(A, case, axis):
    run = MC.RUNS[case]
    kind, family, alpha, rows, cols, n, k, h, w = run
    tr, seq = _make_tracker(A, kind, family, rows, cols, n, alpha), _Sequence(kind, family, rows, cols, n)
    tr.set_targets(k)
    tr.set_target_shapes()
    for zoom, dtype in MC.settings_of(case, axis):
        _run_setting(tr, seq, run, axis, zoom, dtype)
    tr.close()


def test_grey_frames(A):
    run = ("mix", "motion", 0.0, 37, 61, 3, 4, 16, 12)
    kind, family, alpha, rows, cols, n, k, h, w = run
    tr, seq = _make_tracker(A, kind, family, rows, cols, n, channels=1), _Sequence(kind, family, rows, cols, n, channels=1)
    tr.set_targets(k)
    tr.set_target_shapes()
    for axis, zoom, dtype in ((True, 1.37, "float16"), (False, 1.0, "uint8"), (True, 2.0, "float32")):
        _run_setting(tr, seq, run, axis, zoom, dtype)
    tr.close()


@pytest.mark.parametrize("family", MC.FAMILIES)
def test_a_paired_launch_against_single_launches(A, family):
    """The second frame of a paired front launch is labelled from ITS back half into ITS entry: an 11-frame sequence call against one
    device step a frame."""
    kind, rows, cols, n, k, h, w = "designed", 21, 150, 3, 4, 16, 12
    assert CC.paired_second(family, MC.PLAN_LONG)
    seq = _Sequence(kind, family, rows, cols, n)
    for axis, zoom, dtype in ((False, 1.0, "uint8"), (True, 2.0, "float16")):
        got = []
        for single in (False, True):
            tr = _make_tracker(A, kind, family, rows, cols, n)
            tr.set_targets(k)
            tr.set_target_shapes()
            tensor = tr.set_target_mask_tensor(h, w, axis=axis, zoom=zoom, dtype=dtype, capacity=MC.CAPACITY)
            if single:
                entries = []
                for t in range(MC.N_FRAMES):
                    tr.track_dev(seq.ptr(t))
                    entries.append(_host(tr.target_mask_tensor())[0].copy())
                got.append(np.stack(entries))
            else:
                tr.track_sequence_dev([seq.ptr(t) for t in range(MC.N_FRAMES)])
                got.append(_host(tr.target_mask_tensor()).copy())
            del tensor
            tr.close()
        _same(got[0], got[1], (family, axis, zoom))
        assert got[0].any()


@pytest.mark.parametrize("case", [7, 9, 10, 12, 4])
def test_the_upright_u8_mask_is_the_model_on_the_contexts_own_final_tap(A, case):
    """consistency between the taps: the model's labelling of what read_mask(FINAL) shows, through the windows of the context's own
    targets()"""
    import crops_ref as R
    run = MC.RUNS[case]
    kind, family, alpha, rows, cols, n, k, h, w = run
    tr, seq = _make_tracker(A, kind, family, rows, cols, n, alpha), _Sequence(kind, family, rows, cols, n)
    tr.set_targets(k)
    tr.set_target_mask_tensor(h, w, capacity=1)
    seen = 0
    for t in range(MC.N_FRAMES):
        tr.track_dev(seq.ptr(t))
        got = _host(tr.target_mask_tensor())[0]
        targets = tr.targets()[0]
        for s in range(n):
            first = MR.label8(tr.read_mask(FIN, s))
            for j in range(k):
                p = targets[s][0][j]
                rank = dict(valid=bool(p.position_valid), first_pixel=p.first_pixel)
                win = R.window(True, True, p.x, p.y) if rank["valid"] else R.INVALID
                want = MR.to_dtype(MR.window_on(first, rank, win, h, w), "uint8")
                _same(got[s, j], want, (case, t, s, j))
                seen += int(want.any())
    assert seen > 0
    tr.close()


# ----------------------------------------------------------------------------------- behind the RAW8 and the undistorting front end ----

def _masks_model(masks, k, axis, zoom, h, w, dtype):
    """[n, k, h, w]: the model on one frame set's oracle masks (bool [rows, cols] each)"""
    import crop_tensor_ref as TR
    import shapes_ref as SR
    out = []
    for m in masks:
        m8 = m.astype(np.uint8) * 255
        ranks = T.reference(m8, MC.AREA, k)[0]
        wins = TR.zoomed_windows(ranks, SR.reference(m8, MC.AREA, k) if axis else None, axis, zoom)
        out.append(MR.windows_mask(m8, ranks, wins, h, w, dtype))
    return np.stack(out)


def _front_end_run(tr, frames, want, k, h, w, other):
    """a motion tracker behind a front end `other` has switched on or will switch on: steps and a sequence call against the model on
    the oracle chain's masks of the frames the front end makes"""
    tr.set_targets(k)
    tr.set_target_shapes()
    assert "not supported" in _refused(tr.set_target_crops, h, w) and "not supported" in _refused(tr.set_target_crop_tensor, h, w)
    axis, zoom, dtype = True, 1.37, "float16"
    tr.set_target_mask_tensor(h, w, axis=axis, zoom=zoom, dtype=dtype, capacity=4)
    assert "not supported" in _refused(tr.set_target_crops, h, w) and "not supported" in _refused(tr.set_target_crop_tensor, h, w)
    on = 0
    bufs = [_dev(f, 0) for f in frames]
    for t in range(4):
        tr.track_dev(bufs[t][1]) if t % 2 else tr.track(frames[t])
        model = _masks_model([x[2] for x in want[t]], k, axis, zoom, h, w, dtype)
        _same(_host(tr.target_mask_tensor())[0], model, (other, t))
        on += int(model.any())
    tr.track_sequence_dev([bufs[t][1] for t in range(4, 8)])
    got = _host(tr.target_mask_tensor())
    for i, t in enumerate(range(4, 8)):
        model = _masks_model([x[2] for x in want[t]], k, axis, zoom, h, w, dtype)
        _same(got[i], model, (other, "seq", t))
        on += int(model.any())
    assert on >= 4
    # ... and the other order of switching: the front end off and on again with the mask switch on
    return tr


def test_behind_the_raw8_front_end(A):
    import diff_cases as D
    import tracker_bayer_cases as TB
    rows, cols, k, h, w = 37, 91, 4, 16, 12
    rc, want = TB.diff_want(rows, cols, TB.THREE)
    c = rc.c
    tr = A.MotionTracker(rows, cols, n_streams=3, channels=3, diff_threshold=c.diff_threshold, blur=c.blur, area=D.AREA,
                         bayer=list(TB.THREE))
    _front_end_run(tr, rc.raw, want, k, h, w, "bayer")
    tr.bayer(None)                                                     # the front end may go and come with the masks on
    tr.bayer(list(TB.THREE))
    tr.close()


def test_behind_the_undistorting_front_end(A):
    import diff_cases as D
    import tracker_undistort_cases as TU
    rows, cols, k, h, w = 37, 91, 4, 16, 12
    uc, want = TU.diff_want(rows, cols, 3, TU.THREE)
    c = uc.c
    assert tuple(MC.AREA) == tuple(D.AREA)
    tr = A.MotionTracker(rows, cols, n_streams=3, channels=3, diff_threshold=c.diff_threshold, blur=c.blur, area=D.AREA)
    for s, name in enumerate(TU.THREE):
        tr.set_undistort(s, *TU.calibration(rows, cols, name))
    tr.undistort(True)
    _front_end_run(tr, uc.given, want, k, h, w, "undistort")
    tr.undistort(False)
    tr.undistort(True)
    tr.close()


def test_the_front_ends_switch_on_behind_the_mask_switch(A):
    """the other order: masks first, then RAW8 or undistortion -- not a refusal, and the masks follow the new pixel domain"""
    import diff_cases as D
    import tracker_bayer_cases as TB
    rows, cols, k, h, w = 37, 91, 4, 16, 12
    rc, want = TB.diff_want(rows, cols, TB.THREE)
    c = rc.c
    tr = A.MotionTracker(rows, cols, n_streams=3, channels=3, diff_threshold=c.diff_threshold, blur=c.blur, area=D.AREA)
    tr.set_targets(k)
    tr.set_target_mask_tensor(h, w, dtype="uint8", capacity=1)
    tr.bayer(list(TB.THREE))
    for t in range(3):
        tr.track(rc.raw[t])
        _same(_host(tr.target_mask_tensor())[0], _masks_model([x[2] for x in want[t]], k, False, 1.0, h, w, "uint8"), t)
    tr.close()


# ------------------------------------------------------------------------------------------------- beside the other riders ----

def test_a_mask_and_a_crop_tensor_of_one_setting_each_equal_to_its_model(A):
    run = MC.RUNS[7]                                                   # designed, motion, 48 x 64, 3 streams, K = 4, 16 x 12
    kind, family, alpha, rows, cols, n, k, h, w = run
    tr, seq = _make_tracker(A, kind, family, rows, cols, n), _Sequence(kind, family, rows, cols, n)
    tr.set_targets(k)
    tr.set_target_shapes()
    axis, zoom = True, 2.0
    crop = tr.set_target_crop_tensor(h, w, axis=axis, zoom=zoom, dtype="uint8", capacity=MC.N_FRAMES)
    mask = tr.set_target_mask_tensor(h, w, axis=axis, zoom=zoom, dtype="float32", capacity=MC.N_FRAMES)
    tr.track_sequence_dev([seq.ptr(t) for t in range(MC.N_FRAMES)])
    assert len(tr.target_mask_tensor()) == len(tr.target_crop_tensor()) == MC.N_FRAMES
    import crops_ref as R
    for t in range(MC.N_FRAMES):
        _same(_host(mask)[t], MC.entry(run, t, axis, zoom, "float32"), ("mask", t))
        for s in range(n):
            v = MC.variant_of(s)
            wins = MC.sequence_windows(kind, family, rows, cols, v, alpha, k, axis, zoom)[t]
            frame = MC.sequence(kind, family, rows, cols, v)[t]
            _same(_host(crop)[t, s], np.stack([R.crop(frame, win, h, w) for win in wins]), ("crop", t, s))
    tr.close()


KALMAN = dict(kalman=dict(dt=0.02, timeout=0.1, sigma_accel=5.0, sigma_noise=0.5))


def _run_passengers(A, family, rows, cols, n, alpha, k, h, w, seq, masks):
    """-> per frame (positions, targets, shapes, crops, filtered, tracks, the crop tensor's entry); the taps and the state behind the
    last frame"""
    tr = _make_tracker(A, "mix", family, rows, cols, n, alpha)
    tr.set_filters(**KALMAN)
    tr.set_targets(k)
    tr.set_tracks(**TK.image_config())
    tr.set_target_shapes()
    tr.set_target_crops(h, w, axis=True)
    tr.set_target_crop_tensor(h, w, axis=True, zoom=1.37, dtype="float16", scale=1.0 / 255.0, capacity=5)
    if masks:
        tr.set_target_mask_tensor(h + 3, 2 * w, axis=True, zoom=0.5, dtype="float32", capacity=5)      # another size than the crops'
    out = []
    for how, t0, count in TC.calls_of(MC.PLAN):
        pos = _call(tr, seq, how, t0, count)
        tensor = _host(tr.target_crop_tensor()).copy()
        out += list(zip(pos, tr.targets(), tr.target_shapes(), tr.target_crops(), tr.filtered(), tr.tracks(), tensor))
        if masks:
            assert len(tr.target_mask_tensor()) == count
    taps = [[tr.read_mask(which, s) for which in (THR, MORPH, FIN)] for s in range(n)]
    state = [tr.state(s) for s in range(n)] if family == "subtraction" else None
    tr.close()
    return out, taps, state


@pytest.mark.parametrize("family,alpha", [("motion", 0.0), ("subtraction", 0.05)])
def test_masks_are_read_only_passengers(A, family, alpha):
    rows, cols, n, k, h, w = 37, 61, 3, 4, 16, 12
    seq = _Sequence("mix", family, rows, cols, n)
    got, taps, state = _run_passengers(A, family, rows, cols, n, alpha, k, h, w, seq, True)
    plain, ptaps, pstate = _run_passengers(A, family, rows, cols, n, alpha, k, h, w, seq, False)
    assert len(got) == len(plain) == 10
    for t, (a, b) in enumerate(zip(got, plain)):
        assert a[0] == b[0], (t, "the ordinary results move with the switch on")
        assert a[1] == b[1] and a[2] == b[2], (t, "the target or shape sets move with the switch on")
        assert np.array_equal(a[3], b[3]), (t, "the crop sets move with the switch on")
        assert a[4] == b[4] and a[5] == b[5], (t, "the filtered records or the tracks move with the switch on")
        assert MR.same_bits(a[6], b[6]), (t, "the crop tensor moves with the switch on")
    for x, y in zip(taps, ptaps):
        for p, q in zip(x, y):
            assert (p == q).all()
    if state is not None:
        for (bg, acc), (pbg, pacc) in zip(state, pstate):
            assert (bg == pbg).all() and (acc == pacc).all()


# ------------------------------------------------------------------------------------------------------------ refusals ----

def test_a_sequence_call_longer_than_the_capacity_is_refused_and_the_next_call_works(A):
    for family, case in (("subtraction", 11), ("motion", 7)):
        run = MC.RUNS[case]
        kind, family_, alpha, rows, cols, n, k, h, w = run
        assert family_ == family and kind == "designed"
        tr, seq = _make_tracker(A, kind, family, rows, cols, n), _Sequence(kind, family, rows, cols, n)
        plain = _make_tracker(A, kind, family, rows, cols, n)
        for x in (tr, plain):
            x.set_targets(k)
        tensor = tr.set_target_mask_tensor(h, w, zoom=2.0, dtype="float16", capacity=4)
        assert "4 entries" in _refused(tr.track_sequence_dev, [seq.ptr(t) for t in range(11)])
        assert "4 entries" in _refused(tr.track_sequence_dev, [seq.ptr(t) for t in range(5)])
        assert not _host(tensor).any() and "no call has delivered" in _refused(tr.target_mask_tensor)      # nothing was launched
        _refused(tr.targets)
        # ... and nothing changed: the next call is the first of a fresh tracker
        pos = tr.track_sequence_dev([seq.ptr(t) for t in range(4)])
        assert pos == plain.track_sequence_dev([seq.ptr(t) for t in range(4)]) and tr.targets() == plain.targets()
        want = np.stack([MC.entry(run, t, False, 2.0, "float16") for t in range(4)])
        _same(_host(tr.target_mask_tensor()), want, family)
        assert want.any()
        tr.close()
        plain.close()


def test_refusals_each_leaving_a_working_context(A):
    import torch
    from oat_amd import ffi
    run = MC.RUNS[11]                                                  # designed, subtraction, 37 x 61, 3 streams, K = 4, 5 x 4
    kind, family, alpha, rows, cols, n, k, h, w = run
    tr, seq = _make_tracker(A, kind, family, rows, cols, n), _Sequence(kind, family, rows, cols, n)
    lib, ctx = tr.lib, tr.ctx
    room = torch.zeros(2 * n * k * h * w + 64, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    out = C.c_void_p(room.data_ptr())

    def text(rc):
        assert rc == E_INVALID, rc
        return lib.oatgpu_last_error(ctx).decode()

    setter = lib.oatgpu_set_target_mask_tensor
    U, F32 = ffi.CROP_UPRIGHT, ffi.TENSOR_F32
    assert "off" in _refused(tr.target_mask_tensor)                                              # the switch is off
    assert "targets are off" in _refused(tr.set_target_mask_tensor, h, w)                        # targets off
    tr.set_target_mask_tensor(None)                                                              # ... off is always allowed
    tr.set_targets(k)
    assert "shapes" in _refused(tr.set_target_mask_tensor, h, w, axis=True)                      # axis without shapes
    for bad in ((0, 8), (257, 8), (8, 0), (8, 2), (8, 6), (8, 260), (-1, -4)):
        assert "a window is" in _refused(tr.set_target_mask_tensor, *bad)
    assert "mode" in text(setter(ctx, 3, h, w, 1.0, F32, out, 2)) and "mode" in text(setter(ctx, -1, h, w, 1.0, F32, out, 2))
    for dtype in (-1, 3, 99):
        assert "dtype" in text(setter(ctx, U, h, w, 1.0, dtype, out, 2))
    with pytest.raises(ValueError):
        tr.set_target_mask_tensor(h, w, dtype="int8")
    for zoom in (0.0, 0.0624, 16.001, -1.0, math.nan, math.inf, -math.inf):
        assert "zoom" in text(setter(ctx, U, h, w, zoom, F32, out, 2)), zoom
    assert "null" in text(setter(ctx, U, h, w, 1.0, F32, None, 2))
    for off in (1, 4, 8):
        assert "aligned" in text(setter(ctx, U, h, w, 1.0, F32, C.c_void_p(room.data_ptr() + off), 2))
    for cap in (0, -3):
        assert "at least one" in text(setter(ctx, U, h, w, 1.0, F32, out, cap))
    assert "off" in _refused(tr.target_mask_tensor)                                              # nothing of all that switched it on
    assert not _host(room).any()
    # the switch on: what it refuses while it is on
    tr.set_target_mask_tensor(h, w, dtype="float32", capacity=2)
    assert "no call has delivered" in _refused(tr.target_mask_tensor)
    assert "target masks" in _refused(tr.set_targets, k) and "switch them off first" in _refused(tr.set_targets, 0)
    tr.set_target_shapes()
    tr.set_target_shapes(False)                                                                  # upright masks do not need shapes
    tr.set_target_shapes()
    tr.set_target_mask_tensor(h, w, axis=True, zoom=0.5, dtype="uint8", capacity=2)
    assert "target masks" in _refused(tr.set_target_shapes, False)                               # axis masks do
    assert "2 entries" in _refused(tr.track_sequence_dev, [seq.ptr(t) for t in range(3)])
    # steps behind all of that match
    for t in range(2):
        tr.track(seq.host[t])
        _same(_host(tr.target_mask_tensor())[0], MC.entry(run, t, True, 0.5, "uint8"), t)
    tr.track_sequence_dev([seq.ptr(2), seq.ptr(3)])
    for i in range(2):
        _same(_host(tr.target_mask_tensor())[i], MC.entry(run, 2 + i, True, 0.5, "uint8"), 2 + i)
    tr.set_target_mask_tensor(None)
    assert "off" in _refused(tr.target_mask_tensor)
    tr.set_target_shapes(False)
    tr.set_targets(0)                                                                            # ... allowed again with the switch off
    tr.close()


def test_results_outstanding_and_calls_that_deliver_no_mask(A):
    """The fused tracker's own calls deliver none and behave as with the switch off; its outstanding results refuse the switch."""
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
    assert "outstanding" in _refused(hp.set_target_mask_tensor, h, w)
    assert hp.collect() == plain.collect()
    hp.stage(0, f[1][0])                                                        # a frame set partly staged
    _refused(hp.set_target_mask_tensor, h, w)
    hp.stage_abort()
    tensor = hp.set_target_mask_tensor(h, w, capacity=3)
    for t in range(1, 6):
        assert hp.track(f[t]) == plain.track(f[t]), t
        assert hp.targets() == plain.targets(), t
        assert "no call has delivered" in _refused(hp.target_mask_tensor)
    assert not _host(tensor).any()
    hp.close()
    plain.close()
