"""GPU tests of Bayer RAW8 frames inside the fused tracker (oatgpu_set_track_bayer, HotPath.bayer): the chain demosaic ->
[undistort] -> mask -> mog -> col -> posidet -> filters in one context fed RAW8, against a context fed the model's BGR frames
(tests/debayer_ref.py) and against the oracle chain on those frames, on every entry path.  Every comparison is exact.
48 x 64 frames, a dozen frames of a moving saturated disc, mosaicked (debayer_ref.track_sequence; their non-vacuity is
asserted in tests/test_debayer_cpu.py)."""
import numpy as np
import pytest

import debayer_ref as D
import oracle_lib as O

pytestmark = pytest.mark.gpu

ROWS, COLS, T = D.TRACK_ROWS, D.TRACK_COLS, D.TRACK_T
HP_KW = dict(h_thresh=(D.HSV_WIN["h_lo"], D.HSV_WIN["h_hi"]), s_thresh=(D.HSV_WIN["s_lo"], D.HSV_WIN["s_hi"]),
             v_thresh=(D.HSV_WIN["v_lo"], D.HSV_WIN["v_hi"]), erode=D.DETECT["erode"], dilate=D.DETECT["dilate"],
             area=(D.DETECT["min_area"], D.DETECT["max_area"]))
_SEQ = {}


def _seq(seed, pattern):
    """(raw[T], model[T]) of one tracker sequence, computed once and left unchanged"""
    if (seed, pattern) not in _SEQ:
        _SEQ[(seed, pattern)] = D.track_sequence(seed, pattern)
    return _SEQ[(seed, pattern)]


def _sets(seqs, which):
    """[T][n] frame sets of several sequences (one a stream): which = 0 raw, 1 model"""
    return [[_seq(*sq)[which][t] for sq in seqs] for t in range(T)]


def _hp(n=1, bayer=None, **kw):
    import oat_amd
    args = dict(HP_KW)
    args.update(kw)
    hp = oat_amd.HotPath(ROWS, COLS, n_streams=n, adaptation_coeff=D.LR, **args)
    if bayer is not None:
        hp.bayer(bayer)
    return hp


def _pos(p):
    return tuple(vars(p).values())


def _same_model(a, b, tag):
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True), tag


def _same_model_oracle(gpu, ora, tag):
    nm_g, w_g, v_g, m_g, _ = gpu
    nm_o, w_o, v_o, m_o = ora
    assert (nm_g == nm_o).all(), tag
    live = np.arange(w_o.shape[1])[None, :] < nm_o[:, None]
    for g, o in ((w_g, w_o), (v_g, v_o), (m_g, m_o)):
        assert np.array_equal(g[live].view(np.uint32), o[live].view(np.uint32)), tag


def _taps(hp, n):
    from oat_amd import ffi
    return [[hp.read_mask(w, s) for w in (ffi.TAP_THRESHOLD, ffi.TAP_MORPH, ffi.TAP_FINAL)] for s in range(n)]


def _dev(fs):
    import torch
    d = torch.from_numpy(np.stack(fs)).cuda()
    torch.cuda.synchronize()
    return d


# ----------------------------------------------------------------- 1: RAW8 == the model's BGR frames == the oracle --

@pytest.mark.parametrize("seed,pattern", D.TRACK_SEQUENCES[:4])
def test_raw8_equals_bgr_frames_of_the_model_and_the_oracle(seed, pattern):
    raw, model = _seq(seed, pattern)
    a, b = _hp(bayer=D.NAMES[pattern]), _hp()
    orc, p = O.Mog2(ROWS, COLS, 3), O.hsv_params(**D.HSV_WIN, **D.DETECT)
    hits = 0
    try:
        for t in range(T):
            got, ref = a.track([raw[t]])[0], b.track([model[t]])[0]
            want, thr = O.chain_step(orc, model[t], D.LR, p)
            assert _pos(got) == _pos(ref), t
            for ga, gb in zip(_taps(a, 1)[0], _taps(b, 1)[0]):
                assert np.array_equal(ga, gb), t
            assert np.array_equal(a.read_mask(1, 0), thr), t
            assert got.position_valid == want["valid"], t
            if want["valid"]:
                hits += 1
                assert (got.a00, got.a10, got.a01) == (want["a00"], want["a10"], want["a01"]), t
        _same_model(a.mog_state(), b.mog_state(), pattern)
        _same_model_oracle(a.mog_state(), orc.state(), pattern)
    finally:
        a.close()
        b.close()
    assert hits * 2 >= T - 1, hits


# -------------------------------------------------------------------------------------------- 2: every entry path --

def _pinned(fs):
    import torch
    return [torch.from_numpy(f).pin_memory().numpy() for f in fs]


def _run_path(path, hp, frames):
    """positions of every frame set through one entry path"""
    res, keep = [], []
    if path == "batch":
        return [[_pos(p) for p in hp.track(fs)] for fs in frames]
    if path == "batch_dev":
        return [[_pos(p) for p in hp.track_dev(_dev(fs).data_ptr())] for fs in frames]
    if path == "sequence":
        keep = [_dev(fs) for fs in frames]
        return [[_pos(p) for p in fs] for fs in hp.track_sequence_dev([d.data_ptr() for d in keep])]
    if path == "enqueue_dev2":
        hp.set_fusion(2)
    if path == "staged_kernel":
        hp.set_stage_copy(1)
        frames = [_pinned(fs) for fs in frames]
    for fs in frames:
        if hp.outstanding() == 2:
            res.append([_pos(p) for p in hp.collect()])
        if path == "enqueue":
            hp.enqueue(fs)
        elif path == "enqueue_dev2":
            d = _dev(fs)
            hp.enqueue_dev(d.data_ptr(), keepalive=d)
        else:
            for s, f in enumerate(fs):
                hp.stage(s, f)
            hp.enqueue_staged()
    while hp.outstanding():
        res.append([_pos(p) for p in hp.collect()])
    return res


PATHS = ("batch", "batch_dev", "enqueue", "staged_dma", "staged_kernel", "enqueue_dev2", "sequence")


@pytest.mark.parametrize("n_frames", [T, T - 1])
def test_every_entry_path_gives_identical_results(n_frames):
    """track_batch, _batch_dev, enqueue / collect at ring depth 2, stage + enqueue_staged in both stage-copy modes, enqueue_dev
    after set_fusion(2), the sequence call -- with an even and an odd number of frames (two-frame steps, a lone remainder)"""
    seqs = D.TRACK_SEQUENCES[:2]
    pats = [D.NAMES[p] for _, p in seqs]
    raw, model = _sets(seqs, 0)[:n_frames], _sets(seqs, 1)[:n_frames]
    ref = _hp(2, ring_depth=2)
    try:
        want = _run_path("batch", ref, model)
        want_model = [ref.mog_state(s) for s in range(2)]
    finally:
        ref.close()
    assert sum(p[0] for fs in want for p in fs) >= n_frames - 1
    for path in PATHS:
        hp = _hp(2, bayer=pats, ring_depth=2)
        try:
            assert _run_path(path, hp, raw) == want, path
            for s in range(2):
                _same_model(hp.mog_state(s), want_model[s], (path, s))
        finally:
            hp.close()


# -------------------------------------------------------------------------------------- 3: a pattern per stream --

def test_two_streams_with_different_patterns():
    seqs = [D.TRACK_SEQUENCES[2], D.TRACK_SEQUENCES[1]]
    raw, model = _sets(seqs, 0), _sets(seqs, 1)
    a, b = _hp(2, bayer=[p for _, p in seqs]), _hp(2)
    wrong = _hp(2, bayer=[seqs[1][1], seqs[0][1]])
    orcs, p = [O.Mog2(ROWS, COLS, 3) for _ in seqs], O.hsv_params(**D.HSV_WIN, **D.DETECT)
    differs = False
    try:
        for t in range(T):
            got, ref = a.track(raw[t]), b.track(model[t])
            assert [_pos(x) for x in got] == [_pos(x) for x in ref], t
            differs = differs or [_pos(x) for x in wrong.track(raw[t])] != [_pos(x) for x in ref]
            for s in range(2):
                want, thr = O.chain_step(orcs[s], model[t][s], D.LR, p)
                assert np.array_equal(a.read_mask(1, s), thr), (t, s)
                assert got[s].position_valid == want["valid"], (t, s)
        for s in range(2):
            _same_model(a.mog_state(s), b.mog_state(s), s)
            _same_model_oracle(a.mog_state(s), orcs[s].state(), s)
    finally:
        a.close()
        b.close()
        wrong.close()
    assert differs, "the patterns swapped between the streams must show"


# ------------------------------------------------------------------------------------------- 4: undistort as well --

def test_with_undistort_on_the_remap_reads_the_demosaiced_frames():
    import undistort_ref as R
    seed, pattern = D.TRACK_SEQUENCES[0]
    raw, model = _seq(seed, pattern)
    K, Dc = R.cases(ROWS, COLS)["mild5"]
    m1, m2 = R.undistort_map(ROWS, COLS, K, Dc)
    hp = _hp(bayer=pattern, undistort=(K, Dc))
    orc, p = O.Mog2(ROWS, COLS, 3), O.hsv_params(**D.HSV_WIN, **D.DETECT)
    hits = 0
    try:
        for t in range(T):
            got = hp.track([raw[t]])[0] if t % 2 else hp.track_dev(_dev([raw[t]]).data_ptr())[0]
            want, thr = O.chain_step(orc, R.remap(model[t], m1, m2), D.LR, p)
            assert np.array_equal(hp.read_mask(1, 0), thr), t
            assert got.position_valid == want["valid"], t
            if want["valid"]:
                hits += 1
                assert (got.a00, got.a10, got.a01) == (want["a00"], want["a10"], want["a01"]), t
        _same_model_oracle(hp.mog_state(), orc.state(), "undistort")
    finally:
        hp.close()
    assert hits * 2 >= T - 1, hits


# ------------------------------------------------------------------------------- 5, 6: ROI; Kalman + homography --

def _pair_run(setup, n=1, seqs=None):
    """the same calls on a RAW8 context and on a BGR context fed the model's frames: positions, models and taps must agree"""
    seqs = seqs or D.TRACK_SEQUENCES[4:4 + n]
    raw, model = _sets(seqs, 0), _sets(seqs, 1)
    a, b = _hp(n, bayer=[p for _, p in seqs]), _hp(n)
    out = []
    try:
        for t in range(T):
            for hp in (a, b):
                setup(hp, t)
            got, ref = a.track(raw[t]), b.track(model[t])
            assert [_pos(x) for x in got] == [_pos(x) for x in ref], t
            for s in range(n):
                for ga, gb in zip(_taps(a, n)[s], _taps(b, n)[s]):
                    assert np.array_equal(ga, gb), (t, s)
            out.append(got)
        for s in range(n):
            _same_model(a.mog_state(s), b.mog_state(s), s)
    finally:
        a.close()
        b.close()
    return out


def test_a_roi_set_and_removed():
    yy, xx = np.mgrid[0:ROWS, 0:COLS]
    roi = ((xx < 40) & (yy > 4)).astype(np.uint8) * 255

    def setup(hp, t):
        if t == 2:
            hp.set_roi_mask(roi, stream=0)
        if t == 8:
            hp.set_roi_mask(None, stream=0)

    got = _pair_run(setup)
    assert sum(g[0].position_valid for g in got) >= 4


def test_kalman_and_homography_on():
    H = [0.5, 0.01, -3.0, -0.02, 0.6, -2.0, 1e-4, 2e-4, 1.0]

    def setup(hp, t):
        if t == 0:
            hp.set_kalman(True, dt=0.02, timeout=1.0, sigma_accel=5.0, sigma_noise=0.5)
            hp.set_homography(H)

    got = _pair_run(setup, n=2)
    assert sum(g[s].raw_valid for g in got for s in range(2)) >= T - 1
    assert any(g[s].velocity_valid for g in got for s in range(2))


# -------------------------------------------------------------------------------------------------- 7: marker sets --

MARKERS = [dict(h=(100, 125), s=(150, 256), v=(100, 256), erode=0, dilate=3, area=(10.0, 1e6)),
           dict(h=(90, 130), s=(100, 256), v=(50, 256), erode=3, dilate=0, area=(4.0, 1e6))]
OWN = dict(h_thresh=(0, 256), s_thresh=(0, 256), v_thresh=(1, 256))


def _marker_result(r):
    fg, mk, mean = r
    return ([_pos(p) for p in fg], [[_pos(p) for p in ms] for ms in mk], [tuple(vars(c).values()) for c in mean])


def _marker_hp(n, bayer):
    hp = _hp(n, bayer=bayer, ring_depth=2, **OWN)
    hp.set_markers(MARKERS, heading_anchor=0)
    return hp


def test_a_marker_set_of_two_synchronous_and_on_the_marker_pipeline():
    from oat_amd import ffi
    seqs = D.TRACK_SEQUENCES[2:4]
    pats = [p for _, p in seqs]
    raw, model = _sets(seqs, 0), _sets(seqs, 1)
    a, b = _marker_hp(2, pats), _marker_hp(2, None)
    try:
        want = []
        for t in range(T):                                   # synchronous: host frames and device frames in turn
            if t % 2:
                got, ref = a.track_markers(raw[t]), b.track_markers(model[t])
            else:
                got, ref = a.track_markers_dev(_dev(raw[t]).data_ptr()), b.track_markers_dev(_dev(model[t]).data_ptr())
            assert _marker_result(got) == _marker_result(ref), t
            for s in range(2):
                for m in range(2):
                    assert np.array_equal(a.read_marker_mask(m, ffi.TAP_MORPH, s), b.read_marker_mask(m, ffi.TAP_MORPH, s)), (t, s, m)
            want.append(_marker_result(ref))
        assert sum(mk[s][m][0] for _, mk, _ in want for s in range(2) for m in range(2)) >= 2 * (T - 1)
    finally:
        a.close()
        b.close()
    # the marker pipeline: enqueue (host frames) / collect_markers, then the sequence call on device frames
    a, b = _marker_hp(2, pats), _marker_hp(2, None)
    try:
        a.marker_pipeline(True)
        b.marker_pipeline(True)
        half = T // 2

        def piped(hp, frames):
            out = []
            for fs in frames[:half]:
                if hp.outstanding() == 2:
                    out.append(_marker_result(hp.collect_markers()))
                hp.enqueue(fs)
            while hp.outstanding():
                out.append(_marker_result(hp.collect_markers()))
            keep = [_dev(fs) for fs in frames[half:]]
            return out + [_marker_result(r) for r in hp.track_markers_sequence_dev([d.data_ptr() for d in keep])]

        got, ref = piped(a, raw), piped(b, model)
        assert got == ref
        assert ref == want, "the pipelined marker path against the synchronous one"
        for s in range(2):
            _same_model(a.mog_state(s), b.mog_state(s), s)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------- 8, 9, 10: resume; off paths --

def test_checkpoint_and_resume_continue_bit_identically(tmp_path):
    seqs = D.TRACK_SEQUENCES[:2]
    raw = _sets(seqs, 0)
    pats = [p for _, p in seqs]
    a, b = _hp(2, bayer=pats), _hp(2, bayer=pats)
    try:
        for fs in raw[:6]:
            a.track(fs)
        for s in range(2):
            a.save_mog_state(str(tmp_path / f"m{s}.mog"), stream=s)
            b.load_mog_state(str(tmp_path / f"m{s}.mog"), stream=s)
        for t, fs in enumerate(raw[6:]):
            assert [_pos(p) for p in a.track(fs)] == [_pos(p) for p in b.track(fs)], t
        for s in range(2):
            _same_model(a.mog_state(s), b.mog_state(s), s)
    finally:
        a.close()
        b.close()


def test_switch_off_after_on_equals_a_bgr_context_continuing_from_the_same_model():
    seed, pattern = D.TRACK_SEQUENCES[3]
    raw, model = _seq(seed, pattern)
    a, b = _hp(bayer=pattern), _hp()
    try:
        for t in range(6):
            a.track([raw[t]])
        b.set_mog_state(*a.mog_state())                      # a fresh BGR context continuing from the same model
        a.bayer(None)
        for t in range(6, T):
            fs = [model[t]]
            got = a.track(fs) if t % 2 else a.track_dev(_dev(fs).data_ptr())
            assert [_pos(p) for p in got] == [_pos(p) for p in b.track(fs)], t
        _same_model(a.mog_state(), b.mog_state(), "off")
        a.bayer(pattern)                                     # ... and on again
        assert a.frame_shape == (ROWS, COLS)
    finally:
        a.close()
        b.close()


def test_patterns_set_with_the_switch_off_change_nothing():
    seqs = D.TRACK_SEQUENCES[:2]
    model = _sets(seqs, 1)
    plain, toggled = _hp(2), _hp(2, bayer=["GBRG", "BGGR"])
    try:
        toggled.bayer(None)
        for t, fs in enumerate(model):
            assert [_pos(p) for p in toggled.track(fs)] == [_pos(p) for p in plain.track(fs)], t
        for s in range(2):
            _same_model(toggled.mog_state(s), plain.mog_state(s), s)
    finally:
        plain.close()
        toggled.close()


# ---------------------------------------------------------------------------------------------------- 11: refusals --

def test_refusals_and_the_input_consumed_rule():
    import ctypes as C
    import torch
    import oat_amd
    seqs = D.TRACK_SEQUENCES[:2]
    pats = [p for _, p in seqs]
    raw, model = _sets(seqs, 0), _sets(seqs, 1)

    def refused(fn, word):
        with pytest.raises(oat_amd.OatGpuError) as e:
            fn()
        assert e.value.code == -1 and word in str(e.value), str(e.value)

    grey = oat_amd.HotPath(ROWS, COLS, channels=1)
    try:
        refused(lambda: grey.bayer("RGGB"), "channels")
    finally:
        grey.close()
    tiny = oat_amd.HotPath(2, COLS)
    try:
        refused(lambda: tiny.bayer("RGGB"), "3 x 3")
    finally:
        tiny.close()
    hp = _hp(2, ring_depth=2)
    try:
        refused(lambda: hp.bayer(5), "pattern")
        refused(lambda: hp.bayer([1, 0]), "pattern")
        refused(lambda: hp.bayer([1, 2, 3]), "patterns")
        one = (C.c_int32 * 1)(1)
        assert hp.lib.oatgpu_set_track_bayer(hp.ctx, one, 0) == -1
        assert hp.lib.oatgpu_set_track_bayer(hp.ctx, None, 1) == -1
        hp.stage(0, model[0][0])                             # a partly staged set
        refused(lambda: hp.bayer(pats), "staged")
        hp.stage_abort()
        # nothing of the refused calls has stuck: the context still takes BGR frames
        ref = _hp(2)
        assert [_pos(p) for p in hp.track(model[0])] == [_pos(p) for p in ref.track(model[0])]
        ref.close()
        hp.bayer(pats)
        hp.stage(0, raw[1][0])
        refused(lambda: hp.bayer(None), "staged")
        hp.stage_abort()
    finally:
        hp.close()
    # the motion and subtraction trackers do not take Bayer frames
    for cls, call in ((oat_amd.MotionTracker, "oatgpu_diff_batch"), (oat_amd.SubtractionTracker, "oatgpu_bsub_track_batch")):
        tr = cls(ROWS, COLS)
        try:
            oat_amd.HotPath.bayer(tr, "RGGB")
            tr.frame_shape = (ROWS, COLS, 3)
            refused(lambda: tr.track([model[0][0]]), "oatgpu_set_track_bayer")
            oat_amd.HotPath.bayer(tr, None)
            tr.track([model[0][0]])
        finally:
            tr.close()
    # input_consumed (device frames): the caller's buffer is free once it returns -- overwritten then, the results are
    # those of the untouched frames
    ref = _hp(2)
    want = [[_pos(p) for p in ref.track(fs)] for fs in model]
    ref.close()
    hp = _hp(2, bayer=pats, ring_depth=2)
    try:
        hp.set_fusion(2)
        got = []
        for fs in raw:
            d = _dev(fs)
            hp.enqueue_dev(d.data_ptr())
            hp.input_consumed()
            d.zero_()
            torch.cuda.synchronize()
            got.append([_pos(p) for p in hp.collect()])
        assert got == want
    finally:
        hp.close()
