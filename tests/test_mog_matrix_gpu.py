"""Every instantiation of the per-pixel MOG2 kernel, reached on purpose (tests/mog_matrix.py), against the C oracle: one
test id per instantiation on the pipelined track path, cases that cross instantiations, and OpenCV's parameters off their
defaults on the fused path.  Every frame's detection, the threshold bits of every stream at checkpoints and the whole
model at the end must be the oracle's, bit for bit; what the library reports of its choices (workgroup, frames a step,
audited launches) must be what the restated launcher says."""
import numpy as np
import pytest

import mog_matrix as M
import oracle_lib as O
from test_gpu_parity import _same_detection, _same_state

pytestmark = pytest.mark.gpu

RING = 4
N_STREAMS = 2
AREA = (4.0, 1e6)


@pytest.fixture(scope="module")
def A():
    import oat_amd
    return oat_amd


def _windows(ch, which):
    """(HotPath keywords, oracle hsv_params keywords) of a window: 'default' brackets the disc, 'black' holds black but not
    the shadows' colours, 'shadow' holds the shadows' colours but not black."""
    if ch == 3:
        h, s, v = dict(default=((100, 125), (150, 256), (100, 256)), black=((0, 256), (0, 256), (0, 40)),
                       shadow=((0, 256), (0, 256), (60, 256)))[which]
        return (dict(h_thresh=h, s_thresh=s, v_thresh=v),
                dict(h_lo=h[0], h_hi=h[1], s_lo=s[0], s_hi=s[1], v_lo=v[0], v_hi=v[1]))
    h = dict(default=(55, 75), black=(0, 40), shadow=(60, 256))[which]
    return dict(h_thresh=h), dict(h_lo=h[0], h_hi=h[1])


def _context(A, rows, cols, ch, n=N_STREAMS, window="default", over=None):
    hk, ok = _windows(ch, window)
    hp = A.HotPath(rows, cols, n_streams=n, ring_depth=RING, channels=ch, erode=0, dilate=0, area=AREA, **hk,
                   **(over or {}))
    p = O.hsv_params(erode=0, dilate=0, min_area=AREA[0], max_area=AREA[1], **ok)
    return hp, p


def _drive(hp, frames, rates, checkpoints=(), on_enqueue=None):
    """Enqueue frame set t with learning rate rates(t) or rates[t]; collect behind a ring of RING; drain at the
    checkpoints (where no frame is held back for pairing) and read every stream's threshold bits there.
    -> (positions a frame, {t: [threshold mask a stream]}, rates used, workgroup reported after each enqueue)."""
    got, thr, used, shapes, order = {}, {}, [], [], []
    for t, fs in enumerate(frames):
        lr = rates(t) if callable(rates) else rates[t]
        used.append(lr)
        hp.learning_coeff_ = lr
        hp.enqueue(list(fs))
        order.append(t)
        wg, early = hp.last_step_shape()
        assert not early, t
        shapes.append(wg)
        if on_enqueue:
            on_enqueue(t, wg)
        if t in checkpoints:
            while hp.outstanding():
                got[order.pop(0)] = hp.collect()
            thr[t] = [hp.read_mask(A_TAP, s) for s in range(hp.n_streams)]
        elif hp.outstanding() >= RING:
            got[order.pop(0)] = hp.collect()
    while hp.outstanding():
        got[order.pop(0)] = hp.collect()
    return [got[t] for t in range(len(frames))], thr, used, shapes


A_TAP = 0          # oatgpu TAP_THRESHOLD: the threshold bits of the frame collected last


def _against_oracle(hp, frames, res, p, over=None, tag=""):
    got, thr, used, _ = res
    n, ch = hp.n_streams, hp.channels
    orcs = [O.Mog2(hp.rows, hp.cols, ch, params=M.oracle_params(over or {})) for _ in range(n)]
    for t, fs in enumerate(frames):
        for s in range(n):
            want, th = O.chain_step(orcs[s], fs[s], used[t], p)
            _same_detection(got[t][s], want, (tag, t, s))
            if t in thr:
                assert (thr[t][s] == th).all(), (tag, "threshold", t, s, int((thr[t][s] != th).sum()))
    for s in range(n):
        _same_state(hp.mog_state(s), orcs[s].state(), (tag, "model", s))
    return orcs


def _checkpoints(nframes, fusion):
    """Frames behind which nothing is held back for pairing: odd t under fusion 2 (frame 0 is registered, 1 launches both)."""
    return {t for t in (9, 21, nframes - 3) if fusion == 1 or t % 2 == 1}


# ----------------------------------------------------------------------------------------- A: the 27 scenarios ---

@pytest.mark.parametrize("sc", M.SCENARIOS, ids=[sc.id for sc in M.SCENARIOS])
def test_instantiation_scenario(A, sc):
    rows, cols = sc.shape
    ch = sc.channels
    frames = M.frames_of(sc.data, N_STREAMS, rows, cols, ch, sc.nframes, seed=sum(sc.inst))
    hp, p = _context(A, rows, cols, ch)
    hp.set_fusion(sc.fusion)
    hp.set_k1_workgroup(sc.wg_force)
    hp.profile(1)
    if sc.audit:
        hp.traffic_audit(True)
    switched = []

    def on_enqueue(t, wg):
        if sc.data == "dense" and wg == 64 and not switched:
            switched.append(t)
            if sc.wg_after_switch:
                hp.set_k1_workgroup(sc.wg_after_switch)
    res = _drive(hp, frames, sc.rate, _checkpoints(sc.nframes, sc.fusion), on_enqueue)
    prof = hp.profile_read()
    launches = hp.traffic_read()["launches"] if sc.audit else None
    _against_oracle(hp, frames, res, p, tag=sc.id)
    shapes = res[3]
    # what the restated launcher says the run does (density from the frame after which this run switched)
    sw = switched[0] if switched else None
    steps = M.plan(ch, sc.fusion, [sc.rate(t) for t in range(sc.nframes)],
                   lambda t: sw is not None and t >= 5, audit=sc.audit, wg_force=sc.wg_force,
                   wg_after_switch=sc.wg_after_switch)
    # frames a step: what the fusion asks for (a step the profile took for a host stall is one it does not count)
    assert prof["steps"] + prof["dropped"] == len(steps), (sc.id, prof, len(steps))
    assert sc.nframes - 2 * prof["dropped"] <= prof["mog_frames"] <= sc.nframes, (sc.id, prof)
    if sc.audit:
        assert launches == sum(len(s.launches) for s in steps), (sc.id, launches)
        if ch == 1:
            assert launches == sc.nframes                  # GREY under the audit: one frame a launch, fusion 2 or not
    if sc.data == "dense":
        # the switch comes from a density probe: not before the decision at frame 16 (which reads the probe of frame 8),
        # not after the one at frame 32; it holds from then on (forced to 256 afterwards where the row asks for it)
        assert sw is not None and 16 <= sw <= 33, (sc.id, shapes)
        k = sw
        assert set(shapes[:k]) <= {0, 256}, (sc.id, shapes)
        after = shapes[k + 2:]
        assert set(after) == {sc.wg_after_switch or 64}, (sc.id, shapes)
    else:
        # no density switch on sparse data: the workgroup is the forced one or the path's 256 on every step
        assert set(shapes[1 if sc.fusion == 2 else 0:]) == {sc.wg_force or 256}, (sc.id, shapes)
        assert shapes == M.shapes_after_enqueue(steps, sc.nframes), (sc.id, shapes)
    assert sc.inst in [i for s in steps for i in s.launches], sc.id
    hp.close()


# ------------------------------------------------------------------------------ B: cases across instantiations ---

def _until_dense(hp, frames, rate_after, fusion):
    """Rates: 0.02 until the library has switched to the streaming loads (seen as the 64-thread workgroup), then rate_after."""
    state = {"sw": None}

    def rate(t):
        return M.WARM_RATE if state["sw"] is None else rate_after

    def on_enqueue(t, wg):
        if wg == 64 and state["sw"] is None and (fusion == 1 or t % 2 == 1):
            state["sw"] = t
    res = _drive(hp, frames, rate, _checkpoints(len(frames), fusion), on_enqueue)
    assert state["sw"] is not None and state["sw"] <= 33, res[3]
    return res, state["sw"]


@pytest.mark.parametrize("ch", [3, 1])
def test_dense_model_at_rate_zero_on_the_streaming_load_kernel(A, ch):
    """A dense model at rate 0 keeps the streaming loads (the frozen kernels are for plain models): compared with the
    oracle -- renormalisation can move weight bits even at rate 0, so no claim that the model stays as it was."""
    rows, cols, nframes = 40, 101, 44
    frames = M.dense_frames(N_STREAMS, rows, cols, ch, nframes, seed=5)
    hp, p = _context(A, rows, cols, ch)
    hp.set_fusion(2)
    res, sw = _until_dense(hp, frames, 0.0, 2)
    assert res[2].count(0.0) >= 8
    assert set(res[3][sw:]) == {64}
    _against_oracle(hp, frames, res, p, tag=("dense-rate0", ch))
    hp.close()


@pytest.mark.parametrize("mode", ["plain", "streaming"])
@pytest.mark.parametrize("ch", [3, 1])
def test_rate_one_is_never_paired(A, ch, mode):
    """Rate 1.0 re-initialises every frame: fusion 2 still sends every frame alone (fresh), on a plain context and on one
    that has switched to the streaming loads."""
    rows, cols, nframes = 40, 101, 40
    hp, p = _context(A, rows, cols, ch)
    hp.set_fusion(2)
    hp.profile(1)
    if mode == "plain":
        frames = M.sparse_frames(N_STREAMS, rows, cols, ch, nframes, seed=3)
        res = _drive(hp, frames, [1.0] * nframes, _checkpoints(nframes, 2))
        steps = M.plan(ch, 2, [1.0] * nframes, lambda t: False)
    else:
        frames = M.dense_frames(N_STREAMS, rows, cols, ch, nframes, seed=3)
        res, sw = _until_dense(hp, frames, 1.0, 2)
        assert res[2].count(1.0) >= 6
        steps = M.plan(ch, 2, res[2], lambda t: t < sw + 1 and t >= 5)
    assert all(len(s.launches) == len(s.frames) for s in steps if 1.0 in [res[2][t] for t in s.frames])
    prof = hp.profile_read()
    assert prof["steps"] + prof["dropped"] == len(steps), prof
    _against_oracle(hp, frames, res, p, tag=("rate1", mode, ch))
    hp.close()


@pytest.mark.parametrize("ch", [3, 1])
def test_dense_model_with_shrinking_mode_count(A, ch):
    """mog_restore_nmodes = 0 (pruning shrinks the count) on a dense model: the streaming-load kernels, both fusions."""
    rows, cols, nframes = 48, 128, 40
    frames = M.dense_frames(N_STREAMS, rows, cols, ch, nframes, seed=8)
    for fusion in (1, 2):
        hp, p = _context(A, rows, cols, ch, over=dict(mog_restore_nmodes=0))
        hp.set_fusion(fusion)
        res, _ = _until_dense(hp, frames, M.WARM_RATE, fusion)
        _against_oracle(hp, frames, res, p, over=dict(mog_restore_nmodes=0), tag=("dense-shrink", ch, fusion))
        hp.close()


@pytest.mark.parametrize("ch", [3, 1])
def test_dense_and_sparse_stream_in_one_context(A, ch):
    """One dense and one sparse stream: the mean over both crosses the switch, and both streams run the streaming loads."""
    rows, cols, nframes = 40, 101, 40
    d = M.dense_frames(1, rows, cols, ch, nframes, seed=11)
    s = M.sparse_frames(1, rows, cols, ch, nframes, seed=11)
    frames = [[d[t][0], s[t][0]] for t in range(nframes)]
    hp, p = _context(A, rows, cols, ch)
    hp.set_fusion(2)
    res, _ = _until_dense(hp, frames, M.WARM_RATE, 2)
    _against_oracle(hp, frames, res, p, tag=("dense+sparse", ch))
    hp.close()


@pytest.mark.parametrize("ch", [3, 1])
def test_uneven_histories_at_the_automatic_rate(A, ch):
    """Streams at different frame counts at rate -1 have different rates: the launches of a step are split by stream
    group, and groups start at first_stream > 0 -- on a plain model and on a dense one."""
    rows, cols, n, nframes = 40, 101, 3, 40
    for kind in ("sparse", "dense"):
        frames = M.frames_of(kind, n, rows, cols, ch, nframes + 3, seed=13)
        hp, p = _context(A, rows, cols, ch, n=n)
        hp.set_fusion(2)
        orcs = [O.Mog2(rows, cols, ch) for _ in range(n)]
        lib = A.ffi.load()
        for t in range(3):                     # stream 2 three frames ahead, stream 1 one, through the single-stage entry
            for sidx in ((2, 1) if t == 0 else (2,)):
                f = frames[t][sidx]
                out = np.empty_like(f)
                hp._chk(lib.oatgpu_mog_filter(hp.ctx, sidx, A.ffi.u8(f), A.ffi.u8(out), -1.0))
                want, _ = orcs[sidx].filter(f, -1.0)
                assert (out == want).all()
        seq = frames[3:]
        res = _drive(hp, seq, [-1.0] * nframes, _checkpoints(nframes, 2))
        got, thr, _, shapes = res
        for t, fs in enumerate(seq):
            for sidx in range(n):
                want, th = O.chain_step(orcs[sidx], fs[sidx], -1.0, p)
                _same_detection(got[t][sidx], want, (kind, t, sidx))
                if t in thr:
                    assert (thr[t][sidx] == th).all(), (kind, t, sidx)
        for sidx in range(n):
            _same_state(hp.mog_state(sidx), orcs[sidx].state(), (kind, sidx))
        if kind == "dense":
            assert 64 in shapes, shapes
        hp.close()


# ------------------------------------------------------------------------------ C: the parameter grid, fused ---

GRID_FRAMES = 30
GRID_SHAPE = (40, 101)


@pytest.mark.parametrize("fusion", [1, 2])
@pytest.mark.parametrize("ch", [3, 1])
@pytest.mark.parametrize("name", sorted(M.PARAM_GRID))
def test_parameter_grid_on_the_track_path(A, name, ch, fusion):
    over, sched, window, kind = M.PARAM_GRID[name]
    rows, cols = GRID_SHAPE
    frames = M.frames_of(kind, N_STREAMS, rows, cols, ch, GRID_FRAMES, seed=17)
    hp, p = _context(A, rows, cols, ch, window=window, over=over)
    hp.set_fusion(fusion)
    res = _drive(hp, frames, lambda t: M.grid_rate(sched, t), _checkpoints(GRID_FRAMES, fusion))
    assert set(res[3][1 if fusion == 2 else 0:]) == {256}, res[3]          # never dense: plain / frozen kernels only
    orcs = _against_oracle(hp, frames, res, p, over=over, tag=(name, ch, fusion))
    if "nmixtures" in over:
        assert orcs[0].state()[0].max() == over["nmixtures"]
    hp.close()


@pytest.mark.parametrize("ch", [3, 1])
@pytest.mark.parametrize("name", M.SHADOW_GRID)
def test_parameter_grid_mask_bytes(A, name, ch):
    """The cases about mask bytes through BackgroundSubtractorMOG.apply, the one path that returns them: {0, shadow, 255}."""
    over, sched, _, kind = M.PARAM_GRID[name]
    rows, cols = GRID_SHAPE
    frames = M.frames_of(kind, 1, rows, cols, ch, GRID_FRAMES, seed=19)
    g = A.BackgroundSubtractorMOG(rows, cols, channels=ch, **over)
    o = O.Mog2(rows, cols, ch, params=M.oracle_params(over))
    seen = set()
    for t, fs in enumerate(frames):
        lr = M.grid_rate(sched, t)
        mg, mo = g.apply(fs[0], learning_rate=lr), o.apply(fs[0], lr)
        assert (mg == mo).all(), (name, t, int((mg != mo).sum()))
        seen |= set(np.unique(mo).tolist())
    _same_state(g.mog_state(), o.state(), name)
    sv = over.get("shadow_value", 127)
    if over.get("detect_shadows", 1):
        assert sv in seen, (name, seen)
    else:
        assert seen <= {0, 255}
    g.close()
