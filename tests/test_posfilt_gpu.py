"""The position filter stage on an MI355X: `posifilt kalman` on the device (k_kalman, kernels_kalman.hip) and `posifilt
homography` on the host (apply_homography), across the parameter rows, stream counts, launch orders and restarts of
tests/posfilt_cases.py (whose regimes tests/test_posfilt_cpu.py checks on the oracle alone).

The rule everywhere: flags equal, and x, y, vx, vy equal BIT FOR BIT to the oracle filter fed the oracle's detections,
on every sample, valid or not (a NaN of the oracle must be a NaN here; sign and payload of a NaN are not compared: an x86
division and the GPU's division expansion may differ there).  raw_valid / raw_x / raw_y and the integer sums must be the
oracle detection's on every sample -- the control without the filter.

Not reached: the `a00 <= 0` side of the centroid's sign select in k_kalman.  The blob stage reports outer contours, which
have one orientation, so no frame sent through the API produces it, and there is no debug entry point to force it.
"""
import dataclasses
import functools

import numpy as np
import pytest

import blob_load as B
import oracle_lib as O
import posfilt_cases as P
from test_blob_limits_gpu import AT_EDGE, DBL_MAX, LR as PAINT_LR, OVER, OVER2, WIN, _Painter
from test_gpu_parity import _same_state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    import oat_amd
    return oat_amd


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(present, marks, frames, Detections) of a set of posfilt_cases.SETS: computed once, shared, left unchanged."""
    present, marks, fr = P.build(name)
    return present, marks, fr, P.Detections(fr)


def _hotpath(A, rows, cols, n, ring):
    return A.HotPath(rows, cols, n_streams=n, ring_depth=ring, **P.HOTPATH)


def _sync(hp, fr):
    return [hp.track(list(f)) for f in fr]


def _host(hp, fr, ring):
    got = []
    for f in fr:
        if hp.outstanding() >= ring:
            got.append(hp.collect())
        hp.enqueue(list(f))
    while hp.outstanding():
        got.append(hp.collect())
    return got


def _dev(hp, fr, ring, after_enqueue=None):
    import torch
    bufs = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in fr]
    torch.cuda.synchronize()
    got = []
    for b in bufs:
        if hp.outstanding() >= ring:
            got.append(hp.collect())
        hp.enqueue_dev(b.data_ptr(), keepalive=b)
        if after_enqueue:
            after_enqueue()
    while hp.outstanding():
        got.append(hp.collect())
    return got


def _sequence(hp, fr):
    import torch
    bufs = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in fr]
    torch.cuda.synchronize()
    return hp.track_sequence_dev([b.data_ptr() for b in bufs])


def _same_raw(g, d, tag):
    assert g.raw_valid == d["valid"], (tag, g, d)
    assert (g.raw_x, g.raw_y, g.a00, g.a10, g.a01, g.area, g.first_pixel) == \
        (d["x"], d["y"], d["a00"], d["a10"], d["a01"], d["area"], d["first_pixel"]), (tag, g, d)


def _same_filtered(g, k, tag):
    assert (g.position_valid, g.velocity_valid) == (k["position_valid"], k["velocity_valid"]), (tag, g, k)
    for a, b in ((g.x, k["x"]), (g.y, k["y"]), (g.vx, k["vx"]), (g.vy, k["vy"])):
        assert P.same_bits(a, b), (tag, g, k)


def _same_run(got, det, want, tag):
    """Every sample of a run: the raw result against the detection, the filtered one against the oracle filter's."""
    assert len(got) == len(det) == len(want), tag
    for t, (gs, ds, ks) in enumerate(zip(got, det, want)):
        for s, (g, d, k) in enumerate(zip(gs, ds, ks)):
            _same_raw(g, d, (tag, t, s))
            _same_filtered(g, k, (tag, t, s))


def _unfiltered(ds):
    """What the library reports of detections with no filter behind them, in the filter's terms."""
    return [dict(position_valid=d["valid"], velocity_valid=False, x=d["x"], y=d["y"], vx=0.0, vy=0.0) for d in ds]


# ------------------------------------------------------------------------------------------ parameter matrix ---

@pytest.mark.parametrize("row", list(P.PARAMS))
def test_parameter_row_matches_the_oracle(A, row):
    """Three streams through one parameter row, rows alternating between the synchronous call and device frames enqueued
    behind a ring of 4, two frames a launch."""
    name = f"matrix_{row}"
    _, n, rows, cols, _, _ = P.SETS[name]
    present, marks, fr, D = _reference(name)
    want = P.filtered(D.det, row)
    hp = _hotpath(A, rows, cols, n, 4)
    hp.set_kalman(True, **P.kw(row))
    if list(P.PARAMS).index(row) % 2:
        hp.set_fusion(2)
        got = _dev(hp, fr, 4)
    else:
        got = _sync(hp, fr)
    _same_run(got, D.det, want, row)
    for s in range(n):
        _same_state(hp.mog_state(s), D.orc[s].state(), (row, s))
    valid = [[g[s].position_valid for g in got] for s in range(n)]
    thr = P.threshold(row)
    if thr == 0:
        assert not any(map(any, valid))
        assert all((q.x, q.y, q.vx, q.vy) == (6.0,) * 4 for g in got for q in g)
    else:
        assert min(map(sum, valid)) >= 20
    if row == "both0":
        assert sum(np.isnan(q.x) and np.isnan(q.vy) for g in got for q in g) >= 150
    # the drops and re-initialisations, frame by frame: the sample before a gap, the gap, the blob's return
    if row == "thr1":
        for s in range(n):
            a, b = marks[s]["exact"]                # one frame without a blob: dropped on it, found again behind it
            assert b - a == 1 and valid[s][a - 1:b + 1] == [True, False, True], (s, valid[s])
            a, b = marks[s]["long"]                 # three frames
            assert b - a == 3 and valid[s][a - 1:b + 1] == [True, False, False, False, True], (s, valid[s])
    if row in ("below_3", "below_3b"):              # threshold 2, not 3
        for s in range(n):
            a, b = marks[s]["short"]                # one frame: coasts on the stale measurement
            assert b - a == 1 and valid[s][a - 1:b + 1] == [True, True, True], (s, valid[s])
            a, b = marks[s]["exact"]                # two: coasts one, drops on the second
            assert b - a == 2 and valid[s][a - 1:b + 1] == [True, True, False, True], (s, valid[s])
            a, b = marks[s]["long"]                 # four
            assert b - a == 4 and valid[s][a - 1:b + 1] == [True, True, False, False, False, True], (s, valid[s])
    hp.close()


# ------------------------------------------------------------- more streams than a workgroup of k_kalman has lanes ---

@pytest.mark.parametrize("frames_on", ["host", "device"])
@pytest.mark.parametrize("row", ["base", "thr1"])
def test_65_streams_two_workgroups_of_the_filter(A, row, frames_on):
    """n_streams = 65: one full wave whose lanes diverge on every frame, and the lone lane of a second workgroup, which
    gets the script with the most changes of state.  Host frames behind a ring of 3; device frames behind a ring of 4, two
    frames a launch.  The models of the first stream, the last lane of the first workgroup and the lane of the second are
    compared at the end."""
    name = f"many_{row}"
    _, n, rows, cols, _, _ = P.SETS[name]
    present, marks, fr, D = _reference(name)
    want = P.filtered(D.det, row)
    ring = 3 if frames_on == "host" else 4
    hp = _hotpath(A, rows, cols, n, ring)
    hp.set_kalman(True, **P.kw(row))
    if frames_on == "host":
        got = _host(hp, fr, ring)
    else:
        hp.set_fusion(2)
        got = _dev(hp, fr, ring)
    _same_run(got, D.det, want, (row, frames_on))
    assert min(sum(g[s].position_valid for g in got) for s in range(n)) >= 20
    for s in (0, 63, 64):
        _same_state(hp.mog_state(s), D.orc[s].state(), (row, frames_on, s))
    hp.close()


# ------------------------------------------------------------------------------------------------- restarts ---

def test_restarts_into_tracking_filters(A):
    """One context: base -> thr1 -> off -> below_3 -> thr0 -> base, the four ways of handing frames over in turn.  After
    every set_kalman(True, ...) the oracle filters are new ones: the first report is 6.0 until the first measurement,
    nothing of the filter before shows through -- the error covariance, which a re-initialisation inside a run leaves
    alone, is zero again.  While off, the results are the raw ones.  A refused set_kalman (results outstanding, bad
    arguments) leaves the running filter as it was."""
    n, rows, cols, ring = 3, 48, 96, 4
    segs = P.restart_segments(n)
    hp = _hotpath(A, rows, cols, n, ring)
    hp.set_fusion(2)
    orc = [O.Mog2(rows, cols, 3) for _ in range(n)]
    p = O.hsv_params(**P.ORACLE)
    runs = [_sync, lambda h, f: _host(h, f, ring), lambda h, f: _dev(h, f, ring), _sequence]
    bad = [dict(dt=0.0), dict(timeout=-1.0), dict(dt=float("nan")), dict(timeout=float("nan")), dict(sigma_accel=-1.0),
           dict(sigma_noise=float("nan")), dict(dt=1e-9, timeout=3.0), dict(dt=1e-3, timeout=2.0 ** 31 * 1e-3)]
    tracked_at_restart = 0
    for i, (row, thr, present) in enumerate(segs):
        fr = P.frames(present, rows, cols, t0=i * P.SEGMENT_FRAMES)
        det = [[O.chain_step(orc[s], f[s], P.LR, p)[0] for s in range(n)] for f in fr]
        if i and segs[i - 1][0]:
            tracked_at_restart += sum(q.position_valid for q in last)
        if row is None:
            hp.set_kalman(False)
            want = [_unfiltered(ds) for ds in det]
        else:
            hp.set_kalman(True, **P.kw(row))
            want = P.filtered(det, row)
        # in two steps, with the refusals between them: the filter goes on where it was
        cut = P.SEGMENT_FRAMES // 2 + i % 3
        got = runs[i % 4](hp, fr[:cut])
        hp.enqueue(list(fr[cut]))
        with pytest.raises(A.OatGpuError, match="outstanding"):
            hp.set_kalman(True, **P.kw("base"))
        with pytest.raises(A.OatGpuError, match="outstanding"):
            hp.set_kalman(False)
        got.append(hp.collect())
        if row is not None:
            for kw in bad:
                with pytest.raises(A.OatGpuError):
                    hp.set_kalman(True, **{**P.kw(row), **kw})
        got += runs[(i + 1) % 4](hp, fr[cut + 1:])
        _same_run(got, det, want, (i, row))
        # the first report of the segment: a fresh filter's 6.0 (every script begins without a blob), invalid
        if row is not None:
            assert all((q.x, q.y, q.vx, q.vy) == (6.0,) * 4 and not q.position_valid for q in got[0]), (i, row)
            if thr:
                assert min(sum(g[s].position_valid for g in got) for s in range(n)) >= 4, (i, row)
        else:
            assert all(not q.velocity_valid and (q.x, q.y) == (q.raw_x, q.raw_y) and q.position_valid == q.raw_valid
                       for g in got for q in g)
        last = got[-1]
    assert tracked_at_restart >= 4           # restarts happened into filters that were tracking
    for s in range(n):
        _same_state(hp.mog_state(s), orc[s].state(), s)
    hp.close()


# ------------------------------------------------------------------------------- the filter behind both blob paths ---

def _raw_view(q):
    """The detector's own result of a filtered Position2D, in the fields _same_detection reads."""
    return dataclasses.replace(q, position_valid=q.raw_valid, x=q.raw_x, y=q.raw_y)


@pytest.mark.parametrize("fusion", [1, 2])
def test_filter_behind_the_lds_kernel_and_the_global_kernels(A, fusion):
    """Frames at the LDS blob kernel's capacity and one over it, with the filter on.  The context first earns
    speculation with the filter off (a warm-up and 18 steps that the LDS kernel takes).  A speculative record of a
    declined frame carries valid == -2, which the filter would take for a detection: with the filter on every step has
    to run the full launch sequence, and the record that the global kernels write must reach the filter as the oracle's
    detection.  _Painter.check asserts the path each frame takes (blob_load) and the raw result."""
    rows, cols, n, ring = B.PIPELINE_SHAPES[0][0], B.PIPELINE_SHAPES[0][1], 3, 4
    pt = _Painter(rows, cols, n, 90 + fusion)
    hp = A.HotPath(rows, cols, n_streams=n, ring_depth=ring, adaptation_coeff=PAINT_LR, erode=0, dilate=0,
                   area=(0.0, DBL_MAX), **WIN)
    hp.set_fusion(fusion)
    seq = [("empty",) * 3] + [AT_EDGE] * 18
    fr = [pt.frames(k) for k in seq]
    got = _dev(hp, fr, ring)
    for t, (f, kinds) in enumerate(zip(fr, seq)):
        pt.check(got[t], f, kinds, ("off", fusion, t))
    assert sum(pt.masks[k][1]["path"] == "lds" for kinds in seq[1:] for k in kinds) == 18 * 3

    hp.set_kalman(True, **P.kw("base"))
    kal = [O.Kalman(**P.kw("base")) for _ in range(n)]
    seq = [(AT_EDGE, OVER, OVER2)[t % 3] for t in range(16)]
    fr = [pt.frames(k) for k in seq]
    early = []
    got = _dev(hp, fr, ring, after_enqueue=lambda: early.append(hp.last_step_shape()[1]))
    assert early == [False] * len(seq)
    tracked = declined = 0
    for t, (f, kinds) in enumerate(zip(fr, seq)):
        raw = [_raw_view(q) for q in got[t]]
        pt.check(raw, f, kinds, ("on", fusion, t))           # raw == the oracle's detection, bit for bit, from here on
        for s in range(n):
            k = kal[s].filter(raw[s].position_valid, raw[s].x, raw[s].y)
            _same_filtered(got[t][s], k, ("on", fusion, t, s, kinds[s]))
            tracked += k["position_valid"]
            declined += pt.masks[kinds[s]][1]["path"] == "global"
    assert tracked >= 30 and declined >= 10
    for s in range(n):
        _same_state(hp.mog_state(s), pt.orc[s].state(), s)
    hp.close()


# ----------------------------------------------------------------------------------------------- homography ---

def _homography_run(A, H, name, row):
    """Two streams behind a ring of 4, the homography H behind the detector (row None) or the filter of `row`; for the
    last four frames the homography is off again: plain output, the filter going on where it was (its state never saw
    the matrix).  -> (results, the oracle's plain results, what was expected) of the frames under the homography."""
    _, n, rows, cols, _, _ = P.SETS[name]
    _, _, fr, D = _reference(name)
    cut = len(fr) - 4
    hp = _hotpath(A, rows, cols, n, 4)
    if row:
        hp.set_kalman(True, **P.kw(row))
    hp.set_homography(H)
    got = _host(hp, fr[:cut], 4)
    hp.enqueue(list(fr[cut]))
    with pytest.raises(A.OatGpuError, match="outstanding"):
        hp.set_homography(None)
    got.append(hp.collect())
    hp.set_homography(None)
    got += _host(hp, fr[cut + 1:], 4)
    plain = P.filtered(D.det, row) if row else [_unfiltered(ds) for ds in D.det]
    want = [[P.homography_of(H, k) for k in ks] for ks in plain[:cut + 1]] + plain[cut + 1:]
    _same_run(got, D.det, want, (name, row))                  # (raw_x / raw_y stay pixels)
    for s in range(n):
        _same_state(hp.mog_state(s), D.orc[s].state(), (name, row, s))
    hp.close()
    return got[:cut + 1], plain[:cut + 1], want[:cut + 1]


@pytest.mark.parametrize("kalman", [False, True])
@pytest.mark.parametrize("hname", list(P.HOMOGRAPHIES))
def test_homography_matrix_behind_detector_and_filter(A, hname, kalman):
    """Every sample against O.homography of the oracle's (valid, x, y, velocity_valid, vx, vy) -- the invalid ones too:
    they carry the zeros of an empty detection, the 6.0 of a filter that never tracked or its stale state through
    untouched."""
    H = P.HOMOGRAPHIES[hname]
    got, plain, want = _homography_run(A, H, "homography_base", "base" if kalman else None)
    flat = [(k, w) for ks, ws in zip(plain, want) for k, w in zip(ks, ws)]
    valid = sum(k["position_valid"] for k, _ in flat)
    assert valid >= 30 and len(flat) - valid >= 5
    for k, w in flat:
        if not k["position_valid"]:
            assert (w["x"], w["y"], w["vx"], w["vy"]) == (k["x"], k["y"], k["vx"], k["vy"])
    moved = sum((w["x"], w["y"]) != (k["x"], k["y"]) for k, w in flat if k["position_valid"])
    zeroed = sum((w["x"], w["y"]) == (0.0, 0.0) for k, w in flat if k["position_valid"])
    if hname == "identity":
        assert moved == 0
    elif hname in ("w_eq_eps", "zero_row"):
        assert zeroed == valid
    else:
        assert moved == valid and zeroed <= (2 if hname == "vel_w" else 0)
    if kalman:
        assert sum(k["position_valid"] and (k["vx"], k["vy"]) != (0.0, 0.0) for k, _ in flat) >= 30
        assert any(not k["position_valid"] and k["x"] == 6.0 for k, _ in flat)              # never tracked yet
        assert any(not k["position_valid"] and k["x"] != 6.0 for k, _ in flat)              # dropped: the stale state
        if hname == "vel_w":        # the velocity's own w: 0 while the filter is at rest, its result (0, 0) then
            assert any(k["velocity_valid"] and (k["vx"], k["vy"]) == (0.0, 0.0) for k, _ in flat)
            assert any(k["velocity_valid"] and w["vx"] != 0.0 for k, w in flat)


def test_nan_position_through_a_homography_is_zero(A):
    """Row both0 (NaN from the second tracked sample on) behind the projective matrix: fabs(NaN) > FLT_EPSILON is false,
    the result is (0, 0) -- position and velocity -- and still flagged valid."""
    got, plain, _ = _homography_run(A, P.HOMOGRAPHIES["projective"], "homography_both0", "both0")
    nans = [(q, k) for g, ks in zip(got, plain) for q, k in zip(g, ks) if k["position_valid"] and np.isnan(k["x"])]
    assert len(nans) >= 40
    assert all((q.x, q.y, q.vx, q.vy) == (0.0,) * 4 and q.position_valid and q.velocity_valid for q, _ in nans)
