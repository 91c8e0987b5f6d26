"""The position filter cases (tests/posfilt_cases.py) on the CPU: the parameter table is what it claims; every (row,
script) pair the GPU tests run produces the regime it is meant to on the C oracle, so that no GPU test passes emptily; the
C oracle of `posifilt kalman` against the numpy restatement (tests/golden/make_golden.py) off its usual parameters; the
C oracle of `posifilt homography` against a restatement on both sides of |w| > FLT_EPSILON.

Run with -s to see the regime counts of every pair."""
import functools
import importlib.util
import math
import os

import numpy as np
import pytest

import oracle_lib as O
import posfilt_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the table ---

@pytest.mark.parametrize("row", sorted(P.PARAMS))
def test_threshold_of_the_row_is_the_fp64_quotient_truncated(row):
    dt, timeout, _, _, thr = P.PARAMS[row]
    assert int(timeout / dt) == thr
    if row in P.BELOW:
        # a library that rounds the quotient, or divides in fp32, gets the next integer
        nxt = P.BELOW[row]
        assert nxt - 1 < timeout / dt < nxt and thr == nxt - 1
        assert round(timeout / dt) == nxt
        assert int(np.float32(timeout) / np.float32(dt)) == nxt


def test_the_rows_the_issue_names_are_there():
    assert len(P.PARAMS) == 11
    assert {P.threshold(r) for r in P.PARAMS} == {0, 1, 2, 8, 10, 50}
    assert P.PARAMS["noise0"][3] == 0 and P.PARAMS["accel0"][2] == 0 and P.PARAMS["both0"][2:4] == (0.0, 0.0)


# ---------------------------------------------------------------------------- the regimes, on the oracle alone ---

@functools.lru_cache(maxsize=None)
def _oracle(name):
    present, marks, fr = P.build(name)
    D = P.Detections(fr)
    return present, marks, D.det, P.filtered(D.det, P.SETS[name][0])


def _flags(det, out, s):
    return [d[s]["valid"] for d in det], [o[s]["position_valid"] for o in out]


def _wave_states(thr, row, lanes=64):
    """Lane states of one full wave of k_kalman on the row's scripts, frame by frame: the oracle filters fed the blobs'
    corners (the states depend on the flags alone)."""
    present, _ = P.scripts(lanes, thr)
    kal = [O.Kalman(**P.kw(row)) for _ in range(lanes)]
    found = [[kal[s].filter(present[s, t], *P.blob(s, t, 48, 96)[:2])["position_valid"] for t in range(present.shape[1])]
             for s in range(lanes)]
    st = [P.lane_states(list(present[s]), found[s]) for s in range(lanes)]
    return [{st[s][t] for s in range(lanes)} for t in range(present.shape[1])]


@pytest.mark.parametrize("name", sorted(P.SETS))
def test_every_pair_produces_its_regime_on_the_oracle(name):
    row, n, rows, cols, busy, length = P.SETS[name]
    thr = P.threshold(row)
    present, marks, det, out = _oracle(name)
    T = present.shape[1]
    regs = []
    for s in range(n):
        valid, found = _flags(det, out, s)
        assert valid == list(present[s]), (name, s)             # the detector sees the script, nothing else
        assert not valid[0], (name, s)                          # a leading stretch without a blob
        r = P.regime(valid, found)
        regs.append(r)
        # at least one measurement whose centroid is no dyadic rational: the division rounds
        assert any(d[s]["valid"] and not (P.dyadic(d[s]["a10"], 3 * d[s]["a00"]) and P.dyadic(d[s]["a01"], 3 * d[s]["a00"]))
                   for d in det), (name, s)
        # ... and one that is a half-integer (the rectangles)
        assert any(d[s]["valid"] and d[s]["x"] * 2 == int(d[s]["x"] * 2) for d in det), (name, s)
        if thr == 0:
            continue
        assert r["tracked"] >= 20, (name, s, r)
        assert r["drops"] >= 1 and r["reinits"] >= 1, (name, s, r)
        if not length:                                          # a whole round of the script: its three gaps
            a, b = marks[s]["long"]                             # longer than the threshold: dropped inside it
            assert found[a - 1] and not found[b - 1] and not found[b - 2] and found[b], (name, s)
            a, b = marks[s]["exact"]                            # exactly the threshold: drops on its last frame
            assert b - a == thr and found[a - 1:b + 1] == [True] * thr + [False, True], (name, s, found[a - 1:b + 1])
            if thr >= 2:
                a, b = marks[s]["short"]                        # one less: coasts through
                assert b - a == thr - 1 and all(found[a - 1:b + 1]), (name, s)
    print(f"\n{name}: row {row} threshold {thr}, {n} streams x {T} frames")
    for s in sorted({0, 1, n - 2, n - 1}):
        print(f"  stream {s}: {regs[s]}")
    if thr == 0:
        return
    # a frame where one wave holds every lane state: on the set itself where it fills a wave, else on the wave that the
    # row's scripts would fill.  (With threshold 1 the first miss drops: there is no coasting.)
    states = ([set(P.lane_states(*_flags(det, out, s))[t] for s in range(64)) for t in range(T)] if n >= 64
              else _wave_states(thr, row))
    want = {P.INIT, P.TRACK, P.DROPPED} | ({P.COAST} if thr >= 2 else set())
    hist = [sum(1 for st in states if len(st) == k) for k in range(5)]
    print(f"  frames by the number of lane states in wave 0: {dict(enumerate(hist))}")
    assert any(st == want for st in states), name
    if n >= 64:
        assert all(len(st) >= 2 for st in states[1:]), name     # the wave diverges on every frame but the first
        assert sum(len(st) == len(want) for st in states) * 2 > T, name
        # the lone lane of the second workgroup is on the script with the most changes of state
        assert busy == (64,) and regs[64]["changes"] > max(r["changes"] for r in regs[:64]), name


def test_threshold_0_never_tracks_and_reports_6():
    _, _, det, out = _oracle("matrix_thr0")
    assert sum(d["valid"] for ds in det for d in ds) >= 30
    for o in (o for os_ in out for o in os_):
        assert not o["position_valid"] and not o["velocity_valid"]
        assert (o["x"], o["y"], o["vx"], o["vy"]) == (6.0, 6.0, 6.0, 6.0)


@pytest.mark.parametrize("name", ["matrix_both0", "homography_both0"])
def test_both_sigmas_0_is_nan_from_the_second_tracked_sample_on(name):
    """Q = 0 and R = 0: H P' H^T + R is the zero matrix from the first prediction on (errorCovPost is still zero), the
    gain 0 / 0.  The first tracked sample reports the measurement; the corrected state is NaN, and so is every report
    after it -- but for the sample of a re-initialisation, whose predicted state is the new measurement again."""
    n = P.SETS[name][1]
    _, _, det, out = _oracle(name)
    for s in range(n):
        valid, found = _flags(det, out, s)
        st = P.lane_states(valid, found)
        first = st.index(P.INIT)
        for t, o in enumerate(o[s] for o in out):
            vals = (o["x"], o["y"], o["vx"], o["vy"])
            if t < first:
                assert vals == (6.0, 6.0, 6.0, 6.0), (s, t)
            elif st[t] == P.INIT:
                assert vals == (det[t][s]["x"], det[t][s]["y"], 0.0, 0.0), (s, t, vals)
            else:
                assert all(math.isnan(v) for v in vals), (s, t, vals)
        assert st[first + 1] in (P.TRACK, P.COAST) and st.count(P.INIT) >= 2, s


def test_sigma_accel_0_never_leaves_the_first_measurement():
    """Q = 0 over errorCovPost = 0: the predicted covariance is 0, the gain 0 -- for ever; a re-initialisation moves the
    state to the measurement it happens on and the filter stays there."""
    _, _, det, out = _oracle("matrix_accel0")
    moved = 0
    for s in range(3):
        valid, found = _flags(det, out, s)
        st = P.lane_states(valid, found)
        at = None
        for t, o in enumerate(o[s] for o in out):
            if st[t] == P.INIT:
                at = (det[t][s]["x"], det[t][s]["y"])
            if found[t]:
                assert (o["x"], o["y"], o["vx"], o["vy"]) == (at[0], at[1], 0.0, 0.0), (s, t)
                moved += valid[t] and (det[t][s]["x"], det[t][s]["y"]) != at
    assert moved >= 60                                          # ... while the measurements go elsewhere


def test_restart_segments_begin_without_a_blob_and_then_track():
    for i, (row, thr, present) in enumerate(P.restart_segments(3)):
        assert present.shape == (3, P.SEGMENT_FRAMES)
        assert not present[:, 0].any() and present.sum(axis=1).min() >= 5, (i, row)
        assert (~present[:, 1:]).sum(axis=1).min() >= 2, (i, row)


# ------------------------------------------------------------------ the oracle against the numpy restatement ---

def _make_golden():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(ROOT, "tests", "golden", "make_golden.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    return G


@pytest.mark.parametrize("row", sorted(set(P.PARAMS) - {"both0"}))
def test_oracle_against_the_numpy_restatement_off_the_usual_parameters(row):
    """oracle/kalman.c (2x2 system in closed form, sums in cv::gemm's order) against make_golden.kalman_trace (numpy
    matrix algebra, np.linalg.solve) on the measurements the GPU tests use: flags identical, values within the bound
    the project has for this pair, 1e-9 * max(1, |want|).  (both0: the 2x2 system is singular, np.linalg.solve
    raises.)"""
    G = _make_golden()
    _, _, det, out = _oracle(f"matrix_{row}")
    worst = 0.0
    for s, samples in enumerate(P.measurements(det)):
        ref = G.kalman_trace(samples, **P.kw(row))
        for t, w in enumerate(ref):
            g = out[t][s]
            assert g["position_valid"] == w[0] and g["velocity_valid"] == w[0], (row, s, t)
            for a, b in zip((g["x"], g["y"], g["vx"], g["vy"]), w[1:]):
                assert abs(a - b) <= 1e-9 * max(1.0, abs(b)), (row, s, t, a, b)
                worst = max(worst, abs(a - b) / max(1.0, abs(b)))
    print(f"\n{row}: worst relative difference {worst:.3g}")


# -------------------------------------------------------------------------------------------- homography ---

_FLT_EPSILON = 2.0 ** -23
_POS = [(0.0, 0.0), (6.0, 6.0), (10.5, 20.25), (47.0 + 1 / 3, 12.1), (-3.0, 7.0), (2.0, 1.0), (float("nan"), 5.0)]
_VEL = [(0.0, 0.0), (6.0, 6.0), (-120.5, 33.25), (2.0, 1.0), (1e-9, -1e-9), (float("nan"), 1.0)]


def _point(m, x, y):
    """cv::perspectiveTransform on one CV_64FC2 point, restated."""
    w = x * m[6] + y * m[7] + m[8]
    if not abs(w) > _FLT_EPSILON:
        return 0.0, 0.0
    return (x * m[0] + y * m[1] + m[2]) * (1.0 / w), (x * m[3] + y * m[4] + m[5]) * (1.0 / w)


@pytest.mark.parametrize("name", sorted(P.HOMOGRAPHIES))
def test_homography_oracle_against_its_restatement(name):
    h = [float(v) for v in P.HOMOGRAPHIES[name]]
    hv = h[:2] + [0.0] + h[3:5] + [0.0] + h[6:]
    seen = set()
    for (x, y) in _POS:
        for (vx, vy) in _VEL:
            for pv in (False, True):
                for vv in (False, True):
                    got = O.homography(h, pv, x, y, vv, vx, vy)
                    want = (_point(h, x, y) if pv else (x, y)) + (_point(hv, vx, vy) if vv else (vx, vy))
                    assert all(P.same_bits(a, b) for a, b in zip(got, want)), (name, x, y, vx, vy, pv, vv, got, want)
                    seen.add(("p", abs(x * h[6] + y * h[7] + h[8]) > _FLT_EPSILON))
                    seen.add(("v", abs(vx * h[6] + vy * h[7] + h[8]) > _FLT_EPSILON))
    # a NaN position: fabs(NaN) > eps is false
    assert O.homography(h, True, float("nan"), 5.0)[:2] == (0.0, 0.0)
    # both branches of every row that has two (the NaN samples take the second everywhere); these two rows have one
    only = {"w_eq_eps": {False}, "zero_row": {False}}.get(name, {True, False})
    assert {b for k, b in seen if k == "p"} == only and {b for k, b in seen if k == "v"} == only, (name, seen)
    if name == "vel_w":     # ... and without a NaN: w = 0 on the line x = 2 y and at rest
        assert O.homography(h, True, 2.0, 1.0, True, 0.0, 0.0) == (0.0, 0.0, 0.0, 0.0)
        assert 0.0 not in O.homography(h, True, 10.5, 20.25, True, -120.5, 33.25)


def test_the_boundary_rows_sit_on_both_sides_of_flt_epsilon():
    eps = float(np.finfo(np.float32).eps)
    assert eps == _FLT_EPSILON
    H = P.HOMOGRAPHIES
    assert H["w_eq_eps"][8] == eps and not abs(H["w_eq_eps"][8]) > eps
    assert H["w_above_eps"][8] == np.nextafter(eps, 1.0) > eps
    assert H["w_below_neg"][8] == -np.nextafter(eps, 1.0) and abs(H["w_below_neg"][8]) > eps
    assert O.homography(H["w_eq_eps"], True, 3.0, 4.0)[:2] == (0.0, 0.0)
    assert O.homography(H["w_above_eps"], True, 3.0, 4.0)[:2] != (0.0, 0.0)
    x, y = O.homography(H["w_below_neg"], True, 3.0, 4.0)[:2]
    xa, ya = O.homography(H["w_above_eps"], True, 3.0, 4.0)[:2]
    assert (x, y) == (-xa, -ya) and x != 0
    assert H["neg_w"][6:] == [0, 0, -1] and H["zero_row"][6:] == [0, 0, 0] and H["vel_w"][6:] == [1e-3, -2e-3, 0]
