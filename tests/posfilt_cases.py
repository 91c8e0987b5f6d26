"""The position filter stage off its one usual scenario (TEST INFRASTRUCTURE, no GPU imports): parameter rows of
`posifilt kalman`, measurement scripts that put every stream of a launch into another state of the filter, frames that
carry them through the detector, matrices of `posifilt homography`, and the oracle's answer to all of it.

tests/test_posfilt_cpu.py checks on the oracle alone that every (row, script) pair produces the regime it is meant to;
tests/test_posfilt_gpu.py compares the library with the oracle on them, every sample, bit for bit.
"""
import math
from fractions import Fraction

import numpy as np

import oracle_lib as O

# name -> (dt, timeout, sigma_accel, sigma_noise, threshold).  threshold = (int)(timeout / dt) in fp64
# (KalmanFilter2D.cpp:74-76), written out: the tests compare it, they do not compute it.  below_3 / below_3b: the
# quotient is 2.9999999999999996, a threshold rounded, or computed in fp32, would be 3.
PARAMS = {
    "base":       (0.01, 0.08, 30.0, 1.5, 8),
    "below_3":    (0.1, 0.3, 5.0, 1.0, 2),
    "below_3b":   (0.2, 0.6, 5.0, 1.0, 2),
    "thr1":       (0.02, 0.02, 5.0, 0.5, 1),
    "thr0":       (0.02, 0.019, 5.0, 0.5, 0),
    "noise0":     (0.02, 0.2, 5.0, 0.0, 10),
    "accel0":     (0.02, 0.2, 0.0, 2.0, 10),
    "both0":      (0.02, 0.2, 0.0, 0.0, 10),
    "big_dt":     (10.0, 100.0, 1e3, 1e-3, 10),
    "tiny_dt":    (1e-4, 1e-3, 1e-2, 50.0, 10),
    "huge_noise": (0.02, 1.0, 5.0, 1e8, 50),
}
BELOW = {"below_3": 3, "below_3b": 3}          # row -> the integer its quotient stays strictly below


def kw(row):
    """The keywords of HotPath.set_kalman / O.Kalman for a row."""
    dt, timeout, sa, sn, _ = PARAMS[row]
    return dict(dt=dt, timeout=timeout, sigma_accel=sa, sigma_noise=sn)


def threshold(row):
    return PARAMS[row][4]


# the detector of the existing Kalman test: a dark frame, one bright blob
HOTPATH = dict(adaptation_coeff=0.0, erode=0, dilate=3, v_thresh=(200, 256), area=(4.0, 1e6))
ORACLE = dict(v_lo=200, v_hi=256, erode=0, dilate=3, min_area=4.0, max_area=1e6)
LR = 0.0


# ------------------------------------------------------------------------------------------- measurement scripts ---

def script(s, thr, busy=False, length=0):
    """Presence of stream s's blob, frame by frame, against a filter of drop threshold thr.  Behind a leading stretch
    without a blob, one round holds: isolated single misses; a gap of thr + 2 frames (longer than the threshold: the
    filter drops inside it); a gap of exactly thr frames (drops on its last frame); a gap of thr - 1 frames (coasts
    through); runs of blob frames between them.  The round repeats until `length` frames are filled (at least one whole
    round).  Lead, run length and the gap a stream's round begins with depend on s: the gaps of neighbouring streams
    are staggered.
    busy: the shortest runs between the gaps -- the script with the most changes of state in a given length.
    -> (list of bool, {"long" / "exact" / "short": (first frame, one past the last frame) of that gap's first round})."""
    run = 2 if busy else 3 + s % 3
    pairs = [(run + 2, 1, None), (run, thr + 2, "long"), (run + 1, 1, None)]
    if thr >= 1:
        pairs.append((run, thr, "exact"))
    if thr >= 2:
        pairs.append((run + 2, thr - 1, "short"))
    pairs.append((run, 1, None))
    k = s % len(pairs)
    pairs = pairs[k:] + pairs[:k]
    p, marks = [False] * (1 + s % 7), {}
    while True:
        for on, off, name in pairs:
            p.extend([True] * on)
            if name and name not in marks:
                marks[name] = (len(p), len(p) + off)
            p.extend([False] * off)
        if len(p) >= length:
            return (p[:length] if length else p), marks


def scripts(n, thr, busy=(), length=0):
    """(present[n][T], marks[n]): script(s, thr) of every stream at one length: `length` frames exactly (a round may be
    cut short then), or two frames more than the longest stream's first round takes."""
    T = length or max(len(script(s, thr, s in busy)[0]) for s in range(n)) + 2
    ps, ms = zip(*[script(s, thr, s in busy, T) for s in range(n)])
    return np.array(ps, bool), list(ms)


def blob(s, t, rows, cols):
    """(y0, x0, h, w, cut_h, cut_w): the blob of stream s in frame t, clear of the image frame and of the dilation's
    reach.  Even t: a rectangle (cut 0 x 0; its centroid is a half-integer); odd t: an L -- the rectangle without its top
    right cut_h x cut_w block."""
    h, w = 4 + (s + t) % 3, 6 + (2 * s + t) % 4
    y0 = 2 + (2 * t + 5 * s) % (rows - h - 4)
    x0 = 2 + ((3 + s % 5) * t + 7 * s) % (cols - w - 4)
    cut = (1 + (s + t // 2) % 2, 2 + (s + t // 2) % 3) if t % 2 else (0, 0)
    return y0, x0, h, w, cut[0], cut[1]


def frames(present, rows, cols, t0=0):
    """uint8 [T][n][rows][cols][3]: black, the stream's blob of frame t0 + t in white where the script has one."""
    n, T = present.shape
    f = np.zeros((T, n, rows, cols, 3), np.uint8)
    for t in range(T):
        for s in range(n):
            if present[s, t]:
                y0, x0, h, w, ch, cw = blob(s, t0 + t, rows, cols)
                f[t, s, y0:y0 + h, x0:x0 + w] = 255
                if ch:
                    f[t, s, y0:y0 + ch, x0 + w - cw:x0 + w] = 0
    return f


# The (row, script) pairs the GPU tests run: name -> (row, streams, rows, cols, busy streams, frames (0: by the script)).
# The parameter matrix: three streams; more streams than a workgroup of k_kalman has lanes: 65, the lone lane of the
# second workgroup on the busy script; the homography runs: two streams, 40 frames.
SETS = {f"matrix_{row}": (row, 3, 48, 96, (), 0) for row in PARAMS}
SETS.update({f"many_{row}": (row, 65, 24, 64, (64,), 0) for row in ("base", "thr1")})
SETS.update({f"homography_{row}": (row, 2, 48, 96, (), 40) for row in ("base", "both0")})


def build(name):
    """(present, marks, frames) of a set."""
    row, n, rows, cols, busy, length = SETS[name]
    present, marks = scripts(n, threshold(row), busy, length)
    return present, marks, frames(present, rows, cols)


# The restart test: one context, the filter restarted into these rows in turn (None: off), SEGMENT_FRAMES frames each
RESTARTS = ("base", "thr1", None, "below_3", "thr0", "base")
SEGMENT_FRAMES = 18


def restart_segments(n):
    """[(row, threshold the script is written against, present[n][SEGMENT_FRAMES])]: every segment begins without a
    blob (the first report after a restart is the 6.0 of a fresh filter), then tracks, misses and drops."""
    return [(row, thr, scripts(n, thr, length=SEGMENT_FRAMES)[0])
            for row, thr in ((r, threshold(r) if r else 2) for r in RESTARTS)]


# ------------------------------------------------------------------------------------------------- the oracle ---

class Detections:
    """The oracle's chain (MOG2 at LR, the detector of ORACLE) over frames [T][n]...: det[t][s] = detection dict; the
    models stay in .orc for a comparison of the state at the end."""

    def __init__(self, fr, params=None, lr=LR):
        T, n, rows, cols = fr.shape[:4]
        self.orc = [O.Mog2(rows, cols, 3) for _ in range(n)]
        p = O.hsv_params(**(params or ORACLE))
        self.det = [[O.chain_step(self.orc[s], fr[t, s], lr, p)[0] for s in range(n)] for t in range(T)]


def measurements(det):
    """[n][T] of (valid, x, y): what the filter of each stream is fed."""
    return [[(d[s]["valid"], d[s]["x"], d[s]["y"]) for d in det] for s in range(len(det[0]))]


def filtered(det, row):
    """out[t][s]: the oracle filter of `row`, one fresh filter a stream, fed the detections det[t][s]."""
    kal = [O.Kalman(**kw(row)) for _ in det[0]]
    return [[kal[s].filter(d["valid"], d["x"], d["y"]) for s, d in enumerate(ds)] for ds in det]


INIT, TRACK, COAST, DROPPED = "init", "track", "coast", "dropped"


def lane_states(valid, found):
    """What a lane of k_kalman does on each sample of one stream, from the measurement's and the result's flags:
    initialise (a measurement, not tracking before), predict and correct on a measurement, coast on the stale
    measurement, or nothing (dropped, dropping now, or never found)."""
    out, before = [], False
    for v, f in zip(valid, found):
        out.append(DROPPED if not f else (TRACK if before else INIT) if v else COAST)
        before = f
    return out


def regime(valid, found):
    """Counts of one stream's run: tracked samples, drops (tracking -> not), initialisations, changes of lane state."""
    st = lane_states(valid, found)
    return dict(tracked=sum(found), drops=sum(1 for a, b in zip(found, found[1:]) if a and not b),
                inits=st.count(INIT), reinits=max(st.count(INIT) - 1, 0),
                changes=sum(1 for a, b in zip(st, st[1:]) if a != b))


def dyadic(num, den):
    """num / den is a dyadic rational (an fp64 division of small integers is then exact)."""
    d = Fraction(num, den).denominator
    return d & (d - 1) == 0


def same_bits(a, b):
    """a and b are the same fp64 value bit for bit -- or both NaN, whose sign and payload are not compared."""
    if math.isnan(b):
        return math.isnan(a)
    return np.float64(a).tobytes() == np.float64(b).tobytes()


# ------------------------------------------------------------------------------------------------ homographies ---

_EPS = 2.0 ** -23                       # FLT_EPSILON
_UP = float(np.nextafter(_EPS, 1.0))
HOMOGRAPHIES = {
    "identity":    [1, 0, 0, 0, 1, 0, 0, 0, 1],
    "affine":      [1.25, 0.5, -3.0, -0.25, 0.75, 11.5, 0, 0, 1],
    "projective":  [0.02, 0.001, -1.5, -0.002, 0.025, 0.75, 1e-4, -2e-4, 1.0],
    "neg_w":       [0.02, 0.001, -1.5, -0.002, 0.025, 0.75, 0, 0, -1],
    "w_eq_eps":    [0.02, 0.001, -1.5, -0.002, 0.025, 0.75, 0, 0, _EPS],       # |w| > FLT_EPSILON is false: (0, 0)
    "w_above_eps": [0.02, 0.001, -1.5, -0.002, 0.025, 0.75, 0, 0, _UP],
    "w_below_neg": [0.02, 0.001, -1.5, -0.002, 0.025, 0.75, 0, 0, -_UP],
    "zero_row":    [0.02, 0.001, -1.5, -0.002, 0.025, 0.75, 0, 0, 0],          # w = 0 everywhere: (0, 0)
    "vel_w":       [0.02, 0.001, -1.5, -0.002, 0.025, 0.75, 1e-3, -2e-3, 0],   # w from x, y (position), vx, vy (velocity)
}


def homography_of(h, k):
    """A filter result (or a detection: keys valid / x / y) through O.homography, as a filter result."""
    if "position_valid" not in k:
        k = dict(position_valid=k["valid"], velocity_valid=False, x=k["x"], y=k["y"], vx=0.0, vy=0.0)
    x, y, vx, vy = O.homography(h, k["position_valid"], k["x"], k["y"], k["velocity_valid"], k["vx"], k["vy"])
    return dict(position_valid=k["position_valid"], velocity_valid=k["velocity_valid"], x=x, y=y, vx=vx, vy=vy)
