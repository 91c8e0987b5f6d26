"""Scenes, parameters and expected values of the marker filter chain tests (TEST INFRASTRUCTURE, no GPU imports).

Frames in the style of tests/posfilt_cases.py: every marker is a rectangle of its own colour on black that moves with t, and
a script says in which frames it is there -- so position_valid of the combined record drops and returns, and the Kalman
member coasts, times out and restarts.  Marker 0 (blue, the heading anchor) follows posfilt_cases.script of its stream;
marker 1 (red) misses single frames on a period of its own.  Expected values: the oracle chain once per marker
(markers_ref.MarkerOracle), markers_ref.combine, then marker_filters_ref.chain (O.Kalman, O.homography and the restated
heading / region members)."""
import functools

import numpy as np

import marker_filters_ref as R
import markers_ref as MR
import oracle_lib as O
import posfilt_cases as P

LR = 0.0
NZ = dict(h_thresh=(0, 256), s_thresh=(0, 256), v_thresh=(1, 256))                   # the context's own, non-zero window
OWN = dict(adaptation_coeff=LR, erode=0, dilate=3, area=(4.0, 1e6), **NZ)
_MORPH = dict(erode=0, dilate=3, area=(4.0, 1e6))
BLUE = dict(h=(100, 125), s=(150, 256), v=(100, 256), **_MORPH)
RED = dict(h=(0, 20), s=(150, 256), v=(100, 256), **_MORPH)
MARKERS = [BLUE, RED]
BGR = [(255, 0, 0), (0, 0, 255)]

# name -> (streams, rows, cols, markers, frames, the Kalman row the marker-0 scripts are written against, busy streams).
# An odd number of frames everywhere: with two frames a launch a lone frame follows the paired steps.
SHAPES = {
    "matrix": (3, 48, 64, 2, 31, "below_3", ()),
    "many":   (65, 24, 64, 2, 21, "thr1", (64,)),      # two workgroups of the chain kernel; lanes 63 / 64 on different scripts
    "single": (1, 48, 64, 1, 15, "thr1", ()),          # M = 1: the heading is 0 / 0 = NaN with heading_valid 1
}

KALMAN_ROWS = ("below_3", "thr0", "thr1", "both0")


def rect(s, t, m, rows, cols, M):
    """(y0, x0, h, w) of marker m of stream s in frame t: marker m keeps to its own vertical band of the frame, clear of
    the image frame and of the dilation's reach."""
    band = cols // M
    h, w = 3 + (s + t + m) % 2, 4 + (s + 2 * m + t) % 3
    y0 = 2 + (2 * t + 5 * s + 3 * m) % (rows - h - 4)
    x0 = band * m + 2 + ((3 + s % 5) * t + 7 * s + m) % (band - w - 4)
    return y0, x0, h, w


def present(shape):
    """bool [M][n][T]"""
    n, rows, cols, M, T, row, busy = SHAPES[shape]
    p0, _ = P.scripts(n, P.threshold(row), busy, T)
    out = np.ones((M, n, T), bool)
    out[0] = p0
    for m in range(1, M):
        for s in range(n):
            out[m, s, [t for t in range(T) if t % 11 == (5 + s) % 11 or t == 0]] = False
    return out


@functools.lru_cache(maxsize=None)
def frames(shape):
    """uint8 [T][n][rows][cols][3]"""
    n, rows, cols, M, T, _, _ = SHAPES[shape]
    pr = present(shape)
    f = np.zeros((T, n, rows, cols, 3), np.uint8)
    for t in range(T):
        for s in range(n):
            for m in range(M):
                if pr[m, s, t]:
                    y0, x0, h, w = rect(s, t, m, rows, cols, M)
                    f[t, s, y0:y0 + h, x0:x0 + w] = BGR[m]
    return f


@functools.lru_cache(maxsize=None)
def detections(shape):
    """The oracle alone: (det[t][s][m] detection dicts, fg[t][s] the own window's detection, combined[t][s])."""
    n, rows, cols, M, T, _, _ = SHAPES[shape]
    fr = frames(shape)
    cams = [MR.MarkerOracle(rows, cols, 3, MARKERS[:M], nthreads=1) for _ in range(n)]
    own = [O.Mog2(rows, cols, 3) for _ in range(n)]
    own_p = O.hsv_params(h_lo=0, h_hi=256, s_lo=0, s_hi=256, v_lo=1, v_hi=256, erode=0, dilate=3, min_area=4.0, max_area=1e6)
    det, fg, comb = [], [], []
    for t in range(T):
        det.append([cams[s].step(fr[t, s], LR)[0] for s in range(n)])
        fg.append([O.chain_step(own[s], fr[t, s], LR, own_p)[0] for s in range(n)])
        comb.append([MR.combine([(d["valid"], d["x"] if d["valid"] else 0.0, d["y"] if d["valid"] else 0.0) for d in det[t][s]], 0)
                     for s in range(n)])
    return det, fg, comb


# ------------------------------------------------------------------------------------------------ chain members ---

AFFINE = [1.25, 0.5, -3.0, -0.25, 0.75, 11.5, 0, 0, 1]
# w = x - 32.25: the mean x of the two markers (a multiple of 0.25 in 16.. 48) passes 32.25 -- w is 0 on some frames
# (|w| > FLT_EPSILON is false: (0, 0)) and takes both signs on others
PROJECTIVE = [0.5, 0.25, -7.0, -0.125, 0.75, 2.5, 1.0, 0.0, -32.25]
HOMOGRAPHIES = {"affine": AFFINE, "projective": PROJECTIVE}

# two overlapping quadrilaterals (the first configured wins where they overlap) and a concave polygon, in pixels of the
# 48 x 64 scene: the means of the scripted markers land inside, outside, on an edge and on a vertex of them
REGIONS = [
    ("north", [(24.0, 8.0), (36.0, 8.0), (36.0, 22.0), (24.0, 22.0)]),
    ("centre", [(30.4, 14.5), (44.0, 15.0), (44.0, 30.0), (30.0, 30.0)]),            # 30.4 -> 30, 14.5 -> 14 (ties to even)
    ("hook", [(20.0, 24.0), (30.0, 24.0), (30.0, 32.0), (26.0, 32.0), (26.0, 28.0), (20.0, 28.0)]),
]


def expected(shape, kalman=None, homography=None, regions=None, restart_at=()):
    """want[t][s]: marker_filters_ref.chain over the oracle's combined records; kalman: a row of posfilt_cases.PARAMS;
    restart_at: frames before which every camera's filter is a fresh one (set_marker_filters again)."""
    _, _, comb = detections(shape)
    n = SHAPES[shape][0]
    kal = None
    out = []
    for t, cs in enumerate(comb):
        if kalman and (t == 0 or t in restart_at):
            kal = [O.Kalman(**P.kw(kalman)) for _ in range(n)]
        out.append([R.chain(cs[s], kal[s] if kal else None, homography, regions) for s in range(n)])
    return out


# (id, kalman row, homography name, regions on): every member alone, in pairs, all three
CONFIGS = [("kalman_" + r, r, None, False) for r in KALMAN_ROWS] + [
    ("homography_affine", None, "affine", False), ("homography_projective", None, "projective", False),
    ("region", None, None, True),
    ("kalman_homography", "below_3", "affine", False), ("kalman_region", "thr1", None, True),
    ("homography_region", None, "projective", True),
    ("all_affine", "below_3", "affine", True), ("all_projective", "both0", "projective", True), ("all_thr0", "thr0", "affine", True),
]


def config(name):
    """-> (set_marker_filters keywords, expected() keywords)"""
    _, row, hname, reg = next(c for c in CONFIGS if c[0] == name)
    h = HOMOGRAPHIES[hname] if hname else None
    return (dict(kalman=P.kw(row) if row else None, homography=np.array(h).reshape(3, 3) if h else None,
                 regions=REGIONS if reg else None),
            dict(kalman=row, homography=h, regions=REGIONS if reg else None))


def coverage(name, shape="matrix"):
    """What a configuration exercises on a shape, from the expected values alone:
    kalman   per stream, posfilt_cases.regime of (measurement valid, filter found)
    kinds    how often a filtered position lies 'inside' / 'outside' / on an 'edge' / on a 'vertex' of a configured region
    overlap  positions that two regions hold, and how many of them were given to the first configured
    w        the homography's w = x m6 + y m7 + m8 of every transformed position: (|w| <= FLT_EPSILON, w > 0, w < 0) counts"""
    _, kw_exp = config(name)
    _, _, comb = detections(shape)
    want = expected(shape, **kw_exp)
    n = SHAPES[shape][0]
    out = dict(kalman=[], kinds={}, overlap=[0, 0], w=[0, 0, 0])
    if kw_exp["kalman"]:
        for s in range(n):
            out["kalman"].append(P.regime([c[s]["position_valid"] for c in comb], [w[s]["position_valid"] for w in want]))
    pre = expected(shape, kalman=kw_exp["kalman"])           # the positions the homography and the regions are given
    h = kw_exp["homography"]
    for ws, ps in zip(want, pre):
        for w, p in zip(ws, ps):
            if not w["position_valid"]:
                continue
            if h:
                v = p["x"] * h[6] + p["y"] * h[7] + h[8]
                out["w"][0 if abs(v) <= R.FLT_EPSILON else 1 if v > 0 else 2] += 1
            if kw_exp["regions"]:
                hits = []
                for i, (_, pts) in enumerate(REGIONS):
                    kind = R.where(pts, w["x"], w["y"])
                    out["kinds"][kind] = out["kinds"].get(kind, 0) + 1
                    if kind != "outside":
                        hits.append(i)
                assert w["region"] == (REGIONS[hits[0]][0] if hits else None)
                if len(hits) > 1:
                    out["overlap"][0] += 1
                    out["overlap"][1] += w["region"] == REGIONS[hits[0]][0]
    return out
