"""Shared, seeded cases of the filter chain behind the motion and the subtraction tracker (oatgpu_set_tracker_filters, DESIGN.md
9h) and the reference chain, right and wrong (TEST INFRASTRUCTURE, no GPU imports: tests/test_tracker_filters_cpu.py checks the
case list on the reference alone, tests/test_tracker_filters_gpu.py and tests/test_tracker_filters_host_gpu.py feed the same
cases to the kernels and the binaries).

A sequence: noiseless frames[t][s] for n streams.  Every stream has a script present[s][t]: a lead of one or two frames without
a detection, a GAP of three frames without one, later a single miss.  Motion tracker: the lead frames are black, the block moves
one step a present frame and STANDS STILL on the others (an empty difference: an invalid detection).  Subtraction tracker: the
background alone on frame 0 and wherever the script has no block (the block has LEFT), alpha 0.  Streams have different tracks
and their gaps are staggered.

The reference per stream and frame: the oracle detection of the existing case modules (oracle_lib.Diff behind
diff_cases.oracle_frame; bsub_cases.Oracle), then marker_filters_ref.chain with one oracle_lib.Kalman per stream.  A detector
publishes no heading.  The configurations (CONFIGS) that need a position to aim at -- the homography whose w crosses FLT_EPSILON,
the regions -- take it from the reference chain in front of that member, never from the library."""
import functools
import math

import numpy as np

import bsub_cases as BC
import diff_cases as DC
import marker_filters_ref as R
import oracle_lib as O
import posfilt_cases as P

GEOMETRIES = [(48, 64, 3), (37, 61, 1)]        # rows, cols, channels; 37 x 61 is the odd geometry of the narrow front kernel
MANY = (24, 32, 1)                             # 66 streams: two workgroups of the filter kernel
T = 14
DIFF = dict(diff_threshold=12, blur=2)
BSUB = dict(alpha=0.0, erode=0, dilate=3)


# ------------------------------------------------------------------------------------------------------ sequences ----

def lead(s):
    return 1 + s % 2


def gap(s):
    g0 = 6 + s % 2
    return (g0, g0 + 1, g0 + 2)


def present(s, t):
    return t >= lead(s) and t not in gap(s) and t != 11 + s % 2


def _block(rows, cols):
    return max(2, min(9, rows // 4)), max(2, min(11, cols // 4))


def _where(rows, cols, s, k):
    rh, rw = _block(rows, cols)
    return (2 + (2 + s % 3) * k + 3 * s) % (rows - rh - 3) + 1, (3 + (4 + s % 2) * k + 7 * s) % (cols - rw - 3) + 1


def _base(rng, rows, cols, channels):
    shape = (rows, cols, 3) if channels == 3 else (rows, cols)
    b = rng.integers(40, 91, shape).astype(np.uint8)
    if channels == 3:                              # (bsub_cases: a narrow blue channel keeps the block's difference below S = 255)
        b[..., 0] = rng.integers(40, 51, (rows, cols))
    return b


@functools.lru_cache(maxsize=None)
def frames(kind, rows, cols, channels, n, n_frames=T):
    """[t][s] uint8 frames of tracker `kind` ("diff" / "bsub")"""
    rng = np.random.default_rng(rows * 1000 + cols * 10 + channels + n)
    bases = [_base(rng, rows, cols, channels) for _ in range(n)]
    rh, rw = _block(rows, cols)
    colour = (BC.RECT_BGR if channels == 3 else BC.RECT_GREY) if kind == "bsub" else ((90, 250, 130) if channels == 3 else 220)
    out = [[None] * n for _ in range(n_frames)]
    for s in range(n):
        k = 0
        for t in range(n_frames):
            f = bases[s].copy()
            if kind == "diff":
                if t < lead(s):
                    f[:] = 0
                else:
                    k += present(s, t)             # a still frame repeats the one before
                    y, x = _where(rows, cols, s, k)
                    f[y:y + rh, x:x + rw] = colour
            elif present(s, t):
                k += 1
                y, x = _where(rows, cols, s, k)
                f[y:y + rh, x:x + rw] = colour
            out[t][s] = f
    return out


def bsub_case(rows, cols, channels, n):
    """the bsub_cases.Case the subtraction tracker and its oracle are made from"""
    return BC.Case(f"tf-{rows}x{cols}", rows, cols, channels, n, BSUB["alpha"], BSUB["erode"], BSUB["dilate"])


class DetRef:
    """One stream of a tracker's reference detector: frame -> detection dict (valid, x, y, ...)."""

    def __init__(self, kind, rows, cols, channels):
        self.kind, self.args = kind, (rows, cols, channels)
        self.reset()

    def reset(self):
        rows, cols, channels = self.args
        if self.kind == "diff":
            self.o = O.Diff(rows, cols, DIFF["diff_threshold"], DIFF["blur"], *DC.AREA)
        else:
            self.o = BC.Oracle(bsub_case(rows, cols, channels, 1))

    def step(self, frame):
        return self.o.detect(DC.oracle_frame(frame))[0] if self.kind == "diff" else self.o.step(frame)[0]


@functools.lru_cache(maxsize=None)
def detections(kind, rows, cols, channels, n, n_frames=T):
    """det[t][s]: the oracle detections of frames(...)"""
    fr = frames(kind, rows, cols, channels, n, n_frames)
    refs = [DetRef(kind, rows, cols, channels) for _ in range(n)]
    return [[refs[s].step(fr[t][s]) for s in range(n)] for t in range(n_frames)]


# ---------------------------------------------------------------------------------------------- the reference chain ----

def measurement(d):
    """the record in front of the chain: an invalid Position2D keeps its initial (0, 0); a detector has no heading"""
    v = bool(d["valid"])
    return dict(position_valid=v, x=d["x"] if v else 0.0, y=d["y"] if v else 0.0, heading_valid=False, hx=0.0, hy=0.0)


def _round_away(v):
    return math.floor(abs(v) + 0.5) * (1 if v >= 0 else -1)


def _region_away(regions, x, y):
    pt = (_round_away(x), _round_away(y))
    for i, (_, points) in enumerate(regions):
        if R.point_polygon_test(R.contour_of(points), pt) >= 0:
            return i
    return -1


WRONG = ["homography_first", "region_on_pixels", "zero_as_measurement", "state_of_stream0", "pair_swapped", "restart_every_call",
         "round_half_away"]


def pairs(kind, det, t0, t1):
    """The front launches of a sequence call over frames t0 .. t1 - 1 as (first frame, frames): the motion tracker pairs frames
    once every stream has a last image (from the second frame of a context on), the subtraction tracker always."""
    out, t = [], t0
    while t < t1:
        nf = 2 if t + 1 < t1 and (kind == "bsub" or t > 0) else 1
        out.append((t, nf))
        t += nf
    return out


def chain_run(det, kalman=None, homography=None, regions=None, wrong=None, calls=None, kind="diff"):
    """out[t][s] of the chain over det[t][s], one fresh O.Kalman per stream.  calls: [(t0, t1)] the frames of each tracker call
    (default: one sequence call); they matter to the planted wrong chains `pair_swapped` and `restart_every_call` only."""
    n_frames, n = len(det), len(det[0])
    calls = calls or [(0, n_frames)]
    new = (lambda: O.Kalman(**kalman)) if kalman is not None else (lambda: None)
    kal = [new() for _ in range(n)]
    if wrong == "state_of_stream0":
        kal = [kal[0]] * n
    out = [None] * n_frames

    def one(t, s):
        m = measurement(det[t][s])
        if wrong == "zero_as_measurement":
            m["position_valid"] = True
        if wrong == "homography_first" and homography is not None:
            x, y, _, _ = O.homography(homography, m["position_valid"], m["x"], m["y"], False, 0.0, 0.0)
            k = R.chain(dict(m, x=x, y=y), kalman=kal[s])
            k["region_valid"], k["region"] = False, None
            if regions and k["position_valid"]:
                i = R.region_of(regions, k["x"], k["y"])
                k["region_valid"], k["region"] = i >= 0, regions[i][0] if i >= 0 else None
            return k
        if wrong == "region_on_pixels" and regions:
            k = R.chain(m, kalman=kal[s])
            i = R.region_of(regions, k["x"], k["y"]) if k["position_valid"] else -1
            if homography is not None:
                x, y, vx, vy = O.homography(homography, k["position_valid"], k["x"], k["y"], k["velocity_valid"], k["vx"], k["vy"])
                k = dict(k, x=x, y=y, vx=vx, vy=vy)
            return dict(k, region_valid=i >= 0, region=regions[i][0] if i >= 0 else None)
        k = R.chain(m, kalman=kal[s], homography=homography, regions=regions)
        if wrong == "round_half_away" and regions and k["position_valid"]:
            i = _region_away(regions, k["x"], k["y"])
            k = dict(k, region_valid=i >= 0, region=regions[i][0] if i >= 0 else None)
        return k

    for t0, t1 in calls:
        if wrong == "restart_every_call":
            kal = [new() for _ in range(n)]
        order = []
        for t, nf in pairs(kind, det, t0, t1) if t1 - t0 > 1 else [(t0, 1)]:
            order += [t + 1, t] if nf == 2 and wrong == "pair_swapped" else list(range(t, t + nf))
        for t in order:
            out[t] = [one(t, s) for s in range(n)]
    return out


# ------------------------------------------------------------------------------------------------- configurations ----

# rows of tests/posfilt_cases.py: timeout 0 (never tracks); a drop threshold of 2 frames (shorter than the gap of 3) and of 8
# (longer); zero measurement noise
KALMAN = {"k_thr0": "thr0", "k_short": "below_3", "k_long": "base", "k_noise0": "noise0"}
FINITE = ("k_short", "k_long", "k_noise0")
ALL_ROW = "noise0"                             # the Kalman row of the configurations with every member on: it follows the block


def _points(out):
    return [(t, s, k["x"], k["y"]) for t, ks in enumerate(out) for s, k in enumerate(ks) if k["position_valid"]]


def crossing_homography(out):
    """A matrix whose w = y - y* is exactly 0 -- inside FLT_EPSILON -- on the sample (t, s) of `out` (the chain in front of the
    homography) in the middle of its valid ones, and far outside on samples with another y."""
    pts = _points(out)
    y_star = pts[len(pts) // 2][3]
    return [0.02, 0.001, -1.5, -0.002, 0.025, 0.75, 0.0, 1.0, -y_star]


def regions_for(out):
    """[(name, points)] aimed at the positions of `out` (the chain in front of the region member): `west` ends at the column of a
    position whose x is a tie k + 0.5 with k even where there is one (cvRound takes k: on the edge; half away from zero takes k
    + 1: out), `over` overlaps it and reaches five columns further, `tip` is a triangle with a vertex on a position east of both."""
    pts = _points(out)
    xs, ys = [p[2] for p in pts], [p[3] for p in pts]
    x_lo, x_hi, y_lo, y_hi = math.floor(min(xs)) - 4, math.ceil(max(xs)) + 4, math.floor(min(ys)) - 4, math.ceil(max(ys)) + 4
    ties = sorted(x for x in xs if x - math.floor(x) == 0.5 and math.floor(x) % 2 == 0)
    mid = sorted(xs)[len(xs) // 2]
    edge = int(math.floor(ties[len(ties) // 2])) if ties else R.cv_round(mid)
    east = [p for p in pts if R.cv_round(p[2]) > edge + 5]
    regions = [("west", [(x_lo, y_lo), (edge, y_lo), (edge, y_hi), (x_lo, y_hi)]),
               ("over", [(x_lo + 2, y_lo + 1), (edge + 5, y_lo + 1), (edge + 5, y_hi - 1), (x_lo + 2, y_hi - 1)])]
    if east:
        vx, vy = R.cv_round(east[0][2]), R.cv_round(east[0][3])
        regions.append(("tip", [(vx, vy), (vx + 2, vy + 3), (vx - 2, vy + 3)]))
    return regions


HOMOGRAPHIES = {"h_affine": P.HOMOGRAPHIES["affine"], "h_projective": P.HOMOGRAPHIES["projective"]}
CONFIGS = list(KALMAN) + list(HOMOGRAPHIES) + ["h_cross", "regions", "all", "all_cross"]


@functools.lru_cache(maxsize=None)
def config(name, kind, rows, cols, channels, n, n_frames=T):
    """-> dict(kalman=, homography=, regions=): the keywords of set_filters and of chain_run (kalman: O.Kalman's keywords)"""
    det = detections(kind, rows, cols, channels, n, n_frames)
    if name in KALMAN:
        return dict(kalman=P.kw(KALMAN[name]), homography=None, regions=None)
    if name in HOMOGRAPHIES:
        return dict(kalman=None, homography=HOMOGRAPHIES[name], regions=None)
    if name == "h_cross":
        return dict(kalman=None, homography=crossing_homography(chain_run(det)), regions=None)
    if name == "regions":
        return dict(kalman=None, homography=None, regions=regions_for(chain_run(det)))
    k = P.kw(ALL_ROW)
    if name == "all":
        h = HOMOGRAPHIES["h_affine"]
        return dict(kalman=k, homography=h, regions=regions_for(chain_run(det, kalman=k, homography=h)))
    if name == "all_cross":
        return dict(kalman=k, homography=crossing_homography(chain_run(det, kalman=k)), regions=None)
    raise KeyError(name)


def want(name, kind, rows, cols, channels, n, n_frames=T, wrong=None, calls=None):
    det = detections(kind, rows, cols, channels, n, n_frames)
    return chain_run(det, wrong=wrong, calls=calls, kind=kind, **config(name, kind, rows, cols, channels, n, n_frames))


def same(a, b):
    """two reference records agree in what the tests compare (flags and region exactly, doubles by ==, NaN with NaN)"""
    flags = ("position_valid", "velocity_valid", "heading_valid", "region_valid", "region")
    return all(a[k] == b[k] for k in flags) and all(
        (math.isnan(a[k]) and math.isnan(b[k])) or a[k] == b[k] for k in ("x", "y", "vx", "vy", "hx", "hy"))


def differs(a, b):
    return any(not same(x, y) for xs, ys in zip(a, b) for x, y in zip(xs, ys))
