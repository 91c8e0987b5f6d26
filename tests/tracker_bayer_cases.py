"""Shared, seeded cases of the motion and the subtraction tracker on Bayer RAW8 frames (oatgpu_set_tracker_bayer)
and numpy front ends for them, right and wrong (TEST INFRASTRUCTURE: tests/test_tracker_bayer_cpu.py checks the case list
without a GPU, tests/test_diff_bayer_gpu.py and tests/test_bsub_bayer_gpu.py feed the same cases to the kernels).

A raw case wraps a BGR case of tests/diff_cases.py or tests/bsub_cases.py (channels = 3): raw[t][s] =
debayer_ref.mosaic(scene frame, pattern of stream s) is what the camera delivers, bgr[t][s] = debayer_ref.demosaic(raw[t][s],
pattern) is what the chain behind the demosaic sees.  The reference for a RAW8 run is the BGR tracker fed bgr[t][s]; beside it
run diff_cases.Model + the oracle's `posidet diff`, or bsub_cases.Ref, on the same frames."""
import functools
from dataclasses import dataclass

import numpy as np

import bsub_cases as B
import debayer_ref as R
import diff_cases as D
import oracle_lib as O

# diff_cases' five (narrow with Wp > W; wide with whole lanes beyond W; wide with a tail wave; one word a row; one lane a row)
# plus: the smallest frame and the 3-row frame (every output row clamps to row 1), 4 x 8 (even row count: the last row takes
# the other parity), and the shape that crosses wave and workgroup boundaries of the wide mapping
GEOMETRIES = list(D.GEOMETRIES) + [(3, 3), (3, 4), (4, 8), (12, 1040)]
BIG = [g for g in GEOMETRIES if g[0] >= 33]                 # the geometries whose references must detect (non-vacuity)
THREE = (R.RGGB, R.GRBG, R.BGGR)                            # three streams, three patterns
THREE_SWAPPED = (R.GRBG, R.RGGB, R.BGGR)


@dataclass
class RawCase:
    c: object               # the BGR case: parameters, ROI, background from a file, the scene frames
    patterns: tuple         # [s] OATGPU_BAYER_* of every stream
    raw: list               # [t][s] (rows, cols) uint8
    bgr: list               # [t][s] (rows, cols, 3) uint8, the demosaiced frames


def _wrap(c, patterns):
    assert c.channels == 3 and len(patterns) == c.n_streams
    raw = [[R.mosaic(f, patterns[s]) for s, f in enumerate(fs)] for fs in c.frames]
    bgr = [[R.demosaic(r, patterns[s]) for s, r in enumerate(rs)] for rs in raw]
    return RawCase(c, tuple(patterns), raw, bgr)


@functools.lru_cache(maxsize=None)
def diff_case(rows, cols, patterns, roi=False, n_frames=12, thr=12, blur=2):
    c = D.make_case(f"raw-{rows}x{cols}-{patterns}", rows, cols, 3, len(patterns), diff_threshold=thr, blur=blur, roi=roi,
                    n_frames=n_frames, seed=rows + len(patterns))
    return _wrap(c, patterns)


@functools.lru_cache(maxsize=None)
def bsub_case(rows, cols, patterns, alpha=0.05, roi=False, background=False, n_frames=B.N_FRAMES):
    c = B.make_case(f"raw-{rows}x{cols}-{patterns}-a{alpha}", rows, cols, 3, len(patterns), alpha=alpha, roi=roi,
                    background=background, n_frames=n_frames, seed=rows + len(patterns))
    return _wrap(c, patterns)


def diff_cases():
    """every geometry with every pattern; three streams with three patterns, a ROI set and removed on one of them"""
    return ([diff_case(r, c, (p,)) for r, c in GEOMETRIES for p in R.PATTERNS]
            + [diff_case(90, 200, THREE, roi=True), diff_case(37, 91, THREE, roi=True)])


def bsub_cases():
    return ([bsub_case(r, c, (p,), alpha=a) for r, c in GEOMETRIES for p in R.PATTERNS for a in (0.0, 0.05)]
            + [bsub_case(90, 200, THREE, roi=True), bsub_case(37, 91, THREE, alpha=0.0, roi=True)])


# --------------------------------------------------------------------------------------- front ends, right and wrong ----

# the pattern with the R sample's row parity, column parity, or both flipped
_FLIP_ROW = {R.RGGB: R.GBRG, R.GBRG: R.RGGB, R.BGGR: R.GRBG, R.GRBG: R.BGGR}
_FLIP_COL = {R.RGGB: R.GRBG, R.GRBG: R.RGGB, R.BGGR: R.GBRG, R.GBRG: R.BGGR}
_FLIP_BOTH = {R.RGGB: R.BGGR, R.BGGR: R.RGGB, R.GRBG: R.GBRG, R.GBRG: R.GRBG}

# r and b swapped; the row / the column parity flipped; border pixels taking their own site from edge-replicated samples instead
# of the neighbour's triple; the ROI applied to the raw samples; every second frame (the second of a paired launch) of streams
# 1.. demosaiced with stream 0's pattern
WRONG = ["swap_rb", "row_parity", "col_parity", "border_own_site", "roi_on_raw", "pair_pattern0"]


def handed(rc, t, s, wrong=None):
    """-> (BGR frame, ROI or None) as a front end hands frame t of stream s to the chain behind the demosaic"""
    p, raw, roi = rc.patterns[s], rc.raw[t][s], rc.c.roi_at(t, s)
    if wrong is None:
        return rc.bgr[t][s], roi
    if wrong == "swap_rb":
        return np.ascontiguousarray(rc.bgr[t][s][..., ::-1]), roi
    if wrong == "row_parity":
        return R.demosaic(raw, _FLIP_ROW[p]), roi
    if wrong == "col_parity":
        return R.demosaic(raw, _FLIP_COL[p]), roi
    if wrong == "border_own_site":                          # (the padded image's tile starts one row and one column earlier)
        return np.ascontiguousarray(R.demosaic(np.pad(raw, 1, mode="edge"), _FLIP_BOTH[p])[1:-1, 1:-1]), roi
    if wrong == "roi_on_raw":
        if roi is None:
            return rc.bgr[t][s], None
        r = raw.copy()
        r[roi == 0] = 0
        return R.demosaic(r, p), None
    if wrong == "pair_pattern0":
        return (R.demosaic(raw, rc.patterns[0]) if t % 2 == 1 else rc.bgr[t][s]), roi
    raise ValueError(wrong)


def diff_bits(rc, wrong=None):
    """[t][s] threshold bits of the motion chain behind front end `wrong`"""
    ms = [D.Model(rc.c.diff_threshold, rc.c.blur) for _ in rc.patterns]
    return [[ms[s].front(*handed(rc, t, s, wrong))[0] for s in range(len(ms))] for t in range(len(rc.raw))]


def _bsub_models(rc):
    ms = [B.Model(rc.c.alpha) for _ in rc.patterns]
    for s, img in rc.c.background.items():
        ms[s].set_background(img)
    return ms


def bsub_bits(rc, wrong=None):
    """[t][s] (window bits, background) of the subtraction chain behind front end `wrong`"""
    ms = _bsub_models(rc)
    return [[ms[s].front(*handed(rc, t, s, wrong))[:2] for s in range(len(ms))] for t in range(len(rc.raw))]


def tells_apart(rc, chain, wrong):
    right, bad = chain(rc), chain(rc, wrong)
    flat = lambda x: [np.asarray(a) for fs in x for e in fs for a in (e if isinstance(e, tuple) else (e,))]  # noqa: E731
    return any((a != b).any() for a, b in zip(flat(right), flat(bad)))


# ------------------------------------------------------------------------------------------------ the references ----

class DiffRef:
    """One stream of the motion chain's reference: the oracle's `posidet diff` on framefilt mask -> col GREY of the frame, with
    the numpy front end beside it for the THRESHOLD tap.  step -> (detection, threshold bits, oracle mask > 0, first frame?)"""

    def __init__(self, c):
        self.c = c
        self.reset()

    def reset(self):
        self.o = O.Diff(self.c.rows, self.c.cols, self.c.diff_threshold, self.c.blur, *D.AREA)
        self.m = D.Model(self.c.diff_threshold, self.c.blur)

    def step(self, frame, roi=None):
        first = self.m.last is None
        bits, _ = self.m.front(frame, roi)
        det, thr = self.o.detect(D.oracle_frame(frame, roi))
        return det, bits, thr > 0, first


@functools.lru_cache(maxsize=None)
def _diff_want(rows, cols, patterns, roi, n_frames, thr, blur):
    rc = diff_case(rows, cols, patterns, roi, n_frames, thr, blur)
    refs = [DiffRef(rc.c) for _ in patterns]
    return [[refs[s].step(f, rc.c.roi_at(t, s)) for s, f in enumerate(fs)] for t, fs in enumerate(rc.bgr)]


def diff_want(rows, cols, patterns, roi=False, n_frames=12, thr=12, blur=2):
    """-> (raw case, want[t][s] = DiffRef.step of the demosaiced frames), computed once and shared"""
    return diff_case(rows, cols, patterns, roi, n_frames, thr, blur), _diff_want(rows, cols, patterns, roi, n_frames, thr, blur)


@functools.lru_cache(maxsize=None)
def _bsub_want(rows, cols, patterns, alpha, roi, background, n_frames):
    rc = bsub_case(rows, cols, patterns, alpha, roi, background, n_frames)
    refs = [B.Ref(rc.c, s) for s in range(len(patterns))]
    return [[refs[s].step(f, rc.c.roi_at(t, s)) for s, f in enumerate(fs)] for t, fs in enumerate(rc.bgr)]


def bsub_want(rows, cols, patterns, alpha=0.05, roi=False, background=False, n_frames=B.N_FRAMES):
    """-> (raw case, want[t][s] = bsub_cases.Ref.step of the demosaiced frames: (detection, bits, morph > 0, bg, acc))"""
    return (bsub_case(rows, cols, patterns, alpha, roi, background, n_frames),
            _bsub_want(rows, cols, patterns, alpha, roi, background, n_frames))
