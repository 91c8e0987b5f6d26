"""Frame sequences for the motion tracker and the subtraction tracker whose FINAL mask is a chosen mask, exactly -- at the
capacity of the blob stage's LDS kernel or one over it (TEST INFRASTRUCTURE: tests/test_busy_trackers_cpu.py holds the
constructions to the models and the oracle without a GPU, tests/test_busy_trackers_gpu.py feeds them to the kernels).

The masks are blob_load.pipeline_masks(H, W) -- runs_at / runs_over / roots_at / roots_over / empty -- plus `rect` (one
rectangle, the quiet frame of the many-stream cases) and `noise` (50 % salt, for the forms whose mask cannot be set exactly:
an adapting background, a demosaic in front).  Every mask but `empty` and `noise` carries a TAG: the last foreground run of
the rows of its topmost blob is widened by tag(s, t) pixels.  That changes no run count and no component count (the CPU file
checks it), and makes the largest blob -- hence the expected detection -- different for every stream and frame, so that a
stale or mis-indexed result cannot equal the right one.

How a mask M becomes a frame:
  * motion tracker (threshold THR, blur 0): a parity plane P per stream, all zero before the stream's first frame;
    P ^= M, frame = ON where P is set, else 0.  A first frame's bits are g != 0 = M; later |g - last| = ON > THR exactly on M.
    BGR frames carry the value in all three channels (grey(v, v, v) = v).  A reset stream restarts from P = 0.
    With blur 2 the frames are the same and the final mask is the model's dilation of M.
  * subtraction tracker (alpha 0, erode 0, dilate 0): the background is the constant BG (set_background, or a stream's first
    frame: that frame's mask is empty), frame = BG + INSIDE_BGR (GREY: BG + 150) where M is set.
  * the noise forms (alpha 0.05; RAW8 in front of either tracker): the same constructions on `noise` / `rect` / `empty`
    masks; the expected mask is the model's (bsub_cases.Model, diff_cases.Model, debayer_ref.demosaic in front).

A schedule is kinds[t][s].  The standard one has kind_at(t + s): period three in lds / global, so that over 16 frames every
slot t % 4 of the in-flight sequence holds global after lds, lds after global and global after global, for every stream, and
one frame set mixes global and lds streams."""
import functools
import hashlib
from dataclasses import dataclass

import numpy as np

import blob_load as L
import bsub_cases as B
import debayer_ref as R
import diff_cases as D
import oracle_lib as O

DBL_MAX = float(np.finfo(np.float64).max)
AREA = (0.0, DBL_MAX)
SHAPES = ((200, 360), (200, 361))        # four pixels a lane; one pixel a lane with padded rows
MANY = (150, 203)                        # where many streams are needed
THR, ON = 12, 200                        # the motion tracker's threshold and the value of a set parity pixel
BG, GREY_STEP = 10, 150                  # the subtraction tracker's background and the GREY difference (inside GREY_WIN)
NOISE_BGR = (21, 200, 81)                # the noise forms' difference: HSV (50, 228, 200), mid-window, and still inside
#                                          the window at 0.7 of it (an adapted background shrinks the difference)
N_STANDARD = 17                          # 16 frames of schedule and the frame behind the longest sequence
DECLARED = dict(runs_at="lds", runs_over="global", roots_at="lds", roots_over="global", empty="lds", rect="lds", noise="global")
TAGGED = ("runs_at", "runs_over", "roots_at", "roots_over", "rect")
NOISE_OF = dict(runs_at="rect", roots_at="rect", rect="rect", empty="empty", runs_over="noise", roots_over="noise", noise="noise")


def tag(s, t):
    """Pixels by which the mask of stream s on frame t is widened: distinct over 97 streams of a set, and between frame t
    and t - 1, t - 4 of a stream."""
    return 1 + (5 * s + 3 * t) % 97


@functools.lru_cache(maxsize=None)
def _bases(H, W):
    """{kind: (bool mask, [(rows to widen, first column right of their last run)])}"""
    out = {}
    masks = {k: m for k, (m, _) in L.pipeline_masks(H, W).items()}
    rect = np.zeros((H, W), np.uint8)
    L.paint_rect(rect, 3, 12, 4, 41)
    masks["rect"] = rect
    for k, m in masks.items():
        m = m != 0
        spans = []
        if k in TAGGED:
            dirty = m.any(axis=1)
            y0 = int(np.argmax(dirty))
            y1 = y0
            while dirty[y1]:
                y1 += 1
            last = np.array([np.nonzero(m[y])[0][-1] for y in range(y0, y1)])
            spans.append((tuple(int(y0 + i) for i in np.nonzero(last == last.max())[0]), int(last.max()) + 1))
            if k.startswith("runs"):
                # the one-row bar under the comb as well: of area 0 as it stands, but a dilation (blur 2) joins it and the
                # comb's columns into the largest blob
                yb = int(np.nonzero(dirty)[0][-1])
                assert yb > y1
                spans.append(((yb,), int(np.nonzero(m[yb])[0][-1]) + 1))
            for rows, x in spans:
                assert not m[list(rows), x:].any() and x + 98 < W - 1, "the widened runs end their rows, inside the frame"
        out[k] = (m, spans)
    return out


def mask_of(H, W, kind, s, t, block=1):
    """The intended final mask (bool) of stream s on frame t.  noise: seeded 50 % salt in block x block cells."""
    if kind == "noise":
        rng = np.random.default_rng(1000003 * H + 1009 * W + 101 * s + t)
        cells = rng.random((-(-H // block), -(-W // block))) < 0.5
        m = np.repeat(np.repeat(cells, block, axis=0), block, axis=1)[:H, :W]
        return L.frame_zeroed(m).astype(bool)
    m, spans = _bases(H, W)[kind]
    m = m.copy()
    for rows, x in spans:
        m[list(rows), x:x + tag(s, t)] = True
    return m


def kind_at(u):
    """The standard schedule: u % 3 == 0 is an lds frame (runs_at, roots_at, empty in turn), the others global (runs_over and
    roots_over in turn).  u = 6 is `empty` behind global frames at u - 1 and u - 4."""
    if u % 3 == 0:
        return ("runs_at", "roots_at", "empty")[(u // 3) % 3]
    return ("runs_over", "roots_over")[(u - u // 3 - 1) % 2]


def standard(n_streams, n_frames=N_STANDARD):
    return [[kind_at(t + s) for s in range(n_streams)] for t in range(n_frames)]


_LOADS = {}


def load_of(final):
    """blob_load of a final mask, computed once per distinct mask"""
    f = np.ascontiguousarray(np.asarray(final) != 0, np.uint8)
    key = (f.shape, hashlib.sha1(f.tobytes()).digest())
    if key not in _LOADS:
        _LOADS[key] = L.blob_load(f)
    return _LOADS[key]


def largest(final, area=AREA):
    """The largest-blob rule on a final mask"""
    return O.sift_contours(np.where(final, 255, 0).astype(np.uint8), *area)


@dataclass
class Step:
    """One frame set: per stream the kind, the frame handed to the library, the intended mask (None where the form is not
    exact), the expected FINAL tap (bool), the oracle's detection, blob_load's path of the expected tap, first frame?"""
    t: int
    kinds: list
    frames: list
    intended: list
    final: list
    want: list
    path: list
    first: list
    state: list = None      # subtraction tracker: (background, fp32 accumulator or None) of the model behind the frame


class DiffRun:
    """The motion tracker's frames, model and oracle, stream by stream.  patterns: RAW8 frames in front (BGR tracker)."""

    def __init__(self, rows, cols, channels, n, blur=0, patterns=None, area=AREA, block=1):
        assert patterns is None or channels == 3
        self.rows, self.cols, self.channels, self.n = rows, cols, channels, n
        self.blur, self.patterns, self.area, self.block = blur, patterns, area, block
        self.exact = blur == 0 and patterns is None
        self.t = 0
        self.P, self.m, self.o = [None] * n, [None] * n, [None] * n
        for s in range(n):
            self.reset(s)

    def reset(self, s):
        self.P[s] = np.zeros((self.rows, self.cols), bool)
        self.m[s] = D.Model(THR, self.blur, self.area)
        self.o[s] = O.Diff(self.rows, self.cols, THR, self.blur, *self.area)

    def step(self, kinds):
        st = self.step_masks([mask_of(self.rows, self.cols, k, s, self.t, self.block) for s, k in enumerate(kinds)], list(kinds))
        return st

    def step_masks(self, masks, kinds=None):
        st = Step(self.t, kinds or ["given"] * self.n, [], [], [], [], [], [])
        for s, M in enumerate(masks):
            self.P[s] = self.P[s] ^ M
            v = np.where(self.P[s], ON, 0).astype(np.uint8)
            scene = np.ascontiguousarray(np.stack([v, v, v], -1)) if self.channels == 3 else v
            if self.patterns is not None:
                frame = R.mosaic(scene, self.patterns[s])
                seen = R.demosaic(frame, self.patterns[s])
            else:
                frame = seen = scene
            first = self.m[s].last is None
            det, _, mask = self.m[s].detect(seen)
            odet, othr = self.o[s].detect(D.oracle_frame(seen))
            assert D.same_dict(det, odet), ("model and oracle disagree", self.t, s)
            inner = (slice(None),) * 2 if first else (slice(1, -1),) * 2
            assert ((othr > 0)[inner] == mask[inner]).all(), ("model and oracle masks disagree", self.t, s)
            final = L.frame_zeroed(mask).astype(bool)
            st.frames.append(frame)
            st.intended.append(M if self.exact and st.kinds[s] != "noise" else None)
            st.final.append(final)
            st.want.append(odet)
            st.path.append(load_of(final)["path"])
            st.first.append(first)
        self.t += 1
        return st


class BsubRun:
    """The subtraction tracker's frames, model and oracle.  preset: the background comes from set_background (alpha 0 only);
    otherwise a stream's first frame is the constant background and its mask is empty whatever the schedule says."""

    def __init__(self, rows, cols, channels, n, alpha=0.0, preset=True, patterns=None, area=AREA, block=1):
        assert not (preset and alpha > 0) and (patterns is None or channels == 3)
        self.rows, self.cols, self.channels, self.n = rows, cols, channels, n
        self.alpha, self.preset, self.patterns, self.area, self.block = float(alpha), preset, patterns, area, block
        self.exact = alpha == 0 and patterns is None
        self.case = B.Case("busy", rows, cols, channels, n, float(alpha), 0, 0)
        self.shape = self.case.shape
        self.background = np.full(self.shape, BG, np.uint8)
        self.step_value = (B.INSIDE_BGR if self.exact else NOISE_BGR) if channels == 3 else GREY_STEP
        self.t = 0
        self.m, self.o, self.have = [None] * n, [None] * n, [False] * n
        for s in range(n):
            self.reset(s, preset)

    def reset(self, s, preset=False):
        self.m[s] = B.Model(self.alpha)
        self.o[s] = B.Oracle(self.case, self.background if preset else None)
        if preset:
            self.m[s].set_background(self.background)
        self.have[s] = preset

    def tracker_args(self):
        kw = dict(n_streams=self.n, channels=self.channels, alpha=self.alpha, erode=0, dilate=0, area=self.area)
        if self.channels == 3:
            kw.update(h_thresh=B.HSV_WIN["h"], s_thresh=B.HSV_WIN["s"], v_thresh=B.HSV_WIN["v"])
        else:
            kw.update(thresh=B.GREY_WIN)
        return kw

    def step(self, kinds):
        kinds = [k if self.have[s] else "empty" for s, k in enumerate(kinds)]
        return self.step_masks([mask_of(self.rows, self.cols, k, s, self.t, self.block) for s, k in enumerate(kinds)], kinds)

    def step_masks(self, masks, kinds=None):
        st = Step(self.t, kinds or ["given"] * self.n, [], [], [], [], [], [], [])
        for s, M in enumerate(masks):
            first = not self.have[s]
            assert not (first and M.any()), "a first frame is the background"
            scene = self.background.copy()
            scene[M] = np.asarray(self.step_value, np.uint8) + np.uint8(BG)
            if self.patterns is not None:
                frame = R.mosaic(scene, self.patterns[s])
                seen = R.demosaic(frame, self.patterns[s])
            else:
                frame = seen = scene
            bits, bg, acc, d = self.m[s].front(seen)
            _, sub, thr, morph = self.o[s].step(seen)
            assert (d == sub).all() and ((thr > 0) == bits).all(), ("model and oracle disagree", self.t, s)
            final = L.frame_zeroed(morph).astype(bool)
            self.have[s] = True
            st.frames.append(frame)
            st.intended.append(M if self.exact and st.kinds[s] != "noise" else None)
            st.final.append(final)
            st.want.append(O.sift_contours(morph, *self.area))
            st.path.append(load_of(final)["path"])
            st.first.append(first)
            st.state.append((bg, acc))
        self.t += 1
        return st


# ------------------------------------------------------------------------------------------------- the shared cases ----

def _noise(kinds):
    return [[NOISE_OF[k] for k in ks] for ks in kinds]


@functools.lru_cache(maxsize=None)
def diff_standard(rows, cols, channels, n, blur=0, n_frames=N_STANDARD):
    run = DiffRun(rows, cols, channels, n, blur)
    return [run.step(ks) for ks in standard(n, n_frames)]


@functools.lru_cache(maxsize=None)
def bsub_standard(rows, cols, channels, n, alpha=0.0, n_frames=N_STANDARD):
    """alpha 0: exact, the background preset.  alpha > 0: the noise form; frame 0 is the background."""
    run = BsubRun(rows, cols, channels, n, alpha, preset=alpha == 0)
    kinds = standard(n, n_frames)
    return run, [run.step(ks) for ks in (kinds if alpha == 0 else _noise(kinds))]


RAW_PATTERNS = (R.RGGB, R.GRBG, R.BGGR)
RAW_FRAMES = 9


@functools.lru_cache(maxsize=None)
def diff_raw():
    """The noise form behind a demosaic: frame 0 is every stream's first frame (an unpaired launch), the rest are paired."""
    run = DiffRun(*SHAPES[0], 3, 3, blur=2, patterns=RAW_PATTERNS, block=4)
    return run, [run.step(ks) for ks in _noise(standard(3, RAW_FRAMES))]


@functools.lru_cache(maxsize=None)
def bsub_raw():
    run = BsubRun(*SHAPES[0], 3, 3, alpha=0.05, preset=False, patterns=RAW_PATTERNS, block=4)
    return run, [run.step(ks) for ks in _noise(standard(3, RAW_FRAMES))]


RESET_FRONT = dict(before=2, reset=1, n_frames=6)


@functools.lru_cache(maxsize=None)
def diff_reset_in_front(channels=3):
    """Two steps, stream 1 reset, a 6-frame sequence: its first launch is unpaired (stream 1 has no last image), two runs of
    the back half; the next launches are paired."""
    run = DiffRun(*SHAPES[0], channels, 3)
    kinds = standard(3, RESET_FRONT["before"] + RESET_FRONT["n_frames"])
    out = []
    for t, ks in enumerate(kinds):
        if t == RESET_FRONT["before"]:
            run.reset(RESET_FRONT["reset"])
        out.append(run.step(ks))
    return out


@functools.lru_cache(maxsize=None)
def bsub_reset_in_front(channels=3):
    run = BsubRun(*SHAPES[0], channels, 3)
    kinds = standard(3, RESET_FRONT["before"] + RESET_FRONT["n_frames"])
    out = []
    for t, ks in enumerate(kinds):
        if t == RESET_FRONT["before"]:
            run.reset(RESET_FRONT["reset"])
        out.append(run.step(ks))
    return run, out


# streams reset before each step after the first: diff_back issues one launch per run of streams in the same state
MIXED = {3: [(), (1,), (0, 2), (2,), (0,), (0, 1)],
         5: [(), (1, 2, 3), (0, 2), (4,), (1,), (0, 3)]}


def launches(first):
    """[(first_stream, n_streams)] of diff_back for a frame set's first-frame flags"""
    out, s0 = [], 0
    while s0 < len(first):
        s1 = s0 + 1
        while s1 < len(first) and first[s1] == first[s0]:
            s1 += 1
        out.append((s0, s1 - s0))
        s0 = s1
    return out


@functools.lru_cache(maxsize=None)
def diff_mixed(n, blur, channels=3):
    """-> [(streams reset before the step, Step)]: busy masks on every stream, the first-frame state mixed"""
    run = DiffRun(*MANY, channels, n, blur)
    out = []
    for t, resets in enumerate(MIXED[n]):
        for s in resets:
            run.reset(s)
        out.append((resets, run.step([("runs_over", "roots_over")[(s + t) % 2] for s in range(n)])))
    return out


N_MANY = 66
MANY_BUSY = (0, 63, 64, 65)
MANY_AT = (1, 62)
MANY_FRAMES = 7                          # one synchronous step and a 6-frame sequence


def many_kinds(t):
    ks = ["rect"] * N_MANY
    for i, s in enumerate(MANY_BUSY):
        ks[s] = ("runs_over", "roots_over")[(i + t) % 2]
    for i, s in enumerate(MANY_AT):
        ks[s] = ("runs_at", "roots_at")[(i + t) % 2]
    return ks


@functools.lru_cache(maxsize=None)
def diff_many():
    run = DiffRun(*MANY, 3, N_MANY)
    return [run.step(many_kinds(t)) for t in range(MANY_FRAMES)]


@functools.lru_cache(maxsize=None)
def bsub_many():
    run = BsubRun(*MANY, 3, N_MANY)
    return run, [run.step(many_kinds(t)) for t in range(MANY_FRAMES)]


# ---- ties and the area window over capacity: blob_load.edge_cases() masks through one step of each tracker

def _edge_mask(name):
    H, W, ero, dil, build, exp = L.edge_cases()[name]
    assert ero == 0 and dil == 0 and exp["path"] == "global"
    return build() != 0


@functools.lru_cache(maxsize=None)
def area_cases():
    """{name: (mask, area window)}: hundreds of equal areas over the root capacity (the tie goes to the later first pixel), and
    the one real blob of roots_769 shut out by max_area -- equal to its area (the comparison is strict) and just under it"""
    ties, roots = _edge_mask("ties_bands_769"), _edge_mask("roots_769")
    a = largest(roots)["area"]
    assert a > 1
    return {"ties": (ties, AREA), "max_area_equal": (roots, (0.0, a)), "max_area_under": (roots, (0.0, a - 0.5)),
            "min_area_equal": (roots, (a, DBL_MAX))}


@functools.lru_cache(maxsize=None)
def diff_area(name, channels):
    mask, area = area_cases()[name]
    return DiffRun(*mask.shape, channels, 1, area=area).step_masks([mask])


@functools.lru_cache(maxsize=None)
def bsub_area(name, channels):
    mask, area = area_cases()[name]
    run = BsubRun(*mask.shape, channels, 1, area=area)
    return run, run.step_masks([mask])


# ---- one context, every user of scratch set 0

SHARED_SHAPE, SHARED_N = SHAPES[0], 3
# (call, kinds): the fused tracker, the single-stage detectors and the two batched trackers in turn, busy beside quiet
SHARED_OPS = [("track", ("empty", "empty", "empty")),                 # the fused tracker's background
              ("track", ("runs_over", "roots_over", "runs_at")),
              ("diff", ("rect", "empty", "roots_at")),
              ("detect_thresh", ("roots_over", None, None)),
              ("detect_hsv", (None, "runs_over", None)),
              ("bsub", ("roots_over", "runs_over", "roots_over")),
              ("track", ("rect", "roots_at", "empty")),
              ("diff", ("runs_over", "roots_over", "runs_over")),
              ("bsub", ("runs_at", "rect", "empty")),
              ("diff", ("roots_over", "runs_at", "roots_over"))]
ORDINARY = ("track", "detect_thresh", "detect_hsv")


def shared_masks():
    """[op index][stream] -> intended mask or None"""
    H, W = SHARED_SHAPE
    return [[None if k is None else mask_of(H, W, k, s, i) for s, k in enumerate(ks)] for i, (_, ks) in enumerate(SHARED_OPS)]


@functools.lru_cache(maxsize=None)
def shared_steps():
    """-> (BsubRun, {op index: Step}) of the two batched trackers' calls in SHARED_OPS"""
    H, W = SHARED_SHAPE
    dr, br = DiffRun(H, W, 3, SHARED_N), BsubRun(H, W, 3, SHARED_N)
    masks, out = shared_masks(), {}
    for i, (op, ks) in enumerate(SHARED_OPS):
        if op in ("diff", "bsub"):
            out[i] = (dr if op == "diff" else br).step_masks(masks[i], list(ks))
    return br, out
