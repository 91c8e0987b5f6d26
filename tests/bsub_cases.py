"""Shared, seeded cases of the subtraction tracker (`framefilt bsub` -> `col -C HSV` -> `posidet hsv`, GREY: bsub -> `posidet
thresh`; oatgpu_bsub_track_*) and a numpy model of its front end (TEST INFRASTRUCTURE: tests/test_bsub_tracker_cpu.py checks the
model and the cases against the oracle without a GPU, tests/test_bsub_tracker_gpu.py feeds the same cases to the kernels).

A case: rows, cols, channels, n_streams, alpha, erode, dilate, a ROI on one stream for some of the frames, a background "from a
file" for some streams, and frames[t][s].  A frame is a static background with noise and a coloured rectangle that moves; the
rectangle's colour MINUS the background lies inside the window, the rectangle's own HSV does not.  Frames wider than 15 pixels
carry planted pixels (PLANTS_*): their value on a stream's frame 0 makes the background, their value afterwards the difference
-- exactly so at alpha 0.

What stands behind what: the oracle (oracle_lib.Bsub) hands out the subtracted image only, so the CPU file holds the model to it
through that image and the window bits.  The background BYTES are thereby pinned wherever the frame exceeds them; the fp32
ACCUMULATOR is not visible in the oracle at all.  The reference for `acc` in the GPU tests is this numpy model alone: written
independently of the kernel, from the reference's source (accW_ in float, two products and a sum, each rounded)."""
from dataclasses import dataclass, field

import numpy as np

import oracle_lib as O
from diff_cases import GEOMETRIES, same_dict  # noqa: F401  (the motion tracker's five geometries)

AREA = (2.0, 1e6)
HSV_WIN = dict(h=(35, 65), s=(205, 250), v=(120, 240))      # on the DIFFERENCE image; cv::inRange's bounds are inclusive
GREY_WIN = (100, 200)
# the rectangle over a background of B 36..54, G and R 36..94: the difference has V = 156..214, S = 216..248, H = 42..60 (inside the
# window); the rectangle's own HSV has S = 194 (outside)
RECT_BGR, RECT_GREY = (60, 250, 120), 220
ALPHAS = (0.0, 0.01, 0.05, 0.5, 1.0)
MORPHS = ((0, 0), (3, 7), (0, 10))                           # erode / dilate; 0 / 10 is the reference's default
N_FRAMES = 8


def _inside(hsv):
    h, s, v = (hsv[..., i].astype(int) for i in range(3))
    w = HSV_WIN
    return (h >= w["h"][0]) & (h <= w["h"][1]) & (s >= w["s"][0]) & (s <= min(w["s"][1], 255)) & (v >= w["v"][0]) & (v <= w["v"][1])


def _edge_triples():
    """Difference triples (b, g, r) exactly on each edge of the H, S and V window and one step outside it."""
    cand = np.array([(b, g, r) for g in range(119, 242) for b in range(0, 41) for r in range(0, g + 1, 2)], np.uint8)
    hsv = O.bgr2hsv(cand.reshape(1, -1, 3)).reshape(-1, 3).astype(int)
    w = HSV_WIN
    mid = dict(h=(40, 60), s=(215, 245), v=(130, 230))

    def pick(ch, value):
        ok = np.ones(len(cand), bool)
        for i, k in enumerate("hsv"):
            ok &= (hsv[:, i] == value) if k == ch else (hsv[:, i] >= mid[k][0]) & (hsv[:, i] <= mid[k][1])
        assert ok.any(), (ch, value)
        return tuple(int(x) for x in cand[np.argmax(ok)])

    out = []
    for ch in "hsv":
        lo, hi = w[ch]
        out += [(pick(ch, lo), True), (pick(ch, lo - 1), False), (pick(ch, hi), True), (pick(ch, hi + 1), False)]
    return out


EDGES_BGR = _edge_triples()
INSIDE_BGR = EDGES_BGR[0][0]
# (value on frame 0, value on every later frame): x == bg; x == bg + 1; x < bg by an amount inside the window (saturates to 0;
# an absolute difference would be inside); the half-way accumulators of alpha 0.5 in both parities (10.5 -> 10, 11.5 -> 12);
# then a difference exactly on each edge of the window and one step outside
PLANTS_BGR = ([((50,) * 3, (50,) * 3), ((50,) * 3, (51,) * 3), (tuple(10 + x for x in INSIDE_BGR), (10,) * 3),
               ((10,) * 3, (11,) * 3), ((11,) * 3, (12,) * 3)]
              + [((10,) * 3, tuple(10 + x for x in t)) for t, _ in EDGES_BGR])
PLANTS_GREY = [(50, 50), (50, 51), (230, 60), (10, 11), (11, 12), (10, 10 + GREY_WIN[0]), (10, 9 + GREY_WIN[0]),
               (10, 10 + GREY_WIN[1]), (10, 11 + GREY_WIN[1])]


@dataclass
class Case:
    name: str
    rows: int
    cols: int
    channels: int
    n_streams: int
    alpha: float
    erode: int
    dilate: int
    roi: np.ndarray = None
    roi_stream: int = 0
    roi_frames: tuple = ()                         # the frames on which the ROI is in force (set and removed in between)
    background: dict = field(default_factory=dict)  # stream -> background image "from a file" (alpha must be 0)
    frames: list = field(default_factory=list)     # [t][s]

    def roi_at(self, t, s):
        return self.roi if self.roi is not None and s == self.roi_stream and t in self.roi_frames else None

    @property
    def shape(self):
        return (self.rows, self.cols, 3) if self.channels == 3 else (self.rows, self.cols)

    def tracker_args(self):
        kw = dict(n_streams=self.n_streams, channels=self.channels, alpha=self.alpha, erode=self.erode, dilate=self.dilate, area=AREA)
        if self.channels == 3:
            kw.update(h_thresh=HSV_WIN["h"], s_thresh=HSV_WIN["s"], v_thresh=HSV_WIN["v"])
        else:
            kw.update(thresh=GREY_WIN)
        return kw


def plant_positions(rows, cols, count):
    r, per_row = rows // 2, (cols - 4) // 2
    return [(r + 2 * (i // per_row), 2 + 2 * (i % per_row)) for i in range(count)]


def _frame(rng, base, rows, cols, channels, t, s):
    f = np.clip(base + rng.integers(-4, 5, base.shape), 0, 255).astype(np.uint8)
    rh, rw = max(2, min(12, rows // 3)), max(2, min(20, cols // 3))
    x = (2 + 5 * t + 7 * s) % max(1, cols - rw)
    y = (3 + 2 * t) % max(1, rows - rh)
    f[y:y + rh, x:x + rw] = RECT_BGR if channels == 3 else RECT_GREY
    if cols >= 16:
        plants = PLANTS_BGR if channels == 3 else PLANTS_GREY
        for (r, c), (v0, v1) in zip(plant_positions(rows, cols, len(plants)), plants):
            f[r, c] = v0 if t == 0 else v1
    return f


def make_case(name, rows, cols, channels, n_streams, alpha=0.05, erode=0, dilate=10, roi=False, background=False,
              n_frames=N_FRAMES, seed=0):
    rng = np.random.default_rng(seed * 1000 + rows * 7 + cols + channels)
    shape = (rows, cols, 3) if channels == 3 else (rows, cols)
    c = Case(name, rows, cols, channels, n_streams, float(alpha), erode, dilate)
    bases = [rng.integers(40, 91, shape).astype(np.int16) for _ in range(n_streams)]
    if channels == 3:                              # a narrow blue channel keeps the rectangle's difference below S = 255
        for b in bases:
            b[..., 0] = rng.integers(40, 51, b.shape[:2])
    if roi:
        m = np.zeros((rows, cols), np.uint8)
        m[rows // 6:, : max(1, (3 * cols) // 4)] = 255
        c.roi, c.roi_stream, c.roi_frames = m, min(1, n_streams - 1), (0, 1, 2, 5, 6)
    if background:                                 # the noiseless scene, for every second stream
        assert alpha == 0
        c.background = {s: bases[s].astype(np.uint8) for s in range(0, n_streams, 2)}
    for t in range(n_frames):
        c.frames.append([_frame(rng, bases[s], rows, cols, channels, t, s) for s in range(n_streams)])
    return c


def cpu_cases():
    """The cases the CPU file checks the model on (and the GPU file runs): every geometry in both colours, the parameter
    corners, the ROI on one of three streams, the background from a file."""
    out = []
    for i, (r, c) in enumerate(GEOMETRIES):
        for ch in (3, 1):
            out.append(make_case(f"{r}x{c}-ch{ch}", r, c, ch, 1, seed=i))
    for a in ALPHAS:
        out.append(make_case(f"alpha{a}-bgr", 37, 91, 3, 1, alpha=a, seed=20))
        out.append(make_case(f"alpha{a}-grey", 33, 128, 1, 1, alpha=a, seed=21))
    for e, d in MORPHS:
        out.append(make_case(f"morph{e}-{d}", 90, 200, 3, 1, alpha=0.0, erode=e, dilate=d, seed=40))
    out.append(make_case("roi-bgr", 90, 200, 3, 3, roi=True, seed=60))
    out.append(make_case("roi-grey", 37, 91, 1, 3, alpha=0.0, roi=True, seed=61))
    out.append(make_case("file-bgr", 48, 64, 3, 3, alpha=0.0, background=True, seed=70))
    out.append(make_case("file-grey", 90, 200, 1, 2, alpha=0.0, background=True, seed=71))
    return out


# ----------------------------------------------------------------------------- the numpy model of one stream's front end ----

WRONG = ["abs_diff", "half_up", "acc_on_bg", "sub_before", "roi_on_diff", "window_on_frame", "first_not_acc", "fused"]


def window_bits(img):
    """The context's window on an image of differences (HSV by the oracle's cvtColor: the model is about bsub)."""
    if img.ndim == 3:
        return _inside(O.bgr2hsv(img))
    return (img >= GREY_WIN[0]) & (img <= GREY_WIN[1])


class Model:
    """One stream of the front end as the kernel computes it, in float32 arrays with one numpy operation per rounding: x = frame
    (0 outside the ROI); first frame: acc = x, bg = x; alpha > 0: acc = x * a + acc * b, bg = saturate(rint(acc)); d = x > bg ?
    x - bg : 0; bits = window(d).  `wrong` plants one of the wrong front ends the cases must tell apart."""

    def __init__(self, alpha, wrong=None):
        self.alpha, self.wrong = float(alpha), wrong
        self.bg = self.acc = None

    def set_background(self, image):
        self.bg, self.acc = np.array(image, np.uint8), None

    def reset(self):
        self.bg = self.acc = None

    def front(self, frame, roi=None):
        """-> (bits, bg, acc, d): the window bits, the state behind the frame (acc None for a background from a file), the
        subtracted image"""
        w = self.wrong
        x = frame.copy()
        if roi is not None and w != "roi_on_diff":
            x[roi == 0] = 0
        first = self.bg is None
        if first:
            self.acc, self.bg = x.astype(np.float32), x.copy()
        before = self.bg
        if self.alpha > 0 and not (first and w == "first_not_acc"):
            a = np.float32(self.alpha)
            b = np.float32(1) - a
            old = self.bg.astype(np.float32) if w == "acc_on_bg" else self.acc
            if w == "fused":                                    # one rounding: the product is exact in float64
                acc = (x.astype(np.float64) * np.float64(a) + old.astype(np.float64) * np.float64(b)).astype(np.float32)
            else:
                xa = x.astype(np.float32) * a
                ob = old * b
                acc = xa + ob
            r = np.floor(acc + np.float32(0.5)) if w == "half_up" else np.rint(acc)
            self.acc, self.bg = acc, np.clip(r, 0, 255).astype(np.uint8)
        bg = before if w == "sub_before" else self.bg
        xi, bi = x.astype(np.int16), bg.astype(np.int16)
        d = (np.abs(xi - bi) if w == "abs_diff" else np.where(xi > bi, xi - bi, 0)).astype(np.uint8)
        bits = window_bits(x if w == "window_on_frame" else d)
        if roi is not None and w == "roi_on_diff":
            bits = bits & (roi != 0)
        return bits, self.bg.copy(), None if self.acc is None else self.acc.copy(), d


# -------------------------------------------------------------------------------------------------- the oracle chain ----

class Oracle:
    """One stream of the reference chain: framefilt mask -> framefilt bsub -> (col -C HSV) -> inRange -> erode -> dilate ->
    siftContours.  A background from a file is what oracle_lib.Bsub takes as its first frame at alpha 0."""

    def __init__(self, c, background=None):
        self.c, self.background = c, background
        self.reset(background)

    def reset(self, background=None):
        c = self.c
        self.b = O.Bsub(c.rows, c.cols, c.channels, c.alpha)
        if background is not None:
            assert c.alpha == 0
            self.b.filter(background)

    def step(self, frame, roi=None):
        """-> (detection, subtracted image, threshold image, image after erode / dilate)"""
        c = self.c
        f = frame
        if roi is not None:
            f = frame.copy()
            f[roi == 0] = 0
        sub = self.b.filter(f)
        w = HSV_WIN
        thr = (O.inrange3(O.bgr2hsv(sub), [w["h"][0], w["s"][0], w["v"][0]], [w["h"][1], w["s"][1], w["v"][1]]) if c.channels == 3
               else O.inrange1(sub, *GREY_WIN))
        m = thr
        if c.erode > 0:
            m = O.erode(m, c.erode)
        if c.dilate > 0:
            m = O.dilate(m, c.dilate)
        return O.sift_contours(m, *AREA), sub, thr, m


class Ref:
    """One stream: the oracle chain with the model beside it.  step -> (detection, bits, morph > 0, bg, acc)."""

    def __init__(self, c, s=0):
        self.c, self.s = c, s
        self.m = Model(c.alpha)
        bgd = c.background.get(s)
        self.o = Oracle(c, bgd)
        if bgd is not None:
            self.m.set_background(bgd)

    def reset(self):
        self.m.reset()
        self.o.reset()

    def step(self, frame, roi=None):
        bits, bg, acc, d = self.m.front(frame, roi)
        det, sub, thr, morph = self.o.step(frame, roi)
        assert (d == sub).all() and ((thr > 0) == bits).all()
        return det, bits, morph > 0, bg, acc
