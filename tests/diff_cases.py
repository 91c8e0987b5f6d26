"""Shared, seeded cases of the motion tracker (`framefilt col -C GREY` -> `posidet diff`, oatgpu_diff_*) and a numpy model of
its front end (TEST INFRASTRUCTURE: tests/test_diff_tracker_cpu.py checks the model and the cases against the oracle without
a GPU, tests/test_diff_tracker_gpu.py feeds the same cases to the kernels).

A case: rows, cols, channels, n_streams, diff_threshold, blur, roi (None or a (rows, cols) uint8 plane for stream `roi_stream`)
and frames[t][s].  A frame is a static background with noise of amplitude at most a third of the threshold, a bright rectangle
that moves a few pixels a frame -- except on the STILL frames, where it stays and the difference must be empty -- and, on some
frames, activity on the image border (where blur and dilation differ and findContours zeroes the ring)."""
from dataclasses import dataclass, field

import numpy as np

import oracle_lib as O

AREA = (2.0, 1e6)
STILL = (4, 9)          # frames on which the rectangle does not move (t > 0)
BORDER = (6, 10)        # frames with border activity


@dataclass
class Case:
    name: str
    rows: int
    cols: int
    channels: int
    n_streams: int
    diff_threshold: int
    blur: int
    roi: np.ndarray = None
    roi_stream: int = 0
    roi_frames: tuple = ()                         # the frames on which the ROI is in force (set and removed in between)
    frames: list = field(default_factory=list)     # [t][s]

    def roi_at(self, t, s):
        return self.roi if self.roi is not None and s == self.roi_stream and t in self.roi_frames else None


def _steps(t):
    return sum(0 if k in STILL else 1 for k in range(1, t + 1))


def _grey_px(v, channels):
    return (v, v, v) if channels == 3 else v       # grey(v, v, v) = (16384 v + 8192) >> 14 = v


def _frame(rng, base, rows, cols, channels, thr, amp, t, s):
    noise = rng.integers(-amp, amp + 1, base.shape) if amp else 0
    f = np.clip(base + noise, 0, 255).astype(np.uint8)
    rh, rw = max(2, min(12, rows // 3)), max(2, min(20, cols // 3))
    step = _steps(t)
    x = (2 + 5 * step + 7 * s) % max(1, cols - rw)
    y = (3 + 2 * step) % max(1, rows - rh)
    f[y:y + rh, x:x + rw] = 255 if thr >= 128 else (90, 250, 130) if channels == 3 else 220
    if t in BORDER:
        f[0:2, :] = 255
        f[:, 0:2] = 255
    if cols >= 16:
        # planted pixels, drawn last; they change with the rectangle's step, so a still frame stays still
        r, c, even = rows // 2, cols // 2, step % 2 == 0
        f[r, c - 4] = 0                                              # A: an exact zero (the first frame's `!= 0`; its blur)
        f[r, c - 2] = _grey_px(thr if even else 0, channels)         # B: |difference| == thr exactly; on frame 0: 0 < g <= thr
        if channels == 3:
            v = min(thr + 1, 255)                                    # D: grey = thr + 1 with the + 8192, thr without
            f[r, c] = (v - 1, v, v) if even else (0, 0, 0)
            red = min(255, -(-((thr + 1) * 16384 - 8192) // 4899))   # E: red of grey thr + 1; as blue it weighs 1868 / 4899 of that
            f[r, c + 2] = (0, 0, red) if even else (0, 0, 0)
    return f


def make_case(name, rows, cols, channels, n_streams, diff_threshold=12, blur=2, roi=False, n_frames=12, seed=0):
    rng = np.random.default_rng(seed * 1000 + rows * 7 + cols + channels + diff_threshold)
    shape = (rows, cols, 3) if channels == 3 else (rows, cols)
    amp = min(diff_threshold, 255 - diff_threshold) // 3
    c = Case(name, rows, cols, channels, n_streams, diff_threshold, blur)
    # thresholds of 128 and more: only black against white can exceed them
    bases = [(np.zeros(shape, np.int16) if diff_threshold >= 128 else rng.integers(40, 90, shape).astype(np.int16))
             for _ in range(n_streams)]
    if roi:
        m = np.zeros((rows, cols), np.uint8)
        m[rows // 6:, : max(1, (3 * cols) // 4)] = 255
        c.roi, c.roi_stream, c.roi_frames = m, min(1, n_streams - 1), (0, 1, 2, 3, 4, 5, 8, 9)
    for t in range(n_frames):
        c.frames.append([_frame(rng, bases[s], rows, cols, channels, diff_threshold, amp, t, s) for s in range(n_streams)])
    return c


# where the kernel can go wrong: narrow instantiation with Wp > W and P no multiple of 256; wide with whole lanes beyond W;
# wide with Wp == W and a tail wave; one word a row; one lane a row
GEOMETRIES = [(37, 91), (90, 200), (33, 128), (48, 64), (5, 4)]


def cpu_cases():
    """The cases the CPU file checks the model on (and the GPU file runs): every geometry, both colours, the parameter corners."""
    out = []
    for i, (r, c) in enumerate(GEOMETRIES):
        for ch in (3, 1):
            out.append(make_case(f"{r}x{c}-ch{ch}", r, c, ch, 1, seed=i))
    for thr in (0, 12, 254, 255):
        out.append(make_case(f"thr{thr}", 37, 91, 3, 1, diff_threshold=thr, seed=20 + thr))
    for blur in (0, 2, 5, 22):
        out.append(make_case(f"blur{blur}", 90, 200, 1, 1, blur=blur, seed=40 + blur))
    out.append(make_case("roi-bgr", 90, 200, 3, 3, roi=True, seed=60))
    out.append(make_case("roi-grey", 37, 91, 1, 3, roi=True, seed=61))
    return out


# ------------------------------------------------------------------ the numpy model of the front end and the detector ----

def grey_of(frame, bias=8192, wb=1868, wg=9617, wr=4899):
    if frame.ndim == 2:
        return frame.copy()
    f = frame.astype(np.int64)
    return ((wb * f[..., 0] + wg * f[..., 1] + wr * f[..., 2] + bias) >> 14).astype(np.uint8)


class Model:
    """One stream of the tracker as the kernel computes it: g = grey(frame), g = 0 outside the ROI, bits = have ? |g - last| >
    thr : g != 0, last = g; then the blur-as-dilation (not on a first frame) and siftContours.  `wrong` plants one of the wrong
    front ends the cases must tell apart."""

    def __init__(self, thr, blur, area=AREA, wrong=None):
        self.thr, self.blur, self.area, self.wrong = thr, blur, area, wrong
        self.last = None

    def front(self, frame, roi=None):
        w = self.wrong
        g = grey_of(frame, bias=0) if w == "no_bias" else grey_of(frame, wb=4899, wr=1868) if w == "swap_rb" else grey_of(frame)
        if roi is not None and w != "roi_on_diff":
            g = np.where(roi != 0, g, 0).astype(np.uint8)
        first = self.last is None
        if first:
            bits = g.astype(np.int32) > self.thr if w == "first_gt" else g != 0
        else:
            d = g.astype(np.int32) - self.last.astype(np.int32)
            if w != "signed":
                d = np.abs(d)
            bits = d >= self.thr if w == "ge" else d > self.thr
        if roi is not None and w == "roi_on_diff":
            bits = bits & (roi != 0)
        self.last = np.zeros_like(g) if first and w == "stale_last" else g
        return bits, first

    def detect(self, frame, roi=None):
        """-> (detection dict, threshold bits, mask after the blur as the oracle's `thr > 0`)"""
        bits, first = self.front(frame, roi)
        img = np.where(bits, 255, 0).astype(np.uint8)
        if self.blur > 0 and (not first or self.wrong == "blur_first"):
            img = O.blur(img, self.blur)
        return O.sift_contours(img, *self.area), bits, img > 0


WRONG = ["ge", "signed", "no_bias", "swap_rb", "first_gt", "stale_last", "roi_on_diff", "blur_first"]


def oracle_frame(frame, roi=None):
    """What the reference chain hands `posidet diff`: framefilt mask (where a ROI is set) -> col GREY."""
    f = frame
    if roi is not None:
        f = frame.copy()
        f[roi == 0] = 0
    return O.bgr2grey(f) if f.ndim == 3 else f


def same_dict(a, b):
    keys = ("valid", "area", "a00", "a10", "a01", "first_pixel", "x", "y")
    return a["valid"] == b["valid"] and (not a["valid"] or all(a[k] == b[k] for k in keys))
