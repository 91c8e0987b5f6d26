"""Shared, seeded cases of multi-target detection (oatgpu_set_targets / oatgpu_targets) and the reference ranking
(TEST INFRASTRUCTURE: tests/test_targets_cpu.py checks the cases and the reference without a GPU, tests/test_targets_gpu.py and
tests/test_targets_host_gpu.py feed the same cases to the kernels).

The reference for every rank comes from the oracle alone: oracle_lib.find_contours on the oracle's own mask after erode / dilate
(thr_out), never from a device tap.  Candidates are the external contours with m00 > 0 inside the area window; they are ranked by
(m00, first pixel in raster order), descending -- rank 0 is what oat::siftContours picks.

Planted masks go through the single-stage detectors (value 255 under a window on 255); frame sequences go through the three
trackers: several blocks that move (motion), blocks that appear over a fixed background (subtraction), blocks over an aged model
(fused)."""
import functools

import numpy as np

import oracle_lib as O

KS = (1, 3, 8)                      # the K the planted masks are ranked with
TRACKER_K = 3                       # ... and the trackers' sequences
MORPHS = ((0, 0), (3, 5))           # erode / dilate of the planted masks
BIG = 1e6
INVALID = dict(valid=False, area=0.0, a00=0, a10=0, a01=0, first_pixel=-1, x=0.0, y=0.0)


# ------------------------------------------------------------------------------------------------ the reference ranking ----

def contour_dict(c, cols):
    """A contour of oracle_lib.find_contours with the keys of diff_cases.same_dict, as oat_sift_contours fills them."""
    return dict(valid=True, area=c["m00"], a00=int(c["a00"]), a10=int(c["a10"]), a01=int(c["a01"]),
                first_pixel=c["start"][1] * cols + c["start"][0], x=c["m10"] / c["m00"], y=c["m01"] / c["m00"])


def candidates(mask, area):
    """The external contours siftContours considers, in OpenCV's list order."""
    return [c for c in O.find_contours(mask) if c["m00"] > 0 and area[0] <= c["m00"] < area[1]]


def _key(c, cols):
    return (c["m00"], c["start"][1] * cols + c["start"][0])


def reference(mask, area, k):
    """-> (the k ranks as dicts, invalid where fewer candidates exist; n_found)"""
    cols = mask.shape[1]
    cs = sorted(candidates(mask, area), key=lambda c: _key(c, cols), reverse=True)
    ranks = [contour_dict(c, cols) for c in cs[:k]]
    return ranks + [dict(INVALID) for _ in range(k - len(ranks))], len(cs)


# ---- planted wrong rankers: each must differ from the reference on at least one case (tests/test_targets_cpu.py) ----

def components(mask):
    """8-connected foreground components of the mask inside the zeroed one-pixel frame: [(first pixel, [pixels])], raster order."""
    rows, cols = mask.shape
    fg = np.zeros((rows, cols), bool)
    if rows > 2 and cols > 2:
        fg[1:-1, 1:-1] = mask[1:-1, 1:-1] != 0
    seen = np.zeros_like(fg)
    out = []
    for y, x in zip(*np.nonzero(fg)):
        if seen[y, x]:
            continue
        seen[y, x] = True
        stack, px = [(int(y), int(x))], []
        while stack:
            cy, cx = stack.pop()
            px.append((cy, cx))
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    ny, nx = cy + dy, cx + dx
                    if fg[ny, nx] and not seen[ny, nx]:
                        seen[ny, nx] = True
                        stack.append((ny, nx))
        out.append((int(y) * cols + int(x), px))
    return out


WRONG = ["ties_earlier", "ascending", "window_after_cut", "pixel_area", "holes_admitted", "zero_area_admitted"]


def wrong_ranking(mask, area, k, wrong):
    """The reference with one rule replaced; same return value."""
    cols = mask.shape[1]
    every = O.find_contours(mask)
    inside = lambda a: area[0] <= a < area[1]      # noqa: E731
    measure = lambda c: c["m00"]                   # noqa: E731
    if wrong == "holes_admitted":
        comps = components(mask)
        if len(comps) > 200:                       # (the dots: no holes there)
            return reference(mask, area, k)
        every = []
        for _, px in comps:
            alone = np.zeros_like(mask)
            for y, x in px:
                alone[y, x] = 255
            every += O.find_contours(alone)
    if wrong == "pixel_area":
        count = {fp: len(px) for fp, px in components(mask)}
        measure = lambda c: float(count[c["start"][1] * cols + c["start"][0]])      # noqa: E731
    cs = [c for c in every if c["m00"] > 0 or wrong == "zero_area_admitted"]
    if wrong != "window_after_cut":
        cs = [c for c in cs if inside(measure(c))]
    n_found = len(cs)
    if wrong == "ascending":
        cs.sort(key=lambda c: (measure(c), c["start"][1] * cols + c["start"][0]))
    elif wrong == "ties_earlier":
        cs.sort(key=lambda c: (-measure(c), c["start"][1] * cols + c["start"][0]))
    else:
        cs.sort(key=lambda c: (measure(c), c["start"][1] * cols + c["start"][0]), reverse=True)
    cs = cs[:k]
    if wrong == "window_after_cut":
        cs = [c for c in cs if inside(measure(c))]
    ranks = [contour_dict(c, cols) if c["m00"] > 0 else dict(INVALID, valid=True, first_pixel=c["start"][1] * cols + c["start"][0])
             for c in cs]
    return ranks + [dict(INVALID) for _ in range(k - len(ranks))], n_found


def same_ranking(a, b):
    from diff_cases import same_dict
    return a[1] == b[1] and len(a[0]) == len(b[0]) and all(same_dict(x, y) for x, y in zip(a[0], b[0]))


# --------------------------------------------------------------------------------------------------------- planted masks ----

class Planted:
    def __init__(self, name, img, area=(0.5, BIG)):
        self.name, self.img, self.area = name, img, area
        self.rows, self.cols = img.shape

    def __repr__(self):
        return self.name


def _squares(rows, cols, sides, cell, origin=(2, 2)):
    """Squares of the given sides on a grid of `cell`-pixel cells, row by row."""
    img = np.zeros((rows, cols), np.uint8)
    per_row = (cols - origin[1]) // cell
    for i, s in enumerate(sides):
        y, x = origin[0] + cell * (i // per_row), origin[1] + cell * (i % per_row)
        assert y + s < rows and x + s < cols, (rows, cols, i)
        img[y:y + s, x:x + s] = 255
    return img


def planted_cases():
    out = []
    # equal areas at the K / K + 1 boundary of K = 1, 3 and 8: contour areas 25 25 16 16 9 9 9 4 4 1 (with 3 / 5: sides + 2)
    out.append(Planted("ties-48x64", _squares(48, 64, (3, 6, 4, 5, 2, 6, 4, 3, 5, 4), 10)))
    # an odd geometry (Wp > W, P no multiple of 256), blobs touching the frame on every side
    img = _squares(37, 61, (5, 3, 7, 4, 6, 3), 9, origin=(12, 4))
    img[0:5, 0:7] = 255
    img[0:3, 30:38] = 255
    img[33:37, 50:61] = 255
    img[14:22, 58:61] = 255
    img[30:37, 0:2] = 255
    out.append(Planted("frame-37x61", img))
    # three mask words a row: blobs across columns 63 / 64 and 127 / 128
    img = np.zeros((20, 130), np.uint8)
    img[3:9, 60:68] = 255
    img[11:17, 124:129] = 255
    img[12:16, 62:66] = 255
    img[2:6, 100:104] = 255
    img[4:8, 10:18] = 255
    out.append(Planted("words-20x130", img))
    # nothing survives the frame zeroing
    out.append(Planted("tiny-3x3", np.full((3, 3), 255, np.uint8)))
    out.append(Planted("tiny-2x9", np.full((2, 9), 255, np.uint8)))
    # ~1300 candidates of area 1: ranking purely by first pixel, more roots than a workgroup has lanes
    img = np.zeros((96, 130), np.uint8)
    for y in range(1, 93, 3):
        for x in range(1, 127, 3):
            img[y:y + 2, x:x + 2] = 255
    out.append(Planted("dots-96x130", img))
    # a ring with a blob in its hole (not a candidate: inside the ring's external contour), two blobs beside it
    img = np.zeros((48, 64), np.uint8)
    img[6:36, 4:34] = 255
    img[10:32, 8:30] = 0
    img[18:24, 16:22] = 255
    img[8:14, 44:52] = 255
    img[30:34, 42:46] = 255
    out.append(Planted("ring-48x64", img))
    # the area window: contour areas 4 (below), 9 (exactly min_area), 16, 25 (exactly max_area), 36 (above)
    out.append(Planted("window-48x64", _squares(48, 64, (3, 4, 5, 6, 7, 4), 10), area=(9.0, 25.0)))
    # a window from 0: single pixels and one-pixel lines have m00 == 0 and are no candidates
    img = _squares(37, 61, (4, 3), 12, origin=(4, 4))
    img[20, 10] = 255
    img[22, 30:40] = 255
    img[26:33, 50] = 255
    img[30, 5] = 255
    out.append(Planted("zero-37x61", img, area=(0.0, BIG)))
    return out


def thresh_params(case, morph):
    return O.hsv_params(h_lo=255, h_hi=256, erode=morph[0], dilate=morph[1], min_area=case.area[0], max_area=case.area[1])


@functools.lru_cache(maxsize=None)
def _planted_masks():
    """{(name, morph): (oat_detect_thresh's detection, its thr_out)}: computed once, shared, never written to."""
    out = {}
    for c in planted_cases():
        for m in MORPHS:
            det, thr = O.detect_thresh(c.img, thresh_params(c, m))
            thr.setflags(write=False)
            out[(c.name, m)] = (det, thr)
    return out


def planted_mask(case, morph):
    return _planted_masks()[(case.name, morph)]


@functools.lru_cache(maxsize=None)
def planted_reference(name, morph, k):
    case = next(c for c in planted_cases() if c.name == name)
    return reference(planted_mask(case, morph)[1], case.area, k)


# -------------------------------------------------------------------------------------- frame sequences for the trackers ----

GEOMETRIES = ((48, 64), (37, 61))
FAMILIES = ("motion", "subtraction", "fused")
N_FRAMES = 10
AREA = (2.0, BIG)
BLOCK_BGR = (250, 90, 40)                                   # H 113, S 214, V 250
FUSED_WIN = dict(h_thresh=(100, 125), s_thresh=(150, 256), v_thresh=(100, 256))
FUSED_MORPH = (0, 3)
FUSED_LR = 0.01
FUSED_WARM = 3                                              # frames of bare background in front: the model has aged
DIFF = dict(diff_threshold=12, blur=2)
SUB_MORPH = (0, 3)
SUB_ALPHAS = (0.0, 0.05)
# blocks a frame (t = 0 is bare background for every family; the fused tracker sees FUSED_WARM such frames first)
SCHEDULE = (0, 1, 2, 5, 6, 6, 4, 5, 6, 2)
SIZES = ((5, 5), (5, 5), (4, 6), (6, 6), (3, 4), (7, 5))    # (h, w): two of equal area


def sub_window():
    from bsub_cases import HSV_WIN
    return HSV_WIN


def _background(rows, cols, variant):
    rng = np.random.default_rng(4100 + 7 * rows + cols + variant)
    b = rng.integers(40, 91, (rows, cols, 3)).astype(np.uint8)
    b[..., 0] = rng.integers(40, 51, (rows, cols))          # (bsub_cases: a narrow blue channel keeps the difference below S = 255)
    return b


@functools.lru_cache(maxsize=None)
def sequence(family, rows, cols, variant=0):
    """frames[t] (rows, cols, 3) of one camera; variant: which of the three different cameras a stream shows."""
    from bsub_cases import RECT_BGR
    bg = _background(rows, cols, variant)
    colour = RECT_BGR if family == "subtraction" else BLOCK_BGR
    cw, chh = cols // 3, rows // 2
    sched = (0,) * (FUSED_WARM - 1) + SCHEDULE if family == "fused" else SCHEDULE
    frames = []
    for t, nb in enumerate(sched):
        f = bg.copy()
        for i in range(nb):
            j = (i + variant) % len(SIZES)
            h, w = SIZES[j]
            x = (j % 3) * cw + 2 + (3 * t + variant) % (cw - w - 3)
            y = (j // 3) * chh + 2 + (2 * t + i) % (chh - h - 3)
            f[y:y + h, x:x + w] = colour
        f.setflags(write=False)
        frames.append(f)
    return frames


def fused_params():
    w = FUSED_WIN
    return O.hsv_params(h_lo=w["h_thresh"][0], h_hi=w["h_thresh"][1], s_lo=w["s_thresh"][0], s_hi=w["s_thresh"][1],
                        v_lo=w["v_thresh"][0], v_hi=w["v_thresh"][1], erode=FUSED_MORPH[0], dilate=FUSED_MORPH[1],
                        min_area=AREA[0], max_area=AREA[1])


def sub_params():
    w = sub_window()
    return O.hsv_params(h_lo=w["h"][0], h_hi=w["h"][1], s_lo=w["s"][0], s_hi=w["s"][1], v_lo=w["v"][0], v_hi=w["v"][1],
                        erode=SUB_MORPH[0], dilate=SUB_MORPH[1], min_area=AREA[0], max_area=AREA[1])


@functools.lru_cache(maxsize=None)
def sequence_masks(family, rows, cols, variant=0, alpha=0.0):
    """[(the oracle's detection, its mask after erode / dilate)] for every frame of sequence(...): oat_diff_detect for the motion
    tracker, oat_bsub_filter -> oat_bgr2hsv -> oat_detect_hsv for the subtraction tracker, oat_chain_step for the fused one."""
    frames = sequence(family, rows, cols, variant)
    out = []
    if family == "motion":
        d = O.Diff(rows, cols, DIFF["diff_threshold"], DIFF["blur"], *AREA)
        out = [d.detect(O.bgr2grey(f)) for f in frames]
    elif family == "subtraction":
        b, p = O.Bsub(rows, cols, 3, alpha), sub_params()
        out = [O.detect_hsv(O.bgr2hsv(b.filter(f)), p) for f in frames]
    else:
        mog, p = O.Mog2(rows, cols, 3), fused_params()
        out = [O.chain_step(mog, f, FUSED_LR, p) for f in frames]
    for _, m in out:
        m.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def sequence_reference(family, rows, cols, variant=0, alpha=0.0, k=TRACKER_K):
    """[(ranks, n_found)] for every frame."""
    return [reference(m, AREA, k) for _, m in sequence_masks(family, rows, cols, variant, alpha)]


def variant_of(stream):
    return stream % 3
