"""numpy model of the library's Bayer RAW8 -> BGR stage (include/oatgpu.h "Bayer RAW8 -> BGR"), the mosaic that
undoes it, and the inputs the CPU and GPU tests share.  Host-side numpy only; no part of the product.

A pattern is named by the 2 x 2 tile at image rows 0-1, columns 0-1 read row by row; its value is the library's
OATGPU_BAYER_*.  The arithmetic is OpenCV 3.1's bilinear Bayer2RGB_ in 32-bit integers."""
import numpy as np

RGGB, BGGR, GRBG, GBRG = 1, 2, 3, 4
PATTERNS = (RGGB, BGGR, GRBG, GBRG)
NAMES = {RGGB: "RGGB", BGGR: "BGGR", GRBG: "GRBG", GBRG: "GBRG"}
R_AT = {RGGB: (0, 0), BGGR: (1, 1), GRBG: (0, 1), GBRG: (1, 0)}       # (row, column) parity of the R sample
OPENCV_CODE = {RGGB: "COLOR_BayerBG2BGR", BGGR: "COLOR_BayerRG2BGR", GRBG: "COLOR_BayerGB2BGR", GBRG: "COLOR_BayerGR2BGR"}


def _sites(rows, cols, pattern, y0=0, x0=0):
    """(the row holds R samples, the column holds R samples) for the pixels (y0 + i, x0 + j)"""
    ry, rx = R_AT[pattern]
    yy, xx = np.mgrid[y0:y0 + rows, x0:x0 + cols]
    return (yy & 1) == ry, (xx & 1) == rx


def demosaic(raw, pattern):
    """(rows, cols) uint8 -> (rows, cols, 3) uint8 BGR"""
    raw = np.asarray(raw)
    rows, cols = raw.shape
    if rows < 3 or cols < 3:
        raise ValueError("demosaicing needs at least 3 x 3 pixels")
    a = raw.astype(np.int32)
    c = a[1:-1, 1:-1]
    n, s, w, e = a[:-2, 1:-1], a[2:, 1:-1], a[1:-1, :-2], a[1:-1, 2:]
    nw, ne, sw, se = a[:-2, :-2], a[:-2, 2:], a[2:, :-2], a[2:, 2:]
    h, v = (w + e + 1) >> 1, (n + s + 1) >> 1
    p, d = (n + s + w + e + 2) >> 2, (nw + ne + sw + se + 2) >> 2
    row_r, col_r = _sites(rows - 2, cols - 2, pattern, 1, 1)
    rb = row_r == col_r                                     # an R or a B site
    g = np.where(rb, p, c)
    r = np.where(rb, np.where(row_r, c, d), np.where(row_r, h, v))
    b = np.where(rb, np.where(row_r, d, c), np.where(row_r, v, h))
    inner = np.stack([b, g, r], -1).astype(np.uint8)
    iy = np.clip(np.arange(rows), 1, rows - 2) - 1
    ix = np.clip(np.arange(cols), 1, cols - 2) - 1
    return np.ascontiguousarray(inner[iy][:, ix])


def mosaic(bgr, pattern):
    """(rows, cols, 3) BGR -> the (rows, cols) samples a sensor with that pattern keeps"""
    bgr = np.asarray(bgr)
    row_r, col_r = _sites(bgr.shape[0], bgr.shape[1], pattern)
    return np.where(row_r & col_r, bgr[..., 2], np.where(~row_r & ~col_r, bgr[..., 0], bgr[..., 1])).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- the shared inputs --

# The shape that crosses a wave and a workgroup boundary of the wide mapping in x and in y: 12 x 1040 is 6 block rows of
# 260 lanes (4 pixels x 2 rows a lane, lanes in raster order, 64 a wave, 256 a workgroup) -- wave and workgroup boundaries
# fall inside a block row (x) and between block rows (y); 9 x 1041 does the same for the narrow mapping (one pixel a lane).
CROSSING_WIDE = (12, 1040)
CROSSING_NARROW = (9, 1041)
SHAPES = [(3, 3), (4, 4), (6, 8), (5, 12), (7, 10), CROSSING_WIDE, CROSSING_NARROW]


def random_mosaic(rows, cols, seed):
    """seeded random samples with runs of 0 and of 255 planted (saturated sums, zero sums)"""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    flat = raw.reshape(-1)
    for val in (0, 255):
        for _ in range(2):
            n = int(rng.integers(2, max(3, min(flat.size // 3, 3 * cols))))
            at = int(rng.integers(0, flat.size - n + 1))
            flat[at:at + n] = val
    if rows >= 6 and cols >= 6:                             # ... and a 255 block and a 0 block: every neighbourhood sum saturates
        raw[1:4, 1:5] = 255
        raw[rows - 4:rows - 1, cols - 5:cols - 1] = 0
    return raw


def case_list():
    """[(rows, cols, pattern, raw)]: every shape of SHAPES with every pattern"""
    out = []
    for i, (rows, cols) in enumerate(SHAPES):
        for p in PATTERNS:
            out.append((rows, cols, p, random_mosaic(rows, cols, 100 * i + p)))
    return out


# ------------------------------------------------------------------------------------------ the tracker sequences --

TRACK_ROWS, TRACK_COLS, TRACK_T = 48, 64, 12
DISC_BGR = (255, 64, 0)                                     # HSV (112, 255, 255): oat_amd.synth's first disc
DISC_RADIUS = 7
HSV_WIN = dict(h_lo=100, h_hi=125, s_lo=150, s_hi=256, v_lo=100, v_hi=256)
DETECT = dict(erode=0, dilate=3, min_area=10.0, max_area=1e6)
LR = 0.01


def track_scene(seed, t):
    """BGR frame t of tracker sequence `seed`: a noisy grey gradient, from frame 1 on a saturated disc on a straight path"""
    rows, cols = TRACK_ROWS, TRACK_COLS
    rng = np.random.default_rng(1000 * seed + t)
    yy, xx = np.mgrid[0:rows, 0:cols]
    base = 100 + 30 * xx / (cols - 1) + 20 * yy / (rows - 1)
    f = np.stack([base, base + 6, base - 5], -1) + rng.integers(-4, 5, (rows, cols, 3))
    f = np.clip(f, 0, 255).astype(np.uint8)
    if t > 0:
        cx = 12 + (3 + seed % 2) * t + seed % 5
        cy = 12 + 2 * t + seed % 3
        f[(xx - cx) ** 2 + (yy - cy) ** 2 <= DISC_RADIUS ** 2] = DISC_BGR
    return f


def track_sequence(seed, pattern, T=TRACK_T):
    """(raw[T], model[T]): the mosaicked scene frames and the model's demosaiced frames"""
    raw = [mosaic(track_scene(seed, t), pattern) for t in range(T)]
    return raw, [demosaic(r, pattern) for r in raw]


# the sequences of tests/test_track_bayer_gpu.py as (seed, pattern); tests/test_debayer_cpu.py checks each for non-vacuity
TRACK_SEQUENCES = [(1, RGGB), (2, BGGR), (3, GRBG), (4, GBRG), (5, RGGB), (6, GBRG)]
