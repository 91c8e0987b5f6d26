"""Restatement of `framefilt undistort` (src/framefilter/Undistorter.cpp:83-88: cv::undistort(temp, frame, K, D)) in numpy:
the oracle of tests/test_undistort_*.py.

OpenCV 3.1's cv::undistort with no new camera matrix:
  - stripes of stripe0 = min(max(1, 4096 // cols), rows) rows; for the stripe starting at row y, Ar = K with
    Ar[1][2] = K[1][2] - y, and initUndistortRectifyMap(K, D, I, Ar, (cols, stripe), CV_16SC2);
  - ir = inv(Ar) by cv::invert's closed-form 3x3 LU path; per row i of a stripe _x = i*ir[1] + ir[2] (likewise _y, _w),
    then the column loop ADDS ir[0] (ir[3], ir[6]) after every pixel -- np.add.accumulate is that sequential sum;
  - u, v in float64 as initUndistortRectifyMap writes them, iu = cvRound(u * 32) (half to even, INT_MIN for NaN and out of
    int range), map1 = (short)(iu >> 5), (short)(iv >> 5) (wraps), map2 = (iv & 31) * 32 + (iu & 31);
  - remap(INTER_LINEAR, BORDER_CONSTANT 0) of 8-bit data with BilinearTab_i, OpenCV's 15-bit weights:
    dst = (sum S * w + 16384) >> 15, a corner outside the frame reading 0.
float64 throughout; nothing here is shared with the library.
"""
import numpy as np

INT_MIN = -2147483648


def check_coeffs(dist):
    n = len(dist)
    if n < 5 or n > 8:
        raise ValueError("Distortion coefficients consist of 5 to 8 values.")
    if n in (6, 7):
        raise ValueError("6 or 7 distortion coefficients: OpenCV 3.1 accepts 4, 5, 8 or 12")


def cv_round(v):
    """cvRound of float64 values (SSE2 cvtsd2si) as int64 holding int32 values."""
    r = np.rint(v)
    ok = (r >= -2147483648.0) & (r <= 2147483647.0)          # NaN compares false
    out = np.full(np.shape(v), INT_MIN, np.int64)
    out[ok] = r[ok].astype(np.int64)
    return out


def inv3_lu(m):
    """cv::invert(DECOMP_LU) of a 3x3 double matrix (row-major list of 9): det3, d = 1/d, adjugate; singular -> zeros."""
    M = lambda i, j: m[3 * i + j]  # noqa: E731
    d = (M(0, 0) * (M(1, 1) * M(2, 2) - M(1, 2) * M(2, 1)) -
         M(0, 1) * (M(1, 0) * M(2, 2) - M(1, 2) * M(2, 0)) +
         M(0, 2) * (M(1, 0) * M(2, 1) - M(1, 1) * M(2, 0)))
    if d == 0.0:
        return [0.0] * 9
    d = 1. / d
    return [(M(1, 1) * M(2, 2) - M(1, 2) * M(2, 1)) * d,
            (M(0, 2) * M(2, 1) - M(0, 1) * M(2, 2)) * d,
            (M(0, 1) * M(1, 2) - M(0, 2) * M(1, 1)) * d,
            (M(1, 2) * M(2, 0) - M(1, 0) * M(2, 2)) * d,
            (M(0, 0) * M(2, 2) - M(0, 2) * M(2, 0)) * d,
            (M(0, 2) * M(1, 0) - M(0, 0) * M(1, 2)) * d,
            (M(1, 0) * M(2, 1) - M(1, 1) * M(2, 0)) * d,
            (M(0, 1) * M(2, 0) - M(0, 0) * M(2, 1)) * d,
            (M(0, 0) * M(1, 1) - M(0, 1) * M(1, 0)) * d]


def stripe_rows(rows, cols):
    return min(max(1, 4096 // max(cols, 1)), rows)


def row_inverses(rows, cols, K):
    """Per image row: (i, ir) -- the row's index inside its stripe and the stripe's inv(Ar), as a (rows, 9) array."""
    K = [float(k) for k in np.asarray(K, np.float64).reshape(9)]
    s0 = stripe_rows(rows, cols)
    irs = np.empty((rows, 9), np.float64)
    i = np.empty(rows, np.float64)
    for y in range(0, rows, s0):
        n = min(s0, rows - y)
        Ar = list(K)
        Ar[5] = K[5] - y
        irs[y:y + n] = inv3_lu(Ar)
        i[y:y + n] = np.arange(n)
    return i, irs


def _coords(rows, cols, K, dist, sequential=True):
    """u, v (float64, rows x cols) of initUndistortRectifyMap.  sequential=False takes _x0 + j * ir[0] instead of the
    column loop's running sum (the independent float check)."""
    check_coeffs(dist)
    D = [float(d) for d in dist]
    k1, k2, p1, p2, k3 = D[:5]
    k4, k5, k6 = (D[5], D[6], D[7]) if len(D) == 8 else (0., 0., 0.)
    Kf = np.asarray(K, np.float64).reshape(9)
    u0, v0, fx, fy = Kf[2], Kf[5], Kf[0], Kf[4]
    i, ir = row_inverses(rows, cols, K)

    def walk(c0, c1, c2):
        start = i * ir[:, c1] + ir[:, c2]
        if sequential:
            a = np.empty((rows, cols), np.float64)
            a[:, 0] = start
            a[:, 1:] = ir[:, c0][:, None]
            return np.add.accumulate(a, axis=1)
        return start[:, None] + np.arange(cols, dtype=np.float64)[None, :] * ir[:, c0][:, None]

    with np.errstate(all="ignore"):
        _x, _y, _w = walk(0, 1, 2), walk(3, 4, 5), walk(6, 7, 8)
        w = 1. / _w
        x = _x * w
        y = _y * w
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        _2xy = 2 * x * y
        kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
        u = fx * (x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)) + u0
        v = fy * (y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy) + v0
    return u, v


def undistort_map(rows, cols, K, dist):
    """(map1 int16 (rows, cols, 2), map2 uint16 (rows, cols)): cv::undistort's CV_16SC2 map, stripe by stripe."""
    u, v = _coords(rows, cols, K, dist)
    with np.errstate(all="ignore"):
        iu = cv_round(u * 32)
        iv = cv_round(v * 32)
    map1 = np.empty((rows, cols, 2), np.int16)
    map1[..., 0] = (iu >> 5).astype(np.int16)         # (short): keeps the low 16 bits
    map1[..., 1] = (iv >> 5).astype(np.int16)
    map2 = ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)
    return map1, map2


def bilinear_tab():
    """BilinearTab_i: [1024][4] weights (00, 01, 10, 11) of fraction index fy*32 + fx, scale 2^15."""
    f = np.arange(1024)
    fx, fy = f & 31, f >> 5
    return np.stack([32 * (32 - fx) * (32 - fy), 32 * fx * (32 - fy), 32 * (32 - fx) * fy, 32 * fx * fy], axis=1).astype(np.int64)


def remap(src, map1, map2):
    """remap(src, map1, map2, INTER_LINEAR, BORDER_CONSTANT, 0) of an 8-bit (H, W) or (H, W, C) frame."""
    H, W = src.shape[:2]
    s = src.reshape(H, W, -1).astype(np.int64)
    sx = map1[..., 0].astype(np.int64)
    sy = map1[..., 1].astype(np.int64)
    wt = bilinear_tab()[map2.astype(np.int64)]
    acc = np.zeros(map2.shape + (s.shape[2],), np.int64)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        xx, yy = sx + dx, sy + dy
        inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        val = s[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)] * inside[..., None]
        acc += val * wt[..., k][..., None]
    out = ((acc + 16384) >> 15).astype(np.uint8)
    return out.reshape(map2.shape + src.shape[2:])


def undistort(src, K, dist):
    """cv::undistort(src, dst, K, dist) of an 8-bit frame."""
    m1, m2 = undistort_map(src.shape[0], src.shape[1], K, dist)
    return remap(src, m1, m2)


def undistort_float(src, K, dist):
    """Independent float form: u, v from the formulas with _x0 + j * ir[0] (no running sum), no 1/32-px quantisation,
    float bilinear weights, corners outside the frame 0.  Agrees with undistort() to a grey level on smooth content."""
    H, W = src.shape[:2]
    u, v = _coords(H, W, K, dist, sequential=False)
    s = src.reshape(H, W, -1).astype(np.float64)
    with np.errstate(all="ignore"):
        ok = np.isfinite(u) & np.isfinite(v) & (np.abs(u) < 1e9) & (np.abs(v) < 1e9)
        u = np.where(ok, u, -10.0)
        v = np.where(ok, v, -10.0)
    x0, y0 = np.floor(u), np.floor(v)
    ax, ay = (u - x0)[..., None], (v - y0)[..., None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    acc = np.zeros((H, W, s.shape[2]), np.float64)
    for dy, dx, wgt in ((0, 0, (1 - ax) * (1 - ay)), (0, 1, ax * (1 - ay)), (1, 0, (1 - ax) * ay), (1, 1, ax * ay)):
        xx, yy = x0 + dx, y0 + dy
        inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        acc += s[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)] * inside[..., None] * wgt
    return acc.reshape(src.shape)


# ---- the calibrations the tests run (CPU map parity, GPU frame parity) ----

def reference_config():
    """(K, D) of the reference's own [undistort] table (tests/golden/undistort_reference_config.toml)."""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "undistort_reference_config.toml")
    text = "\n".join(l.split("#")[0] for l in open(path).read().splitlines())

    def array(key):
        return [float(v) for v in re.search(key + r"\s*=\s*\[([^\]]*)\]", text).group(1).split(",")]
    return array("camera-matrix"), array("distortion-coeffs")


def scaled_k(rows, cols, f=0.8, skew=0.0):
    """A camera matrix for a rows x cols frame: focal length f * cols, principal point near the centre."""
    return [f * cols, skew, cols / 2.0 - 0.37, 0.0, f * cols * 1.01, rows / 2.0 + 0.29, 0.0, 0.0, 1.0]


def cases(rows, cols):
    """name -> (K, D): 5 and 8 coefficients, strong barrel and pincushion (pixels off-frame and at sx = -1), a skewed K,
    and the reference's own calibration."""
    K, D = reference_config()
    return {
        "reference": (K, D),
        "mild5": (scaled_k(rows, cols), [-0.21, 0.07, 0.0013, -0.0009, -0.011]),
        "rational8": (scaled_k(rows, cols, 0.6), [0.15, -0.04, 0.0007, 0.0011, 0.002, 0.4, -0.05, 0.01]),
        "barrel": (scaled_k(rows, cols, 0.5), [-0.9, 0.6, 0.0, 0.0, -0.2]),
        "pincushion": (scaled_k(rows, cols, 0.5), [1.4, 0.9, 0.002, -0.003, 0.3]),
        "skew": (scaled_k(rows, cols, 0.7, skew=0.08 * cols), [-0.3, 0.1, 0.001, 0.002, 0.0]),
    }
