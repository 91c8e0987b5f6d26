"""The model of target shapes (oatgpu_set_target_shapes / oatgpu_target_shapes), written from the text in
include/oatgpu.h alone (TEST INFRASTRUCTURE, no GPU imports: tests/test_shapes_cpu.py checks it and its cases, the GPU tests compare
the kernels with it bit for bit).

Everything comes from the oracle: oracle_lib.find_contours on the oracle's own mask after erode / dilate hands out every external
contour's CHAIN_APPROX_SIMPLE points; the candidates are ranked with targets_cases' key.  The order-2 sums are contourMoments'
(OpenCV 3.1 imgproc/moments.cpp) over those points in Python ints, the derived fields are Python floats (IEEE doubles, one
rounding per operation, math.sqrt)."""
import math

import numpy as np

import targets_cases as T

INVALID = dict(valid=False, a20=0, a11=0, a02=0, x_min=0, y_min=0, x_max=0, y_max=0, mu20=0.0, mu11=0.0, mu02=0.0,
               axis_valid=False, axis_x=0.0, axis_y=0.0, major=0.0, minor=0.0)
FIELDS = tuple(INVALID)
WRONG = ("hole_edges", "a11_cross_dropped", "ranks_exchanged", "mask_extents", "rounded_centroid", "axis_unsigned", "previous_frame")


# ----------------------------------------------------------------------------------------------------- the integer sums ----

def edges(points):
    """The directed edges of a closed polygon, in contourMoments' order: (last point -> first point) first."""
    return [(points[i - 1], points[i]) for i in range(len(points))]


def unit_steps(points):
    """The same polygon as unit steps between neighbouring border pixels (what the kernel sees): every edge of the
    CHAIN_APPROX_SIMPLE polygon is horizontal, vertical or diagonal."""
    out = []
    for (x0, y0), (x1, y1) in edges(points):
        dx, dy = x1 - x0, y1 - y0
        n = max(abs(dx), abs(dy))
        assert n == 0 or (abs(dx) in (0, n) and abs(dy) in (0, n)), (x0, y0, x1, y1)
        sx, sy = (dx > 0) - (dx < 0), (dy > 0) - (dy < 0)
        out += [((x0 + i * sx, y0 + i * sy), (x0 + (i + 1) * sx, y0 + (i + 1) * sy)) for i in range(n)]
    return out


def terms(e, a11_cross=True):
    """One edge's six terms: (a00, a10, a01, a20, a11, a02)"""
    (x0, y0), (x1, y1) = e
    d = x0 * y1 - x1 * y0
    a11 = d * (x0 * ((y0 + y1) + y0) + x1 * ((y0 + y1) + y1)) if a11_cross else d * (x0 * (y0 + y0) + x1 * (y1 + y1))
    return (d, d * (x0 + x1), d * (y0 + y1), d * (x0 * (x0 + x1) + x1 * x1), a11, d * (y0 * (y0 + y1) + y1 * y1))


def sums(edge_list, a11_cross=True):
    out = [0] * 6
    for e in edge_list:
        for i, v in enumerate(terms(e, a11_cross)):
            out[i] += v
    return tuple(out)


# --------------------------------------------------------------------------------------------------- the derived fields ----

def derive(a00, a10, a01, a20, a11, a02, round_centroid=False, signed=True):
    """mu20, mu11, mu02, axis_valid, axis_x, axis_y, major, minor -- oatgpu.h's list, operation for operation"""
    sg = 1.0 if a00 > 0 else -1.0
    m00 = float(a00) * (sg * 0.5)
    m10 = float(a10) * (sg * 0.16666666666666666666666666666667)
    m01 = float(a01) * (sg * 0.16666666666666666666666666666667)
    m20 = float(a20) * (sg * 0.083333333333333333333333333333333)
    m11 = float(a11) * (sg * 0.041666666666666666666666666666667)
    m02 = float(a02) * (sg * 0.083333333333333333333333333333333)
    inv = 1.0 / m00
    cx, cy = m10 * inv, m01 * inv
    if round_centroid:
        cx, cy = float(round(cx)), float(round(cy))
    mu20, mu11, mu02 = m20 - m10 * cx, m11 - m10 * cy, m02 - m01 * cy
    a, b, c = mu20 * inv, mu11 * inv, mu02 * inv
    h = (a - c) * 0.5
    r = math.sqrt(h * h + b * b)
    l1, l2 = (a + c) * 0.5 + r, (a + c) * 0.5 - r
    major = 2.0 * math.sqrt(l1 if l1 > 0.0 else 0.0)
    minor = 2.0 * math.sqrt(l2 if l2 > 0.0 else 0.0)
    branch = "h>=0" if h >= 0.0 else "h<0"
    vx, vy = (h + r, b) if h >= 0.0 else (b, r - h)
    n = math.sqrt(vx * vx + vy * vy)
    ok = n > 0.0
    ax, ay, flipped = 0.0, 0.0, False
    if ok:
        ax, ay = vx / n, vy / n
        flipped = vx < 0.0 or (vx == 0.0 and vy < 0.0)
        if flipped and signed:
            ax, ay = -ax, -ay
    return dict(mu20=mu20, mu11=mu11, mu02=mu02, axis_valid=ok, axis_x=ax, axis_y=ay, major=major, minor=minor), \
        dict(branch=branch if ok else "none", flipped=flipped, b=b)


def shape_of_contour(c, **kw):
    """A candidate contour of oracle_lib.find_contours -> its shape record"""
    s = sums(edges(c["points"]))
    assert s[:3] == (int(c["a00"]), int(c["a10"]), int(c["a01"])), (s[:3], c["a00"], c["a10"], c["a01"])
    xs, ys = [p[0] for p in c["points"]], [p[1] for p in c["points"]]
    d, _ = derive(*s, **kw)
    return dict(valid=True, a20=s[3], a11=s[4], a02=s[5], x_min=min(xs), y_min=min(ys), x_max=max(xs), y_max=max(ys), **d)


def ranked(mask, area, k):
    """The k best candidates of the mask, in rank order (targets_cases.reference's order)"""
    cols = mask.shape[1]
    return sorted(T.candidates(mask, area), key=lambda c: T._key(c, cols), reverse=True)[:k]


def reference(mask, area, k):
    """-> the k ranks' shapes as dicts, invalid where fewer candidates exist"""
    out = [shape_of_contour(c) for c in ranked(mask, area, k)]
    return out + [dict(INVALID) for _ in range(k - len(out))]


def same(a, b):
    """bit for bit: integers exact, doubles by bit pattern"""
    for f in FIELDS:
        x, y = a[f], b[f]
        if isinstance(x, float) or isinstance(y, float):
            if np.float64(x).tobytes() != np.float64(y).tobytes():
                return False
        elif x != y:
            return False
    return True


def same_set(a, b):
    return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------- the kernel's edge rule, for the identity and a wrong model ----

def outside_background(fg):
    """The background 4-connected to the one-pixel frame (which is background by construction)"""
    rows, cols = fg.shape
    out = np.zeros_like(fg)
    stack = [(0, 0)]
    out[0, 0] = True
    while stack:
        y, x = stack.pop()
        for ny, nx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            if 0 <= ny < rows and 0 <= nx < cols and not fg[ny, nx] and not out[ny, nx]:
                out[ny, nx] = True
                stack.append((ny, nx))
    return out


def pixel_edges(mask, pixels, holes_too=False):
    """The directed edges k_green_select's rule gives the pixels [(y, x)] of one blob: one per side facing outside background (with
    holes_too: any background), towards the next border pixel -- the diagonal neighbour first, then the straight one."""
    rows, cols = mask.shape
    fg = np.zeros((rows, cols), bool)
    fg[1:-1, 1:-1] = mask[1:-1, 1:-1] != 0
    faces = ~fg if holes_too else outside_background(fg)
    out = []
    for y, x in pixels:
        for (sy, sx), (dy, dx), (ty, tx) in (((0, -1), (1, -1), (1, 0)), ((1, 0), (1, 1), (0, 1)), ((0, 1), (-1, 1), (-1, 0)),
                                            ((-1, 0), (-1, -1), (0, -1))):
            if fg[y + sy, x + sx] or not faces[y + sy, x + sx]:
                continue
            if fg[y + dy, x + dx]:
                out.append(((x, y), (x + dx, y + dy)))
            elif fg[y + ty, x + tx]:
                out.append(((x, y), (x + tx, y + ty)))
    return out


# ---------------------------------------------------------------------------------------------------- planted wrong models ----

def wrong_reference(mask, area, k, wrong, previous=None):
    """The model with one rule replaced (WRONG); previous: the frame before's mask, for "previous_frame"."""
    if wrong == "previous_frame":
        return reference(mask if previous is None else previous, area, k)
    cs = ranked(mask, area, k)
    if wrong == "ranks_exchanged" and len(cs) > 1:
        cs[0], cs[1] = cs[1], cs[0]
    comps = {fp: px for fp, px in T.components(mask)} if wrong == "hole_edges" else {}
    out = []
    for c in cs:
        s = shape_of_contour(c, round_centroid=wrong == "rounded_centroid", signed=wrong != "axis_unsigned")
        if wrong in ("hole_edges", "a11_cross_dropped"):
            e = edges(c["points"])
            if wrong == "hole_edges":
                e = pixel_edges(mask, comps[c["start"][1] * mask.shape[1] + c["start"][0]], holes_too=True)
            t = sums(e, a11_cross=wrong != "a11_cross_dropped")
            s.update(a20=t[3], a11=t[4], a02=t[5])
            s.update(derive(int(c["a00"]), int(c["a10"]), int(c["a01"]), t[3], t[4], t[5])[0])
        if wrong == "mask_extents":
            ys, xs = np.nonzero(mask[1:-1, 1:-1])
            s.update(x_min=int(xs.min()) + 1, y_min=int(ys.min()) + 1, x_max=int(xs.max()) + 1, y_max=int(ys.max()) + 1)
        out.append(s)
    return out + [dict(INVALID) for _ in range(k - len(out))]

