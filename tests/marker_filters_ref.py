"""The filter chain behind a marker set's combined record, restated for the tests (TEST INFRASTRUCTURE, no GPU imports):
what `posifilt homography` does to a heading, the (cv::Point) conversion, `posifilt region`'s point-in-polygon test, and the
chain kalman -> homography -> region over the oracle's filters.

Written from the references' behaviour, not from the library's source:
  heading   HomographyTransform2D::filter (HomographyTransform2D.cpp:90-101): cv::perspectiveTransform with the offsets of the
            matrix zeroed, then cv::normalize of the one-element vector (OpenCV 3.1: n = sqrt(hx*hx + hy*hy),
            scale = n > DBL_EPSILON ? 1 / n : 0, every component h * scale + 0)
  point     (cv::Point)cv::Point2d: cvRound per coordinate, round half to even
  region    RegionFilter2D::filter (RegionFilter2D.cpp:130-152): cv::pointPolygonTest(contour, pt, false) >= 0, OpenCV 3.1's
            purely integer branch, regions in configured order, first hit wins
Position and velocity go through oracle_lib (O.Kalman, O.homography)."""
import math
import sys

FLT_EPSILON = 2.0 ** -23
DBL_EPSILON = sys.float_info.epsilon
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


# ------------------------------------------------------------------------------------------------------ heading ---

def heading_through(h, hx, hy):
    """A heading through the 3 x 3 matrix h (9 values, row-major) with its offsets zeroed, then normalised by the
    reciprocal of its length.  Plain doubles, every product and sum rounded on its own, in the reference's order."""
    w = hx * h[6] + hy * h[7] + h[8]
    if abs(w) > FLT_EPSILON:                       # (false for a NaN)
        w = 1.0 / w
        ox = (hx * h[0] + hy * h[1] + 0.0) * w
        oy = (hx * h[3] + hy * h[4] + 0.0) * w
    else:
        ox = oy = 0.0
    n = math.sqrt(ox * ox + oy * oy)
    scale = 1.0 / n if n > DBL_EPSILON else 0.0
    return ox * scale + 0.0, oy * scale + 0.0


# -------------------------------------------------------------------------------------------------------- point ---

def cv_round(v):
    """cvRound of a double: to the nearest integer, ties to even.  None where the reference is undefined: a value that is
    not finite, or beyond int32 once rounded."""
    if not math.isfinite(v):
        return None
    r = round(v)                                   # Python rounds half to even
    return r if INT32_MIN <= r <= INT32_MAX else None


def to_point(x, y):
    """(cv::Point)cv::Point2d(x, y), or None."""
    p = (cv_round(x), cv_round(y))
    return None if None in p else p


def contour_of(points):
    """The std::vector<cv::Point> a configured list of cv::Point2d becomes."""
    return [to_point(x, y) for x, y in points]


# ------------------------------------------------------------------------------------------------------- region ---

def point_polygon_test(contour, pt):
    """cv::pointPolygonTest(contour, pt, measureDist=false) for integer vertices and an integer point: +1 inside, 0 on the
    boundary, -1 outside.  Python integers: no overflow."""
    if not contour:
        return -1
    px, py = pt
    counter = 0
    x0, y0 = contour[-1]
    for x, y in contour:
        if (y0 <= py and y <= py) or (y0 > py and y > py) or (x0 < px and x < px):
            if py == y and (px == x or (py == y0 and (x0 <= px <= x or x <= px <= x0))):
                return 0
        else:
            d = (py - y0) * (x - x0) - (px - x0) * (y - y0)
            if d == 0:
                return 0
            if y < y0:
                d = -d
            counter += d > 0
        x0, y0 = x, y
    return 1 if counter % 2 else -1


def region_of(regions, x, y):
    """Index of the first region of `regions` ([(name, points)], in configured order) that holds the position, or -1."""
    pt = to_point(x, y)
    if pt is None:
        return -1
    for i, (_, points) in enumerate(regions):
        if point_polygon_test(contour_of(points), pt) >= 0:
            return i
    return -1


def where(points, x, y):
    """'vertex' / 'edge' / 'inside' / 'outside': how the position lies to one region (for the tests' coverage checks)."""
    pt, contour = to_point(x, y), contour_of(points)
    r = point_polygon_test(contour, pt)
    if r == 0:
        return "vertex" if pt in contour else "edge"
    return "inside" if r > 0 else "outside"


# -------------------------------------------------------------------------------------------------------- chain ---

def chain(combined, kalman=None, homography=None, regions=None):
    """One frame of one camera through the chain.  combined: markers_ref.combine's dict; kalman: None or this camera's
    O.Kalman (its state advances); homography: None or 9 values; regions: None or [(name, points)].
    -> dict(position_valid, velocity_valid, heading_valid, region_valid, region (name or None), x, y, vx, vy, hx, hy)"""
    import oracle_lib as O
    k = dict(position_valid=bool(combined["position_valid"]), velocity_valid=False, x=combined["x"], y=combined["y"],
             vx=0.0, vy=0.0)
    if kalman is not None:                         # a partial sum under position_valid == 0 is not a measurement
        k = kalman.filter(combined["position_valid"], combined["x"], combined["y"])
    hv, hx, hy = bool(combined["heading_valid"]), combined["hx"], combined["hy"]
    if homography is not None:
        x, y, vx, vy = O.homography(homography, k["position_valid"], k["x"], k["y"], k["velocity_valid"], k["vx"], k["vy"])
        k = dict(k, x=x, y=y, vx=vx, vy=vy)
        if hv:
            hx, hy = heading_through([float(v) for v in homography], hx, hy)
    region = -1
    if regions and k["position_valid"]:
        region = region_of(regions, k["x"], k["y"])
    return dict(position_valid=bool(k["position_valid"]), velocity_valid=bool(k["velocity_valid"]), heading_valid=hv,
                region_valid=region >= 0, region=regions[region][0] if region >= 0 else None,
                x=k["x"], y=k["y"], vx=k["vx"], vy=k["vy"], hx=hx, hy=hy)
