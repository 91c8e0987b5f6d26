"""Marker sets restated for the tests: oat::MeanPosition::combine (src/positioncombiner/MeanPosition.cpp:60-118) in plain
Python doubles, and the expected per-marker results as the existing oracle chain run once per marker.

MOG2 does not depend on the detector, so `posidet hsv` number m behind one `framefilt mog` sees what a chain of its own
(O.Mog2 + O.chain_step with marker m's hsv_params) sees when every chain is fed the same frames."""
import math

import oracle_lib as O


def _div(a, b):
    """IEEE a / b where Python raises: x / 0 is +-inf, 0 / 0 is NaN."""
    if b == 0.0:
        return math.nan if (a == 0.0 or a != a) else math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def combine(positions, anchor=None):
    """positions: [(valid, x, y)] of one camera's markers, in marker order; an invalid marker's x, y are what its
    Position2D holds (the library: 0, 0).  anchor: marker index or None.
    -> dict(position_valid, heading_valid, velocity_valid, n_valid, x, y, hx, hy), MeanPosition::combine's arithmetic:
    every product and sum rounded on its own, in the reference's order."""
    mean_denom = 1.0 / float(len(positions))
    px = py = hx = hy = 0.0
    position_valid, heading_valid, n_valid = True, True, 0
    for valid, x, y in positions:
        if valid:
            px += mean_denom * x
            py += mean_denom * y
            n_valid += 1
        else:
            position_valid = False
        if anchor is not None:
            if position_valid:
                hx += x - positions[anchor][1]
                hy += y - positions[anchor][2]
            else:
                heading_valid = False
        else:
            heading_valid = False          # detectors never set Position2D::heading_valid
    if heading_valid:
        mag = math.sqrt(hx * hx + hy * hy)
        hx, hy = _div(hx, mag), _div(hy, mag)
    return dict(position_valid=position_valid, heading_valid=heading_valid, velocity_valid=False, n_valid=n_valid,
                x=px, y=py, hx=hx, hy=hy)


def hsv_params_of(marker, channels=3):
    """oracle parameters of one marker dict (HotPath.set_markers' form)."""
    h, s, v = marker.get("h", (0, 256)), marker.get("s", (0, 256)), marker.get("v", (0, 256))
    area = marker.get("area", (0.0, 1.7976931348623157e308))
    kw = dict(h_lo=h[0], h_hi=h[1], erode=marker.get("erode", 0), dilate=marker.get("dilate", 10),
              min_area=area[0], max_area=area[1])
    if channels == 3:
        kw.update(s_lo=s[0], s_hi=s[1], v_lo=v[0], v_hi=v[1])
    return O.hsv_params(**kw)


class MarkerOracle:
    """One camera: M oracle chains, one per marker, each with its own model, all fed the same frames."""

    def __init__(self, rows, cols, channels, markers, nthreads=4):
        self.mogs = [O.Mog2(rows, cols, channels) for _ in markers]
        self.params = [hsv_params_of(m, channels) for m in markers]
        self.nthreads = nthreads

    def set_window(self, m, marker, channels=3):
        self.params[m] = hsv_params_of(marker, channels)

    def step(self, frame, lr):
        """-> ([detection dict per marker], [inRange plane per marker])"""
        out = [O.chain_step(mog, frame, lr, p, self.nthreads) for mog, p in zip(self.mogs, self.params)]
        return [d for d, _ in out], [t for _, t in out]
