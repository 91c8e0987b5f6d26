"""The assertions the parity tests share (TEST INFRASTRUCTURE): a Position2D against an oracle detection, a MOG2
model against the oracle's, bit for bit, and two doubles of a filtered record.  They lived in test_gpu_parity.py;
tests/api_sequences.py needs them without a GPU, so they have a module of their own.  What they assert is unchanged."""
import math

import numpy as np

CENTROID_TOL = 1e-4     # px, from BASELINE.json north_star


def _same_detection(got, want, tag=""):
    assert got.position_valid == want["valid"], (tag, got, want)
    assert got.area == want["area"], (tag, got, want)
    if want["valid"]:
        assert (got.a00, got.a10, got.a01) == (want["a00"], want["a10"], want["a01"]), (tag, got, want)
        assert got.first_pixel == want["first_pixel"], (tag, got, want)
        assert abs(got.x - want["x"]) <= CENTROID_TOL and abs(got.y - want["y"]) <= CENTROID_TOL, (tag, got, want)
        assert got.x == want["x"] and got.y == want["y"], (tag, got, want)


def _same_double(a, b):
    """Equal as doubles, a NaN matched by a NaN (the filter chain's records: test_marker_filters_gpu, test_tracker_filters_gpu)."""
    return math.isnan(a) if math.isnan(b) else a == b


def _eq(a, b):
    """Equal, a NaN being equal to a NaN: with the reference's `nmodes = nNewModes;` a pruned slot (weight 0) that
    is matched again at learning rate 0 gets k = alphaT / weight = 0 / 0 -- its mean AND its variance are NaN from then
    on, on both sides (OpenCV's MAX / MIN macros keep a NaN on the left: `NaN < varMin` is false)."""
    return ((a == b) | (np.isnan(a) & np.isnan(b))).all()


def _same_state(gpu_state, ora_state, tag=""):
    nm_g, w_g, v_g, m_g, _ = gpu_state
    nm_o, w_o, v_o, m_o = ora_state
    assert (nm_g == nm_o).all(), tag
    k = w_o.shape[1]
    live = np.arange(k)[None, :] < nm_o[:, None]
    assert _eq(w_g[live], w_o[live]), tag
    assert _eq(v_g[live], v_o[live]), tag
    assert _eq(m_g[live], m_o[live]), tag
