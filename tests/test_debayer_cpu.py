"""CPU tests of the Bayer RAW8 -> BGR definition (tests/debayer_ref.py; include/oatgpu.h): the vectorised model against a
scalar restatement written separately, the known answers, the border rule, the rounding cases the shared inputs cover, the
wrong demosaics they tell from the right one, and the non-vacuity of the GPU test's tracker sequences."""
import numpy as np
import pytest

import debayer_ref as D

TILE = {D.RGGB: "RGGB", D.BGGR: "BGGR", D.GRBG: "GRBG", D.GBRG: "GBRG"}


def scalar_demosaic(raw, pattern, wrong=None):
    """Pixel by pixel from the text of the specification: the colour of a site is looked up in the tile's letters, the
    colours a G site interpolates are those of its east and south neighbours.  `wrong` plants one mistake."""
    raw = np.asarray(raw).astype(int)
    rows, cols = raw.shape
    tile = TILE[pattern]
    shift = 1 if wrong == "shifted" else 0

    def colour(y, x):
        return tile[(y & 1) * 2 + ((x + shift) & 1)]

    r2, r4 = (0, 0) if wrong == "truncate" else (1, 2)
    out = np.zeros((rows, cols, 3), np.uint8)
    slot = {"B": 2, "G": 1, "R": 0} if wrong == "swap_rb" else {"B": 0, "G": 1, "R": 2}
    for y in range(rows):
        for x in range(cols):
            if wrong == "zero_border" and (y in (0, rows - 1) or x in (0, cols - 1)):
                continue
            cy, cx = min(max(y, 1), rows - 2), min(max(x, 1), cols - 2)
            n, s, w, e = raw[cy - 1, cx], raw[cy + 1, cx], raw[cy, cx - 1], raw[cy, cx + 1]
            diag = raw[cy - 1, cx - 1] + raw[cy - 1, cx + 1] + raw[cy + 1, cx - 1] + raw[cy + 1, cx + 1]
            own = colour(cy, cx)
            px = {}
            if own in "RB":
                px[own] = raw[cy, cx]
                px["G"] = (diag + r4) >> 2 if wrong == "g_from_diagonals" else (n + s + w + e + r4) >> 2
                px["B" if own == "R" else "R"] = (diag + r4) >> 2
            else:
                px["G"] = raw[cy, cx]
                hor, ver = colour(cy, cx + 1), colour(cy + 1, cx)
                if wrong == "swap_hv":
                    hor, ver = ver, hor
                px[hor] = (w + e + r2) >> 1
                px[ver] = (n + s + r2) >> 1
            for k, v in px.items():
                out[y, x, slot[k]] = v
    return out


WRONG = ("swap_rb", "shifted", "truncate", "zero_border", "swap_hv", "g_from_diagonals")
SMALL = [c for c in D.case_list() if c[0] * c[1] <= 200]      # the scalar loop is slow: the small shapes, every pattern


def test_model_equals_the_scalar_restatement():
    assert len(SMALL) >= 20
    for rows, cols, p, raw in SMALL:
        assert np.array_equal(D.demosaic(raw, p), scalar_demosaic(raw, p)), (rows, cols, p)
    for rows, cols in ((3, 7), (9, 3), (11, 13)):
        for p in D.PATTERNS:
            raw = D.random_mosaic(rows, cols, rows * cols + p)
            assert np.array_equal(D.demosaic(raw, p), scalar_demosaic(raw, p)), (rows, cols, p)


def test_known_answers():
    m = np.array([[1, 0, 2], [0, 9, 1], [0, 0, 0]], np.uint8)
    assert (D.demosaic(m, D.RGGB) == np.array([9, 0, 1], np.uint8)).all()
    assert (D.demosaic(m, D.GRBG) == np.array([1, 9, 0], np.uint8)).all()
    assert (scalar_demosaic(m, D.RGGB) == np.array([9, 0, 1], np.uint8)).all()
    assert (scalar_demosaic(m, D.GRBG) == np.array([1, 9, 0], np.uint8)).all()


@pytest.mark.parametrize("pattern", D.PATTERNS)
def test_uniform_colours_and_even_ramps_come_back(pattern):
    for rows, cols in ((3, 3), (6, 8), (7, 10)):
        for col in ((0, 0, 0), (255, 255, 255), (255, 64, 0), (1, 2, 3), (17, 250, 99)):
            img = np.empty((rows, cols, 3), np.uint8)
            img[:] = col
            assert np.array_equal(D.demosaic(D.mosaic(img, pattern), pattern), img), (rows, cols, col)
    rows, cols = 9, 12
    yy, xx = np.mgrid[0:rows, 0:cols]
    ramp = np.stack([10 + 2 * xx + 4 * yy, 200 - 6 * xx - 2 * yy, 30 + 8 * xx + 10 * yy], -1)
    assert ramp.min() >= 0 and ramp.max() <= 255
    ramp = ramp.astype(np.uint8)
    got = D.demosaic(D.mosaic(ramp, pattern), pattern)
    assert np.array_equal(got[1:-1, 1:-1], ramp[1:-1, 1:-1])
    assert not np.array_equal(got, ramp)                     # (the border repeats its neighbour: a ramp does not come back there)


@pytest.mark.parametrize("pattern", D.PATTERNS)
def test_border_pixels_equal_their_clamped_neighbour(pattern):
    for rows, cols in ((3, 3), (4, 4), (5, 12), (7, 10)):
        out = D.demosaic(D.random_mosaic(rows, cols, 7 * rows + cols + pattern), pattern)
        for y in range(rows):
            for x in range(cols):
                cy, cx = min(max(y, 1), rows - 2), min(max(x, 1), cols - 2)
                assert np.array_equal(out[y, x], out[cy, cx]), (rows, cols, y, x)


def test_the_shared_inputs_cover_every_rounding_case():
    """4-sums of every remainder mod 4 (plus and diagonal), 2-sums odd and even, saturated (all 255) and zero sums"""
    plus, diag, two, sat, zero = set(), set(), set(), 0, 0
    for rows, cols, p, raw in D.case_list():
        a = raw.astype(int)
        n, s, w, e = a[:-2, 1:-1], a[2:, 1:-1], a[1:-1, :-2], a[1:-1, 2:]
        d4 = a[:-2, :-2] + a[:-2, 2:] + a[2:, :-2] + a[2:, 2:]
        row_r, col_r = D._sites(rows - 2, cols - 2, p, 1, 1)
        rb = row_r == col_r
        p4 = (n + s + w + e)[rb]
        plus |= set((p4 % 4).tolist())
        diag |= set((d4[rb] % 4).tolist())
        two |= set(((w + e)[~rb] % 2).tolist()) | set(((n + s)[~rb] % 2).tolist())
        sat += int((p4 == 1020).sum() and (d4[rb] == 1020).sum() and ((w + e)[~rb] == 510).sum() and ((n + s)[~rb] == 510).sum())
        zero += int((p4 == 0).sum() and (d4[rb] == 0).sum() and ((w + e)[~rb] == 0).sum())
    assert plus == {0, 1, 2, 3} and diag == {0, 1, 2, 3} and two == {0, 1}
    assert sat >= 4 and zero >= 4


@pytest.mark.parametrize("wrong", WRONG)
def test_the_case_list_tells_a_planted_wrong_demosaic_from_the_right_one(wrong):
    told = 0
    for rows, cols, p, raw in SMALL:
        told += not np.array_equal(scalar_demosaic(raw, p, wrong), D.demosaic(raw, p))
    assert told >= len(SMALL) // 2, (wrong, told)


def test_the_tracker_sequences_are_not_vacuous():
    """From frame 2 on the oracle chain on the model's frames finds the disc on at least half of the frames, for every
    sequence tests/test_track_bayer_gpu.py uses."""
    import oracle_lib as O
    p = O.hsv_params(**D.HSV_WIN, **D.DETECT)
    for seed, pattern in D.TRACK_SEQUENCES:
        _, model = D.track_sequence(seed, pattern)
        orc = O.Mog2(D.TRACK_ROWS, D.TRACK_COLS, 3)
        valid = [O.chain_step(orc, f, D.LR, p)[0]["valid"] for f in model]
        later = valid[1:]
        assert len(later) == D.TRACK_T - 1 and sum(later) * 2 >= len(later), (seed, pattern, valid)
