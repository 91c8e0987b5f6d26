"""The seam cases (tests/seam_cases.py), on the CPU: every position the blob kernels' shared border rule can go wrong at really
holds a border pixel in every case's final mask, the cases stay on the LDS kernel's side of its limits, and the references the
GPU test compares with have something to say about them."""
import numpy as np
import pytest

import blob_load as B
import oracle_lib as O
import seam_cases as S
import shapes_ref as R
import targets_cases as T

CASES = S.cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_seam_holds_a_border_pixel(name):
    m = CASES[name]
    assert m.shape == (S.H, S.W) == (12, 200) and -(-S.W // S.WORD) == 4 and S.W % S.WORD == 8
    fin = S.final(m)
    assert (fin == m).all()                                               # nothing planted on the frame: mask == final mask
    bd = S.border(fin)
    ys, xs = np.nonzero(bd)
    bits, words = set(xs % S.WORD), set(xs // S.WORD)
    assert set(S.SEAM_BITS) <= bits, (name, sorted(set(S.SEAM_BITS) - bits))   # bit 0, bit 63, both sides of 15|16, 31|32, 47|48
    assert {0, 3} <= words                                                # the first and the last (partial) word of a row
    assert {1, S.H - 2} <= set(ys)                                        # rows 1 and H - 2
    # a hole: a border pixel with a background 4-neighbour that is not OUTSIDE
    fg = fin != 0
    hole = ~fg & ~R.outside_background(fg)
    assert hole.any()
    ph = np.pad(hole, 1)
    beside_hole = ph[:-2, 1:-1] | ph[2:, 1:-1] | ph[1:-1, :-2] | ph[1:-1, 2:]
    assert (bd & beside_hole).any(), name
    # two squares touching only at a corner across a word boundary: one component
    assert S.corner_contacts(fin), name
    (y, x), = S.corner_contacts(fin)[:1]
    comps = T.components(fin)
    assert any((y, x) in set(p) and (y + 1, x + 1) in set(p) for _, p in comps), name


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_cases_take_the_lds_kernel_and_rank_more_blobs_than_k(name):
    fin = S.final(CASES[name])
    L = B.blob_load(fin)
    assert L["path"] == "lds" and L["NR"] >= 5, L                         # a plain step is k_blob_lds'; more blobs than K = 4
    ranks, n_found = T.reference(fin, S.AREA, S.KS[0])
    assert n_found > S.KS[0] and all(r["valid"] for r in ranks)
    shapes = R.reference(fin, S.AREA, S.KS[0])
    assert all(s["valid"] for s in shapes)
    holed = [c for c in O.find_contours(fin) if c["m00"] > 0]
    assert len(holed) == n_found


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_seam_lies_on_a_blob_whose_record_is_compared(name):
    """The GPU test compares, per case: the one record of a plain step in every window of windows(), and the K ranks (targets and
    shapes) for K = 4 and K = 8.  Every listed seam must have a border pixel on a blob that is (a) the winner of one window --
    the LDS kernel's sums of it are compared -- and (b) among the 8 ranks, and the corner-contact blob and a blob beside a hole among
    them; K = 4 alone leaves the smallest blob out, which is why K = 8 is there."""
    fin = S.final(CASES[name])
    blob_of = {p: first for first, px in T.components(fin) for p in px}            # (y, x) -> the blob's first pixel
    winners = set()
    for lo, hi in S.windows(fin):
        ranks, n_found = T.reference(fin, (lo, hi), 1)
        assert ranks[0]["valid"], (name, lo, hi)
        if (lo, hi) != S.AREA:
            assert n_found == 1, (name, lo, hi, n_found)                           # the window's only candidate
        winners.add(ranks[0]["first_pixel"])
    ranked = {k: {r["first_pixel"] for r in T.reference(fin, S.AREA, k)[0] if r["valid"]} for k in S.KS}
    shaped = {k: sum(s["valid"] for s in R.reference(fin, S.AREA, k)) for k in S.KS}
    every = {first for first, _ in T.components(fin)}
    assert winners == every == ranked[8] and shaped[8] == len(every) == 5, (name, winners, ranked)
    assert len(ranked[4]) == 4 and ranked[4] < every
    for seam, px in S.seams(fin).items():
        assert px, (name, seam)
        on = {blob_of[p] for p in px}
        assert on & winners and on & ranked[8], (name, seam)
    corner = {blob_of[p] for p in S.seams(fin)["corner contact"]}
    assert len(corner) == 1 and corner <= winners and corner <= ranked[8] and not corner & ranked[4]      # ranked by K = 8 only
    # ... and that blob's contour has diagonal edges: the diagonal-before-straight half of the rule at bit 63 | 0
    (c,) = [c for c in O.find_contours(fin) if c["start"][1] * S.W + c["start"][0] in corner]
    pts = [tuple(int(v) for v in q) for q in c["points"]]
    assert any(abs(a[0] - b[0]) == 1 and abs(a[1] - b[1]) == 1 for a, b in zip(pts, pts[1:] + pts[:1])), (name, pts)


def test_the_motion_trackers_first_mask_is_the_planted_mask():
    """tests/test_blob_seams_gpu.py plants the cases as the first GREY frame of a motion tracker (every pixel differs from
    nothing): the oracle's mask of that frame is the case itself."""
    for name, m in CASES.items():
        d = O.Diff(S.H, S.W, 100, 0, *S.AREA)
        assert (d.detect(m)[1] == m).all(), name
