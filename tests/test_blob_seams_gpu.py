"""The seam cases (tests/seam_cases.py) through every kernel that applies the shared border rule (blobedges_inline.h), on the GPU:
a plain step (k_blob_lds), a step with targets on (k_merge, k_green_select, k_blob_rank) and one with shapes on as well
(k_blob_shape) -- with one camera, and with two cameras that show different cases in one launch.  Every field is compared bit for
bit with the oracle's contours (targets_cases.reference) and the shape model (shapes_ref.reference) on the case's own mask.

Every blob's record is compared on every path (tests/test_blob_seams_cpu.py says which seam lies on which blob): a plain step hands
out ONE blob, so it runs once per area window of seam_cases.windows(), each blob the only candidate of one of them; the ranked
steps run with K = 4 and with K = 8, which holds all five blobs of a case.

That a plain step of these masks is k_blob_lds' (path == 1 in the device-side result record) is not visible here: the record's
path field is not part of the public position record.  It is blob_load's prediction from the mask (test_blob_seams_cpu.py), the
same prediction tests/test_blob_limits_gpu.py relies on; a step with targets on takes the global kernels by rule."""
import pytest

import seam_cases as S
import shapes_ref as R
import targets_cases as T
from diff_cases import same_dict

pytestmark = pytest.mark.gpu

NAMES = sorted(S.cases())
ORDERS = [NAMES[:1], NAMES[1:], NAMES, NAMES[::-1]]


def _pos_dict(p):
    return dict(valid=p.position_valid, area=p.area, a00=p.a00, a10=p.a10, a01=p.a01, first_pixel=p.first_pixel, x=p.x, y=p.y)


def _tracker(n, area=S.AREA):
    """the batched motion tracker on GREY frames: its first frame is analysed as it is, all n cameras in one launch of each kernel"""
    import oat_amd.components as comp
    return comp.MotionTracker(S.H, S.W, n_streams=n, channels=1, diff_threshold=100, blur=0, area=area)


@pytest.mark.parametrize("order", ORDERS, ids=lambda o: "+".join(o))
def test_seams_on_the_lds_path_every_blob_in_turn(order):
    masks = [S.cases()[name] for name in order]
    n = len(masks)
    windows = sorted({w for m in masks for w in S.windows(S.final(m))})          # (a window of one case may hold nothing of the other)
    compared = [set() for _ in masks]
    for area in windows:
        tr = _tracker(n, area)
        pos = tr.track(masks)
        tr.close()
        for s, m in enumerate(masks):
            want = T.reference(S.final(m), area, 1)[0][0]
            assert same_dict(_pos_dict(pos[s]), want), (order, s, area, pos[s], want)
            if want["valid"]:
                compared[s].add(want["first_pixel"])
    for s, m in enumerate(masks):
        assert compared[s] == {first for first, _ in T.components(S.final(m))}, (order, s)      # every blob has been the winner


@pytest.mark.parametrize("k", S.KS)
@pytest.mark.parametrize("order", ORDERS, ids=lambda o: "+".join(o))
def test_seams_on_the_global_path_and_with_shapes(order, k):
    masks = [S.cases()[name] for name in order]
    n = len(masks)
    want = [T.reference(S.final(m), S.AREA, k) for m in masks]
    shapes = [R.reference(S.final(m), S.AREA, k) for m in masks]
    for with_shapes in (False, True):
        tr = _tracker(n)
        tr.set_targets(k)
        if with_shapes:
            tr.set_target_shapes()
        pos = tr.track(masks)
        (tset,) = tr.targets()
        for s in range(n):
            ranks, n_found = tset[s]
            assert n_found == want[s][1], (order, s, n_found)
            assert same_dict(_pos_dict(pos[s]), want[s][0][0]), (order, s, "targets", pos[s])
            for j in range(k):
                assert same_dict(_pos_dict(ranks[j]), want[s][0][j]), (order, s, j, ranks[j], want[s][0][j])
                if not want[s][0][j]["valid"]:
                    assert not ranks[j].position_valid and ranks[j].first_pixel == -1, (order, s, j)
        if with_shapes:
            (sset,) = tr.target_shapes()
            for s in range(n):
                for j in range(k):
                    got = {f: getattr(sset[s][j], f) for f in R.FIELDS}
                    assert R.same(got, shapes[s][j]), (order, s, j, got, shapes[s][j])
        tr.close()
