"""GPU tests of the order in which the target family and the batched trackers are switched on: a tracker that is
switched on while targets, shapes, crops, tracks and a crop tensor are on builds every set that stands beside its slots itself, and a
setter of the family starts every delivered list over.  Expected values are the models' of tests/test_crops_gpu.py,
tests/test_tracks_gpu.py and tests/test_crop_tensor_gpu.py on crops_cases' sequences, never a second context's.  Every frame is
under 0.004 MP."""
import ctypes as C

import numpy as np
import pytest

import crop_tensor_cases as XC
import crops_cases as CC
import targets_cases as T
import tracks_cases as TC
import tracks_ref as TR
from test_crop_tensor_gpu import _host, _kw
from test_crop_tensor_gpu import _same as _same_bits
from test_crops_gpu import A, _check_crops, _check_model_inputs, _dev, _frames_at, _make_tracker, _refused      # noqa: F401
from test_tracks_gpu import _check_camera

pytestmark = pytest.mark.gpu

ROWS, COLS, N, K, H, W = 48, 64, 3, 3, 8, 8
CAPACITY, ZOOM, FMT = 3, 2.0, XC.FORMATS[3]
SWITCH = dict(motion="oatgpu_set_diff_tracker", subtraction="oatgpu_set_bsub_tracker")
OTHER = dict(motion="subtraction", subtraction="motion")


def _switch(tr, family, on):
    tr._chk(getattr(tr.lib, SWITCH[family])(tr.ctx, int(on)))


def _riders_on(tr):
    """targets, shapes, axis crops, tracks and an axis crop tensor -> the tensor"""
    tr.set_targets(K)
    tr.set_target_shapes()
    tr.set_target_crops(H, W, axis=True)
    tr.set_tracks(**TC.image_config())
    return tr.set_target_crop_tensor(H, W, axis=True, zoom=ZOOM, capacity=CAPACITY, **_kw(FMT, 3))


class _Models:
    """what the readers of a call that delivered frames t0 .. t0 + count - 1 of `family` must hand out; the tracks' model runs on"""

    def __init__(self, family):
        self.family = family
        self.cams = [TR.Camera(K, TC.IMG_KALMAN, TC.IMG_GATE) for _ in range(N)]

    def check(self, tr, tensor, t0, count):
        fam = self.family
        tgt, shp, crp, trk, view = tr.targets(), tr.target_shapes(), tr.target_crops(), tr.tracks(), tr.target_crop_tensor()
        assert len(tgt) == len(shp) == len(crp) == len(trk) == len(view) == count, (fam, t0, count)
        assert view.data_ptr() == tensor.data_ptr()
        got = _host(view)
        for i in range(count):
            t = t0 + i
            _check_model_inputs(tgt[i], shp[i], fam, ROWS, COLS, N, t, 0.0, K)
            _check_crops(crp[i], fam, ROWS, COLS, N, t, 0.0, K, True, H, W)
            for s in range(N):
                ranks, _ = CC.sequence_targets(fam, ROWS, COLS, CC.variant_of(s), 0.0, K)[t]
                _check_camera(trk[i][s], self.cams[s].step(TC.triples(ranks)), (fam, t, s))
            want = XC.expected(XC.entry_u8(fam, ROWS, COLS, N, t, 0.0, K, True, ZOOM, H, W), FMT, 3)
            _same_bits(got[i], want, (fam, t))


@pytest.mark.parametrize("family", ["motion", "subtraction"])
def test_a_tracker_switched_off_and_on_again_behind_every_rider(A, family):
    tr = _make_tracker(A, family, ROWS, COLS, N)
    tensor = _riders_on(tr)
    _switch(tr, family, 0)
    _switch(tr, family, 1)                             # its sets are the tracker's own alloc's now
    models = _Models(family)
    tr.track(_frames_at(family, ROWS, COLS, N, 0))
    models.check(tr, tensor, 0, 1)
    bufs = [_dev(_frames_at(family, ROWS, COLS, N, t), 1) for t in (1, 2, 3)]
    tr.track_sequence_dev([b[1] for b in bufs])
    models.check(tr, tensor, 1, 3)
    tr.close()


@pytest.mark.parametrize("family", ["motion", "subtraction"])
def test_the_second_tracker_switched_on_last(A, family):
    """`family` is the tracker that comes last, on a context built for the other one, through its raw entry points."""
    from oat_amd import ffi
    win = T.sub_window()
    if family == "subtraction":
        tr = _make_tracker(A, "motion", ROWS, COLS, N)
        tr._set(h_lo=win["h"][0], h_hi=win["h"][1], s_lo=win["s"][0], s_hi=win["s"][1], v_lo=win["v"][0], v_hi=win["v"][1],
                erode=T.SUB_MORPH[0], dilate=T.SUB_MORPH[1])          # (the motion tracker looks at none of these)
    else:
        tr = A.SubtractionTracker(ROWS, COLS, n_streams=N, channels=3, alpha=0.0, h_thresh=win["h"], s_thresh=win["s"], v_thresh=win["v"],
                                  erode=T.SUB_MORPH[0], dilate=T.SUB_MORPH[1], area=T.AREA, **T.DIFF)
    tensor = _riders_on(tr)
    _switch(tr, family, 1)
    models = _Models(family)
    frames = _frames_at(family, ROWS, COLS, N, 0)
    ptrs = (ffi._u8p * N)(*[ffi.u8(f) for f in frames])
    pos = (ffi.Position * (3 * N))()
    if family == "subtraction":
        tr._chk(tr.lib.oatgpu_bsub_track_batch(tr.ctx, ptrs, N, 0.0, pos))
    else:
        tr._chk(tr.lib.oatgpu_diff_batch(tr.ctx, ptrs, N, pos))
    models.check(tr, tensor, 0, 1)
    bufs = [_dev(_frames_at(family, ROWS, COLS, N, t), 1) for t in (1, 2, 3)]
    arr = (C.c_void_p * 3)(*[b[1] for b in bufs])
    if family == "subtraction":
        tr._chk(tr.lib.oatgpu_bsub_track_sequence_dev(tr.ctx, arr, 3, 0.0, pos))
    else:
        tr._chk(tr.lib.oatgpu_diff_sequence_dev(tr.ctx, arr, 3, pos))
    models.check(tr, tensor, 1, 3)
    tr.close()


def test_setters_start_the_lists_over_and_other_calls_deliver_no_crops(A):
    from oat_amd import ffi
    family = "motion"
    tr = _make_tracker(A, family, ROWS, COLS, N)
    tensor = _riders_on(tr)
    models = _Models(family)
    frames = [_frames_at(family, ROWS, COLS, N, t) for t in range(4)]
    tr.track(frames[0])
    models.check(tr, tensor, 0, 1)
    tr.set_target_shapes(True)                         # ... empties targets() too
    assert "no call has delivered" in _refused(tr.targets)
    assert "no call has delivered" in _refused(tr.target_shapes)
    tr.track(frames[1])
    models.check(tr, tensor, 1, 1)
    tr.set_target_crops(H, W, axis=True)
    assert "no call has delivered" in _refused(tr.targets)
    assert "no call has delivered" in _refused(tr.target_shapes)
    assert "no call has delivered a crop set" in _refused(tr.target_crops)
    tr.track(frames[2])
    models.check(tr, tensor, 2, 1)
    # the fused tracker's call on this context: targets and shapes, no crop set, no tensor entry
    ptrs = (ffi._u8p * N)(*[ffi.u8(f) for f in frames[3]])
    pos = (ffi.Position * N)()
    tr._chk(tr.lib.oatgpu_track_batch(tr.ctx, ptrs, N, 0.0, pos))
    assert len(tr.targets()) == 1 and len(tr.target_shapes()) == 1
    assert "no call has delivered a crop set since target crops were switched on" in _refused(tr.target_crops)
    assert "no call has delivered a crop tensor entry since crop tensors were switched on" in _refused(tr.target_crop_tensor)
    tr.track(frames[3])
    models.check(tr, tensor, 3, 1)
    # ... and a single-stage detector's: the planted mask's ranks in its one stream
    case = next(c for c in T.planted_cases() if c.name == "ties-48x64")
    tr._set(h_lo=255, h_hi=256, min_area=case.area[0], max_area=case.area[1])
    p = ffi.Position()
    tr._chk(tr.lib.oatgpu_detect_thresh(tr.ctx, 1, ffi.u8(case.img), C.byref(p)))
    (tset,) = tr.targets()
    ranks, found = T.planted_reference(case.name, (0, 0), K)
    assert tset[1][1] == found and tset[0][1] == 0 and tset[2][1] == 0
    for g, r in zip(tset[1][0], ranks):
        assert (g.position_valid, g.x, g.y, g.area) == (r["valid"], r["x"], r["y"], r["area"]), (g, r)
    assert len(tr.target_shapes()) == 1
    assert "no call has delivered a crop set since target crops were switched on" in _refused(tr.target_crops)
    assert "no call has delivered a crop tensor entry since crop tensors were switched on" in _refused(tr.target_crop_tensor)
    tr.close()
