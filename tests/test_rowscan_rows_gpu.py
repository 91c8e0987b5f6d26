"""Rows a row-scan workgroup (k_rowscan's ROWS: 4, or 16 on a step launched deep in the pipeline), on an MI355X.

Nothing a row writes depends on the height of its workgroup, so a context forced to the wide form, one forced to the narrow
form and the oracle must agree bit for bit: every frame's detection, the MORPH and FINAL taps of the last frame and every
stream's whole model.  The cases sit where the wide form's row groups, LDS rows and shortcut windows differ from the narrow
form's: one group, a last group one row short / full / one row over, three groups; rows one word past the 64-word chunk; the
erode / dilate sizes that move the LDS window and the shortcut's source-row range [ya, yb) past both ends of the frame.
Then the rule that picks the height (plan_step): the LDS edge, the pipeline depth, and a declined frame inside a wide step.
oatgpu_early_blob_timeouts() stays 0 throughout."""
import numpy as np
import pytest

import blob_load as B
import morph_cases as M
from test_blob_limits_gpu import AT_EDGE, LR as BLOB_LR, OVER, WIN, _Painter
from test_gpu_parity import _same_state
from test_morph_routes_gpu import _dets, _early_min_px, _hot, _sequence, _taps

pytestmark = pytest.mark.gpu

DBL_MAX = float(np.finfo(np.float64).max)
NARROW, WIDE = M.RS_ROWS, 16                              # kRsRowsNarrow, kRsRowsDeep
W65 = M.CHUNK_GEOMS[1][1]                                 # 65 words a row: one past the row scan's chunk
SIZES = ((0, 0), (2, 0), (4, 4), (31, 33), (63, 0), (0, 63))
HEIGHTS = (3, 15, 16, 17, 33)                             # groups of 16: one; short by 1 / full / over by 1; three


@pytest.fixture(scope="module")
def A():
    import oat_amd
    return oat_amd


def wide_lds_bytes(W, dil, rows=WIDE):
    """rowscan_lds_bytes_rows(): (rows + max(dil, 1) - 1) eroded rows of 8-byte words."""
    return (rows + (dil if dil > 1 else 1) - 1) * M.words(W) * 8


def _masks(H, W, e, d):
    """masks[t][s]: the background, a dense mask, an impulse at (H - 2, W - 1), another dense mask (whole pairs)."""
    kinds = (("dense", 3), ("impulse", (H - 2, W - 1)), ("dense", 4))
    cases = [M.Case("rows", "chunk", H, W, e, d, k, a, False) for k, a in kinds]
    return [[np.zeros((H, W), np.uint8)] * 3] + [[M.build(c, s) for s in range(3)] for c in cases]


def _through_sequence(A, geom, seq, rows, ring=4):
    """The frames through track_sequence_dev (two frames a launch) of a fresh context set to `rows`; everything against the
    oracle.  Returns (rows of the last step, was it dispatched early)."""
    import torch
    H, W, e, d = geom
    frames, want, states = seq
    hp = _hot(A, H, W, e, d, 1, ring=ring)
    try:
        hp.set_rowscan_rows(rows)
        dev = [torch.from_numpy(f).cuda() for f in frames]
        torch.cuda.synchronize()
        got = hp.track_sequence_dev([x.data_ptr() for x in dev])
        for t in range(len(frames)):
            _dets(got[t], want[t], (geom, rows, t))
        _taps(A, hp, want[-1], (geom, rows, "last"))
        for s in range(3):
            _same_state(hp.mog_state(s), states[s], s)
        assert hp.early_blob_timeouts() == 0
        return hp.last_step_rowscan_rows(), hp.last_step_shape()[1]
    finally:
        hp.close()


def _shortcut_window(H, e, d, rows):
    """[lo, hi) before clipping: the first group's ya and the last group's yb (k_rowscan<true>)."""
    dk = d if d > 1 else 1
    lo = -(dk // 2) - e // 2
    r0 =(-(-H // rows) - 1) * rows - dk // 2
    return lo, r0 + (rows + dk - 1) - e // 2 + e - 1


@pytest.mark.parametrize("sizes", SIZES, ids=lambda v: "e%dd%d" % v)
@pytest.mark.parametrize("H", HEIGHTS)
def test_paired_order_wide_narrow_and_oracle(A, H, sizes):
    """The paired back half (grid z = 2) forced to 16 rows and to 4, three GREY streams."""
    e, d = sizes
    assert wide_lds_bytes(W65, d) <= M.ROWSCAN_LDS_MAX and not M.ero_apart(H, W65, e, d)
    if e > 1:                       # the shortcut's source rows reach above row 0 and to the last row or below it
        lo, hi = _shortcut_window(H, e, d, WIDE)
        assert lo < 0 and hi >= H, (lo, hi)
    geom = (H, W65, e, d)
    seq = _sequence(H, W65, e, d, 1, _masks(H, W65, e, d), 31)
    assert _through_sequence(A, geom, seq, WIDE) == (WIDE, False)
    assert _through_sequence(A, geom, seq, NARROW) == (NARROW, False)


@pytest.mark.parametrize("sizes", SIZES, ids=lambda v: "e%dd%d" % v)
def test_early_order_wide_narrow_and_oracle(A, sizes):
    """The early order (launch_rowscan_signal, parked blob workgroups) at the smallest step it admits."""
    e, d = sizes
    H = -(-_early_min_px() // (3 * M.words(W65) * 64))
    assert 3 * H * M.words(W65) * 64 >= _early_min_px() > 3 * (H - 1) * M.words(W65) * 64
    assert H % WIDE not in (0, WIDE - 1) and wide_lds_bytes(W65, d) <= M.ROWSCAN_LDS_MAX
    if e > 1:
        lo, hi = _shortcut_window(H, e, d, WIDE)
        assert lo < 0 and hi > H, (lo, hi)
    geom = (H, W65, e, d)
    seq = _sequence(H, W65, e, d, 1, _masks(H, W65, e, d), 37)
    assert _through_sequence(A, geom, seq, WIDE) == (WIDE, True)
    assert _through_sequence(A, geom, seq, NARROW) == (NARROW, True)


def test_lds_edge_forced_wide_falls_back_to_narrow(A):
    """Dilate 63: the widest row whose 16 + 62 eroded rows fit the row scan's LDS takes the wide form; one word more and a
    context forced to wide takes the narrow one, still fused (the narrow form's LDS fits: the erosion is not apart)."""
    H, e, d = M.LDS_H, 3, 63
    fits = M.ROWSCAN_LDS_MAX // ((WIDE + d - 1) * 8) * M.WORD
    over = fits + M.WORD
    assert wide_lds_bytes(fits, d) <= M.ROWSCAN_LDS_MAX < wide_lds_bytes(over, d)
    assert M.rowscan_lds_bytes(H, over, d) <= M.ROWSCAN_LDS_MAX and not M.ero_apart(H, over, e, d)
    for W, rows in ((over, NARROW), (fits, WIDE)):
        seq = _sequence(H, W, e, d, 1, _masks(H, W, e, d), 41)
        assert _through_sequence(A, (H, W, e, d), seq, WIDE) == (rows, False), W


def test_depth_rule_picks_the_height(A):
    """Default settings.  Two frames a launch on a ring of 8: the steps launched with 0 and 2 frames ahead of them take 4
    rows, every later one (4, then 6 ahead) 16; the same frames through a ring of 4 and one frame at a time: 4 throughout.
    Every route gives the oracle's results and models."""
    import torch
    H, W, e, d, T = 33, 129, 4, 4, 16
    masks = [[np.zeros((H, W), np.uint8)] * 3]
    masks += [[M.build(M.Case("depth", "word", H, W, e, d, "dense", 10 + t, False), s) for s in range(3)] for t in range(T - 1)]
    seq = _sequence(H, W, e, d, 1, masks, 43)
    frames, want, states = seq

    def loop(ring, fusion):
        """What track_sequence_dev does, call by call: (rows after every launch, results)."""
        hp = _hot(A, H, W, e, d, 1, ring=ring)
        try:
            if fusion == 2:
                hp.set_fusion(2)
            dev = [torch.from_numpy(f).cuda() for f in frames]
            torch.cuda.synchronize()
            rows, got = [], []
            for t in range(T):
                if hp.outstanding() == (ring if fusion == 2 else 1):
                    got.append(hp.collect())
                hp.enqueue_dev(dev[t].data_ptr(), keepalive=dev[t])
                if fusion == 1 or t % 2:
                    rows.append(hp.last_step_rowscan_rows())
            while hp.outstanding():
                got.append(hp.collect())
            for t in range(T):
                _dets(got[t], want[t], ("loop", ring, fusion, t))
            _taps(A, hp, want[-1], ("loop", ring, fusion))
            for s in range(3):
                _same_state(hp.mog_state(s), states[s], s)
            assert hp.early_blob_timeouts() == 0
            return rows
        finally:
            hp.close()

    assert loop(8, 2) == [NARROW, NARROW] + [WIDE] * (T // 2 - 2)
    assert loop(4, 2) == [NARROW] * (T // 2)
    assert loop(8, 1) == [NARROW] * T
    # ... and the sequence call itself: its last step is the loop's last step
    assert _through_sequence(A, (H, W, e, d), seq, 0, ring=8) == (WIDE, False)
    assert _through_sequence(A, (H, W, e, d), seq, 0, ring=4) == (NARROW, False)


def test_declined_frame_in_a_wide_step(A):
    """A stream over the LDS kernel's run capacity in a step forced wide: k_blob_lds declines it, the global kernels redo the
    frame in the repair set when it is collected, and the result is the oracle's."""
    import torch
    rows, cols, n = B.PIPELINE_SHAPES[0][0], B.PIPELINE_SHAPES[0][1], 3
    pt = _Painter(rows, cols, n, 59)
    assert pt.masks["runs_over"][1]["path"] == "global" and B.over_run_capacity(pt.masks["runs_over"][0] * np.uint8(255))
    hp = A.HotPath(rows, cols, n_streams=n, ring_depth=4, adaptation_coeff=BLOB_LR, erode=0, dilate=0, area=(0.0, DBL_MAX), **WIN)
    try:
        hp.set_rowscan_rows(WIDE)
        seq = [("empty",) * 3, AT_EDGE, OVER, AT_EDGE]
        frames = [pt.frames(k) for k in seq]
        dev = [torch.from_numpy(f).cuda() for f in frames]
        torch.cuda.synchronize()
        got = hp.track_sequence_dev([x.data_ptr() for x in dev])
        assert hp.last_step_rowscan_rows() == WIDE and hp.last_step_shape()[1] is False
        for t, (f, kinds) in enumerate(zip(frames, seq)):
            pt.check(got[t], f, kinds, ("declined", t))
        for s in range(n):
            _same_state(hp.mog_state(s), pt.orc[s].state(), s)
        assert hp.early_blob_timeouts() == 0
    finally:
        hp.close()
