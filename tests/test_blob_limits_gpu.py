"""The blob stage at the capacity and geometry limits of its single-workgroup LDS kernel (k_blob_lds), on an MI355X.

Every case of blob_load.edge_cases() lands exactly on one side of a limit of k_blob_lds or k_rowscan (the counts are
checked on the CPU by tests/test_blob_limits_cpu.py); here the detector's result on it must be the CPU oracle's, in an
area window around every blob area of the frame: the largest area, the exact a00 / a10 / a01 sums, the first pixel and
the centroid, on both sides of every limit -- i.e. from k_blob_lds and from the global union-find alike.  The pipelined
layouts (plain speculative order, paired back halves, early dispatch) then get streams at capacity and one over it in the
same step, and the early layout's switch back to speculation is checked step by step.
"""
import numpy as np
import pytest

import blob_load as B
import oracle_lib as O
from test_gpu_parity import _same_detection, _same_state

pytestmark = pytest.mark.gpu

DBL_MAX = float(np.finfo(np.float64).max)


@pytest.fixture(scope="module")
def A():
    import oat_amd
    return oat_amd


def _final(raw, ero, dil):
    f = raw * np.uint8(255)
    if ero:
        f = O.erode(f, ero)
    if dil:
        f = O.dilate(f, dil)
    return f


def _windows(thr):
    """Area windows that pick every group of equal-area blobs on its own, with both window edges ON a blob area:
    [a_i, a_i+1) selects exactly the blobs of area a_i (area >= min_area), [0, a_i) the largest blob below a_i
    (area < max_area); plus the open window."""
    areas = sorted({abs(c["m00"]) for c in O.find_contours(B.frame_zeroed(thr) * np.uint8(255)) if c["m00"] != 0})
    w = [(0.0, DBL_MAX)]
    for i, a in enumerate(areas):
        w.append((a, areas[i + 1] if i + 1 < len(areas) else DBL_MAX))
        w.append((0.0, a))
    return w, areas


# ------------------------------------------------------------------------------- single stage, every edge ---

@pytest.mark.parametrize("name", sorted(B.edge_cases()))
def test_edge_case_single_stage_equals_the_oracle(A, name):
    H, W, ero, dil, build, exp = B.edge_cases()[name]
    img = build() * np.uint8(255)
    thr = _final(img // 255, ero, dil)
    det = A.SimpleThreshold(H, W, thresh=(1, 256), erode=ero, dilate=dil)
    windows, areas = _windows(thr)
    assert areas or name.startswith("height_") and H <= 3, name            # something to select in every case
    for lo, hi in windows:
        det._set(min_area=lo, max_area=hi)
        got = det.detectPosition(img)
        _same_detection(got, O.sift_contours(thr, lo, hi), (name, exp, lo, hi))
    assert (det.read_mask(A.ffi.TAP_MORPH) == thr).all(), name
    det.close()


@pytest.mark.parametrize("name", ["roots_768", "roots_769"])
def test_only_blob_at_max_area_keeps_the_stale_position(A, name):
    """siftContours leaves x / y alone when nothing qualifies (DetectorFunc.cpp:46-62): here the frame's only blob of
    non-zero area has area == max_area (area < max_area is strict), beside hundreds of zero-area contours -- on the LDS
    path (768 components) and on the global one (769).  With min_area == its area the same blob is selected."""
    H, W, ero, dil, build, exp = B.edge_cases()[name]
    img = build() * np.uint8(255)
    thr = _final(img // 255, ero, dil)
    det = A.SimpleThreshold(H, W, thresh=(1, 256))
    pos = det.detectPosition(img)
    _same_detection(pos, O.sift_contours(thr), name)
    assert pos.position_valid and pos.area > 0
    x, y, a = pos.x, pos.y, pos.area
    det._set(min_area=0.0, max_area=a)
    assert not O.sift_contours(thr, 0.0, a)["valid"]
    pos = det.detectPosition(img, pos)
    assert not pos.position_valid and (pos.x, pos.y) == (x, y) and pos.area == 0.0, (name, pos)
    det._set(min_area=a, max_area=DBL_MAX)
    pos = det.detectPosition(img, pos)
    _same_detection(pos, O.sift_contours(thr, a, DBL_MAX), name)
    assert pos.position_valid and pos.area == a
    det.close()


# ------------------------------------------------------------------------------- pipelined layouts ---

WIN = dict(h_thresh=(100, 125), s_thresh=(150, 256), v_thresh=(100, 256))
PARAMS = dict(h_lo=100, h_hi=125, s_lo=150, s_hi=256, v_lo=100, v_hi=256, erode=0, dilate=0, min_area=0.0, max_area=DBL_MAX)
LR = 0.001      # a painted pixel stays foreground for ~100 frames: the threshold masks are exactly the painted masks
AT_EDGE = ("runs_at", "roots_at", "empty")
OVER = ("runs_at", "runs_over", "empty")           # stream 0 at R = 3072, stream 1 at 3073, stream 2 empty: one step
OVER2 = ("roots_over", "runs_at", "roots_at")


class _Painter:
    """BGR frames: a learned grey background with noise, the kind's mask painted in a saturated colour inside the
    HSV window; the oracle's chain follows every stream."""

    def __init__(self, rows, cols, n, seed):
        self.rng = np.random.default_rng(seed)
        self.masks = B.pipeline_masks(rows, cols)
        self.base = self.rng.integers(90, 150, (n, rows, cols, 3)).astype(np.int16)
        self.orc = [O.Mog2(rows, cols, 3) for _ in range(n)]
        self.p = O.hsv_params(**PARAMS)

    def frames(self, kinds):
        f = np.clip(self.base + self.rng.integers(-5, 6, self.base.shape), 0, 255).astype(np.uint8)
        for s, k in enumerate(kinds):
            f[s][self.masks[k][0] != 0] = (255, 64, 0)
        return f

    def check(self, got, f, kinds, tag):
        for s, k in enumerate(kinds):
            want, thr = O.chain_step(self.orc[s], f[s], LR, self.p)
            mask, exp = self.masks[k]
            assert ((thr != 0) == (mask != 0)).all(), (tag, s, k)
            L = B.blob_load(thr)
            assert {q: L[q] for q in exp} == exp, (tag, s, k, L)
            _same_detection(got[s], want, (tag, s, k))


def _steps(n_steps):
    """Warm-up (background only), then at-edge and over-edge steps alternating, each stream changing sides."""
    seq = [("empty",) * 3]
    for t in range(n_steps):
        seq.append((AT_EDGE, OVER, AT_EDGE, OVER2)[t % 4])
    return seq


@pytest.mark.parametrize("fusion,ring", [(1, 3), (1, 4), (2, 4)])
def test_pipelined_streams_at_and_over_capacity_in_one_step(A, fusion, ring):
    """n_streams = 3 on host frames: the plain speculative order (one frame a launch, ring 3 and 4) and the paired
    layout (two frames a launch: one row-scan and one k_blob_lds launch for both).  Declined frames are repaired by
    the global kernels, the full launch sequence runs until the LDS kernel has taken 16 steps in a row."""
    rows, cols, n = B.PIPELINE_SHAPES[0][0], B.PIPELINE_SHAPES[0][1], 3
    pt = _Painter(rows, cols, n, 40 + fusion * 7 + ring)
    hp = A.HotPath(rows, cols, n_streams=n, ring_depth=ring, adaptation_coeff=LR, erode=0, dilate=0, area=(0.0, DBL_MAX), **WIN)
    hp.set_fusion(fusion)
    seq = _steps(13)
    frames = [pt.frames(k) for k in seq]
    got = []
    for f in frames:
        hp.enqueue(list(f))
        if hp.outstanding() >= ring:
            got.append(hp.collect())
    while hp.outstanding():
        got.append(hp.collect())
    assert len(got) == len(frames)
    for t, (f, kinds) in enumerate(zip(frames, seq)):
        pt.check(got[t], f, kinds, (fusion, ring, t))
    for s in range(n):
        _same_state(hp.mog_state(s), pt.orc[s].state(), s)
    assert hp.last_step_shape()[1] is False
    hp.close()


def test_early_layout_at_capacity_and_one_over(A):
    """The early layout (3 x 1080p = 6.2 MP a step, device frames: each step's k_blob_lds workgroups are parked ahead of
    their row scans).  A step whose frames are all at capacity keeps the next step early; a declined frame is repaired
    when it is collected, which clears the speculation (oatgpu_track_collect -> launch_repair): the steps launched after
    that take the plain order in the full launch sequence until kSpecAfter = 16 collected steps in a row were all taken by
    the LDS kernel.  A frame enqueued with nothing outstanding takes the plain order too (lone_plain).  The expected path
    of every step follows that rule; every result, and the model, is the oracle's."""
    import torch
    rows, cols, n = B.PIPELINE_SHAPES[1][0], B.PIPELINE_SHAPES[1][1], 3
    pt = _Painter(rows, cols, n, 77)
    hp = A.HotPath(rows, cols, n_streams=n, ring_depth=4, adaptation_coeff=LR, erode=0, dilate=0, area=(0.0, DBL_MAX), **WIN)
    seq = [("empty",) * 3, AT_EDGE, AT_EDGE, OVER] + [AT_EDGE] * 17 + [OVER2, AT_EDGE, AT_EDGE]
    spec_after = 16
    spec, streak, outstanding = True, 0, []
    frames, got, early, want_early = [], [], [], []

    def collect():
        nonlocal spec, streak
        got.append(hp.collect())
        kinds = seq[outstanding.pop(0)]
        if any(pt.masks[k][1]["path"] == "global" for k in kinds):
            spec, streak = False, 0
        else:
            streak += 1
            if streak >= spec_after:
                spec = True
    for t, kinds in enumerate(seq):
        f = pt.frames(kinds)
        d = torch.from_numpy(f).cuda()
        torch.cuda.synchronize()
        frames.append(f)
        want_early.append(spec and bool(outstanding))
        hp.enqueue_dev(d.data_ptr(), keepalive=d)
        outstanding.append(t)
        early.append(hp.last_step_shape()[1])
        if len(outstanding) >= 2:
            collect()
    while outstanding:
        collect()
    assert hp.early_blob_timeouts() == 0
    assert early == want_early, list(zip(early, want_early))
    assert sum(early) >= 4 and not all(early[1:])
    for t, (f, kinds) in enumerate(zip(frames, seq)):
        pt.check(got[t], f, kinds, ("early", t))
    for s in range(n):
        _same_state(hp.mog_state(s), pt.orc[s].state(), s)
    hp.close()
