"""The bit-packed morphology on every launch route, on an MI355X: the cases of tests/morph_cases.py (checked on the CPU
by tests/test_morph_cases_cpu.py: they straddle the word, row-group, chunk and LDS-budget edges and tell wrong anchors,
borders and windows apart) through

  * the single stage (`posidet thresh` with three streams, `posidet hsv`): k_rowscan<false> (dilate_word), k_rowscan<true>
    (erode_word -> LDS -> dilate_word_lds), k_morph with blockIdx.y > 0, H <= 2;
  * `posidet diff`, whose blur is a dilation;
  * the fused tracker: the synchronous step, the plain speculative order, the paired back half (grid z = 2) from host frames
    and from the sequence call, the early order;
  * the marker sets: marker by marker, the table kernel (k_rowscan<true, true>) with one and two frames a launch, and the
    marker-by-marker fallback of the pipelined path.

Every comparison is bit for bit: the MORPH tap against the oracle's erode -> dilate of the KNOWN input, the FINAL tap
against that with the image frame zeroed, the detection against O.sift_contours of it.  There are no tolerances here
but the project's centroid bar inside _same_detection."""
import os
import re

import numpy as np
import pytest

import blob_load as B
import morph_cases as M
import oracle_lib as O
from test_gpu_parity import _same_detection, _same_state

pytestmark = pytest.mark.gpu

DBL_MAX = float(np.finfo(np.float64).max)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def A():
    import oat_amd
    return oat_amd


def _morph(img, e, d):
    if e:
        img = O.erode(img, e)
    if d:
        img = O.dilate(img, d)
    return img


def _final(morph):
    return B.frame_zeroed(morph) * np.uint8(255)


# --------------------------------------------------------------------------------------------- single stage ---

GEOMS = M.geometries()


@pytest.mark.parametrize("geom", sorted(GEOMS), ids=lambda g: f"{g[0]}x{g[1]}")
def test_single_stage_every_case_three_streams(A, geom):
    """One context a geometry, sizes switched with _set; every stream has its own input and its own taps."""
    H, W = geom
    det = A.SimpleThreshold(H, W, thresh=(1, 256), n_streams=3)
    hsv = A.HSVDetector(H, W, h_thresh=(0, 256), s_thresh=(0, 256), v_thresh=(1, 256), erode=0, dilate=0, n_streams=3)
    try:
        for i, c in enumerate(GEOMS[geom]):
            det._set(erode=c.e, dilate=c.d)
            imgs = [M.build(c, s) for s in range(3)]
            want = [_morph(m, c.e, c.d) for m in imgs]
            got = [det.detectPosition(imgs[s], stream=s) for s in range(3)]
            for s in range(3):
                assert (det.read_mask(A.ffi.TAP_MORPH, s) == want[s]).all(), (c.name, s, M.route(H, W, c.e, c.d))
                assert (det.read_mask(A.ffi.TAP_FINAL, s) == _final(want[s])).all(), (c.name, s)
                _same_detection(got[s], O.sift_contours(want[s]), (c.name, s))
            if i % 3 == 0 and (H != M.LDS_H or i == 0):      # the thinner pass: inRange on 3-channel input in front
                hsv._set(erode=c.e, dilate=c.d)
                got = [hsv.detectPosition(np.repeat(imgs[s][:, :, None], 3, axis=2), stream=s) for s in (2, 0, 1)]
                for k, s in enumerate((2, 0, 1)):
                    assert (hsv.read_mask(A.ffi.TAP_MORPH, s) == want[s]).all(), (c.name, s, "hsv")
                    _same_detection(got[k], O.sift_contours(want[s]), (c.name, s, "hsv"))
    finally:
        det.close()
        hsv.close()


# ------------------------------------------------------------------------------------------------ posidet diff ---

@pytest.mark.parametrize("cols", [64, 65, 129])
@pytest.mark.parametrize("blur", [2, 3, 21, 22])
def test_posidet_diff_blur_at_word_edges(A, blur, cols):
    """test_posidet_diff_parity's comparison (the outermost ring is excluded as there: the reference blurs with a
    reflected border, which a dilation reproduces everywhere but on the ring) at word-edge widths, two streams."""
    rows, n = 24, 2
    rng = np.random.default_rng(100 * blur + cols)
    det = A.DifferenceDetector(rows, cols, diff_threshold=12, blur=blur, area=(2.0, 1e6), n_streams=n)
    orcs = [O.Diff(rows, cols, 12, blur, 2.0, 1e6) for _ in range(n)]
    base = [rng.integers(40, 90, (rows, cols)).astype(np.int16) for _ in range(n)]
    hits = 0
    try:
        for t in range(8):
            for s in range(n):
                f = np.clip(base[s] + rng.integers(-4, 5, (rows, cols)), 0, 255).astype(np.uint8)
                x, y = (5 + 9 * t + 20 * s) % (cols - 4), 2 + 2 * t
                f[y:y + 5, x:x + 6] = 220                      # a block that moves across the word edge ...
                f[rows - 3 - t % 2:rows - 1, cols - 3:cols] = 220 if t % 2 else 60      # ... and one in the last word's last pixels
                got = det.detectPosition(f, stream=s)
                want, thr = orcs[s].detect(f)
                if t > 0:
                    assert ((det.read_mask(1, s) > 0)[1:-1, 1:-1] == (thr > 0)[1:-1, 1:-1]).all(), (t, s)
                _same_detection(got, want, (t, s))
                hits += got.position_valid
        assert hits >= 10
    finally:
        det.close()


# ---------------------------------------------------------------------------------------------- fused tracker ---

LR = 0.001      # a painted pixel stays foreground for ~100 frames: the threshold masks are exactly the painted masks
BGR_WIN = dict(h_thresh=(100, 125), s_thresh=(150, 256), v_thresh=(100, 256))
BGR_P = dict(h_lo=100, h_hi=125, s_lo=150, s_hi=256, v_lo=100, v_hi=256)
GREY_WIN = dict(h_thresh=(200, 256))
GREY_P = dict(h_lo=200, h_hi=256)
_SEQ = {}


def _sequence(H, W, e, d, ch, masks, seed):
    """Frames for 3 streams -- a learned grey background with noise, masks[t][s] painted in a colour inside the window --
    and what the oracle's chain makes of them, once per distinct input: (frames[t] (3, H, W[, 3]), want[t][s] = (morph,
    detection), final model states).  The oracle's RAW threshold must be the painted mask."""
    key = (H, W, e, d, ch, seed, len(masks))
    if key in _SEQ:
        return _SEQ[key]
    rng = np.random.default_rng(seed)
    shape = (3, H, W, 3) if ch == 3 else (3, H, W)
    base = rng.integers(90, 150, shape).astype(np.int16)
    kw = dict(BGR_P if ch == 3 else GREY_P, min_area=0.0, max_area=DBL_MAX)
    p, p_raw = O.hsv_params(erode=e, dilate=d, **kw), O.hsv_params(erode=0, dilate=0, **kw)
    orc = [O.Mog2(H, W, ch) for _ in range(3)]
    raw = [O.Mog2(H, W, ch) for _ in range(3)]
    frames, want = [], []
    for t, ms in enumerate(masks):
        f = np.clip(base + rng.integers(-5, 6, shape), 0, 255).astype(np.uint8)
        row = []
        for s in range(3):
            f[s][ms[s] != 0] = (255, 64, 0) if ch == 3 else 230
            det, thr = O.chain_step(orc[s], f[s], LR, p)
            assert ((O.chain_step(raw[s], f[s], LR, p_raw)[1] != 0) == (ms[s] != 0)).all(), ("raw", t, s)
            if H * W <= 20000:                               # (large frames: the chain's own erode / dilate of that raw mask)
                assert (thr == _morph(np.where(ms[s] != 0, 255, 0).astype(np.uint8), e, d)).all(), ("oracle chain", t, s)
            row.append((thr, det))
        frames.append(f)
        want.append(row)
    _SEQ[key] = (frames, want, [o.state() for o in orc])
    return _SEQ[key]


def _hot(A, H, W, e, d, ch, ring=4):
    win = BGR_WIN if ch == 3 else GREY_WIN
    return A.HotPath(H, W, n_streams=3, channels=ch, ring_depth=ring, adaptation_coeff=LR, erode=e, dilate=d,
                     area=(0.0, DBL_MAX), **win)


def _taps(A, hp, row, tag):
    for s in range(3):
        assert (hp.read_mask(A.ffi.TAP_MORPH, s) == row[s][0]).all(), (tag, s, "morph")
        assert (hp.read_mask(A.ffi.TAP_FINAL, s) == _final(row[s][0])).all(), (tag, s, "final")


def _dets(got, row, tag):
    for s in range(3):
        _same_detection(got[s], row[s][1], (tag, s))


def _set_masks(H, W, e, d, lead):
    """masks[t][s]: `lead` empty frames (the background; one more moves every case to the other place of a pair), then the
    set's cases in table order, every stream its own input."""
    cases = [c for c in M.PIPELINED if (c.H, c.W, c.e, c.d) == (H, W, e, d)]
    assert len(cases) >= 3
    blank = [np.zeros((H, W), np.uint8)] * 3
    return [blank] * lead + [[M.build(c, s) for s in range(3)] for c in cases]


# GREY and BGR at every set but the two 12 x 8000-pixel ones, which take one each
FUSED = [(p, ch) for i, p in enumerate(M.PIPE_SETS) for ch in (1, 3) if p[0] != M.LDS_H or ch == (1, 3)[i % 2]]


@pytest.mark.parametrize("pset,ch", FUSED, ids=lambda v: "%dx%d-e%dd%d" % v if isinstance(v, tuple) else ("grey", "", "bgr")[v - 1])
def test_fused_tracker_synchronous_and_pipelined(A, pset, ch):
    """track; enqueue / collect with set_fusion(1) (a lone frame's inline back half, then the plain speculative order);
    set_fusion(2) on host frames and track_sequence_dev (two frames a launch: the paired back half wherever the erosion is
    fused -- plan_step does not pair a step whose erosion is apart, which has no public observable: those sets run the same
    calls and must give the same results).  The taps are those of the latest launched frame: with two frames out, the
    second one's; every sequence runs twice, the second time behind one more background frame, so that every case is
    once the first and once the second of a pair."""
    import torch
    H, W, e, d = pset
    for lead in (1, 2):
        masks = _set_masks(H, W, e, d, lead)
        if len(masks) % 2:
            masks.append(masks[lead])                          # an even count: whole pairs
        frames, want, states = _sequence(H, W, e, d, ch, masks, 7 * lead + ch)
        T = len(frames)
        # the synchronous step
        hp = _hot(A, H, W, e, d, ch)
        try:
            for t in range(T):
                _dets(hp.track(list(frames[t])), want[t], ("track", lead, t))
                _taps(A, hp, want[t], ("track", lead, t))
            for s in range(3):
                _same_state(hp.mog_state(s), states[s], s)
        finally:
            hp.close()
        # two frames out at a time, host frames: one frame a launch, then two frames a launch
        for fusion in (1, 2):
            hp = _hot(A, H, W, e, d, ch)
            try:
                hp.set_fusion(fusion)
                hp.profile(1)
                for t in range(0, T, 2):
                    hp.enqueue(list(frames[t]))
                    hp.enqueue(list(frames[t + 1]))
                    _taps(A, hp, want[t + 1], ("fusion", fusion, lead, t + 1))
                    _dets(hp.collect(), want[t], ("fusion", fusion, lead, t))
                    _dets(hp.collect(), want[t + 1], ("fusion", fusion, lead, t + 1))
                prof = hp.profile_read()
                assert prof["steps"] > 0 and prof["mog_frames"] == fusion * prof["steps"], (fusion, prof)
                assert hp.last_step_shape()[1] is False
                for s in range(3):
                    _same_state(hp.mog_state(s), states[s], s)
            finally:
                hp.close()
        # the sequence call on device frames
        hp = _hot(A, H, W, e, d, ch)
        try:
            hp.set_fusion(2)
            hp.profile(1)
            dev = [torch.from_numpy(f).cuda() for f in frames]
            torch.cuda.synchronize()
            got = hp.track_sequence_dev([x.data_ptr() for x in dev])
            for t in range(T):
                _dets(got[t], want[t], ("sequence", lead, t))
            _taps(A, hp, want[T - 1], ("sequence", lead, T - 1))
            prof = hp.profile_read()
            assert prof["mog_frames"] == 2 * prof["steps"] > 0, prof
            for s in range(3):
                _same_state(hp.mog_state(s), states[s], s)
        finally:
            hp.close()


# ------------------------------------------------------------------------------------------------- early order ---

def _early_min_px():
    with open(os.path.join(ROOT, "oat_amd", "csrc", "oatgpu_ctx.h")) as f:
        return int(re.search(r"size_t early_min_px = (\d+);", f.read()).group(1))


@pytest.mark.parametrize("sizes", [(4, 4), (31, 33)], ids=["even", "large-odd"])
def test_early_order_at_the_smallest_step_it_admits(A, sizes):
    """Three streams of GREY device frames, 65 words a row (one word past the row scan's chunk), as few rows as make a step of
    early_min_px padded pixels: every step enqueued with a step outstanding takes the early order (launch_rowscan_signal)."""
    import torch
    e, d = sizes
    W = M.CHUNK_GEOMS[1][1]
    H = -(-_early_min_px() // (3 * M.words(W) * 64))
    assert 3 * H * M.words(W) * 64 >= _early_min_px() > 3 * (H - 1) * M.words(W) * 64
    kinds = (("dense", 3), ("impulse", (H - 2, W - 1)))
    cases = [M.Case("early", "chunk", H, W, e, d, k, a, False) for k, a in kinds]
    masks = [[np.zeros((H, W), np.uint8)] * 3] + [[M.build(c, s) for s in range(3)] for c in cases]
    frames, want, states = _sequence(H, W, e, d, 1, masks, 5)
    hp = _hot(A, H, W, e, d, 1)
    try:
        early, got, out = [], [], 0
        for t, f in enumerate(frames):
            dv = torch.from_numpy(f).cuda()
            torch.cuda.synchronize()
            hp.enqueue_dev(dv.data_ptr(), keepalive=dv)
            out += 1
            early.append(hp.last_step_shape()[1])
            if out >= 2:
                got.append(hp.collect())
                out -= 1
        _taps(A, hp, want[-1], ("early", "last"))
        while out:
            got.append(hp.collect())
            out -= 1
        assert early == [False] + [True] * (len(frames) - 1), early
        assert hp.early_blob_timeouts() == 0
        for t in range(len(frames)):
            _dets(got[t], want[t], ("early", t))
        for s in range(3):
            _same_state(hp.mog_state(s), states[s], s)
    finally:
        hp.close()


# ------------------------------------------------------------------------------------------------- marker sets ---

MK_SIZES = ((0, 0), (1, 1), (0, 63), (63, 0), (4, 6), (33, 2))          # ONE table: the LDS is sized by 63, the planes differ
MK_BGR = ((0, 0, 255), (0, 255, 255), (0, 255, 0), (255, 255, 0), (255, 0, 0), (255, 0, 255))     # hue 0, 30, 60, 90, 120, 150
MK_HUE = (0, 30, 60, 90, 120, 150)


def _markers():
    return [dict(h=(max(h - 5, 0), h + 6), s=(150, 256), v=(100, 256), erode=e, dilate=d, area=(0.0, DBL_MAX))
            for h, (e, d) in zip(MK_HUE, MK_SIZES)]


def _marker_frames(H, W, T, only=None, seed=0):
    """[t][s] BGR frames for 2 cameras: a grey background, and from t = 1 on every marker's own dense mask (another one
    per camera and frame) in the marker's colour; where masks overlap the later marker wins, so labels[t][s] says what each
    marker really shows.  only: paint that marker alone."""
    rng = np.random.default_rng(seed)
    base = rng.integers(90, 150, (2, H, W, 3)).astype(np.int16)
    frames, labels = [], []
    # the 33 x 33 and the 63 x 63 erosion need wide bars that nothing paints over: the first is painted last on even
    # frames, the second -- last -- on odd frames only (only: that marker on every frame)
    for t in range(T):
        f = np.clip(base + rng.integers(-5, 6, base.shape), 0, 255).astype(np.uint8)
        lab = np.full((2, H, W), -1, np.int8)
        for s in range(2):
            for m in (0, 1, 4, 2, 5, 3) if t else ():
                if (only is not None and m != only) or (only is None and m == 3 and t % 2 == 0):
                    continue
                e, d = MK_SIZES[m]
                mask = M.build(M.Case("marker", "word", H, W, e, d, "dense", 10 * t + m, False), s)
                lab[s][mask != 0] = m
            for m in range(6):
                f[s][lab[s] == m] = MK_BGR[m]
        frames.append([f[0], f[1]])
        labels.append(lab)
    return frames, labels


def _check_markers(A, hp, rig, got, fs, lab, tag, seen):
    want, planes = rig.check(got, fs, None, tag)
    for s in range(2):
        for m, (e, d) in enumerate(MK_SIZES):
            morph = _morph(np.where(lab[s] == m, 255, 0).astype(np.uint8), e, d)
            assert (planes[s][m] == morph).all(), (tag, s, m, "oracle")
            assert (hp.read_marker_mask(m, A.ffi.TAP_MORPH, s) == morph).all(), (tag, s, m, "morph")
            assert (hp.read_marker_mask(m, A.ffi.TAP_FINAL, s) == _final(morph)).all(), (tag, s, m, "final")
            seen[m] += int(morph.any() and not morph.all())


MK_TABLE_GEOM = (9, 129)
MK_FALLBACK_GEOM = (M.LDS_H, M.lds_edge_widths(63)[1])        # the table's LDS for a dilation of 63 is over the budget


@pytest.mark.parametrize("route,only", [(r, o) for r in ("sync", "table-1", "table-2", "fallback-2") for o in (None, 2, 5)
                                        if o is None or r != "fallback-2"],
                         ids=lambda v: {None: "all", 2: "only-dil-63", 5: "only-dil-2"}.get(v, v))
def test_marker_planes_each_with_its_own_sizes(A, route, only):
    """Six markers, two cameras: the synchronous step (marker by marker), the pipelined table route with one and two
    frames a launch, and a geometry whose table does not fit the row scan's LDS (marker by marker, first_stream = m * n).
    only-dil-63 / only-dil-2: the plane of the largest / the smallest dilation alone is painted -- a plane taking the
    launch's dilation instead of its own would grow the one or not grow the other."""
    from test_markers_gpu import _Rig, _hp
    H, W = MK_FALLBACK_GEOM if route.startswith("fallback") else MK_TABLE_GEOM
    assert (M.rowscan_lds_bytes(H, W, 63) > M.ROWSCAN_LDS_MAX) == route.startswith("fallback") and M.lds_able(H, W)
    T = 5
    frames, labels = _marker_frames(H, W, T, only, seed=3)
    markers = _markers()
    rig = _Rig(H, W, 2, markers)
    hp = _hp(H, W, 2, ring_depth=3)
    seen = [0] * 6
    try:
        hp.set_markers(markers, heading_anchor=None)
        if route == "sync":
            for t in range(T):
                _check_markers(A, hp, rig, hp.track_markers(frames[t]), frames[t], labels[t], (route, t), seen)
        else:
            hp.marker_pipeline(True)
            per = int(route[-1])
            hp.set_fusion(per)
            for t in range(0, T, per):
                chunk = list(range(t, min(t + per, T)))
                for k in chunk:
                    hp.enqueue(frames[k])
                for k in chunk:
                    _check_markers(A, hp, rig, hp.collect_markers(), frames[k], labels[k], (route, k), seen)
        live = [m for m in range(6) if only in (None, m)]
        assert all(seen[m] >= 2 for m in live), seen           # neither empty nor full: every painted plane showed something
    finally:
        hp.close()
