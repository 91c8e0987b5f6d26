"""Shared, seeded cases of the motion and the subtraction tracker with lens undistortion inside the front kernel
(oatgpu_set_tracker_undistort) and numpy front ends for them, right and wrong (TEST INFRASTRUCTURE:
tests/test_tracker_undistort_cpu.py checks the case list without a GPU, tests/test_diff_undistort_gpu.py and
tests/test_bsub_undistort_gpu.py feed the same cases to the kernels).

A case wraps a BGR or GREY case of tests/diff_cases.py or tests/bsub_cases.py: given[t][s] is the scene frame, what the camera
delivers; und[t][s] = undistort_ref.remap(given[t][s], map of stream s) is what the chain behind `framefilt undistort` sees.  The
reference for a run with the switch on is the packed tracker fed und[t][s]; beside it run diff_cases.Model + the oracle's `posidet
diff`, or bsub_cases.Ref, on the same frames."""
import functools
from dataclasses import dataclass

import numpy as np

import bsub_cases as B
import diff_cases as D
import undistort_ref as R
from tracker_bayer_cases import DiffRef  # noqa: F401  (one stream of the motion chain's reference: oracle + numpy front end)

# diff_cases' five (narrow with Wp > W; wide with whole lanes beyond W; wide with a tail wave; one word a row; one lane a row)
# plus: the smallest frames, 4 x 8, and the shape that crosses wave and workgroup boundaries of the wide mapping
GEOMETRIES = list(D.GEOMETRIES) + [(3, 3), (3, 4), (4, 8), (12, 1040)]
BIG = [g for g in GEOMETRIES if g[0] >= 33]                 # the geometries whose references must detect (non-vacuity)
CALS = ("mild5", "pincushion", "skew")                      # of undistort_ref.cases(rows, cols)
# (geometry, calibration) whose references must detect: every calibration on BIG; (12, 1040) with pincushion only (skew leaves
# the subtraction chain nothing valid there: taps are compared instead)
DETECTING = [(r, c, k) for r, c in BIG for k in CALS] + [(12, 1040, "pincushion")]
THREE = ("mild5", "pincushion", "skew")                     # three streams, three calibrations
THREE_SWAPPED = ("pincushion", "mild5", "skew")


@functools.lru_cache(maxsize=None)
def calibration(rows, cols, name):
    """-> (K, D) of undistort_ref.cases"""
    return R.cases(rows, cols)[name]


@functools.lru_cache(maxsize=None)
def maps(rows, cols, name):
    return R.undistort_map(rows, cols, *calibration(rows, cols, name))


@dataclass
class UndCase:
    c: object               # the packed case: parameters, ROI, background from a file, the scene frames
    cals: tuple             # [s] calibration name of every stream
    maps: list              # [s] (map1, map2)
    given: list             # [t][s] the scene frames (c.frames)
    und: list               # [t][s] the undistorted frames

    def calibration(self, s):
        return calibration(self.c.rows, self.c.cols, self.cals[s])


def _wrap(c, cals):
    assert len(cals) == c.n_streams
    ms = [maps(c.rows, c.cols, k) for k in cals]
    und = [[R.remap(f, *ms[s]) for s, f in enumerate(fs)] for fs in c.frames]
    return UndCase(c, tuple(cals), ms, c.frames, und)


@functools.lru_cache(maxsize=None)
def diff_case(rows, cols, channels, cals, roi=False, n_frames=12, thr=12, blur=2):
    c = D.make_case(f"und-{rows}x{cols}-ch{channels}-{cals}", rows, cols, channels, len(cals), diff_threshold=thr, blur=blur, roi=roi,
                    n_frames=n_frames, seed=rows + len(cals))
    return _wrap(c, cals)


@functools.lru_cache(maxsize=None)
def bsub_case(rows, cols, channels, cals, alpha=0.05, roi=False, background=False, n_frames=B.N_FRAMES):
    c = B.make_case(f"und-{rows}x{cols}-ch{channels}-{cals}-a{alpha}", rows, cols, channels, len(cals), alpha=alpha, roi=roi,
                    background=background, n_frames=n_frames, seed=rows + len(cals))
    return _wrap(c, cals)


def plain_case(uc):
    """The same chain without undistortion: every map the identity (und = given)"""
    return UndCase(uc.c, uc.cals, uc.maps, uc.given, uc.given)


# --------------------------------------------------------------------------------------- front ends, right and wrong ----

def remap_variant(src, map1, map2, replicate=False, bias=16384, swap_f=False):
    """undistort_ref.remap with its border rule, its rounding bias and its fraction fields open to a planted mistake (the
    defaults are undistort_ref.remap: the CPU file asserts so)."""
    H, W = src.shape[:2]
    s = src.reshape(H, W, -1).astype(np.int64)
    sx, sy = map1[..., 0].astype(np.int64), map1[..., 1].astype(np.int64)
    m2 = map2.astype(np.int64)
    if swap_f:
        m2 = (m2 & 31) * 32 + (m2 >> 5)
    wt = R.bilinear_tab()[m2]
    acc = np.zeros(map2.shape + (s.shape[2],), np.int64)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        xx, yy = sx + dx, sy + dy
        inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        val = s[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]
        if not replicate:
            val = val * inside[..., None]
        acc += val * wt[..., k][..., None]
    return ((acc + bias) >> 15).astype(np.uint8).reshape(map2.shape + src.shape[2:])


# grey / subtraction taken before the remap; the ROI applied to the distorted frame; stream 0's map for every stream; the second
# frame of every pair (every odd frame) left as given; BORDER_REPLICATE; the + 512 (of 1024) dropped; fx and fy swapped
WRONG = ["before_remap", "roi_on_distorted", "map0", "pair_unremapped", "border_replicate", "no_round", "swap_fxfy"]


def handed(uc, t, s, wrong=None):
    """-> (frame, ROI or None) as a front end hands frame t of stream s to the chain behind the remap ("before_remap" is the
    chains' own business: diff_bits, bsub_bits)"""
    f, roi, (m1, m2) = uc.given[t][s], uc.c.roi_at(t, s), uc.maps[s]
    if wrong is None:
        return uc.und[t][s], roi
    if wrong == "roi_on_distorted":
        if roi is None:
            return uc.und[t][s], None
        g = f.copy()
        g[roi == 0] = 0
        return R.remap(g, m1, m2), None
    if wrong == "map0":
        return R.remap(f, *uc.maps[0]), roi
    if wrong == "pair_unremapped":
        return (f if t % 2 == 1 else uc.und[t][s]), roi
    if wrong == "border_replicate":
        return remap_variant(f, m1, m2, replicate=True), roi
    if wrong == "no_round":
        return remap_variant(f, m1, m2, bias=0), roi
    if wrong == "swap_fxfy":
        return remap_variant(f, m1, m2, swap_f=True), roi
    raise ValueError(wrong)


def diff_bits(uc, wrong=None):
    """[t][s] threshold bits of the motion chain behind front end `wrong`"""
    ms = [D.Model(uc.c.diff_threshold, uc.c.blur) for _ in uc.cals]
    out = []
    for t in range(len(uc.given)):
        row = []
        for s in range(len(ms)):
            if wrong == "before_remap":                     # the grey image is remapped: another rounding
                fr, roi = R.remap(D.grey_of(uc.given[t][s]), *uc.maps[s]), uc.c.roi_at(t, s)
            else:
                fr, roi = handed(uc, t, s, wrong)
            row.append(ms[s].front(fr, roi)[0])
        out.append(row)
    return out


def _bsub_models(uc):
    ms = [B.Model(uc.c.alpha) for _ in uc.cals]
    for s, img in uc.c.background.items():
        ms[s].set_background(img)
    return ms


def bsub_bits(uc, wrong=None):
    """[t][s] (window bits, background) of the subtraction chain behind front end `wrong`"""
    ms = _bsub_models(uc)
    out = []
    for t in range(len(uc.given)):
        row = []
        for s in range(len(ms)):
            if wrong == "before_remap":                     # bsub on the distorted frame, its difference image remapped
                roi = uc.c.roi_at(t, s)
                _, bg, _, d = ms[s].front(uc.given[t][s], None)
                d = R.remap(d, *uc.maps[s])
                if roi is not None:
                    d[roi == 0] = 0
                row.append((B.window_bits(d), R.remap(bg, *uc.maps[s])))
            else:
                row.append(ms[s].front(*handed(uc, t, s, wrong))[:2])
        out.append(row)
    return out


def tells_apart(uc, chain, wrong):
    right, bad = chain(uc), chain(uc, wrong)
    flat = lambda x: [np.asarray(a) for fs in x for e in fs for a in (e if isinstance(e, tuple) else (e,))]  # noqa: E731
    return any((a != b).any() for a, b in zip(flat(right), flat(bad)))


def branch_counts(rows, cols, name):
    """-> (inside, partly inside, fully outside) pixel counts of remap_px's three branches under the calibration's map"""
    m1, _ = maps(rows, cols, name)
    sx, sy = m1[..., 0].astype(int), m1[..., 1].astype(int)
    inside = (sx >= 0) & (sx < cols - 1) & (sy >= 0) & (sy < rows - 1)
    outside = (sx >= cols) | (sx + 1 < 0) | (sy >= rows) | (sy + 1 < 0)
    return int(inside.sum()), int((~inside & ~outside).sum()), int(outside.sum())


# ------------------------------------------------------------------------------------------------ the references ----

@functools.lru_cache(maxsize=None)
def _diff_want(rows, cols, channels, cals, roi, n_frames, thr, blur, plain):
    uc = diff_case(rows, cols, channels, cals, roi, n_frames, thr, blur)
    refs = [DiffRef(uc.c) for _ in cals]
    frames = uc.given if plain else uc.und
    return [[refs[s].step(f, uc.c.roi_at(t, s)) for s, f in enumerate(fs)] for t, fs in enumerate(frames)]


def diff_want(rows, cols, channels, cals, roi=False, n_frames=12, thr=12, blur=2, plain=False):
    """-> (case, want[t][s] = DiffRef.step of the undistorted frames (plain: of the given frames)), computed once and shared"""
    return (diff_case(rows, cols, channels, cals, roi, n_frames, thr, blur),
            _diff_want(rows, cols, channels, cals, roi, n_frames, thr, blur, plain))


@functools.lru_cache(maxsize=None)
def _bsub_want(rows, cols, channels, cals, alpha, roi, background, n_frames, plain):
    uc = bsub_case(rows, cols, channels, cals, alpha, roi, background, n_frames)
    refs = [B.Ref(uc.c, s) for s in range(len(cals))]
    frames = uc.given if plain else uc.und
    return [[refs[s].step(f, uc.c.roi_at(t, s)) for s, f in enumerate(fs)] for t, fs in enumerate(frames)]


def bsub_want(rows, cols, channels, cals, alpha=0.05, roi=False, background=False, n_frames=B.N_FRAMES, plain=False):
    """-> (case, want[t][s] = bsub_cases.Ref.step of the undistorted frames: (detection, bits, morph > 0, bg, acc))"""
    return (bsub_case(rows, cols, channels, cals, alpha, roi, background, n_frames),
            _bsub_want(rows, cols, channels, cals, alpha, roi, background, n_frames, plain))
