"""Shared, seeded cases of target masks (oatgpu_set_target_mask_tensor) (TEST INFRASTRUCTURE, no GPU imports:
tests/test_target_masks_cpu.py checks the cases on the model alone, tests/test_target_masks_gpu.py feeds the same cases to the kernel).
The model is tests/target_masks_ref.py.

Two kinds of frame sequences go through the motion and the subtraction tracker:
  "mix"       crops_cases' sequences with its tracker parameters, runs and plans, imported and not edited -- at most 64 pixels wide, so
              every mask row is one word;
  "designed"  frames painted so that the final mask holds what membership can get wrong (DESIGNS below), in crops_cases' two
              geometries and in a third, 21 x 150: three mask words a row, the last partial.  Their trackers run without morphology
              (motion: blur 0; subtraction: no erode, no dilate, alpha 0), so that the final mask IS the painted design -- a
              corner contact would not survive a dilation."""
import functools

import numpy as np

import crop_tensor_cases as TC
import crop_tensor_ref as TR
import crops_cases as CC
import oracle_lib as O
import shapes_ref as SR
import target_masks_ref as MR
import targets_cases as T

GEOMETRIES = CC.GEOMETRIES + ((21, 150),)
WIDE = (21, 150)
ZOOMS = TC.ZOOMS
PLAN, PLAN_LONG, RUN_CALLS, RESET_BEFORE, CAPACITY = TC.PLAN, TC.PLAN_LONG, TC.RUN_CALLS, TC.RESET_BEFORE, TC.CAPACITY
N_FRAMES = CC.N_FRAMES
MASK_SIZES = ((5, 4), (16, 12), (64, 128))
FAMILIES = ("motion", "subtraction")
AREA = T.AREA
variant_of = CC.variant_of

# crops_cases.TRACKER_RUNS with the window sizes of masks: (kind, family, alpha, rows, cols, n_streams, k, h, w)
_MIX_SIZES = ((16, 12), (5, 4), (5, 4), (64, 128), (16, 12), (64, 128), (16, 12))
MIX_RUNS = tuple(("mix",) + run[:6] + hw for run, hw in zip(CC.TRACKER_RUNS, _MIX_SIZES))
DESIGNED_RUNS = (
    ("designed", "motion", 0.0, 48, 64, 3, 4, 16, 12),
    ("designed", "motion", 0.0, 37, 61, 1, 8, 64, 128),
    ("designed", "motion", 0.0, 21, 150, 3, 4, 16, 12),
    ("designed", "subtraction", 0.0, 48, 64, 1, 1, 16, 12),
    ("designed", "subtraction", 0.0, 37, 61, 3, 4, 5, 4),
    ("designed", "subtraction", 0.0, 21, 150, 3, 8, 16, 12),
)
RUNS = MIX_RUNS + DESIGNED_RUNS
COMBOS = tuple((z, d) for z in ZOOMS for d in MR.DTYPES)          # every zoom with every dtype


def settings_of(case, axis):
    """the three (zoom, dtype) a run goes through in one mode: consecutive triples of COMBOS, every triple in both modes over the runs"""
    start = (3 * case + 3 * int(axis)) % len(COMBOS)
    return [COMBOS[(start + i) % len(COMBOS)] for i in range(3)]


# ---------------------------------------------------------------------------------------------------------- the designs ----

DESIGNS = ("full", "few")
MOTION_BGR = (255, 255, 255)                 # far from the background's grey for every pixel (diff_threshold 12)
DESIGNED_DIFF = dict(diff_threshold=12, blur=0)
DESIGNED_MORPH = (0, 0)


def _rect(img, y0, y1, x0, x1):
    img[y0:y1 + 1, x0:x1 + 1] = True


@functools.lru_cache(maxsize=None)
def design(rows, cols, which, variant=0):
    """bool [rows, cols]: what is painted.  Everything but the blob on the frame's edge moves right with the camera's variant.
    "full": E  a blob on the frame's top-left edge (its row 0 and column 0 are lost to the frame zeroing);
            R  a 9 x 9 ring with a 3 x 3 blob in its hole;
            A, B  two 4 x 4 squares that touch only at a corner: one component;
            C, D  a 5 x 5 and a 4 x 3 blob one column apart (two ranked blobs inside one window), and a 2 x 2 blob below the area
                  window next to them;
            a comb (five teeth joined by a bar at the bottom) and a staircase running down to the left: their run heads merge late
            and in a row, so the union-find chain from a late head to the root is longer than one step;
            at 150 columns: two blobs joined only by a one-pixel run across columns 63 / 64 and 127 / 128.
    "few":  E and R alone: two candidates, so that ranks from 2 on are invalid."""
    assert rows >= 21 and cols >= 61
    img = np.zeros((rows, cols), bool)
    d = variant
    _rect(img, 0, 5, 0, 9)                                        # E
    _rect(img, 8, 16, 1 + d, 9 + d)                               # R ...
    img[10:15, 3 + d:8 + d] = False                               # ... its hole ...
    _rect(img, 11, 13, 4 + d, 6 + d)                              # ... and the blob in it
    if which == "full":
        _rect(img, 1, 4, 13 + d, 16 + d)                          # A
        _rect(img, 5, 8, 17 + d, 20 + d)                          # B: corner to corner with A
        _rect(img, 11, 15, 12 + d, 16 + d)                        # C
        _rect(img, 11, 14, 18 + d, 20 + d)                        # D
        _rect(img, 18, 19, 14 + d, 15 + d)                        # contour area 1: below the area window
        for x in range(24, 33, 2):                                # the comb's teeth ...
            _rect(img, 1, 7, x + d, x + d)
        _rect(img, 8, 8, 24 + d, 32 + d)                          # ... and its bar
        for i in range(8):                                        # the staircase
            _rect(img, 10 + i, 10 + i, 44 - 2 * i + d, 46 - 2 * i + d)
        if cols >= 140:
            _rect(img, 2, 6, 58 + d, 61 + d)
            _rect(img, 2, 6, 130 + d, 133 + d)
            _rect(img, 4, 4, 62 + d, 129 + d)                     # the only connection: a run through two word boundaries
    img.setflags(write=False)
    return img


def design_at(t):
    """the design frame t shows: "full" and "few" in turn, two frames each (a motion tracker sees a design appear, then vanish)"""
    return DESIGNS[((t - 1) // 2) % 2] if t > 0 else None


@functools.lru_cache(maxsize=None)
def designed_sequence(family, rows, cols, variant=0, channels=3):
    """frames[t] of one camera.  subtraction: the bare background, then a design a frame; motion: designs and the bare background in
    turn, so that every difference image from frame 1 on is a design."""
    bare = T._background(rows, cols, variant)
    from bsub_cases import RECT_BGR
    out = []
    for t in range(N_FRAMES):
        f = bare.copy()
        shown = t > 0 if family == "subtraction" else t % 2 == 1
        if shown:
            which = design_at(t)
            f[design(rows, cols, which, variant)] = RECT_BGR if family == "subtraction" else MOTION_BGR
        if channels == 1:
            f = O.bgr2grey(f)
        f = np.ascontiguousarray(f)
        f.setflags(write=False)
        out.append(f)
    return out


def sequence(kind, family, rows, cols, variant=0, channels=3):
    return CC.sequence(family, rows, cols, variant, channels) if kind == "mix" else designed_sequence(family, rows, cols, variant, channels)


def designed_sub_params():
    w = T.sub_window()
    return O.hsv_params(h_lo=w["h"][0], h_hi=w["h"][1], s_lo=w["s"][0], s_hi=w["s"][1], v_lo=w["v"][0], v_hi=w["v"][1],
                        erode=DESIGNED_MORPH[0], dilate=DESIGNED_MORPH[1], min_area=AREA[0], max_area=AREA[1])


@functools.lru_cache(maxsize=None)
def sequence_masks(kind, family, rows, cols, variant=0, alpha=0.0):
    """the oracle chain's mask after erode / dilate of every frame"""
    if kind == "mix":
        return CC.sequence_masks(family, rows, cols, variant, alpha)
    frames = designed_sequence(family, rows, cols, variant)
    if family == "motion":
        d = O.Diff(rows, cols, DESIGNED_DIFF["diff_threshold"], DESIGNED_DIFF["blur"], *AREA)
        out = [d.detect(O.bgr2grey(f))[1] for f in frames]
    else:
        b, p = O.Bsub(rows, cols, 3, alpha), designed_sub_params()
        out = [O.detect_hsv(O.bgr2hsv(b.filter(f)), p)[1] for f in frames]
    for m in out:
        m.setflags(write=False)
    return tuple(out)


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def sequence_labels(kind, family, rows, cols, variant, alpha, wrong=None):
    """[target_masks_ref.labels_for(mask)] for every frame: computed once, shared, never written to"""
    return [_frozen(MR.labels_for(m, wrong)) for m in sequence_masks(kind, family, rows, cols, variant, alpha)]


@functools.lru_cache(maxsize=None)
def sequence_targets(kind, family, rows, cols, variant, alpha, k):
    return [T.reference(m, AREA, k) for m in sequence_masks(kind, family, rows, cols, variant, alpha)]


@functools.lru_cache(maxsize=None)
def sequence_shapes(kind, family, rows, cols, variant, alpha, k):
    return [SR.reference(m, AREA, k) for m in sequence_masks(kind, family, rows, cols, variant, alpha)]


@functools.lru_cache(maxsize=None)
def sequence_windows(kind, family, rows, cols, variant, alpha, k, axis, zoom):
    """[the k windows] for every frame: the oracle chain's targets and shapes through crop_tensor_ref's direction rule"""
    tg = sequence_targets(kind, family, rows, cols, variant, alpha, k)
    sh = sequence_shapes(kind, family, rows, cols, variant, alpha, k) if axis else [None] * len(tg)
    return [TR.zoomed_windows(ranks, shp, axis, zoom) for (ranks, _), shp in zip(tg, sh)]


@functools.lru_cache(maxsize=None)
def sequence_on(kind, family, rows, cols, variant, alpha, k, axis, zoom, h, w, wrong=None, pairs=()):
    """[bool [k, h, w]] for every frame of one camera: the ON elements; computed once, never written to.  wrong: one of
    target_masks_ref.WRONG_LABEL / WRONG_PIXEL, or "first_of_pair" with pairs = the frames that were the second of a paired launch
    (their windows are labelled from the frame before)."""
    label_rule = wrong if wrong in MR.WRONG_LABEL and wrong != "rank0_root" else None
    labels = sequence_labels(kind, family, rows, cols, variant, alpha, label_rule)
    tg = sequence_targets(kind, family, rows, cols, variant, alpha, k)
    out = []
    for t, wins in enumerate(sequence_windows(kind, family, rows, cols, variant, alpha, k, axis, zoom)):
        first = labels[t - 1] if wrong == "first_of_pair" and t in pairs else labels[t]
        ranks = tg[t][0]
        on = []
        for rank, win in zip(ranks, wins):
            r = ranks[0] if wrong == "rank0_root" and rank["valid"] else rank
            on.append(MR.window_on(first, r, win, h, w, wrong if wrong in MR.WRONG_PIXEL else None))
        out.append(_frozen(np.stack(on)))
    return out


def sequence_valid(kind, family, rows, cols, variant, alpha, k):
    """[bool [k]] for every frame: the ranks' validity"""
    return [np.array([r["valid"] for r in ranks], bool) for ranks, _ in sequence_targets(kind, family, rows, cols, variant, alpha, k)]


def entry(run, t, axis, zoom, dtype, wrong=None, pairs=()):
    """frame t's entry of a run, [n, k, h, w] of the dtype"""
    kind, family, alpha, rows, cols, n, k, h, w = run
    seq_wrong = wrong if wrong not in MR.WRONG_VALUE + ("entry_is_slot", "stale_entry") else None
    per = {v: sequence_on(kind, family, rows, cols, v, alpha, k, axis, zoom, h, w, seq_wrong, pairs)[t] for v in {variant_of(s) for s in range(n)}}
    return MR.to_dtype(np.stack([per[variant_of(s)] for s in range(n)]), dtype, wrong)


def entry_valid(run, t):
    kind, family, alpha, rows, cols, n, k, h, w = run
    return np.stack([sequence_valid(kind, family, rows, cols, variant_of(s), alpha, k)[t] for s in range(n)])
