"""Shared, seeded cases of target crops (oatgpu_set_target_crops / oatgpu_target_crops / oatgpu_crop_windows_dev)
(TEST INFRASTRUCTURE, no GPU imports: tests/test_crops_cpu.py checks the cases on the model alone, tests/test_crops_gpu.py feeds the
same cases to the kernel).  The model is tests/crops_ref.py.

Explicit windows go through oatgpu_crop_windows_dev on pattern frames; frame sequences go through the motion and the subtraction
tracker.  A sequence here is made of shapes_cases' bar / staircase frames and targets_cases' block frames -- both draw on the same
background, imported and not edited -- so that ranks with and without a body axis, and a frame without any blob behind frames with
several, all occur behind a tracker's first two frames."""
import functools
import math

import numpy as np

import crops_ref as R
import oracle_lib as O
import shapes_cases as S
import shapes_ref as SR
import targets_cases as T

GEOMETRIES = ((48, 64), (37, 61))
CROP_SIZES = ((8, 8), (5, 4), (16, 12), (33, 64), (64, 128))      # (h, w): 33 x 64 is wider than 61, 64 x 128 larger than both frames
STREAMS = (1, 3, 66)
KS = (1, 4, 8)
PER_STREAM = 8


# ---------------------------------------------------------------------------------------------------------- pattern frames ----

@functools.lru_cache(maxsize=None)
def pattern(rows, cols, channels, variant=0):
    """A frame whose value depends on the position: no two pixels of a 3 x 3 neighbourhood are equal (|7 dx + 31 dy| < 256 and
    never 0 for |dx|, |dy| <= 2), the channels differ (by 85), and so do the cameras (by 53 a variant)."""
    y, x = np.mgrid[0:rows, 0:cols]
    base = 7 * x + 31 * y + 53 * variant
    f = (base % 256).astype(np.uint8) if channels == 1 else np.stack([(base + 85 * c) % 256 for c in range(3)], axis=2).astype(np.uint8)
    f.setflags(write=False)
    return f


# -------------------------------------------------------------------------------------------------------- explicit windows ----

@functools.lru_cache(maxsize=None)
def explicit_windows(rows, cols, h, w):
    """The windows of one (frame, crop size): upright ones first, then turned ones; invalid ones in between."""
    W = R.window
    rng = np.random.default_rng(9100 + 131 * rows + 17 * cols + 5 * h + w)
    xm, ym = cols // 2, rows // 2
    centres = [(10.5, 11.5), (11.5, 10.5), (10.49999, 12.50001), (20.50001, 7.49999),                 # x.5 on both parities
               (0.0, 0.0), (cols - 1.0, 0.0), (0.0, rows - 1.0), (cols - 1.0, rows - 1.0),            # corners
               (float(xm), 0.0), (float(xm), rows - 1.0), (0.0, float(ym)), (cols - 1.0, float(ym)),  # edges
               (-300.0, 10.0), (cols + 300.0, float(ym)), (float(xm), -300.0), (float(xm), rows + 300.0),
               (-(w // 2) - 3.0, float(ym)), (float(xm) + 0.25, float(ym) - 0.25)]
    out = [W(True, True, cx, cy) for cx, cy in centres]
    out.insert(3, R.INVALID)
    out.insert(7, W(True, True, math.nan, 5.0))
    out.insert(11, W(True, True, 5.0, 1e6 + 1.0))
    out.insert(12, W(True, True, 5.0, 5.0, math.inf, 0.0))                   # (an axis that is not finite, even where it is not used)
    r = math.sqrt(0.5)
    axes = [(1.0, 0.0), (0.0, 1.0), (r, r), (r, -r), (1.5, 0.25), (0.5, 0.0), (1e9, 0.0)]
    axes += [(math.cos(a), math.sin(a)) for a in rng.uniform(-math.pi / 2, math.pi / 2, 5)]
    turned = []
    for i, (cx, cy) in enumerate(centres):
        ax, ay = axes[i % len(axes)]
        turned.append(W(True, False, cx, cy, ax, ay))
    for ax, ay in axes:                                                       # every axis at a centre inside, with fractions
        turned.append(W(True, False, xm + float(rng.uniform(-3, 3)), ym + float(rng.uniform(-3, 3)), ax, ay))
    turned.append(W(True, False, cols - 1.0, float(ym), 1.0, 0.0))            # sx = W - 1 with fx = 0
    turned.insert(2, W(False, False, 10.0, 10.0, 1.0, 0.0))
    turned.insert(9, W(True, False, 10.0, math.inf, 1.0, 0.0))
    turned.insert(15, W(True, False, -1e6 - 1.0, 10.0, 0.0, 1.0))
    turned.insert(20, W(True, False, 10.0, 10.0, math.nan, 1.0))
    return tuple(out), tuple(turned)


def groups(windows):
    """a list of windows in groups of PER_STREAM, the last one padded with invalid windows"""
    ws = list(windows)
    ws += [R.INVALID] * (-len(ws) % PER_STREAM)
    return [ws[i:i + PER_STREAM] for i in range(0, len(ws), PER_STREAM)]


def coverage(win, rows, cols, h, w):
    """What the samples of a valid window touch: dict(inside, left, right, top, bottom, frac, last_col) -- a sample (corner) inside
    the frame, beyond each edge; an axis sample with fx != 0 != fy; one with sx == cols - 1"""
    c = dict(inside=False, left=False, right=False, top=False, bottom=False, frac=False, last_col=False)
    if not R.is_valid(win):
        return c
    _, upright, cx, cy, _, _ = win
    for i in range(h):
        for j in range(w):
            if upright:
                xs, ys = [int(round(cx)) - w // 2 + j], [int(round(cy)) - h // 2 + i]
            else:
                q = R.sample_position(win, h, w, i, j)
                if q is None:
                    c["left"] = c["right"] = c["top"] = c["bottom"] = True      # (somewhere far outside)
                    continue
                sx, sy = q[0] >> 5, q[1] >> 5
                xs, ys = [sx, sx + 1], [sy, sy + 1]
                c["frac"] |= (q[0] & 31) != 0 and (q[1] & 31) != 0
                c["last_col"] |= sx == cols - 1 and 0 <= sy < rows
            c["inside"] |= any(0 <= x < cols for x in xs) and any(0 <= y < rows for y in ys)
            c["left"] |= min(xs) < 0
            c["right"] |= max(xs) >= cols
            c["top"] |= min(ys) < 0
            c["bottom"] |= max(ys) >= rows
    return c


# ------------------------------------------------------------------------------------------------------ tracker sequences ----

N_FRAMES = 11
# frames 0 .. 9: a host step, a device step, sequence calls of 1, 2 and 5 frames; or one sequence call of all 11
PLAN = (("track", 1), ("track_dev", 1), ("seq", 1), ("seq", 2), ("seq", 5))
PLAN_LONG = (("seq", 11),)
SEQ_SLOTS = 4                                       # a tracker's slots: frame i of a sequence call sits in slot i % 4, a step in slot 0
# (source, frame of the source): bars and a staircase, then blocks (squares among them), then the bare background twice -- the second
# one is empty for the motion tracker too --, then bars again
MIX = (("shapes", 0), ("shapes", 1), ("shapes", 2), ("shapes", 3), ("targets", 4), ("targets", 5), ("targets", 6), ("targets", 7),
       ("bare", 0), ("bare", 0), ("shapes", 4))
FAMILIES = (("motion", 0.0), ("subtraction", 0.0), ("subtraction", 0.05))


def slots_of(plan):
    """[slot of frame t] under a plan"""
    out = []
    for how, count in plan:
        out += [i % SEQ_SLOTS if how == "seq" else 0 for i in range(count)]
    return out


def predecessor(plan, t):
    """the latest frame before t that sat in t's slot, or None"""
    slots = slots_of(plan)
    return next((u for u in range(t - 1, -1, -1) if slots[u] == slots[t]), None)


def paired_second(family, plan):
    """The frames that are the second of a paired front launch: the subtraction tracker pairs wherever a next frame exists in the
    call, the motion tracker wherever, besides, every stream has a last image (from its second frame on)."""
    out, t = set(), 0
    for how, count in plan:
        i = 0
        while i < count:
            if how == "seq" and i + 1 < count and (family == "subtraction" or t + i > 0):
                out.add(t + i + 1)
                i += 2
            else:
                i += 1
        t += count
    return out


@functools.lru_cache(maxsize=None)
def sequence(family, rows, cols, variant=0, channels=3):
    """frames[t] of one camera, (rows, cols, 3) -- or (rows, cols) GREY for the motion tracker with channels = 1"""
    fam = "subtraction" if family == "subtraction" else "motion"
    src = dict(shapes=S.sequence(fam, rows, cols, variant), targets=T.sequence(fam, rows, cols, variant))
    bare = T._background(rows, cols, variant)
    out = []
    for source, t in MIX:
        f = bare if source == "bare" else src[source][t]
        if channels == 1:
            f = O.bgr2grey(f)
        f = np.ascontiguousarray(f)
        f.setflags(write=False)
        out.append(f)
    return out


@functools.lru_cache(maxsize=None)
def sequence_masks(family, rows, cols, variant=0, alpha=0.0):
    """the oracle's mask after erode / dilate of every frame (the chains of targets_cases.sequence_masks)"""
    frames = sequence(family, rows, cols, variant)
    if family == "motion":
        d = O.Diff(rows, cols, T.DIFF["diff_threshold"], T.DIFF["blur"], *T.AREA)
        out = [d.detect(O.bgr2grey(f))[1] for f in frames]
    else:
        b, p = O.Bsub(rows, cols, 3, alpha), T.sub_params()
        out = [O.detect_hsv(O.bgr2hsv(b.filter(f)), p)[1] for f in frames]
    for m in out:
        m.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def sequence_targets(family, rows, cols, variant, alpha, k):
    """[(ranks, n_found)] for every frame: the oracle chain's own targets"""
    return [T.reference(m, T.AREA, k) for m in sequence_masks(family, rows, cols, variant, alpha)]


@functools.lru_cache(maxsize=None)
def sequence_shapes(family, rows, cols, variant, alpha, k):
    """[the k ranks' shapes] for every frame: the oracle chain's own shapes"""
    return [SR.reference(m, T.AREA, k) for m in sequence_masks(family, rows, cols, variant, alpha)]


@functools.lru_cache(maxsize=None)
def sequence_windows(family, rows, cols, variant, alpha, k, axis):
    """[the k windows] for every frame"""
    tg = sequence_targets(family, rows, cols, variant, alpha, k)
    sh = sequence_shapes(family, rows, cols, variant, alpha, k) if axis else [None] * len(tg)
    return [R.windows_of(ranks, shp, axis) for (ranks, _), shp in zip(tg, sh)]


@functools.lru_cache(maxsize=None)
def sequence_crops(family, rows, cols, variant, alpha, k, axis, h, w, channels=3):
    """[uint8 [k, h, w(, 3)]] for every frame of one camera: the model's crops; computed once, never written to"""
    frames = sequence(family, rows, cols, variant, channels)
    out = []
    for f, wins in zip(frames, sequence_windows(family, rows, cols, variant, alpha, k, axis)):
        c = np.stack([R.crop(f, win, h, w) for win in wins])
        c.setflags(write=False)
        out.append(c)
    return out


variant_of = T.variant_of

# (family, alpha, rows, cols, n_streams, k, h, w): every K and every stream count, both geometries, windows smaller than, wider
# than and larger than the frame
TRACKER_RUNS = (
    ("motion", 0.0, 37, 61, 1, 1, 16, 12),
    ("motion", 0.0, 37, 61, 3, 8, 8, 8),
    ("motion", 0.0, 48, 64, 66, 4, 5, 4),
    ("subtraction", 0.0, 48, 64, 1, 4, 16, 12),
    ("subtraction", 0.05, 48, 64, 3, 4, 33, 64),
    ("subtraction", 0.0, 37, 61, 3, 8, 64, 128),
    ("subtraction", 0.05, 37, 61, 66, 4, 8, 8),
)
