"""Shared cases of target tracks (oatgpu_set_tracks / oatgpu_tracks / oatgpu_tracks_update) (TEST INFRASTRUCTURE, no
GPU imports: tests/test_tracks_cpu.py checks the cases on the model alone, tests/test_tracks_gpu.py and
tests/test_tracks_host_gpu.py feed the same cases to the kernels and the binaries).  The model is tests/tracks_ref.py.

Two kinds of cases:
  fed     detection lists given as exact doubles (FED; through oatgpu_tracks_update), 12 - 16 frames, K = 1, 3, 8: ranks that swap
          while the slots persist, a miss shorter and one longer than the timeout, a birth into the first free slot, K + 1
          objects, a detection just inside and one just outside the gate, gate = inf and gate = 0, a track that dies on the frame a
          detection arrives, an exact cost tie.  Stream s sees the same scene shifted by an exact binary offset.
  image   frame sequences for the motion and the subtraction tracker: three blocks of equal area in three column bands move up
          and down at different speeds (their ranks cross: equal areas rank by the later first pixel), one vanishes for 2 frames,
          one for 5.  The detections are targets_cases.reference on the oracle's own mask, never a device tap."""
import functools
import math

import numpy as np

import bsub_cases as BC
import diff_cases as DC
import oracle_lib as O
import posfilt_cases as P
import targets_cases as T
import tracks_ref as TR

KALMAN = dict(dt=0.5, timeout=2.0, sigma_accel=2.0, sigma_noise=1.0)      # the track runs out on its 4th frame without a measurement
THRESHOLD = 4
NONE = (False, 0.0, 0.0)


# ----------------------------------------------------------------------------------------------------------- fed cases ----

class Fed:
    def __init__(self, name, k, gate, scene, homography=None, regions=None):
        self.name, self.k, self.gate, self.scene, self.homography, self.regions = name, k, gate, scene, homography, regions

    def __repr__(self):
        return self.name

    def frames(self, stream=0):
        """[t] -> k triples (valid, x, y): the valid ones first, as ranks are; stream s is shifted by (s % 5 / 4, s % 3 / 2)"""
        ox, oy = (stream % 5) * 0.25, (stream % 3) * 0.5
        out = []
        for dets in self.scene:
            row = [(True, float(x) + ox, float(y) + oy) for x, y in dets]
            assert len(row) <= self.k
            out.append(row + [NONE] * (self.k - len(row)))
        return out

    def config(self):
        return dict(kalman=KALMAN, gate=self.gate, homography=self.homography, regions=self.regions)

    def want(self, stream=0, wrong=None):
        return TR.run(self.frames(stream), self.k, wrong=wrong, **self.config())


def _swap():
    scene = []
    for t in range(14):
        a, b = (10 + 3 * t, 10 + t), (60 - 3 * t, 40 - 0.5 * t)
        row = [a, b] if t % 2 == 0 else [b, a]
        if t >= 5:                                   # a third object, born into the first free slot; it moves through the ranks
            row.insert(0 if t % 3 == 0 else 2, (30 + 0.5 * t, 55))
        scene.append(row)
    return scene


def _miss():
    """A misses frames 4 - 5 and resumes; B misses from frame 3 on and runs out on frame 6 -- the frame D arrives on, beyond the
    gate of everything: no slot is free until frame 7.  C stands still in slot 2."""
    scene = []
    for t in range(14):
        row = []
        if t not in (4, 5):
            row.append((10 + 2 * t, 10))
        if t < 3:
            row.append((50, 50 + t))
        row.append((90, 10))
        if t >= 6:
            row.append((90, 90 + 0.5 * (t - 6)))
        scene.append(row[:3])
    return scene


def _one():
    pts = {0: (10, 10), 1: (12, 10), 2: (14, 10), 6: (50, 50), 7: (51, 50), 8: (52, 50), 9: (53, 50), 10: (54, 50), 11: (55, 50),
           13: (57, 50)}
    return [[pts[t]] if t in pts else [] for t in range(14)]


def _gate(gate):
    """Frames 0 - 5: A and B move; frame 6: A's detection sits gate - 0.01 from where slot 0 expects it (assigned), B's gate + 0.01
    from where slot 1 expects it (a birth into slot 2; slot 1 coasts).  From frame 7 a fourth object E finds every slot live and
    is dropped until slot 1 has run out."""
    head = [[(20 + 2 * t, 20), (60, 60 + 2 * t)] for t in range(6)]
    cam = TR.Camera(3, KALMAN, gate)
    for row in Fed("gate-head", 3, gate, head).frames():
        cam.step(row)
    (ax, ay), (bx, by) = cam.predicted(0), cam.predicted(1)
    a6, b6 = (ax + gate - 0.01, ay), (bx + gate + 0.01, by)
    scene = head + [[a6, b6]]
    for t in range(7, 14):
        scene.append([(a6[0] + 2 * (t - 6), a6[1]), (b6[0], b6[1] + 2 * (t - 6)), (5, 90)])
    return scene


def _gate0():
    return [[(20, 20), (40 + 3 * t, 40)] for t in range(12)]


def _tie():
    """Two tracks born at (10, 20) and (30, 20); one detection at (20, 20) on the next frame: both costs are exactly 100."""
    return [[(10, 20), (30, 20)], [(20, 20)]] + [[(20 + t, 20)] for t in range(1, 11)]


def _many():
    scene = []
    for t in range(16):
        objs = []
        for q in range(8):
            if (t + q) % 7 == 5 or (q == 3 and 4 <= t <= 9):
                continue
            objs.append((q, (15 + 25 * (q % 4) + (q % 3 - 1) * t, 15 + 30 * (q // 4) + ((q + 1) % 3 - 1) * t)))
        r = t % max(len(objs), 1)
        scene.append([p for _, p in objs[r:] + objs[:r]])
    return scene


def _regions_for(case):
    """two regions in WORLD units aimed at where the model's positions go under the case's homography"""
    out, _ = TR.run(case.frames(), case.k, kalman=KALMAN, gate=case.gate, homography=case.homography)
    xs = sorted(r["x"] for rs in out for r in rs if r["position_valid"])
    ys = sorted(r["y"] for rs in out for r in rs if r["position_valid"])
    x0, x1, xm = math.floor(xs[0]) - 1, math.ceil(xs[-1]) + 1, round(xs[len(xs) // 2])
    y0, y1 = math.floor(ys[0]) - 1, math.ceil(ys[-1]) + 1
    return [("low", [(x0, y0), (xm, y0), (xm, y1), (x0, y1)]), ("wide", [(x0, y0), (x1, y0), (x1, y1), (x0, y1 - 1)])]


@functools.lru_cache(maxsize=None)
def fed_cases():
    out = [Fed("swap-k3-inf", 3, math.inf, _swap()), Fed("miss-k3", 3, 20.0, _miss()), Fed("one-k1", 1, 5.0, _one()),
           Fed("gate-k3", 3, 10.0, _gate(10.0)), Fed("gate0-k3", 3, 0.0, _gate0()), Fed("tie-k3-inf", 3, math.inf, _tie()),
           Fed("many-k8", 8, 12.0, _many())]
    chain = Fed("chain-k3", 3, 20.0, _miss(), homography=P.HOMOGRAPHIES["affine"])
    chain.regions = _regions_for(chain)
    return tuple(out + [chain])


def fed(name):
    return next(c for c in fed_cases() if c.name == name)


# --------------------------------------------------------------------------------------------------------- image cases ----

GEOMETRIES = ((48, 64, 3), (37, 61, 1))            # rows, cols, channels
MANY = (24, 32, 1)                                 # 66 streams
IMG_T = 21
RESET_AT = 10                                      # the GPU tests reset the detector (not the tracks) in front of this frame
IMG_K = 3
IMG_KALMAN = dict(dt=0.03125, timeout=0.125, sigma_accel=300.0, sigma_noise=0.5)     # runs out on the 4th frame without a measurement
IMG_GATE = 10.0
DIFF = dict(diff_threshold=12, blur=2)
SUB_MORPH = (0, 3)
FAMILIES = (("motion", 0.0), ("subtraction", 0.0), ("subtraction", 0.05))
GONE = {1: (5, 6), 2: (8, 9, 10, 11, 12)}           # block -> the frames it is not in the scene: 2 frames, 5 frames
SPEED = (1, 2, 3)
PHASE = (0, 5, 9)


def _tri(v, span):
    """a triangle wave 0 .. span .. 0"""
    v %= 2 * span
    return v if v <= span else 2 * span - v


def _block(rows, cols):
    return max(3, rows // 8), max(3, cols // 12)


@functools.lru_cache(maxsize=None)
def sequence(family, rows, cols, channels, variant=0):
    """frames[t] of one camera; variant: which of three different cameras a stream shows.  Frame 0 is the bare background."""
    rng = np.random.default_rng(5200 + 7 * rows + cols + channels + variant)
    shape = (rows, cols, 3) if channels == 3 else (rows, cols)
    bg = rng.integers(40, 91, shape).astype(np.uint8)
    if channels == 3:
        bg[..., 0] = rng.integers(40, 51, (rows, cols))
    if family == "subtraction":
        colour = BC.RECT_BGR if channels == 3 else BC.RECT_GREY
    else:
        colour = (90, 250, 130) if channels == 3 else 220
    h, w = _block(rows, cols)
    band, span = cols // 3, rows - h - 5
    frames = []
    for t in range(IMG_T):
        f = bg.copy()
        for b in range(3):
            if t == 0 or t in GONE.get(b, ()):
                continue
            x = b * band + 2 + _tri(t + variant, max(1, band - w - 3))
            y = 2 + _tri(SPEED[b] * t + PHASE[(b + variant) % 3], span)
            f[y:y + h, x:x + w] = colour
        f.setflags(write=False)
        frames.append(f)
    return frames


def sub_case(rows, cols, channels, n, alpha):
    return BC.Case(f"tracks-{rows}x{cols}", rows, cols, channels, n, float(alpha), SUB_MORPH[0], SUB_MORPH[1])


@functools.lru_cache(maxsize=None)
def image_targets(family, rows, cols, channels, variant=0, alpha=0.0, k=IMG_K, resets=()):
    """[(ranks, n_found)] of every frame: targets_cases.reference on the oracle's mask after erode / dilate.  resets: the frames
    in front of which the detector starts over (oatgpu_diff_reset / oatgpu_bsub_reset)"""
    frames = sequence(family, rows, cols, channels, variant)
    masks = []
    if family == "motion":
        for t, f in enumerate(frames):
            if t == 0 or t in resets:
                d = O.Diff(rows, cols, DIFF["diff_threshold"], DIFF["blur"], *DC.AREA)
            masks.append(d.detect(DC.oracle_frame(f))[1])
    else:
        o = BC.Oracle(sub_case(rows, cols, channels, 1, alpha))
        for t, f in enumerate(frames):
            if t in resets:
                o.reset()
            masks.append(o.step(f)[3])
    return [T.reference(m, DC.AREA, k) for m in masks]


def triples(ranks):
    return [(r["valid"], r["x"] if r["valid"] else 0.0, r["y"] if r["valid"] else 0.0) for r in ranks]


def image_config():
    return dict(kalman=IMG_KALMAN, gate=IMG_GATE, homography=None, regions=None)


@functools.lru_cache(maxsize=None)
def image_want(family, rows, cols, channels, variant=0, alpha=0.0, k=IMG_K, wrong=None, resets=()):
    """(out[t][i], log) of one camera over its sequence: the tracks run on through a detector's reset"""
    dets = [triples(r) for r, _ in image_targets(family, rows, cols, channels, variant, alpha, k, resets)]
    return TR.run(dets, k, kalman=IMG_KALMAN, gate=IMG_GATE, wrong=wrong)


def variant_of(stream):
    return stream % 3
