"""Shared, seeded cases of target shapes (oatgpu_set_target_shapes / oatgpu_target_shapes) (TEST INFRASTRUCTURE, no
GPU imports: tests/test_shapes_cpu.py checks the cases on the model alone, tests/test_shapes_gpu.py and
tests/test_shapes_host_gpu.py feed the same cases to the kernels and the binaries).  The model is tests/shapes_ref.py.

Planted masks go through the single-stage detectors: targets_cases' own (imported, not edited) and the ones below, each aimed at
one thing the kernel can get wrong.  Frame sequences go through the three trackers: targets_cases' own, and sequences of three
elongated blobs a camera (a horizontal bar, a vertical bar, a staircase) so that every frame behind a tracker's first frames has
ranks with an axis."""
import functools

import numpy as np

import oracle_lib as O
import shapes_ref as R
import targets_cases as T

KS = (1, 4, 8)
MORPHS = T.MORPHS
BIG = T.BIG
STREAMS = (1, 3, 66)


def _diag(img, y, x, n, w, down=True):
    """a stripe of n steps, w pixels wide, going down-right (down) or up-right"""
    for i in range(n):
        yy = y + i if down else y - i
        img[yy, x + i:x + i + w] = 255


def planted_cases():
    P = T.Planted
    out = []
    # a blob with a hole, a blob inside that hole (no candidate), a second hole touching the first at a corner
    img = np.zeros((48, 64), np.uint8)
    img[4:40, 6:50] = 255
    img[8:30, 10:40] = 0
    img[30:36, 40:46] = 0
    img[14:22, 16:30] = 255
    img[42:46, 8:30] = 255
    out.append(P("hole-48x64", img))
    # one-pixel diagonal lines in both directions (m00 = 0: no candidates, but border pixels in the words of ranked blobs), an
    # 8-connected self-touching shape (two squares joined at a corner, a ring closed by a diagonal contact), thick diagonals
    img = np.zeros((37, 61), np.uint8)
    _diag(img, 2, 2, 8, 1, True)
    _diag(img, 10, 14, 8, 1, False)
    img[4:8, 26:30] = 255
    img[8:12, 30:34] = 255
    img[14:20, 4:10] = 255
    img[15:19, 5:9] = 0
    img[14, 4] = 0
    img[13, 3] = 255
    _diag(img, 22, 4, 10, 4, True)                  # b > 0
    _diag(img, 33, 30, 10, 4, False)                # b < 0
    img[3:6, 40:58] = 255                           # a horizontal bar
    img[10:34, 52:55] = 255                         # a vertical bar
    out.append(P("diag-37x61", img, area=(0.0, BIG)))
    # bars, diagonals and a square at the smallest size; the square sits on the frame's diagonal (x range = y range)
    img = np.zeros((24, 32), np.uint8)
    img[2:10, 2:10] = 255                           # the square: no axis
    img[12:14, 2:14] = 255                          # horizontal bar
    img[3:15, 16:18] = 255                          # vertical bar: vx == 0 before the sign rule
    _diag(img, 16, 2, 6, 3, True)
    _diag(img, 21, 18, 6, 3, False)
    img[3:7, 22:26] = 255                           # equal areas: two 4 x 4
    img[9:13, 24:28] = 255
    out.append(P("axes-24x32", img))
    # blobs across row-group boundaries of 4 and of 16 rows, more blobs than K, unranked blobs in the mask words of ranked ones
    img = np.zeros((48, 64), np.uint8)
    img[2:6, 2:8] = 255                             # rows 3 | 4
    img[13:19, 10:13] = 255                         # rows 15 | 16
    img[30:34, 4:20] = 255                          # rows 31 | 32
    for i in range(9):
        img[22:22 + 1 + i % 3, 3 + 6 * i:3 + 6 * i + 2 + i % 4] = 255
    img[36:46, 40:60] = 255
    img[38:40, 30:36] = 255
    out.append(P("groups-48x64", img))
    # blobs touching each frame edge and corner
    img = np.zeros((37, 61), np.uint8)
    img[0:6, 0:4] = 255
    img[0:3, 52:61] = 255
    img[30:37, 0:9] = 255
    img[33:37, 55:61] = 255
    img[0:4, 20:34] = 255
    img[31:37, 22:30] = 255
    img[12:24, 0:3] = 255
    img[10:20, 57:61] = 255
    img[14:20, 20:40] = 255
    out.append(P("edges-37x61", img))
    # a blob at x > 1000: the per-edge terms pass 2^31; blobs across x = 63 / 64 and the last word's end
    img = np.zeros((64, 1100), np.uint8)
    img[10:30, 1010:1090] = 255
    img[14:26, 1020:1060] = 0
    _diag(img, 34, 1005, 20, 6, True)
    img[40:50, 58:70] = 255
    img[5:8, 60:68] = 255
    img[52:60, 1080:1100] = 255
    img[20:24, 500:530] = 255
    out.append(P("far-64x1100", img))
    # more than one workgroup a stream: the arrival path chooses; blobs in every workgroup's rows, across x = 63 / 64 / 127 / 128
    img = np.zeros((140, 200), np.uint8)
    img[4:20, 50:80] = 255
    img[8:14, 56:70] = 0
    img[40:48, 120:134] = 255
    img[60:100, 10:16] = 255
    _diag(img, 70, 60, 40, 8, True)
    _diag(img, 130, 100, 30, 5, False)
    img[120:136, 150:190] = 255
    img[50:53, 170:196] = 255
    for i in range(6):
        img[24:27 + i % 2, 100 + 9 * i:104 + 9 * i] = 255
    out.append(P("arrival-140x200", img))
    return out


@functools.lru_cache(maxsize=None)
def all_planted():
    """targets_cases' planted cases and this module's"""
    return tuple(T.planted_cases() + planted_cases())


def planted_params(case, morph, kind="thresh"):
    if kind == "hsv":
        return O.hsv_params(h_lo=255, h_hi=256, s_lo=255, s_hi=256, v_lo=255, v_hi=256, erode=morph[0], dilate=morph[1],
                            min_area=case.area[0], max_area=case.area[1])
    return T.thresh_params(case, morph)


@functools.lru_cache(maxsize=None)
def planted_mask(name, morph):
    """the oracle's mask after erode / dilate of a planted case (oat_detect_thresh's thr_out): computed once, never written to"""
    case = next(c for c in all_planted() if c.name == name)
    m = O.detect_thresh(case.img, planted_params(case, morph))[1]
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def planted_reference(name, morph, k):
    case = next(c for c in all_planted() if c.name == name)
    return R.reference(planted_mask(name, morph), case.area, k)


# -------------------------------------------------------------------------------------- frame sequences for the trackers ----

GEOMETRIES = ((48, 64), (37, 61), (24, 32))
N_FRAMES = 11                                       # a host step, a device step, sequence calls of 1, 2 and 5 ... or of 11
TRACKER_K = 4
# frames in front of which a tracker's mask is empty (or one blob) by its own definition: the subtraction tracker's first frame is
# its background; the fused tracker's model sees FUSED_WARM frames of bare background first; the motion tracker's first frame is
# analysed as it is (every pixel differs from nothing)
WARM = dict(motion=1, subtraction=1, fused=T.FUSED_WARM)


@functools.lru_cache(maxsize=None)
def sequence(family, rows, cols, variant=0):
    """frames[t] (rows, cols, 3) of one camera: a horizontal bar, a vertical bar and a staircase in three column bands, moving
    up and down; a fourth, square block comes and goes."""
    from bsub_cases import RECT_BGR
    bg = T._background(rows, cols, variant)
    colour = RECT_BGR if family == "subtraction" else T.BLOCK_BGR
    band = cols // 3
    n = WARM[family] + N_FRAMES - 1 if family == "fused" else N_FRAMES
    frames = []
    for t in range(n):
        f = bg.copy()
        live = t >= WARM[family] if family != "motion" else True
        if live:
            u = t + variant
            bw, bh = min(band - 4, 9), 2
            y = 2 + (2 * u) % (rows - bh - 5)
            f[y:y + bh, 2:2 + bw] = colour                                   # horizontal bar
            vh = min(rows // 3, 9)
            y = 2 + (3 * u + 5) % (rows - vh - 5)
            f[y:y + vh, band + 3:band + 5] = colour                          # vertical bar
            sn = min(rows // 4, band - 5, 7)
            y = 2 + (u + 3) % (rows - sn - 5)
            for i in range(sn):
                xi = 2 * band + 2 + (i if variant % 2 == 0 else sn - 1 - i)
                f[y + i, xi:xi + 2] = colour                                 # staircase: down-right or down-left
            if u % 4 < 2 and rows >= 37:
                y = rows - 9 - u % 3
                f[y:y + 4, band + 9:band + 13] = colour                      # a square that comes and goes
        f.setflags(write=False)
        frames.append(f)
    return frames


@functools.lru_cache(maxsize=None)
def sequence_masks(family, rows, cols, variant=0, alpha=0.0, source="shapes"):
    """the oracle's mask after erode / dilate of every frame; source: this module's sequence or targets_cases'"""
    if source == "targets":
        return tuple(m for _, m in T.sequence_masks(family, rows, cols, variant, alpha))
    frames = sequence(family, rows, cols, variant)
    if family == "motion":
        d = O.Diff(rows, cols, T.DIFF["diff_threshold"], T.DIFF["blur"], *T.AREA)
        out = [d.detect(O.bgr2grey(f))[1] for f in frames]
    elif family == "subtraction":
        b, p = O.Bsub(rows, cols, 3, alpha), T.sub_params()
        out = [O.detect_hsv(O.bgr2hsv(b.filter(f)), p)[1] for f in frames]
    else:
        mog, p = O.Mog2(rows, cols, 3), T.fused_params()
        out = [O.chain_step(mog, f, T.FUSED_LR, p)[1] for f in frames]
    for m in out:
        m.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def sequence_reference(family, rows, cols, variant=0, alpha=0.0, k=TRACKER_K, source="shapes"):
    """[the k ranks' shapes] for every frame"""
    return [R.reference(m, T.AREA, k) for m in sequence_masks(family, rows, cols, variant, alpha, source)]


@functools.lru_cache(maxsize=None)
def sequence_targets(family, rows, cols, variant=0, alpha=0.0, k=TRACKER_K, source="shapes"):
    """[(ranks, n_found)] for every frame: targets_cases.reference on the same masks"""
    return [T.reference(m, T.AREA, k) for m in sequence_masks(family, rows, cols, variant, alpha, source)]


def frames_of(family, rows, cols, variant=0, source="shapes"):
    return T.sequence(family, rows, cols, variant) if source == "targets" else sequence(family, rows, cols, variant)


variant_of = T.variant_of
