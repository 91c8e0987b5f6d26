"""The model of target masks (oatgpu_set_target_mask_tensor / oatgpu_target_mask_tensor_sets), written from the text in
include/oatgpu.h ("target masks") (TEST INFRASTRUCTURE, no GPU imports: tests/test_target_masks_cpu.py checks it and its cases, the
GPU tests compare the kernel with it bit for bit).

An element of a mask is ON where its source pixel lies inside the frame, is set in the final mask -- the mask after erode / dilate
with the one-pixel frame zeroed -- and belongs to the 8-connected component whose first pixel in raster order is the rank's
first_pixel.  label8 is that labelling, dependency-free; windows_mask cuts the windows of crop_tensor_ref.zoomed_windows out of
it (numpy: float64 ufuncs, one rounding each); element_scalar is one element in Python ints and floats.  deliver is
crop_tensor_ref's: frame set t of a call lands in entry t of a buffer that is never cleared."""
import numpy as np

import crop_tensor_ref as TR
import crops_ref as R

DTYPES = TR.DTYPES
deliver = TR.deliver
same_bits = TR.same_bits
WRONG_LABEL = ("four_connected", "any_foreground", "frame_not_zeroed", "holes_filled", "rank0_root", "head_in_word")
WRONG_PIXEL = ("no_plus_16", "rint_x")
WRONG_ENTRY = ("entry_is_slot", "first_of_pair", "stale_entry")
WRONG_VALUE = ("on_is_1",)
WRONG = WRONG_LABEL + WRONG_PIXEL + WRONG_ENTRY + WRONG_VALUE


# ------------------------------------------------------------------------------------------------------------ labelling ----

def zero_frame(mask):
    """the mask findContours sees: foreground as bool, the one-pixel frame zeroed"""
    fg = np.zeros(mask.shape, bool)
    if mask.shape[0] > 2 and mask.shape[1] > 2:
        fg[1:-1, 1:-1] = np.asarray(mask)[1:-1, 1:-1] != 0
    return fg


def _label(fg, eight=True):
    """-> int64 [rows, cols]: for every foreground pixel the raster index (y * cols + x) of the first pixel of its component, -1 for
    background.  A flood fill from every unseen pixel in raster order: the seed IS the component's first pixel."""
    rows, cols = fg.shape
    first = np.full((rows, cols), -1, np.int64)
    steps = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy or dx) and (eight or not (dy and dx))]
    for y, x in zip(*np.nonzero(fg)):
        if first[y, x] >= 0:
            continue
        seed = int(y) * cols + int(x)
        first[y, x] = seed
        stack = [(int(y), int(x))]
        while stack:
            cy, cx = stack.pop()
            for dy, dx in steps:
                ny, nx = cy + dy, cx + dx
                if 0 <= ny < rows and 0 <= nx < cols and fg[ny, nx] and first[ny, nx] < 0:
                    first[ny, nx] = seed
                    stack.append((ny, nx))
    return first


def label8(mask):
    """The 8-connected labelling of the frame-zeroed mask, by first pixel (see _label)"""
    return _label(zero_frame(mask), True)


def labels_for(mask, wrong=None):
    """label8(mask), or one of the planted labellings"""
    if wrong == "four_connected":
        return _label(zero_frame(mask), False)
    if wrong == "frame_not_zeroed":
        return _label(np.asarray(mask) != 0, True)
    first = label8(mask)
    if wrong == "any_foreground":
        return np.where(first >= 0, -2, -1)                       # (-2: "some foreground"; own_pixels knows)
    if wrong == "holes_filled":
        return _fill_holes(first)
    if wrong == "head_in_word":
        return _heads_in_words(first)
    return first


def _fill_holes(first):
    """a planted mistake: everything a component encloses -- its holes and what lies in them -- counts as the component"""
    rows, cols = first.shape
    out = first.copy()
    for seed in np.unique(first[first >= 0]):
        comp = first == seed
        padded = np.zeros((rows + 2, cols + 2), bool)
        padded[1:-1, 1:-1] = ~comp
        padded[0, :] = padded[-1, :] = padded[:, 0] = padded[:, -1] = True
        outside = _label(padded, False) == 0                      # the 4-connected background that reaches the border
        out[~outside[1:-1, 1:-1] & ~comp] = seed
    return out


def _heads_in_words(first):
    """a planted mistake: the start of a pixel's run is looked for inside the pixel's own 64-pixel word only; a run that entered the
    word from the left is not found and its pixels belong to nothing"""
    out = first.copy()
    fg = first >= 0
    rows, cols = first.shape
    for y in range(rows):
        for x0 in range(64, cols, 64):
            if fg[y, x0] and fg[y, x0 - 1]:                       # a run crosses into this word
                x = x0
                while x < cols and x < x0 + 64 and fg[y, x]:
                    out[y, x] = -1
                    x += 1
    return out


def own_pixels(first, rank_first_pixel):
    """bool [rows, cols]: the pixels of the component whose first pixel is rank_first_pixel"""
    if (first == -2).any():                                       # "any_foreground"
        return first == -2
    return first == rank_first_pixel


# ----------------------------------------------------------------------------------------------------------- the window ----

def source_pixels(win, h, w, wrong=None):
    """(x, y, ok) int64 / bool [h, w] of a valid window: the source pixel of every element; ok False where the position lies outside
    every frame"""
    _, upright, cx, cy, ax, ay = win
    jj, ii = np.arange(w, dtype=np.int64) - w // 2, np.arange(h, dtype=np.int64) - h // 2
    if upright:
        y = (int(round(cy)) + ii)[:, None] + np.zeros((1, w), np.int64)
        x = (int(round(cx)) + jj)[None, :] + np.zeros((h, 1), np.int64)
        return x, y, np.ones((h, w), bool)
    u, v = jj.astype(np.float64)[None, :], ii.astype(np.float64)[:, None]
    cx, cy, ax, ay = (np.float64(t) for t in (cx, cy, ax, ay))
    with np.errstate(all="ignore"):
        X = (cx + u * ax) - v * ay
        Y = (cy + u * ay) + v * ax
        qxf, qyf = np.rint(X * 32.0), np.rint(Y * 32.0)
        ok = (np.abs(qxf) < R.Q_LIMIT) & (np.abs(qyf) < R.Q_LIMIT)             # (false for a NaN)
        if wrong == "rint_x":
            return (np.where(ok, np.rint(X), 0.0).astype(np.int64), np.where(ok, np.rint(Y), 0.0).astype(np.int64), ok)
    qx, qy = np.where(ok, qxf, 0.0).astype(np.int64), np.where(ok, qyf, 0.0).astype(np.int64)
    if wrong == "no_plus_16":
        return qx >> 5, qy >> 5, ok
    return (qx + 16) >> 5, (qy + 16) >> 5, ok


def window_on(first, rank, win, h, w, wrong=None):
    """bool [h, w]: the ON elements of one rank's window; first: labels_for(mask)"""
    if not rank["valid"] or not R.is_valid(win):
        return np.zeros((h, w), bool)
    rows, cols = first.shape
    x, y, ok = source_pixels(win, h, w, wrong)
    inside = ok & (x >= 0) & (x < cols) & (y >= 0) & (y < rows)
    own = own_pixels(first, rank["first_pixel"])
    return inside & own[np.clip(y, 0, rows - 1), np.clip(x, 0, cols - 1)]


def to_dtype(on, dtype, wrong=None):
    assert dtype in DTYPES
    if dtype == "uint8":
        return on.astype(np.uint8) * np.uint8(1 if wrong == "on_is_1" else 255)
    return on.astype(np.float16 if dtype == "float16" else np.float32)


def windows_mask(mask, ranks, windows, h, w, dtype, wrong=None):
    """One camera of one frame: mask -- the oracle's mask after erode / dilate; ranks -- targets_cases.reference(...)[0]; windows --
    crop_tensor_ref.zoomed_windows(...) -> [k, h, w] of the dtype"""
    first = labels_for(mask, wrong if wrong in WRONG_LABEL else None)
    out = []
    for j, (rank, win) in enumerate(zip(ranks, windows)):
        r = ranks[0] if wrong == "rank0_root" and rank["valid"] else rank
        out.append(window_on(first, r, win, h, w, wrong if wrong in WRONG_PIXEL else None))
    return to_dtype(np.stack(out), dtype, wrong)


# ------------------------------------------------------------------------------------------------ the contract, by element ----

def element_scalar(mask, rank, win, h, w, i, j):
    """One element in Python ints and floats (IEEE doubles, one rounding per operation; round() rounds half to even) -> bool"""
    if not rank["valid"] or not R.is_valid(win):
        return False
    _, upright, cx, cy, _, _ = win
    if upright:
        x, y = int(round(cx)) - w // 2 + j, int(round(cy)) - h // 2 + i
    else:
        q = R.sample_position(win, h, w, i, j)
        if q is None:
            return False
        x, y = (q[0] + 16) >> 5, (q[1] + 16) >> 5
    rows, cols = mask.shape
    if not (0 <= x < cols and 0 <= y < rows):
        return False
    if not (0 < x < cols - 1 and 0 < y < rows - 1) or mask[y, x] == 0:         # the frame is zeroed; the bit is not set
        return False
    # the component of (x, y), pixel by pixel, until the rank's first pixel is met or the component is exhausted
    fy, fx = divmod(int(rank["first_pixel"]), cols)
    seen, stack = {(y, x)}, [(y, x)]
    while stack:
        cy_, cx_ = stack.pop()
        if (cy_, cx_) == (fy, fx):
            return True
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                ny, nx = cy_ + dy, cx_ + dx
                if 0 < ny < rows - 1 and 0 < nx < cols - 1 and mask[ny, nx] != 0 and (ny, nx) not in seen:
                    seen.add((ny, nx))
                    stack.append((ny, nx))
    return False
