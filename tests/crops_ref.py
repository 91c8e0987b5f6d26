"""The model of target crops (oatgpu_set_target_crops / oatgpu_target_crops / oatgpu_crop_windows_dev), written from
the text in include/oatgpu.h alone (TEST INFRASTRUCTURE, no GPU imports: tests/test_crops_cpu.py checks it and its cases, the GPU
tests compare the kernel with it bit for bit).

A window is (valid, upright, cx, cy, ax, ay).  crop_scalar is the contract pixel by pixel in Python ints and floats (IEEE doubles,
one rounding per operation; round() rounds half to even); crop is the same in numpy (float64 ufuncs: one rounding each, nothing
contracted), the form the GPU tests use.  tests/test_crops_cpu.py holds the two equal on every case.

In the trackers the windows come from targets_cases.reference (the rank's valid, x, y) and shapes_ref.reference (axis_valid,
axis_x, axis_y) on the oracle's own mask: windows_of."""
import math

import numpy as np

WRONG_PIXEL = ("half_up", "truncated_centre", "ay_negated", "replicated_border", "rgb_order", "fractions_swapped")
WRONG_SET = ("stale_crop", "stream0_frame", "first_of_pair")
WRONG = WRONG_PIXEL + WRONG_SET
LIMIT = 1e6                       # |cx|, |cy| beyond: no window
Q_LIMIT = 1 << 30                 # |rint(X * 32)| from here on: outside every frame


def window(valid, upright, cx, cy, ax=0.0, ay=0.0):
    return (bool(valid), bool(upright), float(cx), float(cy), float(ax), float(ay))


INVALID = window(False, True, 0.0, 0.0)


def is_valid(win):
    valid, _, cx, cy, ax, ay = win
    return bool(valid) and all(math.isfinite(v) for v in (cx, cy, ax, ay)) and abs(cx) <= LIMIT and abs(cy) <= LIMIT


def _shape(frame, h, w):
    return (h, w) + frame.shape[2:]


# ------------------------------------------------------------------------------------------------ the contract, by pixel ----

def _round_centre(c, wrong):
    if wrong == "half_up":
        return int(math.floor(c + 0.5))
    if wrong == "truncated_centre":
        return int(c)
    return int(round(c))                              # half to even, as cvRound


def _px(frame, y, x, wrong=None):
    """frame(y, x), all channels, as ints; outside the frame 0"""
    H, W = frame.shape[:2]
    if wrong == "replicated_border":
        y, x = min(max(y, 0), H - 1), min(max(x, 0), W - 1)
    if 0 <= y < H and 0 <= x < W:
        return [int(v) for v in np.atleast_1d(frame[y, x])]
    return [0] * (frame.shape[2] if frame.ndim == 3 else 1)


def sample_position(win, h, w, i, j, wrong=None):
    """Axis mode: (qx, qy) of output pixel (i, j), or None where the position lies outside every frame"""
    _, _, cx, cy, ax, ay = win
    if wrong == "ay_negated":
        ay = -ay
    u, v = float(j - w // 2), float(i - h // 2)
    X = (cx + u * ax) - v * ay
    Y = (cy + u * ay) + v * ax
    qxf, qyf = X * 32.0, Y * 32.0
    if not (math.isfinite(qxf) and math.isfinite(qyf)):
        return None
    qx, qy = int(round(qxf)), int(round(qyf))
    if abs(qx) >= Q_LIMIT or abs(qy) >= Q_LIMIT:
        return None
    return qx, qy


def crop_scalar(frame, win, h, w, wrong=None):
    """One window of one frame ((H, W) or (H, W, 3) uint8), pixel by pixel"""
    out = np.zeros(_shape(frame, h, w), np.uint8)
    if not is_valid(win):
        return out
    _, upright, cx, cy, _, _ = win
    for i in range(h):
        for j in range(w):
            if upright:
                px = _px(frame, _round_centre(cy, wrong) - h // 2 + i, _round_centre(cx, wrong) - w // 2 + j, wrong)
            else:
                q = sample_position(win, h, w, i, j, wrong)
                if q is None:
                    continue
                qx, qy = q
                sx, sy, fx, fy = qx >> 5, qy >> 5, qx & 31, qy & 31
                if wrong == "fractions_swapped":
                    fx, fy = fy, fx
                c00, c01, c10, c11 = (_px(frame, sy, sx, wrong), _px(frame, sy, sx + 1, wrong), _px(frame, sy + 1, sx, wrong),
                                      _px(frame, sy + 1, sx + 1, wrong))
                px = [(a * (32 - fx) * (32 - fy) + b * fx * (32 - fy) + c * (32 - fx) * fy + d * fx * fy + 512) >> 10
                      for a, b, c, d in zip(c00, c01, c10, c11)]
            if wrong == "rgb_order":
                px = px[::-1]
            out[i, j] = px if frame.ndim == 3 else px[0]
    return out


# ---------------------------------------------------------------------------------------------- the contract, in numpy ----

def _gather(frame, y, x):
    """frame[y, x] as int64 with 0 outside the frame; y, x int64 arrays of one shape"""
    H, W = frame.shape[:2]
    inside = (y >= 0) & (y < H) & (x >= 0) & (x < W)
    v = frame[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)].astype(np.int64)
    return np.where(inside[..., None] if frame.ndim == 3 else inside, v, 0)


def crop(frame, win, h, w):
    """crop_scalar(frame, win, h, w), vectorised"""
    if not is_valid(win):
        return np.zeros(_shape(frame, h, w), np.uint8)
    _, upright, cx, cy, ax, ay = win
    jj, ii = np.arange(w, dtype=np.int64) - w // 2, np.arange(h, dtype=np.int64) - h // 2
    if upright:
        y = (int(round(cy)) + ii)[:, None] + np.zeros((1, w), np.int64)
        x = (int(round(cx)) + jj)[None, :] + np.zeros((h, 1), np.int64)
        return _gather(frame, y, x).astype(np.uint8)
    u, v = jj.astype(np.float64)[None, :], ii.astype(np.float64)[:, None]
    cx, cy, ax, ay = (np.float64(t) for t in (cx, cy, ax, ay))
    with np.errstate(all="ignore"):
        X = (cx + u * ax) - v * ay
        Y = (cy + u * ay) + v * ax
        qxf, qyf = np.rint(X * 32.0), np.rint(Y * 32.0)
        ok = (np.abs(qxf) < Q_LIMIT) & (np.abs(qyf) < Q_LIMIT)                 # (false for a NaN)
    qx = np.where(ok, qxf, 0.0).astype(np.int64)
    qy = np.where(ok, qyf, 0.0).astype(np.int64)
    sx, sy, fx, fy = qx >> 5, qy >> 5, qx & 31, qy & 31
    if frame.ndim == 3:
        fx, fy, ok = fx[..., None], fy[..., None], ok[..., None]
    acc = (_gather(frame, sy, sx) * ((32 - fx) * (32 - fy)) + _gather(frame, sy, sx + 1) * (fx * (32 - fy)) +
           _gather(frame, sy + 1, sx) * ((32 - fx) * fy) + _gather(frame, sy + 1, sx + 1) * (fx * fy) + 512) >> 10
    return np.where(ok, acc, 0).astype(np.uint8)


def crop_set(frames, windows, h, w):
    """frames[s]: one camera's frame; windows[s]: its windows -> uint8 [n, per_stream, h, w(, 3)]"""
    return np.stack([np.stack([crop(f, win, h, w) for win in wins]) for f, wins in zip(frames, windows)])


# ------------------------------------------------------------------------------------------------- windows in the trackers ----

def windows_of(ranks, shapes, axis):
    """The windows of one camera of one frame: ranks -- targets_cases.reference(...)[0], shapes -- shapes_ref.reference(...) (or
    None while axis is False)"""
    out = []
    for j, r in enumerate(ranks):
        if not r["valid"]:
            out.append(INVALID)
        elif axis and shapes[j]["valid"] and shapes[j]["axis_valid"]:
            out.append(window(True, False, r["x"], r["y"], shapes[j]["axis_x"], shapes[j]["axis_y"]))
        else:
            out.append(window(True, True, r["x"], r["y"]))
    return out


# ---------------------------------------------------------------------------------------------------- planted wrong croppers ----

def wrong_sequence(frames, windows, h, w, wrong, pairs=()):
    """A sequence of crop sets from a cropper with one rule replaced.  frames[t][s], windows[t][s] -> [crop set of frame t];
    pairs: the t whose frame was the second of a paired launch."""
    out, previous = [], None
    for t, (fs, ws) in enumerate(zip(frames, windows)):
        if wrong == "stream0_frame":
            fs = [fs[0]] * len(fs)
        if wrong == "first_of_pair" and t in pairs:
            fs = frames[t - 1]
        if wrong in WRONG_PIXEL:
            cur = np.stack([np.stack([crop_scalar(f, win, h, w, wrong) for win in wins]) for f, wins in zip(fs, ws)])
        else:
            cur = crop_set(fs, ws, h, w)
        if wrong == "stale_crop" and previous is not None:
            for s, wins in enumerate(ws):
                for j, win in enumerate(wins):
                    if not is_valid(win):
                        cur[s, j] = previous[s, j]
        out.append(cur)
        previous = cur
    return out
