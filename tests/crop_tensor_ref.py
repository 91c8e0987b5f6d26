"""The model of crop tensors (oatgpu_set_target_crop_tensor / oatgpu_crop_tensor_windows_dev), written from the text in
include/oatgpu.h and built from the model of target crops, tests/crops_ref.py (TEST INFRASTRUCTURE, no GPU imports:
tests/test_crop_tensor_cpu.py checks it and its cases, the GPU tests compare the kernel with it bit for bit).

A crop tensor element is a window of crops_ref followed by a conversion.  zoomed_windows is the direction rule: crops_ref.windows_of,
then -- for any zoom but 1 -- every valid window becomes a gather along (zoom * ax, zoom * ay), an upright one along (zoom, 0.0);
crops_ref.crop with such a non-unit axis is the window's pixels.  convert is the conversion in numpy (np.float32 multiply, then add,
then .astype(np.float16)); convert_scalar the same for one value in exact rational arithmetic with one explicit rounding per
operation, which tests/test_crop_tensor_cpu.py holds equal to it on all 256 inputs of every format.

deliver() is what a caller sees of the entries: frame set t of a call lands in entry t of a buffer that is never cleared."""
import functools
import struct
from fractions import Fraction

import numpy as np

import crops_ref as R

DTYPES = ("uint8", "float16", "float32")
WRONG_VALUE = ("contracted", "hwc_floats", "half_truncated", "channels_reversed")
WRONG_WINDOW = ("zoom_ignored_upright", "zoom_u_only", "gather_at_zoom_1")
WRONG_ENTRY = ("stale_entry", "entry_is_slot", "first_of_pair")
WRONG = WRONG_VALUE + WRONG_WINDOW + WRONG_ENTRY
ZOOM_MIN, ZOOM_MAX = 1.0 / 16, 16.0


# ----------------------------------------------------------------------------------------------------------- the window ----

def zoomed_windows(ranks, shapes, axis, zoom, wrong=None):
    """The windows of one camera of one frame at a zoom (source pixels per output pixel)"""
    zoom = float(zoom)
    out = []
    for win in R.windows_of(ranks, shapes, axis):
        valid, upright, cx, cy, ax, ay = win
        if wrong == "gather_at_zoom_1" and valid and upright and zoom == 1.0:
            win = R.window(True, False, cx, cy, 1.0, 0.0)
        elif zoom == 1.0 or not valid:
            pass
        elif upright:
            win = win if wrong == "zoom_ignored_upright" else R.window(True, False, cx, cy, zoom, 0.0)
        else:
            win = R.window(True, False, cx, cy, zoom * ax, zoom * ay)            # one fp64 multiply each
        out.append(win)
    return out


def crop_u_only(frame, win, zoom, h, w):
    """A planted mistake: the zoom reaches the window's u direction only -- X = (cx + u * (zoom ax)) - v * ay, Y likewise; win is the
    window at zoom 1 (an upright one along (1, 0))"""
    if not R.is_valid(win):
        return np.zeros((h, w) + frame.shape[2:], np.uint8)
    _, upright, cx, cy, ax, ay = win
    if upright:
        ax, ay = 1.0, 0.0
    jj, ii = np.arange(w, dtype=np.int64) - w // 2, np.arange(h, dtype=np.int64) - h // 2
    u, v = jj.astype(np.float64)[None, :], ii.astype(np.float64)[:, None]
    X = (np.float64(cx) + u * np.float64(zoom * ax)) - v * np.float64(ay)
    Y = (np.float64(cy) + u * np.float64(zoom * ay)) + v * np.float64(ax)
    qx, qy = np.rint(X * 32.0).astype(np.int64), np.rint(Y * 32.0).astype(np.int64)
    sx, sy, fx, fy = qx >> 5, qy >> 5, qx & 31, qy & 31
    if frame.ndim == 3:
        fx, fy = fx[..., None], fy[..., None]
    acc = (R._gather(frame, sy, sx) * ((32 - fx) * (32 - fy)) + R._gather(frame, sy, sx + 1) * (fx * (32 - fy)) +
           R._gather(frame, sy + 1, sx) * ((32 - fx) * fy) + R._gather(frame, sy + 1, sx + 1) * (fx * fy) + 512) >> 10
    return acc.astype(np.uint8)


# ------------------------------------------------------------------------------------------------------- the conversion ----

def per_channel(v, channels):
    """scale or bias as the C ABI takes it: a scalar for every channel, or one value per channel; fp32"""
    a = np.asarray(v, np.float64).reshape(-1)
    a = np.repeat(a, channels) if a.size == 1 else a
    assert a.size == channels, (v, channels)
    return a.astype(np.float32)


def convert(u8, dtype, scale, bias, channels, wrong=None):
    """u8: windows [..., h, w] (channels == 1) or [..., h, w, 3] -> "uint8": the same bytes [..., h, w(, 3)]; "float32" / "float16":
    planar [..., C, h, w], fl32(fl32((float)p * scale[c]) + bias[c]), then to nearest even to half"""
    assert dtype in DTYPES and u8.dtype == np.uint8
    if dtype == "uint8":
        return u8
    x = u8[..., None] if channels == 1 else u8
    assert x.shape[-1] == channels
    s, b = per_channel(scale, channels), per_channel(bias, channels)
    if wrong == "channels_reversed":
        s, b = s[::-1], b[::-1]
    if wrong == "contracted":
        v = np.empty(x.shape, np.float32)
        for c in range(channels):
            v[..., c] = _contracted_table(float(s[c]), float(b[c]))[x[..., c]]
    else:
        v = x.astype(np.float32) * s                                       # fp32 multiply: one rounding
        v = v + b                                                          # fp32 add: one rounding
    assert v.dtype == np.float32
    if wrong != "hwc_floats":
        v = np.moveaxis(v, -1, -3)
    if dtype == "float32":
        return np.ascontiguousarray(v)
    hv = v.astype(np.float16)                                              # to nearest even
    if wrong == "half_truncated":
        over = np.abs(hv.astype(np.float32)) > np.abs(v)
        hv = np.where(over, np.nextafter(hv, np.float16(0)), hv)
    return np.ascontiguousarray(hv)


@functools.lru_cache(maxsize=None)
def _contracted_table(s, b):
    """a planted mistake: fl32(p * s + b) with ONE rounding, for every byte"""
    return np.array([_round(Fraction(p) * Fraction(s) + Fraction(b), "f") for p in range(256)], np.float32)


def _bits(v, code):
    return struct.unpack("<I" if code == "f" else "<H", struct.pack("<" + code, v))[0]


def _round(x, code):
    """the exact rational x to the nearest fp32 ("f") or half ("e"), ties to the even significand; finite values only"""
    near = struct.unpack("<" + code, struct.pack("<" + code, float(x)))[0]                # close by; its neighbours decide
    kind = np.float32 if code == "f" else np.float16
    cands = {float(near), float(np.nextafter(kind(near), kind(np.inf))), float(np.nextafter(kind(near), kind(-np.inf)))}
    best = min(cands, key=lambda v: (abs(Fraction(v) - x), _bits(v, code) & 1))
    assert np.isfinite(best)
    return best


def convert_scalar(p, dtype, scale, bias):
    """one uint8 value p with one channel's scale and bias (Python floats that are fp32 values) -> the element as a Python float"""
    if dtype == "uint8":
        return int(p)
    m = _round(Fraction(int(p)) * Fraction(float(scale)), "f")
    v = _round(Fraction(m) + Fraction(float(bias)), "f")
    return v if dtype == "float32" else _round(Fraction(v), "e")


def same_bits(got, want):
    """bit for bit: integers, or fp32 / fp16 bit patterns"""
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype == np.uint8:
        return bool(np.array_equal(got, want))
    as_int = np.uint32 if got.dtype == np.float32 else np.uint16
    return bool(np.array_equal(np.ascontiguousarray(got).view(as_int), np.ascontiguousarray(want).view(as_int)))


# ------------------------------------------------------------------------------------------------------------ the entries ----

SEQ_SLOTS = 4


def deliver(calls, sets, valid, capacity, wrong=None):
    """What the caller's memory shows behind every call of a run.  calls: [(how, first frame, count)] (crop_tensor_cases.calls_of);
    sets[t] is the entry of frame t ([n, k, ...]), valid[t] its ranks' validity [n, k] (bool).  -> [the view tensor[:count] behind call
    i]; the memory starts as zeros and is never cleared.  (The third mistake of WRONG_ENTRY, the first frame of a pair used for both,
    is a matter of the sets: crop_tensor_cases.sequence_u8.)"""
    buf = np.zeros((capacity,) + sets[0].shape, sets[0].dtype)
    out = []
    for how, t, count in calls:
        for i in range(count):
            cur = sets[t + i]
            entry = i % SEQ_SLOTS if wrong == "entry_is_slot" and how == "seq" else i
            if wrong == "stale_entry":
                keep = ~valid[t + i]
                cur = cur.copy()
                cur[keep] = buf[entry][keep]
            buf[entry] = cur
        out.append(buf[:count].copy())
    return out
