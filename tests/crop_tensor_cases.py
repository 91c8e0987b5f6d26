"""Shared, seeded cases of crop tensors (oatgpu_set_target_crop_tensor / oatgpu_crop_tensor_windows_dev) (TEST
INFRASTRUCTURE, no GPU imports: tests/test_crop_tensor_cpu.py checks the cases on the model alone, tests/test_crop_tensor_gpu.py
feeds the same cases to the kernel).  The model is tests/crop_tensor_ref.py; the frames, windows, tracker runs and plans are those of
target crops, tests/crops_cases.py, imported and not edited."""
import functools

import numpy as np

import crop_tensor_ref as TR
import crops_cases as CC
import crops_ref as R

GEOMETRIES, CROP_SIZES, explicit_windows, TRACKER_RUNS, PLAN, PLAN_LONG = (CC.GEOMETRIES, CC.CROP_SIZES, CC.explicit_windows,
                                                                           CC.TRACKER_RUNS, CC.PLAN, CC.PLAN_LONG)
ZOOMS = (1.0, 0.5, 2.0, 1.37)
FLOAT_SIZES = ((5, 4), (16, 12), (64, 128))        # F16 and F32 in the explicit form; U8 takes every crop size
CAPACITY = 11

# ImageNet's statistics in the frame's channel order (BGR), on 0..255 inputs: scale = 1 / (255 std), bias = -mean / std
_MEAN, _STD = (0.406, 0.456, 0.485), (0.225, 0.224, 0.229)
IMAGENET_SCALE = tuple(1.0 / (255.0 * s) for s in _STD)
IMAGENET_BIAS = tuple(-m / s for m, s in zip(_MEAN, _STD))
# a format on which a fused multiply-add and two roundings part (tests/test_crop_tensor_cpu.py counts the inputs on which they do)
FMA_SCALE, FMA_BIAS = 1.0 / 3.0, 1.0 / 7.0

# (name, dtype, scale, bias)
FORMATS = (
    ("u8", "uint8", 1.0, 0.0),
    ("f16_unit", "float16", 1.0 / 255.0, 0.0),
    ("f32_unit", "float32", 1.0 / 255.0, 0.0),
    ("f16_imagenet", "float16", IMAGENET_SCALE, IMAGENET_BIAS),
    ("f32_imagenet", "float32", IMAGENET_SCALE, IMAGENET_BIAS),
    ("f32_fma", "float32", FMA_SCALE, FMA_BIAS),
    ("f16_fma", "float16", FMA_SCALE, FMA_BIAS),
)
FLOAT_FORMATS = FORMATS[1:]


def fmt_for(fmt, channels):
    """(dtype, scale, bias) of a format for a context of `channels`: a GREY context takes the first channel's values"""
    _, dtype, scale, bias = fmt
    if channels == 1:
        scale = scale[0] if isinstance(scale, tuple) else scale
        bias = bias[0] if isinstance(bias, tuple) else bias
    return dtype, scale, bias


def expected(u8, fmt, channels, wrong=None):
    dtype, scale, bias = fmt_for(fmt, channels)
    return TR.convert(u8, dtype, scale, bias, channels, wrong)


# ------------------------------------------------------------------------------------------------------ tracker sequences ----

@functools.lru_cache(maxsize=None)
def sequence_windows(family, rows, cols, variant, alpha, k, axis, zoom, wrong=None):
    """[the k windows] for every frame at a zoom: the oracle chain's targets and shapes through the direction rule"""
    tg = CC.sequence_targets(family, rows, cols, variant, alpha, k)
    sh = CC.sequence_shapes(family, rows, cols, variant, alpha, k) if axis else [None] * len(tg)
    return [TR.zoomed_windows(ranks, shp, axis, zoom, wrong) for (ranks, _), shp in zip(tg, sh)]


@functools.lru_cache(maxsize=None)
def sequence_u8(family, rows, cols, variant, alpha, k, axis, zoom, h, w, channels=3, wrong=None, pairs=()):
    """[uint8 [k, h, w(, 3)]] for every frame of one camera: the windows' pixels before the conversion; computed once, never written
    to.  wrong: one of crop_tensor_ref.WRONG_WINDOW, or "first_of_pair" with pairs = the frames that were the second of a paired
    launch (they are cut from the frame before)."""
    frames = CC.sequence(family, rows, cols, variant, channels)
    window_rule = wrong if wrong in ("zoom_ignored_upright", "gather_at_zoom_1") else None
    out = []
    for t, wins in enumerate(sequence_windows(family, rows, cols, variant, alpha, k, axis, zoom, window_rule)):
        f = frames[t - 1] if wrong == "first_of_pair" and t in pairs else frames[t]
        if wrong == "zoom_u_only" and zoom != 1.0:
            plain = sequence_windows(family, rows, cols, variant, alpha, k, axis, 1.0)[t]
            c = np.stack([TR.crop_u_only(f, win, zoom, h, w) for win in plain])
        else:
            c = np.stack([R.crop(f, win, h, w) for win in wins])
        c.setflags(write=False)
        out.append(c)
    return out


def sequence_valid(family, rows, cols, variant, alpha, k):
    """[bool [k]] for every frame: the ranks' validity"""
    return [np.array([r["valid"] for r in ranks], bool) for ranks, _ in CC.sequence_targets(family, rows, cols, variant, alpha, k)]


def entry_u8(family, rows, cols, n, t, alpha, k, axis, zoom, h, w, channels=3, wrong=None, pairs=()):
    """frame t's entry before the conversion, uint8 [n, k, h, w(, 3)]"""
    return np.stack([sequence_u8(family, rows, cols, CC.variant_of(s), alpha, k, axis, zoom, h, w, channels, wrong, pairs)[t]
                     for s in range(n)])


def calls_of(plan):
    """[(how, first frame, count)] of a plan"""
    out, t = [], 0
    for how, count in plan:
        out.append((how, t, count))
        t += count
    return out


# One run of a tracker under one setting of the switch, into one tensor: the long sequence call -- every entry is taken --, the
# tracker reset, then the plan of steps and short calls from frame 0 again: their frames land in entries that hold windows of the
# long call, so that a window that is not written shows.
RUN_CALLS = tuple(calls_of(PLAN_LONG) + calls_of(PLAN))
RESET_BEFORE = len(PLAN_LONG)                        # the call of RUN_CALLS in front of which the tracker starts over
