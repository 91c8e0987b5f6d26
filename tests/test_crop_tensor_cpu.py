"""CPU tests of crop tensors: the model of tests/crop_tensor_ref.py and the cases of tests/crop_tensor_cases.py are
checked on their own -- the scalar and the numpy form of the conversion agree, the cases reach what they are aimed at, ten planted
wrong implementations each differ somewhere -- then the header, the struct, the binding and the exports.

Non-vacuity is a condition on the model alone.  An entry is what a stale window would survive in: frame i of a call lands in entry i
of the caller's memory, so "an invalid rank following a valid one in the same entry" is asked of the frame that took the entry in
the call before, under the plan the GPU test runs."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import crop_tensor_cases as TC
import crop_tensor_ref as TR
import crops_cases as CC
import crops_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("oatgpu_set_target_crop_tensor", "oatgpu_target_crop_tensor_sets", "oatgpu_crop_tensor_windows_dev")
ALL_BYTES = np.arange(256, dtype=np.uint8)


def _runs():
    for family, alpha, rows, cols, n, k, h, w in TC.TRACKER_RUNS:
        yield family, alpha, rows, cols, min(n, 3), k, h, w


def _small_runs():
    return [r for r in _runs() if r[6] * r[7] <= 1024]


# ------------------------------------------------------------------------------------------------ the two forms of the model ----

@pytest.mark.parametrize("fmt", TC.FORMATS, ids=[f[0] for f in TC.FORMATS])
def test_the_scalar_and_the_numpy_form_of_the_conversion_agree_on_every_byte(fmt):
    for channels in (1, 3):
        dtype, scale, bias = TC.fmt_for(fmt, channels)
        s, b = TR.per_channel(scale, channels), TR.per_channel(bias, channels)
        u8 = np.repeat(ALL_BYTES[:, None], channels, axis=1).reshape(16, 16, channels)
        got = TR.convert(u8[..., 0] if channels == 1 else u8, dtype, scale, bias, channels)
        if dtype == "uint8":
            assert got.dtype == np.uint8 and np.array_equal(got, u8[..., 0] if channels == 1 else u8)
            continue
        assert got.shape == (channels, 16, 16) and got.dtype == np.dtype(dtype)
        for c in range(channels):
            want = np.array([TR.convert_scalar(p, dtype, float(s[c]), float(b[c])) for p in range(256)], np.float64).astype(dtype)
            assert TR.same_bits(got[c].reshape(-1), want), (fmt[0], channels, c)


def test_rounding_to_the_nearest_even():
    assert TR._round(Fraction(1) + Fraction(1, 2 ** 24), "f") == 1.0                      # a tie: the even neighbour
    assert TR._round(Fraction(1) + Fraction(3, 2 ** 24), "f") == 1.0 + 2.0 ** -22
    assert TR._round(Fraction(1) + Fraction(1, 2 ** 11), "e") == 1.0
    assert TR._round(Fraction(1) + Fraction(3, 2 ** 11), "e") == 1.0 + 2.0 ** -9
    assert TR._round(Fraction(1) + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 80), "f") == 1.0 + 2.0 ** -23      # just above a tie


def test_one_format_separates_a_fused_multiply_add_from_two_roundings():
    fmt = next(f for f in TC.FORMATS if f[0] == "f32_fma")
    s, b = np.float32(fmt[2]), np.float32(fmt[3])
    two = np.array([TR.convert_scalar(p, "float32", float(s), float(b)) for p in range(256)])
    fused = np.array([TR._round(Fraction(p) * Fraction(float(s)) + Fraction(float(b)), "f") for p in range(256)])
    assert (two != fused).sum() >= 1, "pick another scale and bias"
    assert (two == fused).sum() >= 1


def test_a_zoomed_window_is_a_gather_with_a_non_unit_axis():
    ranks = [dict(valid=True, x=10.5, y=7.25), dict(valid=True, x=3.0, y=4.0), dict(valid=False, x=0.0, y=0.0)]
    shapes = [dict(valid=True, axis_valid=True, axis_x=0.6, axis_y=-0.8), dict(valid=True, axis_valid=False, axis_x=0.0, axis_y=0.0),
              dict(valid=False, axis_valid=False, axis_x=0.0, axis_y=0.0)]
    assert TR.zoomed_windows(ranks, shapes, True, 1.0) == R.windows_of(ranks, shapes, True)
    assert TR.zoomed_windows(ranks, None, False, 1.0) == R.windows_of(ranks, None, False)
    a, b, c = TR.zoomed_windows(ranks, shapes, True, 1.37)
    assert a == (True, False, 10.5, 7.25, 1.37 * 0.6, 1.37 * -0.8) and b == (True, False, 3.0, 4.0, 1.37, 0.0) and c == R.INVALID
    a, b, c = TR.zoomed_windows(ranks, None, False, 0.5)
    assert a == (True, False, 10.5, 7.25, 0.5, 0.0) and b == (True, False, 3.0, 4.0, 0.5, 0.0) and c == R.INVALID
    # zoom 2 on whole-pixel centres: every second pixel of the frame, exactly
    f = CC.pattern(48, 64, 3, 0)
    got = R.crop(f, (True, False, 32.0, 24.0, 2.0, 0.0), 8, 8)
    assert np.array_equal(got, f[24 - 8:24 + 8:2, 32 - 8:32 + 8:2])


# ------------------------------------------------------------------------------------------------------- the cases reach ----

def test_every_tracker_sequence_has_what_the_rules_need_at_every_zoom():
    """per sequence and zoom: a valid rank with and one without an axis; per sequence, and per zoom: a window the frame clips (a
    small window at zoom 0.5 covers a few pixels only -- not every sequence has a blob that close to an edge)"""
    clipped_at = {z: False for z in TC.ZOOMS}
    for family, alpha, rows, cols, n, k, h, w in _runs():
        for plan in (TC.PLAN, TC.PLAN_LONG):
            count = sum(c for _, c in plan)
            clipped = False
            for zoom in TC.ZOOMS:
                axis0 = axis1 = found = False
                for s in range(n):
                    v = CC.variant_of(s)
                    wins = TC.sequence_windows(family, rows, cols, v, alpha, k, True, zoom)
                    plain = CC.sequence_windows(family, rows, cols, v, alpha, k, True)
                    for t in range(count):
                        for win, was in zip(wins[t], plain[t]):
                            if not R.is_valid(win):
                                continue
                            axis0 |= was[1]
                            axis1 |= not was[1]
                            if not found:                                                   # (a pixel loop: until one is found)
                                cov = CC.coverage(win, rows, cols, h, w)
                                if cov["inside"] and (cov["left"] or cov["right"] or cov["top"] or cov["bottom"]):
                                    found = clipped = clipped_at[zoom] = True
                            assert (win[1] and zoom == 1.0) or not win[1]                   # any other zoom: always the gather
                assert axis0 and axis1, (family, alpha, rows, cols, k, zoom, axis0, axis1)
            assert clipped, (family, alpha, rows, cols, k)
    assert all(clipped_at.values()), clipped_at


def test_an_invalid_rank_follows_a_valid_one_in_the_same_entry():
    """under the run the GPU test makes: what held the entry before is the latest earlier call with that many frames"""
    for family, alpha, rows, cols, n, k, h, w in _runs():
        hit = False
        for s in range(n):
            valid = TC.sequence_valid(family, rows, cols, CC.variant_of(s), alpha, k)
            held = {}
            for _, t0, count in TC.RUN_CALLS:
                for e in range(count):
                    if e in held:
                        hit |= bool((valid[held[e]] & ~valid[t0 + e]).any())
                    held[e] = t0 + e
        assert hit, (family, alpha, rows, cols, k)
    assert [c for _, _, c in TC.RUN_CALLS] == [11, 1, 1, 1, 2, 5] and TC.RESET_BEFORE == 1


# ---------------------------------------------------------------------------------------------- planted wrong implementations ----

def _sets(run, axis, zoom, fmt, wrong_u8=None, wrong_value=None, pairs=()):
    family, alpha, rows, cols, n, k, h, w = run
    return [TC.expected(TC.entry_u8(family, rows, cols, n, t, alpha, k, axis, zoom, h, w, 3, wrong_u8, pairs), fmt, 3, wrong_value)
            for t in range(CC.N_FRAMES)]


def _fmt(name):
    return next(f for f in TC.FORMATS if f[0] == name)


@pytest.mark.parametrize("wrong", TR.WRONG)
def test_a_planted_wrong_implementation_differs(wrong):
    runs = _small_runs()
    assert runs
    if wrong in TR.WRONG_VALUE:
        names = {"contracted": ("f32_fma",), "hwc_floats": ("f16_unit", "f32_unit"),
                 "half_truncated": ("f16_unit", "f16_imagenet"), "channels_reversed": ("f16_imagenet", "f32_imagenet")}[wrong]
        for run in runs:
            for name in names:
                good, bad = _sets(run, True, 1.0, _fmt(name)), _sets(run, True, 1.0, _fmt(name), wrong_value=wrong)
                assert any(a.shape != b.shape or not TR.same_bits(a, b) for a, b in zip(good, bad)), (wrong, run, name)
        return
    if wrong in TR.WRONG_WINDOW:
        for run in runs:
            zooms = (1.0,) if wrong == "gather_at_zoom_1" else tuple(z for z in TC.ZOOMS if z != 1.0)
            for zoom in zooms:
                # without the axis every valid rank is upright: the mistakes that concern upright windows show there
                good, bad = _sets(run, False, zoom, _fmt("u8")), _sets(run, False, zoom, _fmt("u8"), wrong_u8=wrong)
                assert any(not np.array_equal(a, b) for a, b in zip(good, bad)), (wrong, run, zoom)
                if wrong == "zoom_u_only":
                    good, bad = _sets(run, True, zoom, _fmt("u8")), _sets(run, True, zoom, _fmt("u8"), wrong_u8=wrong)
                    assert any(not np.array_equal(a, b) for a, b in zip(good, bad)), (wrong, run, zoom, "axis")
        return
    for run in runs:
        family, alpha, rows, cols, n, k, h, w = run
        valid = [np.stack([TC.sequence_valid(family, rows, cols, CC.variant_of(s), alpha, k)[t] for s in range(n)])
                 for t in range(CC.N_FRAMES)]
        for fmt in (_fmt("u8"), _fmt("f16_imagenet")):
            good = _sets(run, True, 2.0, fmt)
            if wrong == "first_of_pair":
                for plan in (TC.PLAN, TC.PLAN_LONG):
                    pairs = tuple(sorted(CC.paired_second(family, plan)))
                    assert pairs
                    bad = _sets(run, True, 2.0, fmt, wrong_u8=wrong, pairs=pairs)
                    assert any(not TR.same_bits(a, b) for a, b in zip(good, bad)), (wrong, run, plan)
                continue
            a = TR.deliver(TC.RUN_CALLS, good, valid, TC.CAPACITY)
            b = TR.deliver(TC.RUN_CALLS, good, valid, TC.CAPACITY, wrong)
            differs = [not TR.same_bits(x, y) for x, y in zip(a, b)]
            assert any(differs), (wrong, run)
            if wrong == "entry_is_slot":                                                # exactly the 5- and the 11-frame sequence call
                assert differs == [count > TR.SEQ_SLOTS for _, _, count in TC.RUN_CALLS], (run, differs)


def test_the_model_delivers_what_it_is_given_where_nothing_is_replaced():
    run = _small_runs()[0]
    family, alpha, rows, cols, n, k, h, w = run
    good = _sets(run, False, 0.5, _fmt("f32_unit"))
    valid = [np.ones((n, k), bool)] * CC.N_FRAMES
    for (how, t0, count), got in zip(TC.RUN_CALLS, TR.deliver(TC.RUN_CALLS, good, valid, TC.CAPACITY)):
        assert len(got) == count and all(TR.same_bits(got[i], good[t0 + i]) for i in range(count))
    assert len(TR.WRONG) == 10 and len(set(TR.WRONG)) == 10
    assert TC.ZOOMS == (1.0, 0.5, 2.0, 1.37) and all(TR.ZOOM_MIN <= z <= TR.ZOOM_MAX for z in TC.ZOOMS)
    assert set(TC.FLOAT_SIZES) <= set(TC.CROP_SIZES)


# --------------------------------------------------------------------------------------------- header, library, binding ----

@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(ROOT, "oat_amd", "lib", "liboatgpu.so")):
        subprocess.check_call(["make", "-s", "-j4", "-C", ROOT, "oat_amd/lib/liboatgpu.so"])
    from oat_amd import ffi
    return ffi.load()


def test_crop_tensors_are_declared_exported_and_bound(lib, tmp_path):
    from oat_amd import ffi
    header = open(os.path.join(ROOT, "include", "oatgpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(lib, name) and name in ffi.SIGNATURES
    fmtp = C.POINTER(ffi.CropTensorFmt)
    assert ffi.SIGNATURES["oatgpu_set_target_crop_tensor"][1] == [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, fmtp,
                                                                  C.c_void_p, C.c_int32]
    assert ffi.SIGNATURES["oatgpu_target_crop_tensor_sets"][1] == [C.c_void_p]
    assert ffi.SIGNATURES["oatgpu_crop_tensor_windows_dev"][1] == [C.c_void_p, C.c_void_p, C.POINTER(ffi.CropWindow), C.c_int32, C.c_int32,
                                                                   C.c_int32, fmtp, C.c_void_p]
    fields = ("dtype", "reserved", "scale", "bias")
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "oatgpu.h"\nint main(){printf("%zu ' + "%zu " * len(fields) +
                   '%d %d %d %d\\n",sizeof(oatgpu_crop_tensor_fmt),' + ",".join("offsetof(oatgpu_crop_tensor_fmt,%s)" % f for f in fields) +
                   ',OATGPU_TENSOR_U8,OATGPU_TENSOR_F16,OATGPU_TENSOR_F32,OATGPU_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "t"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    want = [32, 0, 4, 8, 20, 0, 1, 2, 9]
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want
    assert [C.sizeof(ffi.CropTensorFmt)] + [getattr(ffi.CropTensorFmt, f).offset for f in fields] == want[:5]
    assert [ffi.TENSOR_U8, ffi.TENSOR_F16, ffi.TENSOR_F32] == want[5:8]
    assert ffi.ABI_VERSION == 9 == lib.oatgpu_abi_version()                     # additive entries: the version stays


def test_the_header_states_the_semantics():
    header = open(os.path.join(ROOT, "include", "oatgpu.h")).read()
    text = " ".join(" ".join(re.sub(r"^\s*\*\s", "", line) for line in header.splitlines()).split())
    for words in ("(zoom * axis_x, zoom * axis_y)", "(zoom, 0.0) otherwise", "one fp64 multiply", "used as given, not normalised",
                  "source pixels per output pixel", "point-sampled bilinear, not an area filter", "1/16 <= zoom <= 16",
                  "fl32(fl32((float)p * scale[c]) + bias[c])", "no fused multiply-add", "rounded to nearest even",
                  "holds bias[c]", "interleaved [h][w][C]", "planar [C][h][w]", "CALLER-OWNED DEVICE memory", "16-byte aligned",
                  "never allocates, frees or copies it", "entries past the delivered count are not touched",
                  "before anything is launched and with nothing changed", "independent of oatgpu_set_target_crops",
                  "The fused tracker's own calls and the single-stage detectors deliver none", "There is no zoom argument"):
        assert words.lower() in text.lower(), words


def test_every_detector_class_has_crop_tensors():
    import oat_amd.components as comp
    for cls in ("HotPath", "MotionTracker", "SubtractionTracker", "HSVDetector", "SimpleThreshold", "DifferenceDetector"):
        k = getattr(comp, cls)
        assert all(callable(getattr(k, m, None)) for m in ("set_target_crop_tensor", "target_crop_tensor", "crop_tensor_windows")), cls


def test_the_binding_does_not_import_torch_at_module_level():
    for name in ("ffi.py", "components.py"):
        src = open(os.path.join(ROOT, "oat_amd", name)).read()
        assert not re.search(r"^(import torch|from torch)", src, flags=re.M), name


def test_the_new_units_are_in_the_makefile_lists():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    kernels = re.search(r"^KERNELS\s*=(.*)$", mk, flags=re.M).group(1).split()
    api = re.search(r"^API\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "kernels_croptensor" in kernels and "api_croptensor" in api
