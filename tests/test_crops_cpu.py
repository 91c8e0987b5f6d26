"""CPU tests of target crops: the model of tests/crops_ref.py and the cases of tests/crops_cases.py are checked on
their own -- the scalar and the numpy form of the contract agree, the cases reach what they are aimed at, nine planted wrong
croppers each differ somewhere -- then the header, the struct, the binding, the exports and oat-posidet-hip's start-up refusals.

Non-vacuity is a condition on the model alone.  A tracker's slot is what a stale crop would survive in: frame i of a sequence call
sits in slot i % 4, a synchronous step in slot 0 (crops_cases.slots_of); "an invalid rank following a valid one in the same slot"
is asked of the frame that sat in the slot before, under the plan the GPU test runs."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import crops_cases as CC
import crops_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("oatgpu_set_target_crops", "oatgpu_target_crops", "oatgpu_crop_windows_dev")
LISTS = [(rows, cols, h, w) for rows, cols in CC.GEOMETRIES for h, w in CC.CROP_SIZES]


# ------------------------------------------------------------------------------------------------ the two forms of the model ----

@pytest.mark.parametrize("rows,cols,h,w", LISTS)
def test_the_scalar_and_the_numpy_form_agree_on_every_explicit_window(rows, cols, h, w):
    step = 1 if h * w <= 1024 else 5              # (the pixel loop of the large windows: every fifth window, both kinds)
    for channels in (1, 3):
        frame = CC.pattern(rows, cols, channels, 1)
        for kind in CC.explicit_windows(rows, cols, h, w):
            for win in kind[(channels + h) % step::step]:
                assert np.array_equal(R.crop_scalar(frame, win, h, w), R.crop(frame, win, h, w)), (channels, win)


def test_the_two_forms_agree_on_tracker_windows():
    family, alpha, rows, cols, _, k, h, w = CC.TRACKER_RUNS[0]
    for axis in (False, True):
        for v in range(3):
            frames = CC.sequence(family, rows, cols, v)
            for t, wins in enumerate(CC.sequence_windows(family, rows, cols, v, alpha, k, axis)):
                for j, win in enumerate(wins):
                    assert np.array_equal(R.crop_scalar(frames[t], win, h, w), CC.sequence_crops(family, rows, cols, v, alpha, k, axis, h, w)[t][j])


def test_the_pattern_has_no_equal_neighbours():
    for rows, cols in CC.GEOMETRIES:
        for channels in (1, 3):
            f = CC.pattern(rows, cols, channels).astype(np.int64)
            for dy in range(0, 3):
                for dx in range(-2, 3):
                    if (dy, dx) > (0, 0):
                        a, b = f[dy:, max(dx, 0):cols + min(dx, 0)], f[:rows - dy, max(-dx, 0):cols + min(-dx, 0)]
                        assert (a != b).all(), (rows, cols, channels, dy, dx)
            if channels == 3:
                assert (f[..., 0] != f[..., 1]).all() and (f[..., 1] != f[..., 2]).all() and (f[..., 0] != f[..., 2]).all()
        assert (CC.pattern(rows, cols, 1, 0) != CC.pattern(rows, cols, 1, 1)).all()


# ------------------------------------------------------------------------------------------------------- the cases reach ----

@pytest.mark.parametrize("rows,cols,h,w", LISTS)
def test_every_explicit_list_is_clipped_at_every_edge_and_has_a_window_outside(rows, cols, h, w):
    upright, turned = CC.explicit_windows(rows, cols, h, w)
    for kind in (upright, turned):
        cov = [CC.coverage(win, rows, cols, h, w) for win in kind if R.is_valid(win)]
        for edge in ("left", "right", "top", "bottom"):
            assert any(c["inside"] and c[edge] for c in cov), edge
        assert any(not c["inside"] for c in cov)
        assert sum(not R.is_valid(win) for win in kind) >= 4
        # an invalid window stands between valid ones
        assert any(not R.is_valid(kind[i]) and R.is_valid(kind[i - 1]) and R.is_valid(kind[i + 1]) for i in range(1, len(kind) - 1))
    cov = [CC.coverage(win, rows, cols, h, w) for win in turned]
    assert any(c["frac"] for c in cov) and any(c["last_col"] for c in cov)
    assert all(win[1] for win in upright) and not any(win[1] for win in turned)
    # x.5 on both parities, and just below / above a half
    assert {int(round(win[2])) for win in upright if win[2] in (10.5, 11.5)} == {10, 12}
    assert any(win[2] == 10.49999 for win in upright) and any(win[2] == 20.50001 for win in upright)
    # axes at 0, 90 and +-45 degrees, a non-unit one, one that leaves every frame
    axes = {(win[4], win[5]) for win in turned}
    r = 0.5 ** 0.5
    assert {(1.0, 0.0), (0.0, 1.0), (r, r), (r, -r), (1.5, 0.25), (1e9, 0.0)} <= axes
    assert max(abs(win[2]) for win in upright if R.is_valid(win)) >= 300


def _runs():
    for family, alpha, rows, cols, n, k, h, w in CC.TRACKER_RUNS:
        yield family, alpha, rows, cols, min(n, 3), k, h, w


def test_every_tracker_sequence_has_what_a_stale_crop_and_both_rules_need():
    for family, alpha, rows, cols, n, k, h, w in _runs():
        for plan in (CC.PLAN, CC.PLAN_LONG):
            count = sum(c for _, c in plan)
            stale = axis0 = axis1 = False
            for s in range(n):
                v = CC.variant_of(s)
                tg = CC.sequence_targets(family, rows, cols, v, alpha, k)
                sh = CC.sequence_shapes(family, rows, cols, v, alpha, k)
                for t in range(2, count):
                    p = CC.predecessor(plan, t)
                    if p is not None:
                        stale |= any(tg[p][0][j]["valid"] and not tg[t][0][j]["valid"] for j in range(k))
                    axis0 |= any(r["valid"] and not r["axis_valid"] for r in sh[t])
                    axis1 |= any(r["valid"] and r["axis_valid"] for r in sh[t])
            assert stale and axis0 and axis1, (family, alpha, rows, cols, k, plan, stale, axis0, axis1)


def test_the_sequences_change_from_frame_to_frame_and_from_camera_to_camera():
    for family, alpha, rows, cols, n, k, h, w in _runs():
        for v in range(3):
            frames = CC.sequence(family, rows, cols, v)
            assert len(frames) == CC.N_FRAMES
            assert all((frames[t] != frames[t + 1]).any() for t in range(len(frames) - 1) if CC.MIX[t] != CC.MIX[t + 1])
            assert (frames[0] != CC.sequence(family, rows, cols, (v + 1) % 3)[0]).any()
    assert {k for *_, k, _, _ in CC.TRACKER_RUNS} == set(CC.KS) and {n for _, _, _, _, n, *_ in CC.TRACKER_RUNS} == set(CC.STREAMS)
    assert {(r, c) for _, _, r, c, *_ in CC.TRACKER_RUNS} == set(CC.GEOMETRIES)
    assert {(h, w) for *_, h, w in CC.TRACKER_RUNS} == set(CC.CROP_SIZES)


# ------------------------------------------------------------------------------------------------ planted wrong croppers ----

def _explicit_sequences(channels=3):
    """every explicit list as a two-frame, three-camera sequence of groups of 8 windows (so that set-level mistakes show too)"""
    for rows, cols, h, w in LISTS:
        if h * w > 1024:
            continue
        for kind in CC.explicit_windows(rows, cols, h, w):
            gs = CC.groups(kind)
            frames = [[CC.pattern(rows, cols, channels, 3 * t + s) for s in range(3)] for t in range(2)]
            windows = [[gs[(s + t) % len(gs)] for s in range(3)] for t in range(2)]
            yield frames, windows, h, w


@pytest.mark.parametrize("wrong", R.WRONG)
def test_a_planted_wrong_cropper_differs(wrong):
    hit = 0
    if wrong in ("half_up", "truncated_centre", "ay_negated", "replicated_border", "rgb_order", "fractions_swapped", "stream0_frame"):
        for frames, windows, h, w in _explicit_sequences():
            good = [R.crop_set(fs, ws, h, w) for fs, ws in zip(frames, windows)]
            bad = R.wrong_sequence(frames, windows, h, w, wrong)
            hit += any(not np.array_equal(a, b) for a, b in zip(good, bad))
        assert hit, wrong
        return
    # the set-level mistakes, on the trackers' sequences under the plan the GPU test runs
    for family, alpha, rows, cols, n, k, h, w in _runs():
        if h * w > 1024:
            continue
        for axis in (False, True):
            count = sum(c for _, c in CC.PLAN)
            frames = [[CC.sequence(family, rows, cols, CC.variant_of(s))[t] for s in range(n)] for t in range(count)]
            windows = [[CC.sequence_windows(family, rows, cols, CC.variant_of(s), alpha, k, axis)[t] for s in range(n)] for t in range(count)]
            good = [R.crop_set(fs, ws, h, w) for fs, ws in zip(frames, windows)]
            if wrong == "first_of_pair":
                bad = R.wrong_sequence(frames, windows, h, w, wrong, pairs=CC.paired_second(family, CC.PLAN))
                differs = any(not np.array_equal(a, b) for a, b in zip(good, bad))
            else:                                 # a stale crop: what sat in the slot before shows through an invalid rank
                differs = False
                for t in range(2, count):
                    p = CC.predecessor(CC.PLAN, t)
                    if p is None:
                        continue
                    for s in range(n):
                        for j, win in enumerate(windows[t][s]):
                            differs |= not R.is_valid(win) and good[p][s, j].any()
            assert differs, (wrong, family, alpha, rows, cols, k, axis)
            hit += 1
    assert hit, wrong


def test_the_wrong_croppers_are_the_model_where_nothing_is_replaced():
    rows, cols, h, w = 37, 61, 8, 8
    gs = CC.groups(CC.explicit_windows(rows, cols, h, w)[1])
    frames, windows = [[CC.pattern(rows, cols, 3, 0)]], [[gs[0]]]
    assert np.array_equal(R.wrong_sequence(frames, windows, h, w, None)[0], R.crop_set(frames[0], windows[0], h, w))
    assert len(R.WRONG) >= 8


# --------------------------------------------------------------------------------------------- header, library, binding ----

@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(ROOT, "oat_amd", "lib", "liboatgpu.so")):
        subprocess.check_call(["make", "-s", "-j4", "-C", ROOT, "oat_amd/lib/liboatgpu.so"])
    from oat_amd import ffi
    return ffi.load()


def test_crops_are_declared_exported_and_bound(lib, tmp_path):
    from oat_amd import ffi
    header = open(os.path.join(ROOT, "include", "oatgpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(lib, name) and name in ffi.SIGNATURES
    assert ffi.SIGNATURES["oatgpu_set_target_crops"][1] == [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    assert ffi.SIGNATURES["oatgpu_target_crops"][1] == [C.c_void_p, C.POINTER(C.c_uint8), C.c_int32]
    assert ffi.SIGNATURES["oatgpu_crop_windows_dev"][1] == [C.c_void_p, C.c_void_p, C.POINTER(ffi.CropWindow), C.c_int32, C.c_int32,
                                                            C.c_int32, C.POINTER(C.c_uint8)]
    fields = ("valid", "upright", "cx", "cy", "ax", "ay")
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "oatgpu.h"\nint main(){printf("%zu ' + "%zu " * len(fields) +
                   '%d %d %d %d %d %d\\n",sizeof(oatgpu_crop_window),' + ",".join("offsetof(oatgpu_crop_window,%s)" % f for f in fields) +
                   ',OATGPU_CROP_OFF,OATGPU_CROP_UPRIGHT,OATGPU_CROP_AXIS,OATGPU_CROP_MAX_SIDE,OATGPU_CROP_MAX_WINDOWS,'
                   'OATGPU_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "t"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    want = [40, 0, 4, 8, 16, 24, 32, 0, 1, 2, 256, 8, 9]
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want
    assert [C.sizeof(ffi.CropWindow)] + [getattr(ffi.CropWindow, f).offset for f in fields] == want[:7]
    assert [ffi.CROP_OFF, ffi.CROP_UPRIGHT, ffi.CROP_AXIS, ffi.CROP_MAX_SIDE, ffi.CROP_MAX_WINDOWS] == want[7:12]
    assert ffi.ABI_VERSION == 9 == lib.oatgpu_abi_version()                     # additive entries: the version stays


def test_the_header_states_the_semantics():
    header = open(os.path.join(ROOT, "include", "oatgpu.h")).read()
    text = " ".join(" ".join(re.sub(r"^\s*\*\s", "", line) for line in header.splitlines()).split())
    for words in ("X0 = (int)rint(cx) - w / 2", "X = (cx + u * ax) - v * ay", "Y = (cy + u * ay) + v * ax", "qx = (int)rint(X * 32.0)",
                  "sx = qx >> 5 (arithmetic shift)", "(sum S * p + 512) >> 10", "BORDER_CONSTANT 0", "Every byte of every window is written",
                  "exceeds 1e6, is invalid", "before the ROI mask", "oatgpu_track.rank indexes the frame's crop set", "Left out:",
                  "the axis still has no front"):
        assert words in text, words


def test_every_detector_class_has_crops():
    import oat_amd.components as comp
    for cls in ("HotPath", "MotionTracker", "SubtractionTracker", "HSVDetector", "SimpleThreshold", "DifferenceDetector"):
        k = getattr(comp, cls)
        assert all(callable(getattr(k, m, None)) for m in ("set_target_crops", "target_crops", "crop_windows")), cls


# ---------------------------------------------------------------------------------------------- the binary's start-up refusals ----

BIN = os.path.join(ROOT, "build", "bin")


@pytest.fixture(scope="module")
def host_bins():
    if not os.path.exists(os.path.join(BIN, "oat-posidet-hip")):
        subprocess.check_call(["make", "-s", "-j4", "-C", ROOT, "host"])
    return BIN


CROPS = ["--crop-sinks", "c0", "--crop-size", "8x8"]
REFUSALS = [
    (["diff", "src", "snk"] + CROPS, "--crop-sinks needs --target-sinks or --track-sinks"),
    (["hsv", "src", "snk", "--bsub"] + CROPS, "--crop-sinks needs --target-sinks or --track-sinks"),
    (["diff", "src", "snk", "--target-sinks", "a", "--crop-sinks", "c0,c1", "--crop-size", "8x8"], "--crop-sinks names 2 sinks for 1 ranked blobs"),
    (["diff", "src", "snk", "--target-sinks", "a,b"] + CROPS + ["--crop-axis"], "--crop-axis needs --target-shape"),
    (["diff", "src", "snk", "--target-sinks", "a,b", "--crop-sinks", "c0", "--crop-size", "8x6"], "a window is 1..256 rows by 4..256 columns"),
    (["diff", "src", "snk", "--target-sinks", "a,b", "--crop-sinks", "c0", "--crop-size", "0x8"], "a window is 1..256 rows by 4..256 columns"),
    (["diff", "src", "snk", "--target-sinks", "a,b", "--crop-sinks", "c0", "--crop-size", "8x260"], "a window is 1..256 rows by 4..256 columns"),
    (["diff", "src", "snk", "--target-sinks", "a,b", "--crop-sinks", "c0", "--crop-size", "8"], "--crop-size: expected HxW"),
    (["diff", "src", "snk", "--target-sinks", "a,b", "--crop-sinks", "c0"], "--crop-sinks needs --crop-size"),
    (["diff", "src", "snk", "--target-sinks", "a,b", "--bayer", "RGGB"] + CROPS, "--crop-sinks does not go with --bayer or --camera-matrix"),
    (["diff", "src", "snk", "--target-sinks", "a,b", "--camera-matrix", "[1,0,0,0,1,0,0,0,1]", "--distortion-coeffs", "[0,0,0,0,0]"] + CROPS,
     "--crop-sinks does not go with --bayer or --camera-matrix"),
    (["thresh", "src", "snk", "--target-sinks", "a,b"] + CROPS, "--crop-sinks with TYPE thresh needs --bsub"),
    (["diff", "src", "snk", "--target-sinks", "a,b", "--crop-sinks", "a", "--crop-size", "8x8"], "sink 'a' is named twice"),
    (["diff", "src", "snk", "--crop-size", "8x8"], "--crop-size and --crop-axis are parameters of --crop-sinks"),
]


@pytest.mark.parametrize("args,text", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_the_binary_refuses_at_start_up(host_bins, args, text):
    r = subprocess.run([os.path.join(host_bins, "oat-posidet-hip")] + args, capture_output=True, text=True, timeout=20)
    assert r.returncode != 0 and text in r.stderr, (r.returncode, r.stderr)


def test_the_crop_keys_in_a_config_file_are_checked_the_same_way(host_bins, tmp_path):
    cfg = tmp_path / "c.toml"
    run = lambda: subprocess.run([os.path.join(host_bins, "oat-posidet-hip"), "diff", "src", "snk", "-c", str(cfg), "det"],      # noqa: E731
                                 capture_output=True, text=True, timeout=20)
    cfg.write_text('[det]\ncrop-sinks = "c0"\ncrop-size = "8x8"\n')
    r = run()
    assert r.returncode != 0 and "--crop-sinks needs --target-sinks or --track-sinks" in r.stderr, r.stderr
    cfg.write_text('[det]\ntarget-sinks = "a,b"\ncrop-sinks = "c0"\ncrop-size = "8x8"\ncrop-axis = true\n')
    r = run()
    assert r.returncode != 0 and "--crop-axis needs --target-shape" in r.stderr, r.stderr
    cfg.write_text('[det]\ntarget-sinks = "a,b"\ncrop-sinks = "c0"\ncrop-size = "8x10"\n')
    r = run()
    assert r.returncode != 0 and "a window is 1..256 rows by 4..256 columns" in r.stderr, r.stderr
    cfg.write_text('[det]\ntarget-sinks = "a,b"\ncrop-sinks = "c0"\ncrop-size = "8x8"\ncrop-axis = 3\n')
    r = run()
    assert r.returncode != 0 and "must be a TOML value of type bool" in r.stderr, r.stderr
