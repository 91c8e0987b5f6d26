"""CPU tests for the trackers' undistorting front ends (oatgpu_set_tracker_undistort): the case list of
tests/tracker_undistort_cases.py is not vacuous and tells the planted wrong front ends apart, so that
tests/test_diff_undistort_gpu.py and tests/test_bsub_undistort_gpu.py cannot pass on empty masks or on a remap that is wrong
where it matters; and the interface around the new entry -- header, binding, library, `oat-posidet-hip --camera-matrix
--distortion-coeffs` with its start-up refusals -- which needs no device."""
import os
import re
import subprocess

import numpy as np
import pytest

import diff_cases as D
import tracker_undistort_cases as T
import undistort_ref as R
from test_host_pipeline import host_bins  # noqa: F401  (the fixture builds the binaries)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K9 = "[160,0,99.63,0,161.6,45.29,0,0,1]"
D5 = "[-0.21,0.07,0.0013,-0.0009,-0.011]"


# ------------------------------------------------------------------------------------------- the case list ----

def test_geometries_cover_the_lane_mappings():
    g = T.GEOMETRIES
    assert set(D.GEOMETRIES) <= set(g) and {(3, 3), (3, 4), (4, 8), (12, 1040)} <= set(g)
    assert any(c % 4 for _, c in g) and any(c % 4 == 0 for _, c in g)          # narrow and wide
    assert any(c == 4 for _, c in g)                                            # one lane a row
    assert any(r * c > 1024 and c % 4 == 0 and c > 256 for r, c in g)           # a row longer than a wave's 256 pixels


@pytest.mark.parametrize("rows,cols", T.GEOMETRIES)
def test_pincushion_takes_every_branch_of_the_remap(rows, cols):
    inside, partly, outside = T.branch_counts(rows, cols, "pincushion")
    assert inside > 0 and partly > 0 and outside > 0


@pytest.mark.parametrize("rows,cols", T.BIG + [(12, 1040)])
def test_mild5_is_inside_almost_everywhere(rows, cols):
    inside, partly, outside = T.branch_counts(rows, cols, "mild5")
    assert inside >= 0.9 * rows * cols and outside == 0


def test_the_variant_remap_is_the_references_by_default():
    uc = T.diff_case(37, 91, 3, ("pincushion",))
    assert np.array_equal(T.remap_variant(uc.given[3][0], *uc.maps[0]), R.remap(uc.given[3][0], *uc.maps[0]))


def _differing(want, plain):
    return sum(not D.same_dict(a[0][0], b[0][0]) for a, b in zip(want, plain))


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("rows,cols,cal", T.DETECTING)
def test_motion_reference_is_not_vacuous(rows, cols, cal, channels):
    """detections on >= 10 of 12 frames, other than the same chain's without undistortion on >= 9"""
    _, want = T.diff_want(rows, cols, channels, (cal,))
    _, plain = T.diff_want(rows, cols, channels, (cal,), plain=True)
    assert len(want) == 12 and sum(w[0][0]["valid"] for w in want) >= 10
    assert _differing(want, plain) >= 9
    assert any(w[0][1].any() for w in want[1:]) and not any(w[0][1].all() for w in want[1:])


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("alpha", [0.0, 0.05])
@pytest.mark.parametrize("rows,cols,cal", T.DETECTING)
def test_subtraction_reference_is_not_vacuous(rows, cols, cal, alpha, channels):
    """detections on >= 7 of 8 frames, other than the same chain's without undistortion on >= 3"""
    _, want = T.bsub_want(rows, cols, channels, (cal,), alpha=alpha)
    _, plain = T.bsub_want(rows, cols, channels, (cal,), alpha=alpha, plain=True)
    assert len(want) == 8 and sum(w[0][0]["valid"] for w in want) >= 7
    assert _differing(want, plain) >= 3
    assert any(w[0][1].any() for w in want) and not any(w[0][1].all() for w in want)


@pytest.mark.parametrize("channels", [3, 1])
def test_multi_stream_references_are_not_vacuous(channels):
    for _, want in (T.diff_want(90, 200, channels, T.THREE, roi=True), T.bsub_want(90, 200, channels, T.THREE, roi=True)):
        for s in range(3):
            later = [w[s] for w in want[1:]]
            assert 2 * sum(w[0]["valid"] for w in later) >= len(later), s
            assert any(w[1].any() for w in later) and not any(w[1].all() for w in later)


def test_swapped_calibration_assignment_differs():
    uc = T.diff_case(90, 200, 3, T.THREE, roi=True)
    t = 3
    for s in (0, 1):
        assert (R.remap(uc.given[t][s], *T.maps(90, 200, T.THREE_SWAPPED[s])) != uc.und[t][s]).any()
    assert T.THREE[2] == T.THREE_SWAPPED[2]


# ----------------------------------------------------------------------------------- planted wrong front ends ----

def test_the_list_of_wrong_front_ends():
    assert T.WRONG == ["before_remap", "roi_on_distorted", "map0", "pair_unremapped", "border_replicate", "no_round", "swap_fxfy"]


def test_grey_before_the_remap_is_told_apart_on_bgr_frames():
    """(GREY frames: the grey of a grey frame is the frame, the two orders are one.  The subtraction chain at alpha 0 keeps a
    static background, which commutes with the remap wherever the frame does not exceed it by much: held at alpha 0.05.)"""
    for rows, cols, cal in T.DETECTING:
        assert T.tells_apart(T.diff_case(rows, cols, 3, (cal,)), T.diff_bits, "before_remap"), (rows, cols, cal)
    for rows, cols in T.BIG:
        for cal in T.CALS:
            assert T.tells_apart(T.bsub_case(rows, cols, 3, (cal,), alpha=0.05), T.bsub_bits, "before_remap"), (rows, cols, cal)


@pytest.mark.parametrize("channels", [3, 1])
def test_border_replicate_is_told_apart_wherever_pixels_fall_off_the_frame(channels):
    """pincushion: every geometry has pixels partly and fully outside"""
    for rows, cols in T.GEOMETRIES:
        assert T.tells_apart(T.diff_case(rows, cols, channels, ("pincushion",)), T.diff_bits, "border_replicate"), (rows, cols)
        for a in (0.0, 0.05):
            assert T.tells_apart(T.bsub_case(rows, cols, channels, ("pincushion",), alpha=a), T.bsub_bits, "border_replicate"), (rows, cols, a)


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("wrong", ["no_round", "swap_fxfy"])
def test_the_fixed_point_arithmetic_is_told_apart(wrong, channels):
    for rows, cols, cal in T.DETECTING:
        assert T.tells_apart(T.diff_case(rows, cols, channels, (cal,)), T.diff_bits, wrong), (rows, cols, cal)
        for a in (0.0, 0.05):
            assert T.tells_apart(T.bsub_case(rows, cols, channels, (cal,), alpha=a), T.bsub_bits, wrong), (rows, cols, cal, a)


@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("wrong", ["roi_on_distorted", "map0", "pair_unremapped"])
def test_multi_stream_cases_tell_roi_map_and_pair_mistakes_apart(wrong, channels):
    for cals in (T.THREE, T.THREE_SWAPPED):
        for rows, cols in ((90, 200), (37, 91)):
            assert T.tells_apart(T.diff_case(rows, cols, channels, cals, roi=True), T.diff_bits, wrong), (rows, cols)
            assert T.tells_apart(T.bsub_case(rows, cols, channels, cals, roi=True), T.bsub_bits, wrong), (rows, cols)
            assert T.tells_apart(T.bsub_case(rows, cols, channels, cals, alpha=0.0, roi=True), T.bsub_bits, wrong), (rows, cols)


def test_the_right_front_end_is_not_told_apart_from_itself():
    uc = T.diff_case(37, 91, 3, T.THREE, roi=True)
    assert not T.tells_apart(uc, T.diff_bits, None)
    assert not T.tells_apart(T.bsub_case(37, 91, 3, T.THREE, roi=True), T.bsub_bits, None)


# ------------------------------------------------------------------------------------------------ interface ----

@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(ROOT, "oat_amd", "lib", "liboatgpu.so")):
        subprocess.check_call(["make", "-s", "-j4", "-C", ROOT, "oat_amd/lib/liboatgpu.so"])
    from oat_amd import ffi
    return ffi.load()


def test_header_binding_and_library_agree_on_the_new_entry(lib):
    import ctypes as C
    from oat_amd import ffi
    src = open(os.path.join(ROOT, "include", "oatgpu.h")).read()
    assert re.search(r"#define OATGPU_ABI_VERSION 9\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"int\s+oatgpu_set_tracker_undistort\s*\(\s*oatgpu_ctx\s*\*\s*ctx\s*,\s*int32_t\s+on\s*\)\s*;", code)
    assert ffi.SIGNATURES["oatgpu_set_tracker_undistort"] == (C.c_int, [C.c_void_p, C.c_int32])
    assert hasattr(lib, "oatgpu_set_tracker_undistort")
    assert lib.oatgpu_abi_version() == ffi.ABI_VERSION == 9
    assert lib.oatgpu_set_tracker_undistort(None, 1) == -1             # OATGPU_E_INVALID without a context, no device needed


def test_python_trackers_have_the_switch():
    import inspect
    import oat_amd
    for cls in (oat_amd.MotionTracker, oat_amd.SubtractionTracker):
        assert "undistort" in inspect.signature(cls.__init__).parameters
        assert callable(cls.undistort) and callable(cls.set_undistort)


def test_posidet_help_names_the_calibration(host_bins):  # noqa: F811
    r = subprocess.run([os.path.join(host_bins, "oat-posidet-hip"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--camera-matrix" in r.stdout and "--distortion-coeffs" in r.stdout


@pytest.mark.parametrize("args,text", [
    (["diff", "a", "b", "--camera-matrix", K9], "Required configuration value 'distortion-coeffs' was not specified."),
    (["diff", "a", "b", "--bgr", "--distortion-coeffs", D5], "Required configuration value 'camera-matrix' was not specified."),
    (["hsv", "a", "b", "--bsub", "--camera-matrix", K9], "Required configuration value 'distortion-coeffs' was not specified."),
    (["thresh", "a", "b", "--bsub", "--distortion-coeffs", D5], "Required configuration value 'camera-matrix' was not specified."),
    (["diff", "a", "b", "--bayer", "GRBG", "--camera-matrix", K9, "--distortion-coeffs", D5], "and --bayer exclude each other"),
    (["diff", "a", "b", "--bayer", "GRBG", "--distortion-coeffs", D5], "and --bayer exclude each other"),
    (["hsv", "a", "b", "--bsub", "--bayer", "RGGB", "--camera-matrix", K9], "and --bayer exclude each other"),
    (["diff", "a", "b", "--camera-matrix", K9, "--distortion-coeffs", "[0.1,0,0,0,0,0]"], "6 or 7 values"),
    (["hsv", "a", "b", "--bsub", "--camera-matrix", K9, "--distortion-coeffs", "[0.1,0,0,0,0,0,0]"], "6 or 7 values"),
    (["diff", "a", "b", "--camera-matrix", K9, "--distortion-coeffs", "[1,2,3,4]"], "Distortion coefficients consist of 5 to 8 values."),
    (["diff", "a", "b", "--camera-matrix", "[1,2,3]", "--distortion-coeffs", "[1,2,3,4]"], "Distortion coefficients consist of 5 to 8 values."),
    (["hsv", "a", "b", "--camera-matrix", K9, "--distortion-coeffs", D5], "need --bsub"),
    (["thresh", "a", "b", "--camera-matrix", K9, "--distortion-coeffs", D5], "need --bsub"),
])
def test_posidet_calibration_start_up_refusals(host_bins, args, text):  # noqa: F811
    r = subprocess.run([os.path.join(host_bins, "oat-posidet-hip"), *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 255 and text in r.stderr, r.stderr


def test_posidet_reads_the_calibration_from_the_configuration_table(host_bins, tmp_path):  # noqa: F811
    cfg = tmp_path / "c.toml"
    cfg.write_text("[det]\ncamera-matrix = " + K9 + "\ndistortion-coeffs = [0.1,0,0,0,0,0]\n")
    r = subprocess.run([os.path.join(host_bins, "oat-posidet-hip"), "diff", "a", "b", "-c", str(cfg), "det"], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 255 and "6 or 7 values" in r.stderr, r.stderr
    cfg.write_text("[det]\ncamera-matrix = " + K9 + "\n")
    r = subprocess.run([os.path.join(host_bins, "oat-posidet-hip"), "hsv", "a", "b", "--bsub", "-c", str(cfg), "det"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 255 and "'distortion-coeffs' was not specified" in r.stderr, r.stderr
