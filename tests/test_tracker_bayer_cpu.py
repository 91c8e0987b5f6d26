"""CPU tests for the trackers' RAW8 front ends (oatgpu_set_tracker_bayer): the case list of tests/tracker_bayer_cases.py is not
vacuous and tells the planted wrong front ends apart, so that tests/test_diff_bayer_gpu.py and tests/test_bsub_bayer_gpu.py
cannot pass on empty masks or on a demosaic that is wrong where it matters; and the interface around the new entry -- header,
binding, library, `oat-posidet-hip --bayer` with its start-up refusals -- which needs no device."""
import os
import re
import subprocess

import pytest

import debayer_ref as R
import tracker_bayer_cases as T
from test_host_pipeline import host_bins  # noqa: F401  (the fixture builds the binaries)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------- the case list ----

def test_geometries_cover_the_lane_mappings():
    g = T.GEOMETRIES
    assert any(c % 4 for _, c in g) and any(c % 4 == 0 for _, c in g)          # narrow and wide
    assert any(c == 4 for _, c in g)                                            # one lane a row
    assert any(r == 3 for r, _ in g)                                            # every output row clamps to row 1
    assert any(r % 2 for r, _ in g if r > 3) and any(r % 2 == 0 for r, _ in g)  # the last row takes either parity
    assert any(r * c > 1024 and c % 4 == 0 and c > 256 for r, c in g)           # a row longer than a wave's 256 pixels


@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("rows,cols", T.BIG)
def test_motion_reference_is_not_vacuous(rows, cols, pattern):
    """(A stream's first frame is `grey != 0`: full by construction, the mosaic smooths diff_cases' planted zero away.  The plane
    is held to `not full` on every later frame.)"""
    rc, want = T.diff_want(rows, cols, (pattern,))
    later = want[1:]
    assert 2 * sum(w[0][0]["valid"] for w in later) >= len(later)
    assert want[0][0][1].all()
    assert any(w[0][1].any() for w in later) and not any(w[0][1].all() for w in later)


@pytest.mark.parametrize("alpha", [0.0, 0.05])
@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("rows,cols", T.BIG)
def test_subtraction_reference_is_not_vacuous(rows, cols, pattern, alpha):
    rc, want = T.bsub_want(rows, cols, (pattern,), alpha=alpha)
    later = want[1:]
    assert 2 * sum(w[0][0]["valid"] for w in later) >= len(later)
    assert any(w[0][1].any() for w in want) and not any(w[0][1].all() for w in want)


def test_multi_stream_references_are_not_vacuous():
    for rc, want in (T.diff_want(90, 200, T.THREE, roi=True), T.bsub_want(90, 200, T.THREE, roi=True)):
        for s in range(3):
            later = [w[s] for w in want[1:]]
            assert 2 * sum(w[0]["valid"] for w in later) >= len(later), s
            assert any(w[s][1].any() for w in want[1:]) and not any(w[s][1].all() for w in want[1:])


def test_small_geometries_still_move_the_motion_chain():
    """(5, 4) and (4, 8) are too small for the subtraction chain's window, not for the motion chain"""
    for rows, cols in ((5, 4), (4, 8)):
        for p in R.PATTERNS:
            _, want = T.diff_want(rows, cols, (p,))
            assert sum(w[0][0]["valid"] for w in want) >= 9, (rows, cols, p)


def test_swapped_pattern_assignment_differs():
    """two streams, two patterns: the same raw frames under the swapped assignment give other bits"""
    rc = T.diff_case(90, 200, T.THREE, roi=True)
    t = 3
    for s in (0, 1):
        assert (R.demosaic(rc.raw[t][s], T.THREE[s]) != R.demosaic(rc.raw[t][s], T.THREE_SWAPPED[s])).any()


# ----------------------------------------------------------------------------------- planted wrong front ends ----

FOUR = ["swap_rb", "row_parity", "col_parity", "border_own_site"]


@pytest.mark.parametrize("wrong", FOUR)
def test_every_motion_case_tells_a_wrong_demosaic_apart(wrong):
    """every geometry x pattern of the case list but the two 3-row frames (one or two triples a frame, no detection in either
    chain: the GPU files compare taps and state there)"""
    for rows, cols in T.GEOMETRIES:
        if rows == 3:
            continue
        for p in R.PATTERNS:
            assert T.tells_apart(T.diff_case(rows, cols, (p,)), T.diff_bits, wrong), (rows, cols, p)


@pytest.mark.parametrize("wrong", FOUR)
def test_big_subtraction_cases_tell_a_wrong_demosaic_apart(wrong):
    for rows, cols in T.BIG:
        for p in R.PATTERNS:
            for a in (0.0, 0.05):
                assert T.tells_apart(T.bsub_case(rows, cols, (p,), alpha=a), T.bsub_bits, wrong), (rows, cols, p, a)


@pytest.mark.parametrize("wrong", ["roi_on_raw", "pair_pattern0"])
def test_multi_stream_cases_tell_roi_and_pair_mistakes_apart(wrong):
    for rows, cols in ((90, 200), (37, 91)):
        assert T.tells_apart(T.diff_case(rows, cols, T.THREE, roi=True), T.diff_bits, wrong), (rows, cols)
    assert T.tells_apart(T.bsub_case(90, 200, T.THREE, roi=True), T.bsub_bits, wrong)
    assert T.tells_apart(T.bsub_case(37, 91, T.THREE, alpha=0.0, roi=True), T.bsub_bits, wrong)


def test_the_right_front_end_is_not_told_apart_from_itself():
    rc = T.diff_case(37, 91, T.THREE, roi=True)
    assert not T.tells_apart(rc, T.diff_bits, None)


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
    assert re.search(r"int\s+oatgpu_set_tracker_bayer\s*\(\s*oatgpu_ctx\s*\*\s*ctx\s*,\s*const\s+int32_t\s*\*\s*patterns\s*,\s*int32_t\s+n_patterns\s*\)\s*;",
                     code)
    assert ffi.SIGNATURES["oatgpu_set_tracker_bayer"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int32])
    assert hasattr(lib, "oatgpu_set_tracker_bayer")
    assert lib.oatgpu_abi_version() == ffi.ABI_VERSION == 9
    assert lib.oatgpu_set_tracker_bayer(None, None, 0) == -1           # OATGPU_E_INVALID without a context, no device needed


def test_python_trackers_have_the_switch():
    import inspect
    import oat_amd
    for cls in (oat_amd.MotionTracker, oat_amd.SubtractionTracker):
        assert "bayer" in inspect.signature(cls.__init__).parameters and callable(cls.bayer)


def test_posidet_help_names_bayer(host_bins):  # noqa: F811
    r = subprocess.run([os.path.join(host_bins, "oat-posidet-hip"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.count("--bayer") >= 2


@pytest.mark.parametrize("args,text", [
    (["diff", "a", "b", "--bayer", "GRBG", "--bgr"], "--bayer and --bgr"),
    (["thresh", "a", "b", "--bayer", "GRBG"], "--bayer goes with TYPE diff"),
    (["thresh", "a", "b", "--bsub", "--bayer", "GRBG"], "--bayer goes with TYPE diff"),
    (["hsv", "a", "b", "--bayer", "GRBG"], "--bayer with TYPE hsv needs --bsub"),
    (["diff", "a", "b", "--bayer", "RGBG"], "Invalid Bayer pattern"),
])
def test_posidet_bayer_start_up_refusals(host_bins, args, text):  # noqa: F811
    r = subprocess.run([os.path.join(host_bins, "oat-posidet-hip"), *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 255 and text in r.stderr, r.stderr
