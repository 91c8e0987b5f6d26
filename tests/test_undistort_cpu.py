"""CPU tests of `framefilt undistort` (src/framefilter/Undistorter.cpp): the library's context-free map builder
(oatgpu_undistort_map) against the numpy restatement of OpenCV 3.1's cv::undistort (tests/undistort_ref.py) bit for bit,
known answers, an independent float check of the restatement, and the drop-in binary's refusals (no device touched)."""
import os
import subprocess

import numpy as np
import pytest

import undistort_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(ROOT, "oat_amd", "lib", "liboatgpu.so")):
        subprocess.check_call(["make", "-s", "-j4", "-C", ROOT, "oat_amd/lib/liboatgpu.so"])
    from oat_amd import ffi
    return ffi.load()


# widths on both sides of cv::undistort's 4096-column stripe rule; odd heights leave a short last stripe
SHAPES = [(23, 37), (61, 640), (520, 816), (45, 1920), (19, 3840), (7, 4100)]


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_map_equals_the_restatement_bit_for_bit(lib, rows, cols):
    from oat_amd import undistort_map
    assert R.stripe_rows(rows, cols) == min(max(1, 4096 // cols), rows)
    for name, (K, D) in R.cases(rows, cols).items():
        m1, m2 = undistort_map(rows, cols, K, D)
        w1, w2 = R.undistort_map(rows, cols, K, D)
        assert m1.shape == (rows, cols, 2) and m2.shape == (rows, cols)
        assert np.array_equal(m1, w1), (name, int((m1 != w1).sum()))
        assert np.array_equal(m2, w2), (name, int((m2 != w2).sum()))


def test_the_cases_reach_the_border_rules(lib):
    """The strong distortions put many pixels off-frame, some exactly at sx = -1 / sy = -1 (one corner column inside)."""
    rows, cols = 520, 816
    c = R.cases(rows, cols)
    seen_minus1 = seen_off = 0
    for name in ("barrel", "pincushion", "reference"):
        m1, _ = R.undistort_map(rows, cols, *c[name])
        sx, sy = m1[..., 0].astype(int), m1[..., 1].astype(int)
        seen_minus1 += int(((sx == -1) | (sy == -1)).sum())
        seen_off += int(((sx < -1) | (sx >= cols) | (sy < -1) | (sy >= rows)).sum())
    assert seen_minus1 > 0 and seen_off > 1000


def test_the_running_sum_is_not_the_direct_form():
    """_x0 + j * ir[0] instead of the column loop's running sum gives other u, v in the last bits (why the restatement
    accumulates); a 1/32-px cell flips only where u * 32 lies within those bits of a half, which these cases do not hit."""
    rows, cols = 520, 816
    moved = 0
    for K, D in R.cases(rows, cols).values():
        u, v = R._coords(rows, cols, K, D)
        ud, vd = R._coords(rows, cols, K, D, sequential=False)
        with np.errstate(all="ignore"):
            moved += int((u != ud).sum() + (v != vd).sum())
    assert moved > 0


def test_zero_coefficients_give_the_identity(lib):
    from oat_amd import undistort_map
    for rows, cols in ((37, 53), (64, 4100)):
        K = R.scaled_k(rows, cols)
        m1, m2 = undistort_map(rows, cols, K, [0.0] * 5)
        yy, xx = np.mgrid[0:rows, 0:cols]
        assert (m2 == 0).all()
        assert (m1[..., 0] == xx).all() and (m1[..., 1] == yy).all()
        img = np.random.default_rng(1).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
        assert np.array_equal(R.remap(img, m1, m2), img)


def test_k1_only_keeps_the_principal_point(lib):
    from oat_amd import undistort_map
    rows, cols = 101, 161
    K = [120.0, 0.0, 80.0, 0.0, 118.0, 50.0, 0.0, 0.0, 1.0]       # principal point on a pixel
    for k1 in (-0.4, 0.3):
        m1, m2 = undistort_map(rows, cols, K, [k1, 0.0, 0.0, 0.0, 0.0])
        assert tuple(m1[50, 80]) == (80, 50) and m2[50, 80] == 0
        assert not (m1[..., 0] == np.arange(cols)).all()                # ... and moves the rest


def test_fixed_point_identity_over_every_fraction():
    """(sum S * w + 16384) >> 15 with BilinearTab_i's weights == (sum S * w/32 + 512) >> 10 (the kernel's form), for all
    1024 fractions and extreme samples; the weights are exact and sum to 32768."""
    tab = R.bilinear_tab()
    assert (tab.sum(axis=1) == 32768).all() and (tab % 32 == 0).all()
    rng = np.random.default_rng(7)
    S = np.concatenate([np.array([[0, 0, 0, 0], [255, 255, 255, 255], [255, 0, 0, 255], [0, 255, 255, 0], [255, 0, 0, 0],
                                  [0, 0, 0, 255], [1, 254, 254, 1]]), rng.integers(0, 256, (500, 4))])
    A = S @ (tab // 32).T                                  # [samples, fractions]
    assert np.array_equal((32 * A + 16384) >> 15, (A + 512) >> 10)
    assert ((A + 512) >> 10).max() <= 255


def _smooth(rows, cols, ch):
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    edge = np.minimum(np.minimum(xx, cols - 1 - xx), np.minimum(yy, rows - 1 - yy))
    base = (120 + 30 * np.sin(xx / 23.0) * np.cos(yy / 31.0)) * np.clip(edge / 40.0, 0, 1)
    planes = [base + 10 * c * np.cos((xx + yy) / 50.0) for c in range(ch)]
    return np.clip(np.rint(np.stack(planes, axis=-1)), 0, 255).astype(np.uint8).reshape((rows, cols) + ((ch,) if ch > 1 else ()))


@pytest.mark.parametrize("ch", [1, 3])
def test_restatement_agrees_with_a_float_bilinear(ch):
    """Independent check: u, v from the formulas with a direct j * ir[0], unquantised, float weights -- within one grey
    level of the fixed-point restatement on at least 99.9 % of the pixels (smooth content, dark frame edge)."""
    rows, cols = 520, 816
    img = _smooth(rows, cols, ch)
    for name, (K, D) in R.cases(rows, cols).items():
        fixed = R.undistort(img, K, D).astype(np.float64)
        flt = R.undistort_float(img, K, D)
        close = np.abs(fixed - flt) <= 1.0
        assert close.mean() >= 0.999, (name, close.mean())


def _run(args, timeout=30):
    return subprocess.run([os.path.join(BIN, "oat-framefilt-hip"), "undistort", "oat_t_src", "oat_t_snk"] + args,
                          capture_output=True, text=True, timeout=timeout)


@pytest.fixture(scope="module")
def framefilt():
    subprocess.check_call(["make", "-s", "-j4", "-C", ROOT, "host"])
    return os.path.join(BIN, "oat-framefilt-hip")


K9 = "[7473.00,0,408.433,0,8828.00,260.437,0,0,1]"


@pytest.mark.parametrize("args,text", [
    (["-k", K9], "Required configuration value 'distortion-coeffs' was not specified."),
    (["-d", "[-53.7,20443.3,0.43,-0.17,51.4]"], "Required configuration value 'camera-matrix' was not specified."),
    (["-k", K9, "-d", "[1,2,3,4]"], "Distortion coefficients consist of 5 to 8 values."),
    (["-k", K9, "-d", "[1,2,3,4,5,6,7,8,9]"], "Distortion coefficients consist of 5 to 8 values."),
    (["-k", K9, "-d", "[0.1,0,0,0,0,0]"], "6 or 7 values"),
    (["-k", K9, "-d", "[0.1,0,0,0,0,0,0]"], "6 or 7 values"),
    (["-k", "[7473,0,408,0,8828,260,0,0]", "-d", "[0.1,0,0,0,0]"], "'camera-matrix' must be a TOML vector containing 9 elements."),
])
def test_binary_refuses_bad_calibrations_before_touching_a_device(framefilt, args, text):
    r = _run(args)
    assert r.returncode != 0 and text in r.stderr, r.stderr


def test_library_refuses_six_or_seven_coefficients(lib):
    from oat_amd import OatGpuError, undistort_map
    K = R.scaled_k(8, 8)
    for n in (4, 6, 7, 9):
        with pytest.raises(OatGpuError) as e:
            undistort_map(8, 8, K, [0.01] * n)
        assert e.value.code == -1
    with pytest.raises(ValueError):
        undistort_map(8, 8, K[:8], [0.0] * 5)


def test_usage_names_undistort(framefilt):
    r = subprocess.run([framefilt, "--help"], capture_output=True, text=True, timeout=30)
    assert "undistort" in r.stdout and "--camera-matrix" in r.stdout and "--distortion-coeffs" in r.stdout
