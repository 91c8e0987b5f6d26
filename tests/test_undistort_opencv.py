"""Pins tests/undistort_ref.py to OpenCV itself wherever a cv2 is importable (skipped otherwise, like
tests/test_opencv_crosscheck.py): the library's map against cv2.initUndistortRectifyMap stripe by stripe, and the
restatement's frames against cv2.undistort.  The reference builds against OpenCV 3.1.0; the version met is recorded."""
import numpy as np
import pytest

import undistort_ref as R

cv2 = pytest.importorskip("cv2")


@pytest.mark.parametrize("rows,cols", [(61, 640), (520, 816), (9, 4100)])
def test_map_and_frames_equal_opencv(rows, cols, record_property):
    from oat_amd import undistort_map
    record_property("cv2_version", cv2.__version__)
    img = np.random.default_rng(rows).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    s0 = R.stripe_rows(rows, cols)
    for name, (K, D) in R.cases(rows, cols).items():
        Km, Dm = np.array(K, np.float64).reshape(3, 3), np.array(D, np.float64)
        m1, m2 = undistort_map(rows, cols, K, D)
        for y in range(0, rows, s0):
            n = min(s0, rows - y)
            Ar = Km.copy()
            Ar[1, 2] = Km[1, 2] - y
            c1, c2 = cv2.initUndistortRectifyMap(Km, Dm, np.eye(3), Ar, (cols, n), cv2.CV_16SC2)
            assert np.array_equal(m1[y:y + n], c1), (name, cv2.__version__, y)
            assert np.array_equal(m2[y:y + n], c2), (name, cv2.__version__, y)
        assert np.array_equal(R.undistort(img, K, D), cv2.undistort(img, Km, Dm)), (name, cv2.__version__)
