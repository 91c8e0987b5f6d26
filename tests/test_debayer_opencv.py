"""Pins tests/debayer_ref.py to OpenCV itself wherever a cv2 is importable (skipped otherwise, like
tests/test_undistort_opencv.py): the model equals cv2.cvtColor with the four COLOR_Bayer*2BGR codes of the pattern table
(include/oatgpu.h).  The reference's frame server converts with the camera vendor's library, which cannot be restated; the
project's definition is chosen to equal the OpenCV the oracle follows (3.1.0).  The version met is recorded."""
import numpy as np
import pytest

import debayer_ref as D

cv2 = pytest.importorskip(
    "cv2", reason="no OpenCV here: the Bayer definition stays pinned to the model's restatement of Bayer2RGB_ alone; with a cv2 "
                  "a disagreement would mean that the model (and so the kernel, which equals it bit for bit) is not "
                  "cv::cvtColor(COLOR_Bayer*2BGR), or that the pattern table maps a tile to the wrong OpenCV code")


@pytest.mark.parametrize("pattern", D.PATTERNS)
def test_model_equals_cvtcolor(pattern, record_property):
    record_property("cv2_version", cv2.__version__)
    code = getattr(cv2, D.OPENCV_CODE[pattern])
    for rows, cols, p, raw in D.case_list():
        if p == pattern:
            assert np.array_equal(D.demosaic(raw, pattern), cv2.cvtColor(raw, code)), (rows, cols, cv2.__version__)
    m = np.array([[1, 0, 2], [0, 9, 1], [0, 0, 0]], np.uint8)
    assert np.array_equal(D.demosaic(m, pattern), cv2.cvtColor(m, code))
