"""GPU tests of the Bayer RAW8 -> BGR stage (oatgpu_debayer_filter, oatgpu_debayer_dev; oat_amd.Debayer) against the numpy
model of tests/debayer_ref.py, bit for bit: every pattern at the shapes where the two lane mappings can go wrong, a misaligned
device pointer, several streams with several patterns, more streams than one launch takes, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import debayer_ref as D

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("rows,cols", D.SHAPES)
def test_filter_and_dev_equal_the_model(rows, cols):
    """3 x 3, 4 x 4, 6 x 8 (wide), 5 x 12 (wide, odd rows), 7 x 10 (narrow), and the two shapes that cross wave and workgroup
    boundaries of the mappings in x and y (debayer_ref.CROSSING_WIDE = 12 x 1040, CROSSING_NARROW = 9 x 1041)."""
    import torch
    import oat_amd
    db = oat_amd.Debayer(rows, cols)
    try:
        for r, c, p, raw in D.case_list():
            if (r, c) != (rows, cols):
                continue
            want = D.demosaic(raw, p)
            assert np.array_equal(db.filter(raw, p), want), D.NAMES[p]
            assert np.array_equal(db.filter(raw, D.NAMES[p]), want), D.NAMES[p]
            src, dst = _dev(raw), torch.zeros((rows, cols, 3), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            db.filter_dev(src.data_ptr(), dst.data_ptr(), p)
            db.synchronize()
            assert np.array_equal(dst.cpu().numpy(), want), D.NAMES[p]
    finally:
        db.close()


@pytest.mark.parametrize("pattern", D.PATTERNS)
def test_a_device_pointer_off_by_one_byte_takes_the_narrow_form(pattern):
    """6 x 8 is a wide shape; from raw + 1 and into bgr + 1 the dword accesses of the wide form would be misaligned"""
    import torch
    import oat_amd
    rows, cols = 6, 8
    raw = D.random_mosaic(rows, cols, 40 + pattern)
    want = D.demosaic(raw, pattern)
    db = oat_amd.Debayer(rows, cols)
    try:
        for off_in, off_out in ((1, 0), (0, 1), (1, 1), (2, 3)):
            src = torch.zeros(rows * cols + 8, dtype=torch.uint8, device="cuda")
            dst = torch.full((rows * cols * 3 + 8,), 0xA5, dtype=torch.uint8, device="cuda")
            src[off_in:off_in + rows * cols] = _dev(raw.reshape(-1))
            torch.cuda.synchronize()
            db.filter_dev(src.data_ptr() + off_in, dst.data_ptr() + off_out, pattern)
            db.synchronize()
            got = dst.cpu().numpy()
            assert np.array_equal(got[off_out:off_out + rows * cols * 3].reshape(rows, cols, 3), want), (off_in, off_out)
            assert (got[:off_out] == 0xA5).all() and (got[off_out + rows * cols * 3:] == 0xA5).all(), (off_in, off_out)
    finally:
        db.close()


@pytest.mark.parametrize("rows,cols", [(6, 8), (7, 10)])
def test_three_streams_three_patterns_in_one_launch(rows, cols):
    import torch
    import oat_amd
    pats = [D.GBRG, D.RGGB, D.GRBG]
    raws = [D.random_mosaic(rows, cols, 60 + s) for s in range(3)]
    db = oat_amd.Debayer(rows, cols, n_streams=3)
    try:
        src, dst = _dev(np.stack(raws)), torch.zeros((3, rows, cols, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        db.filter_dev(src.data_ptr(), dst.data_ptr(), [D.NAMES[p] for p in pats])
        db.synchronize()
        got = dst.cpu().numpy()
        for s in range(3):
            assert np.array_equal(got[s], D.demosaic(raws[s], pats[s])), s
        db.filter_dev(src.data_ptr(), dst.data_ptr(), D.BGGR)           # one pattern for all
        db.synchronize()
        got = dst.cpu().numpy()
        for s in range(3):
            assert np.array_equal(got[s], D.demosaic(raws[s], D.BGGR)), s
    finally:
        db.close()


def test_66_streams_need_two_launches():
    import torch
    import oat_amd
    rows, cols, n = 8, 8, 66
    pats = [D.PATTERNS[(s * 7 + s // 5) % 4] for s in range(n)]
    raws = [D.random_mosaic(rows, cols, 200 + s) for s in range(n)]
    db = oat_amd.Debayer(rows, cols, n_streams=n, ring_depth=1)
    try:
        src, dst = _dev(np.stack(raws)), torch.zeros((n, rows, cols, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        db.filter_dev(src.data_ptr(), dst.data_ptr(), pats)
        db.synchronize()
        got = dst.cpu().numpy()
        for s in range(n):
            assert np.array_equal(got[s], D.demosaic(raws[s], pats[s])), s
    finally:
        db.close()


def test_refusals():
    import torch
    import oat_amd
    from oat_amd import ffi
    for rows, cols in ((2, 8), (8, 2)):
        small = oat_amd.Debayer(rows, cols)
        try:
            with pytest.raises(oat_amd.OatGpuError) as e:
                small.filter(np.zeros((rows, cols), np.uint8), D.RGGB)
            assert e.value.code == -1 and "3 x 3" in str(e.value)
        finally:
            small.close()
    db = oat_amd.Debayer(6, 8, n_streams=3)
    try:
        raw = np.zeros((6, 8), np.uint8)
        for bad in (0, 5, -1):
            with pytest.raises(oat_amd.OatGpuError) as e:
                db.filter(raw, bad)
            assert e.value.code == -1 and "pattern" in str(e.value)
        with pytest.raises(ValueError):
            db.filter(raw, "RGBG")
        src = torch.zeros(3 * 48, dtype=torch.uint8, device="cuda")
        dst = torch.zeros(3 * 48 * 3, dtype=torch.uint8, device="cuda")
        for pats in ([1, 2], [1, 2, 3, 4], [1, 9, 2]):
            with pytest.raises(oat_amd.OatGpuError) as e:
                db.filter_dev(src.data_ptr(), dst.data_ptr(), pats)
            assert e.value.code == -1
        lib = db.lib
        one = (C.c_int32 * 1)(1)
        assert lib.oatgpu_debayer_dev(db.ctx, one, 1, None, C.c_void_p(dst.data_ptr())) == -1
        assert lib.oatgpu_debayer_dev(db.ctx, None, 1, C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr())) == -1
        assert lib.oatgpu_debayer_dev(db.ctx, one, 1, C.c_void_p(src.data_ptr()), C.c_void_p(src.data_ptr())) == -1
        assert lib.oatgpu_debayer_dev(db.ctx, one, 0, C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr())) == -1
        assert lib.oatgpu_debayer_filter(db.ctx, 1, None, ffi.u8(np.zeros((6, 8, 3), np.uint8))) == -1
        torch.cuda.synchronize()
        assert (dst.cpu().numpy() == 0).all()                # nothing was launched by a refused call
    finally:
        db.close()
