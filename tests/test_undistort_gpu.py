"""GPU tests of `framefilt undistort` (src/framefilter/Undistorter.cpp:83-88) on an MI355X: the HIP remap against the numpy
restatement of OpenCV 3.1's cv::undistort (tests/undistort_ref.py) byte for byte -- single frames, the one-launch
multi-stream device entry, deferred completion, in place, recalibration -- and the drop-in binary in a process pipeline."""
import ctypes as C

import numpy as np
import pytest

import undistort_ref as R

pytestmark = pytest.mark.gpu


def _frame(rows, cols, ch, seed):
    """Texture with edges and every grey level: random blocks over a ramp, so every fraction of the bilinear cell matters."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:rows, 0:cols]
    ramp = ((xx * 7 + yy * 3) % 256).astype(np.int64)
    blocks = rng.integers(0, 256, ((rows + 7) // 8, (cols + 7) // 8, ch)).repeat(8, 0).repeat(8, 1)[:rows, :cols]
    noise = rng.integers(0, 64, (rows, cols, ch))
    f = ((ramp[..., None] + blocks + noise) % 256).astype(np.uint8)
    return f if ch == 3 else f[..., 0].copy()


@pytest.mark.parametrize("rows,cols,ch,names", [
    (2160, 3840, 3, ("reference", "barrel", "rational8")),
    (2160, 3840, 1, ("pincushion", "skew")),
    (1080, 1920, 3, ("mild5", "pincushion", "skew")),
    (1080, 1920, 1, ("reference", "barrel", "rational8", "mild5")),
    (61, 37, 3, ("reference", "barrel", "pincushion", "skew")),      # odd size: the frame's last lane is partial
])
def test_filter_equals_the_restatement(rows, cols, ch, names):
    import oat_amd
    cases = R.cases(rows, cols)
    img = _frame(rows, cols, ch, rows + cols + ch)
    K0, D0 = cases[names[0]]
    ud = oat_amd.Undistorter(rows, cols, K0, D0, channels=ch)
    try:
        for name in names:
            K, D = cases[name]
            ud.set_calibration(0, K, D)
            got = ud.filter(img)
            want = R.undistort(img, K, D)
            assert got.shape == img.shape
            assert np.array_equal(got, want), (name, int((got != want).sum()))
    finally:
        ud.close()


def test_three_streams_three_calibrations_in_one_launch():
    import torch
    import oat_amd
    rows, cols = 1080, 1920
    cases = R.cases(rows, cols)
    names = ("reference", "barrel", "rational8")
    ud = oat_amd.Undistorter(rows, cols, *cases["mild5"], channels=3, n_streams=3)
    try:
        for s, name in enumerate(names):
            ud.set_calibration(s, *cases[name])
        imgs = np.stack([_frame(rows, cols, 3, 100 + s) for s in range(3)])
        fin = torch.from_numpy(imgs).cuda()
        fout = torch.zeros_like(fin)
        torch.cuda.synchronize()
        ud.filter_dev(fin.data_ptr(), fout.data_ptr())
        ud.synchronize()
        got = fout.cpu().numpy()
        for s, name in enumerate(names):
            want = R.undistort(imgs[s], *cases[name])
            assert np.array_equal(got[s], want), (s, name, int((got[s] != want).sum()))
        # a stream without a map: the device entry refuses the whole launch, the frame entry that stream
        ud.set_calibration(1, None, None)
        with pytest.raises(oat_amd.OatGpuError) as e:
            ud.filter_dev(fin.data_ptr(), fout.data_ptr())
        assert e.value.code == -1 and "no undistortion map" in str(e.value)
        with pytest.raises(oat_amd.OatGpuError):
            ud.filter(imgs[1], stream=1)
        assert np.array_equal(ud.filter(imgs[2], stream=2), R.undistort(imgs[2], *cases["rational8"]))
    finally:
        ud.close()


def test_deferred_in_place_and_recalibration():
    import oat_amd
    from oat_amd import ffi
    rows, cols = 480, 640
    cases = R.cases(rows, cols)
    img = _frame(rows, cols, 3, 5)
    ud = oat_amd.Undistorter(rows, cols, *cases["barrel"], channels=3)
    lib = ud.lib
    try:
        want = R.undistort(img, *cases["barrel"])
        # deferred: the output argument is left alone, oatgpu_fetch_frame delivers the plain call's bytes
        ffi.check(lib, ud.ctx, lib.oatgpu_set_deferred(ud.ctx, 1))
        out = np.full_like(img, 99)
        ffi.check(lib, ud.ctx, lib.oatgpu_undistort_filter(ud.ctx, 0, ffi.u8(img), ffi.u8(out)))
        assert (out == 99).all()
        ffi.check(lib, ud.ctx, lib.oatgpu_fetch_frame(ud.ctx, ffi.u8(out)))
        assert np.array_equal(out, want)
        ffi.check(lib, ud.ctx, lib.oatgpu_set_deferred(ud.ctx, 0))
        # in place (the reference clones first)
        buf = img.copy()
        ffi.check(lib, ud.ctx, lib.oatgpu_undistort_filter(ud.ctx, 0, ffi.u8(buf), ffi.u8(buf)))
        assert np.array_equal(buf, want)
        # a new calibration between frames takes effect at the next frame
        ud.set_calibration(0, *cases["pincushion"])
        assert np.array_equal(ud.filter(img), R.undistort(img, *cases["pincushion"]))
        # refused calibrations leave the map alone
        for bad in ([0.1] * 4, [0.1] * 6, [0.1] * 7):
            with pytest.raises(oat_amd.OatGpuError):
                ud.set_calibration(0, cases["pincushion"][0], bad)
        assert np.array_equal(ud.filter(img), R.undistort(img, *cases["pincushion"]))
        # removed: the stream fails cleanly
        ud.set_calibration(0, None, None)
        with pytest.raises(oat_amd.OatGpuError) as e:
            ud.filter(img)
        assert e.value.code == -1
    finally:
        ud.close()


def test_pipeline_frameserve_undistort_from_config_file(tmp_path):
    """oat-frameserve-raw -> oat-framefilt-hip undistort -c golden.toml undistort -> oat-posidet-hip thresh -> oat-posi-cout:
    every frame's position is the one of the restated undistortion, and END reaches the reader (every process exits 0).
    The reference's own calibration (tests/golden/undistort_reference_config.toml) on its 520 x 816 frames."""
    import os
    import subprocess
    import oracle_lib as O
    from test_host_pipeline import BIN, ROOT, _grey_chain
    subprocess.check_call(["make", "-s", "-j4", "-C", ROOT, "host"])
    rows, cols = 520, 816
    K, D = R.reference_config()
    frames = []
    for t in range(5):
        f = np.zeros((rows, cols), np.uint8)
        yy, xx = np.mgrid[0:rows, 0:cols]
        cx, cy = 380 + 9 * t, 240 + 5 * t
        d2 = (xx - cx) ** 2 + (yy - cy) ** 2
        f[:] = np.clip(255 - d2 // 12, 0, 255)           # a soft disc: its thresholded area follows every grey level
        frames.append(f)
    cfg = os.path.join(ROOT, "tests", "golden", "undistort_reference_config.toml")
    got = _grey_chain(BIN, tmp_path, frames, ["undistort", "-c", cfg, "undistort"])
    p = O.hsv_params(h_lo=100, h_hi=256, erode=0, dilate=0, min_area=4.0, max_area=1e5)
    assert len(got) == len(frames)
    for f, g in zip(frames, got):
        want, _ = O.detect_thresh(R.undistort(f, K, D), p)
        assert want["valid"] and g["pos_ok"]
        # (oat-posi-cout prints the position to the reference's serializer precision)
        assert abs(g["pos_xy"][0] - want["x"]) < 1e-4 and abs(g["pos_xy"][1] - want["y"]) < 1e-4
