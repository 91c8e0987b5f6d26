"""Host-side mirror of the reference's operator interface for the hot path.

Class and method names follow jonnew/Oat so that the parity tests read like the
reference's call sites:

    BackgroundSubtractorMOG.filter(frame)      src/framefilter/BackgroundSubtractorMOG.cpp:114-127
    ColorConvert.filter(frame)                 src/framefilter/ColorConvert.cpp:101-107
    HSVDetector.detectPosition(frame, pos)     src/positiondetector/HSVDetector.cpp:142-173
    SimpleThreshold.detectPosition(frame, pos) src/positiondetector/SimpleThreshold.cpp:114-134
    Undistorter.filter(frame)                  src/framefilter/Undistorter.cpp:83-88

``HotPath`` is the fused, batched form (N camera streams, one launch per stage).
All pixel work happens in liboatgpu.so on the GPU.
"""
import ctypes as C
import os
import re
from dataclasses import dataclass

import numpy as np

from . import ffi

DBL_MAX = float(np.finfo(np.float64).max)


@dataclass
class Position2D:
    """The fields posidet writes into oat::Position2D (lib/datatypes/Position2D.h:112-127)."""
    position_valid: bool = False
    x: float = 0.0
    y: float = 0.0
    area: float = 0.0          # siftContours' object_area out-parameter
    a00: int = 0
    a10: int = 0
    a01: int = 0
    first_pixel: int = -1
    velocity_valid: bool = False   # set by the position filter (HotPath.set_kalman)
    vx: float = 0.0
    vy: float = 0.0
    raw_valid: bool = False        # the detector's own result when the filter is on
    raw_x: float = 0.0
    raw_y: float = 0.0

    @staticmethod
    def from_c(p):
        return Position2D(bool(p.valid), p.x, p.y, p.area, p.a00, p.a10, p.a01, p.first_pixel,
                          bool(p.velocity_valid), p.vx, p.vy, bool(p.raw_valid), p.raw_x, p.raw_y)


@dataclass
class Combined:
    """What `posicom mean` writes into oat::Position2D (src/positioncombiner/MeanPosition.cpp:60-118): the mean of a camera's
    markers and, with a heading anchor, the unit vector from the anchor marker to the others."""
    position_valid: bool = False
    x: float = 0.0
    y: float = 0.0
    heading_valid: bool = False
    hx: float = 0.0
    hy: float = 0.0
    velocity_valid: bool = False   # always False here: the filter chain publishes its own record (Filtered)
    n_valid: int = 0               # markers found

    @staticmethod
    def from_c(p):
        return Combined(bool(p.position_valid), p.x, p.y, bool(p.heading_valid), p.hx, p.hy, bool(p.velocity_valid), p.n_valid)


@dataclass
class Filtered:
    """The combined record of one camera behind the filter chain of HotPath.set_marker_filters (`posifilt kalman` ->
    `posifilt homography` -> `posifilt region`): what the camera's oat::Position2D holds behind the three filters."""
    position_valid: bool = False
    x: float = 0.0
    y: float = 0.0
    velocity_valid: bool = False
    vx: float = 0.0
    vy: float = 0.0
    heading_valid: bool = False
    hx: float = 0.0
    hy: float = 0.0
    region_valid: bool = False
    region: str = None             # name of the first configured region that holds the position, None: none

    @staticmethod
    def from_c(p, names):
        return Filtered(bool(p.position_valid), p.x, p.y, bool(p.velocity_valid), p.vx, p.vy, bool(p.heading_valid), p.hx, p.hy,
                        bool(p.region_valid), names[p.region] if p.region_valid else None)


@dataclass
class Track(Filtered):
    """One track slot of one camera (set_tracks): the slot's record behind kalman -> homography -> region, and its identity."""
    id: int = 0                    # 0: the slot is not live
    rank: int = -1                 # the rank the slot took this frame, -1: none
    age: int = 0                   # frames since birth
    missed: int = 0                # consecutive frames without a measurement

    @staticmethod
    def from_c(t, names):
        f = Filtered.from_c(t.filtered, names)
        return Track(**f.__dict__, id=int(t.id), rank=int(t.rank), age=int(t.age), missed=int(t.missed))


@dataclass
class Shape:
    """One ranked blob's shape (set_target_shapes; oatgpu_shape in include/oatgpu.h has the exact definitions): the exact order-2
    sums of its external contour, its bounding box (cv::boundingRect: x_min, y_min, x_max - x_min + 1, y_max - y_min + 1), the
    central moments, the unit vector along the body (axis_x >= 0: an axis has no front) and the axes of the equivalent ellipse."""
    valid: bool = False
    a20: int = 0
    a11: int = 0
    a02: int = 0
    x_min: int = 0
    y_min: int = 0
    x_max: int = 0
    y_max: int = 0
    mu20: float = 0.0
    mu11: float = 0.0
    mu02: float = 0.0
    axis_valid: bool = False
    axis_x: float = 0.0
    axis_y: float = 0.0
    major: float = 0.0
    minor: float = 0.0

    @staticmethod
    def from_c(p):
        return Shape(bool(p.valid), int(p.a20), int(p.a11), int(p.a02), int(p.x_min), int(p.y_min), int(p.x_max), int(p.y_max),
                     p.mu20, p.mu11, p.mu02, bool(p.axis_valid), p.axis_x, p.axis_y, p.major, p.minor)


def _marker(m):
    """dict(h=(lo,hi), s=(lo,hi), v=(lo,hi), erode=K, dilate=K, area=(a,b)) -- every key optional, the defaults are
    HSVDetector's (all-pass window, erode off, dilate 10, area [0, DBL_MAX)); GREY contexts: h is the intensity window --
    or an ffi.Marker."""
    if isinstance(m, ffi.Marker):
        return m
    m = dict(m)
    h, s, v = m.pop("h", (0, 256)), m.pop("s", (0, 256)), m.pop("v", (0, 256))
    area = m.pop("area", (0.0, DBL_MAX))
    out = ffi.Marker(int(h[0]), int(h[1]), int(s[0]), int(s[1]), int(v[0]), int(v[1]), int(m.pop("erode", 0)),
                     int(m.pop("dilate", 10)), float(area[0]), float(area[1]))
    if m:
        raise TypeError(f"unknown marker option(s) {sorted(m)}")
    return out


def _frame(a, shape):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.shape != shape:
        raise ValueError(f"expected frame of shape {shape}, got {a.shape}")
    return a


class _Context:
    """Owns one oatgpu_ctx."""

    def __init__(self, rows, cols, n_streams=1, device=0, ring_depth=4, **overrides):
        self.lib = ffi.load()
        cfg = ffi.Config()
        self.lib.oatgpu_default_config(C.byref(cfg))
        cfg.rows, cfg.cols, cfg.n_streams, cfg.device, cfg.ring_depth = rows, cols, n_streams, device, ring_depth
        for k, v in overrides.items():
            if not hasattr(cfg, k):
                raise TypeError(f"unknown option {k}")
            setattr(cfg, k, v)
        self.cfg = cfg
        self.rows, self.cols, self.n_streams = rows, cols, n_streams
        self.channels = cfg.channels
        self.frame_shape = (rows, cols, 3) if cfg.channels == 3 else (rows, cols)
        self.ctx = self.lib.oatgpu_create(C.byref(cfg))
        if not self.ctx:
            raise ffi.OatGpuError(-1, (self.lib.oatgpu_last_error(None) or b"").decode())

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.oatgpu_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        ffi.check(self.lib, self.ctx, rc)

    def set_roi_mask(self, mask, stream=0):
        """framefilt mask fused in front of mog: mask (rows, cols) uint8, nonzero = keep; None clears."""
        if mask is None:
            self._chk(self.lib.oatgpu_set_roi_mask(self.ctx, stream, None))
        else:
            m = _frame(mask, (self.rows, self.cols))
            self._chk(self.lib.oatgpu_set_roi_mask(self.ctx, stream, ffi.u8(m)))

    def traffic_audit(self, on=True):
        """Count what the fused per-pixel kernel loads and stores (slower launches; never time them)."""
        self._chk(self.lib.oatgpu_traffic_audit(self.ctx, 1 if on else 0))

    def traffic_read(self):
        t = ffi.Traffic()
        self._chk(self.lib.oatgpu_traffic_read(self.ctx, C.byref(t)))
        return {n: getattr(t, n) for n, _ in ffi.Traffic._fields_}

    def measure_hbm(self, nbytes=1 << 30, reps=5):
        """(read_GBps, copy_GBps) of plain streaming kernels on this device."""
        r, c = C.c_double(0), C.c_double(0)
        self._chk(self.lib.oatgpu_measure_hbm(self.ctx, int(nbytes), int(reps), C.byref(r), C.byref(c)))
        return r.value, c.value

    # -- taps ------------------------------------------------------------
    def read_mask(self, which=ffi.TAP_MORPH, stream=0):
        out = np.empty((self.rows, self.cols), np.uint8)
        self._chk(self.lib.oatgpu_read_mask(self.ctx, stream, which, ffi.u8(out)))
        return out

    def mog_state(self, stream=0):
        n, k = self.rows * self.cols, self.cfg.nmixtures
        nm = np.empty(n, np.uint8)
        w = np.empty((n, k), np.float32)
        v = np.empty((n, k), np.float32)
        m = np.empty((n, k, self.channels), np.float32)
        nf = C.c_int32(0)
        self._chk(self.lib.oatgpu_mog_get_state(self.ctx, stream, ffi.u8(nm), ffi.f32(w), ffi.f32(v), ffi.f32(m),
                                                C.byref(nf)))
        return nm, w, v, m, nf.value

    def set_mog_state(self, nm, w, v, m, nframes, stream=0):
        nm = np.ascontiguousarray(nm, np.uint8)
        w, v, m = (np.ascontiguousarray(a, np.float32) for a in (w, v, m))
        self._chk(self.lib.oatgpu_mog_set_state(self.ctx, stream, ffi.u8(nm), ffi.f32(w), ffi.f32(v), ffi.f32(m),
                                                int(nframes)))


    def save_mog_state(self, path, stream=0):
        """Checkpoint the MOG2 model of one stream to a file (oatgpu_mog_save)."""
        self._chk(self.lib.oatgpu_mog_save(self.ctx, stream, os.fsencode(path)))

    def load_mog_state(self, path, stream=0):
        """Resume from a checkpoint; geometry / channels / mixture count must match."""
        self._chk(self.lib.oatgpu_mog_load(self.ctx, stream, os.fsencode(path)))


class BackgroundSubtractorMOG(_Context):
    """framefilt mog.  ``adaptation_coeff`` is the reference's -a option (default 0)."""

    def __init__(self, rows, cols, adaptation_coeff=0.0, **kw):
        if not 0.0 <= adaptation_coeff <= 1.0:
            raise ValueError("adaptation-coeff must be in [0, 1]")   # BackgroundSubtractorMOG.cpp:86-88
        super().__init__(rows, cols, **kw)
        self.learning_coeff_ = float(adaptation_coeff)

    def filter(self, frame, stream=0):
        """In place, like FrameFilter::filter(cv::Mat&); also returns the frame."""
        f = _frame(frame, self.frame_shape)
        out = frame if (isinstance(frame, np.ndarray) and frame.flags.c_contiguous and frame.dtype == np.uint8) else f
        self._chk(self.lib.oatgpu_mog_filter(self.ctx, stream, ffi.u8(f), ffi.u8(out), self.learning_coeff_))
        return out

    def apply(self, frame, learning_rate=None, stream=0):
        """cv::BackgroundSubtractorMOG2::apply: returns the {0,127,255} mask."""
        f = _frame(frame, self.frame_shape)
        mask = np.empty((self.rows, self.cols), np.uint8)
        lr = self.learning_coeff_ if learning_rate is None else float(learning_rate)
        self._chk(self.lib.oatgpu_mog_apply(self.ctx, stream, ffi.u8(f), ffi.u8(mask), lr))
        return mask


class BackgroundSubtractor(_Context):
    """framefilt bsub (BackgroundSubtractor.cpp): -a adaptation coefficient, first frame = background."""

    def __init__(self, rows, cols, adaptation_coeff=0.0, **kw):
        super().__init__(rows, cols, **kw)
        self.alpha_ = float(adaptation_coeff)

    def filter(self, frame, stream=0):
        f = _frame(frame, self.frame_shape)
        out = np.empty_like(f)
        self._chk(self.lib.oatgpu_bsub_filter(self.ctx, stream, ffi.u8(f), ffi.u8(out), self.alpha_))
        return out


class Threshold(_Context):
    """framefilt thresh (Threshold.cpp): -I [min,max] intensity passband."""

    def __init__(self, rows, cols, intensity=(0, 256), **kw):
        super().__init__(rows, cols, **kw)
        self.i_min_, self.i_max_ = int(intensity[0]), int(intensity[1])

    def filter(self, frame):
        f = _frame(frame, self.frame_shape)
        out = np.empty_like(f)
        self._chk(self.lib.oatgpu_thresh_filter(self.ctx, ffi.u8(f), ffi.u8(out), self.i_min_, self.i_max_))
        return out


def _calibration(camera_matrix, distortion_coeffs):
    K = np.ascontiguousarray(camera_matrix, np.float64).reshape(-1)
    if K.size != 9:
        raise ValueError("'camera-matrix' must be a TOML vector containing 9 elements.")   # TOMLSanitize.h:338-341
    D = np.ascontiguousarray(distortion_coeffs, np.float64).reshape(-1)
    return K, D


def undistort_map(rows, cols, camera_matrix, distortion_coeffs):
    """cv::undistort's map (OpenCV 3.1, CV_16SC2) of a rows x cols frame, built on the host without a device:
    (map1 int16 (rows, cols, 2) = (sx, sy), map2 uint16 (rows, cols) = fy * 32 + fx in 1/32 px)."""
    lib = ffi.load()
    K, D = _calibration(camera_matrix, distortion_coeffs)
    map1 = np.empty((rows, cols, 2), np.int16)
    map2 = np.empty((rows, cols), np.uint16)
    ffi.check(lib, None, lib.oatgpu_undistort_map(rows, cols, K.ctypes.data_as(C.POINTER(C.c_double)),
                                                  D.ctypes.data_as(C.POINTER(C.c_double)), D.size,
                                                  map1.ctypes.data_as(C.POINTER(C.c_int16)),
                                                  map2.ctypes.data_as(C.POINTER(C.c_uint16))))
    return map1, map2


class Undistorter(_Context):
    """framefilt undistort (Undistorter.cpp): -k camera matrix (9 values), -d distortion coefficients (5 or 8).
    Every stream starts with the same calibration; set_calibration gives one stream its own."""

    def __init__(self, rows, cols, camera_matrix, distortion_coeffs, channels=3, n_streams=1, **kw):
        super().__init__(rows, cols, n_streams=n_streams, channels=channels, **kw)
        for s in range(n_streams):
            self.set_calibration(s, camera_matrix, distortion_coeffs)

    def set_calibration(self, stream, camera_matrix, distortion_coeffs):
        """New calibration of one stream; distortion_coeffs None or empty removes its map."""
        if distortion_coeffs is None or len(distortion_coeffs) == 0:
            self._chk(self.lib.oatgpu_set_undistort(self.ctx, stream, None, None, 0))
            return
        K, D = _calibration(camera_matrix, distortion_coeffs)
        self._chk(self.lib.oatgpu_set_undistort(self.ctx, stream, K.ctypes.data_as(C.POINTER(C.c_double)),
                                                D.ctypes.data_as(C.POINTER(C.c_double)), D.size))

    def filter(self, frame, stream=0):
        f = _frame(frame, self.frame_shape)
        out = np.empty_like(f)
        self._chk(self.lib.oatgpu_undistort_filter(self.ctx, stream, ffi.u8(f), ffi.u8(out)))
        return out

    def filter_dev(self, frames_dev, out_dev):
        """Every stream's frame, device pointers (stream-major), one launch on the context's stream (not waited for)."""
        self._chk(self.lib.oatgpu_undistort_dev(self.ctx, C.c_void_p(frames_dev), C.c_void_p(out_dev)))

    def synchronize(self):
        self._chk(self.lib.oatgpu_synchronize(self.ctx))

    def get_stream(self):
        return self.lib.oatgpu_get_stream(self.ctx)


_BAYER_NAMES = {"RGGB": ffi.BAYER_RGGB, "BGGR": ffi.BAYER_BGGR, "GRBG": ffi.BAYER_GRBG, "GBRG": ffi.BAYER_GBRG}


def bayer_pattern(p):
    """A Bayer pattern as the library's value: a name ("RGGB": the 2 x 2 tile at rows 0-1, columns 0-1, row by row) or the
    value itself (1..4; anything else is left for the library to refuse)."""
    if isinstance(p, str):
        if p.upper() not in _BAYER_NAMES:
            raise ValueError(f"unknown Bayer pattern {p!r} (RGGB, BGGR, GRBG or GBRG)")
        return _BAYER_NAMES[p.upper()]
    return int(p)


def _bayer_patterns(patterns):
    ps = [patterns] if isinstance(patterns, (str, int, np.integer)) else list(patterns)
    vals = [bayer_pattern(p) for p in ps]
    return (C.c_int32 * max(len(vals), 1))(*vals), len(vals)


class Debayer(_Context):
    """Bayer RAW8 -> BGR, the frame server's pixel-format conversion (PointGreyCam.cpp:48-50, :729) as a component:
    OpenCV 3.1's bilinear demosaic, bit for bit (include/oatgpu.h)."""

    def filter(self, raw, pattern):
        f = _frame(raw, (self.rows, self.cols))
        out = np.empty((self.rows, self.cols, 3), np.uint8)
        self._chk(self.lib.oatgpu_debayer_filter(self.ctx, bayer_pattern(pattern), ffi.u8(f), ffi.u8(out)))
        return out

    def filter_dev(self, raw_dev, bgr_dev, patterns):
        """Every stream's frame, device pointers (stream-major: n_streams*rows*cols bytes in, *3 out), one launch on the
        context's stream (not waited for); patterns: one for all streams, or one a stream."""
        arr, n = _bayer_patterns(patterns)
        self._chk(self.lib.oatgpu_debayer_dev(self.ctx, arr, n, C.c_void_p(raw_dev), C.c_void_p(bgr_dev)))

    def synchronize(self):
        self._chk(self.lib.oatgpu_synchronize(self.ctx))

    def get_stream(self):
        return self.lib.oatgpu_get_stream(self.ctx)


PIX_BINARY, PIX_GREY, PIX_BGR, PIX_HSV = 0, 1, 2, 3      # oat::PixelColor (Color.h:29-34)
_COLOR_NAMES = {"BINARY": PIX_BINARY, "GREY": PIX_GREY, "BGR": PIX_BGR, "HSV": PIX_HSV}


class ColorConvert(_Context):
    """framefilt col -C COLOR (ColorConvert.cpp): `color` = the colour to convert to, as the reference's
    --color option (default HSV, the bridge in front of `posidet hsv`); the source colour is what the
    frame source carries (`from_color`, default BGR).  Pairs with nothing to do or not possible raise
    with the reference's texts."""

    def __init__(self, rows, cols, color="HSV", from_color="BGR", **kw):
        super().__init__(rows, cols, **kw)
        self.color_ = _COLOR_NAMES[color] if isinstance(color, str) else int(color)
        self.from_ = _COLOR_NAMES[from_color] if isinstance(from_color, str) else int(from_color)

    def filter(self, frame):
        shape_in = (self.rows, self.cols, 3) if self.from_ >= PIX_BGR else (self.rows, self.cols)
        f = _frame(frame, shape_in)
        out = np.empty((self.rows, self.cols, 3) if self.color_ >= PIX_BGR else (self.rows, self.cols), np.uint8)
        self._chk(self.lib.oatgpu_cvt_color(self.ctx, self.from_, self.color_, ffi.u8(f), ffi.u8(out)))
        return out


class _Detector(_Context):
    def _set(self, **kw):
        c = self.cfg
        for k, v in kw.items():
            setattr(c, k, v)
        self._chk(self.lib.oatgpu_set_detector(self.ctx, c.h_lo, c.h_hi, c.s_lo, c.s_hi, c.v_lo, c.v_hi,
                                               c.erode, c.dilate, c.min_area, c.max_area))

    # -- what the readers of the target family share --
    def _delivered(self, room, read):
        """The sets the latest delivering call handed out, through one of the oatgpu_* readers: room(sets) -> buffers for `sets`
        frame sets, read(buffers, sets) -> the reader's return.  A sequence call delivers more sets than there was room for at
        first: the refusal names their number.  -> (buffers, sets delivered)"""
        sets = 1
        while True:
            bufs = room(sets)
            rc = read(bufs, sets)
            if rc >= 0:
                return bufs, rc
            text = (self.lib.oatgpu_last_error(self.ctx) or b"").decode()
            m = re.search(r"the latest call delivered (\d+)", text)
            if not m or int(m.group(1)) <= sets:
                self._chk(rc)
            sets = int(m.group(1))

    def _window_table(self, windows):
        """windows: one list per camera, all of one length, of ffi.CropWindow or (valid, upright, cx, cy, ax, ay) -> (the table as
        the explicit calls take it, windows a camera)"""
        n = self.n_streams
        if len(windows) != n:
            raise ValueError(f"expected windows of {n} cameras, got {len(windows)}")
        per = len(windows[0])
        if any(len(cam) != per for cam in windows):
            raise ValueError("every camera takes the same number of windows")
        arr = (ffi.CropWindow * max(n * per, 1))()
        for s, cam in enumerate(windows):
            for q, win in enumerate(cam):
                if not isinstance(win, ffi.CropWindow):
                    valid, upright, cx, cy, ax, ay = win
                    win = ffi.CropWindow(int(bool(valid)), int(bool(upright)), float(cx), float(cy), float(ax), float(ay))
                arr[s * per + q] = win
        return arr, per

    # -- multi-target detection (oatgpu_set_targets / oatgpu_targets) --
    def set_targets(self, k):
        """The k largest blobs of every camera, ranked, beside the ordinary result of every detecting call; 0 switches it off
        (the default), at most ffi.MAX_TARGETS.  A step with targets on takes the global blob kernels and, in HotPath, the plain
        launch order."""
        self._chk(self.lib.oatgpu_set_targets(self.ctx, int(k)))
        self._targets_k = int(k)

    def targets(self):
        """oatgpu_targets: the target sets of the frame sets the latest result-delivering call handed out -- a list with one
        entry per frame set (one for a track / collect / detectPosition call, one per frame for a sequence call), each a list
        with one (ranks, n_found) pair per camera: ranks is k Position2D, area descending, ties to the later first pixel, rank
        0 the ordinary result, invalid where fewer candidates exist; n_found is the number of candidates (it may exceed k).
        Nothing is consumed."""
        n, k = self.n_streams, getattr(self, "_targets_k", 0)
        (out, found), got = self._delivered(lambda sets: ((ffi.Position * (sets * n * max(k, 1)))(), (C.c_int32 * (sets * n))()),
                                            lambda bufs, sets: self.lib.oatgpu_targets(self.ctx, bufs[0], bufs[1], sets))
        return [[([Position2D.from_c(out[(t * n + s) * k + j]) for j in range(k)], int(found[t * n + s])) for s in range(n)]
                for t in range(got)]

    # -- target shapes (oatgpu_set_target_shapes / oatgpu_target_shapes) --
    def set_target_shapes(self, on=True):
        """Second moments, bounding box and body axis of every ranked blob beside every target set (set_targets must be on): one
        more kernel behind the ranking.  A successful call starts the delivered lists over, targets() included."""
        self._chk(self.lib.oatgpu_set_target_shapes(self.ctx, 1 if on else 0))

    def target_shapes(self):
        """oatgpu_target_shapes: the shape sets of the frame sets the latest result-delivering call handed out -- a list with one
        entry per frame set, each a list with one list of k Shape (rank order, as targets()) per camera.  With tracks on,
        shapes[track.rank] is the shape of an identified animal.  Nothing is consumed."""
        n, k = self.n_streams, getattr(self, "_targets_k", 0)
        out, got = self._delivered(lambda sets: (ffi.Shape * (sets * n * max(k, 1)))(),
                                   lambda out, sets: self.lib.oatgpu_target_shapes(self.ctx, out, sets))
        return [[[Shape.from_c(out[(t * n + s) * k + j]) for j in range(k)] for s in range(n)] for t in range(got)]

    # -- target crops (oatgpu_set_target_crops / oatgpu_target_crops / oatgpu_crop_windows_dev) --
    def _crop_shape(self, *lead):
        return lead + ((3,) if self.channels == 3 else ())

    def set_target_crops(self, h, w=None, axis=False):
        """An h x w window of the input frame around every ranked blob beside every target set of the motion and the subtraction
        tracker (set_targets must be on; axis=True turns each window so that the blob's body axis lies along its +x and needs
        set_target_shapes).  set_target_crops(None) switches crops off.  1 <= h <= 256, 4 <= w <= 256, w a multiple of 4.  A
        successful call starts the delivered lists over, targets() and target_shapes() included."""
        if h is None:
            self._chk(self.lib.oatgpu_set_target_crops(self.ctx, ffi.CROP_OFF, 0, 0))
            self._crop_hw = None
            return
        w = h if w is None else w
        self._chk(self.lib.oatgpu_set_target_crops(self.ctx, ffi.CROP_AXIS if axis else ffi.CROP_UPRIGHT, int(h), int(w)))
        self._crop_hw = (int(h), int(w))

    def target_crops(self):
        """oatgpu_target_crops: the crop sets of the frame sets the latest track / track_dev / track_sequence_dev call of a
        batched tracker handed out -- a uint8 array [sets, n_streams, k, h, w] (GREY) or [sets, n_streams, k, h, w, 3]; rank
        order as targets(), zeros where a rank is empty.  With tracks on, crops[t, s, track.rank] is the window of an
        identified animal.  Nothing is consumed."""
        n, k = self.n_streams, getattr(self, "_targets_k", 0)
        h, w = getattr(self, "_crop_hw", None) or (1, 4)
        out, got = self._delivered(lambda sets: np.empty(self._crop_shape(sets, n, max(k, 1), h, w), np.uint8),
                                   lambda out, sets: self.lib.oatgpu_target_crops(self.ctx, ffi.u8(out), sets))
        return out[:got]

    def crop_windows(self, frames_dev, windows, h, w):
        """oatgpu_crop_windows_dev: h x w windows at given centres and axes from one frame set in device memory (frames_dev: the
        device address of n_streams * rows * cols * channels bytes, stream-major, any alignment).  windows: one list per camera,
        all of one length 1..8, of ffi.CropWindow or (valid, upright, cx, cy, ax, ay).  Returns a uint8 array
        [n_streams, per_stream, h, w] or [..., 3]; an invalid window is zeros."""
        n = self.n_streams
        arr, per = self._window_table(windows)
        out = np.empty(self._crop_shape(n, max(per, 1), max(int(h), 1), max(int(w), 1)), np.uint8)
        self._chk(self.lib.oatgpu_crop_windows_dev(self.ctx, C.c_void_p(frames_dev), arr, per, int(h), int(w), ffi.u8(out)))
        return out

    # -- crop tensors (oatgpu_set_target_crop_tensor / oatgpu_target_crop_tensor_sets / oatgpu_crop_tensor_windows_dev) --
    _TENSOR_DTYPES = {"uint8": ffi.TENSOR_U8, "float16": ffi.TENSOR_F16, "float32": ffi.TENSOR_F32}

    def _tensor_fmt(self, dtype, scale, bias):
        name = str(dtype).replace("torch.", "")
        if name not in self._TENSOR_DTYPES:
            raise ValueError(f"dtype must be 'uint8', 'float16' or 'float32', got {dtype!r}")

        def three(v, what):
            v = [float(x) for x in (v if hasattr(v, "__len__") else [v] * self.channels)]
            if len(v) != self.channels:
                raise ValueError(f"{what}: a scalar or one value per channel ({self.channels}), got {len(v)}")
            return (C.c_float * 3)(*(v + [v[-1]] * (3 - len(v))))
        return name, ffi.CropTensorFmt(self._TENSOR_DTYPES[name], 0, three(scale, "scale"), three(bias, "bias"))

    def _tensor_shape(self, name, lead, h, w):
        return tuple(lead) + ((h, w, self.channels) if name == "uint8" else (self.channels, h, w))

    def _torch_device(self):
        import torch
        return torch.device("cuda", self.cfg.device)

    def set_target_crop_tensor(self, h, w=None, axis=False, zoom=1.0, dtype="float16", scale=1.0, bias=0.0, capacity=1):
        """Crop tensors: the windows of set_target_crops as a torch tensor on the context's device, written by the same track /
        track_dev / track_sequence_dev calls of a batched tracker with no host round trip (set_targets must be on; axis=True needs
        set_target_shapes).  zoom: source pixels per output pixel (1/16 .. 16; not 1: always the bilinear gather, point-sampled).
        dtype "float16" / "float32": planar values float32(float32(p * scale[c]) + bias[c]), scale and bias scalars or one value
        per channel in the frame's order (BGR); "uint8": the window's bytes.  Allocates a zeroed tensor
        [capacity, n_streams, k, C, h, w] ([capacity, n_streams, k, h, w, C] for "uint8"; C = 1 for GREY contexts), keeps it alive
        and returns it; frame set t of a call lands in entry t, so a sequence call takes at most `capacity` frames.
        set_target_crop_tensor(None) switches it off and drops the tensor.  Independent of set_target_crops."""
        if h is None:
            self._chk(self.lib.oatgpu_set_target_crop_tensor(self.ctx, ffi.CROP_OFF, 0, 0, 1.0, None, None, 0))
            self._crop_tensor = None
            return None
        import torch
        w = h if w is None else w
        name, fmt = self._tensor_fmt(dtype, scale, bias)
        k = getattr(self, "_targets_k", 0)
        shape = self._tensor_shape(name, (max(int(capacity), 1), self.n_streams, max(k, 1)), max(int(h), 1), max(int(w), 1))
        t = torch.zeros(shape, dtype=getattr(torch, name), device=self._torch_device())
        torch.cuda.synchronize(t.device)
        self._chk(self.lib.oatgpu_set_target_crop_tensor(self.ctx, ffi.CROP_AXIS if axis else ffi.CROP_UPRIGHT, int(h), int(w), float(zoom),
                                                         C.byref(fmt), C.c_void_p(t.data_ptr()), int(capacity)))
        self._crop_tensor = t
        return t

    def target_crop_tensor(self):
        """The entries the latest track / track_dev / track_sequence_dev call of a batched tracker wrote: the zero-copy view
        tensor[:sets] of set_target_crop_tensor's tensor (one entry for a step, one per frame for a sequence call)."""
        sets = self.lib.oatgpu_target_crop_tensor_sets(self.ctx)
        if sets < 0:
            self._chk(sets)
        return self._crop_tensor[:sets]

    def crop_tensor_windows(self, frames_dev, windows, h, w, dtype="float16", scale=1.0, bias=0.0):
        """oatgpu_crop_tensor_windows_dev: crop_windows' windows, converted, as a fresh torch tensor on the context's device --
        [n_streams, per_stream, C, h, w], or [n_streams, per_stream, h, w, C] for "uint8".  There is no zoom argument: a window
        that is not upright carries it in (ax, ay)."""
        import torch
        n = self.n_streams
        arr, per = self._window_table(windows)
        name, fmt = self._tensor_fmt(dtype, scale, bias)
        out = torch.zeros(self._tensor_shape(name, (n, max(per, 1)), max(int(h), 1), max(int(w), 1)), dtype=getattr(torch, name),
                          device=self._torch_device())
        torch.cuda.synchronize(out.device)
        self._chk(self.lib.oatgpu_crop_tensor_windows_dev(self.ctx, C.c_void_p(frames_dev), arr, per, int(h), int(w), C.byref(fmt),
                                                          C.c_void_p(out.data_ptr())))
        return out

    # -- target masks (oatgpu_set_target_mask_tensor / oatgpu_target_mask_tensor_sets) --
    def set_target_mask_tensor(self, h, w=None, axis=False, zoom=1.0, dtype="uint8", capacity=1):
        """Target masks: for the window set_target_crop_tensor(h, w, axis, zoom) cuts around every ranked blob, which of its pixels
        ARE that blob -- not another animal, a reflection, a blob in its hole or background -- as a torch tensor on the context's
        device, written by the same track / track_dev / track_sequence_dev calls of a batched tracker (set_targets must be on;
        axis=True needs set_target_shapes).  An element is ON where the pixel nearest to where the crop tensor samples is set in
        the final mask and belongs to the rank's 8-connected component: 255 / 0 for "uint8", 1.0 / 0.0 for "float16" / "float32".
        Allocates a zeroed tensor [capacity, n_streams, k, h, w] (no channel axis), keeps it alive and returns it; frame set t of
        a call lands in entry t, so a sequence call takes at most `capacity` frames.  set_target_mask_tensor(None) switches it off
        and drops the tensor.  Independent of set_target_crops and set_target_crop_tensor; works behind bayer(...) and
        undistort(True), where those two are refused."""
        if h is None:
            self._chk(self.lib.oatgpu_set_target_mask_tensor(self.ctx, ffi.CROP_OFF, 0, 0, 1.0, 0, None, 0))
            self._mask_tensor = None
            return None
        import torch
        w = h if w is None else w
        name = str(dtype).replace("torch.", "")
        if name not in self._TENSOR_DTYPES:
            raise ValueError(f"dtype must be 'uint8', 'float16' or 'float32', got {dtype!r}")
        k = getattr(self, "_targets_k", 0)
        shape = (max(int(capacity), 1), self.n_streams, max(k, 1), max(int(h), 1), max(int(w), 1))
        t = torch.zeros(shape, dtype=getattr(torch, name), device=self._torch_device())
        torch.cuda.synchronize(t.device)
        self._chk(self.lib.oatgpu_set_target_mask_tensor(self.ctx, ffi.CROP_AXIS if axis else ffi.CROP_UPRIGHT, int(h), int(w), float(zoom),
                                                         self._TENSOR_DTYPES[name], C.c_void_p(t.data_ptr()), int(capacity)))
        self._mask_tensor = t
        return t

    def target_mask_tensor(self):
        """The entries the latest track / track_dev / track_sequence_dev call of a batched tracker wrote: the zero-copy view
        tensor[:sets] of set_target_mask_tensor's tensor (one entry for a step, one per frame for a sequence call)."""
        sets = self.lib.oatgpu_target_mask_tensor_sets(self.ctx)
        if sets < 0:
            self._chk(sets)
        return self._mask_tensor[:sets]

    # -- target tracks (oatgpu_set_tracks / oatgpu_tracks / oatgpu_tracks_update) --
    def set_tracks(self, kalman=None, gate=float("inf"), homography=None, regions=None):
        """oatgpu_set_tracks: k persistent track slots per camera (k of set_targets, which must be on) behind the ranked
        detections -- greedy nearest-neighbour assignment inside `gate` pixels, one Kalman filter a slot (kalman: a dict as
        set_filters takes it, required), then homography and regions where given.  kalman=None switches tracks off.  A
        successful call restarts every slot and the ids.  The batched trackers advance tracks with every frame; every other
        detector goes through update_tracks."""
        if kalman is None:
            self._chk(self.lib.oatgpu_set_tracks(self.ctx, None, float(gate)))
            return
        f, names, _keep = _filter_chain(kalman, homography, regions)
        self._chk(self.lib.oatgpu_set_tracks(self.ctx, C.byref(f), float(gate)))
        self._track_region_names = names

    def _tracks_out(self, out, sets):
        n, k, names = self.n_streams, getattr(self, "_targets_k", 0), getattr(self, "_track_region_names", [])
        return [[[Track.from_c(out[(t * n + s) * k + i], names) for i in range(k)] for s in range(n)] for t in range(sets)]

    def tracks(self):
        """oatgpu_tracks: the track sets of the frame sets the latest delivering call handed out -- a list with one entry per
        frame set, each a list with one list of k Track (slot order) per camera.  Nothing is consumed."""
        n, k = self.n_streams, getattr(self, "_targets_k", 0)
        out, got = self._delivered(lambda sets: (ffi.Track * (sets * n * max(k, 1)))(),
                                   lambda out, sets: self.lib.oatgpu_tracks(self.ctx, out, sets))
        return self._tracks_out(out, got)

    def update_tracks(self, targets):
        """oatgpu_tracks_update: one association step on one frame set of detections -- targets: one entry of targets(), or a
        list with one list of k Position2D (or (valid, x, y)) per camera.  Returns one list of k Track per camera."""
        n, k = self.n_streams, getattr(self, "_targets_k", 0)
        if len(targets) != n:
            raise ValueError(f"expected detections of {n} cameras, got {len(targets)}")
        arr = (ffi.Position * (n * max(k, 1)))()
        for s, cam in enumerate(targets):
            ranks = cam[0] if isinstance(cam, tuple) and len(cam) == 2 and isinstance(cam[1], (int, np.integer)) else cam
            if len(ranks) != k:
                raise ValueError(f"expected {k} detections a camera, got {len(ranks)}")
            for j, p in enumerate(ranks):
                valid, x, y = (p.position_valid, p.x, p.y) if isinstance(p, Position2D) else p
                a = arr[s * k + j]
                a.valid, a.x, a.y = int(bool(valid)), float(x), float(y)
        out = (ffi.Track * (n * max(k, 1)))()
        self._chk(self.lib.oatgpu_tracks_update(self.ctx, arr, out))
        return self._tracks_out(out, 1)[0]


class HSVDetector(_Detector):
    """posidet hsv.  Options follow HSVDetector.cpp:49-75 (-H -S -V -e -d -a)."""

    def __init__(self, rows, cols, h_thresh=(0, 256), s_thresh=(0, 256), v_thresh=(0, 256),
                 erode=0, dilate=10, area=(0.0, DBL_MAX), **kw):
        super().__init__(rows, cols, h_lo=h_thresh[0], h_hi=h_thresh[1], s_lo=s_thresh[0], s_hi=s_thresh[1],
                         v_lo=v_thresh[0], v_hi=v_thresh[1], erode=erode, dilate=dilate,
                         min_area=area[0], max_area=area[1], **kw)

    def detectPosition(self, frame, position=None, stream=0):
        f = _frame(frame, (self.rows, self.cols, 3))
        p = ffi.Position()
        self._chk(self.lib.oatgpu_detect_hsv(self.ctx, stream, ffi.u8(f), C.byref(p)))
        return _merge(position, p)


class SimpleThreshold(_Detector):
    """posidet thresh.  Options follow SimpleThreshold.cpp:49-69 (-T -e -d -a); erode/dilate default off."""

    def __init__(self, rows, cols, thresh=(0, 256), erode=0, dilate=0, area=(0.0, DBL_MAX), **kw):
        super().__init__(rows, cols, h_lo=thresh[0], h_hi=thresh[1], erode=erode, dilate=dilate,
                         min_area=area[0], max_area=area[1], **kw)

    def detectPosition(self, frame, position=None, stream=0):
        f = _frame(frame, (self.rows, self.cols))
        p = ffi.Position()
        self._chk(self.lib.oatgpu_detect_thresh(self.ctx, stream, ffi.u8(f), C.byref(p)))
        return _merge(position, p)


class DifferenceDetector(_Detector):
    """posidet diff.  Options follow DifferenceDetector.cpp:47-64 (-d diff-threshold, -b blur, -a area)."""

    def __init__(self, rows, cols, diff_threshold=10, blur=2, area=(0.0, DBL_MAX), **kw):
        super().__init__(rows, cols, diff_threshold=diff_threshold, blur=blur, erode=0, dilate=0,
                         min_area=area[0], max_area=area[1], **kw)

    def detectPosition(self, frame, position=None, stream=0):
        f = _frame(frame, (self.rows, self.cols))
        p = ffi.Position()
        self._chk(self.lib.oatgpu_detect_diff(self.ctx, stream, ffi.u8(f), C.byref(p)))
        return _merge(position, p)


def _filter_chain(kalman, homography, regions):
    """ffi.MarkerFilters of a chain kalman -> homography -> region (oatgpu_set_marker_filters, oatgpu_set_tracker_filters):
    kalman = None or a dict with any of dt / timeout / sigma_accel / sigma_noise (set_kalman's defaults); homography = None or a
    3x3 matrix; regions = None or a list of (name, points) with points = [(x, y), ...].  Returns (struct, region names, what
    the struct points into: to be kept alive across the call)."""
    f = ffi.MarkerFilters()
    if kalman is not None:
        k = dict(dt=0.02, timeout=0.0, sigma_accel=5.0, sigma_noise=0.0)
        unknown = set(kalman) - set(k)
        if unknown:
            raise TypeError(f"unknown kalman option(s) {sorted(unknown)}")
        k.update(kalman)
        f.kalman, f.dt, f.timeout, f.sigma_accel, f.sigma_noise = 1, k["dt"], k["timeout"], k["sigma_accel"], k["sigma_noise"]
    if homography is not None:
        f.homography = 1
        f.h = (C.c_double * 9)(*np.asarray(homography, np.float64).reshape(9))
    regions = list(regions or [])
    arr = (ffi.Region * max(len(regions), 1))()
    keep, names = [], []
    for r, (name, points) in zip(arr, regions):
        raw = name.encode() if isinstance(name, str) else bytes(name)
        pts = np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 2))
        keep.append(pts)
        r.name = raw[:10]                              # (10 bytes leave no room for the terminator: the library refuses)
        r.n_points = len(pts)
        r.xy = pts.ctypes.data_as(C.POINTER(C.c_double))
        names.append(raw.decode())
    f.n_regions = len(regions)
    f.regions = arr
    return f, names, (arr, keep)


def _set_chain(ctx, entry, kalman, homography, regions):
    """A chain through `entry` (oatgpu_set_marker_filters, oatgpu_set_tracker_filters); the context remembers its region names."""
    f, names, _keep = _filter_chain(kalman, homography, regions)
    ctx._chk(entry(ctx.ctx, C.byref(f)))
    ctx._region_names = names


def _read_chain(ctx, entry, sets):
    """The filtered sets of the latest delivering call through `entry` (oatgpu_marker_filtered, oatgpu_tracker_filtered), with
    room for `sets` of them: a list with one list of n_streams Filtered per frame set."""
    n, sets = ctx.n_streams, max(sets, 1)
    out = (ffi.Filtered * (sets * n))()
    rc = entry(ctx.ctx, out, sets)
    if rc < 0:
        ctx._chk(rc)
    names = getattr(ctx, "_region_names", [])
    return [[Filtered.from_c(out[t * n + s], names) for s in range(n)] for t in range(rc)]


def _packed_shape(ctx):
    """A BGR / GREY frame of the context, whatever its track calls take at the moment."""
    return (ctx.rows, ctx.cols, 3) if ctx.channels == 3 else (ctx.rows, ctx.cols)


def _set_bayer(ctx, entry, patterns):
    """Bayer RAW8 ingest through `entry` (oatgpu_set_track_bayer, oatgpu_set_tracker_bayer), and the frames the track calls take."""
    if patterns is None:
        ctx._chk(entry(ctx.ctx, None, 0))
        ctx.frame_shape = _packed_shape(ctx)
        return
    arr, n = _bayer_patterns(patterns)
    ctx._chk(entry(ctx.ctx, arr, n))
    ctx.frame_shape = (ctx.rows, ctx.cols)


class _TrackerBayer:
    """oatgpu_set_tracker_bayer for the batched trackers (HotPath.bayer is the same body, _set_bayer, on its own entry point)."""

    def bayer(self, patterns):
        """oatgpu_set_tracker_bayer: track, track_dev and track_sequence_dev take Bayer RAW8 frames (rows, cols) and the front
        kernel demosaics them in registers; the state stays in the demosaiced domain.  patterns: a name ("RGGB") or value for
        every stream, a list of n_streams of them, or None to switch it off (frames are BGR again)."""
        _set_bayer(self, self.lib.oatgpu_set_tracker_bayer, patterns)


class _TrackerUndistort:
    """oatgpu_set_tracker_undistort for the batched trackers (mirrors HotPath.undistort; set_undistort is HotPath's too)."""

    def set_undistort(self, stream, camera_matrix, distortion_coeffs):
        """The undistortion map of one camera stream (oatgpu_set_undistort): camera_matrix 9 values, distortion_coeffs
        5 or 8.  Allowed while undistort() is on (a recalibration: it takes effect from the next frame)."""
        K, D = _calibration(camera_matrix, distortion_coeffs)
        self._chk(self.lib.oatgpu_set_undistort(self.ctx, int(stream), K.ctypes.data_as(C.POINTER(C.c_double)),
                                                D.ctypes.data_as(C.POINTER(C.c_double)), D.size))

    def undistort(self, on=True):
        """oatgpu_set_tracker_undistort: track, track_dev and track_sequence_dev remap each stream's frame with its map inside
        the front kernel, ahead of the ROI mask; the state stays in the undistorted domain.  Every stream needs a map
        (set_undistort) to switch it on; not together with bayer()."""
        self._chk(self.lib.oatgpu_set_tracker_undistort(self.ctx, 1 if on else 0))

    def _undistort_all(self, calibration):
        """The constructor's undistort=(K, D): one calibration for every stream, switched on."""
        K, D = calibration
        for st in range(self.n_streams):
            self.set_undistort(st, K, D)
        self.undistort(True)


class _TrackerFilters:
    """oatgpu_set_tracker_filters / oatgpu_tracker_filtered for the batched trackers (HotPath.set_marker_filters / marker_filtered
    are the same bodies, _set_chain / _read_chain, on their own entry points)."""

    def set_filters(self, kalman=None, homography=None, regions=None):
        """oatgpu_set_tracker_filters: the chain behind every camera's detection, in the fixed order kalman -> homography ->
        region; arguments as HotPath.set_marker_filters.  All None switches the chain off.  A successful call restarts every
        camera's Kalman state; track, track_dev and track_sequence_dev then advance it by one sample a frame."""
        _set_chain(self, self.lib.oatgpu_set_tracker_filters, kalman, homography, regions)

    def filtered(self):
        """oatgpu_tracker_filtered: the filtered records of the frame sets the latest track call delivered -- a list with one
        entry per frame set (one for track / track_dev, one per frame for track_sequence_dev), each a list of n_streams
        Filtered.  Nothing is consumed."""
        return _read_chain(self, self.lib.oatgpu_tracker_filtered, getattr(self, "_tf_sets", 1))


class MotionTracker(_Detector, _TrackerBayer, _TrackerUndistort, _TrackerFilters):
    """The batched motion tracker: `framefilt col -C GREY` -> `posidet diff` for N camera streams, one front launch a step
    (oatgpu_set_diff_tracker).  channels = 3: BGR frames (rows, cols, 3); 1: GREY frames (rows, cols).  Options follow
    DifferenceDetector.cpp:47-64 (-d diff-threshold, -b blur, -a area).  A ROI (set_roi_mask) masks the frame first.
    bayer: Bayer RAW8 frames (rows, cols) of a BGR tracker, see bayer().
    undistort: a (camera_matrix, distortion_coeffs) tuple -- `framefilt undistort` in front of the chain for every stream, see
    set_undistort() and undistort()."""

    def __init__(self, rows, cols, n_streams=1, channels=3, diff_threshold=10, blur=2, area=(0.0, DBL_MAX), device=0, bayer=None,
                 undistort=None, **kw):
        super().__init__(rows, cols, n_streams=n_streams, channels=channels, diff_threshold=diff_threshold, blur=blur,
                         erode=0, dilate=0, min_area=area[0], max_area=area[1], device=device, **kw)
        self._pos = (ffi.Position * n_streams)()
        self._chk(self.lib.oatgpu_set_diff_tracker(self.ctx, 1))
        if bayer is not None:
            self.bayer(bayer)
        if undistort is not None:
            self._undistort_all(undistort)

    def _out(self):
        return [Position2D.from_c(p) for p in self._pos]

    def track(self, frames):
        """frames: sequence of n_streams host arrays -> one Position2D per stream (oatgpu_diff_batch)."""
        fs = [_frame(f, self.frame_shape) for f in frames]
        ptrs = (ffi._u8p * max(len(fs), 1))(*[ffi.u8(f) for f in fs])
        self._tf_sets = 1                                  # (filtered: one frame set is delivered)
        self._chk(self.lib.oatgpu_diff_batch(self.ctx, ptrs, len(fs), self._pos))
        return self._out()

    def track_dev(self, dev_ptr):
        """dev_ptr: device address of n_streams*rows*cols*channels bytes, stream-major (oatgpu_diff_batch_dev)."""
        self._tf_sets = 1
        self._chk(self.lib.oatgpu_diff_batch_dev(self.ctx, C.c_void_p(dev_ptr), self._pos))
        return self._out()

    def track_sequence_dev(self, dev_ptrs):
        """A recorded sequence in one call (oatgpu_diff_sequence_dev): dev_ptrs[t] = device address of frame set t; returns
        one list of Position2D per frame set."""
        T, n = len(dev_ptrs), self.n_streams
        arr = (C.c_void_p * max(T, 1))(*dev_ptrs)
        out = (ffi.Position * max(T * n, 1))()
        self._tf_sets = T
        self._chk(self.lib.oatgpu_diff_sequence_dev(self.ctx, arr, T, out))
        return [[Position2D.from_c(out[t * n + s]) for s in range(n)] for t in range(T)]

    def reset(self, stream=None):
        """Forget the last image of one stream (None: of all): its next frame is a first frame again (oatgpu_diff_reset)."""
        self._chk(self.lib.oatgpu_diff_reset(self.ctx, -1 if stream is None else int(stream)))

    def read_mask(self, which=ffi.TAP_MORPH, stream=0):
        """A plane of the latest diff frame (oatgpu_read_diff_mask)."""
        out = np.empty((self.rows, self.cols), np.uint8)
        self._chk(self.lib.oatgpu_read_diff_mask(self.ctx, int(stream), which, ffi.u8(out)))
        return out


class SubtractionTracker(_Detector, _TrackerBayer, _TrackerUndistort, _TrackerFilters):
    """The batched subtraction tracker: `framefilt bsub` -> `framefilt col -C HSV` -> `posidet hsv` for N camera streams, one front
    launch a step (oatgpu_set_bsub_tracker).  channels = 3: BGR frames (rows, cols, 3) and the h / s / v window on the difference
    image; 1: GREY frames (rows, cols), `framefilt bsub` -> `posidet thresh` with `thresh`.  alpha is bsub's -a (0: the background
    stays the first frame); erode / dilate / area as HSVDetector.cpp:49-75.  A ROI (set_roi_mask) masks the frame first.
    bayer: Bayer RAW8 frames (rows, cols) of a BGR tracker, see bayer(); the background and its state stay BGR.
    undistort: a (camera_matrix, distortion_coeffs) tuple -- `framefilt undistort` in front of the chain for every stream, see
    set_undistort() and undistort(); the background and its state are images in undistorted coordinates."""

    def __init__(self, rows, cols, n_streams=1, channels=3, alpha=0.0, h_thresh=(0, 256), s_thresh=(0, 256), v_thresh=(0, 256),
                 thresh=None, erode=0, dilate=10, area=(0.0, DBL_MAX), device=0, bayer=None, undistort=None, **kw):
        if thresh is not None:
            h_thresh = thresh
        super().__init__(rows, cols, n_streams=n_streams, channels=channels, h_lo=h_thresh[0], h_hi=h_thresh[1], s_lo=s_thresh[0],
                         s_hi=s_thresh[1], v_lo=v_thresh[0], v_hi=v_thresh[1], erode=erode, dilate=dilate, min_area=area[0],
                         max_area=area[1], device=device, **kw)
        self.alpha_ = float(alpha)
        self._pos = (ffi.Position * n_streams)()
        self._chk(self.lib.oatgpu_set_bsub_tracker(self.ctx, 1))
        if bayer is not None:
            self.bayer(bayer)
        if undistort is not None:
            self._undistort_all(undistort)

    def _alpha(self, alpha):
        return float(getattr(self, "alpha_", 0.0) if alpha is None else alpha)

    def track(self, frames, alpha=None):
        """frames: sequence of n_streams host arrays -> one Position2D per stream (oatgpu_bsub_track_batch)."""
        fs = [_frame(f, self.frame_shape) for f in frames]
        ptrs = (ffi._u8p * max(len(fs), 1))(*[ffi.u8(f) for f in fs])
        pos = (ffi.Position * self.n_streams)()
        self._tf_sets = 1                                  # (filtered: one frame set is delivered)
        self._chk(self.lib.oatgpu_bsub_track_batch(self.ctx, ptrs, len(fs), SubtractionTracker._alpha(self, alpha), pos))
        return [Position2D.from_c(p) for p in pos]

    def track_dev(self, dev_ptr, alpha=None):
        """dev_ptr: device address of n_streams*rows*cols*channels bytes, stream-major (oatgpu_bsub_track_batch_dev)."""
        pos = (ffi.Position * self.n_streams)()
        self._tf_sets = 1
        self._chk(self.lib.oatgpu_bsub_track_batch_dev(self.ctx, C.c_void_p(dev_ptr), SubtractionTracker._alpha(self, alpha), pos))
        return [Position2D.from_c(p) for p in pos]

    def track_sequence_dev(self, dev_ptrs, alpha=None):
        """A recorded sequence in one call (oatgpu_bsub_track_sequence_dev): dev_ptrs[t] = device address of frame set t; returns
        one list of Position2D per frame set."""
        T, n = len(dev_ptrs), self.n_streams
        arr = (C.c_void_p * max(T, 1))(*dev_ptrs)
        out = (ffi.Position * max(T * n, 1))()
        self._tf_sets = T
        self._chk(self.lib.oatgpu_bsub_track_sequence_dev(self.ctx, arr, T, SubtractionTracker._alpha(self, alpha), out))
        return [[Position2D.from_c(out[t * n + s]) for s in range(n)] for t in range(T)]

    def reset(self, stream=None):
        """Forget the background of one stream (None: of all): its next frame is a first frame again (oatgpu_bsub_reset)."""
        self._chk(self.lib.oatgpu_bsub_reset(self.ctx, -1 if stream is None else int(stream)))

    def set_background(self, image, stream=0):
        """`framefilt bsub -f FILE`: the background of one stream from an image; it cannot adapt (oatgpu_bsub_set_background)."""
        im = _frame(image, _packed_shape(self))
        self._chk(self.lib.oatgpu_bsub_set_background(self.ctx, int(stream), ffi.u8(im)))

    def state(self, stream=0, acc=True):
        """(background uint8, accumulator float32 or None) of one stream as it stands (oatgpu_bsub_get_state)."""
        bg = np.empty(_packed_shape(self), np.uint8)
        f = np.empty(_packed_shape(self), np.float32) if acc else None
        self._chk(self.lib.oatgpu_bsub_get_state(self.ctx, int(stream), ffi.u8(bg), ffi.f32(f) if acc else None))
        return bg, f

    def read_mask(self, which=ffi.TAP_MORPH, stream=0):
        """A plane of the latest subtraction-tracker frame (oatgpu_read_bsub_mask)."""
        out = np.empty((self.rows, self.cols), np.uint8)
        self._chk(self.lib.oatgpu_read_bsub_mask(self.ctx, int(stream), which, ffi.u8(out)))
        return out


def _merge(position, p):
    """siftContours only writes x/y when a blob is found (DetectorFunc.cpp:46,58-60)."""
    new = Position2D.from_c(p)
    if position is None:
        return new
    position.position_valid = new.position_valid
    position.area = new.area
    if new.position_valid:
        position.x, position.y = new.x, new.y
    position.a00, position.a10, position.a01, position.first_pixel = new.a00, new.a10, new.a01, new.first_pixel
    return position


class HotPath(_Detector):
    """The fused chain for N camera streams: mog + setTo + BGR2HSV + inRange + erode + dilate + blob.  The detector is
    re-configured between frames with _set(h_lo=.., erode=.., min_area=..) (oatgpu_set_detector).

    undistort: `framefilt undistort` in front of the chain (oatgpu_set_track_undistort) -- one (camera_matrix,
    distortion_coeffs) tuple for every stream, or a list of n_streams such tuples (one calibration per camera)."""

    def __init__(self, rows, cols, n_streams=1, adaptation_coeff=0.0, h_thresh=(0, 256), s_thresh=(0, 256),
                 v_thresh=(0, 256), erode=0, dilate=10, area=(0.0, DBL_MAX), undistort=None, **kw):
        super().__init__(rows, cols, n_streams=n_streams, h_lo=h_thresh[0], h_hi=h_thresh[1], s_lo=s_thresh[0],
                         s_hi=s_thresh[1], v_lo=v_thresh[0], v_hi=v_thresh[1], erode=erode, dilate=dilate,
                         min_area=area[0], max_area=area[1], **kw)
        self.learning_coeff_ = float(adaptation_coeff)
        self._pos = (ffi.Position * n_streams)()
        if undistort is not None:
            cals = undistort if isinstance(undistort, list) else [undistort] * n_streams
            if len(cals) != n_streams:
                raise ValueError(f"undistort: {len(cals)} calibrations for {n_streams} streams (give one, or one a stream)")
            for st, (K, D) in enumerate(cals):
                self.set_undistort(st, K, D)
            self.undistort(True)

    set_undistort = _TrackerUndistort.set_undistort        # (oatgpu_set_undistort: a stream's one map, whichever tracker reads it)

    def undistort(self, on=True):
        """oatgpu_set_track_undistort: every track call remaps each stream's frame with its map before the ROI mask and
        MOG2.  Every stream needs a map (set_undistort) to switch it on."""
        self._chk(self.lib.oatgpu_set_track_undistort(self.ctx, 1 if on else 0))

    def bayer(self, patterns):
        """oatgpu_set_track_bayer: every track call takes Bayer RAW8 frames (rows, cols) and demosaics them on the device
        before anything else.  patterns: a name ("RGGB") or value for every stream, a list of n_streams of them, or None to
        switch it off (frames are BGR again)."""
        _set_bayer(self, self.lib.oatgpu_set_track_bayer, patterns)

    def _out(self):
        return [Position2D.from_c(p) for p in self._pos]

    def detect_hsv(self, hsv, stream=0):
        """The single-stage `posidet hsv` of this context (oatgpu_detect_hsv) on an HSV image: synchronous, never filtered."""
        p = ffi.Position()
        self._chk(self.lib.oatgpu_detect_hsv(self.ctx, int(stream), ffi.u8(_frame(hsv, (self.rows, self.cols, 3))), C.byref(p)))
        return Position2D.from_c(p)

    def detect_thresh(self, grey, stream=0):
        """The single-stage `posidet thresh` (oatgpu_detect_thresh) on a GREY image; -T is the context's h window."""
        p = ffi.Position()
        self._chk(self.lib.oatgpu_detect_thresh(self.ctx, int(stream), ffi.u8(_frame(grey, (self.rows, self.cols))), C.byref(p)))
        return Position2D.from_c(p)

    def track(self, frames):
        """frames: sequence of n_streams host arrays (rows, cols, 3), or (rows, cols) when channels == 1."""
        fs = [_frame(f, self.frame_shape) for f in frames]
        ptrs = (ffi._u8p * len(fs))(*[ffi.u8(f) for f in fs])
        self._chk(self.lib.oatgpu_track_batch(self.ctx, ptrs, len(fs), self.learning_coeff_, self._pos))
        return self._out()

    def track_dev(self, dev_ptr):
        """dev_ptr: device address of n_streams*rows*cols*3 bytes (e.g. torch tensor .data_ptr())."""
        self._chk(self.lib.oatgpu_track_batch_dev(self.ctx, C.c_void_p(dev_ptr), self.learning_coeff_, self._pos))
        return self._out()

    def track_sequence_dev(self, dev_ptrs, timed=False):
        """A recorded sequence in one call (oatgpu_track_sequence_dev): dev_ptrs[t] = device address of
        frame set t; returns one list of Position2D per frame -- and, with timed=True
        (oatgpu_track_sequence_dev_timed), the seconds after the call's entry at which each frame's result was collected."""
        n = len(dev_ptrs)
        arr = (C.c_void_p * n)(*dev_ptrs)
        out = (ffi.Position * (n * self.n_streams))()
        if timed:
            done = (C.c_double * max(n, 1))()
            self._chk(self.lib.oatgpu_track_sequence_dev_timed(self.ctx, arr, n, self.learning_coeff_, out, done))
        else:
            self._chk(self.lib.oatgpu_track_sequence_dev(self.ctx, arr, n, self.learning_coeff_, out))
        res = [[Position2D.from_c(out[t * self.n_streams + s]) for s in range(self.n_streams)] for t in range(n)]
        return (res, [done[t] for t in range(n)]) if timed else res

    # -- marker sets: several colour windows per camera behind one model pass, `posicom mean` behind them --------------
    def set_markers(self, markers, heading_anchor=None):
        """oatgpu_set_markers: markers = a list of up to 8 marker dicts (see _marker) used for every camera; heading_anchor =
        index of the marker headings are taken from (`posicom mean --heading-anchor`), None for no heading.  An empty list
        switches markers off and frees their scratch.  The context's own window must be the non-zero window
        (h_thresh=(0,256), s_thresh=(0,256), v_thresh=(1,256); GREY: h_thresh=(1,256)) when track_markers is called."""
        ms = [_marker(m) for m in markers]
        arr = (ffi.Marker * max(len(ms), 1))(*ms)
        self._chk(self.lib.oatgpu_set_markers(self.ctx, len(ms), arr if ms else None,
                                              -1 if heading_anchor is None else int(heading_anchor)))
        self.n_markers = len(ms)
        self._mpos = (ffi.Position * max(self.n_streams * len(ms), 1))()
        self._mean = (ffi.Combined * self.n_streams)()
        self._region_names = []                            # (every successful oatgpu_set_markers drops the filter chain)

    def set_marker_filters(self, kalman=None, homography=None, regions=None):
        """oatgpu_set_marker_filters: the chain behind every camera's combined record, in the fixed order kalman -> homography
        -> region.  kalman = None or a dict with any of dt / timeout / sigma_accel / sigma_noise (set_kalman's defaults);
        homography = None or a 3x3 matrix; regions = None or a list of (name, points) with points = [(x, y), ...], tested in
        the order given.  All None switches the chain off.  A successful call restarts every camera's Kalman state."""
        _set_chain(self, self.lib.oatgpu_set_marker_filters, kalman, homography, regions)

    def marker_filtered(self):
        """oatgpu_marker_filtered: the filtered records of the frame sets the latest marker-result call delivered -- a list with
        one entry per frame set, each a list of n_streams Filtered.  Nothing is consumed."""
        return _read_chain(self, self.lib.oatgpu_marker_filtered, getattr(self, "_mf_sets", 1))

    def set_marker_window(self, stream, marker, h=(0, 256), s=(0, 256), v=(0, 256)):
        """oatgpu_set_marker_window: the colour window of one marker for ONE camera; morphology and area stay per marker."""
        m = _marker(dict(h=h, s=s, v=v))
        self._chk(self.lib.oatgpu_set_marker_window(self.ctx, int(stream), int(marker), C.byref(m)))

    def _markers_out(self):
        M = self.n_markers
        self._mf_sets = 1                                  # (marker_filtered: one frame set was delivered)
        return (self._out(), [[Position2D.from_c(self._mpos[s * M + m]) for m in range(M)] for s in range(self.n_streams)],
                [Combined.from_c(p) for p in self._mean])

    def track_markers(self, frames):
        """One synchronous marker step on host frames (oatgpu_track_markers) -> (fg[n], markers[n][M], mean[n]): the largest
        foreground blob of each camera, every marker's Position2D, the combined position and heading."""
        if not getattr(self, "n_markers", 0):
            raise ffi.OatGpuError(-1, "marker sets are not configured (set_markers)")
        fs = [_frame(f, self.frame_shape) for f in frames]
        ptrs = (ffi._u8p * len(fs))(*[ffi.u8(f) for f in fs])
        self._chk(self.lib.oatgpu_track_markers(self.ctx, ptrs, len(fs), self.learning_coeff_, self._pos, self._mpos, self._mean))
        return self._markers_out()

    def track_markers_dev(self, dev_ptr):
        """The same on frames in device memory (oatgpu_track_markers_dev; dev_ptr as track_dev's)."""
        if not getattr(self, "n_markers", 0):
            raise ffi.OatGpuError(-1, "marker sets are not configured (set_markers)")
        self._chk(self.lib.oatgpu_track_markers_dev(self.ctx, C.c_void_p(dev_ptr), self.learning_coeff_, self._pos, self._mpos,
                                                    self._mean))
        return self._markers_out()

    def marker_pipeline(self, on=True):
        """oatgpu_set_marker_pipeline: marker sets on the pipelined path.  While on, every enqueue form (enqueue, enqueue_dev,
        stage + enqueue_staged, the sequence calls) also queues its frames' marker work; collect_markers() hands it out.
        Needs markers configured, the non-zero own window, no Kalman filter / homography and nothing outstanding."""
        self._chk(self.lib.oatgpu_set_marker_pipeline(self.ctx, 1 if on else 0))

    def collect_markers(self):
        """oatgpu_track_collect_markers: the oldest outstanding frame set -> (fg[n], markers[n][M], mean[n]) as track_markers."""
        if not getattr(self, "n_markers", 0):              # (nothing configured: the library refuses, with its own words)
            self._mpos, self._mean = (ffi.Position * 1)(), (ffi.Combined * self.n_streams)()
        self._chk(self.lib.oatgpu_track_collect_markers(self.ctx, self._pos, self._mpos, self._mean))
        if getattr(self, "_held", None):
            self._held.pop(0)
        return self._markers_out()

    def track_markers_sequence_dev(self, dev_ptrs):
        """A recorded sequence through the pipelined marker path in one call (oatgpu_track_markers_sequence_dev): dev_ptrs[t] =
        device address of frame set t; returns one (fg[n], markers[n][M], mean[n]) per frame set."""
        T, n, M = len(dev_ptrs), self.n_streams, getattr(self, "n_markers", 0)
        arr = (C.c_void_p * max(T, 1))(*dev_ptrs)
        fg = (ffi.Position * max(T * n, 1))()
        mk = (ffi.Position * max(T * n * M, 1))()
        mean = (ffi.Combined * max(T * n, 1))()
        self._chk(self.lib.oatgpu_track_markers_sequence_dev(self.ctx, arr, T, self.learning_coeff_, fg, mk, mean))
        self._mf_sets = T                                  # (marker_filtered: T frame sets were delivered)
        return [([Position2D.from_c(fg[t * n + s]) for s in range(n)],
                 [[Position2D.from_c(mk[(t * n + s) * M + m]) for m in range(M)] for s in range(n)],
                 [Combined.from_c(mean[t * n + s]) for s in range(n)]) for t in range(T)]

    def read_marker_mask(self, marker, which=ffi.TAP_MORPH, stream=0):
        out = np.empty((self.rows, self.cols), np.uint8)
        self._chk(self.lib.oatgpu_read_marker_mask(self.ctx, int(stream), int(marker), which, ffi.u8(out)))
        return out

    def enqueue(self, frames):
        """Pipelined host-frame form (oatgpu_track_enqueue): frames must stay untouched until the
        matching collect(); they are kept referenced here until then."""
        fs = [_frame(f, self.frame_shape) for f in frames]
        ptrs = (ffi._u8p * len(fs))(*[ffi.u8(f) for f in fs])
        self._chk(self.lib.oatgpu_track_enqueue(self.ctx, ptrs, len(fs), self.learning_coeff_))
        self._held = getattr(self, "_held", [])
        self._held.append(fs)

    def enqueue_dev(self, dev_ptr, keepalive=None):
        """Pipelined device-frame form (oatgpu_track_enqueue_dev): dev_ptr -> n_streams*rows*cols*channels bytes.
        By default the per-pixel kernel that reads the frame is queued on the context's stream inside the call.
        After set_fusion(2) it may go out with the NEXT frame's (two frames a launch): the buffer must then stay
        valid and untouched until the frame's result was collected or input_consumed() returned -- pass the owning
        object (a torch tensor) as `keepalive` and it is held here until the matching collect()."""
        self._chk(self.lib.oatgpu_track_enqueue_dev(self.ctx, C.c_void_p(dev_ptr), self.learning_coeff_))
        self._held = getattr(self, "_held", [])
        self._held.append(keepalive)

    def input_consumed(self):
        """Block until every frame handed over so far has been read out of the caller's buffers
        (oatgpu_track_input_consumed): host frames copied, device frames read by their per-pixel kernel."""
        self._chk(self.lib.oatgpu_track_input_consumed(self.ctx))

    def stage(self, stream, frame):
        """oatgpu_track_stage: ONE camera's frame of the next frame set starts its H2D copy now."""
        f = _frame(frame, self.frame_shape)
        self._staged_keep = getattr(self, "_staged_keep", []) + [f]
        self._chk(self.lib.oatgpu_track_stage(self.ctx, int(stream), ffi.u8(f)))

    def enqueue_staged(self):
        """oatgpu_track_enqueue_staged: every stream staged -> the set is registered like enqueue()."""
        self._chk(self.lib.oatgpu_track_enqueue_staged(self.ctx, self.learning_coeff_))
        self._held = getattr(self, "_held", [])
        self._held.append(self._staged_keep)
        self._staged_keep = []

    def set_stage_copy(self, mode):
        """oatgpu_set_stage_copy: 0 = stage() copies by DMA (default), 1 = by a kernel reading the host frame in place."""
        self._chk(self.lib.oatgpu_set_stage_copy(self.ctx, int(mode)))

    def stage_abort(self):
        """oatgpu_track_stage_abort: give up a partly staged set (copies already started are waited for)."""
        self._chk(self.lib.oatgpu_track_stage_abort(self.ctx))
        self._staged_keep = []

    def input_consumed_stream(self, stream):
        """The frame of ONE camera stream of the latest enqueue() has left the caller's buffer
        (oatgpu_track_input_consumed_stream; call for the streams in ascending order)."""
        self._chk(self.lib.oatgpu_track_input_consumed_stream(self.ctx, int(stream)))

    def collect(self):
        self._chk(self.lib.oatgpu_track_collect(self.ctx, self._pos))
        if getattr(self, "_held", None):
            self._held.pop(0)
        return self._out()

    def ready(self):
        """True if collect() would return without blocking (oatgpu_track_ready)."""
        rc = self.lib.oatgpu_track_ready(self.ctx)
        if rc < 0:
            self._chk(rc)
        return rc == 1

    def outstanding(self):
        return self.lib.oatgpu_track_outstanding(self.ctx)

    def set_kalman(self, enable=True, dt=0.02, timeout=0.0, sigma_accel=5.0, sigma_noise=0.0):
        """`posifilt kalman` on the batch (KalmanFilter2D.cpp:63-141; option names and defaults are the
        reference's).  (Re)starts every stream's filter."""
        self._chk(self.lib.oatgpu_set_kalman(self.ctx, int(bool(enable)), dt, timeout, sigma_accel, sigma_noise))

    def set_homography(self, h=None):
        """`posifilt homography` behind the detector / the position filter (HomographyTransform2D.cpp): h = nine numbers,
        row-major [h11, h12, ..., h33]; None turns it off."""
        if h is None:
            self._chk(self.lib.oatgpu_set_homography(self.ctx, 0, None))
        else:
            a = (C.c_double * 9)(*[float(v) for v in np.asarray(h, np.float64).reshape(9)])
            self._chk(self.lib.oatgpu_set_homography(self.ctx, 1, a))

    def set_stream(self, hip_stream):
        self._chk(self.lib.oatgpu_set_stream(self.ctx, C.c_void_p(hip_stream)))

    def get_stream(self):
        """hipStream_t (as an integer) the per-pixel kernel is launched on (oatgpu_get_stream)."""
        return int(self.lib.oatgpu_get_stream(self.ctx) or 0)

    def synchronize(self):
        self._chk(self.lib.oatgpu_synchronize(self.ctx))

    def set_fusion(self, frames_per_launch):
        """Frames per launch of the fused per-pixel kernel on the pipelined path: 1 or 2 (default 2)."""
        self._chk(self.lib.oatgpu_set_fusion(self.ctx, int(frames_per_launch)))

    def set_early_blob(self, on=True):
        """oatgpu_set_early_blob: the blob workgroup of a device-frame step is dispatched ahead of its row scan.
        None: the library's choice by shape (at most three streams, 4 MP a step and more), True / False: forced."""
        self._chk(self.lib.oatgpu_set_early_blob(self.ctx, -1 if on is None else (1 if on else 0)))

    def set_k1_workgroup(self, threads=0):
        """oatgpu_set_k1_workgroup: threads of a workgroup of the per-pixel kernel, 0 = by path (default), 64 or 256."""
        self._chk(self.lib.oatgpu_set_k1_workgroup(self.ctx, int(threads)))

    def last_step_shape(self):
        """(threads of a per-pixel workgroup, blob workgroup dispatched early?) of the latest pipelined step."""
        wg, early = C.c_int32(0), C.c_int32(0)
        self._chk(self.lib.oatgpu_last_step_shape(self.ctx, C.byref(wg), C.byref(early)))
        return wg.value, bool(early.value)

    def set_rowscan_rows(self, rows=0):
        """oatgpu_set_rowscan_rows: image rows a row-scan workgroup takes on the pipelined path, 0 = by pipeline depth
        (default: 16 with four and more frames ahead in the ring, else 4), 4 or 16 = on every eligible step."""
        self._chk(self.lib.oatgpu_set_rowscan_rows(self.ctx, int(rows)))

    def last_step_rowscan_rows(self):
        """Rows a row-scan workgroup of the latest pipelined step took (oatgpu_last_step_rowscan_rows)."""
        return int(self.lib.oatgpu_last_step_rowscan_rows(self.ctx))

    def early_blob_timeouts(self):
        """Frames whose parked blob workgroup gave up waiting for its row scan (oatgpu_early_blob_timeouts)."""
        return int(self.lib.oatgpu_early_blob_timeouts(self.ctx))

    def profile(self, every=1):
        """every = 0/False: off; 1/True: time every step; N: time every Nth step."""
        self._chk(self.lib.oatgpu_profile_enable(self.ctx, int(every)))

    def profile_reset(self):
        self._chk(self.lib.oatgpu_profile_reset(self.ctx))

    def profile_read(self):
        p = ffi.Profile()
        self._chk(self.lib.oatgpu_profile_read(self.ctx, C.byref(p)))
        return dict(steps=p.steps, mog_ms=p.mog_ms, morph_ms=p.morph_ms, blob_ms=p.blob_ms, total_ms=p.total_ms,
                    event_pair_ms=p.event_pair_ms, mog_frames=p.mog_frames, dropped=p.dropped)
