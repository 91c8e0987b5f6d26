"""GPU tests of crop tensors (oatgpu_set_target_crop_tensor / oatgpu_target_crop_tensor_sets / oatgpu_crop_tensor_windows_dev;
_Detector.set_target_crop_tensor / .target_crop_tensor / .crop_tensor_windows; k_crop_tensor in kernels_croptensor.hip).
Every element of every window is compared with the model of tests/crop_tensor_ref.py -- integers, or fp32 / fp16 bit patterns: bit for
bit, no tolerance anywhere -- fed with the oracle chain's own targets and shapes; U8 at zoom 1 with target_crops() and crop_windows()
of the same context; and the ordinary results, targets(), target_shapes(), target_crops(), tracks(), filtered(), the taps and the
states with those of a second context that has the switch off.  Every frame is under 0.004 MP."""
import ctypes as C
import math

import numpy as np
import pytest

import crop_tensor_cases as TC
import crop_tensor_ref as TR
import crops_cases as CC
import crops_ref as R
import targets_cases as T
import tracks_cases as TK

pytestmark = pytest.mark.gpu

E_INVALID = -1
THR, MORPH, FIN = 0, 1, 2
U8 = TC.FORMATS[0]


@pytest.fixture(scope="module")
def A():
    import oat_amd
    import oat_amd.components as comp
    for name in ("SimpleThreshold", "HSVDetector", "DifferenceDetector"):
        if not hasattr(oat_amd, name):
            setattr(oat_amd, name, getattr(comp, name))
    return oat_amd


def _dev(frames, offset=0):
    """frames of one set, stream-major, in device memory `offset` bytes behind an allocation's start -> (tensor kept alive, address)"""
    import torch
    flat = np.concatenate([np.ascontiguousarray(f).reshape(-1) for f in frames])
    buf = torch.zeros(flat.size + offset, dtype=torch.uint8, device="cuda")
    buf[offset:] = torch.from_numpy(flat).cuda()
    torch.cuda.synchronize()
    return buf, buf.data_ptr() + offset


def _refused(fn, *a, **kw):
    from oat_amd.ffi import OatGpuError
    with pytest.raises(OatGpuError) as e:
        fn(*a, **kw)
    assert e.value.code == E_INVALID, e.value
    return str(e.value)


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _same(got, want, tag):
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    if not TR.same_bits(got, want):
        as_int = {1: np.uint8, 2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
        bad = np.argwhere(np.ascontiguousarray(got).view(as_int) != np.ascontiguousarray(want).view(as_int))
        raise AssertionError((tag, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


def _kw(fmt, channels):
    dtype, scale, bias = TC.fmt_for(fmt, channels)
    return dict(dtype=dtype, scale=scale, bias=bias)


# ------------------------------------------------------------------------------------------ oatgpu_crop_tensor_windows_dev ----

EXPLICIT_U8 = [(rows, cols, h, w, ch) for rows, cols in TC.GEOMETRIES for h, w in TC.CROP_SIZES for ch in (1, 3)]
EXPLICIT_FLOAT = [(rows, cols, h, w, ch) for rows, cols in TC.GEOMETRIES for h, w in TC.FLOAT_SIZES for ch in (1, 3)]


def _cropper(A, rows, cols, n, channels):
    """any detector will do: the call needs no switch"""
    return A.MotionTracker(rows, cols, n_streams=n, channels=channels, area=T.AREA, **T.DIFF)


def _explicit_calls(rows, cols, h, w, channels):
    """-> (groups of 8 windows, and for every stream count its calls: (n, frames, offset, [group of stream s]))"""
    gs = [g for kind in TC.explicit_windows(rows, cols, h, w) for g in CC.groups(kind)]
    calls = []
    for n in CC.STREAMS:
        frames = [CC.pattern(rows, cols, channels, CC.variant_of(s)) for s in range(n)]
        for call in range(len(gs) if n == 1 else 2):
            offset = (call + n) % 2                                    # the frame set one byte off a 256-byte boundary, and on it
            calls.append((n, frames, offset, [(call + 5 * s) % len(gs) for s in range(n)]))
    return gs, calls


@pytest.mark.parametrize("rows,cols,h,w,channels", EXPLICIT_U8)
def test_explicit_u8_is_byte_equal_to_crop_windows(A, rows, cols, h, w, channels):
    gs, calls = _explicit_calls(rows, cols, h, w, channels)
    dets = {}
    for i, (n, frames, offset, pick) in enumerate(calls):
        det = dets.setdefault(n, _cropper(A, rows, cols, n, channels))
        keep, ptr = _dev(frames, offset)
        wins = [gs[g] for g in pick]
        got = _host(det.crop_tensor_windows(ptr, wins, h, w, dtype="uint8"))
        assert got.shape == (n, CC.PER_STREAM, h, w, channels)
        got = got[..., 0] if channels == 1 else got
        _same(got, det.crop_windows(ptr, wins, h, w), (n, i))
        if i % 7 == 0:                                                 # ... which is the model's (tests/test_crops_gpu.py); once more here
            _same(got[0], np.stack([R.crop(frames[0], win, h, w) for win in wins[0]]), (n, i, "model"))
        del keep
    for det in dets.values():
        det.close()


@pytest.mark.parametrize("rows,cols,h,w,channels", EXPLICIT_FLOAT)
def test_explicit_floats_against_the_model(A, rows, cols, h, w, channels):
    gs, calls = _explicit_calls(rows, cols, h, w, channels)
    model, dets, used = {}, {}, set()

    def want(variant, g):
        if (variant, g) not in model:
            model[(variant, g)] = np.stack([R.crop(CC.pattern(rows, cols, channels, variant), win, h, w) for win in gs[g]])
        return model[(variant, g)]
    for i, (n, frames, offset, pick) in enumerate(calls):
        det = dets.setdefault(n, _cropper(A, rows, cols, n, channels))
        fmt = TC.FLOAT_FORMATS[(i + h) % len(TC.FLOAT_FORMATS)]
        used.add((n == 1, fmt[0]))
        keep, ptr = _dev(frames, offset)
        got = _host(det.crop_tensor_windows(ptr, [gs[g] for g in pick], h, w, **_kw(fmt, channels)))
        assert got.shape == (n, CC.PER_STREAM, channels, h, w)
        for s in range(n):
            _same(got[s], TC.expected(want(CC.variant_of(s), pick[s]), fmt, channels), (n, i, s, fmt[0]))
        del keep
    assert {name for one, name in used if one} == {f[0] for f in TC.FLOAT_FORMATS}       # every format on every list
    for det in dets.values():
        det.close()


def test_fewer_windows_a_stream_and_a_zoom_in_the_axis(A):
    from oat_amd import ffi
    rows, cols, h, w = 37, 61, 16, 12
    det = _cropper(A, rows, cols, 3, 3)
    frames = [CC.pattern(rows, cols, 3, s) for s in range(3)]
    keep, ptr = _dev(frames, 1)
    fmt = TC.FORMATS[3]
    for per in (1, 3):
        wins = [[R.window(True, False, 20.25 + s, 15.5 - q, z * math.cos(0.3 * q), z * math.sin(0.3 * q)) for q in range(per)]
                for s, z in enumerate(TC.ZOOMS[1:])]
        asc = [[ffi.CropWindow(int(v), int(u), cx, cy, ax, ay) for v, u, cx, cy, ax, ay in cam] for cam in wins]
        got = _host(det.crop_tensor_windows(ptr, asc, h, w, **_kw(fmt, 3)))
        _same(got, TC.expected(R.crop_set(frames, wins, h, w), fmt, 3), per)
    got = _host(det.crop_tensor_windows(ptr, [[R.INVALID]] * 3, 256, 256, **_kw(TC.FORMATS[4], 3)))         # the largest window, invalid: bias
    _same(got, TC.expected(np.zeros((3, 1, 256, 256, 3), np.uint8), TC.FORMATS[4], 3), "256")
    assert (got[:, :, 0] == np.float32(TC.IMAGENET_BIAS[0])).all() and (got[:, :, 2] == np.float32(TC.IMAGENET_BIAS[2])).all()
    det.close()


# ------------------------------------------------------------------------------------------------- the batched trackers ----

KALMAN = dict(kalman=dict(dt=0.02, timeout=0.1, sigma_accel=5.0, sigma_noise=0.5))


def _make_tracker(A, family, rows, cols, n, alpha=0.0, channels=3):
    if family == "motion":
        return A.MotionTracker(rows, cols, n_streams=n, channels=channels, area=T.AREA, **T.DIFF)
    win = T.sub_window()
    return A.SubtractionTracker(rows, cols, n_streams=n, channels=3, alpha=alpha, h_thresh=win["h"], s_thresh=win["s"], v_thresh=win["v"],
                                erode=T.SUB_MORPH[0], dilate=T.SUB_MORPH[1], area=T.AREA)


def _frames_at(family, rows, cols, n, t, channels=3):
    return [CC.sequence(family, rows, cols, CC.variant_of(s), channels)[t] for s in range(n)]


class _Sequence:
    """the 11 frame sets of a run on the host and, one byte off an allocation's start, on the device"""

    def __init__(self, family, rows, cols, n, channels=3):
        self.host = [_frames_at(family, rows, cols, n, t, channels) for t in range(CC.N_FRAMES)]
        self.bufs = [_dev(f, 1) for f in self.host]

    def ptr(self, t):
        return self.bufs[t][1]


def _call(tr, seq, how, t0, count, single=False):
    """one call of a run -> the positions of its frames"""
    if how == "track":
        return [tr.track(seq.host[t0])]
    if how == "track_dev":
        return [tr.track_dev(seq.ptr(t0))]
    if single:
        return [tr.track_dev(seq.ptr(t0 + i)) for i in range(count)]
    return tr.track_sequence_dev([seq.ptr(t0 + i) for i in range(count)])


def _run_setting(tr, seq, run, axis, zoom, fmt, channels=3, crops=False):
    """One setting of the switch on a tracker through TC.RUN_CALLS into one tensor of TC.CAPACITY entries: every element of the WHOLE
    tensor against the model behind every call -- the entries the call delivered, and those it must not touch."""
    family, alpha, rows, cols, n, k, h, w = run
    tensor = tr.set_target_crop_tensor(h, w, axis=axis, zoom=zoom, capacity=TC.CAPACITY, **_kw(fmt, channels))
    want = [TC.expected(TC.entry_u8(family, rows, cols, n, t, alpha, k, axis, zoom, h, w, channels), fmt, channels)
            for t in range(CC.N_FRAMES)]
    if fmt[1] == "uint8" and channels == 1:
        want = [x[..., None] for x in want]                                        # [.., h, w, C] with C = 1
    assert tuple(tensor.shape) == (TC.CAPACITY,) + want[0].shape and not _host(tensor).any()
    mirror = np.zeros((TC.CAPACITY,) + want[0].shape, want[0].dtype)
    assert "no call has delivered" in _refused(tr.target_crop_tensor)
    for i, (how, t0, count) in enumerate(TC.RUN_CALLS):
        if i in (0, TC.RESET_BEFORE):
            tr.reset()
        pos = _call(tr, seq, how, t0, count)
        view = tr.target_crop_tensor()
        assert len(pos) == count == len(view) and view.data_ptr() == tensor.data_ptr()            # zero-copy
        mirror[:count] = np.stack(want[t0:t0 + count])
        _same(_host(tensor), mirror, (family, axis, zoom, fmt[0], how, t0, count))
        if crops:                                                                  # U8 at zoom 1: byte for byte oatgpu_target_crops
            _same(_host(view), tr.target_crops(), (family, axis, "target_crops", how, t0))
    return tensor


@pytest.mark.parametrize("axis", [False, True], ids=["upright", "axis"])
@pytest.mark.parametrize("case", range(len(TC.TRACKER_RUNS)))
def test_batched_trackers(A, case, axis):
    run = TC.TRACKER_RUNS[case]
    family, alpha, rows, cols, n, k, h, w = run
    tr, seq = _make_tracker(A, family, rows, cols, n, alpha), _Sequence(family, rows, cols, n)
    tr.set_targets(k)
    tr.set_target_shapes()
    F, i = TC.FLOAT_FORMATS, case + (3 if axis else 0)
    # zoom 1 in bytes beside target crops of the same size and mode, both switches on in one context
    tr.set_target_crops(h, w, axis=axis)
    _run_setting(tr, seq, run, axis, 1.0, U8, crops=True)
    tr.set_target_crops(None)
    # ... and with only tensors on: every other zoom in a float format, zoom 1 converted (the copy path), one zoom in bytes
    for zoom, fmt in ((0.5, F[i % 6]), (2.0, F[(i + 2) % 6]), (1.37, F[(i + 4) % 6]), (1.0, F[(i + 1) % 6]), (TC.ZOOMS[1 + i % 3], U8)):
        _run_setting(tr, seq, run, axis, zoom, fmt)
    tr.close()


def test_every_zoom_meets_every_dtype_in_the_tracker_runs():
    seen = set()
    for case in range(len(TC.TRACKER_RUNS)):
        for axis in (False, True):
            F, i = TC.FLOAT_FORMATS, case + (3 if axis else 0)
            seen |= {(0.5, F[i % 6][1]), (2.0, F[(i + 2) % 6][1]), (1.37, F[(i + 4) % 6][1]), (1.0, F[(i + 1) % 6][1]),
                     (TC.ZOOMS[1 + i % 3], "uint8"), (1.0, "uint8")}
    assert seen == {(z, d) for z in TC.ZOOMS for d in TR.DTYPES}


def test_grey_frames(A):
    run = ("motion", 0.0, 37, 61, 3, 4, 16, 12)
    family, alpha, rows, cols, n, k, h, w = run
    tr, seq = _make_tracker(A, family, rows, cols, n, channels=1), _Sequence(family, rows, cols, n, channels=1)
    tr.set_targets(k)
    tr.set_target_shapes()
    for axis, zoom, fmt in ((True, 1.37, TC.FORMATS[3]), (False, 1.0, TC.FORMATS[2]), (True, 2.0, U8)):
        t = _run_setting(tr, seq, run, axis, zoom, fmt, channels=1)
        assert tuple(t.shape) == ((TC.CAPACITY, n, k, h, w, 1) if fmt is U8 else (TC.CAPACITY, n, k, 1, h, w))
    tr.close()


@pytest.mark.parametrize("family,alpha", [("motion", 0.0), ("subtraction", 0.05)])
def test_a_paired_launch_against_single_launches(A, family, alpha):
    """The second frame of a paired front launch is cut from ITS frame set into ITS entry: an 11-frame sequence call against one device
    step a frame."""
    rows, cols, n, k, h, w = 48, 64, 3, 4, 16, 12
    assert CC.paired_second(family, TC.PLAN_LONG)
    seq = _Sequence(family, rows, cols, n)
    for axis, zoom, fmt in ((False, 1.0, U8), (True, 2.0, TC.FORMATS[3])):
        got = []
        for single in (False, True):
            tr = _make_tracker(A, family, rows, cols, n, alpha)
            tr.set_targets(k)
            tr.set_target_shapes()
            tensor = tr.set_target_crop_tensor(h, w, axis=axis, zoom=zoom, capacity=TC.CAPACITY, **_kw(fmt, 3))
            if single:
                entries = []
                for t in range(CC.N_FRAMES):
                    tr.track_dev(seq.ptr(t))
                    entries.append(_host(tr.target_crop_tensor())[0].copy())
                got.append(np.stack(entries))
            else:
                tr.track_sequence_dev([seq.ptr(t) for t in range(CC.N_FRAMES)])
                got.append(_host(tr.target_crop_tensor()).copy())
            del tensor
            tr.close()
        _same(got[0], got[1], (family, axis, zoom))


def _run_passengers(A, family, rows, cols, n, alpha, k, h, w, seq, tensor):
    """-> per frame (positions, targets, shapes, crops, filtered, tracks); the taps and the state behind the last frame"""
    tr = _make_tracker(A, family, rows, cols, n, alpha)
    tr.set_filters(**KALMAN)
    tr.set_targets(k)
    tr.set_tracks(**TK.image_config())
    tr.set_target_shapes()
    tr.set_target_crops(h, w, axis=True)
    if tensor:
        tr.set_target_crop_tensor(h + 3, 2 * w, axis=True, zoom=1.37, capacity=5, **_kw(TC.FORMATS[3], 3))       # another size than the crops'
    out = []
    for how, t0, count in TC.calls_of(TC.PLAN):
        pos = _call(tr, seq, how, t0, count)
        out += list(zip(pos, tr.targets(), tr.target_shapes(), tr.target_crops(), tr.filtered(), tr.tracks()))
    taps = [[tr.read_mask(which, s) for which in (THR, MORPH, FIN)] for s in range(n)]
    state = [tr.state(s) for s in range(n)] if family == "subtraction" else None
    tr.close()
    return out, taps, state


@pytest.mark.parametrize("family,alpha", [("motion", 0.0), ("subtraction", 0.05)])
def test_tensors_are_read_only_passengers(A, family, alpha):
    rows, cols, n, k, h, w = 37, 61, 3, 4, 16, 12
    seq = _Sequence(family, rows, cols, n)
    got, taps, state = _run_passengers(A, family, rows, cols, n, alpha, k, h, w, seq, True)
    plain, ptaps, pstate = _run_passengers(A, family, rows, cols, n, alpha, k, h, w, seq, False)
    assert len(got) == len(plain) == 10
    for t, (a, b) in enumerate(zip(got, plain)):
        assert a[0] == b[0], (t, "the ordinary results move with the switch on")
        assert a[1] == b[1] and a[2] == b[2], (t, "the target or shape sets move with the switch on")
        assert np.array_equal(a[3], b[3]), (t, "the crop sets move with the switch on")
        assert a[4] == b[4] and a[5] == b[5], (t, "the filtered records or the tracks move with the switch on")
    for x, y in zip(taps, ptaps):
        for p, q in zip(x, y):
            assert (p == q).all()
    if state is not None:
        for (bg, acc), (pbg, pacc) in zip(state, pstate):
            assert (bg == pbg).all() and (acc == pacc).all()


# ------------------------------------------------------------------------------------------------------------ refusals ----

def test_a_sequence_call_longer_than_the_capacity_is_refused_and_the_next_call_works(A):
    run = ("subtraction", 0.0, 37, 61, 3, 4, 16, 12)
    family, alpha, rows, cols, n, k, h, w = run
    for family in ("subtraction", "motion"):
        tr, seq = _make_tracker(A, family, rows, cols, n), _Sequence(family, rows, cols, n)
        plain = _make_tracker(A, family, rows, cols, n)
        for x in (tr, plain):
            x.set_targets(k)
        fmt = TC.FORMATS[1]
        tensor = tr.set_target_crop_tensor(h, w, zoom=2.0, capacity=4, **_kw(fmt, 3))
        assert "4 entries" in _refused(tr.track_sequence_dev, [seq.ptr(t) for t in range(11)])
        assert "4 entries" in _refused(tr.track_sequence_dev, [seq.ptr(t) for t in range(5)])
        assert not _host(tensor).any() and "no call has delivered" in _refused(tr.target_crop_tensor)      # nothing was launched
        _refused(tr.targets)
        # ... and nothing changed: the next call is the first of a fresh tracker
        pos = tr.track_sequence_dev([seq.ptr(t) for t in range(4)])
        assert pos == plain.track_sequence_dev([seq.ptr(t) for t in range(4)]) and tr.targets() == plain.targets()
        want = np.stack([TC.expected(TC.entry_u8(family, rows, cols, n, t, 0.0, k, False, 2.0, h, w), fmt, 3) for t in range(4)])
        _same(_host(tr.target_crop_tensor()), want, family)
        tr.close()
        plain.close()


def test_refusals_each_leaving_a_working_context(A):
    import torch
    from oat_amd import ffi
    family, alpha, rows, cols, n, k, h, w = "subtraction", 0.0, 37, 61, 3, 4, 16, 12
    tr, seq = _make_tracker(A, family, rows, cols, n), _Sequence(family, rows, cols, n)
    lib, ctx = tr.lib, tr.ctx
    room = torch.zeros(2 * n * k * 3 * h * w + 64, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    out = C.c_void_p(room.data_ptr())

    def fmt(dtype=ffi.TENSOR_F32, reserved=0, scale=(1.0, 1.0, 1.0), bias=(0.0, 0.0, 0.0)):
        return C.byref(ffi.CropTensorFmt(dtype, reserved, (C.c_float * 3)(*scale), (C.c_float * 3)(*bias)))

    def text(rc):
        assert rc == E_INVALID, rc
        return lib.oatgpu_last_error(ctx).decode()

    setter = lib.oatgpu_set_target_crop_tensor
    assert "off" in _refused(tr.target_crop_tensor)                                              # the switch is off
    assert "targets are off" in _refused(tr.set_target_crop_tensor, h, w)                        # targets off
    tr.set_target_crop_tensor(None)                                                              # ... off is always allowed
    tr.set_targets(k)
    assert "shapes" in _refused(tr.set_target_crop_tensor, h, w, axis=True)                      # axis without shapes
    for bad in ((0, 8), (257, 8), (8, 0), (8, 2), (8, 6), (8, 260), (-1, -4)):
        assert "a window is" in _refused(tr.set_target_crop_tensor, *bad)
    assert "mode" in text(setter(ctx, 3, h, w, 1.0, fmt(), out, 2)) and "mode" in text(setter(ctx, -1, h, w, 1.0, fmt(), out, 2))
    for dtype in (-1, 3, 99):
        assert "dtype" in text(setter(ctx, ffi.CROP_UPRIGHT, h, w, 1.0, fmt(dtype=dtype), out, 2))
    assert "reserved" in text(setter(ctx, ffi.CROP_UPRIGHT, h, w, 1.0, fmt(reserved=1), out, 2))
    for zoom in (0.0, 0.0624, 16.001, -1.0, math.nan, math.inf, -math.inf):
        assert "zoom" in text(setter(ctx, ffi.CROP_UPRIGHT, h, w, zoom, fmt(), out, 2)), zoom
    for v in (math.nan, math.inf, -math.inf):
        assert "finite" in text(setter(ctx, ffi.CROP_UPRIGHT, h, w, 1.0, fmt(scale=(1.0, v, 1.0)), out, 2))
        assert "finite" in text(setter(ctx, ffi.CROP_UPRIGHT, h, w, 1.0, fmt(bias=(0.0, 0.0, v)), out, 2))
    assert "null" in text(setter(ctx, ffi.CROP_UPRIGHT, h, w, 1.0, None, out, 2))
    assert "null" in text(setter(ctx, ffi.CROP_UPRIGHT, h, w, 1.0, fmt(), None, 2))
    for off in (1, 4, 8):
        assert "aligned" in text(setter(ctx, ffi.CROP_UPRIGHT, h, w, 1.0, fmt(), C.c_void_p(room.data_ptr() + off), 2))
    for cap in (0, -3):
        assert "at least one" in text(setter(ctx, ffi.CROP_UPRIGHT, h, w, 1.0, fmt(), out, cap))
    tr.bayer("RGGB")                                                                             # RAW8 front end
    assert "Bayer" in _refused(tr.set_target_crop_tensor, h, w)
    tr.bayer(None)
    K = [60.0, 0, cols / 2, 0, 60.0, rows / 2, 0, 0, 1]
    for s in range(n):
        tr.set_undistort(s, K, [0.1, 0.0, 0.0, 0.0, 0.0])
    tr.undistort(True)                                                                           # undistorting front end
    assert "undistortion" in _refused(tr.set_target_crop_tensor, h, w)
    tr.undistort(False)
    assert "off" in _refused(tr.target_crop_tensor)                                              # nothing of all that switched it on
    assert not _host(room).any()
    # the explicit form's own
    wins = [[R.window(True, True, 10, 10)]] * n
    assert "windows a stream" in _refused(tr.crop_tensor_windows, seq.ptr(0), [[R.INVALID] * 9] * n, h, w)
    assert "windows a stream" in _refused(tr.crop_tensor_windows, seq.ptr(0), [[]] * n, h, w)
    assert "a window is" in _refused(tr.crop_tensor_windows, seq.ptr(0), wins, 8, 6)
    assert "null" in _refused(tr.crop_tensor_windows, 0, wins, h, w)
    win1 = (ffi.CropWindow * n)(*[ffi.CropWindow(1, 1, 10.0, 10.0, 0.0, 0.0)] * n)
    explicit = lib.oatgpu_crop_tensor_windows_dev
    assert "dtype" in text(explicit(ctx, C.c_void_p(seq.ptr(0)), win1, 1, h, w, fmt(dtype=7), out))
    assert "reserved" in text(explicit(ctx, C.c_void_p(seq.ptr(0)), win1, 1, h, w, fmt(reserved=-1), out))
    assert "finite" in text(explicit(ctx, C.c_void_p(seq.ptr(0)), win1, 1, h, w, fmt(bias=(math.nan, 0.0, 0.0)), out))
    assert "null" in text(explicit(ctx, C.c_void_p(seq.ptr(0)), win1, 1, h, w, fmt(), None))
    assert "aligned" in text(explicit(ctx, C.c_void_p(seq.ptr(0)), win1, 1, h, w, fmt(), C.c_void_p(room.data_ptr() + 2)))
    assert not _host(room).any()
    # the switch on: what it refuses while it is on
    tr.set_target_crop_tensor(h, w, capacity=2, **_kw(TC.FORMATS[2], 3))
    assert "no call has delivered" in _refused(tr.target_crop_tensor)
    assert "crop tensors" in _refused(tr.bayer, "RGGB")
    assert "crop tensors" in _refused(tr.undistort, True)
    assert "switch them off first" in _refused(tr.set_targets, k)
    assert "switch them off first" in _refused(tr.set_targets, 0)
    tr.set_target_shapes()
    tr.set_target_shapes(False)                                                                  # upright tensors do not need shapes
    tr.set_target_shapes()
    tr.set_target_crop_tensor(h, w, axis=True, zoom=0.5, capacity=2, **_kw(TC.FORMATS[4], 3))
    assert "switch them off first" in _refused(tr.set_target_shapes, False)                      # axis tensors do
    assert "2 entries" in _refused(tr.track_sequence_dev, [seq.ptr(t) for t in range(3)])
    # steps behind all of that match
    for t in range(2):
        tr.track(seq.host[t])
        _same(_host(tr.target_crop_tensor())[0], TC.expected(TC.entry_u8(family, rows, cols, n, t, alpha, k, True, 0.5, h, w), TC.FORMATS[4], 3), t)
    tr.track_sequence_dev([seq.ptr(2), seq.ptr(3)])
    for i in range(2):
        _same(_host(tr.target_crop_tensor())[i], TC.expected(TC.entry_u8(family, rows, cols, n, 2 + i, alpha, k, True, 0.5, h, w), TC.FORMATS[4], 3), 2 + i)
    tr.set_target_crop_tensor(None)
    assert "off" in _refused(tr.target_crop_tensor)
    tr.set_target_shapes(False)
    tr.set_targets(0)                                                                            # ... allowed again with the switch off
    tr.close()


def test_results_outstanding_and_calls_that_deliver_no_tensor(A):
    """The fused tracker's own calls deliver none and behave as with the switch off; its outstanding results refuse the switch and the
    explicit form, which is how it reaches tensors."""
    import shapes_cases as S
    rows, cols, n, k, h, w = 48, 64, 2, 4, 8, 8
    mk = lambda: A.HotPath(rows, cols, n_streams=n, adaptation_coeff=T.FUSED_LR, erode=T.FUSED_MORPH[0], dilate=T.FUSED_MORPH[1],     # noqa: E731
                           area=T.AREA, ring_depth=4, **T.FUSED_WIN)
    hp, plain = mk(), mk()
    f = [[S.frames_of("fused", rows, cols, S.variant_of(s))[t] for s in range(n)] for t in range(6)]
    for x in (hp, plain):
        x.set_targets(k)
    hp.enqueue(f[0])
    plain.enqueue(f[0])
    assert "outstanding" in _refused(hp.set_target_crop_tensor, h, w)
    keep, ptr = _dev(f[0])
    wins = [[R.window(True, False, 30.5, 20.5, 2.0, 0.0)]] * n
    assert "outstanding" in _refused(hp.crop_tensor_windows, ptr, wins, h, w)
    assert hp.collect() == plain.collect()
    hp.stage(0, f[1][0])                                                        # a frame set partly staged
    _refused(hp.set_target_crop_tensor, h, w)
    hp.stage_abort()
    tensor = hp.set_target_crop_tensor(h, w, capacity=3)
    for t in range(1, 6):
        assert hp.track(f[t]) == plain.track(f[t]), t
        assert hp.targets() == plain.targets(), t
        assert "no call has delivered" in _refused(hp.target_crop_tensor)
    assert not _host(tensor).any()
    got = _host(hp.crop_tensor_windows(ptr, wins, h, w, **_kw(TC.FORMATS[3], 3)))
    _same(got, TC.expected(R.crop_set(f[0], wins, h, w), TC.FORMATS[3], 3), "hotpath")
    hp.close()
    plain.close()


def test_steps_with_the_switch_on_off_and_other_calls_in_turn(A):
    family, alpha, rows, cols, n, k = "motion", 0.0, 37, 61, 3, 4
    tr, plain = _make_tracker(A, family, rows, cols, n), _make_tracker(A, family, rows, cols, n)
    seq = _Sequence(family, rows, cols, n)
    for x in (tr, plain):
        x.set_targets(k)
        x.set_target_shapes()
    F = TC.FORMATS
    # (h, w, axis, zoom, format) of the tensor, (h, w, axis) of target crops beside it
    modes = [(None, None), ((16, 12, False, 1.0, F[0]), None), ((16, 12, True, 2.0, F[3]), (8, 8, False)), (None, (16, 12, True)),
             ((5, 4, True, 0.5, F[2]), (5, 4, True)), ((33, 64, False, 1.37, F[1]), None), ((8, 8, True, 1.0, F[4]), (33, 64, False)),
             ((8, 8, False, 1.0, F[0]), (8, 8, False)), (None, None), ((64, 128, True, 2.0, F[6]), None)]
    pat = [CC.pattern(rows, cols, 3, s) for s in range(n)]
    keep, ptr = _dev(pat, 1)
    wins = [CC.groups(TC.explicit_windows(rows, cols, 8, 8)[1])[s] for s in range(n)]
    for t, (tensor, crops) in enumerate(modes):
        if tensor is None:
            tr.set_target_crop_tensor(None)
        else:
            h, w, axis, zoom, fmt = tensor
            tr.set_target_crop_tensor(h, w, axis=axis, zoom=zoom, capacity=1 + t % 2, **_kw(fmt, 3))
        if crops is None:
            tr.set_target_crops(None)
        else:
            tr.set_target_crops(crops[0], crops[1], axis=crops[2])
        if t % 3 == 1:                                                          # other calls of the context in between
            _same(tr.crop_windows(ptr, wins, 8, 8), R.crop_set(pat, wins, 8, 8), t)
            _same(_host(tr.crop_tensor_windows(ptr, wins, 8, 8, **_kw(F[5], 3))), TC.expected(R.crop_set(pat, wins, 8, 8), F[5], 3), t)
        pos = tr.track(seq.host[t]) if t % 2 else tr.track_dev(seq.ptr(t))
        assert pos == (plain.track(seq.host[t]) if t % 2 else plain.track_dev(seq.ptr(t))), t
        assert tr.targets() == plain.targets() and tr.target_shapes() == plain.target_shapes(), t

        def check():
            if tensor is None:
                assert "off" in _refused(tr.target_crop_tensor)
            else:
                want = TC.expected(TC.entry_u8(family, rows, cols, n, t, alpha, k, axis, zoom, h, w), fmt, 3)
                _same(_host(tr.target_crop_tensor())[0], want, (t, "tensor"))
            if crops is None:
                assert "off" in _refused(tr.target_crops)
            else:
                for s in range(n):
                    _same(tr.target_crops()[0][s], CC.sequence_crops(family, rows, cols, CC.variant_of(s), alpha, k, crops[2], crops[0], crops[1])[t],
                          (t, s, "crops"))
        check()
        if t % 3 == 2:
            tr.read_mask(MORPH, 1)
            _same(_host(tr.crop_tensor_windows(ptr, wins, 8, 8, dtype="uint8")), R.crop_set(pat, wins, 8, 8), t)
            check()                                                             # the stand-alone call touches nothing a switch owns
    tr.close()
    plain.close()
