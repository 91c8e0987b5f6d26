"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through
the C ABI (oat_amd -> liboatgpu.so), against the CPU oracle on the same inputs.

Bar: bit-exact for every byte/integer result (masks, HSV, model counters, Green
sums) AND for the fp32 MOG2 model (same operation order, no FMA contraction);
centroids within 1e-4 px (BASELINE.json north_star) -- they are expected to be
identical because both sides finish the same exact int64 sums in double.
"""
import json
import os

import numpy as np
import pytest

import oracle_lib as O
from parity_asserts import CENTROID_TOL, _eq, _same_detection, _same_state  # noqa: F401  (other test modules import them from here)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    import oat_amd
    return oat_amd


# ------------------------------------------------------------------ colour --

def test_bgr2hsv_exhaustive_256cubed(A):
    """All 16.7M colours (computed, not stored)."""
    n = 4096
    idx = np.arange(n * n, dtype=np.uint32)
    bgr = np.stack([(idx & 255), (idx >> 8) & 255, (idx >> 16) & 255], -1).astype(np.uint8).reshape(n, n, 3)
    got = A.ColorConvert(n, n).filter(bgr)
    assert (got == O.bgr2hsv(bgr)).all()


def test_bgr2hsv_known_answers(A, golden_dir):
    g = json.load(open(os.path.join(golden_dir, "hsv_kat.json")))
    bgr = np.zeros((1, 64, 3), np.uint8)
    bgr[0, :len(g["bgr"])] = g["bgr"]
    got = A.ColorConvert(1, 64).filter(bgr)
    assert got[0, :len(g["bgr"])].tolist() == g["hsv"]


def test_cvt_color_exhaustive_256cubed(A):
    """`framefilt col` beyond HSV (oat::color_conv_table, Color.h:45-51): BGR -> GREY and HSV -> BGR over all
    16.7M inputs (hues beyond 179 included), GREY -> BGR over a full frame."""
    n = 4096
    idx = np.arange(n * n, dtype=np.uint32)
    px = np.stack([(idx & 255), (idx >> 8) & 255, (idx >> 16) & 255], -1).astype(np.uint8).reshape(n, n, 3)
    got = A.ColorConvert(n, n, color="GREY").filter(px)
    assert got.shape == (n, n) and (got == O.bgr2grey(px)).all()
    got = A.ColorConvert(n, n, color="BINARY").filter(px)          # BGR -> BINARY is COLOR_BGR2GRAY as well
    assert (got == O.bgr2grey(px)).all()
    got = A.ColorConvert(n, n, color="BGR", from_color="HSV").filter(px)
    assert (got == O.hsv2bgr(px)).all()
    grey = (idx * 2654435761 >> 13).astype(np.uint8).reshape(n, n)
    got = A.ColorConvert(n, n, color="BGR", from_color="GREY").filter(grey)
    assert got.shape == (n, n, 3) and (got == grey[..., None]).all()


@pytest.mark.parametrize("shape", [(1, 1), (1, 3), (3, 5), (7, 9), (37, 101), (2, 2)])
def test_cvt_color_ragged_sizes_and_known_answers(A, golden_dir, shape):
    """Pixel counts that are not a multiple of the kernel's four-pixel groups; the golden known answers."""
    rows, cols = shape
    rng = np.random.default_rng(rows * 131 + cols)
    bgr = rng.integers(0, 256, (rows, cols, 3)).astype(np.uint8)
    g = json.load(open(os.path.join(golden_dir, "cvt_color_kat.json")))
    k = min(rows * cols, len(g["bgr"]))
    bgr.reshape(-1, 3)[:k] = g["bgr"][:k]
    hsv = rng.integers(0, 256, (rows, cols, 3)).astype(np.uint8)
    hsv.reshape(-1, 3)[:k] = g["hsv"][:k]
    got = A.ColorConvert(rows, cols, color="GREY").filter(bgr)
    assert (got == O.bgr2grey(bgr)).all() and got.reshape(-1)[:k].tolist() == g["grey"][:k]
    got = A.ColorConvert(rows, cols, color="BGR", from_color="HSV").filter(hsv)
    assert (got == O.hsv2bgr(hsv)).all() and got.reshape(-1, 3)[:k].tolist() == g["bgr_of_hsv"][:k]
    grey = bgr[..., 1].copy()
    assert (A.ColorConvert(rows, cols, color="BGR", from_color="BINARY").filter(grey) == grey[..., None]).all()
    assert (A.ColorConvert(rows, cols, color="HSV").filter(bgr) == O.bgr2hsv(bgr)).all()


def test_cvt_color_refusals_carry_the_references_texts(A):
    """ColorConvert.cpp:79-85 ("Nothing to be done ...") and Color.h:92-93 ("... not possible.")."""
    from oat_amd import ffi
    f3, f1 = np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4), np.uint8)
    for src, dst, text in (("BGR", "BGR", "Nothing to be done for BGR to BGR conversion."),
                           ("GREY", "BINARY", "Nothing to be done for GREY to BINARY conversion."),
                           ("HSV", "HSV", "Nothing to be done for HSV to HSV conversion."),
                           ("HSV", "GREY", "Requested color conversion is not possible."),
                           ("GREY", "HSV", "Requested color conversion is not possible.")):
        with pytest.raises(ffi.OatGpuError, match=text):
            A.ColorConvert(4, 4, color=dst, from_color=src).filter(f3 if src in ("BGR", "HSV") else f1)


def test_grey_chain_from_bgr_frames(A):
    """BGR camera -> framefilt col -C GREY -> framefilt mog -> posidet thresh (what SimpleThreshold.cpp:46 asks
    for in front of it), stage by stage through the C ABI, against the oracle chain."""
    from oat_amd.synth import SyntheticStream
    rows, cols = 120, 200
    st = SyntheticStream(rows, cols, 11, n_discs=1, radius=12)
    col = A.ColorConvert(rows, cols, color="GREY")
    hp = A.HotPath(rows, cols, n_streams=1, channels=1, adaptation_coeff=0.01, h_thresh=(30, 110), erode=3, dilate=7,
                   area=(20.0, 1e5))
    p = O.hsv_params(h_lo=30, h_hi=110, erode=3, dilate=7, min_area=20.0, max_area=1e5)
    orc = O.Mog2(rows, cols, 1)
    hits = 0
    for t in range(20):
        f = st.frame(t, with_discs=t > 0)
        grey = col.filter(f)
        assert (grey == O.bgr2grey(f)).all()
        got = hp.track([grey])[0]
        want, thr = O.chain_step(orc, grey, 0.01, p)
        assert (hp.read_mask(1, 0) == thr).all(), t
        _same_detection(got, want, t)
        hits += got.position_valid
    assert hits >= 15


# --------------------------------------------------------------------- MOG2 --

@pytest.mark.parametrize("shape", [(48, 64), (37, 101), (5, 3), (1, 1), (33, 256)])
@pytest.mark.parametrize("rate", [0.0, 0.01, 0.3])
@pytest.mark.parametrize("restore", [1, 0])
def test_mog2_mask_and_model_parity(A, shape, rate, restore):
    """restore = 1: MOG2Invoker's `nmodes = nNewModes;` (the default); 0: pruning shrinks the mode count
    (oracle/mog2.c "Mode count").  Masks and the full fp32 model, both readings."""
    rows, cols = shape
    rng = np.random.default_rng(rows * 1000 + cols + int(rate * 100))
    g = A.BackgroundSubtractorMOG(rows, cols, adaptation_coeff=rate, mog_restore_nmodes=restore)
    o = O.Mog2(rows, cols, 3, params=dict(restore_nmodes=restore))
    base = rng.integers(0, 256, (rows, cols, 3)).astype(np.int16)
    alt = rng.integers(0, 256, (rows, cols, 3)).astype(np.int16)
    for t in range(120):
        sel = rng.random((rows, cols, 1)) < 0.25
        f = np.where(sel, alt, base) + rng.integers(-12, 13, (rows, cols, 3))
        if t % 17 == 3:
            f[:] = rng.integers(0, 256, (rows, cols, 3))
        if t % 23 == 5:
            f[rows // 2:] = 0
        f = np.clip(f, 0, 255).astype(np.uint8)
        mg = g.apply(f)
        mo = o.apply(f, rate)
        assert (mg == mo).all(), (shape, rate, t, int((mg != mo).sum()))
        if t % 20 == 19 or t < 3:
            _same_state(g.mog_state(), o.state(), (shape, rate, t))


def test_mog2_nan_variance_of_a_rematched_pruned_slot(A):
    """k = alphaT / weight = 0 / 0: a pruned slot (weight 0, kept by `nmodes = nNewModes;`) matched again at learning rate 0.
    OpenCV's MAX / MIN macros keep the NaN variance (a comparison with a NaN is false) -- v_maximum3_f32 / v_minimum3_f32 in
    the kernel, the macro's comparisons in the oracle (rounds 1-4 clamped it to varMin on both sides).
    Stage-by-stage call and the fused pipelined path (one and two frames a launch), masks and the whole model."""
    rows, cols = 8, 64
    a = np.full((rows, cols, 3), 40, np.uint8)
    b = np.full((rows, cols, 3), 200, np.uint8)
    seq = [(a, 0.3)] * 3 + [(b, 0.3)] + [(a, 0.3)] * 40 + [(b, 0.0)] * 3 + [(a, 0.0), (b, 0.0), (a, 0.01), (b, 0.01)] * 3
    g = A.BackgroundSubtractorMOG(rows, cols)
    o = O.Mog2(rows, cols, 3)
    for t, (f, rate) in enumerate(seq):
        assert (g.apply(f, learning_rate=rate) == o.apply(f, rate)).all(), t
        if t == 46:
            nm, w, v, m = o.state()
            assert nm[0] == 2 and w[0, 1] == 0.0 and np.isnan(v[0, 1]) and np.isnan(m[0, 1]).all()      # the case IS reached
            gv = g.mog_state()[2]
            assert np.isnan(gv[:, 1]).all()
        _same_state(g.mog_state(), o.state(), t)
    for fusion in (1, 2):
        hp = A.HotPath(rows, cols, n_streams=1, ring_depth=4, v_thresh=(100, 256), erode=0, dilate=0, area=(0.5, 1e9))
        hp.set_fusion(fusion)
        o = O.Mog2(rows, cols, 3)
        for t, (f, rate) in enumerate(seq):
            hp.learning_coeff_ = rate
            hp.enqueue([f])
            o.apply(f, rate)
            if hp.outstanding() == 3:
                hp.collect()
        while hp.outstanding():
            hp.collect()
        _same_state(hp.mog_state(), o.state(), ("fused", fusion))
        assert np.isnan(hp.mog_state()[2]).any(1).all()          # (the NaN slot has moved down the list by now: later modes overtook it)
        hp.close()


def test_mog2_single_pixel_traces(A, golden_dir):
    """The hand-independent float32 traces of tests/golden/mog2_trace.json, on the GPU."""
    for tr in json.load(open(os.path.join(golden_dir, "mog2_trace.json"))):
        g = A.BackgroundSubtractorMOG(1, 1, mog_restore_nmodes=tr.get("restore", 1))
        for t, (px, want) in enumerate(zip(tr["pixels"], tr["frames"])):
            mask = g.apply(np.array(px, np.uint8).reshape(1, 1, 3), learning_rate=tr["rate"])
            nm, w, v, mu, _ = g.mog_state()
            k = want["nmodes"]
            assert int(mask[0, 0]) == want["mask"], (tr["name"], t)
            assert int(nm[0]) == k, (tr["name"], t)
            assert w[0, :k].tolist() == [np.float32(x) for x in want["weight"]], (tr["name"], t)
            assert v[0, :k].tolist() == [np.float32(x) for x in want["variance"]], (tr["name"], t)
            assert mu[0, :k].tolist() == [[np.float32(c) for c in r] for r in want["mean"]], (tr["name"], t)


def test_mog_filter_frame1_and_frozen_model(A):
    """BackgroundSubtractorMOG::filter with Oat's default -a 0."""
    rng = np.random.default_rng(3)
    rows, cols = 40, 70
    f1 = rng.integers(1, 256, (rows, cols, 3), dtype=np.uint8)
    f1[0, 0] = 0
    g = A.BackgroundSubtractorMOG(rows, cols, adaptation_coeff=0.0)
    o = O.Mog2(rows, cols, 3)
    out = g.filter(f1.copy())
    assert (out == f1).all()                       # first output frame is the unmodified input
    o.filter(f1, 0.0)
    for t in range(5):
        f = np.clip(f1.astype(int) + rng.integers(-14, 15, f1.shape), 0, 255).astype(np.uint8)
        want, _ = o.filter(f, 0.0)
        got = g.filter(f.copy())
        assert (got == want).all()
    _same_state(g.mog_state(), o.state())


def test_mog_state_roundtrip_and_resume(A):
    rng = np.random.default_rng(5)
    rows, cols = 30, 90
    a = A.BackgroundSubtractorMOG(rows, cols, adaptation_coeff=0.02)
    frames = [rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8) for _ in range(12)]
    for f in frames[:6]:
        a.apply(f)
    nm, w, v, m, nf = a.mog_state()
    b = A.BackgroundSubtractorMOG(rows, cols, adaptation_coeff=0.02)
    live = np.arange(w.shape[1])[None, :] < nm[:, None]
    w = np.where(live, w, 0); v = np.where(live, v, 0); m = np.where(live[..., None], m, 0)
    b.set_mog_state(nm, w, v, m, nf)
    for f in frames[6:]:
        assert (a.apply(f) == b.apply(f)).all()


@pytest.mark.parametrize("channels", [3, 1])
def test_mog_checkpoint_file_resumes_bit_identically(A, tmp_path, channels):
    """oatgpu_mog_save / _load: a run resumed from the file equals the uninterrupted run AND the
    oracle (masks and full model); equal models give byte-identical files; mismatching or damaged
    files are refused."""
    rng = np.random.default_rng(15)
    rows, cols, n = 37, 101, 2
    shape = (n, rows, cols, 3) if channels == 3 else (n, rows, cols)
    frames = [np.clip(100 + rng.normal(0, 12, shape), 0, 255).astype(np.uint8) for _ in range(14)]
    kw = dict(n_streams=n, channels=channels, adaptation_coeff=0.03, dilate=0)
    if channels == 1:
        kw.update(h_thresh=(1, 256))
    a = A.HotPath(rows, cols, **kw)
    o = [O.Mog2(rows, cols, channels=channels) for _ in range(n)]
    for f in frames[:8]:
        a.track(list(f))
        for s in range(n):
            o[s].apply(f[s], 0.03)
    files = [str(tmp_path / f"s{s}.mog") for s in range(n)]
    for s in range(n):
        a.save_mog_state(files[s], stream=s)
    a.save_mog_state(str(tmp_path / "again.mog"), stream=0)
    assert open(files[0], "rb").read() == open(tmp_path / "again.mog", "rb").read()
    assert os.path.getsize(files[0]) == 64 + rows * cols * (1 + 4 * 5 * (2 + channels))

    b = A.HotPath(rows, cols, **kw)
    for s in range(n):
        b.load_mog_state(files[s], stream=s)
    for f in frames[8:]:
        ra, rb = a.track(list(f)), b.track(list(f))
        for s in range(n):
            o[s].apply(f[s], 0.03)
            assert ra[s] == rb[s]
            assert (a.read_mask(0, stream=s) == b.read_mask(0, stream=s)).all()
    for s in range(n):
        nm, w, v, m, nf = b.mog_state(stream=s)
        onm, ow, ov, om = o[s].state()
        live = np.arange(5)[None, :] < nm[:, None]
        assert nf == 14 and (nm == onm.ravel()).all()
        assert (w[live] == ow.reshape(-1, 5)[live]).all() and (v[live] == ov.reshape(-1, 5)[live]).all()
        assert (m[live] == om.reshape(-1, 5, channels)[live]).all()

    with pytest.raises(A.OatGpuError, match="is 37x101"):
        A.HotPath(rows, cols + 1, **kw).load_mog_state(files[0])
    with pytest.raises(A.OatGpuError, match="with 5 mixtures"):
        A.HotPath(rows, cols, nmixtures=3, **kw).load_mog_state(files[0])
    blob = open(files[0], "rb").read()
    (tmp_path / "short.mog").write_bytes(blob[:-5])
    with pytest.raises(A.OatGpuError):
        b.load_mog_state(str(tmp_path / "short.mog"))
    (tmp_path / "junk.mog").write_bytes(b"not a checkpoint" * 10)
    with pytest.raises(A.OatGpuError, match="not a MOG2 model checkpoint"):
        b.load_mog_state(str(tmp_path / "junk.mog"))
    with pytest.raises(A.OatGpuError):
        b.load_mog_state(str(tmp_path / "missing.mog"))


# --------------------------------------------------------------- morphology --

@pytest.mark.parametrize("shape", [(40, 64), (35, 130), (9, 7), (64, 200)])
def test_erode_dilate_parity(A, shape):
    rows, cols = shape
    rng = np.random.default_rng(rows + cols)
    for e, d in [(0, 0), (0, 10), (3, 7), (7, 7), (2, 2), (13, 1), (1, 13), (5, 0), (10, 3)]:
        img = (rng.random((rows, cols)) < rng.uniform(0.3, 0.97)).astype(np.uint8) * 255
        det = A.SimpleThreshold(rows, cols, thresh=(1, 256), erode=e, dilate=d)
        det.detectPosition(img)
        want = img
        if e:
            want = O.erode(want, e)
        if d:
            want = O.dilate(want, d)
        got = det.read_mask(1)
        assert (got == want).all(), (shape, e, d)


def test_morph_impulses_golden(A, golden_dir):
    for c in json.load(open(os.path.join(golden_dir, "morph_impulse.json"))):
        img = np.zeros((c["rows"], c["cols"]), np.uint8)
        img[c["y0"], c["x0"]] = 255
        want = np.zeros_like(img)
        want[c["y_lo"]:c["y_hi"] + 1, c["x_lo"]:c["x_hi"] + 1] = 255
        det = A.SimpleThreshold(c["rows"], c["cols"], thresh=(1, 256), erode=0, dilate=c["k"])
        det.detectPosition(img)
        assert (det.read_mask(1) == want).all(), c
        det = A.SimpleThreshold(c["rows"], c["cols"], thresh=(1, 256), erode=c["k"], dilate=0)
        det.detectPosition(255 - img)
        assert (det.read_mask(1) == 255 - want).all(), c


# ------------------------------------------------------------ blob analysis --

def test_contour_known_answers(A, golden_dir):
    for c in json.load(open(os.path.join(golden_dir, "contours.json"))):
        img = np.array(c["img"], np.uint8) * 255
        det = A.SimpleThreshold(img.shape[0], img.shape[1], thresh=(1, 256),
                                area=(c.get("min_area", 0.0), c.get("max_area", float(np.finfo(np.float64).max))))
        p = det.detectPosition(img)
        assert p.position_valid == c["valid"], (c["name"], p)
        assert p.area == c["area"], (c["name"], p)
        if c["valid"]:
            assert p.x == c["x"] and p.y == c["y"], (c["name"], p)


def _blob_images(n, seed, max_hw=90):
    rng = np.random.default_rng(seed)
    for it in range(n):
        h, w = int(rng.integers(1, max_hw)), int(rng.integers(1, max_hw * 2))
        img = (rng.random((h, w)) < rng.uniform(0.15, 0.9)).astype(np.uint8) * 255
        if it % 3 == 0 and h > 3 and w > 3:
            img = O.dilate(img, int(rng.integers(2, 5)))
        if it % 5 == 0:
            img = O.erode(img, 2)
        if it % 7 == 0 and h > 8 and w > 8:
            img[:] = 0
            step = int(rng.integers(2, 4))
            for k in range(0, min(h, w) // 2 - 1, step):
                img[k + 1:h - k - 1, k + 1:w - k - 1] = 255 if (k // step) % 2 == 0 else 0
            img ^= ((rng.random((h, w)) < 0.04) * 255).astype(np.uint8)
        yield img, rng


def test_blob_parity_random_images(A):
    """Noise, dilated noise, nested rings: sequential OpenCV-3.1 border following
    (oracle) vs the run-based union-find + crack sums on the GPU."""
    cache = {}
    for img, rng in _blob_images(400, 21):
        lo = float(rng.choice([0.0, 0.0, 2.0, 10.0]))
        hi = float(rng.choice([np.finfo(np.float64).max, 60.0, 400.0]))
        key = img.shape
        if key not in cache:
            cache[key] = A.SimpleThreshold(img.shape[0], img.shape[1], thresh=(1, 256))
        det = cache[key]
        det._set(min_area=lo, max_area=hi)
        got = det.detectPosition(img)
        want = O.sift_contours(img, lo, hi)
        _same_detection(got, want, (img.shape, lo, hi))
        if len(cache) > 64:
            cache.clear()


@pytest.mark.parametrize("shape", [(480, 640), (300, 1000), (1080, 1920)])
def test_blob_parity_large_noise(A, shape):
    """Union-find stress: ~50% noise gives hundreds of thousands of runs and deep merges."""
    rows, cols = shape
    rng = np.random.default_rng(rows)
    det = A.SimpleThreshold(rows, cols, thresh=(1, 256))
    for dens, dil in [(0.5, 0), (0.42, 0), (0.6, 2), (0.08, 9), (0.995, 0)]:
        img = (rng.random((rows, cols)) < dens).astype(np.uint8) * 255
        det._set(dilate=dil)
        got = det.detectPosition(img)
        thr = O.dilate(img, dil) if dil else img
        assert (det.read_mask(1) == thr).all()
        _same_detection(got, O.sift_contours(thr), (shape, dens, dil))


def test_all_pass_default_is_one_full_frame_contour(A):
    """posidet hsv defaults (HSVDetector.h:86-94): everything passes, dilate 10."""
    rows, cols = 120, 200
    hsv = np.random.default_rng(0).integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    det = A.HSVDetector(rows, cols)
    got = det.detectPosition(hsv)
    want, thr = O.detect_hsv(hsv, O.hsv_params())
    _same_detection(got, want)
    assert got.area == (rows - 3) * (cols - 3)      # frame ring zeroed: (W-2) x (H-2) pixels
    assert (det.read_mask(1) == thr).all()


def test_detect_hsv_parity(A):
    rng = np.random.default_rng(8)
    rows, cols = 96, 160
    for it in range(25):
        hsv = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
        # a few coherent blobs so that windows select something
        for _ in range(4):
            y, x = int(rng.integers(0, rows - 20)), int(rng.integers(0, cols - 30))
            hsv[y:y + int(rng.integers(3, 20)), x:x + int(rng.integers(3, 30))] = (int(rng.integers(90, 120)), 220, 200)
        h = sorted(rng.integers(0, 257, 2).tolist()) if it % 4 else [90, 125]
        s = sorted(rng.integers(0, 257, 2).tolist()) if it % 3 else [0, 256]
        v = sorted(rng.integers(0, 257, 2).tolist()) if it % 5 else [1, 256]
        e, d = int(rng.integers(0, 6)), int(rng.integers(0, 12))
        area = (float(rng.choice([0, 5, 20])), float(rng.choice([1e5, 300.0])))
        det = A.HSVDetector(rows, cols, h_thresh=h, s_thresh=s, v_thresh=v, erode=e, dilate=d, area=area)
        got = det.detectPosition(hsv)
        p = O.hsv_params(h_lo=h[0], h_hi=h[1], s_lo=s[0], s_hi=s[1], v_lo=v[0], v_hi=v[1], erode=e, dilate=d,
                         min_area=area[0], max_area=area[1])
        want, thr = O.detect_hsv(hsv, p)
        assert (det.read_mask(1) == thr).all(), it
        _same_detection(got, want, it)


def test_position_keeps_stale_xy_when_nothing_found(A):
    """siftContours leaves position.x/y untouched when no contour qualifies (DetectorFunc.cpp:46-62)."""
    det = A.SimpleThreshold(20, 20, thresh=(1, 256))
    img = np.zeros((20, 20), np.uint8); img[5:9, 5:9] = 255
    pos = det.detectPosition(img)
    assert pos.position_valid and (pos.x, pos.y) == (6.5, 6.5)
    pos = det.detectPosition(np.zeros((20, 20), np.uint8), pos)
    assert not pos.position_valid and (pos.x, pos.y) == (6.5, 6.5) and pos.area == 0.0


# -------------------------------------------------------------- fused chain --

def _chain_oracles(rows, cols, n):
    return [O.Mog2(rows, cols, 3) for _ in range(n)]


@pytest.mark.parametrize("rate", [0.0, 0.01])
def test_hot_path_chain_parity_640x480(A, rate):
    """BASELINE config 1 shape, 3 batched streams, 60 frames: threshold masks pixel-exact,
    positions identical to the reference CPU chain (oracle)."""
    from oat_amd.synth import SyntheticStream, disc_hsv_window
    rows, cols, n = 480, 640, 3
    win = disc_hsv_window()
    hp = A.HotPath(rows, cols, n_streams=n, adaptation_coeff=rate, erode=3, dilate=7, area=(20.0, 1e5), **win)
    p = O.hsv_params(h_lo=win["h_thresh"][0], h_hi=win["h_thresh"][1], s_lo=win["s_thresh"][0],
                     s_hi=win["s_thresh"][1], v_lo=win["v_thresh"][0], v_hi=win["v_thresh"][1],
                     erode=3, dilate=7, min_area=20.0, max_area=1e5)
    streams = [SyntheticStream(rows, cols, s, n_discs=1 + s % 3) for s in range(n)]
    oracles = _chain_oracles(rows, cols, n)
    found = 0
    for t in range(60):
        frames = [st.frame(t, with_discs=(t > 0)) for st in streams]
        got = hp.track(frames)
        for s in range(n):
            want, thr = O.chain_step(oracles[s], frames[s], rate, p)
            if t % 10 == 0 or t < 3:
                assert (hp.read_mask(1, s) == thr).all(), (t, s)
            _same_detection(got[s], want, (t, s))
            found += got[s].position_valid
    assert found > 100          # the discs really are tracked
    for s in range(n):
        _same_state(hp.mog_state(s), oracles[s].state(), s)


@pytest.mark.parametrize("shape,frames", [((1080, 1920), 4), ((2160, 3840), 3)])
def test_hot_path_full_size_parity(A, shape, frames):
    """BASELINE configs 2 and 5 shapes against the oracle directly (a few frames each)."""
    from oat_amd.synth import SyntheticStream, disc_hsv_window
    rows, cols = shape
    win = disc_hsv_window()
    hp = A.HotPath(rows, cols, n_streams=1, adaptation_coeff=0.01, erode=7, dilate=7, area=(20.0, 1e5), **win)
    p = O.hsv_params(h_lo=100, h_hi=125, s_lo=150, s_hi=256, v_lo=100, v_hi=256, erode=7, dilate=7,
                     min_area=20.0, max_area=1e5)
    st = SyntheticStream(rows, cols, 0, n_discs=2)
    orc = O.Mog2(rows, cols, 3)
    for t in range(frames):
        f = st.frame(t, with_discs=(t > 0))
        got = hp.track([f])[0]
        want, thr = O.chain_step(orc, f, 0.01, p, nthreads=8)
        assert (hp.read_mask(1) == thr).all(), t
        _same_detection(got, want, t)
    _same_state(hp.mog_state(), orc.state())


def test_hot_path_size_independent_properties(A):
    """4K properties that need no oracle: (i) with a frozen model the same frame gives the
    same answer twice (idempotence); (ii) translating the blob by (dx,dy) translates the
    centroid by exactly (dx,dy) and keeps the area (linearity of the Green sums)."""
    rows, cols = 2160, 3840
    hp = A.HotPath(rows, cols, n_streams=1, adaptation_coeff=0.0, erode=3, dilate=7, area=(20.0, 1e6),
                   h_thresh=(100, 125), s_thresh=(150, 256), v_thresh=(100, 256))
    bg = np.full((rows, cols, 3), 120, np.uint8)
    hp.track([bg])                                   # frame 1 learns the background

    def with_blob(x0, y0):
        f = bg.copy()
        yy, xx = np.mgrid[0:81, 0:121]
        m = ((xx - 60) / 60.0) ** 2 + ((yy - 40) / 40.0) ** 2 <= 1.0
        f[y0:y0 + 81, x0:x0 + 121][m] = (255, 64, 0)
        return f
    a1 = hp.track([with_blob(500, 700)])[0]
    a2 = hp.track([with_blob(500, 700)])[0]
    b = hp.track([with_blob(500 + 2613, 700 + 1111)])[0]
    assert a1.position_valid and a1 == a2
    assert b.area == a1.area and b.a00 == a1.a00
    assert abs((b.x - a1.x) - 2613) <= CENTROID_TOL and abs((b.y - a1.y) - 1111) <= CENTROID_TOL


def test_enqueue_collect_order_and_ring_limits(A):
    import torch
    from oat_amd import ffi
    rows, cols, n = 64, 128, 2
    hp = A.HotPath(rows, cols, n_streams=n, ring_depth=3, adaptation_coeff=0.0, dilate=0, erode=0,
                   v_thresh=(200, 256), area=(0.5, 1e9))
    dev = torch.device("cuda:0")

    def frames(k):
        f = np.zeros((n, rows, cols, 3), np.uint8)
        if k:
            f[0, 10:10 + k + 2, 10:14] = 255      # area grows with k
            f[1, 20:24, 30:30 + k + 2] = 255
        return f
    bufs = [torch.from_numpy(frames(k)).to(dev) for k in range(5)]
    torch.cuda.synchronize()
    hp.track_dev(bufs[0].data_ptr())
    for k in (1, 2, 3):
        hp.enqueue_dev(bufs[k].data_ptr())
    with pytest.raises(A.OatGpuError) as ei:
        hp.enqueue_dev(bufs[4].data_ptr())
    assert ei.value.code == ffi.E_RING_FULL
    for k in (1, 2, 3):
        r = hp.collect()
        assert r[0].position_valid and r[0].area == (k + 1) * 3.0
        assert r[1].position_valid and r[1].area == 3.0 * (k + 1)
    with pytest.raises(A.OatGpuError) as ei:
        hp.collect()
    assert ei.value.code == ffi.E_RING_EMPTY


@pytest.mark.parametrize("rate", [0.0, 0.02])
def test_grey_mog2_parity(A, rate):
    """framefilt mog on GREY frames (MOG2's generic-channel path), mask + model."""
    rows, cols = 41, 150
    rng = np.random.default_rng(77)
    g = A.BackgroundSubtractorMOG(rows, cols, adaptation_coeff=rate, channels=1)
    o = O.Mog2(rows, cols, 1)
    base = rng.integers(0, 256, (rows, cols)).astype(np.int16)
    alt = rng.integers(0, 256, (rows, cols)).astype(np.int16)
    for t in range(80):
        f = np.where(rng.random((rows, cols)) < 0.25, alt, base) + rng.integers(-10, 11, (rows, cols))
        if t % 19 == 4:
            f[:] = rng.integers(0, 256, (rows, cols))
        f = np.clip(f, 0, 255).astype(np.uint8)
        assert (g.apply(f) == o.apply(f, rate)).all(), t
        if t % 20 == 19 or t < 2:
            _same_state(g.mog_state(), o.state(), t)
    f = np.clip(base + rng.integers(-30, 31, (rows, cols)), 0, 255).astype(np.uint8)
    want, _ = o.filter(f, rate)
    assert (g.filter(f.copy()) == want).all()


def test_grey_chain_mog_then_thresh(A):
    """frameserve -C GREY -> framefilt mog -> posidet thresh, fused on the GPU vs the oracle chain."""
    rows, cols, n = 200, 320, 2
    rng = np.random.default_rng(9)
    hp = A.HotPath(rows, cols, n_streams=n, channels=1, adaptation_coeff=0.01, h_thresh=(180, 256), erode=2,
                   dilate=5, area=(10.0, 1e5))
    p = O.hsv_params(h_lo=180, h_hi=256, erode=2, dilate=5, min_area=10.0, max_area=1e5)
    orcs = [O.Mog2(rows, cols, 1) for _ in range(n)]
    base = [rng.integers(60, 120, (rows, cols)).astype(np.int16) for _ in range(n)]
    hits = 0
    for t in range(25):
        frames = []
        for s in range(n):
            f = np.clip(base[s] + rng.integers(-5, 6, (rows, cols)), 0, 255).astype(np.uint8)
            if t > 0:
                x, y = 20 + 9 * t + 30 * s, 30 + 5 * t
                f[y:y + 18, x:x + 25] = 230
            frames.append(f)
        got = hp.track(frames)
        for s in range(n):
            want, thr = O.chain_step(orcs[s], frames[s], 0.01, p)
            assert (hp.read_mask(1, s) == thr).all(), (t, s)
            _same_detection(got[s], want, (t, s))
            hits += got[s].position_valid
    assert hits >= 40


@pytest.mark.parametrize("rate", [-1.0, 1.0])
def test_mog2_auto_and_reinit_learning_rates(A, rate):
    """learningRate < 0 -> 1/min(2n, history); learningRate >= 1 -> the model is re-initialised every frame."""
    rows, cols = 24, 70
    rng = np.random.default_rng(31)
    g = A.BackgroundSubtractorMOG(rows, cols)
    o = O.Mog2(rows, cols, 3)
    base = rng.integers(0, 256, (rows, cols, 3)).astype(np.int16)
    for t in range(40):
        f = np.clip(base + rng.integers(-20, 21, base.shape), 0, 255).astype(np.uint8)
        assert (g.apply(f, learning_rate=rate) == o.apply(f, rate)).all(), t
    _same_state(g.mog_state(), o.state())


def test_mog2_non_default_parameters(A):
    """3 mixtures, no shadow detection, tighter thresholds: the parameters are honoured, not baked in."""
    rows, cols = 30, 64
    over = dict(nmixtures=3, detect_shadows=0, var_threshold=10.0, var_threshold_gen=6.0, var_init=20.0,
                var_min=2.0, var_max=60.0, background_ratio=0.8, ct=0.02)
    rng = np.random.default_rng(32)
    g = A.BackgroundSubtractorMOG(rows, cols, adaptation_coeff=0.05, **over)
    o = O.Mog2(rows, cols, 3, params=over)
    cols6 = rng.integers(0, 256, (6, 3))
    for t in range(100):
        idx = rng.integers(0, 6, (rows, cols))
        f = np.clip(cols6[idx] + rng.integers(-8, 9, (rows, cols, 3)), 0, 255).astype(np.uint8)
        mg, mo = g.apply(f), o.apply(f, 0.05)
        assert (mg == mo).all(), t
        assert set(np.unique(mg)) <= {0, 255}              # no shadow value without shadow detection
    _same_state(g.mog_state(), o.state())
    assert o.state()[0].max() == 3


@pytest.mark.parametrize("cols", [4300, 8200])
def test_wide_frame_and_large_kernels(A, cols):
    """W > 4096 (row scan loops over 64-word chunks), W not a multiple of 64, k up to 63.  At 8200
    columns the (5, 63) case exceeds the LDS budget of the fused erosion and takes the two-pass route."""
    rows = 70
    rng = np.random.default_rng(33)
    det = A.SimpleThreshold(rows, cols, thresh=(1, 256))
    for e, d, dens in [(0, 0, 0.5), (5, 63, 0.9), (63, 0, 0.9997), (9, 33, 0.97)]:
        img = (rng.random((rows, cols)) < dens).astype(np.uint8) * 255
        img[20:50, 3900:4250] = 255                          # a blob that crosses the 4096-px chunk boundary
        det._set(erode=e, dilate=d)
        got = det.detectPosition(img)
        thr = img
        if e:
            thr = O.erode(thr, e)
        if d:
            thr = O.dilate(thr, d)
        assert (det.read_mask(1) == thr).all(), (e, d)
        _same_detection(got, O.sift_contours(thr), (e, d))
    with pytest.raises(A.OatGpuError):
        det._set(dilate=64)                                  # documented limit of the bit-packed morphology


def test_batch_with_uneven_stream_histories_and_ring_depth_one(A):
    """Streams whose models are at different frame counts cannot share a launch: results stay per-stream exact."""
    from oat_amd.synth import SyntheticStream, disc_hsv_window
    rows, cols, n = 120, 192, 3
    win = disc_hsv_window()
    hp = A.HotPath(rows, cols, n_streams=n, ring_depth=1, adaptation_coeff=-1.0, erode=0, dilate=5,
                   area=(5.0, 1e5), **win)
    hp.learning_coeff_ = -1.0        # auto rate depends on each stream's own frame count
    p = O.hsv_params(h_lo=100, h_hi=125, s_lo=150, s_hi=256, v_lo=100, v_hi=256, erode=0, dilate=5,
                     min_area=5.0, max_area=1e5)
    streams = [SyntheticStream(rows, cols, 10 + s, n_discs=1, radius=7) for s in range(n)]
    orcs = [O.Mog2(rows, cols, 3) for _ in range(n)]
    # advance stream 1 alone by two frames through the single-stage entry point
    pre = A.ffi.load()
    for t in range(2):
        f = streams[1].frame(t, with_discs=False)
        out = np.empty_like(f)
        hp._chk(pre.oatgpu_mog_filter(hp.ctx, 1, A.ffi.u8(f), A.ffi.u8(out), -1.0))
        want, _ = orcs[1].filter(f, -1.0)
        assert (out == want).all()
    for t in range(12):
        frames = [st.frame(t + 2, with_discs=t > 0) for st in streams]
        got = hp.track(frames)
        for s in range(n):
            want, thr = O.chain_step(orcs[s], frames[s], -1.0, p)
            assert (hp.read_mask(1, s) == thr).all(), (t, s)
            _same_detection(got[s], want, (t, s))
    for s in range(n):
        _same_state(hp.mog_state(s), orcs[s].state(), s)


def test_roi_mask_fused_before_mog(A):
    """`framefilt mask` -> `framefilt mog` -> ... (examples/two-color-test/track.sh:34-38): the ROI mask
    (FrameMasker.cpp:71-75, frame.setTo(0, roi == 0)) fused into the per-pixel kernel, per stream."""
    from oat_amd.synth import SyntheticStream, disc_hsv_window
    rows, cols, n = 150, 200, 2
    win = disc_hsv_window()
    hp = A.HotPath(rows, cols, n_streams=n, adaptation_coeff=0.02, erode=0, dilate=3, area=(3.0, 1e5), **win)
    p = O.hsv_params(h_lo=100, h_hi=125, s_lo=150, s_hi=256, v_lo=100, v_hi=256, erode=0, dilate=3,
                     min_area=3.0, max_area=1e5)
    yy, xx = np.mgrid[0:rows, 0:cols]
    roi = (((xx - 100) ** 2 + (yy - 75) ** 2) < 70 ** 2).astype(np.uint8) * 255     # circular arena
    hp.set_roi_mask(roi, stream=1)                                                  # stream 0 stays unmasked
    streams = [SyntheticStream(rows, cols, 20 + s, n_discs=1, radius=6) for s in range(n)]
    orcs = [O.Mog2(rows, cols, 3) for _ in range(n)]
    for t in range(30):
        frames = [st.frame(t, with_discs=t > 0) for st in streams]
        got = hp.track(frames)
        for s in range(n):
            f = frames[s].copy()
            if s == 1:
                f[roi == 0] = 0
            want, thr = O.chain_step(orcs[s], f, 0.02, p)
            assert (hp.read_mask(1, s) == thr).all(), (t, s)
            _same_detection(got[s], want, (t, s))
    hp.set_roi_mask(None, stream=1)
    frames = [st.frame(31) for st in streams]
    got = hp.track(frames)
    want, _ = O.chain_step(orcs[1], frames[1], 0.02, p)
    _same_detection(got[1], want)


@pytest.mark.parametrize("blur", [0, 2, 5, 22])
def test_posidet_diff_parity(A, blur):
    """posidet diff (DifferenceDetector.cpp:98-173): absdiff -> threshold -> blur -> siftContours, stateful."""
    rows, cols, n = 90, 200, 2
    rng = np.random.default_rng(40 + blur)
    det = A.DifferenceDetector(rows, cols, diff_threshold=12, blur=blur, area=(2.0, 1e6), n_streams=n)
    orcs = [O.Diff(rows, cols, 12, blur, 2.0, 1e6) for _ in range(n)]
    base = [rng.integers(40, 90, (rows, cols)).astype(np.int16) for _ in range(n)]
    hits = 0
    for t in range(20):
        for s in range(n):
            f = np.clip(base[s] + rng.integers(-4, 5, (rows, cols)), 0, 255).astype(np.uint8)
            x, y = 10 + 8 * t + 20 * s, 15 + 3 * t
            f[y:y + 12, x:x + 20] = 220
            if t % 7 == 3:
                f[0:3, :] = 255; f[:, 0:2] = 255          # activity on the image border (reflect-101 ring)
            got = det.detectPosition(f, stream=s)
            want, thr = orcs[s].detect(f)
            if t > 0:
                assert ((det.read_mask(1, s) > 0)[1:-1, 1:-1] == (thr > 0)[1:-1, 1:-1]).all(), (t, s)
            _same_detection(got, want, (t, s))
            hits += got.position_valid
    assert hits >= 30
    with pytest.raises(A.OatGpuError):
        A.DifferenceDetector(rows, cols, blur=23)


@pytest.mark.parametrize("alpha,channels", [(0.0, 3), (0.05, 3), (0.3, 1), (1.0, 3)])
def test_framefilt_bsub_parity(A, alpha, channels):
    """framefilt bsub (BackgroundSubtractor.cpp:87-100): fp32 accumulateWeighted + saturating subtract."""
    rows, cols = 37, 90
    rng = np.random.default_rng(int(alpha * 100) + channels)
    shape = (rows, cols, 3) if channels == 3 else (rows, cols)
    g = A.BackgroundSubtractor(rows, cols, adaptation_coeff=alpha, channels=channels)
    o = O.Bsub(rows, cols, channels, alpha)
    base = rng.integers(0, 256, shape).astype(np.int16)
    for t in range(40):
        f = np.clip(base + rng.integers(-40, 41, shape) + (3 * t if t % 2 else 0), 0, 255).astype(np.uint8)
        assert (g.filter(f) == o.filter(f)).all(), t


def test_framefilt_thresh_parity(A):
    """framefilt thresh (Threshold.cpp:67-81): BGR->grey (all 16.7M colours), inRange, setTo(0)."""
    n = 4096
    idx = np.arange(n * n, dtype=np.uint32)
    bgr = np.stack([(idx & 255), (idx >> 8) & 255, (idx >> 16) & 255], -1).astype(np.uint8).reshape(n, n, 3)
    for lo, hi in [(0, 256), (100, 180), (200, 100), (256, 256)]:
        got = A.Threshold(n, n, intensity=(lo, hi)).filter(bgr)
        assert (got == O.thresh_filter(bgr, lo, hi)).all(), (lo, hi)
    grey = np.random.default_rng(1).integers(0, 256, (50, 70), dtype=np.uint8)
    assert (A.Threshold(50, 70, intensity=(90, 160), channels=1).filter(grey) == O.thresh_filter(grey, 90, 160)).all()
    with pytest.raises(A.OatGpuError):
        A.Threshold(8, 8, intensity=(0, 300)).filter(np.zeros((8, 8, 3), np.uint8))      # Threshold.cpp:62-63


def test_hot_path_random_configurations(A):
    """Fuzz: random frame shapes, stream counts, learning rates, HSV windows, morphology sizes and area
    windows through the fused chain, every frame checked against the oracle chain."""
    from oat_amd.synth import SyntheticStream
    rng = np.random.default_rng(2026)
    for case in range(14):
        rows, cols = int(rng.integers(20, 140)), int(rng.integers(20, 260))
        n = int(rng.integers(1, 4))
        rate = float(rng.choice([0.0, 0.005, 0.05, 0.5, -1.0]))
        e, d = int(rng.choice([0, 0, 2, 3, 5])), int(rng.choice([0, 3, 7, 10, 16]))
        h = sorted(rng.integers(0, 257, 2).tolist()) if case % 3 else [100, 125]
        s_ = sorted(rng.integers(0, 257, 2).tolist()) if case % 4 == 0 else [0, 256]
        v = [int(rng.integers(0, 120)), 256]
        area = (float(rng.choice([0.0, 3.0, 30.0])), float(rng.choice([1e9, 500.0])))
        hp = A.HotPath(rows, cols, n_streams=n, adaptation_coeff=rate, h_thresh=h, s_thresh=s_, v_thresh=v,
                       erode=e, dilate=d, area=area, ring_depth=int(rng.integers(1, 6)))
        hp.learning_coeff_ = rate
        p = O.hsv_params(h_lo=h[0], h_hi=h[1], s_lo=s_[0], s_hi=s_[1], v_lo=v[0], v_hi=v[1], erode=e, dilate=d,
                         min_area=area[0], max_area=area[1])
        streams = [SyntheticStream(rows, cols, 100 * case + s, n_discs=1 + s, radius=max(3, min(rows, cols) // 9),
                                   noise=int(rng.integers(2, 20)), flicker=bool(case % 2)) for s in range(n)]
        orcs = [O.Mog2(rows, cols, 3) for _ in range(n)]
        for t in range(9):
            frames = [st.frame(t, with_discs=t > 0) for st in streams]
            got = hp.track(frames)
            for s in range(n):
                want, thr = O.chain_step(orcs[s], frames[s], rate, p)
                assert (hp.read_mask(1, s) == thr).all(), (case, t, s)
                _same_detection(got[s], want, (case, t, s))
        for s in range(n):
            _same_state(hp.mog_state(s), orcs[s].state(), (case, s))
        hp.close()


def test_two_contexts_interleaved_share_nothing(A):
    """Two contexts (different geometry and parameters) used alternately in one process."""
    from oat_amd.synth import SyntheticStream, disc_hsv_window
    win = disc_hsv_window()
    cfgs = [dict(rows=96, cols=128, erode=0, dilate=5), dict(rows=70, cols=200, erode=3, dilate=0)]
    hps, orcs, ps, sts = [], [], [], []
    for i, c in enumerate(cfgs):
        hps.append(A.HotPath(c["rows"], c["cols"], n_streams=1, adaptation_coeff=0.02, erode=c["erode"],
                             dilate=c["dilate"], area=(3.0, 1e6), **win))
        orcs.append(O.Mog2(c["rows"], c["cols"], 3))
        ps.append(O.hsv_params(h_lo=100, h_hi=125, s_lo=150, s_hi=256, v_lo=100, v_hi=256, erode=c["erode"],
                               dilate=c["dilate"], min_area=3.0, max_area=1e6))
        sts.append(SyntheticStream(c["rows"], c["cols"], 50 + i, n_discs=1, radius=6))
    for t in range(15):
        for i in (0, 1, 1, 0)[: 2 + (t % 2)]:
            f = sts[i].frame()
            got = hps[i].track([f])[0]
            want, thr = O.chain_step(orcs[i], f, 0.02, ps[i])
            assert (hps[i].read_mask(1) == thr).all(), (t, i)
            _same_detection(got, want, (t, i))


def test_error_behaviour(A):
    with pytest.raises(A.OatGpuError):
        A.HSVDetector(10, 10, area=(5.0, 1.0))          # HSVDetector.cpp:135
    with pytest.raises(A.OatGpuError):
        A.HSVDetector(10, 10, h_thresh=(0, 300))        # HSVDetector.cpp:87
    with pytest.raises(ValueError):
        A.BackgroundSubtractorMOG(10, 10, adaptation_coeff=1.5)
    d = A.HSVDetector(10, 10)
    with pytest.raises(A.OatGpuError):
        d.detectPosition(np.zeros((10, 10, 3), np.uint8), stream=3)


# ------------------------------------------------------- posifilt kalman ----

def _kalman_frames(rows, cols, n, nframes, gaps):
    """Per stream one bright square on a straight path; no square during the gaps."""
    out = []
    for t in range(nframes):
        f = np.zeros((n, rows, cols, 3), np.uint8)
        for s in range(n):
            if any(a <= t < b for a, b in gaps[s]):
                continue
            x = 10 + (3 + s) * t % (cols - 30)
            y = 8 + (2 * t + 5 * s) % (rows - 24)
            f[s, y:y + 9 + s, x:x + 12] = 255
        out.append(f)
    return out


@pytest.mark.parametrize("pipelined", [False, True])
def test_kalman_filter_on_the_batch_matches_oracle(A, pipelined):
    """oatgpu_set_kalman: detections of every stream filtered on the device, in frame order even
    though consecutive frames use different HIP streams; equal (bit for bit) to the oracle filter
    fed with the oracle detections."""
    import torch
    rows, cols, n, nframes = 96, 160, 3, 60
    gaps = [((20, 23),), ((0, 4), (30, 45)), ()]
    frames = _kalman_frames(rows, cols, n, nframes, gaps)
    kw = dict(dt=0.01, timeout=0.08, sigma_accel=30.0, sigma_noise=1.5)
    hp = A.HotPath(rows, cols, n_streams=n, ring_depth=4, adaptation_coeff=0.0, erode=0, dilate=3,
                   v_thresh=(200, 256), area=(4.0, 1e6))
    hp.set_kalman(True, **kw)
    hp.set_fusion(2)                 # device frames pair only on request (oatgpu_set_fusion)
    p = O.hsv_params(v_lo=200, v_hi=256, erode=0, dilate=3, min_area=4.0, max_area=1e6)
    orc = [O.Mog2(rows, cols, 3) for _ in range(n)]
    kal = [O.Kalman(**kw) for _ in range(n)]
    want = []
    for f in frames:
        row = []
        for s in range(n):
            d, _ = O.chain_step(orc[s], f[s], 0.0, p)
            row.append((d, kal[s].filter(d["valid"], d["x"], d["y"])))
        want.append(row)

    got = []
    if pipelined:
        dev = torch.device("cuda:0")
        bufs = [torch.from_numpy(f).to(dev) for f in frames]
        torch.cuda.synchronize()
        for t in range(nframes):
            if hp.outstanding() == 4:
                got.append(hp.collect())
            hp.enqueue_dev(bufs[t].data_ptr())
        while hp.outstanding():
            got.append(hp.collect())
    else:
        got = [hp.track(list(f)) for f in frames]

    tracked = 0
    for t in range(nframes):
        for s in range(n):
            g, (d, k) = got[t][s], want[t][s]
            assert g.raw_valid == d["valid"], (t, s)
            if d["valid"]:
                assert (g.raw_x, g.raw_y, g.a00) == (d["x"], d["y"], d["a00"]), (t, s)
            assert g.position_valid == k["position_valid"] and g.velocity_valid == k["velocity_valid"], (t, s)
            assert (g.x, g.y, g.vx, g.vy) == (k["x"], k["y"], k["vx"], k["vy"]), (t, s, g, k)
            tracked += g.position_valid
    assert tracked > 100
    # stream 1 sees nothing for 15 frames: the filter coasts 8 frames on the stale measurement, then drops
    assert [got[t][1].position_valid for t in range(29, 46)] == [True] * 8 + [False] * 8 + [True]

    # the reference's defaults (--timeout 0) never track; turning the filter off restores raw output
    hp.set_kalman(True)
    r = hp.track(list(frames[10]))
    assert all((not q.position_valid) and (q.x, q.y, q.vx, q.vy) == (6.0, 6.0, 6.0, 6.0) and q.raw_valid for q in r)
    hp.set_kalman(False)
    r = hp.track(list(frames[11]))
    assert all(q.position_valid and not q.velocity_valid and (q.x, q.y) == (q.raw_x, q.raw_y) for q in r)
    with pytest.raises(A.OatGpuError):
        hp.set_kalman(True, dt=0.0)


def test_pipelined_host_frames_equal_the_synchronous_call(A):
    """oatgpu_track_enqueue (host frames, copy stream, per-slot staging) vs oatgpu_track_batch."""
    from oat_amd.synth import SyntheticStream
    rows, cols, n, nframes = 120, 200, 2, 20
    sts = [SyntheticStream(rows, cols, 40 + s, n_discs=1) for s in range(n)]
    frames = [[st.frame(t, with_discs=t > 0) for st in sts] for t in range(nframes)]
    kw = dict(n_streams=n, adaptation_coeff=0.02, erode=3, dilate=5, area=(10.0, 1e5), h_thresh=(100, 125),
              s_thresh=(150, 256), v_thresh=(100, 256))
    a = A.HotPath(rows, cols, ring_depth=3, **kw)
    b = A.HotPath(rows, cols, **kw)
    want = [b.track(f) for f in frames]
    got = []
    for f in frames:
        if a.outstanding() == 3:
            got.append(a.collect())
        a.enqueue(f)
    with pytest.raises(A.OatGpuError):
        a.enqueue(frames[0][:1])                    # wrong number of frames
    while a.outstanding():
        got.append(a.collect())
    assert got == want and sum(p.position_valid for r in got for p in r) >= 30
    _same_state(a.mog_state(1), b.mog_state(1)[:4])


def test_track_sequence_equals_frame_by_frame(A):
    """oatgpu_track_sequence_dev (the enqueue/collect loop inside the library) vs per-frame calls."""
    import torch
    from oat_amd.synth import SyntheticStream, disc_hsv_window
    rows, cols, n, nframes = 90, 150, 2, 23
    sts = [SyntheticStream(rows, cols, 70 + s, n_discs=1) for s in range(n)]
    frames = [np.stack([st.frame(t, with_discs=t > 0) for st in sts]) for t in range(nframes)]
    dev = torch.device("cuda:0")
    bufs = [torch.from_numpy(f).to(dev) for f in frames]
    torch.cuda.synchronize()
    kw = dict(n_streams=n, adaptation_coeff=0.02, erode=3, dilate=5, area=(10.0, 1e5), **disc_hsv_window())
    a = A.HotPath(rows, cols, ring_depth=5, **kw)
    b = A.HotPath(rows, cols, **kw)
    got = a.track_sequence_dev([t.data_ptr() for t in bufs])
    want = [b.track(list(f)) for f in frames]
    assert got == want and sum(p.position_valid for r in got for p in r) >= 30
    assert a.track_sequence_dev([]) == []
    # ... and the timed form (bench.py's block timing): same results, collection times ascending from the call's entry
    c = A.HotPath(rows, cols, ring_depth=5, **kw)
    got_t, done = c.track_sequence_dev([t.data_ptr() for t in bufs], timed=True)
    assert got_t == want and len(done) == len(bufs)
    assert done[0] > 0 and all(y >= x for x, y in zip(done, done[1:])) and done[-1] < 5.0
    a.enqueue_dev(bufs[0].data_ptr())
    with pytest.raises(A.OatGpuError):
        a.track_sequence_dev([bufs[1].data_ptr()])          # results outstanding
    a.collect()


# ------------------------------------------- BASELINE configs 3 and 4 (batched) --

@pytest.mark.parametrize("n", [16, 8])
def test_hot_path_batched_1080p(A, n):
    """BASELINE configs[2] (16 x 1080p batched on one GPU) and the per-GPU shard of configs[3]
    (8 x 1080p): ONE context, one launch per stage for all streams, every stream against its OWN
    oracle instance.  The discs differ per stream (count, radius, path), so a stream mix-up inside
    the batched kernels cannot pass.  Masks, contour sums, centroids and the full fp32 model."""
    from oat_amd.synth import SyntheticStream, disc_hsv_window
    rows, cols = 1080, 1920
    win = disc_hsv_window()
    hp = A.HotPath(rows, cols, n_streams=n, adaptation_coeff=0.01, erode=3, dilate=7, area=(20.0, 1e5), **win)
    p = O.hsv_params(h_lo=100, h_hi=125, s_lo=150, s_hi=256, v_lo=100, v_hi=256, erode=3, dilate=7,
                     min_area=20.0, max_area=1e5)
    streams = [SyntheticStream(rows, cols, 100 + s, n_discs=1 + s % 3, radius=14 + 3 * s) for s in range(n)]
    oracles = _chain_oracles(rows, cols, n)
    seen = set()
    for t in range(3):
        frames = [st.frame(t, with_discs=(t > 0)) for st in streams]
        got = hp.track(frames)
        for s in range(n):
            want, thr = O.chain_step(oracles[s], frames[s], 0.01, p, nthreads=8)
            assert (hp.read_mask(1, s) == thr).all(), (t, s)
            _same_detection(got[s], want, (t, s))
            if want["valid"]:
                seen.add((want["a00"], want["a10"], want["a01"]))
    assert len(seen) >= n                   # the streams really do give different answers
    for s in range(n):
        _same_state(hp.mog_state(s), oracles[s].state(), s)
    hp.close()


def test_measurement_env_is_inert_in_the_product_library(A):
    """OATGPU_EXPT=1 used to make the shipped library skip the whole back half
    and still return OATGPU_OK.  The product build no longer reads any OATGPU_* measurement switch:
    a child process with all of them set must produce the same positions as the oracle."""
    import subprocess
    import sys
    code = r"""
import os, sys, json
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), 'tests'))
import oat_amd
from oat_amd.synth import SyntheticStream, disc_hsv_window
st = SyntheticStream(120, 200, 3, n_discs=1, radius=9)
hp = oat_amd.HotPath(120, 200, n_streams=1, adaptation_coeff=0.01, erode=3, dilate=5, area=(5.0, 1e5), **disc_hsv_window())
out = []
for t in range(5):
    r = hp.track([st.frame(t, with_discs=t > 0)])[0]
    out.append([int(r.position_valid), r.a00, r.a10, r.a01, r.first_pixel])
print(json.dumps(out))
"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, OATGPU_EXPT="1", OATGPU_SERIAL="1", OATGPU_NB="1", OATGPU_GRAPH="1",
               OATGPU_PRIVATE_STREAMS="1", OATGPU_COPY_PAD="2")
    env.pop("OATGPU_LIB", None)
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    from oat_amd.synth import SyntheticStream
    st = SyntheticStream(120, 200, 3, n_discs=1, radius=9)
    orc = O.Mog2(120, 200, 3)
    p = O.hsv_params(h_lo=100, h_hi=125, s_lo=150, s_hi=256, v_lo=100, v_hi=256, erode=3, dilate=5,
                     min_area=5.0, max_area=1e5)
    nvalid = 0
    for t in range(5):
        want, _ = O.chain_step(orc, st.frame(t, with_discs=t > 0), 0.01, p)
        assert got[t][0] == int(want["valid"]), (t, got[t], want)
        if want["valid"]:
            assert got[t][1:] == [want["a00"], want["a10"], want["a01"], want["first_pixel"]], (t, got[t], want)
            nvalid += 1
    assert nvalid >= 3


# ------------------------------------------------ round-2 entry points of the C ABI --

def test_traffic_audit_counts_what_the_kernel_moves(A):
    """oatgpu_traffic_audit: the audited instantiation of the per-pixel kernel must (i) leave every result as it
    is, (ii) count close to the full 104 B/px of reads on an input with five live modes where the matching one is
    rarely the first, and far less on a static scene -- where a matched single-mode pixel costs 24 B read
    (3 BGR + 1 counter + 20 mode 0) and 20 B written."""
    rows, cols = 64, 128
    rng = np.random.default_rng(5)
    table = np.array([[20, 30, 40], [90, 200, 60], [200, 60, 120], [240, 240, 230], [40, 130, 220]], np.int16)
    phase = rng.integers(0, 5, (rows, cols))
    hp = A.HotPath(rows, cols, n_streams=1, adaptation_coeff=0.05, erode=0, dilate=0, area=(1.0, 1e9))
    ref = A.HotPath(rows, cols, n_streams=1, adaptation_coeff=0.05, erode=0, dilate=0, area=(1.0, 1e9))
    frames = [np.clip(table[(phase + t) % 5] + rng.integers(-4, 5, (rows, cols, 3)), 0, 255).astype(np.uint8) for t in range(40)]
    for f in frames[:30]:
        hp.track([f]); ref.track([f])
    hp.traffic_audit(True)
    for f in frames[30:]:
        assert hp.track([f]) == ref.track([f])                      # same results with the audit on
    t = hp.traffic_read()
    hp.traffic_audit(False)
    assert t["launches"] == 10 and t["pixels"] == 10 * rows * cols
    # nearly every lane loads every plane, the counter and the pixel (104 B); never more than that
    assert 80 * t["pixels"] <= t["lane_bytes_read"] <= 104 * t["pixels"]
    assert t["lane_bytes_read"] <= t["sector32_bytes_read"] <= t["sector64_bytes_read"] <= 128 * t["pixels"]
    assert 20 * t["pixels"] <= t["lane_bytes_written"] <= 101 * t["pixels"]
    for a, b in zip(hp.mog_state(), ref.mog_state()):
        assert (np.asarray(a) == np.asarray(b)).all()
    # a static scene: one mode everywhere
    st = A.HotPath(rows, cols, n_streams=1, adaptation_coeff=0.05, erode=0, dilate=0, area=(1.0, 1e9))
    still = np.full((rows, cols, 3), 90, np.uint8)
    for _ in range(5):
        st.track([still])
    st.traffic_audit(True)
    st.track([still])
    u = st.traffic_read()
    # + the threshold mask: one 8-byte word per 64 pixels
    assert u["lane_bytes_read"] == 24 * rows * cols and u["lane_bytes_written"] == 20 * rows * cols + rows * cols // 8
    # two frames a launch (the pipelined path): the second frame adds its 3 B/px and its threshold words, nothing else
    st.traffic_audit(True)
    st.enqueue([still]); st.enqueue([still])
    st.collect(); st.collect()
    u = st.traffic_read()
    assert u["launches"] == 1 and u["pixels"] == rows * cols
    assert u["lane_bytes_read"] == 27 * rows * cols and u["lane_bytes_written"] == 20 * rows * cols + 2 * (rows * cols // 8)


def test_mask_filter_and_bsub_background_entry_points(A):
    """oatgpu_mask_filter (FrameMasker.cpp:71-75) and oatgpu_bsub_set_background (BackgroundSubtractor.cpp:63-71)."""
    import ctypes as C
    from oat_amd import ffi
    rows, cols = 37, 70
    rng = np.random.default_rng(9)
    f = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    m = (rng.random((rows, cols)) < 0.5).astype(np.uint8) * 255
    g = A.BackgroundSubtractorMOG(rows, cols)
    out = np.empty_like(f)
    g._chk(g.lib.oatgpu_mask_filter(g.ctx, 0, ffi.u8(f), ffi.u8(out)))
    assert (out == f).all()                                           # no mask set: untouched
    g.set_roi_mask(m)
    g._chk(g.lib.oatgpu_mask_filter(g.ctx, 0, ffi.u8(f), ffi.u8(out)))
    assert (out == np.where(m[..., None] != 0, f, 0)).all()
    bg = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    b = A.BackgroundSubtractor(rows, cols, adaptation_coeff=0.0)
    b._chk(b.lib.oatgpu_bsub_set_background(b.ctx, 0, ffi.u8(bg)))
    assert (b.filter(f) == np.clip(f.astype(int) - bg, 0, 255)).all()  # frame - background, saturating
    adapt = A.BackgroundSubtractor(rows, cols, adaptation_coeff=0.1)
    adapt._chk(adapt.lib.oatgpu_bsub_set_background(adapt.ctx, 0, ffi.u8(bg)))
    with pytest.raises(A.OatGpuError):                               # the reference's accumulateWeighted asserts here
        adapt.filter(f)


def test_track_ready_and_input_consumed(A):
    """The two calls the batched C++ component pipelines with: after input_consumed the host frames may be
    overwritten; track_ready turns 1 once the oldest result can be collected without blocking."""
    import time
    rows, cols, n = 120, 160, 2
    from oat_amd.synth import SyntheticStream, disc_hsv_window
    hp = A.HotPath(rows, cols, n_streams=n, adaptation_coeff=0.01, erode=3, dilate=5, area=(5.0, 1e5), ring_depth=3,
                   **disc_hsv_window())
    ref = A.HotPath(rows, cols, n_streams=n, adaptation_coeff=0.01, erode=3, dilate=5, area=(5.0, 1e5), **disc_hsv_window())
    streams = [SyntheticStream(rows, cols, 40 + s, n_discs=1, radius=10) for s in range(n)]
    assert hp.lib.oatgpu_track_ready(hp.ctx) == 0                    # nothing outstanding
    bufs = [np.empty((rows, cols, 3), np.uint8) for _ in range(n)]    # ONE set of host buffers, reused every step
    for t in range(8):
        frames = [st.frame(t, with_discs=t > 0) for st in streams]
        for b, f in zip(bufs, frames):
            b[...] = f
        hp.enqueue(bufs)
        hp._chk(hp.lib.oatgpu_track_input_consumed(hp.ctx))
        for b in bufs:
            b[...] = 0                                                # scribble: the device must have its copy by now
        deadline = time.time() + 10
        while hp.lib.oatgpu_track_ready(hp.ctx) != 1:
            assert time.time() < deadline
        assert hp.collect() == ref.track(frames), t


def test_input_consumed_per_stream(A):
    """oatgpu_track_input_consumed_stream: an N-camera component posts SOURCE i as soon as frame i has left its buffer.  After
    the call for stream i the host buffer of stream i (and of every stream before it) may be overwritten; the first
    call falls back to the whole set and switches the per-stream events on; out-of-range indices are refused."""
    rows, cols, n = 96, 200, 3
    from oat_amd.synth import SyntheticStream, disc_hsv_window
    kw = dict(n_streams=n, adaptation_coeff=0.01, erode=3, dilate=5, area=(5.0, 1e5), **disc_hsv_window())
    hp = A.HotPath(rows, cols, ring_depth=3, **kw)
    ref = A.HotPath(rows, cols, **kw)
    streams = [SyntheticStream(rows, cols, 60 + s, n_discs=1, radius=9) for s in range(n)]
    bufs = [np.empty((rows, cols, 3), np.uint8) for _ in range(n)]
    assert hp.lib.oatgpu_track_input_consumed_stream(hp.ctx, n) < 0 and hp.lib.oatgpu_track_input_consumed_stream(hp.ctx, -1) < 0
    for t in range(10):
        frames = [st.frame(t, with_discs=t > 0) for st in streams]
        for b, f in zip(bufs, frames):
            b[...] = f
        hp.enqueue(bufs)
        for s_ in range(n):
            hp.input_consumed_stream(s_)
            bufs[s_][...] = 255 - bufs[s_]                            # scribble at once: this frame must be on the device
        assert hp.collect() == ref.track(frames), t


@pytest.mark.parametrize("stage_copy", [0, 1])
def test_stage_camera_by_camera_equals_enqueue(A, stage_copy):
    """oatgpu_track_stage / oatgpu_track_enqueue_staged: the host-frame path camera by camera (any order, each camera's
    buffer reusable after its own input_consumed_stream) gives what oatgpu_track_enqueue gives; a set cannot be
    registered before it is complete, a stream cannot be staged twice, and enqueue() is refused while a set is open.
    stage_copy = 1 (oatgpu_set_stage_copy, r04): the frames are moved by a copy KERNEL that reads page-locked host memory
    in place -- two cameras hand over page-locked frames (rows x cols chosen so that a frame is not a multiple of 16
    bytes: the kernel's tail), the third ordinary memory, which silently takes the DMA path."""
    import torch
    rows, cols, n = 90, 170, 3
    from oat_amd.synth import SyntheticStream, disc_hsv_window
    kw = dict(n_streams=n, adaptation_coeff=0.01, erode=3, dilate=5, area=(5.0, 1e5), **disc_hsv_window())
    hp = A.HotPath(rows, cols, ring_depth=2, **kw)
    hp.set_stage_copy(stage_copy)
    ref = A.HotPath(rows, cols, **kw)
    streams = [SyntheticStream(rows, cols, 80 + s, n_discs=1, radius=9) for s in range(n)]
    pinned = [torch.empty((rows, cols, 3), dtype=torch.uint8).pin_memory() for _ in range(n - 1)]
    bufs = [t.numpy() for t in pinned] + [np.empty((rows, cols, 3), np.uint8)]
    want = []
    for t in range(9):
        frames = [st.frame(t, with_discs=t > 0) for st in streams]
        want.append(ref.track(frames))
        order = [(t + k) % n for k in range(n)]
        for k, s_ in enumerate(order):
            bufs[s_][...] = frames[s_]
            hp.stage(s_, bufs[s_])
            if k == 0:
                assert hp.lib.oatgpu_track_stage(hp.ctx, s_, A.ffi.u8(bufs[s_])) < 0          # twice
                assert hp.lib.oatgpu_track_enqueue_staged(hp.ctx, 0.01) < 0                  # incomplete
                ptrs = (A.ffi._u8p * n)(*[A.ffi.u8(b) for b in bufs])
                assert hp.lib.oatgpu_track_enqueue(hp.ctx, ptrs, n, 0.01) < 0                # a set is open
            hp.input_consumed_stream(s_)
            bufs[s_][...] = 7                                         # scribble: the frame is on the device
        hp.enqueue_staged()
        if t % 2 == 1:                                               # ring of two: collect in pairs
            assert hp.collect() == want[t - 1], t - 1
            assert hp.collect() == want[t], t
    assert hp.collect() == want[8]
    hp.stage(0, bufs[0])                                             # ring empty again: a third set may start ...
    hp.stage(1, bufs[1]); hp.stage(2, bufs[2]); hp.enqueue_staged()
    hp.stage(0, bufs[0]); hp.stage(1, bufs[1]); hp.stage(2, bufs[2]); hp.enqueue_staged()
    assert hp.lib.oatgpu_track_stage(hp.ctx, 0, A.ffi.u8(bufs[0])) == A.ffi.E_RING_FULL      # ... and the ring limit holds
    hp.collect(); hp.collect()


def test_deferred_single_stage_calls_equal_the_plain_ones(A):
    """oatgpu_set_deferred (ABI 7): a frame filter / detector returns when its input has been read and keeps its result on the
    device; oatgpu_fetch_frame / oatgpu_fetch_position deliver what the plain call would have written -- mog (the model
    advances exactly once per call), bsub, thresh, cvt_color, detect_hsv.  The caller's input buffer may be scribbled on
    as soon as the call has returned; a second call before the fetch is refused; a fetch with nothing waiting too."""
    import ctypes as C
    from oat_amd import ffi
    from oat_amd.synth import SyntheticStream, disc_hsv_window
    rows, cols = 120, 200
    st = SyntheticStream(rows, cols, 7, n_discs=2, radius=10)
    frames = [st.frame(t, with_discs=t > 0) for t in range(6)]
    kw = dict(erode=2, dilate=4, area=(5.0, 1e5), **disc_hsv_window())
    plain, dfr = A.HotPath(rows, cols, adaptation_coeff=0.02, **kw), A.HotPath(rows, cols, adaptation_coeff=0.02, **kw)
    lib = dfr.lib
    assert lib.oatgpu_fetch_frame(dfr.ctx, ffi.u8(np.empty((rows, cols, 3), np.uint8))) < 0       # nothing waiting
    ffi.check(lib, dfr.ctx, lib.oatgpu_set_deferred(dfr.ctx, 1))
    for t, f in enumerate(frames):
        want = np.empty_like(f)
        ffi.check(lib, plain.ctx, lib.oatgpu_mog_filter(plain.ctx, 0, ffi.u8(f), ffi.u8(want), 0.02))
        buf, got = f.copy(), np.full_like(f, 99)
        ffi.check(lib, dfr.ctx, lib.oatgpu_mog_filter(dfr.ctx, 0, ffi.u8(buf), ffi.u8(got), 0.02))
        assert (got == 99).all()                                     # deferred: the output argument is not written
        buf[...] = 7                                                 # the input has been read: scribble
        assert lib.oatgpu_mog_filter(dfr.ctx, 0, ffi.u8(f), ffi.u8(got), 0.02) < 0           # one result at a time
        assert lib.oatgpu_fetch_position(dfr.ctx, C.byref(ffi.Position())) < 0              # ... and of the right kind
        ffi.check(lib, dfr.ctx, lib.oatgpu_fetch_frame(dfr.ctx, ffi.u8(got)))
        assert (got == want).all(), t
        # the filtered frame through col -C HSV and posidet hsv, both deferred
        hsv_w, hsv_g = np.empty_like(f), np.empty_like(f)
        ffi.check(lib, plain.ctx, lib.oatgpu_cvt_color(plain.ctx, 2, 3, ffi.u8(want), ffi.u8(hsv_w)))
        ffi.check(lib, dfr.ctx, lib.oatgpu_cvt_color(dfr.ctx, 2, 3, ffi.u8(got), ffi.u8(hsv_g)))
        ffi.check(lib, dfr.ctx, lib.oatgpu_fetch_frame(dfr.ctx, ffi.u8(hsv_g)))
        assert (hsv_g == hsv_w).all(), t
        pw, pg = ffi.Position(), ffi.Position()
        ffi.check(lib, plain.ctx, lib.oatgpu_detect_hsv(plain.ctx, 0, ffi.u8(hsv_w), C.byref(pw)))
        ffi.check(lib, dfr.ctx, lib.oatgpu_detect_hsv(dfr.ctx, 0, ffi.u8(hsv_g), None))
        assert lib.oatgpu_fetch_frame(dfr.ctx, ffi.u8(got)) < 0
        ffi.check(lib, dfr.ctx, lib.oatgpu_fetch_position(dfr.ctx, C.byref(pg)))
        assert (pg.valid, pg.a00, pg.a10, pg.a01, pg.x, pg.y) == (pw.valid, pw.a00, pw.a10, pw.a01, pw.x, pw.y), t
    assert (plain.mog_state()[1] == dfr.mog_state()[1]).all()                               # same model on both sides
    # bsub and thresh the same way
    for name, args in (("oatgpu_bsub_filter", lambda c, i, o: (c, 0, i, o, 0.05)), ("oatgpu_thresh_filter", lambda c, i, o: (c, i, o, 100, 200))):
        for f in frames[:3]:
            want, got = np.empty_like(f), np.empty_like(f)
            ffi.check(lib, plain.ctx, getattr(lib, name)(*args(plain.ctx, ffi.u8(f), ffi.u8(want))))
            ffi.check(lib, dfr.ctx, getattr(lib, name)(*args(dfr.ctx, ffi.u8(f), ffi.u8(got))))
            ffi.check(lib, dfr.ctx, lib.oatgpu_fetch_frame(dfr.ctx, ffi.u8(got)))
            assert (got == want).all(), name
    ffi.check(lib, dfr.ctx, lib.oatgpu_set_deferred(dfr.ctx, 0))
    got = np.empty_like(frames[0])
    ffi.check(lib, dfr.ctx, lib.oatgpu_thresh_filter(dfr.ctx, ffi.u8(frames[0]), ffi.u8(got), 100, 200))    # plain again
    assert lib.oatgpu_fetch_frame(dfr.ctx, ffi.u8(got)) < 0


def test_stage_abort_gives_up_a_partly_staged_set(A):
    """oatgpu_track_stage_abort (ABI 7): a camera ended in the middle of a round.  The set is forgotten --
    no result is owed, the model has not moved -- and the context goes on: the next complete set gives what a context
    that never saw the aborted frames gives, enqueue() is accepted again, and aborting nothing is a no-op."""
    rows, cols, n = 90, 170, 3
    from oat_amd.synth import SyntheticStream, disc_hsv_window
    kw = dict(n_streams=n, adaptation_coeff=0.01, erode=3, dilate=5, area=(5.0, 1e5), **disc_hsv_window())
    hp = A.HotPath(rows, cols, ring_depth=2, **kw)
    ref = A.HotPath(rows, cols, **kw)
    streams = [SyntheticStream(rows, cols, 90 + s, n_discs=1, radius=9) for s in range(n)]
    hp.stage_abort()                                                  # nothing staged: no-op
    junk = np.full((rows, cols, 3), 200, np.uint8)
    for t in range(8):
        frames = [st.frame(t, with_discs=t > 0) for st in streams]
        want = ref.track(frames)
        if t % 3 == 1:                                               # a round that dies after one or two cameras
            for s_ in range(1 + t % 2):
                hp.stage(s_, junk)
            assert hp.lib.oatgpu_track_enqueue_staged(hp.ctx, 0.01) < 0
            hp.stage_abort()
            assert hp.outstanding() == 0                             # nothing was registered
        if t % 2 == 0:
            for s_ in range(n):
                hp.stage(s_, frames[s_])
            hp.enqueue_staged()
        else:
            hp.enqueue(frames)                                       # accepted again: no set is open
        assert hp.collect() == want, t
    assert hp.outstanding() == 0


def test_back_half_speculation_and_repair(A):
    """The pipelined path launches the row scan + the single-workgroup LDS blob kernel only, as long as frames are
    sparse enough for it; a frame that is not (here: thousands of foreground specks) comes back marked and
    oatgpu_track_collect runs the global kernels on its threshold bits before handing the result out.  Sparse and
    busy frames alternate in every pattern the ring can see; every result must be the oracle's."""
    rows, cols, n = 240, 320, 2
    rng = np.random.default_rng(11)
    win = dict(h_thresh=(100, 125), s_thresh=(150, 256), v_thresh=(100, 256))
    hp = A.HotPath(rows, cols, n_streams=n, ring_depth=4, adaptation_coeff=0.01, erode=0, dilate=2, area=(4.0, 1e9), **win)
    p = O.hsv_params(h_lo=100, h_hi=125, s_lo=150, s_hi=256, v_lo=100, v_hi=256, erode=0, dilate=2, min_area=4.0, max_area=1e9)
    orc = [O.Mog2(rows, cols, 3) for _ in range(n)]
    base = rng.integers(90, 140, (n, rows, cols, 3)).astype(np.int16)

    def frame(t, busy):
        f = np.clip(base + rng.integers(-5, 6, base.shape), 0, 255).astype(np.uint8)
        if t > 0:
            for s in range(n):
                cy, cx = 40 + (7 * t + 30 * s) % 150, 50 + (11 * t + 40 * s) % 200
                f[s, cy:cy + 20, cx:cx + 25] = (255, 64, 0)
                if busy:                                     # specks of the blob colour all over: > 3072 runs
                    m = rng.random((rows, cols)) < 0.08
                    f[s][m] = (255, 64, 0)
        return f
    pattern = [0] * 20 + [1, 0, 0, 1, 1, 0, 1, 1, 1, 1] + [0] * 24 + [1] + [0] * 5
    frames = [frame(t, b) for t, b in enumerate(pattern)]
    got = []
    for f in frames:
        hp.enqueue(list(f))
        if hp.outstanding() >= 4:
            got.append(hp.collect())
    while hp.outstanding():
        got.append(hp.collect())
    assert len(got) == len(frames)
    for t, f in enumerate(frames):
        for s in range(n):
            want = O.chain_step(orc[s], f[s], 0.01, p)[0]
            _same_detection(got[t][s], want, (t, s, pattern[t]))


@pytest.mark.parametrize("fusion,ring,kalman", [(2, 4, False), (1, 2, False), (2, 3, True), (2, 3, False), (2, 5, False), (1, 3, False)])
def test_early_blob_dispatch_equals_the_plain_path(A, fusion, ring, kalman):
    """Early dispatch of the blob workgroup (r04; oatgpu_set_early_blob, kernels_bloblds.hip): on the pipelined device-frame path
    the k_blob_lds workgroup of a frame is submitted on its own stream ahead of the frame's row scan and waits on the
    device for the row scan's ticket.  Frames big enough to take that path (>= 4 MP a step), quiet and BUSY ones in every
    pattern a ring can see (busy = declined by the LDS kernel -> repaired by the global kernels in scratch set 2; then the
    full launch sequence until the streak is back), with and without two frames a launch, with ODD ring depths (two
    consecutive frames then sit in ring slots of the same parity -- the scratch sets go by frame parity) and with the
    position filter (never speculative: the plain order): every result equals the plain path's and the oracle's, the
    threshold masks too."""
    import torch
    rows, cols, n = 1080, 1920, 2                                   # 2 x 2.07 MP = 4.15 MP a step
    rng = np.random.default_rng(31 + fusion + ring)
    win = dict(h_thresh=(100, 125), s_thresh=(150, 256), v_thresh=(100, 256))
    kw = dict(n_streams=n, ring_depth=ring, adaptation_coeff=0.01, erode=3, dilate=5, area=(20.0, 1e6), **win)
    hp, ref = A.HotPath(rows, cols, **kw), A.HotPath(rows, cols, **kw)
    hp.set_early_blob(True)
    ref.set_early_blob(False)
    for h in (hp, ref):
        h.set_fusion(fusion)
        if kalman:
            h.set_kalman(True, dt=0.02, timeout=1.0, sigma_accel=5.0, sigma_noise=1.0)
    p = O.hsv_params(h_lo=100, h_hi=125, s_lo=150, s_hi=256, v_lo=100, v_hi=256, erode=3, dilate=5, min_area=20.0, max_area=1e6)
    orc = [O.Mog2(rows, cols, 3) for _ in range(n)]
    base = rng.integers(90, 150, (n, rows, cols, 3)).astype(np.int16)

    def frame(t, busy):
        f = np.clip(base + rng.integers(-5, 6, base.shape), 0, 255).astype(np.uint8)
        if t > 0:
            for s_ in range(n):
                cy, cx = 40 + (7 * t + 30 * s_) % 900, 50 + (11 * t + 40 * s_) % 1700
                f[s_, cy:cy + 30, cx:cx + 45] = (255, 64, 0)
                if busy:                                             # specks of the blob colour: far more than 3 072 runs
                    f[s_][rng.random((rows, cols)) < 0.01] = (255, 64, 0)
        return f
    pattern = [0] * 5 + [1, 0, 0, 1, 1, 0] + [0] * 18 + [1] + [0] * 2
    frames = [frame(t, b) for t, b in enumerate(pattern)]
    dev = [torch.from_numpy(f).cuda() for f in frames]
    torch.cuda.synchronize()

    def run(h):
        out = []
        for d in dev:
            h.enqueue_dev(d.data_ptr(), keepalive=d)
            if h.outstanding() >= ring:
                out.append(h.collect())
        while h.outstanding():
            out.append(h.collect())
        return out
    got, plain = run(hp), run(ref)
    assert len(got) == len(frames) and got == plain
    if not kalman:
        for t, f in enumerate(frames):
            for s_ in range(n):
                _same_detection(got[t][s_], O.chain_step(orc[s_], f[s_], 0.01, p)[0], (t, s_, pattern[t]))
    for s_ in range(n):
        assert (hp.read_mask(A.ffi.TAP_MORPH, s_) == ref.read_mask(A.ffi.TAP_MORPH, s_)).all()
        assert (hp.read_mask(A.ffi.TAP_FINAL, s_) == ref.read_mask(A.ffi.TAP_FINAL, s_)).all()
    # ... and both paths in ONE context, switched between steps (the B streams are drained at the switch)
    hp.set_early_blob(False)
    hp.enqueue_dev(dev[-1].data_ptr(), keepalive=dev[-1]); hp.set_early_blob(True); hp.enqueue_dev(dev[-2].data_ptr(), keepalive=dev[-2])
    ref.enqueue_dev(dev[-1].data_ptr(), keepalive=dev[-1]); ref.enqueue_dev(dev[-2].data_ptr(), keepalive=dev[-2])
    assert [hp.collect(), hp.collect()] == [ref.collect(), ref.collect()]


@pytest.mark.parametrize("shape", [(2160, 3840, 1, 1), (1080, 1920, 2, 1), (2160, 3840, 1, 2)])
def test_early_order_survives_a_tool_that_serialises_dispatches(shape):
    """the default path of ONE stream of >= 4 MP (and of two 1080p streams) parks a blob workgroup that
    waits on the device for a ticket a later kernel publishes -- two kernels resident at once, which HIP does not promise.
    A child process runs 44 frames through that path with the ring kept full under everything that serialises dispatches
    here: AMD_SERIALIZE_KERNEL=3, HIP_LAUNCH_BLOCKING=1, and a counter-collecting rocprofv3 (the tool that produced the
    100 ms waits in round 4).  Whatever the runtime does with the parked workgroup: one result per frame, in order
    (PositionDetector.cpp:58-99), every one identical to the oracle's, the whole model too; at most ONE time-out episode,
    after which the context has switched the early order off and says so; and the run is not slower than a single 100 ms
    wait explains."""
    import shutil
    import subprocess
    import sys
    import tempfile
    rows, cols, n, fusion = shape                  # fusion 2: both frames of a step park together -- still ONE episode
    child = [sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "children", "early_fallback_child.py"),
             str(rows), str(cols), str(n), "44", str(fusion)]
    base = {k: v for k, v in os.environ.items() if k not in ("AMD_SERIALIZE_KERNEL", "HIP_LAUNCH_BLOCKING")}
    modes = [("plain", {}, []), ("AMD_SERIALIZE_KERNEL=3", {"AMD_SERIALIZE_KERNEL": "3"}, []), ("HIP_LAUNCH_BLOCKING=1", {"HIP_LAUNCH_BLOCKING": "1"}, [])]
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    tmp = tempfile.mkdtemp(prefix="oat_early_", dir="/tmp")
    if os.path.exists(prof):
        modes.append(("rocprofv3 --pmc", {"TMPDIR": "/tmp"}, [prof, "--kernel-trace", "--pmc", "SQ_WAVES", "-d", tmp, "-o", "r", "--"]))
    seen = {}
    try:
        for name, env, prefix in modes:
            r = subprocess.run(prefix + child, env=dict(base, **env), cwd="/tmp", capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, (name, r.stderr[-2000:])
            j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
            seen[name] = j
            assert j["results"] == 44 and j["mismatches"] == [] and j["model_ok"], (name, j)
            assert j["timeouts"] <= 1, (name, j)
            if j["timeouts"]:
                assert "early blob dispatch switched off" in j["last_error"], (name, j)
                assert j["early_steps"] < j["steps"], (name, j)            # the steps behind the episode took the plain order
            assert j["wall_s"] < (2.0 if not prefix else 30.0) + 0.15 * j["timeouts"], (name, j)    # (a profiler's own cost aside)
        assert seen["plain"]["timeouts"] == 0 and seen["plain"]["early_steps"] >= (40 if fusion == 1 else 20), seen["plain"]   # the path under test IS the default
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
        try:
            os.makedirs(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out"), exist_ok=True)
            with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out",
                                   "early_fallback_%dx%dx%d_fusion%d.json" % shape), "w") as f:
                json.dump(seen, f, indent=1)
        except OSError:
            pass


# ------------------------------------------- two frames a launch (temporal fusion) --

def test_two_one_stream_contexts_on_the_default_early_path_interleaved(A):
    """r05: a context of ONE stream of >= 4 MP takes, by default, the early blob dispatch with the one-wave-a-workgroup
    per-pixel kernel.  All contexts of a process share the device's four streams: two such contexts, their steps
    interleaved and their rings kept full (parked blob workgroups of both queued on the one B2 stream, row scans of both on
    B0 / B1), with a busy frame in each (declined -> repaired) -- every result equals the oracle's, and the pair is not
    slower than a ticket time-out would make it."""
    import time
    import torch
    rows, cols = 2048, 2176                                          # 4.46 MP a step
    win = dict(h_thresh=(100, 125), s_thresh=(150, 256), v_thresh=(100, 256))
    kw = dict(n_streams=1, ring_depth=4, adaptation_coeff=0.01, erode=3, dilate=5, area=(20.0, 1e6), **win)
    p = O.hsv_params(h_lo=100, h_hi=125, s_lo=150, s_hi=256, v_lo=100, v_hi=256, erode=3, dilate=5, min_area=20.0, max_area=1e6)
    nframes = 17
    hps, orcs, devs, frames = [], [], [], []
    for c in range(2):
        rng = np.random.default_rng(900 + c)
        base = rng.integers(90, 150, (rows, cols, 3)).astype(np.int16)
        fs = []
        for t in range(nframes):
            f = np.clip(base + rng.integers(-5, 6, base.shape), 0, 255).astype(np.uint8)
            if t > 0:
                cy, cx = 40 + (37 * t + 300 * c) % 1900, 50 + (53 * t + 400 * c) % 2000
                f[cy:cy + 30, cx:cx + 45] = (255, 64, 0)
                if t == 6 + 3 * c:                                   # specks of the blob colour: the LDS kernel declines the frame
                    f[rng.random((rows, cols)) < 0.01] = (255, 64, 0)
            fs.append(f)
        frames.append(fs)
        devs.append([torch.from_numpy(f).cuda() for f in fs])
        hp = A.HotPath(rows, cols, **kw)
        hp.set_fusion(2)
        hps.append(hp)
        orcs.append(O.Mog2(rows, cols, 3))
    torch.cuda.synchronize()
    got = [[], []]
    t0 = time.perf_counter()
    for t in range(nframes):
        for c in (0, 1) if t % 3 else (1, 0):                        # (the order of the two contexts varies)
            hps[c].enqueue_dev(devs[c][t].data_ptr(), keepalive=devs[c][t])
            if hps[c].outstanding() >= 4:
                got[c].append(hps[c].collect())
    for c in range(2):
        while hps[c].outstanding():
            got[c].append(hps[c].collect())
    elapsed = time.perf_counter() - t0
    hits = 0
    for c in range(2):
        assert len(got[c]) == nframes
        for t in range(nframes):
            want, _ = O.chain_step(orcs[c], frames[c][t], 0.01, p, nthreads=16)
            _same_detection(got[c][t][0], want, (c, t))
            hits += want["valid"]
        _same_state(hps[c].mog_state(0), orcs[c].state(), ("ctx", c))
        hps[c].close()
    assert hits >= 2 * (nframes - 3)
    assert elapsed < 1.0, elapsed                                    # 34 frames of ~60 us; a 100 ms ticket time-out a step would be seconds


def _noisy_sequence(rng, n, rows, cols, ch, nframes, noise):
    """Frames whose pixels leave and re-enter their first mode often enough that every path between the two
    frames of a launch is taken: matched/matched, matched/full (the late record loads), full/matched, full/full."""
    shape = (n, rows, cols, 3) if ch == 3 else (n, rows, cols)
    base = rng.integers(60, 180, shape).astype(np.int16)
    alt = rng.integers(0, 256, shape).astype(np.int16)
    out = []
    for t in range(nframes):
        f = base + rng.integers(-noise, noise + 1, shape)
        jump = rng.random(shape[:3]) < 0.08                    # 8 % of the pixels show their other colour this frame
        f = np.where(jump[..., None] if ch == 3 else jump, alt + rng.integers(-3, 4, shape), f)
        f = np.clip(f, 0, 255).astype(np.uint8)
        if t > 0:
            for s in range(n):
                y, x = 5 + (3 * t + 7 * s) % (rows - 22), 6 + (5 * t + 11 * s) % (cols - 28)
                f[s, y:y + 14, x:x + 20] = (255, 64, 0) if ch == 3 else 250
        out.append(f)
    return out


@pytest.mark.parametrize("ch,restore,ring", [(3, 1, 4), (3, 0, 2), (1, 1, 3), (3, 1, 2)])
def test_two_frames_a_launch_equals_one_frame_a_launch(A, ch, restore, ring):
    """oatgpu_set_fusion: the pipelined path takes two consecutive frames on one pass over the model.  Every
    position and, at the end, the WHOLE model must be what one launch a frame gives -- and what the oracle gives."""
    rows, cols, n, nframes = 70, 200, 2, 41                    # an odd count: the last frame goes out alone
    rng = np.random.default_rng(100 * ch + 10 * restore + ring)
    kw = dict(n_streams=n, ring_depth=ring, adaptation_coeff=0.02, erode=2, dilate=4, area=(10.0, 1e6), channels=ch,
              mog_restore_nmodes=restore)
    if ch == 3:
        kw.update(h_thresh=(100, 125), s_thresh=(150, 256), v_thresh=(100, 256))
        p = O.hsv_params(h_lo=100, h_hi=125, s_lo=150, s_hi=256, v_lo=100, v_hi=256, erode=2, dilate=4, min_area=10.0,
                         max_area=1e6)
    else:
        kw.update(h_thresh=(200, 256))
        p = O.hsv_params(h_lo=200, h_hi=256, erode=2, dilate=4, min_area=10.0, max_area=1e6)
    frames = _noisy_sequence(rng, n, rows, cols, ch, nframes, noise=7)
    runs = {}
    for fusion in (1, 2):
        hp = A.HotPath(rows, cols, **kw)
        hp.set_fusion(fusion)
        hp.profile(1)
        got = []
        for f in frames:
            hp.enqueue(list(f))
            if hp.outstanding() >= ring:
                got.append(hp.collect())
        while hp.outstanding():
            got.append(hp.collect())
        prof = hp.profile_read()
        # fusion 2: frame 1 initialises the model (alone), then pairs, an odd one at the end
        # (a sample the profile took for a host stall -- oatgpu_profile.dropped -- is a step it does not count)
        assert nframes - 2 * prof["dropped"] <= prof["mog_frames"] <= nframes, prof
        assert prof["steps"] + prof["dropped"] == (nframes if fusion == 1 else 1 + (nframes - 1) // 2 + (nframes - 1) % 2), prof
        runs[fusion] = (got, [hp.mog_state(s) for s in range(n)], hp.read_mask(1, 0))
        hp.close()
    orcs = [O.Mog2(rows, cols, ch, params=dict(restore_nmodes=restore)) for _ in range(n)]
    hits = 0
    for t, f in enumerate(frames):
        for s in range(n):
            want, thr = O.chain_step(orcs[s], f[s], 0.02, p)
            for fusion in (1, 2):
                _same_detection(runs[fusion][0][t][s], want, (fusion, t, s))
            hits += want["valid"]
    assert hits >= nframes            # the block is found most of the time, in both streams
    assert (runs[1][2] == runs[2][2]).all()          # threshold image of the last frame, stream 0
    for s in range(n):
        _same_state(runs[2][1][s], orcs[s].state(), ("fused", s))
        for a, b in zip(runs[1][1][s][:4], runs[2][1][s][:4]):
            assert _eq(a, b)          # every slot of every plane, live or not


@pytest.mark.parametrize("ch,case", [(3, "tiny_rate"), (1, "tiny_rate"), (3, "wild_model"), (1, "wild_model"),
                                     (3, "wild_model_frozen"), (3, "ct_zero"), (3, "rate_then_zero")])
def test_launches_outside_the_in_range_division_stay_exact(A, ch, case):
    """r05: the product instantiations of the per-pixel kernel divide with an 8-instruction sequence that equals the IEEE
    division whenever no rescaling is needed (kernels_mog.hip, div_inrange).  The launcher sends everything else -- a rate
    below 2^-40, a complexity-reduction constant of 0, an imported model with weights no run produces -- through the
    instantiations that keep the compiler's division, one frame a launch.  Positions and the WHOLE model against the
    oracle, on the pipelined two-frames-a-launch path; 'rate_then_zero' is the in-range mixed pair (a rate, then 0)."""
    rows, cols, n, nframes = 70, 200, 2, 23
    rng = np.random.default_rng(77 + ch)
    lr = 1e-14 if case == "tiny_rate" else 0.02
    over = dict(ct=0.0) if case == "ct_zero" else {}
    kw = dict(n_streams=n, ring_depth=4, adaptation_coeff=lr, erode=2, dilate=4, area=(10.0, 1e6), channels=ch, **over)
    if ch == 3:
        kw.update(h_thresh=(100, 125), s_thresh=(150, 256), v_thresh=(100, 256))
        p = O.hsv_params(h_lo=100, h_hi=125, s_lo=150, s_hi=256, v_lo=100, v_hi=256, erode=2, dilate=4, min_area=10.0,
                         max_area=1e6)
    else:
        kw.update(h_thresh=(200, 256))
        p = O.hsv_params(h_lo=200, h_hi=256, erode=2, dilate=4, min_area=10.0, max_area=1e6)
    frames = _noisy_sequence(rng, n, rows, cols, ch, nframes, noise=7)
    hp = A.HotPath(rows, cols, **kw)
    hp.set_fusion(2)
    orcs = [O.Mog2(rows, cols, ch, params=over) for _ in range(n)]
    rates = [lr] * nframes
    if case == "rate_then_zero":
        rates = [lr if (t // 3) % 2 == 0 else 0.0 for t in range(nframes)]
    start = 0
    if case.startswith("wild_model"):
        # six ordinary frames, then every weight of stream 0's model scaled on both sides -- by 2^12 (weights of thousands: one
        # frame's renormalisation brings them back), or by 2^-80 under a frozen model (at a rate above 0 such weights are
        # pruned at once and the all-zero mixture's 0 * inf is NaN territory, where oracle and kernel were never pinned):
        # 1 / total then needs the rescaling the in-range sequence leaves out
        start = 6
        scale = np.float32(2.0 ** 12 if case == "wild_model" else 2.0 ** -80)
        if case == "wild_model_frozen":
            rates = [lr] * start + [0.0] * (nframes - start)
        for t in range(start):
            hp.learning_coeff_ = rates[t]
            hp.enqueue(list(frames[t]))
            got1 = hp.collect()
            for s in range(n):
                _same_detection(got1[s], O.chain_step(orcs[s], frames[t][s], rates[t], p)[0], ("warm", t, s))
        nm, w, v, m, nf = hp.mog_state(0)
        live = np.arange(w.shape[1])[None, :] < nm[:, None]
        w = np.where(live, w * scale, 0).astype(np.float32)
        v = np.where(live, v, 0).astype(np.float32); m = np.where(live[..., None], m, 0).astype(np.float32)
        hp.set_mog_state(nm, w, v, m, nf, stream=0)
        orcs[0].set_state(nm, w, v, m, nf)
    got = []
    for t in range(start, nframes):
        hp.learning_coeff_ = rates[t]
        hp.enqueue(list(frames[t]))
        if hp.outstanding() >= 4:
            got.append(hp.collect())
    while hp.outstanding():
        got.append(hp.collect())
    for i, t in enumerate(range(start, nframes)):
        for s in range(n):
            want, _ = O.chain_step(orcs[s], frames[t][s], rates[t], p)
            _same_detection(got[i][s], want, (case, t, s))
    for s in range(n):
        _same_state(hp.mog_state(s), orcs[s].state(), (case, s))
    hp.close()


@pytest.mark.parametrize("fusion", [1, 2])
def test_frozen_model_is_read_only_except_where_the_update_changes_bits(A, fusion):
    """Learning rate 0 (Oat's default) runs K1's FROZEN instantiations: a fitted record goes back to memory only when the
    update changed its bits.  With k = 0 it normally does not -- but a variance outside [varMin, varMax] is clamped, equal
    weights still swap, and weights that do not sum to 1 are renormalised: an imported model with all three must come out
    as the oracle's, masks and full model, through the synchronous and the pipelined (two frames a launch) path."""
    rng = np.random.default_rng(77)
    rows, cols = 41, 150
    n = rows * cols
    base = rng.integers(40, 200, (rows, cols, 3)).astype(np.int16)
    frames = [np.clip(base + rng.integers(-4, 5, base.shape), 0, 255).astype(np.uint8) for _ in range(9)]
    nm = np.full(n, 2, np.uint8)
    w = np.zeros((n, 5), np.float32); w[:, 0] = 0.45; w[:, 1] = 0.45           # equal weights, sum 0.9
    v = np.zeros((n, 5), np.float32); v[:, 0] = 100.0; v[:, 1] = 2.0            # outside the clamp [4, 75]
    m = np.zeros((n, 5, 3), np.float32)
    m[:, 0] = base.reshape(n, 3); m[:, 1] = 255 - base.reshape(n, 3)
    third = np.arange(n) % 3 == 0                                              # a third of the pixels: everyday, in-range model
    v[third, 0] = 15.0; w[third, 0] = 1.0; w[third, 1] = 0.0; nm[third] = 1; v[third, 1] = 0.0; m[third, 1] = 0.0
    # (r05) ... some of them with a blue mean of -0.f under blue pixels of 0: d = -0 - 0 = -0, k * d = -0, mean - (-0) = +0 --
    # the one way a rate-0 update of a sane-looking record changes bits.  (An imported model like this one is not PLAIN:
    # oatgpu_mog_set_state says so and the launches compute every update.)
    negz = third & (np.arange(n) % 15 == 0)
    m[negz, 0, 0] = -0.0
    for f in frames:
        f.reshape(n, 3)[negz, 0] = 0
    hp = A.HotPath(rows, cols, adaptation_coeff=0.0, dilate=3, ring_depth=8)
    hp.set_fusion(fusion)
    orc = O.Mog2(rows, cols)
    hp.track([frames[0]]); orc.apply(frames[0], 0.0)                           # (a first frame: geometry, frame counter)
    hp.set_mog_state(nm, w, v, m, 5)
    orc.set_state(nm, w, v, m, 5)
    if fusion == 1:
        for f in frames[1:]:
            hp.track([f])
    else:
        for f in frames[1:]:
            hp.enqueue([f])
        for _ in frames[1:]:
            hp.collect()
    for f in frames[1:]:
        orc.apply(f, 0.0)
    _same_state(hp.mog_state(), orc.state(), ("frozen", fusion))
    gv = hp.mog_state()[2]
    assert (gv[~third, 0] == 75.0).all() and (gv[third, 0] == 15.0).all()       # the clamp acted on the fitted mode, and was stored
    gm = hp.mog_state()[3]
    assert not np.signbit(gm[negz, 0, 0]).any()                                  # -0.f became +0.f, as in the reference


def test_two_frames_a_launch_with_changing_rates_and_early_collects(A):
    """The second frame of a launch carries its own learning rate (automatic 1/min(2n, history), fixed, 0, and >= 1 =
    re-initialise, which is never paired); collects that reach a frame still only registered send it off alone."""
    rows, cols, n = 48, 130, 2
    rng = np.random.default_rng(77)
    rates = [-1.0, -1.0, -1.0, 0.01, 0.3, 0.0, 0.0, 0.05, 1.0, 0.05, 0.05, -1.0, 0.2, 0.2, 1.5, -1.0, 0.01, 0.01, 0.01,
             0.5, 0.0, 0.1, 0.1]
    frames = _noisy_sequence(rng, n, rows, cols, 3, len(rates), noise=9)
    win = dict(h_thresh=(100, 125), s_thresh=(150, 256), v_thresh=(100, 256))
    hp = A.HotPath(rows, cols, n_streams=n, ring_depth=3, erode=0, dilate=3, area=(5.0, 1e6), **win)
    p = O.hsv_params(h_lo=100, h_hi=125, s_lo=150, s_hi=256, v_lo=100, v_hi=256, erode=0, dilate=3, min_area=5.0, max_area=1e6)
    orcs = [O.Mog2(rows, cols, 3) for _ in range(n)]
    # after which enqueues everything outstanding is drained (so that frames go out alone, in pairs, alone ...)
    drain_after = {0, 3, 4, 9, 10, 11, 17}
    got = []
    for t, (f, lr) in enumerate(zip(frames, rates)):
        hp.learning_coeff_ = lr
        hp.enqueue(list(f))
        if t in drain_after:
            while hp.outstanding():
                got.append(hp.collect())
        elif hp.outstanding() >= 3:
            got.append(hp.collect())
        if t == 12:                                           # a synchronous tap in between: the last ENQUEUED frame's mask
            want_thr = None
            oc = [O.Mog2(rows, cols, 3) for _ in range(1)]
            for tt in range(13):
                _, want_thr = O.chain_step(oc[0], frames[tt][0], rates[tt], p)
            assert (hp.read_mask(1, 0) == want_thr).all()
    while hp.outstanding():
        got.append(hp.collect())
    assert len(got) == len(rates)
    for t, (f, lr) in enumerate(zip(frames, rates)):
        for s in range(n):
            want, _ = O.chain_step(orcs[s], f[s], lr, p)
            _same_detection(got[t][s], want, (t, s))
    for s in range(n):
        _same_state(hp.mog_state(s), orcs[s].state(), s)


def test_homography_behind_detector_and_kalman(A):
    """oatgpu_set_homography (`posifilt homography`, HomographyTransform2D.cpp:62-107) on the batch: behind the detector
    alone and behind the position filter (velocity through the matrix without its offsets); raw_x / raw_y keep pixels."""
    from oat_amd.synth import SyntheticStream
    rows, cols, n = 120, 200, 2
    H = [0.02, 0.001, -1.5, -0.002, 0.025, 0.75, 1e-4, -2e-4, 1.0]
    win = dict(h_thresh=(100, 125), s_thresh=(150, 256), v_thresh=(100, 256))
    p = O.hsv_params(h_lo=100, h_hi=125, s_lo=150, s_hi=256, v_lo=100, v_hi=256, erode=3, dilate=7, min_area=20.0, max_area=1e5)
    streams = [SyntheticStream(rows, cols, 20 + s, n_discs=1, radius=10) for s in range(n)]
    frames = [[st.frame(t, with_discs=t > 0) for st in streams] for t in range(30)]
    for kalman in (False, True):
        hp = A.HotPath(rows, cols, n_streams=n, adaptation_coeff=0.01, erode=3, dilate=7, area=(20.0, 1e5), ring_depth=4, **win)
        if kalman:
            hp.set_kalman(True, dt=0.02, timeout=0.1, sigma_accel=5.0, sigma_noise=1.0)
        hp.set_homography(H)
        orcs = [O.Mog2(rows, cols, 3) for _ in range(n)]
        kfs = [O.Kalman(dt=0.02, timeout=0.1, sigma_accel=5.0, sigma_noise=1.0) for _ in range(n)] if kalman else None
        got = []
        for f in frames:
            hp.enqueue(f)
            if hp.outstanding() >= 4:
                got.append(hp.collect())
        while hp.outstanding():
            got.append(hp.collect())
        hits = 0
        for t, f in enumerate(frames):
            for s in range(n):
                want, _ = O.chain_step(orcs[s], f[s], 0.01, p)
                g = got[t][s]
                if kalman:
                    k = kfs[s].filter(want["valid"], want["x"], want["y"])
                    x, y, vx, vy = O.homography(H, k["position_valid"], k["x"], k["y"], k["velocity_valid"], k["vx"], k["vy"])
                    assert g.position_valid == k["position_valid"] and g.velocity_valid == k["velocity_valid"], (t, s)
                    if k["position_valid"]:
                        assert (g.x, g.y, g.vx, g.vy) == (x, y, vx, vy), (t, s)
                        hits += 1
                else:
                    assert g.position_valid == want["valid"], (t, s)
                    if want["valid"]:
                        x, y, _, _ = O.homography(H, True, want["x"], want["y"])
                        assert (g.x, g.y) == (x, y) and (g.raw_x, g.raw_y) == (want["x"], want["y"]), (t, s, g, want)
                        hits += 1
        assert hits >= 40
        hp.set_homography(None)
        hp.close()


def test_set_fusion_arguments_and_switching_with_a_frame_registered(A):
    """oatgpu_set_fusion takes 1 or 2; switching while a frame is only registered sends that frame off first, and the
    results stay those of one launch a frame."""
    from oat_amd import ffi
    rows, cols = 40, 96
    rng = np.random.default_rng(3)
    frames = _noisy_sequence(rng, 1, rows, cols, 3, 12, noise=6)
    win = dict(h_thresh=(100, 125), s_thresh=(150, 256), v_thresh=(100, 256))
    hp = A.HotPath(rows, cols, n_streams=1, ring_depth=4, adaptation_coeff=0.05, erode=0, dilate=3, area=(5.0, 1e6), **win)
    ref = A.HotPath(rows, cols, n_streams=1, ring_depth=4, adaptation_coeff=0.05, erode=0, dilate=3, area=(5.0, 1e6), **win)
    ref.set_fusion(1)
    for bad in (0, 3, -1):
        with pytest.raises(ffi.OatGpuError, match="frames_per_launch must be 1 or 2"):
            hp.set_fusion(bad)
    got = []
    for t, f in enumerate(frames):
        hp.enqueue(list(f))
        if t in (2, 7):
            hp.set_fusion(1 if t == 2 else 2)          # frame t is registered, not launched, at this point
        if hp.outstanding() >= 3:
            got.append(hp.collect())
    while hp.outstanding():
        got.append(hp.collect())
    want = [ref.track(list(f)) for f in frames]
    assert got == want
    for a, b in zip(hp.mog_state()[:4], ref.mog_state()[:4]):
        assert _eq(np.asarray(a), np.asarray(b))


# ------------------------------------------- round 3: frame lifetime, repairs under single-stage calls --

def _frames_per_launch(hp, run):
    hp.profile(1)
    hp.profile_reset()
    run()
    p = hp.profile_read()
    hp.profile(0)
    return p["mog_frames"] / max(p["steps"], 1)


def test_default_fusion_pairs_only_where_the_library_owns_the_frames(A):
    """oatgpu_set_fusion's default: host frames (copied to a staging slot) and track_sequence_dev (all frames in hand)
    take two frames a launch; oatgpu_track_enqueue_dev queues its kernel inside the call -- one frame a launch --
    until oatgpu_set_fusion(2) opts in."""
    import torch
    rows, cols = 96, 128
    rng = np.random.default_rng(3)
    frames = [rng.integers(0, 256, (1, rows, cols, 3)).astype(np.uint8) for _ in range(9)]
    bufs = [torch.from_numpy(f).cuda() for f in frames]
    torch.cuda.synchronize()

    def mk():
        hp = A.HotPath(rows, cols, n_streams=1, ring_depth=4, adaptation_coeff=0.02, dilate=3)
        hp.track(list(frames[0]))
        return hp

    def dev_loop(hp):
        def run():
            for b in bufs[1:]:
                hp.enqueue_dev(b.data_ptr(), keepalive=b)
                if hp.outstanding() == 4:
                    hp.collect()
            while hp.outstanding():
                hp.collect()
        return run

    def host_loop(hp):
        def run():
            for f in frames[1:]:
                hp.enqueue(list(f))
                if hp.outstanding() == 4:
                    hp.collect()
            while hp.outstanding():
                hp.collect()
        return run
    hp = mk()
    assert _frames_per_launch(hp, dev_loop(hp)) == 1.0
    hp = mk()
    hp.set_fusion(2)
    assert _frames_per_launch(hp, dev_loop(hp)) == 2.0
    hp = mk()
    assert _frames_per_launch(hp, host_loop(hp)) == 2.0
    hp = mk()
    assert _frames_per_launch(hp, lambda: hp.track_sequence_dev([b.data_ptr() for b in bufs[1:]])) == 2.0
    hp = mk()
    hp.set_fusion(1)
    assert _frames_per_launch(hp, host_loop(hp)) == 1.0


def test_device_buffer_reused_in_stream_order_and_input_consumed(A):
    """(1) Default: a caller that refills ONE device buffer on the context's stream between enqueue_dev calls gets
    the right results (the kernel was queued inside the call).  (2) With oatgpu_set_fusion(2) the buffer may be
    overwritten once oatgpu_track_input_consumed returned (the registered frame is launched first)."""
    import torch
    from oat_amd.synth import disc_hsv_window
    rows, cols, nfr = 120, 160, 14
    rng = np.random.default_rng(5)
    frames = _noisy_sequence(rng, 1, rows, cols, 3, nfr, 8)
    kw = dict(n_streams=1, ring_depth=4, adaptation_coeff=0.02, erode=0, dilate=3, area=(4.0, 1e9), **disc_hsv_window())
    ref = A.HotPath(rows, cols, **kw)
    want = [ref.track(list(f)) for f in frames]
    pinned = [torch.from_numpy(f).pin_memory() for f in frames]
    for fusion in (None, 2):
        hp = A.HotPath(rows, cols, **kw)
        if fusion:
            hp.set_fusion(fusion)
        buf = torch.empty((1, rows, cols, 3), dtype=torch.uint8, device="cuda:0")
        st = torch.cuda.ExternalStream(hp.get_stream(), device=torch.device("cuda:0"))
        got = []
        for t in range(nfr):
            if fusion:
                hp.input_consumed()                      # the kernel that read `buf` has finished (launches a registered frame)
            with torch.cuda.stream(st):
                buf.copy_(pinned[t], non_blocking=True)  # stream order on the context's own stream
            hp.enqueue_dev(buf.data_ptr())
            if hp.outstanding() == 3:
                got.append(hp.collect())
        while hp.outstanding():
            got.append(hp.collect())
        assert got == want, fusion
        nm_a, w_a, v_a, m_a, _ = hp.mog_state(0)
        nm_b, w_b, v_b, m_b, _ = ref.mog_state(0)
        assert (nm_a == nm_b).all() and (w_a == w_b).all() and (v_a == v_b).all() and (m_a == m_b).all()


def test_declined_frame_survives_single_stage_calls_and_ready(A):
    """A frame the single-workgroup LDS kernel declined is redone by the global kernels from the threshold bits in
    its ring slot.  A single-stage call made while it is outstanding writes ITS threshold bits into slot 0's buffer:
    the quiesce() in front of it must have redone the frame by then.  oatgpu_track_ready on such a
    frame starts the redo and reports 0 until it is done; collect then hands out the oracle's result."""
    import time
    rows, cols = 240, 320
    rng = np.random.default_rng(12)
    win = dict(h_thresh=(100, 125), s_thresh=(150, 256), v_thresh=(100, 256))
    p = O.hsv_params(h_lo=100, h_hi=125, s_lo=150, s_hi=256, v_lo=100, v_hi=256, erode=0, dilate=2, min_area=4.0, max_area=1e9)
    base = rng.integers(90, 140, (rows, cols, 3)).astype(np.int16)

    def frame(t, busy):
        f = np.clip(base + rng.integers(-5, 6, base.shape), 0, 255).astype(np.uint8)
        if t > 0:
            f[60:80, 70 + 3 * t:95 + 3 * t] = (255, 64, 0)
            if busy:
                f[rng.random((rows, cols)) < 0.08] = (255, 64, 0)
        return f
    hsv_probe = O.bgr2hsv(frame(1, False))
    for use_ready in (False, True):
        hp = A.HotPath(rows, cols, n_streams=1, ring_depth=4, adaptation_coeff=0.01, erode=0, dilate=2, area=(4.0, 1e9), **win)
        orc = O.Mog2(rows, cols, 3)
        frames = [frame(t, False) for t in range(5)]
        for f in frames[:4]:
            got = hp.track([f])[0]
            _same_detection(got, O.chain_step(orc, f, 0.01, p)[0], "warm")
        busy = frame(5, True)
        calm = frame(6, False)
        # the busy frame lands in ring slot 0 (four synchronous steps went before it: 4 % 4 == 0)
        hp.enqueue([busy])
        hp.enqueue([calm])
        if use_ready:
            t0 = time.perf_counter()
            while not hp.ready():
                assert time.perf_counter() - t0 < 10.0
                time.sleep(0.0005)
        else:
            import ctypes as C
            from oat_amd import ffi
            out = ffi.Position()                     # a single-stage call on the SAME context: writes slot 0's buffer
            assert hp.lib.oatgpu_detect_hsv(hp.ctx, 0, ffi.u8(np.ascontiguousarray(hsv_probe)), C.byref(out)) == 0
        r1 = hp.collect()[0]
        r2 = hp.collect()[0]
        _same_detection(r1, O.chain_step(orc, busy, 0.01, p)[0], ("busy", use_ready))
        _same_detection(r2, O.chain_step(orc, calm, 0.01, p)[0], ("calm", use_ready))


def test_device_count_and_numa_node(A):
    """oatgpu_device_count / oatgpu_device_numa_node: what the multi-device tracker pins its shard threads by."""
    from oat_amd import ffi
    lib = ffi.load()
    n = lib.oatgpu_device_count()
    assert n >= 1
    node = lib.oatgpu_device_numa_node(0)
    assert node >= -1
    if node >= 0:
        assert os.path.exists(f"/sys/devices/system/node/node{node}/cpulist")
    assert lib.oatgpu_device_numa_node(n + 5) == -1


@pytest.mark.parametrize("ring", [2, 3, 5, 8])
@pytest.mark.parametrize("geom", [(96, 200, 3), (480, 640, 1)])
def test_paired_back_half_equals_one_frame_a_launch_and_the_oracle(A, ring, geom):
    """Round 5: outside the early order both frames of a two-frame step share ONE row-scan launch and ONE k_blob_lds launch
    (grid z = frame; steps alternate between two B streams with two scratch sets each).  Quiet and BUSY frames (busy = the LDS
    kernel declines the frame -> repaired by the global kernels in the REPAIR set (scratch set 4, on B2); then the plain order until
    the streak is back -> a switch of paths with a drain), even and odd ring depths, one and several streams, an odd number of
    frames (the last one goes out alone): every result equals one frame a launch (the per-frame plain order) and the oracle;
    the step shape query says what ran."""
    import torch
    rows, cols, n = geom
    rng = np.random.default_rng(ring * 7 + n)
    win = dict(h_thresh=(100, 125), s_thresh=(150, 256), v_thresh=(100, 256))
    kw = dict(n_streams=n, ring_depth=ring, adaptation_coeff=0.01, erode=3, dilate=5, area=(8.0, 1e6), **win)
    hp, ref = A.HotPath(rows, cols, **kw), A.HotPath(rows, cols, **kw)
    hp.set_fusion(2)
    ref.set_fusion(1)
    p = O.hsv_params(h_lo=100, h_hi=125, s_lo=150, s_hi=256, v_lo=100, v_hi=256, erode=3, dilate=5, min_area=8.0, max_area=1e6)
    orc = [O.Mog2(rows, cols, 3) for _ in range(n)]
    base = rng.integers(90, 150, (n, rows, cols, 3)).astype(np.int16)

    def frame(t, busy):
        f = np.clip(base + rng.integers(-5, 6, base.shape), 0, 255).astype(np.uint8)
        if t > 0:
            for s_ in range(n):
                cy, cx = 8 + (7 * t + 11 * s_) % (rows - 40), 9 + (11 * t + 17 * s_) % (cols - 60)
                f[s_, cy:cy + 14, cx:cx + 21] = (255, 64, 0)
                if busy:                                             # specks of the blob colour: far more runs than the LDS kernel takes
                    f[s_][rng.random((rows, cols)) < (0.25 if rows < 200 else 0.02)] = (255, 64, 0)
        return f
    # (6, 7) and (28, 29): BOTH frames of a paired step busy -- the second one is collected, and repaired, after later steps have gone
    # out in the plain order: its repair must not touch a scratch set those use from another stream (tools/fuzz.py --seed 11,
    # configuration 301, found exactly that in the first cut: repairs now have a set and a stream of their own)
    pattern = [0] * 6 + [1, 1, 0, 1, 1, 0] + [0] * 16 + [1, 1] + [0] * 4 + [1]        # 35 frames: odd
    frames = [frame(t, b) for t, b in enumerate(pattern)]
    dev = [torch.from_numpy(f).cuda() for f in frames]
    torch.cuda.synchronize()

    def run(h):
        out = []
        for d in dev:
            h.enqueue_dev(d.data_ptr(), keepalive=d)
            if h.outstanding() >= ring:
                out.append(h.collect())
        while h.outstanding():
            out.append(h.collect())
        return out
    got, plain = run(hp), run(ref)
    assert len(got) == len(frames) and got == plain
    for t, f in enumerate(frames):
        for s_ in range(n):
            _same_detection(got[t][s_], O.chain_step(orc[s_], f[s_], 0.01, p)[0], (t, s_, pattern[t]))
    for s_ in range(n):
        assert (hp.read_mask(A.ffi.TAP_MORPH, s_) == ref.read_mask(A.ffi.TAP_MORPH, s_)).all()
        assert (hp.read_mask(A.ffi.TAP_FINAL, s_) == ref.read_mask(A.ffi.TAP_FINAL, s_)).all()
        _same_state(hp.mog_state(s_), orc[s_].state(), s_)
    wg, early = hp.last_step_shape()
    assert wg in (64, 256) and early is False                       # (well below 4 MP a step: never the early order)
    assert hp.early_blob_timeouts() == 0
    hp.close(); ref.close()


def test_abi8_plumbing_k1_workgroup_latency_sequence_and_open_retries(A):
    """oatgpu_set_k1_workgroup (results identical whatever the workgroup size; oatgpu_last_step_shape reports it),
    oatgpu_track_sequence_dev_latency (hand-over before collection, both ascending), oatgpu_device_open_retries."""
    import ctypes as C
    import torch
    rows, cols = 120, 256
    from oat_amd.synth import SyntheticStream, disc_hsv_window
    st = SyntheticStream(rows, cols, 5, n_discs=1, radius=9)
    frames = [torch.from_numpy(st.frame(t, with_discs=t > 0)[None].copy()).cuda() for t in range(21)]
    torch.cuda.synchronize()
    outs = []
    for wg in (0, 64, 256):
        hp = A.HotPath(rows, cols, n_streams=1, ring_depth=4, adaptation_coeff=0.01, erode=3, dilate=5, area=(5.0, 1e5), **disc_hsv_window())
        hp.set_k1_workgroup(wg)
        res = hp.track_sequence_dev([f.data_ptr() for f in frames])
        outs.append([(r[0].position_valid, r[0].a00, r[0].a10, r[0].a01, r[0].first_pixel) for r in res])
        if wg:
            assert hp.last_step_shape()[0] == wg
        hp.close()
    assert outs[0] == outs[1] == outs[2] and sum(o[0] for o in outs[0]) >= 15
    hp = A.HotPath(rows, cols, n_streams=1, ring_depth=4, adaptation_coeff=0.01, erode=3, dilate=5, area=(5.0, 1e5), **disc_hsv_window())
    with pytest.raises(A.ffi.OatGpuError):
        hp.set_k1_workgroup(128)
    n = len(frames)
    arr = (C.c_void_p * n)(*[f.data_ptr() for f in frames])
    out = (A.ffi.Position * n)()
    done, enq = (C.c_double * n)(), (C.c_double * n)()
    A.ffi.check(hp.lib, hp.ctx, hp.lib.oatgpu_track_sequence_dev_latency(hp.ctx, arr, n, 0.01, out, done, enq))
    d, e = list(done), list(enq)
    assert all(e[i] <= d[i] for i in range(n)) and d == sorted(d) and e == sorted(e) and e[0] >= 0.0
    assert all(e[i + 4] >= d[i] for i in range(n - 4))              # ring depth 4: frame i + 4 is handed over after frame i was collected
    assert [(o.valid, o.a00) for o in out] == [(v, a) for v, a, *_ in outs[0]]
    # (the counter is the process's: >= 0, and it does not move while this context -- long since open -- works; a sibling process
    # opening the device at the same instant is exactly what the retry absorbs, so "== 0" was the wrong assertion: ADVICE r05)
    r0 = hp.lib.oatgpu_device_open_retries()
    assert r0 >= 0
    hp.track_dev(frames[0].data_ptr())
    assert hp.lib.oatgpu_device_open_retries() == r0
    p = hp.profile_read()
    assert set(p) >= {"steps", "mog_ms", "mog_frames", "dropped"} and p["dropped"] == 0          # (profiling was never on here)
    hp.close()
