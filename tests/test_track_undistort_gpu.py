"""GPU tests of `framefilt undistort` inside the fused tracker (oatgpu_set_track_undistort, HotPath.undistort): the chain
undistort -> mask -> mog -> col -> posidet -> posifilt kalman -> posifilt homography in one context, against the oracle chain
fed the numpy restatement's undistorted frames (tests/undistort_ref.py), against the two-step form (oatgpu_undistort_dev
into a buffer, then a plain context), on every entry path, and in a process pipeline."""
import json
import os
import subprocess
import uuid

import numpy as np
import pytest

import oracle_lib as O
import undistort_ref as R

pytestmark = pytest.mark.gpu

HSV_WIN = dict(h_thresh=(100, 125), s_thresh=(150, 256), v_thresh=(100, 256))
HSV_P = dict(h_lo=100, h_hi=125, s_lo=150, s_hi=256, v_lo=100, v_hi=256)
LR = 0.01


def _maps(rows, cols, name):
    K, D = R.cases(rows, cols)[name]
    return (K, D), R.undistort_map(rows, cols, K, D)


def _frames(rows, cols, ch, n_streams, T, seed=0, radius=None):
    """[T][n_streams] frames with moving discs (BGR), or their GREY conversion."""
    from oat_amd.synth import SyntheticStream
    sts = [SyntheticStream(rows, cols, seed + s, n_discs=1, radius=radius) for s in range(n_streams)]
    out = []
    for t in range(T):
        fs = [st.frame(t, with_discs=t > 0) for st in sts]
        out.append([O.bgr2grey(f) if ch == 1 else f for f in fs])
    return out


def _hp(rows, cols, n, ch, **kw):
    import oat_amd
    if ch == 1:
        return oat_amd.HotPath(rows, cols, n_streams=n, channels=1, adaptation_coeff=LR, h_thresh=(30, 110), erode=3,
                               dilate=7, area=(20.0, 1e6), **kw)
    return oat_amd.HotPath(rows, cols, n_streams=n, adaptation_coeff=LR, erode=3, dilate=7, area=(20.0, 1e6), **HSV_WIN, **kw)


def _oracle_p(ch):
    if ch == 1:
        return O.hsv_params(h_lo=30, h_hi=110, erode=3, dilate=7, min_area=20.0, max_area=1e6)
    return O.hsv_params(**HSV_P, erode=3, dilate=7, min_area=20.0, max_area=1e6)


def _pos(p):
    return tuple(vars(p).values())


def _same_model(a, b, tag):
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True), tag


def _same_model_oracle(gpu, ora, tag):
    nm_g, w_g, v_g, m_g, _ = gpu
    nm_o, w_o, v_o, m_o = ora
    assert (nm_g == nm_o).all(), tag
    live = np.arange(w_o.shape[1])[None, :] < nm_o[:, None]
    for g, o in ((w_g, w_o), (v_g, v_o), (m_g, m_o)):
        assert np.array_equal(g[live].view(np.uint32), o[live].view(np.uint32)), tag


def _taps(hp, n):
    from oat_amd import ffi
    return [[hp.read_mask(w, s) for w in (ffi.TAP_THRESHOLD, ffi.TAP_MORPH, ffi.TAP_FINAL)] for s in range(n)]


# --------------------------------------------------------------------------- 1: parity with the restatement --

@pytest.mark.parametrize("rows,cols", [(480, 640), (1080, 1920), (150, 328)])
@pytest.mark.parametrize("ch", [3, 1])
def test_parity_with_the_oracle_chain_on_undistorted_frames(rows, cols, ch):
    cal, (m1, m2) = _maps(rows, cols, "mild5")
    hp = _hp(rows, cols, 1, ch, undistort=cal)
    orc, p = O.Mog2(rows, cols, ch), _oracle_p(ch)
    hits = 0
    try:
        for t, fs in enumerate(_frames(rows, cols, ch, 1, 30, seed=3, radius=max(8, rows // 25))):
            got = hp.track(fs)[0]
            uf = R.remap(fs[0], m1, m2)
            want, thr = O.chain_step(orc, uf, LR, p)
            assert np.array_equal(hp.read_mask(1, 0), thr), t
            assert got.position_valid == want["valid"], t
            if want["valid"]:
                hits += 1
                assert (got.a00, got.a10, got.a01) == (want["a00"], want["a10"], want["a01"]), t
                assert abs(got.x - want["x"]) <= 1e-4 and abs(got.y - want["y"]) <= 1e-4, t
        _same_model_oracle(hp.mog_state(), orc.state(), (rows, cols, ch))
    finally:
        hp.close()
    assert hits >= 20, hits


# ------------------------------------------------------------------------- 2: oracle-free equivalence --

def _two_step(rows, cols, n, ch, cals, frames, setup=None):
    """oatgpu_undistort_dev into a buffer, then a plain context on that buffer: positions, model and taps a step."""
    import torch
    import oat_amd
    ud = oat_amd.Undistorter(rows, cols, *cals[0], channels=ch, n_streams=n)
    hp = _hp(rows, cols, n, ch)
    if setup:
        setup(hp)
    out = []
    try:
        for s in range(n):
            ud.set_calibration(s, *cals[s])
        for fs in frames:
            fin = torch.from_numpy(np.stack(fs)).cuda()
            fout = torch.empty_like(fin)
            torch.cuda.synchronize()
            ud.filter_dev(fin.data_ptr(), fout.data_ptr())
            ud.synchronize()
            out.append([_pos(p) for p in hp.track_dev(fout.data_ptr())])
        return out, [hp.mog_state(s) for s in range(n)], _taps(hp, n)
    finally:
        ud.close()
        hp.close()


@pytest.mark.parametrize("ch", [3, 1])
def test_equals_undistort_dev_then_a_plain_context(ch):
    import torch
    rows, cols, n, T = 1080, 1920, 2, 24
    cals = [R.cases(rows, cols)[k] for k in ("mild5", "rational8")]
    frames = _frames(rows, cols, ch, n, T, seed=7, radius=30)
    want, want_model, want_taps = _two_step(rows, cols, n, ch, cals, frames)
    hp = _hp(rows, cols, n, ch, undistort=cals)
    try:
        got = []
        for fs in frames:
            fin = torch.from_numpy(np.stack(fs)).cuda()
            torch.cuda.synchronize()
            got.append([_pos(p) for p in hp.track_dev(fin.data_ptr())])
        assert got == want
        for s in range(n):
            _same_model(hp.mog_state(s), want_model[s], s)
        for s, (g, w) in enumerate(zip(_taps(hp, n), want_taps)):
            for k in range(3):
                assert np.array_equal(g[k], w[k]), (s, k)
    finally:
        hp.close()
    assert sum(p[0] for fs in want for p in fs) >= n * (T - 3)


# ---------------------------------------------------------------------- 3: one calibration per stream --

def test_three_streams_three_calibrations():
    rows, cols, n = 480, 640, 3
    names = ("mild5", "rational8", "skew")
    cals = [R.cases(rows, cols)[k] for k in names]
    maps = [R.undistort_map(rows, cols, *c) for c in cals]
    hp = _hp(rows, cols, n, 3, undistort=cals)
    orcs, p = [O.Mog2(rows, cols, 3) for _ in range(n)], _oracle_p(3)
    hits = 0
    try:
        for t, fs in enumerate(_frames(rows, cols, 3, n, 20, seed=11, radius=14)):
            got = hp.track(fs)
            for s in range(n):
                want, thr = O.chain_step(orcs[s], R.remap(fs[s], *maps[s]), LR, p)
                assert np.array_equal(hp.read_mask(1, s), thr), (t, s)
                assert got[s].position_valid == want["valid"], (t, s)
                if want["valid"]:
                    hits += 1
                    assert (got[s].a00, got[s].a10, got[s].a01) == (want["a00"], want["a10"], want["a01"]), (t, s)
        for s in range(n):
            _same_model_oracle(hp.mog_state(s), orcs[s].state(), s)
    finally:
        hp.close()
    assert hits >= 40


# ----------------------------------------------------------------------------- 4: every entry path --

def _run_path(path, rows, cols, n, ch, cal, frames):
    """positions of every frame + the final model, through one entry path with the switch on; the path's step shape."""
    import torch
    hp = _hp(rows, cols, n, ch, undistort=cal)
    res, shape = [], None
    dev = [torch.from_numpy(np.stack(fs)).cuda() for fs in frames] if path in ("batch_dev", "enq_dev1", "enq_dev2",
                                                                            "sequence") else None
    torch.cuda.synchronize()
    try:
        if path == "batch":
            res = [[_pos(p) for p in hp.track(fs)] for fs in frames]
        elif path == "batch_dev":
            res = [[_pos(p) for p in hp.track_dev(d.data_ptr())] for d in dev]
        elif path in ("enq_dev1", "enq_dev2"):
            hp.set_fusion(1 if path == "enq_dev1" else 2)
            for d in dev:
                if hp.outstanding() == 2:
                    res.append([_pos(p) for p in hp.collect()])
                hp.enqueue_dev(d.data_ptr(), keepalive=d)
            while hp.outstanding():
                res.append([_pos(p) for p in hp.collect()])
        elif path in ("enqueue", "staged_dma", "staged_kernel"):
            if path == "staged_kernel":
                hp.set_stage_copy(1)
            for fs in frames:
                if hp.outstanding() == 2:
                    res.append([_pos(p) for p in hp.collect()])
                if path == "enqueue":
                    hp.enqueue(fs)
                else:
                    for s, f in enumerate(fs):
                        hp.stage(s, f)
                    hp.enqueue_staged()
            while hp.outstanding():
                res.append([_pos(p) for p in hp.collect()])
        elif path == "sequence":
            res = [[_pos(p) for p in fs] for fs in hp.track_sequence_dev([d.data_ptr() for d in dev])]
            shape = hp.last_step_shape()
        if path == "batch":
            shape = hp.last_step_shape()
        return res, [hp.mog_state(s) for s in range(n)], shape
    finally:
        hp.close()


@pytest.mark.parametrize("rows,cols,n,ch,T", [(1080, 1920, 1, 3, 16), (480, 640, 3, 1, 16)])
def test_every_entry_path_gives_identical_results(rows, cols, n, ch, T):
    """track_batch (a lone frame: the inline back half), _batch_dev, _enqueue_dev with fusion 1 and 2 (one 1080p stream,
    two frames a launch: the paired order), _enqueue (host), staged with both copy modes, _sequence_dev."""
    cal = R.cases(rows, cols)["mild5"]
    frames = _frames(rows, cols, ch, n, T, seed=5, radius=20)
    want, want_model, _ = _run_path("batch", rows, cols, n, ch, cal, frames)
    for path in ("batch_dev", "enq_dev1", "enq_dev2", "enqueue", "staged_dma", "staged_kernel", "sequence"):
        got, model, _ = _run_path(path, rows, cols, n, ch, cal, frames)
        assert got == want, path
        for s in range(n):
            _same_model(model[s], want_model[s], (path, s))
    assert sum(p[0] for fs in want for p in fs) >= n * (T - 3)


def test_4k_device_frames_take_the_early_order():
    rows, cols, T = 2160, 3840, 10
    cal = R.cases(rows, cols)["rational8"]
    frames = _frames(rows, cols, 3, 1, T, seed=2, radius=60)
    want, want_model, _ = _run_path("batch", rows, cols, 1, 3, cal, frames)
    got, model, (wg, early) = _run_path("sequence", rows, cols, 1, 3, cal, frames)
    assert early, "4K x 1 device frames: the early order"
    assert got == want
    _same_model(model[0], want_model[0], "4K")
    assert sum(p[0] for fs in want for p in fs) >= T - 2


# ------------------------------------------------------------------ 5: ROI, Kalman and homography --

def test_roi_kalman_and_homography_with_the_switch_on():
    """The ROI mask applies to the UNDISTORTED image: the fused context equals undistort_dev + a plain context with the
    same mask, Kalman filter and homography."""
    import torch
    rows, cols, n, T = 480, 640, 2, 24
    cals = [R.cases(rows, cols)[k] for k in ("barrel", "mild5")]
    yy, xx = np.mgrid[0:rows, 0:cols]
    roi = (((xx - 330) ** 2 + (yy - 230) ** 2) < 190 ** 2).astype(np.uint8) * 255
    H = [0.01, 0.0002, -3.0, -0.0001, 0.012, -2.0, 1e-6, 2e-6, 1.0]

    def setup(hp):
        hp.set_roi_mask(roi, stream=0)
        hp.set_kalman(True, dt=0.02, timeout=1.0, sigma_accel=5.0, sigma_noise=0.5)
        hp.set_homography(H)

    frames = _frames(rows, cols, 3, n, T, seed=13, radius=14)
    want, want_model, want_taps = _two_step(rows, cols, n, 3, cals, frames, setup)
    hp = _hp(rows, cols, n, 3, undistort=cals)
    setup(hp)
    try:
        got = []
        for fs in frames:
            fin = torch.from_numpy(np.stack(fs)).cuda()
            torch.cuda.synchronize()
            got.append([_pos(p) for p in hp.track_dev(fin.data_ptr())])
        assert got == want
        for s in range(n):
            _same_model(hp.mog_state(s), want_model[s], s)
            assert np.array_equal(hp.read_mask(2, s), want_taps[s][2]), s
    finally:
        hp.close()
    assert sum(p[11] for fs in want for p in fs) >= T and any(p[8] for fs in want for p in fs)   # detected, filtered


# --------------------------------------------------------------------------------- 6: checkpoint/resume --

def test_checkpoint_and_resume_continue_bit_identically(tmp_path):
    rows, cols, n = 480, 640, 2
    cals = [R.cases(rows, cols)[k] for k in ("rational8", "skew")]
    frames = _frames(rows, cols, 3, n, 24, seed=17, radius=14)
    a = _hp(rows, cols, n, 3, undistort=cals)
    b = _hp(rows, cols, n, 3, undistort=cals)
    try:
        for fs in frames[:12]:
            a.track(fs)
        for s in range(n):
            a.save_mog_state(str(tmp_path / f"m{s}.mog"), stream=s)
            b.load_mog_state(str(tmp_path / f"m{s}.mog"), stream=s)
        for t, fs in enumerate(frames[12:]):
            assert [_pos(p) for p in a.track(fs)] == [_pos(p) for p in b.track(fs)], t
        for s in range(n):
            _same_model(a.mog_state(s), b.mog_state(s), s)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------ 7: the off path --

def test_maps_with_the_switch_off_change_nothing():
    rows, cols, n = 480, 640, 2
    cals = [R.cases(rows, cols)[k] for k in ("barrel", "pincushion")]
    frames = _frames(rows, cols, 3, n, 16, seed=19, radius=14)
    plain = _hp(rows, cols, n, 3)
    mapped = _hp(rows, cols, n, 3)
    toggled = _hp(rows, cols, n, 3, undistort=cals)
    try:
        for s in range(n):
            mapped.set_undistort(s, *cals[s])
        toggled.undistort(False)
        for t, fs in enumerate(frames):
            want = [_pos(p) for p in plain.track(fs)]
            assert [_pos(p) for p in mapped.track(fs)] == want, t
            assert [_pos(p) for p in toggled.track(fs)] == want, t
        for s in range(n):
            _same_model(mapped.mog_state(s), plain.mog_state(s), s)
            _same_model(toggled.mog_state(s), plain.mog_state(s), s)
    finally:
        plain.close()
        mapped.close()
        toggled.close()


# ------------------------------------------------------------------------------------ 8: refusals --

def test_refusals_and_the_input_consumed_rule():
    import torch
    import oat_amd
    rows, cols, n = 240, 320, 2
    cals = [R.cases(rows, cols)[k] for k in ("mild5", "barrel")]
    hp = _hp(rows, cols, n, 3)
    try:
        hp.set_undistort(0, *cals[0])
        with pytest.raises(oat_amd.OatGpuError) as e:        # stream 1 has no map
            hp.undistort(True)
        assert e.value.code == -1 and "stream 1" in str(e.value)
        hp.set_undistort(1, *cals[1])
        hp.undistort(True)
        lib = hp.lib
        assert lib.oatgpu_set_undistort(hp.ctx, 1, None, None, 0) == -1          # removing a map while on
        assert "stream 1" in lib.oatgpu_last_error(hp.ctx).decode()
        hp.set_undistort(1, *cals[0])                                           # a recalibration is allowed ...
        hp.set_undistort(1, *cals[1])
        # input_consumed (device frames): the caller's buffer is free once it returns -- overwritten then, the results
        # are those of the untouched frames
        frames = _frames(rows, cols, 3, n, 12, seed=23, radius=12)
        ref = _hp(rows, cols, n, 3, undistort=cals)
        want = [[_pos(p) for p in ref.track(fs)] for fs in frames]
        ref.close()
        hp.set_fusion(2)
        got = []
        for fs in frames:
            d = torch.from_numpy(np.stack(fs)).cuda()
            torch.cuda.synchronize()
            hp.enqueue_dev(d.data_ptr())
            hp.input_consumed()
            d.zero_()
            torch.cuda.synchronize()
            got.append([_pos(p) for p in hp.collect()])
        assert got == want
        hp.undistort(False)
        assert lib.oatgpu_set_undistort(hp.ctx, 1, None, None, 0) == 0           # ... and removal once it is off
    finally:
        hp.close()


# ----------------------------------------------------------------------------- 9: process pipeline --

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin")
GOLDEN = os.path.join(ROOT, "tests", "golden", "undistort_reference_config.toml")


def _chain(tmp_path, frames, stages):
    """frameserve-raw -> stages[0] -> ... -> posi-cout; stages are argument lists with SRC / SNK placeholders."""
    from test_host_pipeline import _consumers_ready
    rows, cols = frames[0].shape[:2]
    raw = tmp_path / f"frames{uuid.uuid4().hex[:6]}.raw"
    np.stack(frames).tofile(raw)
    tag = "oat_t_" + uuid.uuid4().hex[:8]
    addr = [f"{tag}n{i}" for i in range(len(stages) + 1)]
    B = lambda b: os.path.join(BIN, b)
    reader = subprocess.Popen([B("oat-posi-cout"), addr[-1]], stdout=subprocess.PIPE, text=True)
    procs = [subprocess.Popen([B(st[0])] + [addr[i] if a == "SRC" else addr[i + 1] if a == "SNK" else a for a in st[1:]])
             for i, st in enumerate(stages)]
    _consumers_ready(*addr)
    feeder = subprocess.Popen([B("oat-frameserve-raw"), addr[0], "-f", str(raw), "--rows", str(rows), "--cols", str(cols),
                               "-n", str(len(frames)), "-r", "200"])
    try:
        out, _ = reader.communicate(timeout=180)
        feeder.wait(timeout=60)
        for p in procs:
            p.wait(timeout=60)
    finally:
        for p in procs + [feeder, reader]:
            if p.poll() is None:
                p.kill()
        subprocess.run([B("oat-clean-hip")] + addr, capture_output=True)
    assert all(p.returncode == 0 for p in procs), [p.returncode for p in procs]
    return [(g["tick"], g["pos_ok"], g.get("pos_xy")) for g in (json.loads(l) for l in out.splitlines() if l.strip())]


def _arr(v):
    return "[" + ",".join(repr(float(x)) for x in v) + "]"


@pytest.mark.parametrize("chain", ["bgr", "grey"])
def test_process_pipeline_fused_equals_separate(tmp_path, chain):
    subprocess.check_call(["make", "-s", "-j4", "-C", ROOT, "host"])
    rows, cols, n = 480, 640, 20
    frames = [fs[0] for fs in _frames(rows, cols, 3, 1, n, seed=29, radius=16)]
    K, D = R.cases(rows, cols)["mild5"]
    det = (["--thresh", "[30,110]"] if chain == "grey" else ["-H", "[100,125]", "-S", "[150,256]", "-V", "[100,256]"])
    track = ["oat-track-hip", "SRC", "SNK", "-a", "0.01", "-e", "3", "-d", "7", "--area", "[20,1000000]"] + det
    front = [["oat-framefilt-hip", "col", "SRC", "SNK", "-C", "GREY"]] if chain == "grey" else []
    cal = ["--camera-matrix", _arr(K), "--distortion-coeffs", _arr(D)]
    separate = _chain(tmp_path, frames, front + [["oat-framefilt-hip", "undistort", "SRC", "SNK"] + cal, track])
    fused = _chain(tmp_path, frames, front + [track + cal])
    assert len(separate) == n and fused == separate
    assert sum(ok for _, ok, _ in fused) >= n - 3
    # the reference's own [undistort] table, unmodified, named by --undistort-key (and by framefilt's -c)
    separate = _chain(tmp_path, frames, front + [["oat-framefilt-hip", "undistort", "SRC", "SNK", "-c", GOLDEN, "undistort"], track])
    fused = _chain(tmp_path, frames, front + [track + ["-c", GOLDEN, "undistort", "--undistort-key", "undistort"]])
    assert len(separate) == n and fused == separate
