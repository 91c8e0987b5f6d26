"""GPU tests of the filter chain behind a marker set's combined record (oatgpu_set_marker_filters, oatgpu_marker_filtered;
HotPath.set_marker_filters / .marker_filtered; k_marker_filters in kernels_trackfilt.hip): `posifilt kalman` -> `posifilt
homography` -> `posifilt region` on the record `posicom mean` publishes, on the synchronous marker step and on every
pipelined form.

Expected values come from the oracle alone (tests/marker_filters_cases.py): the oracle chain once per marker,
markers_ref.combine, then O.Kalman / O.homography and the restated heading and region members of
tests/marker_filters_ref.py.  Every filtered record is compared on every frame, valid or not: flags and region name equal,
x / y / vx / vy / hx / hy equal as doubles (==), a NaN matched by a NaN; the sign of a zero is not pinned.  The marker and
combined records in front of the chain are held to the oracle too (integers exact, x / y equal, the combined record bit
for bit), so a chain fed something else cannot pass."""
import functools
import json
import math
import os
import subprocess
import uuid

import numpy as np
import pytest

import marker_filters_cases as K
import marker_filters_ref as R
import markers_ref as MR
import oracle_lib as O
import posfilt_cases as P
from parity_asserts import _same_double

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin")
DOUBLES = ("x", "y", "vx", "vy", "hx", "hy")


@pytest.fixture(scope="module")
def A():
    import oat_amd
    return oat_amd


def _hp(A, shape, ring=4, chain=None):
    n, rows, cols, M = K.SHAPES[shape][:4]
    hp = A.HotPath(rows, cols, n_streams=n, ring_depth=ring, **K.OWN)
    hp.set_markers(K.MARKERS[:M], heading_anchor=0)
    if chain:
        hp.set_marker_filters(**chain)
    return hp


def _same_filtered(got, want, tag):
    """(Not test_tracker_filters_gpu's: every member is compared with the expected record, the heading included.)"""
    assert (got.position_valid, got.velocity_valid, got.heading_valid, got.region_valid, got.region) == \
        (want["position_valid"], want["velocity_valid"], want["heading_valid"], want["region_valid"], want["region"]), (tag, got, want)
    for k in DOUBLES:
        assert _same_double(getattr(got, k), want[k]), (tag, k, got, want)


def _same_front(got, shape, t, tag):
    """The records in front of the chain against the oracle: fg, every marker, the combined record."""
    det, fgs, comb = K.detections(shape)
    fg, markers, mean = got
    for s in range(len(fg)):
        for g, w in [(fg[s], fgs[t][s])] + list(zip(markers[s], det[t][s])):
            assert g.position_valid == w["valid"], (tag, t, s, g, w)
            if w["valid"]:
                assert (g.first_pixel, g.a00, g.a10, g.a01, g.x, g.y) == (w["first_pixel"], w["a00"], w["a10"], w["a01"], w["x"], w["y"]), (tag, t, s, g, w)
        c, w = mean[s], comb[t][s]
        assert (c.position_valid, c.heading_valid, c.velocity_valid, c.n_valid) == \
            (w["position_valid"], w["heading_valid"], False, w["n_valid"]), (tag, t, s, c, w)
        for k in ("x", "y", "hx", "hy"):
            assert _same_double(getattr(c, k), w[k]), (tag, t, s, k, c, w)


# ----------------------------------------------------------------------------------------------------- the paths ---

SYNC = ("track_markers_dev", "track_markers")
RING = ("enqueue_dev", "enqueue_dev_fuse2", "enqueue", "staged")
SEQUENCE = ("sequence_fuse1", "sequence_fuse2")


def _device(fr):
    import torch
    bufs = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in fr]
    torch.cuda.synchronize()
    return bufs


def _run(hp, fr, form, ring=4, with_filtered=True):
    """fr[t][s] through one entry point -> ([t] (fg, markers, mean), [t] filtered records of the n cameras)."""
    got, filt = [], []

    def take(result):
        got.append(result)
        if with_filtered:
            sets = hp.marker_filtered()
            assert len(sets) == 1
            filt.append(sets[0])

    if form in SYNC:
        bufs = _device(fr) if form == "track_markers_dev" else None
        for t, f in enumerate(fr):
            take(hp.track_markers_dev(bufs[t].data_ptr()) if bufs else hp.track_markers(list(f)))
        return got, filt
    hp.marker_pipeline(True)
    if form in SEQUENCE:
        hp.set_fusion(int(form[-1]))
        bufs = _device(fr)
        got = hp.track_markers_sequence_dev([b.data_ptr() for b in bufs])
        return got, (hp.marker_filtered() if with_filtered else [])
    if form == "enqueue_dev_fuse2":
        hp.set_fusion(2)
    bufs = _device(fr) if form.startswith("enqueue_dev") else None
    for t, f in enumerate(fr):
        if hp.outstanding() >= ring:
            take(hp.collect_markers())
        if bufs:
            hp.enqueue_dev(bufs[t].data_ptr(), keepalive=bufs[t])
        elif form == "enqueue":
            hp.enqueue(list(f))
        else:
            for s in reversed(range(len(f))):
                hp.stage(s, f[s])
            hp.enqueue_staged()
    while hp.outstanding():
        take(hp.collect_markers())
    return got, filt


def _check_run(A, shape, name, form, ring, seen):
    chain, kw_exp = K.config(name)
    want = _want(shape, name)
    fr = K.frames(shape)
    hp = _hp(A, shape, ring, chain)
    try:
        got, filt = _run(hp, fr, form, ring)
    finally:
        hp.close()
    assert len(got) == len(filt) == len(fr), (form, ring)
    for t in range(len(fr)):
        _same_front(got[t], shape, t, (name, form, ring))
        for s in range(len(want[t])):
            _same_filtered(filt[t][s], want[t][s], (name, form, ring, t, s))
    seen.append([[tuple(repr(v) for v in vars(f).values()) for f in fs] for fs in filt])


@functools.lru_cache(maxsize=None)
def _want(shape, name):
    return K.expected(shape, **K.config(name)[1])


# --------------------------------------------- 1: every member alone, in pairs, all three -- on every path ---

@pytest.mark.parametrize("name", [c[0] for c in K.CONFIGS])
def test_chain_matches_the_oracle_on_every_path(A, name):
    """3 streams, 48 x 64, M = 2, anchor 0, 31 frames (odd: a lone frame follows the paired steps).  The synchronous step on
    device and host frames; with the marker pipeline on, enqueue_dev, enqueue_dev after set_fusion(2), enqueue, stage +
    enqueue_staged at ring depths 2 and 4, and the sequence call with one and two frames a launch.  All paths give
    identical filtered records, equal to the oracle chain."""
    cov = K.coverage(name)
    print(name, "coverage:", cov)
    _, kw_exp = K.config(name)
    if kw_exp["kalman"] in ("below_3", "thr1"):               # the filter tracks, coasts, times out and restarts
        assert all(r["tracked"] > 0 and r["drops"] > 0 and r["reinits"] > 0 for r in cov["kalman"]), cov
    if kw_exp["kalman"] == "thr0":                            # the every-sample timeout test: threshold 0 never tracks
        assert all(r["tracked"] == 0 for r in cov["kalman"]), cov
    if kw_exp["kalman"] == "both0":
        assert all(r["tracked"] > 0 for r in cov["kalman"]), cov
    if name == "region":                                      # inside, outside, on an edge, on a vertex; the first configured wins
        assert all(cov["kinds"].get(k, 0) > 0 for k in ("inside", "outside", "edge", "vertex")), cov
        assert cov["overlap"][0] > 0 and cov["overlap"][0] == cov["overlap"][1], cov
    if name == "homography_projective":                       # w crosses FLT_EPSILON: (0, 0) on a frame, both signs on others
        assert all(v > 0 for v in cov["w"]), cov
    seen = []
    for form in SYNC + SEQUENCE:
        _check_run(A, "matrix", name, form, 4, seen)
    for form in RING:
        for ring in (2, 4):
            _check_run(A, "matrix", name, form, ring, seen)
    assert all(s == seen[0] for s in seen)


# ------------------------------------------------------- 2: 65 streams: two workgroups of the chain kernel ---

@pytest.mark.parametrize("name", ["all_affine", "kalman_thr1"])
def test_65_streams_two_workgroups(A, name):
    """65 streams, 24 x 64: the lone lane of the second workgroup, different scripts in lanes 63 / 64."""
    want = _want("many", name)
    assert [w[63]["position_valid"] for w in want] != [w[64]["position_valid"] for w in want]
    assert any(w[64]["position_valid"] for w in want) and not all(w[64]["position_valid"] for w in want)
    seen = []
    for form, ring in (("track_markers_dev", 4), ("enqueue_dev_fuse2", 4), ("staged", 2), ("sequence_fuse2", 4)):
        _check_run(A, "many", name, form, ring, seen)
    assert all(s == seen[0] for s in seen)


# ------------------------------------------------------------ 3: M = 1: a NaN heading through the homography ---

@pytest.mark.parametrize("name", ["homography_affine", "all_affine"])
def test_nan_heading_through_the_homography_is_zero(A, name):
    _, _, comb = K.detections("single")
    want = _want("single", name)
    nan_in = [t for t, c in enumerate(comb) if c[0]["heading_valid"] and math.isnan(c[0]["hx"]) and math.isnan(c[0]["hy"])]
    assert len(nan_in) >= 5                                   # one marker: the heading is 0 / 0 wherever the marker is found
    for t in nan_in:
        assert want[t][0]["heading_valid"] and (want[t][0]["hx"], want[t][0]["hy"]) == (0.0, 0.0)
    seen = []
    for form, ring in (("track_markers", 4), ("enqueue", 2), ("sequence_fuse2", 4)):
        _check_run(A, "single", name, form, ring, seen)
    assert all(s == seen[0] for s in seen)


def test_nan_heading_passes_a_chain_without_homography(A):
    """kalman + region only: the heading is not touched, NaN stays NaN."""
    want = _want("single", "kalman_region")
    assert any(w[0]["heading_valid"] and math.isnan(w[0]["hx"]) for w in want)
    _check_run(A, "single", "kalman_region", "sequence_fuse2", 4, [])


# ------------------------------------------------------------------------------------- 4: unchanged ground ---

def _records(got):
    return [[repr(tuple(vars(p).values())) for p in fg] + [repr(tuple(vars(p).values())) for cam in mk for p in cam] +
            [repr(tuple(vars(c).values())) for c in mean] for fg, mk, mean in got]


@pytest.mark.parametrize("form", ["track_markers", "enqueue", "sequence_fuse2"])
def test_chain_leaves_everything_else_bit_identical(A, form):
    """fg / markers / mean, the three marker taps and the MOG2 model with a chain on equal the same run with the chain off."""
    from oat_amd import ffi
    n, rows, cols, M = K.SHAPES["matrix"][:4]
    fr = K.frames("matrix")
    out = {}
    for on in (False, True):
        hp = _hp(A, "matrix", 4, K.config("all_affine")[0] if on else None)
        try:
            got, _ = _run(hp, fr, form, 4, with_filtered=on)
            taps = [hp.read_marker_mask(m, which, s) for s in range(n) for m in range(M)
                    for which in (ffi.TAP_THRESHOLD, ffi.TAP_MORPH, ffi.TAP_FINAL)]
            model = [np.asarray(a) for s in range(n) for a in hp.mog_state(s)]
            out[on] = (_records(got), taps, model)
        finally:
            hp.close()
    assert out[False][0] == out[True][0]
    assert any(t.any() for t in out[True][1])
    for a, b in zip(out[False][1] + out[False][2], out[True][1] + out[True][2]):
        assert np.array_equal(a, b, equal_nan=True)


# ------------------------------------------------------------------------------------------- 5: life cycle ---

def _refused(fn, text):
    """text: the complete message, as the source before the setters and getters had one body printed it"""
    from oat_amd import ffi
    with pytest.raises(ffi.OatGpuError) as e:
        fn()
    assert e.value.code == -1 and str(e.value) == f"oatgpu error -1: {text}", str(e.value)


NO_CHAIN = "no filter chain is configured (oatgpu_set_marker_filters)"
NO_RESULT = "no marker result has been delivered since the filter chain was configured"
OUTSTANDING = "set_marker_filters while enqueued results are outstanding"
BAD_KALMAN = "kalman: dt must be > 0, timeout / sigma-accel / sigma-noise >= 0"


def test_life_cycle(A):
    from oat_amd import ffi
    shape, name = "matrix", "all_affine"
    chain, kw_exp = K.config(name)
    n, rows, cols, M, T = K.SHAPES[shape][:5]
    fr = K.frames(shape)
    cut = 15
    want = K.expected(shape, restart_at=(cut,), **kw_exp)
    assert want[cut:] != _want(shape, name)[cut:]              # the restart shows
    hp = A.HotPath(rows, cols, n_streams=n, ring_depth=4, **K.OWN)
    try:
        _refused(lambda: hp.set_marker_filters(**chain), "marker sets are not configured (oatgpu_set_markers)")            # no markers yet
        hp.set_markers(K.MARKERS[:M], heading_anchor=0)
        _refused(hp.marker_filtered, NO_CHAIN)                               # the chain is off
        hp.track_markers(list(fr[0]))                                                 # (a chain-off step: no record is kept)
        _refused(hp.marker_filtered, NO_CHAIN)
        hp.close()
        hp = _hp(A, shape, 4, chain)
        _refused(hp.marker_filtered, NO_RESULT)                              # before any result
        t = 0

        def sync_step():
            nonlocal t
            got = hp.track_markers(list(fr[t]))
            _same_front(got, shape, t, "life")
            a, b = hp.marker_filtered(), hp.marker_filtered()                         # nothing is consumed
            assert len(a) == 1 and repr(a) == repr(b)
            for s in range(n):
                _same_filtered(a[0][s], want[t][s], ("life", t, s))
            t += 1

        for _ in range(5):
            sync_step()
        # refused with nothing changed: limits, names, parameters -- the filter goes on where it was
        sq = [(0, 0), (10, 0), (10, 10), (0, 10)]
        _refused(lambda: hp.set_marker_filters(regions=[(f"r{i}", sq) for i in range(17)]), "at most 16 regions (got 17)")
        _refused(lambda: hp.set_marker_filters(regions=[("a", [(i, i * i % 7) for i in range(65)])]),
                 "region 0 (a): at most 64 points (got 65)")
        _refused(lambda: hp.set_marker_filters(regions=[("tenletters", sq)]), "region 0: a name takes at most 9 bytes")
        _refused(lambda: hp.set_marker_filters(regions=[("a", [(0, 0), (40000, 0), (5, 5)])]),
                 "region 0 (a): point 1 is beyond +-32767")
        _refused(lambda: hp.set_marker_filters(kalman=dict(dt=0.0)), BAD_KALMAN)
        _refused(lambda: hp.set_marker_filters(kalman=dict(sigma_noise=-1.0)), BAD_KALMAN)
        for _ in range(2):
            sync_step()
        hp.set_marker_filters(regions=[("ninebytes", sq)] + [(f"r{i}", sq) for i in range(15)])     # the limits themselves pass
        hp.set_marker_filters(regions=[("a", [(i, i * i % 7) for i in range(64)]), ("e", [])])
        hp.track_markers(list(fr[t]))
        assert [f.region for f in hp.marker_filtered()[0]] == [None] * n               # (an empty contour is never hit)
        hp.close()

        hp = _hp(A, shape, 4, chain)
        hp.marker_pipeline(True)                              # the pipeline after the chain ...
        t = 0
        while t < 7:                                          # pipelined, one set in flight
            hp.enqueue(list(fr[t]))
            if t == 3:                                        # refused with results outstanding: state and results unaffected
                _refused(lambda: hp.set_marker_filters(**chain), OUTSTANDING)
                _refused(lambda: hp.set_marker_filters(), OUTSTANDING)
            got = hp.collect_markers()
            _same_front(got, shape, t, "pipe")
            sets = hp.marker_filtered()
            for s in range(n):
                _same_filtered(sets[0][s], want[t][s], ("pipe", t, s))
            t += 1
        for _ in range(2):
            sync_step()                                       # the synchronous step between drained runs advances the same filter
        # oatgpu_track_collect retires a set, filtered record included; the next set's record is its own
        hp.enqueue(list(fr[t]))
        hp.enqueue(list(fr[t + 1]))
        before = repr(hp.marker_filtered())
        hp.collect()
        assert repr(hp.marker_filtered()) == before           # (not a marker-result call: the latest delivered set stays)
        got = hp.collect_markers()
        _same_front(got, shape, t + 1, "after collect")
        for s in range(n):
            _same_filtered(hp.marker_filtered()[0][s], want[t + 1][s], ("after collect", t + 1, s))
        t += 2
        # the sequence call delivers its n_frames sets; max_sets too small is refused, nothing consumed
        k = cut - t
        bufs = _device(fr[t:cut])
        hp.track_markers_sequence_dev([b.data_ptr() for b in bufs])
        small = (ffi.Filtered * ((k - 1) * n))()
        assert hp.lib.oatgpu_marker_filtered(hp.ctx, small, k - 1) == -1
        sets = hp.marker_filtered()
        assert len(sets) == k
        for i in range(k):
            for s in range(n):
                _same_filtered(sets[i][s], want[t + i][s], ("sequence", t + i, s))
        t = cut
        # ... and the chain after the pipeline: set_marker_filters again restarts the filter (expected: a fresh O.Kalman)
        hp.set_marker_filters(**chain)
        _refused(hp.marker_filtered, NO_RESULT)
        bufs = _device(fr[t:])
        hp.set_fusion(2)
        hp.track_markers_sequence_dev([b.data_ptr() for b in bufs])
        sets = hp.marker_filtered()
        assert len(sets) == T - cut
        for i in range(T - cut):
            for s in range(n):
                _same_filtered(sets[i][s], want[t + i][s], ("restarted", t + i, s))
        # switching the chain off; set_markers drops it
        hp.set_marker_filters()
        _refused(hp.marker_filtered, NO_CHAIN)
        hp.set_marker_filters(**chain)
        hp.marker_pipeline(False)
        hp.set_markers(K.MARKERS[:M], heading_anchor=0)
        _refused(hp.marker_filtered, NO_CHAIN)
        hp.track_markers(list(fr[0]))
        _refused(hp.marker_filtered, NO_CHAIN)
        # the foreground filters stay refused on marker contexts
        hp.set_kalman(True, dt=0.02, timeout=1.0)
        _refused(lambda: hp.track_markers(list(fr[0])),
                 "track_markers with the position filter on (oatgpu_set_kalman) is not supported")
        hp.set_kalman(False)
    finally:
        hp.close()


# --------------------------------------------------------------- 6: a frame the LDS blob kernel declines ---

def test_busy_frame_in_the_middle_of_a_pipelined_run(A):
    """270 x 480, one camera, two markers, 50 % noise in marker 0's window on three frames (test_markers_pipeline_gpu's busy
    plane): the LDS blob kernel declines those planes, the global kernels redo them, and the chain behind the combiner sees
    the repaired records.  Expected: the chain over markers_ref.combine of the oracle's marker results."""
    from oat_amd.synth import DISC_BGR
    from test_markers_gpu import BLUE, RED, _Rig, _hp as _disc_hp, _streams
    import blob_load as B
    rows, cols, n, T = 270, 480, 1, 13
    rng = np.random.default_rng(11)
    frames = _streams(rows, cols, n, T, n_discs=2, seed=3)
    markers = [dict(BLUE, erode=0, dilate=0, area=(0.0, 1e9)), RED]
    busy = (6, 7, 9)
    for t in busy:
        f = frames[t][0].copy()
        f[rng.random((rows, cols)) < 0.5] = DISC_BGR[0]
        frames[t] = [f]
    regions = [("left", [(0, 0), (240, 0), (240, 270), (0, 270)]), ("right", [(240, 0), (480, 0), (480, 270), (240, 270)])]
    row, h = "below_3", K.AFFINE
    rig = _Rig(rows, cols, n, markers)
    hp = _disc_hp(rows, cols, n, ring_depth=4)
    try:
        hp.set_markers(markers, heading_anchor=1)
        hp.marker_pipeline(True)
        hp.set_marker_filters(kalman=P.kw(row), homography=np.array(h).reshape(3, 3), regions=regions)
        got, filt = _run(hp, [fs for fs in frames], "enqueue", 4)
    finally:
        hp.close()
    kal = O.Kalman(**P.kw(row))
    paths, found = [], 0
    for t in range(T):
        want, planes = rig.check(got[t], frames[t], 1, ("busy", t))
        paths.append(B.blob_load(planes[0][0])["path"])
        # (the library's centroids equal the oracle's to 1e-4 px on these scenes, rig.check's bar, and the combined record is
        # checked bit for bit against the library's own: the chain's expected input is that record)
        c = got[t][2][0]
        comb = dict(position_valid=c.position_valid, heading_valid=c.heading_valid, x=c.x, y=c.y, hx=c.hx, hy=c.hy)
        w = R.chain(comb, kal, h, regions)
        _same_filtered(filt[t][0], w, ("busy", t))
        found += w["position_valid"]
    print("paths of marker 0:", paths, "frames tracked:", found)
    assert all((p == "global") == (t in busy) for t, p in enumerate(paths)), paths
    assert found >= T // 2


# ------------------------------------------------------------------------------------ 7: the process pipeline ---

_MK = "H=[{h[0]},{h[1]}] S=[{s[0]},{s[1]}] V=[{v[0]},{v[1]}] e={erode} d={dilate} area=[{area[0]},{area[1]}]"
_PIPE = {}


def _pipeline(tmp_path, extra):
    """oat-frameserve-raw -> oat-track-hip (camera 0 of the matrix scene) -> 3 x oat-posi-cout: [marker 0, marker 1, SINK] records"""
    from test_host_pipeline import _consumers_ready
    n, rows, cols, M, T = K.SHAPES["matrix"][:5]
    raw = tmp_path / "frames.raw"
    np.ascontiguousarray(K.frames("matrix")[:, 0]).tofile(raw)
    tag = "oat_mf_" + uuid.uuid4().hex[:8]
    exe = lambda b: os.path.join(BIN, b)
    src, pos, msinks = tag + "src", tag + "pos", [tag + "m0", tag + "m1"]
    addrs = msinks + [pos]
    readers = [subprocess.Popen([exe("oat-posi-cout"), a], stdout=subprocess.PIPE, text=True) for a in addrs]
    args = [exe("oat-track-hip"), src, pos, "-a", str(K.LR), "-e", "0", "-d", "3", "--area", "[4,1000000]"]
    for m in K.MARKERS[:M]:
        args += ["--marker", _MK.format(**m)]
    args += ["--marker-sinks", ",".join(msinks), "--heading-anchor", "0"] + list(extra)
    track = subprocess.Popen(args)
    _consumers_ready(src, *addrs)
    feeder = subprocess.Popen([exe("oat-frameserve-raw"), src, "-f", str(raw), "--rows", str(rows), "--cols", str(cols), "-n", str(T),
                               "-r", "200"])
    try:
        outs = [r.communicate(timeout=120)[0] for r in readers]
        track.wait(timeout=60)
        feeder.wait(timeout=60)
    finally:
        for p in readers + [track, feeder]:
            if p.poll() is None:
                p.kill()
        subprocess.run([exe("oat-clean-hip"), src, *addrs], capture_output=True)
    assert track.returncode == 0
    recs = [[json.loads(l) for l in o.splitlines() if l.strip()] for o in outs]
    assert [len(r) for r in recs] == [T] * 3, [len(r) for r in recs]
    return recs


@pytest.mark.parametrize("ring", [0, 3])
def test_process_pipeline_publishes_the_filtered_position(tmp_path, ring):
    """oat-frameserve-raw -> oat-track-hip --marker x2 --heading-anchor 0 --mean-kalman -T 0.1 --mean-homography .. --region x3,
    without and with --marker-ring 3: the camera's SINK carries the filtered Position2D -- position, velocity, heading, flags,
    region name, the WORLD unit tag -- of the oracle chain for every frame (oat-posi-cout prints numbers cut to 5 places);
    the per-marker sinks are those of the run without the new options."""
    subprocess.check_call(["make", "-s", "-j4", "-C", ROOT, "host"])
    T = K.SHAPES["matrix"][4]
    if "plain" not in _PIPE:
        (tmp_path / "plain").mkdir()
        _PIPE["plain"] = _pipeline(tmp_path / "plain", [])
    plain = _PIPE["plain"]
    assert all(r["unit"] == 0 and not r["vel_ok"] and not r["reg_ok"] for r in plain[2])
    regs = [f"{name}=[{','.join(f'[{x},{y}]' for x, y in pts)}]" for name, pts in K.REGIONS]
    extra = ["--mean-kalman", "-T", "0.1", "--mean-homography", "[" + ",".join(str(v) for v in K.AFFINE) + "]"]
    for r in regs:
        extra += ["--region", r]
    recs = _pipeline(tmp_path, extra + (["--marker-ring", str(ring)] if ring else []))
    assert recs[0] == plain[0] and recs[1] == plain[1]        # the per-marker sinks are unchanged
    _, _, comb = K.detections("matrix")
    kal = O.Kalman(dt=0.02, timeout=0.1, sigma_accel=5.0, sigma_noise=0.0)       # --mean-kalman's defaults, -T 0.1
    cut = 1e-5 * (1 + 1e-9)                                   # a number printed cut to 5 places is less than 1e-5 below its value
    near = lambda g, w: all(abs(a - b) <= cut for a, b in zip(g, w))
    hits = 0
    for t in range(T):
        w = R.chain(comb[t][0], kal, K.AFFINE, K.REGIONS)
        g = recs[2][t]
        assert (g["tick"], g["unit"], g["pos_ok"], g["vel_ok"], g["head_ok"], g["reg_ok"]) == \
            (plain[2][t]["tick"], 1, w["position_valid"], w["velocity_valid"], w["heading_valid"], w["region_valid"]), (t, g, w)
        if w["position_valid"]:
            assert near(g["pos_xy"], (w["x"], w["y"])) and near(g["vel_xy"], (w["vx"], w["vy"])), (t, g, w)
        if w["heading_valid"]:
            assert near(g["head_xy"], (w["hx"], w["hy"])), (t, g, w)
        if w["region_valid"]:
            assert g["reg"] == w["region"], (t, g, w)
            hits += 1
    assert hits > 0
