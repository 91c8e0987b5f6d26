"""CPU tests of the filter chain behind the motion and the subtraction tracker (oatgpu_set_tracker_filters): the
case list of tests/tracker_filters_cases.py on the reference alone -- every regime the GPU tests rely on is there, and the list
tells seven planted wrong chains apart --, the two entries in header, binding and library, and what oat-posidet-hip does with the
filter options before it opens a device."""
import ctypes as C
import os
import re
import subprocess

import pytest

import marker_filters_ref as R
import tracker_filters_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin")
N = 3
SHAPES = [(kind, *g) for kind in ("diff", "bsub") for g in K.GEOMETRIES]
# the tracker calls the wrong chains `pair_swapped` and `restart_every_call` are judged on: a sequence, two batch calls, a sequence
CALLS = [(0, 3), (3, 4), (4, 5), (5, K.T)]


@pytest.mark.parametrize("kind, rows, cols, ch", SHAPES)
def test_scripts_reach_the_detector(kind, rows, cols, ch):
    """the detections follow the script: a lead, a gap of three frames and a single miss without one, per stream and staggered"""
    det = K.detections(kind, rows, cols, ch, N)
    for s in range(N):
        for t in range(K.T):
            assert bool(det[t][s]["valid"]) == (K.present(s, t) and (kind == "diff" or t > 0)), (s, t)
    tracks = {tuple((d[s]["x"], d[s]["y"]) for d in det if d[s]["valid"]) for s in range(N)}
    assert len(tracks) == N                                                  # streams have different tracks


@pytest.mark.parametrize("kind, rows, cols, ch", SHAPES)
def test_kalman_cases_track_drop_and_bridge(kind, rows, cols, ch):
    det = K.detections(kind, rows, cols, ch, N)
    assert not any(k["position_valid"] for ks in K.want("k_thr0", kind, rows, cols, ch, N) for k in ks)     # timeout 0 never tracks
    for name in K.FINITE:
        w = K.want(name, kind, rows, cols, ch, N)
        for s in range(N):
            found = [w[t][s]["position_valid"] for t in range(K.T)]
            assert True in found and False in found, (name, s)
            assert any(found[t] and not det[t][s]["valid"] for t in range(K.T)), (name, s, "no bridged frame")
            assert all(w[t][s]["velocity_valid"] == found[t] for t in range(K.T))
    short, long_ = K.want("k_short", kind, rows, cols, ch, N), K.want("k_long", kind, rows, cols, ch, N)
    for s in range(N):
        g = K.gap(s)
        assert short[g[0]][s]["position_valid"] and not short[g[-1]][s]["position_valid"]       # shorter than the gap: drops in it
        assert all(long_[t][s]["position_valid"] for t in g)                                    # longer: coasts through


@pytest.mark.parametrize("kind, rows, cols, ch", SHAPES)
def test_homography_cases_change_every_valid_position(kind, rows, cols, ch):
    plain = K.chain_run(K.detections(kind, rows, cols, ch, N))
    for name in ("h_affine", "h_projective", "h_cross"):
        w = K.want(name, kind, rows, cols, ch, N)
        moved = [(w[t][s]["x"], w[t][s]["y"]) != (plain[t][s]["x"], plain[t][s]["y"])
                 for t in range(K.T) for s in range(N) if plain[t][s]["position_valid"]]
        assert moved and all(moved), name
    for name, front in (("h_cross", plain), ("all_cross", K.chain_run(K.detections(kind, rows, cols, ch, N), kalman=K.P.kw(K.ALL_ROW)))):
        h = K.config(name, kind, rows, cols, ch, N)["homography"]
        ws = [abs(k["x"] * h[6] + k["y"] * h[7] + h[8]) for ks in front for k in ks if k["position_valid"]]
        assert any(v <= R.FLT_EPSILON for v in ws) and any(v > R.FLT_EPSILON for v in ws), name
        w = K.want(name, kind, rows, cols, ch, N)
        assert any(k["position_valid"] and (k["x"], k["y"]) == (0.0, 0.0) for ks in w for k in ks), name


@pytest.mark.parametrize("kind, rows, cols, ch", SHAPES)
def test_region_cases_hit_every_kind(kind, rows, cols, ch):
    for name in ("regions", "all"):
        cfg = K.config(name, kind, rows, cols, ch, N)
        regions = dict(cfg["regions"])
        w = K.want(name, kind, rows, cols, ch, N)
        hit = {k["region"] for ks in w for k in ks if k["position_valid"]}
        assert None in hit and len(hit - {None}) >= 2, (name, hit)
        assert all(k["region"] is None for ks in w for k in ks if not k["position_valid"])
    # the pixel case: every way a position can lie to its region, and the overlap decided by the configured order
    cfg, w = K.config("regions", kind, rows, cols, ch, N), K.want("regions", kind, rows, cols, ch, N)
    regions = dict(cfg["regions"])
    kinds = {R.where(regions[k["region"]], k["x"], k["y"]) for ks in w for k in ks if k["region"]}
    assert {"inside", "edge", "vertex"} <= kinds, kinds
    both = [k for ks in w for k in ks if k["position_valid"] and R.where(regions["west"], k["x"], k["y"]) != "outside"
            and R.where(regions["over"], k["x"], k["y"]) != "outside"]
    assert both and all(k["region"] == "west" for k in both)
    swapped = K.chain_run(K.detections(kind, rows, cols, ch, N), regions=[cfg["regions"][1], cfg["regions"][0]] + cfg["regions"][2:])
    assert K.differs(w, swapped)


def test_the_case_list_tells_the_wrong_chains_apart():
    told = {x: [] for x in K.WRONG}
    for kind, rows, cols, ch in SHAPES:
        for name in K.CONFIGS:
            w = K.want(name, kind, rows, cols, ch, N, calls=CALLS)
            assert not K.differs(w, K.want(name, kind, rows, cols, ch, N))    # the right chain does not care how it is called
            for x in K.WRONG:
                if K.differs(w, K.want(name, kind, rows, cols, ch, N, wrong=x, calls=CALLS)):
                    told[x].append((kind, rows, name))
    assert all(told.values()), {x: len(v) for x, v in told.items()}
    # ... and both trackers tell apart the ones about state and order, on the configuration all members are on in
    for kind in ("diff", "bsub"):
        for x in ("homography_first", "region_on_pixels", "zero_as_measurement", "state_of_stream0", "pair_swapped", "restart_every_call"):
            assert any(k == kind and name == "all" for k, _, name in told[x]), (kind, x)


def test_many_streams_case_detects_on_both_workgroups():
    rows, cols, ch = K.MANY
    for kind in ("diff", "bsub"):
        w = K.want("k_long", kind, rows, cols, ch, 66, 12)
        for s in (0, 63, 64, 65):
            assert any(ks[s]["position_valid"] for ks in w) and not all(ks[s]["position_valid"] for ks in w), (kind, s)


# ---------------------------------------------------------------------------------------------------- ABI ---

@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(ROOT, "oat_amd", "lib", "liboatgpu.so")):
        subprocess.check_call(["make", "-s", "-j4", "-C", ROOT, "oat_amd/lib/liboatgpu.so"])
    from oat_amd import ffi
    return ffi.load()


def test_entries_are_declared_exported_and_bound(lib):
    from oat_amd import ffi
    import oat_amd
    header = open(os.path.join(ROOT, "include", "oatgpu.h")).read()
    assert re.search(r"^int oatgpu_set_tracker_filters\(oatgpu_ctx \*ctx, const oatgpu_marker_filters \*f\);", header, re.M)
    assert re.search(r"^int oatgpu_tracker_filtered\(oatgpu_ctx \*ctx, oatgpu_filtered \*out, int32_t max_sets\);", header, re.M)
    assert re.search(r"#define OATGPU_ABI_VERSION 9\b", header) and lib.oatgpu_abi_version() == ffi.ABI_VERSION == 9
    assert ffi.SIGNATURES["oatgpu_set_tracker_filters"] == (C.c_int, [C.c_void_p, C.POINTER(ffi.MarkerFilters)])
    assert ffi.SIGNATURES["oatgpu_tracker_filtered"] == (C.c_int, [C.c_void_p, C.POINTER(ffi.Filtered), C.c_int32])
    for name in ("oatgpu_set_tracker_filters", "oatgpu_tracker_filtered"):
        assert hasattr(lib, name)
    for cls in (oat_amd.MotionTracker, oat_amd.SubtractionTracker):
        assert callable(cls.set_filters) and callable(cls.filtered)


# ----------------------------------------------------------------- oat-posidet-hip: what needs no device ---

def _posidet(*args):
    exe = os.path.join(BIN, "oat-posidet-hip")
    subprocess.check_call(["make", "-s", "-j4", "-C", ROOT, "host"])
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)


SQ = "[[0,0],[10,0],[10,10],[0,10]]"
EYE = "[1,0,0,0,1,0,0,0,1]"


@pytest.mark.parametrize("kind", ["hsv", "thresh"])
@pytest.mark.parametrize("extra", [["--kalman"], ["--homography", EYE], ["--region", "a=" + SQ],
                                   ["--kalman", "--timeout", "0.1", "--homography", EYE, "--region", "a=" + SQ]])
def test_posidet_refuses_the_chain_without_bsub_and_says_why(kind, extra):
    r = _posidet(kind, "tf_src", "tf_pos", *extra)
    assert r.returncode != 0 and "--bsub" in r.stderr and "batched trackers" in r.stderr and kind in r.stderr, r.stderr


def test_posidet_refuses_region_tables_of_the_config_file_without_bsub(tmp_path):
    cfg = tmp_path / "rig.toml"
    cfg.write_text('[det]\nerode = 0\n\n[[det.region]]\nname = "north"\npoints = [[0,0],[10,0],[10,10]]\n')
    r = _posidet("hsv", "tf_src", "tf_pos", "-c", str(cfg), "det")
    assert r.returncode != 0 and "--bsub" in r.stderr and "--region" in r.stderr, r.stderr
    cfg.write_text('[det]\nbsub = true\nkalman = true\ndt = 0\n')
    r = _posidet("hsv", "tf_src", "tf_pos", "-c", str(cfg), "det")
    assert r.returncode != 0 and "--dt" in r.stderr, r.stderr


@pytest.mark.parametrize("kind_args", [["diff"], ["diff", "--bgr"], ["hsv", "--bsub"], ["thresh", "--bsub"]])
@pytest.mark.parametrize("extra, word", [
    (["--region", "a"], "--region"), (["--region", "=" + SQ], "name"), (["--region", "a=[[0,0],[1,x]]"], "--region"),
    (["--region", "a=[[0,0],[10],[10,10]]"], "pair"),
    (["--region", "tenletters=" + SQ], "tenletters"),
    (sum((["--region", f"r{i}=" + SQ] for i in range(17)), []), "at most 16"),
    (["--region", "a=[" + ",".join(f"[{i},{i * i % 7}]" for i in range(65)) + "]"], "at most 64"),
    (["--region", "a=[[0,0],[40000,0],[10,10]]"], "32767"),
    (["--homography", "[1,0,0,0,1,0,0,0]"], "homography"),
    (["--kalman", "--dt", "0"], "--dt"),
    (["--dt", "0.1"], "--kalman"), (["--sigma-noise", "1"], "--kalman"),
])
def test_posidet_refuses_malformed_chain_options_before_a_device_is_opened(kind_args, extra, word):
    r = _posidet(kind_args[0], "tf_src", "tf_pos", *kind_args[1:], *extra)
    assert r.returncode != 0 and word in r.stderr, r.stderr


def test_posidet_help_names_every_chain_option():
    h = _posidet("--help")
    assert h.returncode == 0
    for w in ("--kalman", "--dt", "--timeout", "--sigma-accel", "--sigma-noise", "--homography", "--region", "[[KEY.region]]",
              "--bsub", "WORLD", "Long names only"):
        assert w in h.stdout, w
