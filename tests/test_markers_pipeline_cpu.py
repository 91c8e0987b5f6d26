"""CPU tests of marker sets on the pipelined path: the new ABI entries (declared, exported, bound), the Python surface, and
`oat-track-hip --marker-ring` argument handling -- none of it needs a GPU (options are parsed before any device work)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin")
NEW = ("oatgpu_set_marker_pipeline", "oatgpu_track_collect_markers", "oatgpu_track_markers_sequence_dev")
MK = "H=[100,125] S=[150,256] V=[100,256] e=3 d=7 area=[20,1000000]"


def test_new_entries_are_declared_exported_and_bound():
    from oat_amd import ffi
    lib = ffi.load()
    src = open(os.path.join(ROOT, "include", "oatgpu.h")).read()
    assert re.search(r"#define OATGPU_ABI_VERSION 9\b", src) and lib.oatgpu_abi_version() == 9      # additive entries only
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, src), name
        assert getattr(lib, name).restype is C.c_int
    sig = ffi.SIGNATURES
    P, K = C.POINTER(ffi.Position), C.POINTER(ffi.Combined)
    assert sig["oatgpu_set_marker_pipeline"][1][1:] == [C.c_int32]
    assert sig["oatgpu_track_collect_markers"][1][1:] == [P, P, K]
    assert sig["oatgpu_track_markers_sequence_dev"][1][1:] == [C.POINTER(C.c_void_p), C.c_int32, C.c_double, P, P, K]


def test_python_surface():
    import oat_amd
    for name in ("marker_pipeline", "collect_markers", "track_markers_sequence_dev"):
        assert callable(getattr(oat_amd.HotPath, name)), name


def _track(*args):
    exe = os.path.join(BIN, "oat-track-hip")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-j4", "-C", ROOT, "host"])
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)


def test_marker_ring_needs_a_marker():
    r = _track("mr_src", "mr_pos", "--marker-ring", "3")
    assert r.returncode != 0 and "--marker-ring" in r.stderr and "--marker" in r.stderr, r.stderr


@pytest.mark.parametrize("value", ["1", "0", "-2", "x", "2.5", "65"])
def test_marker_ring_below_two_or_not_a_depth_is_an_argument_error(value):
    r = _track("mr_src", "mr_pos", "--marker", MK, "--marker-sinks", "mr_a", "--marker-ring", value)
    assert r.returncode != 0 and "--marker-ring" in r.stderr, r.stderr


def test_ring_with_marker_stays_refused_and_points_at_marker_ring():
    r = _track("mr_src", "mr_pos", "--marker", MK, "--marker-sinks", "mr_a", "--ring", "4")
    assert r.returncode != 0
    assert "--marker" in r.stderr and "--ring" in r.stderr and "--marker-ring" in r.stderr, r.stderr
    r = _track("mr_src", "mr_pos", "--marker", MK, "--marker-sinks", "mr_a", "--ring", "4", "--marker-ring", "3")
    assert r.returncode != 0 and "--ring" in r.stderr, r.stderr


@pytest.mark.parametrize("extra, word", [(["--kalman"], "--kalman"), (["--homography", "[1,0,0,0,1,0,0,0,1]"], "--homography"),
                                         (["--ingest-root", "0"], "--ingest-root")])
def test_marker_ring_keeps_marker_modes_refusals(extra, word):
    r = _track("mr_src", "mr_pos", "--marker", MK, "--marker-sinks", "mr_a", "--marker-ring", "3", *extra)
    assert r.returncode != 0 and "--marker" in r.stderr and word in r.stderr, r.stderr


def test_accepted_forms_get_past_the_argument_checks(tmp_path):
    """An accepted --marker-ring (command line, or marker-ring in the -c table) passes every argument check: what stops
    the run is a later one, here --marker-sinks' count, reported only after --marker-ring was taken."""
    for form in (["--marker-ring", "2"], ["--marker-ring", "64"]):
        r = _track("mr_src", "mr_pos", "--marker", MK, "--marker", MK, "--marker-sinks", "mr_a", *form)
        assert r.returncode != 0 and "names 1 sinks for 2 markers" in r.stderr and "--marker-ring" not in r.stderr, (form, r.stderr)
    cfg = tmp_path / "rig.toml"
    cfg.write_text('[track]\nmarker-sinks = ["mr_a"]\nmarker-ring = 3\n[[track.marker]]\n[[track.marker]]\n')
    r = _track("mr_src", "mr_pos", "-c", str(cfg), "track")
    assert r.returncode != 0 and "names 1 sinks for 2 markers" in r.stderr, r.stderr
    cfg.write_text('[track]\nmarker-sinks = ["mr_a"]\nmarker-ring = 1\n[[track.marker]]\n')
    r = _track("mr_src", "mr_pos", "-c", str(cfg), "track")
    assert r.returncode != 0 and "--marker-ring" in r.stderr, r.stderr


def test_help_names_marker_ring():
    h = _track("--help")
    assert h.returncode == 0 and "--marker-ring" in h.stdout + h.stderr
