"""CPU tests of the marker sets (oatgpu_set_markers / oatgpu_track_markers*, `posicom mean`): the new ABI entries, the
restated combiner on known answers, the identity the design rests on -- with the oracle alone -- and oat-track-hip's
argument refusals.  No GPU here: nothing below makes a compute call."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import markers_ref as MR
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin")
NEW = ("oatgpu_set_markers", "oatgpu_set_marker_window", "oatgpu_track_markers_dev", "oatgpu_track_markers",
       "oatgpu_read_marker_mask")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(ROOT, "oat_amd", "lib", "liboatgpu.so")):
        subprocess.check_call(["make", "-s", "-j4", "-C", ROOT, "oat_amd/lib/liboatgpu.so"])
    from oat_amd import ffi
    return ffi.load()


# ---------------------------------------------------------------------------------------------- the ABI ---

def test_new_entries_are_declared_exported_and_bound(lib):
    from oat_amd import ffi
    src = open(os.path.join(ROOT, "include", "oatgpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, code), f"{n} is not declared in include/oatgpu.h"
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in ffi.SIGNATURES
    # additive: the version stays, and the new entries have a comment of their own behind the version comment
    assert lib.oatgpu_abi_version() == 9
    assert "oatgpu_set_track_undistort */" in src
    assert re.search(r"/\*[^/]*additive entries of ABI 9[^/]*oatgpu_set_markers", src)
    sig = ffi.SIGNATURES
    M, P, K = C.POINTER(ffi.Marker), C.POINTER(ffi.Position), C.POINTER(ffi.Combined)
    assert sig["oatgpu_set_markers"] == (C.c_int, [C.c_void_p, C.c_int32, M, C.c_int32])
    assert sig["oatgpu_set_marker_window"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, M])
    assert sig["oatgpu_track_markers_dev"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, P, P, K])
    assert sig["oatgpu_track_markers"][1][3:] == [C.c_double, P, P, K]
    assert sig["oatgpu_read_marker_mask"][1][1:4] == [C.c_int32] * 3


def test_struct_layouts_match_the_header(lib, tmp_path):
    from oat_amd import ffi
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "oatgpu.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n",'
                   'sizeof(oatgpu_marker),offsetof(oatgpu_marker,erode),offsetof(oatgpu_marker,min_area),'
                   'sizeof(oatgpu_combined),offsetof(oatgpu_combined,n_valid),offsetof(oatgpu_combined,x),offsetof(oatgpu_combined,hy),'
                   'sizeof(oatgpu_config),sizeof(oatgpu_position));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(ffi.Marker), ffi.Marker.erode.offset, ffi.Marker.min_area.offset,
                   C.sizeof(ffi.Combined), ffi.Combined.n_valid.offset, ffi.Combined.x.offset, ffi.Combined.hy.offset,
                   C.sizeof(ffi.Config), C.sizeof(ffi.Position)]
    assert got[0] == 48 and got[3] == 48


def test_python_surface():
    import oat_amd
    from oat_amd.components import _marker
    for name in ("set_markers", "set_marker_window", "track_markers", "track_markers_dev", "read_marker_mask"):
        assert callable(getattr(oat_amd.HotPath, name))
    assert oat_amd.Combined().heading_valid is False
    m = _marker(dict(h=(100, 125), s=(150, 256), v=(100, 256), erode=3, dilate=7, area=(20.0, 1e6)))
    assert (m.h_lo, m.h_hi, m.s_lo, m.s_hi, m.v_lo, m.v_hi, m.erode, m.dilate, m.min_area, m.max_area) == \
        (100, 125, 150, 256, 100, 256, 3, 7, 20.0, 1e6)
    d = _marker({})                        # HSVDetector's defaults
    assert (d.h_lo, d.h_hi, d.erode, d.dilate, d.min_area) == (0, 256, 0, 10, 0.0) and d.max_area > 1e308
    with pytest.raises(TypeError):
        _marker(dict(hue=(1, 2)))


# ----------------------------------------------------------------------------------- the restated combiner ---

def test_combiner_known_answers():
    c = MR.combine([(True, 10.0, 20.0), (True, 14.0, 20.0)], anchor=0)
    assert (c["position_valid"], c["heading_valid"], c["velocity_valid"], c["n_valid"]) == (True, True, False, 2)
    assert (c["x"], c["y"], c["hx"], c["hy"]) == (12.0, 20.0, 1.0, 0.0)
    c = MR.combine([(True, 10.0, 20.0), (True, 14.0, 20.0)], anchor=1)          # from the anchor to the others
    assert (c["hx"], c["hy"]) == (-1.0, 0.0)
    c = MR.combine([(True, 0.0, 0.0), (True, 0.0, 5.0), (True, 0.0, 7.0)], anchor=0)
    assert (c["x"], c["hx"], c["hy"]) == (0.0, 0.0, 1.0) and c["y"] == 1.0 / 3.0 * 5.0 + 1.0 / 3.0 * 7.0
    c = MR.combine([(True, 1.0, 1.0), (True, 4.0, 5.0)], anchor=0)
    assert (c["hx"], c["hy"]) == (3.0 / 5.0, 4.0 / 5.0)
    # the mean is (1 / M) * x summed in marker order, each product rounded on its own: not sum / M
    xs = [0.1, 0.7, 0.3]
    c = MR.combine([(True, x, 0.0) for x in xs], anchor=None)
    d = 1.0 / 3.0
    assert c["x"] == ((0.0 + d * xs[0]) + d * xs[1]) + d * xs[2]
    assert (c["position_valid"], c["heading_valid"], c["hx"], c["hy"]) == (True, False, 0.0, 0.0)   # no anchor: no heading


def test_combiner_one_invalid_marker_clears_both_flags():
    c = MR.combine([(True, 10.0, 20.0), (False, 0.0, 0.0), (True, 30.0, 40.0)], anchor=0)
    assert (c["position_valid"], c["heading_valid"], c["n_valid"]) == (False, False, 2)
    assert (c["x"], c["y"]) == (1.0 / 3.0 * 10.0 + 1.0 / 3.0 * 30.0, 1.0 / 3.0 * 20.0 + 1.0 / 3.0 * 40.0)   # the partial sum, as the reference
    assert (c["hx"], c["hy"]) == (0.0, 0.0)              # marker 0 - anchor, then nothing more: never normalised
    c = MR.combine([(False, 0.0, 0.0), (True, 3.0, 4.0)], anchor=1)
    assert (c["position_valid"], c["heading_valid"]) == (False, False)


def test_combiner_single_marker_with_anchor_is_nan_and_valid():
    c = MR.combine([(True, 10.0, 20.0)], anchor=0)
    assert c["position_valid"] and c["heading_valid"] and (c["x"], c["y"]) == (10.0, 20.0)
    assert math.isnan(c["hx"]) and math.isnan(c["hy"])        # (0, 0) / 0, kept as the reference has it
    c = MR.combine([(True, 5.0, 5.0), (True, 5.0, 5.0)], anchor=0)     # coincident markers: the same
    assert c["heading_valid"] and math.isnan(c["hx"]) and math.isnan(c["hy"])


# --------------------------------------------------------- the identity the design rests on, oracle alone ---

WINDOWS = (((100, 150, 100), (125, 256, 256)),          # a disc colour
           ((0, 0, 0), (20, 256, 256)),                 # contains (0,0,0): selects the background
           ((50, 0, 0), (70, 256, 60)),
           ((0, 0, 0), (256, 256, 256)),                # all-pass
           ((30, 10, 10), (20, 256, 256)))              # lo > hi: empty


def test_marker_masks_are_a_function_of_the_frame_and_z():
    """inRange_m(hsv(masked)) of framefilt mog's output == inRange_m(hsv(Z ? px : 0)) with Z = "masked is non-zero" computed
    by the non-zero window H [0,256] S [0,256] V [1,256] -- including black foreground pixels and windows holding (0,0,0)."""
    from oat_amd.synth import SyntheticStream
    rows, cols, T = 90, 120, 25
    st = SyntheticStream(rows, cols, 3, n_discs=3)
    mog = O.Mog2(rows, cols, 3)
    rng = np.random.default_rng(7)
    black_fg = 0
    for t in range(T):
        f = st.frame(t, with_discs=t > 0)
        if t > 2:                                  # pure black pixels on a learned background: foreground, and zero
            ys, xs = rng.integers(0, rows, 40), rng.integers(0, cols, 40)
            f[ys, xs] = 0
            f[10:14, 20 + t:26 + t] = 0
        masked, mask = mog.filter(f, 0.01)
        black_fg += int(((mask != 0) & (f.reshape(rows, cols, 3).max(-1) == 0)).sum())
        z = O.inrange3(O.bgr2hsv(masked), (0, 0, 1), (256, 256, 256)) != 0
        assert (z == (masked.max(-1) != 0)).all()                       # Z is "the masked pixel is non-zero"
        rebuilt = np.where(z[..., None], f, 0).astype(np.uint8)
        assert (rebuilt == masked).all(), t                             # Z ? px : 0 IS the published frame
        for lo, hi in WINDOWS:
            assert (O.inrange3(O.bgr2hsv(rebuilt), lo, hi) == O.inrange3(O.bgr2hsv(masked), lo, hi)).all(), (t, lo, hi)
    assert black_fg > 100                                                # the case was exercised
    assert (O.bgr2hsv(np.zeros((1, 1, 3), np.uint8)) == 0).all()        # hsv(0) = (0,0,0)


def test_grey_identity():
    from oat_amd.synth import SyntheticStream
    rows, cols = 60, 80
    st = SyntheticStream(rows, cols, 1, n_discs=2)
    mog = O.Mog2(rows, cols, 1)
    for t in range(12):
        g = O.bgr2grey(st.frame(t, with_discs=t > 0))
        if t > 2:
            g[5:9, 10 + t:16 + t] = 0
        masked, _ = mog.filter(g, 0.01)
        z = O.inrange1(masked, 1, 256) != 0
        rebuilt = np.where(z, g, 0).astype(np.uint8)
        assert (rebuilt == masked).all()
        for lo, hi in ((60, 110), (0, 40), (200, 100)):
            assert (O.inrange1(rebuilt, lo, hi) == O.inrange1(masked, lo, hi)).all()


# -------------------------------------------------------------------------- oat-track-hip: what it refuses ---

def _track(*args):
    exe = os.path.join(BIN, "oat-track-hip")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-j4", "-C", ROOT, "host"])
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)


MK = "H=[100,125] S=[150,256] V=[100,256] e=3 d=7 area=[20,1000000]"


@pytest.mark.parametrize("extra, word", [
    (["--kalman"], "--kalman"),
    (["--homography", "[1,0,0,0,1,0,0,0,1]"], "--homography"),
    (["--ring", "4"], "--ring"),
    (["--ingest-root", "0"], "--ingest-root"),
])
def test_track_hip_refuses_marker_with(extra, word):
    r = _track("mk_src", "mk_pos", "--marker", MK, "--marker-sinks", "mk_a", *extra)
    assert r.returncode != 0
    assert "--marker" in r.stderr and word in r.stderr, r.stderr


def test_track_hip_marker_argument_errors():
    r = _track("mk_src", "mk_pos", "--marker", "H=[100,125] q=3", "--marker-sinks", "mk_a")
    assert r.returncode != 0 and "--marker" in r.stderr
    r = _track("mk_src", "mk_pos", "--marker", MK, "--marker", MK, "--marker-sinks", "mk_a")        # two markers, one sink
    assert r.returncode != 0 and "--marker-sinks" in r.stderr
    r = _track("mk_src", "mk_pos", "--marker", MK, "--marker-sinks", "mk_a", "--heading-anchor", "1")
    assert r.returncode != 0 and "--heading-anchor" in r.stderr
    r = _track("mk_src", "mk_pos", "--heading-anchor", "0")
    assert r.returncode != 0 and "--marker" in r.stderr
    h = _track("--help")
    assert h.returncode == 0
    for w in ("--marker", "--marker-sinks", "--heading-anchor", "[[track.marker]]"):
        assert w in h.stdout + h.stderr, w


def test_track_hip_reads_marker_tables_of_the_config_file(tmp_path):
    cfg = tmp_path / "rig.toml"
    cfg.write_text('[track]\nadaptation-coeff = 0.01\nmarker-sinks = ["mk_a"]\nheading-anchor = 1\n\n'
                   '[[track.marker]]\nh-thresh = [100, 125]\ns-thresh = [150, 256]\nerode = 3\n\n'
                   '[[track.marker]]\nh-thresh = [0, 20]\narea = [20.0, 1e6]\n\n[other]\nx = 1\n')
    r = _track("mk_src", "mk_pos", "-c", str(cfg), "track")
    assert r.returncode != 0 and "names 1 sinks for 2 markers" in r.stderr, r.stderr     # both tables were read
    cfg.write_text('[track]\nmarker-sinks = ["mk_a,mk_b"]\nheading-anchor = 2\n[[track.marker]]\n[[track.marker]]\n')
    r = _track("mk_src", "mk_pos", "-c", str(cfg), "track")
    assert r.returncode != 0 and "--heading-anchor" in r.stderr, r.stderr
    cfg.write_text('[track]\nmarker-sinks = ["mk_a"]\n[[track.marker]]\nhue = [1, 2]\n')
    r = _track("mk_src", "mk_pos", "-c", str(cfg), "track")
    assert r.returncode != 0 and "hue" in r.stderr, r.stderr
