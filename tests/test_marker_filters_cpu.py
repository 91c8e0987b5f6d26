"""CPU tests of the filter chain behind a marker set's combined record (oatgpu_set_marker_filters): the restatement of
`posifilt region` and of the heading through `posifilt homography` (tests/marker_filters_ref.py) against known answers and
against an exact even-odd count, the ABI of the new structs, and what oat-track-hip accepts and refuses before it opens a
device."""
import ctypes as C
import math
import os
import random
import subprocess
from fractions import Fraction

import pytest

import marker_filters_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin")

SQUARE = [(2, 2), (8, 2), (8, 8), (2, 8)]
TRIANGLE = [(0, 0), (10, 0), (0, 10)]                                        # a slanted edge x + y = 10
NOTCHED = [(0, 0), (10, 0), (10, 10), (6, 10), (6, 4), (4, 4), (4, 10), (0, 10)]   # concave: a notch open at the top


# ------------------------------------------------------------------------------- region: known answers ---

@pytest.mark.parametrize("contour,pt,want", [
    (SQUARE, (5, 5), 1), (SQUARE, (9, 5), -1), (SQUARE, (5, 1), -1), (SQUARE, (1, 1), -1),
    (SQUARE, (2, 2), 0), (SQUARE, (8, 8), 0),                                 # vertices
    (SQUARE, (5, 2), 0), (SQUARE, (5, 8), 0),                                 # horizontal edges
    (SQUARE, (2, 5), 0), (SQUARE, (8, 5), 0),                                 # vertical edges
    (TRIANGLE, (4, 6), 0), (TRIANGLE, (5, 5), 0),                             # the slanted edge
    (TRIANGLE, (3, 3), 1), (TRIANGLE, (6, 5), -1),
    (NOTCHED, (5, 7), -1), (NOTCHED, (5, 4), 0), (NOTCHED, (5, 3), 1),        # in the notch, on its floor, below it
    (NOTCHED, (2, 7), 1), (NOTCHED, (8, 7), 1), (NOTCHED, (4, 7), 0), (NOTCHED, (5, 10), -1),
])
def test_region_known_answers(contour, pt, want):
    assert R.point_polygon_test(contour, pt) == want
    assert R.point_polygon_test(contour[::-1], pt) == want                    # clockwise = counter-clockwise
    for k in range(len(contour)):                                             # ... from whichever vertex the walk starts
        assert R.point_polygon_test(contour[k:] + contour[:k], pt) == want


def test_region_degenerate_contours():
    assert R.point_polygon_test([], (0, 0)) == -1                             # an empty contour is never hit
    assert R.point_polygon_test([(3, 4)], (3, 4)) == 0 and R.point_polygon_test([(3, 4)], (3, 5)) == -1
    seg = [(1, 1), (5, 3)]
    assert R.point_polygon_test(seg, (3, 2)) == 0 and R.point_polygon_test(seg, (1, 1)) == 0
    assert R.point_polygon_test(seg, (3, 3)) == -1 and R.point_polygon_test(seg, (7, 4)) == -1


def test_region_order_and_conversions():
    a = ("a", [(0, 0), (6, 0), (6, 6), (0, 6)])
    b = ("b", [(4, 4), (10, 4), (10, 10), (4, 10)])
    assert R.region_of([a, b], 5.0, 5.0) == 0 and R.region_of([b, a], 5.0, 5.0) == 0      # overlapping: the first configured
    assert R.region_of([a, b], 8.0, 8.0) == 1 and R.region_of([a, b], 12.0, 1.0) == -1
    assert R.region_of([], 1.0, 1.0) == -1
    # (cv::Point): cvRound per coordinate, ties to even
    assert R.to_point(2.5, 3.5) == (2, 4) and R.to_point(-0.5, -1.5) == (0, -2) and R.to_point(2.4999, 2.5001) == (2, 3)
    assert R.contour_of([(0.5, 0.5), (1.5, 0.49)]) == [(0, 0), (2, 0)]
    half = ("h", [(0.5, 0.5), (4.0, 0.5), (4.0, 4.0), (0.5, 4.0)])             # the vertex 0.5 becomes 0
    assert R.where(half[1], 0.0, 0.0) == "vertex" and R.where(half[1], 0.4, 2.0) == "edge"
    assert R.region_of([half], 6.5, 3.5) == -1 and R.region_of([half], 4.5, 3.5) == 0     # 4.5 -> 4: on the edge
    # not finite, or beyond int32 once rounded: no region
    big = ("big", [(-32767, -32767), (32767, -32767), (32767, 32767), (-32767, 32767)])
    for x in (math.nan, math.inf, -math.inf, 2.0 ** 31, -2.0 ** 31 - 1, 1e300):
        assert R.region_of([big], x, 0.0) == -1 and R.region_of([big], 0.0, x) == -1
    assert R.to_point(2.0 ** 31 - 1, -2.0 ** 31) == (2 ** 31 - 1, -2 ** 31)
    assert R.region_of([big], 32767.4, -32767.0) == 0 and R.region_of([big], 32768.0, 0.0) == -1


# ------------------------------------------------------------------- region: against an exact even-odd count ---

def _on_segment(a, b, p):
    (ax, ay), (bx, by), (px, py) = a, b, p
    if (bx - ax) * (py - ay) - (by - ay) * (px - ax) != 0:
        return False
    return min(ax, bx) <= px <= max(ax, bx) and min(ay, by) <= py <= max(ay, by)


def _exact(contour, p):
    """+1 / 0 / -1 by definition: on a segment of the closed polygon -> 0; else the parity of the crossings of the ray from p
    in direction (1009, 1), which meets no lattice point of a grid smaller than 1009, in rational arithmetic."""
    n = len(contour)
    if n == 0:
        return -1
    edges = [(contour[i - 1], contour[i]) for i in range(n)]
    if any(_on_segment(a, b, p) for a, b in edges):
        return 0
    dx, dy = 1009, 1
    crossings = 0
    for (ax, ay), (bx, by) in edges:
        ex, ey = bx - ax, by - ay
        den = dx * ey - dy * ex
        if den == 0:                               # a zero-length edge (the grid has no edge parallel to the ray)
            assert ex == 0 and ey == 0
            continue
        qx, qy = ax - p[0], ay - p[1]
        t = Fraction(qx * ey - qy * ex, den)       # along the ray
        u = Fraction(qx * dy - qy * dx, den)       # along the edge
        assert not (t > 0 and u in (0, 1))         # the ray meets no vertex
        crossings += t > 0 and 0 < u < 1
    return 1 if crossings % 2 else -1


def test_region_restatement_against_an_exact_even_odd_count():
    rng = random.Random(20240607)
    polygons, total, boundary, inside = 0, 0, 0, 0
    for G in (4, 6, 9):
        for _ in range(7000):
            contour = [(rng.randint(0, G), rng.randint(0, G)) for _ in range(rng.randint(1, 8))]
            polygons += 1
            for _ in range(3):
                p = (rng.randint(-1, G + 1), rng.randint(-1, G + 1))
                want = _exact(contour, p)
                assert R.point_polygon_test(contour, p) == want, (contour, p, want)
                total += 1
                boundary += want == 0
                inside += want > 0
    print("polygons:", polygons, "points:", total, "on the boundary:", boundary, "inside:", inside)
    # (against a vacuous pass: all three answers are common -- small grids make boundary hits frequent)
    assert polygons >= 20000 and boundary >= total // 100 and inside >= total // 100


# ------------------------------------------------------------------------------------------------ heading ---

IDENTITY = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]


def test_heading_restatement():
    # identity: the unit vector, computed by the reciprocal (h * (1 / n)), not by the division the combiner uses
    hx, hy = 3.0, 7.0
    n = math.sqrt(hx * hx + hy * hy)
    got = R.heading_through(IDENTITY, hx, hy)
    assert got == (hx * (1.0 / n), hy * (1.0 / n))
    differ = 0
    for a in range(1, 40):
        for b in range(1, 40):
            n = math.sqrt(float(a * a + b * b))
            g = R.heading_through(IDENTITY, float(a), float(b))
            assert g == (a * (1.0 / n), b * (1.0 / n)) and abs(g[0] * g[0] + g[1] * g[1] - 1.0) < 1e-15
            differ += g != (a / n, b / n)
    assert differ > 0                              # the two roundings do differ: the test can tell them apart
    # a rotation by 90 degrees, with offsets that a heading ignores
    rot = [0.0, -1.0, 123.0, 1.0, 0.0, -45.0, 0, 0, 1.0]
    assert R.heading_through(rot, 1.0, 0.0) == (0.0, 1.0) and R.heading_through(rot, 0.0, 2.0) == (-1.0, 0.0)
    assert R.heading_through(rot, 0.6, 0.8) == R.heading_through([0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0, 0, 1.0], 0.6, 0.8)
    # a scaling changes nothing of a heading but its rounding
    g = R.heading_through([5.0, 0, 9.0, 0, 5.0, 9.0, 0, 0, 1.0], 0.6, 0.8)
    assert abs(g[0] - 0.6) < 1e-15 and abs(g[1] - 0.8) < 1e-15
    # NaN in (one marker, coincident markers): |w| > FLT_EPSILON is false -> (0, 0), and (0, 0) stays (0, 0)
    assert R.heading_through(IDENTITY, math.nan, math.nan) == (0.0, 0.0)
    assert R.heading_through(IDENTITY, math.nan, 1.0) == (0.0, 0.0)
    # |w| <= FLT_EPSILON -> (0, 0); just above it the heading is a unit vector again
    eps = 2.0 ** -23
    assert R.heading_through([1, 0, 0, 0, 1, 0, 0, 0, eps], 0.6, 0.8) == (0.0, 0.0)
    assert R.heading_through([1, 0, 0, 0, 1, 0, 0, 0, -eps], 0.6, 0.8) == (0.0, 0.0)
    assert R.heading_through([1, 0, 0, 0, 1, 0, 1.0, 0, -0.6], 0.6, 0.8) == (0.0, 0.0)        # w from the heading itself
    g = R.heading_through([1, 0, 0, 0, 1, 0, 0, 0, math.nextafter(eps, 1.0)], 0.6, 0.8)
    assert abs(g[0] * g[0] + g[1] * g[1] - 1.0) < 1e-15
    # a length that is not above DBL_EPSILON: scale 0
    assert R.heading_through([1e-17, 0, 0, 0, 1e-17, 0, 0, 0, 1.0], 0.6, 0.8) == (0.0, 0.0)


# ---------------------------------------------------------------------------------------------------- ABI ---

@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(ROOT, "oat_amd", "lib", "liboatgpu.so")):
        subprocess.check_call(["make", "-s", "-j4", "-C", ROOT, "oat_amd/lib/liboatgpu.so"])
    from oat_amd import ffi
    return ffi.load()


def test_struct_sizes_and_abi_version(lib, tmp_path):
    from oat_amd import ffi
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "oatgpu.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu\\n",'
                   'sizeof(oatgpu_region),sizeof(oatgpu_marker_filters),sizeof(oatgpu_filtered),'
                   'offsetof(oatgpu_region,xy),offsetof(oatgpu_marker_filters,regions),offsetof(oatgpu_filtered,hy));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(ffi.Region), C.sizeof(ffi.MarkerFilters), C.sizeof(ffi.Filtered), ffi.Region.xy.offset,
                   ffi.MarkerFilters.regions.offset, ffi.Filtered.hy.offset]
    assert C.sizeof(ffi.Filtered) == 72
    assert lib.oatgpu_abi_version() == ffi.ABI_VERSION == 9                   # additive entries: the version stays
    for name in ("oatgpu_set_marker_filters", "oatgpu_marker_filtered"):
        assert hasattr(lib, name) and name in ffi.SIGNATURES


# --------------------------------------------------------------------- oat-track-hip: argument handling ---

def _track(*args):
    exe = os.path.join(BIN, "oat-track-hip")
    subprocess.check_call(["make", "-s", "-j4", "-C", ROOT, "host"])
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)


MK = "H=[100,125] S=[150,256] V=[100,256] e=3 d=7 area=[20,1000000]"
TWO = ["--marker", MK, "--marker", MK, "--marker-sinks", "mf_a"]              # two markers, one sink: where accepted runs stop
PAST = "names 1 sinks for 2 markers"
SQ = "[[0,0],[10,0],[10,10],[0,10]]"


@pytest.mark.parametrize("extra, word", [
    (["--mean-kalman"], "--mean-kalman"),
    (["--mean-homography", "[1,0,0,0,1,0,0,0,1]"], "--mean-homography"),
    (["--region", "a=" + SQ], "--region"),
])
def test_track_hip_refuses_chain_options_without_marker(extra, word):
    r = _track("mf_src", "mf_pos", *extra)
    assert r.returncode != 0 and "--marker" in r.stderr and word in r.stderr, r.stderr


@pytest.mark.parametrize("extra", [
    ["--region", "a"], ["--region", "=" + SQ], ["--region", "a=[[0,0],[1,1]"], ["--region", "a=[[0,0],[1,x]]"],
    ["--region", "a=[[0,0],[10,0,3],[10,10]]"],                               # a point that is not a pair
    ["--region", "a=[[0,0],[10],[10,10]]"],
    ["--region", "tenletters=" + SQ],                                         # a 10-byte name
    sum((["--region", f"r{i}=" + SQ] for i in range(17)), []),                # 17 regions
    ["--region", "a=[" + ",".join(f"[{i},{i * i % 7}]" for i in range(65)) + "]"],          # 65 vertices
    ["--region", "a=[[0,0],[40000,0],[10,10]]"],                              # a vertex beyond 32767
    ["--mean-homography", "[1,0,0,0,1,0,0,0]"],
    ["--mean-kalman", "--dt", "0"],
])
def test_track_hip_refuses_malformed_chain_options(extra):
    r = _track("mf_src", "mf_pos", *TWO, *extra)
    assert r.returncode != 0 and PAST not in r.stderr, r.stderr
    assert "--region" in r.stderr or "--mean-" in r.stderr or "--dt" in r.stderr, r.stderr


@pytest.mark.parametrize("extra", [
    ["--mean-kalman"],
    ["--mean-kalman", "--dt", "0.01", "-T", "0.1", "--sigma-accel", "3", "-n", "0.5"],
    ["--mean-kalman", "--timeout", "0.1", "--sigma-noise", "0.5"],
    ["--mean-homography", "[1,0,0,0,1,0,0,0,1]"], ["--mean-homography", "[ 0.5, 0, -3, 0, 0.5, 2e1, 1e-3, 0, 1 ]"],
    ["--region", "ninebytes=" + SQ, "--region", "b=[[0.5,0.5],[3,1],[2,7.25]]"],
    sum((["--region", f"r{i}=" + SQ] for i in range(16)), []),
    ["--region", "a=[" + ",".join(f"[{i},{i * i % 7}]" for i in range(64)) + "]"],
    ["--mean-kalman", "--mean-homography", "[2,0,1,0,2,1,0,0,1]", "--region", "a=" + SQ, "--marker-ring", "3"],
])
def test_track_hip_accepts_chain_options(extra):
    r = _track("mf_src", "mf_pos", *TWO, *extra)
    assert r.returncode != 0 and PAST in r.stderr, r.stderr                   # past the argument checks


def test_track_hip_still_refuses_the_foreground_filters_with_marker():
    for extra, word in ((["--kalman"], "--kalman"), (["--homography", "[1,0,0,0,1,0,0,0,1]"], "--homography")):
        r = _track("mf_src", "mf_pos", "--marker", MK, "--marker-sinks", "mf_a", *extra)
        assert r.returncode != 0 and "--marker" in r.stderr and word in r.stderr, r.stderr


def test_track_hip_reads_region_tables_of_the_config_file(tmp_path):
    cfg = tmp_path / "rig.toml"
    head = '[track]\nmarker-sinks = ["mf_a"]\nmean-kalman = true\nmean-homography = [1,0,0, 0,1,0, 0,0,1]\n'
    two = '[[track.marker]]\nh-thresh = [100, 125]\n\n[[track.marker]]\nh-thresh = [0, 20]\n\n'
    cfg.write_text(head + two + '[[track.region]]\nname = "north"\npoints = [[0,0],[10,0],[10,10]]\n\n'
                   '[[track.region]]\nname = "south"\npoints = [[0.5,20],[10,20],[10,30],[0,30]]\n')
    r = _track("mf_src", "mf_pos", "-c", str(cfg), "track")
    assert r.returncode != 0 and PAST in r.stderr, r.stderr
    cfg.write_text(head + two + '[[track.region]]\nname = "tenletters"\npoints = [[0,0],[10,0],[10,10]]\n')
    r = _track("mf_src", "mf_pos", "-c", str(cfg), "track")
    assert r.returncode != 0 and PAST not in r.stderr and "tenletters" in r.stderr, r.stderr
    cfg.write_text(head + two + '[[track.region]]\nname = "a"\npoints = [[0,0],[10],[10,10]]\n')
    r = _track("mf_src", "mf_pos", "-c", str(cfg), "track")
    assert r.returncode != 0 and PAST not in r.stderr and "region" in r.stderr, r.stderr
    cfg.write_text(head + two + '[[track.region]]\nname = "a"\nvertices = [[0,0],[10,0],[10,10]]\n')
    r = _track("mf_src", "mf_pos", "-c", str(cfg), "track")
    assert r.returncode != 0 and PAST not in r.stderr and "vertices" in r.stderr, r.stderr
    cfg.write_text('[track]\nmean-kalman = true\n')                            # the chain needs markers in a file, too
    r = _track("mf_src", "mf_pos", "-c", str(cfg), "track")
    assert r.returncode != 0 and "--marker" in r.stderr and "mean-kalman" in r.stderr, r.stderr


def test_track_hip_help_names_every_chain_option():
    h = _track("--help")
    assert h.returncode == 0
    for w in ("--mean-kalman", "--mean-homography", "--region", "--dt", "--timeout", "--sigma-accel", "--sigma-noise",
              "[[track.region]]"):
        assert w in h.stdout + h.stderr, w
