"""CPU tests of target shapes: the model of tests/shapes_ref.py and the cases of tests/shapes_cases.py are checked
on their own -- the cases reach what they are aimed at, the unit-step identity the kernel rests on holds, seven planted wrong
models each differ somewhere -- then the header, the struct, the binding, the exports and the binaries' start-up refusals.

Non-vacuity is a condition on the model alone.  "At least two ranks with an axis on every sequence frame" is asked of every frame
behind a tracker's first ones (shapes_cases.WARM): the subtraction tracker's first frame IS its background and the fused tracker's
model first sees bare background, so their masks are empty there by definition, and the motion tracker analyses its first frame
as it is -- one blob, the whole frame.  The GPU tests compare those frames too.  Of the two sign flips of the axis rule the second
(vx == 0 and vy < 0) cannot occur in exact arithmetic -- vx == 0 means h < 0 and b == 0, and then vy = r - h > 0 -- so "both flips"
is checked as: flipped and unflipped axes both occur."""
import ctypes as C
import os
import re
import subprocess

import pytest

import shapes_cases as S
import shapes_ref as R
import targets_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin")
ENTRIES = ("oatgpu_set_target_shapes", "oatgpu_target_shapes")
PLANTED = S.all_planted()


def _contours():
    """(case, morph, candidate contour) of every planted case"""
    for c in PLANTED:
        for m in S.MORPHS:
            for q in T.candidates(S.planted_mask(c.name, m), c.area):
                yield c, m, q


def _sequence_runs():
    for family, alpha in (("motion", 0.0), ("subtraction", 0.0), ("subtraction", 0.05), ("fused", 0.0)):
        for rows, cols in S.GEOMETRIES:
            for v in range(3):
                yield family, alpha, rows, cols, v


# ------------------------------------------------------------------------------------------------------- the cases reach ----

def test_every_sequence_frame_has_two_ranks_with_an_axis():
    for family, alpha, rows, cols, v in _sequence_runs():
        refs = S.sequence_reference(family, rows, cols, v, alpha)
        assert len(refs) >= 10
        for t, ranks in enumerate(refs):
            if t >= S.WARM[family]:
                assert sum(r["valid"] and r["axis_valid"] for r in ranks) >= 2, (family, alpha, rows, cols, v, t)


def test_every_branch_of_the_axis_rule_occurs():
    seen = set()
    for _, _, q in _contours():
        _, info = R.derive(*R.sums(R.edges(q["points"])))
        seen.add((info["branch"], info["flipped"], (info["b"] > 0) - (info["b"] < 0)))
    assert ("none", False, 0) in seen                                  # the square: no axis
    assert {("h>=0", False, 1), ("h>=0", False, -1), ("h>=0", False, 0)} <= seen      # wider than tall: b > 0, b < 0, a horizontal bar
    assert ("h<0", False, 1) in seen and ("h<0", True, -1) in seen     # taller than wide: unflipped, flipped
    assert ("h<0", False, 0) in seen                                   # a vertical bar: vx == 0 before the sign rule
    for family, alpha, rows, cols, v in _sequence_runs():              # ... and flipped axes in the trackers' sequences as well
        if any(r["axis_valid"] and r["mu11"] < 0 and r["mu02"] > r["mu20"] for ranks in S.sequence_reference(family, rows, cols, v, alpha)
               for r in ranks):
            break
    else:
        raise AssertionError("no sequence frame has a flipped axis")


def test_a_term_passes_two_to_the_31():
    big = [c.name for c, _, q in _contours() if any(abs(v) > 2 ** 31 for e in R.unit_steps(q["points"]) for v in R.terms(e))]
    assert "far-64x1100" in big
    # ... while every sum stays far below 2^53, where the doubles of contourMoments are exact too
    assert all(abs(v) < 2 ** 53 for _, _, q in _contours() for v in R.sums(R.edges(q["points"])))


def test_the_cases_hold_what_they_are_named_for():
    ref = lambda name, k=8, morph=(0, 0): S.planted_reference(name, morph, k)      # noqa: E731
    mask = S.planted_mask("hole-48x64", (0, 0))
    assert len(T.components(mask)) == 3 and len(T.candidates(mask, (0.5, T.BIG))) == 2      # the blob in the hole is no candidate
    axes = ref("axes-24x32")
    assert axes[0]["valid"] and not axes[0]["axis_valid"] and axes[0]["major"] == axes[0]["minor"] > 0      # the square
    assert any(r["axis_valid"] and (r["axis_x"], r["axis_y"]) == (1.0, 0.0) for r in axes)                  # the horizontal bar
    assert any(r["axis_valid"] and (r["axis_x"], r["axis_y"]) == (0.0, 1.0) for r in axes)                  # the vertical bar
    assert any(r["axis_valid"] and r["axis_x"] > 0 and r["axis_y"] > 0 for r in axes)                       # diagonals both ways
    assert any(r["axis_valid"] and r["axis_x"] > 0 and r["axis_y"] < 0 for r in axes)
    areas = [c["m00"] for c in R.ranked(S.planted_mask("axes-24x32", (0, 0)), (0.5, T.BIG), 8)]
    assert len(areas) != len(set(areas))                                                                    # two blobs of equal area
    far = ref("far-64x1100")
    assert any(r["x_min"] > 1000 for r in far) and any(r["x_min"] <= 63 < r["x_max"] for r in far)
    for name, bounds in (("groups-48x64", (4, 16, 32)), ("arrival-140x200", (16,))):
        rs = ref(name)
        for b in bounds:
            assert any(r["valid"] and r["y_min"] < b <= r["y_max"] for r in rs), (name, b)
    groups = S.planted_mask("groups-48x64", (0, 0))
    assert len(T.candidates(groups, (0.5, T.BIG))) > 8                                                     # more blobs than K
    edges = ref("edges-37x61")
    assert min(r["x_min"] for r in edges) == 1 and min(r["y_min"] for r in edges) == 1                     # (the frame itself is zeroed)
    assert max(r["x_max"] for r in edges) == 59 and max(r["y_max"] for r in edges) == 35
    diag = S.planted_mask("diag-37x61", (0, 0))
    assert len(T.components(diag)) > len(T.candidates(diag, (0.0, T.BIG)))                                  # the one-pixel lines: m00 = 0
    # more than one workgroup a stream (k_green_select's grid: 4 threads a mask word of an interior row, 1024 a workgroup)
    for name in ("arrival-140x200", "far-64x1100"):
        c = next(c for c in PLANTED if c.name == name)
        assert (c.rows - 2) * ((c.cols + 63) // 64) * 4 > 2 * 1024


# -------------------------------------------------------------------------------------------------- the unit-step identity ----

def test_the_sums_over_the_polygon_equal_the_sums_over_unit_steps():
    n = 0
    for _, _, q in _contours():
        s = R.sums(R.edges(q["points"]))
        assert s[:3] == (int(q["a00"]), int(q["a10"]), int(q["a01"]))              # orders 0 and 1: the oracle's own sums
        assert R.sums(R.unit_steps(q["points"])) == s
        n += 1
    assert n > 100


def test_the_kernels_edge_rule_walks_the_same_steps():
    """One edge per side of a pixel that faces outside background, towards the diagonal neighbour first: as a multiset these are the
    unit steps of the external contour."""
    for c in PLANTED:
        if c.rows * c.cols > 30000 or c.name.startswith("dots"):
            continue
        mask = S.planted_mask(c.name, (0, 0))
        comps = dict(T.components(mask))
        for q in T.candidates(mask, c.area):
            px = comps[q["start"][1] * c.cols + q["start"][0]]
            assert sorted(R.pixel_edges(mask, px)) == sorted(R.unit_steps(q["points"])), (c.name, q["start"])


# ------------------------------------------------------------------------------------------------- planted wrong models ----

@pytest.mark.parametrize("wrong", R.WRONG)
def test_a_planted_wrong_model_differs(wrong):
    if wrong == "previous_frame":
        for family, alpha, rows, cols, v in _sequence_runs():
            masks = S.sequence_masks(family, rows, cols, v, alpha)
            differs = [not R.same_set(R.wrong_reference(masks[t], T.AREA, 4, wrong, previous=masks[t - 1]), R.reference(masks[t], T.AREA, 4))
                       for t in range(S.WARM[family] + 1, len(masks))]
            assert all(differs), (family, rows, cols, v)
        return
    hit = []
    for c in PLANTED:
        if c.name.startswith("dots") or (wrong == "hole_edges" and c.rows * c.cols > 30000):
            continue
        for m in S.MORPHS:
            mask = S.planted_mask(c.name, m)
            for k in S.KS:
                if not R.same_set(R.wrong_reference(mask, c.area, k, wrong), R.reference(mask, c.area, k)):
                    hit.append((c.name, m, k))
    assert hit, wrong
    expect = dict(hole_edges="hole-48x64", mask_extents="groups-48x64", axis_unsigned="diag-37x61").get(wrong)
    assert expect is None or any(h[0] == expect for h in hit), (wrong, hit)


# ------------------------------------------------------------------------------------- header, library, binding, binary ----

@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(ROOT, "oat_amd", "lib", "liboatgpu.so")):
        subprocess.check_call(["make", "-s", "-j4", "-C", ROOT, "oat_amd/lib/liboatgpu.so"])
    from oat_amd import ffi
    return ffi.load()


def test_shapes_are_declared_exported_and_bound(lib, tmp_path):
    from oat_amd import ffi
    header = open(os.path.join(ROOT, "include", "oatgpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(lib, name) and name in ffi.SIGNATURES
    assert ffi.SIGNATURES["oatgpu_set_target_shapes"][1] == [C.c_void_p, C.c_int32]
    assert ffi.SIGNATURES["oatgpu_target_shapes"][1] == [C.c_void_p, C.POINTER(ffi.Shape), C.c_int32]
    fields = ("valid", "axis_valid", "a20", "a02", "x_min", "y_max", "mu20", "axis_x", "major", "minor")
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "oatgpu.h"\nint main(){printf("%zu ' + "%zu " * len(fields) +
                   '%d\\n",sizeof(oatgpu_shape),' + ",".join("offsetof(oatgpu_shape,%s)" % f for f in fields) +
                   ',OATGPU_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    want = [104, 0, 4, 8, 24, 32, 44, 48, 72, 88, 96, 9]
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == want
    assert [C.sizeof(ffi.Shape)] + [getattr(ffi.Shape, f).offset for f in fields] == want[:-1]
    assert ffi.ABI_VERSION == 9 == lib.oatgpu_abi_version()


def test_the_header_states_the_semantics():
    header = open(os.path.join(ROOT, "include", "oatgpu.h")).read()
    text = " ".join(" ".join(re.sub(r"^\s*\*\s", "", line) for line in header.splitlines()).split())
    for words in ("a20 += d * (x0 * (x0 + x1) + x1 * x1)", "a11 += d * (x0 * ((y0 + y1) + y0) + x1 * ((y0 + y1) + y1))",
                  "a02 += d * (y0 * (y0 + y1) + y1 * y1)", "an edge facing a hole is not one", "wherever those stay below 2^53",
                  "An axis has no front", "An invalid rank is all zeros", "oatgpu_track.rank indexes the frame's shape set",
                  "mu20 = m20 - m10 * cx", "v = (h + r, b) if h >= 0, else (b, r - h)"):
        assert words in text, words


def test_every_detector_class_has_shapes():
    import oat_amd.components as comp
    for cls in ("HotPath", "MotionTracker", "SubtractionTracker", "HSVDetector", "SimpleThreshold", "DifferenceDetector"):
        k = getattr(comp, cls)
        assert all(callable(getattr(k, m, None)) for m in ("set_targets", "set_target_shapes", "target_shapes")), cls


@pytest.fixture(scope="module")
def host_bins():
    if not os.path.exists(os.path.join(BIN, "oat-posidet-hip")):
        subprocess.check_call(["make", "-s", "-j4", "-C", ROOT, "host"])
    return BIN


NEEDS = "--target-shape needs --target-sinks"
REFUSALS = [
    ("oat-posidet-hip", ["diff", "src", "snk", "--target-shape"], NEEDS),
    ("oat-posidet-hip", ["hsv", "src", "snk", "--target-shape"], NEEDS),
    ("oat-posidet-hip", ["thresh", "src", "snk", "--bsub", "--target-shape"], NEEDS),
    ("oat-posidet-hip", ["diff", "src", "snk", "--track-sinks", "a,b", "--kalman", "--target-shape"], NEEDS),
    ("oat-track-hip", ["src", "snk", "--target-shape"], NEEDS),
    ("oat-track-hip", ["src", "snk", "--target-shape", "--marker", "H=[0,10]", "--marker-sinks", "m"], NEEDS),
]


@pytest.mark.parametrize("prog,args,text", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_the_binaries_refuse_a_target_shape_without_target_sinks(host_bins, prog, args, text):
    r = subprocess.run([os.path.join(host_bins, prog)] + args, capture_output=True, text=True, timeout=20)
    assert r.returncode != 0 and text in r.stderr, (r.returncode, r.stderr)


def test_target_shape_in_a_config_file_is_checked_the_same_way(host_bins, tmp_path):
    cfg = tmp_path / "c.toml"
    cfg.write_text('[det]\ntarget-shape = true\n')
    for prog, args in (("oat-posidet-hip", ["diff", "src", "snk"]), ("oat-track-hip", ["src", "snk"])):
        r = subprocess.run([os.path.join(host_bins, prog)] + args + ["-c", str(cfg), "det"], capture_output=True, text=True, timeout=20)
        assert r.returncode != 0 and NEEDS in r.stderr, (prog, r.stderr)
    cfg.write_text('[det]\ntarget-shape = 3\n')
    r = subprocess.run([os.path.join(host_bins, "oat-posidet-hip"), "diff", "src", "snk", "-c", str(cfg), "det"], capture_output=True,
                       text=True, timeout=20)
    assert r.returncode != 0 and "must be a TOML value of type bool" in r.stderr, r.stderr
