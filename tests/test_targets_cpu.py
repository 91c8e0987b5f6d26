"""CPU tests of multi-target detection (oatgpu_set_targets / oatgpu_targets): the reference ranking of
tests/targets_cases.py against the oracle's own selection, the conditions that keep the GPU tests from being vacuous, planted wrong
rankers, the header / binding / library, and the start-up refusals of the host binaries' --target-sinks."""
import ctypes as C
import os
import re
import subprocess

import pytest

import oracle_lib as O
import targets_cases as T
from diff_cases import same_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin")
PLANTED = [(c, m) for c in T.planted_cases() for m in T.MORPHS]
SEQUENCES = [(f, r, c, v, a) for f in T.FAMILIES for (r, c) in T.GEOMETRIES for v in range(3)
             for a in (T.SUB_ALPHAS if f == "subtraction" else (0.0,))]


# ---- rank 0 of the reference is the oracle's own selection ----

@pytest.mark.parametrize("case,morph", PLANTED, ids=lambda x: str(x))
def test_rank0_is_sift_contours_on_planted_masks(case, morph):
    det, mask = T.planted_mask(case, morph)
    for k in T.KS:
        ranks, n_found = T.planted_reference(case.name, morph, k)
        assert len(ranks) == k and n_found == len(T.candidates(mask, case.area))
        assert same_dict(ranks[0], det)
        assert same_dict(ranks[0], O.sift_contours(mask, *case.area))
        assert same_dict(ranks[0], O.sift_cracks(mask, *case.area))
        # the ranks are the first k of ONE order: descending (area, first pixel), invalid behind the last candidate
        valid = [r for r in ranks if r["valid"]]
        assert len(valid) == min(k, n_found) and all(not r["valid"] for r in ranks[len(valid):])
        keys = [(r["area"], r["first_pixel"]) for r in valid]
        assert keys == sorted(keys, reverse=True) and len(set(keys)) == len(keys)


@pytest.mark.parametrize("family,rows,cols,variant,alpha", SEQUENCES)
def test_rank0_is_sift_contours_on_tracker_frames(family, rows, cols, variant, alpha):
    masks = T.sequence_masks(family, rows, cols, variant, alpha)
    ref = T.sequence_reference(family, rows, cols, variant, alpha)
    assert 8 <= len(masks) <= 12
    for (det, mask), (ranks, n_found) in zip(masks, ref):
        assert same_dict(ranks[0], det)
        assert same_dict(ranks[0], O.sift_contours(mask, *T.AREA))
        assert same_dict(ranks[0], O.sift_cracks(mask, *T.AREA))
        assert sum(r["valid"] for r in ranks) == min(T.TRACKER_K, n_found)


# ---- non-vacuity, as conditions on the inputs ----

@pytest.mark.parametrize("family,rows,cols,variant,alpha", SEQUENCES)
def test_tracker_sequences_hold_several_blobs(family, rows, cols, variant, alpha):
    counts = [n for _, n in T.sequence_reference(family, rows, cols, variant, alpha)]
    assert 2 * sum(n >= 3 for n in counts) >= len(counts), counts
    assert any(n < T.TRACKER_K for n in counts) and any(n > T.TRACKER_K for n in counts), counts


def test_planted_cases_hold_ties_and_both_window_bounds():
    tie_k, below, at_max, nested, zero, many = set(), False, False, False, False, False
    for case, morph in PLANTED:
        mask = T.planted_mask(case, morph)[1]
        every = O.find_contours(mask)
        below = below or any(0 < c["m00"] < case.area[0] for c in every)
        at_max = at_max or any(c["m00"] == case.area[1] for c in every)
        zero = zero or (case.area[0] == 0.0 and any(c["m00"] == 0 for c in every))
        nested = nested or len(T.components(mask)) > len(every)
        many = many or len(every) > 1024
        for k in T.KS:
            ranks, n_found = T.planted_reference(case.name, morph, k + 1)
            if n_found > k and ranks[k - 1]["area"] == ranks[k]["area"]:
                tie_k.add(k)                                  # equal areas on both sides of the cut to k
    assert tie_k == set(T.KS) and below and at_max and nested and zero and many


@pytest.mark.parametrize("wrong", T.WRONG)
def test_cases_tell_a_wrong_ranker_apart(wrong):
    for case, morph in PLANTED:
        mask = T.planted_mask(case, morph)[1]
        for k in T.KS:
            if not T.same_ranking(T.wrong_ranking(mask, case.area, k, wrong), T.planted_reference(case.name, morph, k)):
                return
    pytest.fail(f"no planted case tells the '{wrong}' ranker from the reference")


# ---- header, binding, library ----

@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(ROOT, "oat_amd", "lib", "liboatgpu.so")):
        subprocess.check_call(["make", "-s", "-j4", "-C", ROOT, "oat_amd/lib/liboatgpu.so"])
    from oat_amd import ffi
    return ffi.load()


def test_targets_are_declared_exported_and_bound(lib, tmp_path):
    from oat_amd import ffi
    header = open(os.path.join(ROOT, "include", "oatgpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("oatgpu_set_targets", "oatgpu_targets"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(lib, name) and name in ffi.SIGNATURES
    assert ffi.SIGNATURES["oatgpu_set_targets"][1] == [C.c_void_p, C.c_int32]
    assert ffi.SIGNATURES["oatgpu_targets"][1] == [C.c_void_p, C.POINTER(ffi.Position), C.POINTER(C.c_int32), C.c_int32]
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include "oatgpu.h"\nint main(){printf("%d %d %zu\\n",OATGPU_MAX_TARGETS,'
                   'OATGPU_ABI_VERSION,sizeof(oatgpu_position));return 0;}\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == [8, 9, 96]          # sizeof(oatgpu_position): what it was before targets
    assert ffi.MAX_TARGETS == 8 and ffi.ABI_VERSION == 9 == lib.oatgpu_abi_version() and C.sizeof(ffi.Position) == 96


def test_every_detector_class_has_targets():
    import oat_amd
    for cls in ("HotPath", "MotionTracker", "SubtractionTracker", "HSVDetector", "SimpleThreshold", "DifferenceDetector"):
        k = getattr(oat_amd, cls, None) or getattr(__import__("oat_amd.components", fromlist=[cls]), cls)
        assert callable(getattr(k, "set_targets", None)) and callable(getattr(k, "targets", None)), cls


# ---- the host binaries refuse a wrong --target-sinks at start-up, before a device is opened ----

@pytest.fixture(scope="module")
def host_bins():
    if not all(os.path.exists(os.path.join(BIN, b)) for b in ("oat-posidet-hip", "oat-track-hip")):
        subprocess.check_call(["make", "-s", "-j4", "-C", ROOT, "host"])
    return BIN


REFUSALS = [
    ("oat-posidet-hip", ["thresh", "src", "snk", "--target-sinks", "1,2,3,4,5,6,7,8,9"], "names 9 sinks, at most 8"),
    ("oat-posidet-hip", ["hsv", "src", "snk", "--target-sinks", "a,b", "--marker", "H=[0,10]"], "--target-sinks does not go with --marker"),
    ("oat-posidet-hip", ["diff", "src", "snk", "--target-sinks", "a,b,a"], "sink 'a' is named twice"),
    ("oat-posidet-hip", ["thresh", "src", "snk", "--target-sinks", "a,snk"], "sink 'snk' is named twice"),
    ("oat-posidet-hip", ["thresh", "src", "snk", "--target-sinks", "a", "--target-sinks", "b"], "2 lists for 1 SOURCEs"),
    ("oat-track-hip", ["s0", "k0", "--target-sinks", "1,2,3,4,5,6,7,8,9"], "names 9 sinks, at most 8"),
    ("oat-track-hip", ["s0,s1", "k0,k1", "--target-sinks", "a,b", "--target-sinks", "c"], "lists of different lengths (2 and 1)"),
    ("oat-track-hip", ["s0,s1", "k0,k1", "--target-sinks", "a,b"], "1 lists for 2 SOURCEs"),
    ("oat-track-hip", ["s0", "k0", "--target-sinks", "a,b", "--marker", "H=[0,10]", "--marker-sinks", "m"], "--target-sinks does not go with --marker"),
    ("oat-track-hip", ["s0,s1", "k0,k1", "--target-sinks", "a,b", "--target-sinks", "c,a"], "sink 'a' is named twice"),
    ("oat-track-hip", ["s0,s1", "k0,k1", "--target-sinks", "a,b", "--target-sinks", "c,k0"], "sink 'k0' is named twice"),
]


@pytest.mark.parametrize("binary,args,text", REFUSALS, ids=[f"{b}-{i}" for i, (b, _, _) in enumerate(REFUSALS)])
def test_host_binaries_refuse_wrong_target_sinks(host_bins, binary, args, text):
    r = subprocess.run([os.path.join(host_bins, binary)] + args, capture_output=True, text=True, timeout=20)
    assert r.returncode != 0 and text in r.stderr, (r.returncode, r.stderr)


def test_target_sinks_in_a_config_file_are_checked_the_same_way(host_bins, tmp_path):
    cfg = tmp_path / "c.toml"
    cfg.write_text('[track]\ntarget-sinks = ["a,b", "c"]\n')
    r = subprocess.run([os.path.join(host_bins, "oat-track-hip"), "s0,s1", "k0,k1", "-c", str(cfg), "track"], capture_output=True,
                       text=True, timeout=20)
    assert r.returncode != 0 and "lists of different lengths (2 and 1)" in r.stderr, r.stderr
