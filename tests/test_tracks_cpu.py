"""Target tracks (oatgpu_set_tracks) without a GPU: the cases of tests/tracks_cases.py are not vacuous -- each
condition is asserted on the model (tests/tracks_ref.py) alone --, seven planted wrong trackers each differ from the model
somewhere, the header declares what the library exports and the binding binds, and oat-posidet-hip refuses a wrong --track-sinks
at start-up."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest

import tracks_cases as TC
import tracks_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "build", "bin")
ENTRIES = ("oatgpu_set_tracks", "oatgpu_tracks", "oatgpu_tracks_update")
IMAGE = [(f, a, g) for f, a in TC.FAMILIES for g in TC.GEOMETRIES + (TC.MANY,)]


def _crossed(records):
    """the measured slots' ranks, in slot order, are not ascending: rank order is not slot order"""
    ranks = [r["rank"] for r in records if r["rank"] >= 0]
    return ranks != sorted(ranks)


def _resumed(out):
    return [(t + 1, i) for t, (a, b) in enumerate(zip(out, out[1:])) for i, (x, y) in enumerate(zip(a, b))
            if x["missed"] > 0 and y["missed"] == 0 and y["id"] == x["id"] != 0]


# ------------------------------------------------------------------------------------------------------ the fed cases ----

def test_fed_cases_have_the_shapes_the_issue_names():
    cases = TC.fed_cases()
    assert {c.k for c in cases} == {1, 3, 8}
    assert all(12 <= len(c.scene) <= 16 for c in cases)
    assert any(math.isinf(c.gate) for c in cases) and any(c.gate == 0.0 for c in cases)
    assert any(c.homography is not None and c.regions for c in cases)
    for c in cases:                                  # valid ranks come first, as k_blob_rank's do
        for row in c.frames(2):
            flags = [v for v, _, _ in row]
            assert flags == sorted(flags, reverse=True) and len(row) == c.k


def test_ranks_swap_while_slots_persist():
    out, _ = TC.fed("swap-k3-inf").want()
    assert sum(_crossed(rs) for rs in out) >= 3
    for i, first in ((0, 0), (1, 0), (2, 5)):        # slot i carries one id from its birth to the end
        assert [rs[i]["id"] for rs in out[first:]] == [i + 1] * (len(out) - first)
        assert [rs[i]["age"] for rs in out[first:]] == list(range(len(out) - first))
    assert out[4][2]["id"] == 0 and out[5][2]["rank"] >= 0          # the third object is born into the first free slot


def test_a_short_miss_resumes_and_a_long_one_expires():
    out, log = TC.fed("miss-k3").want()
    assert [rs[0]["missed"] for rs in out[3:7]] == [0, 1, 2, 0] and {rs[0]["id"] for rs in out} == {1}
    assert (6, 0) in _resumed(out)
    assert [rs[1]["id"] for rs in out[2:8]] == [2, 2, 2, 2, 0, 4]   # B runs out on frame 6; D takes the slot a frame later, as id 4
    assert log[6]["expired"] == [2] and log[6]["dropped"] == [2] and log[7]["born"] == {1: 2}
    assert out[6][1]["rank"] == -1 and out[6][1]["age"] == 0 and out[6][1]["missed"] == 0
    ids = [r["id"] for rs in out for r in rs if r["id"]]
    assert 3 in ids and max(ids) == 4               # never reused


def test_a_dying_track_keeps_its_slot_for_the_frame():
    out, log = TC.fed("one-k1").want()
    assert log[6]["live"] == [True] and log[6]["dropped"] == [0] and log[6]["expired"] == [1]
    assert out[6][0]["id"] == 0 and out[7][0]["id"] == 2 and out[7][0]["age"] == 0
    assert (13, 0) in _resumed(out)


def test_the_gate_admits_inside_and_gives_birth_outside():
    c = TC.fed("gate-k3")
    out, log = c.want()
    cam = TR.Camera(c.k, TC.KALMAN, c.gate)
    rows = c.frames()
    for row in rows[:6]:
        cam.step(row)
    ca, cb = cam.cost(0, rows[6][0]), cam.cost(1, rows[6][1])
    assert 0.99 * c.gate ** 2 < ca <= c.gate ** 2 < cb < 1.01 * c.gate ** 2, (ca, cb)
    assert log[6]["taken"] == {0: 0} and log[6]["born"] == {2: 1} and log[6]["gated"] == [1]
    assert out[6][1]["id"] == 2 and out[6][1]["missed"] == 1        # the old slot coasts
    assert [l["dropped"] for l in log[7:11]] == [[2], [2], [2], []]  # K + 1 objects: one is dropped until a slot is free
    assert log[10]["born"] == {1: 2}


def test_gate_zero_and_gate_inf():
    out, log = TC.fed("gate0-k3").want()
    assert {rs[0]["id"] for rs in out} == {1} and all(rs[0]["rank"] == 0 for rs in out)      # the object that stands still: cost 0
    assert all(l["gated"] == [1] for l in log[1:])                                           # the one that moves never matches
    out, log = TC.fed("swap-k3-inf").want()
    assert not any(l["gated"] or l["dropped"] for l in log)


def test_the_exact_tie():
    c = TC.fed("tie-k3-inf")
    for s in range(4):                               # ... on every stream's shifted copy
        rows = c.frames(s)
        cam = TR.Camera(c.k, TC.KALMAN, c.gate)
        cam.step(rows[0])
        assert cam.cost(0, rows[1][0]) == cam.cost(1, rows[1][0]) == 100.0
        out = cam.step(rows[1])
        assert cam.log[1]["ties"] == [(100.0, [(0, 0), (1, 0)])]
        assert out[0]["rank"] == 0 and out[1]["rank"] == -1


def test_the_chain_tail_is_exercised():
    c = TC.fed("chain-k3")
    out, _ = c.want()
    regions = {r["region"] for rs in out for r in rs}
    assert {"low", "wide", None} <= regions
    plain, _ = TC.fed("miss-k3").want()
    assert any(a["x"] != b["x"] for ra, rb in zip(out, plain) for a, b in zip(ra, rb) if a["position_valid"])
    assert [[r["id"] for r in rs] for rs in out] == [[r["id"] for r in rs] for rs in plain]    # the assignment works in pixels


def test_k8_fills_every_slot():
    out, log = TC.fed("many-k8").want()
    assert any(all(r["id"] for r in rs) for rs in out)
    assert any(l["expired"] for l in log) and any(l["dropped"] for l in log) and _resumed(out)


@pytest.mark.parametrize("wrong", TR.WRONG)
def test_a_planted_wrong_tracker_differs(wrong):
    hits = [c.name for c in TC.fed_cases() if TR.differs(c.want()[0], c.want(wrong=wrong)[0])]
    assert hits, wrong
    if wrong != "ties_to_higher_slot":               # (a tie needs planted doubles) ... and on the image sequences
        assert any(TR.differs(TC.image_want(f, *g, v, a)[0], TC.image_want(f, *g, v, a, wrong=wrong)[0])
                   for f, a, g in IMAGE for v in range(3)), wrong


def test_streams_see_shifted_copies():
    c = TC.fed("many-k8")
    a, b = c.want(0)[0], c.want(7)[0]
    assert [[(r["id"], r["rank"]) for r in rs] for rs in a] == [[(r["id"], r["rank"]) for r in rs] for rs in b]
    assert TR.differs(a, b)


# ---------------------------------------------------------------------------------------------------- the image cases ----

@pytest.mark.parametrize("family,alpha,geometry", IMAGE, ids=[f"{f}-{a}-{g[0]}x{g[1]}" for f, a, g in IMAGE])
def test_image_sequences_cross_ranks_and_lose_blocks(family, alpha, geometry):
    rows, cols, channels = geometry
    for v in range(3):
        frames = TC.sequence(family, rows, cols, channels, v)
        assert len(frames) == TC.IMG_T and frames[0].shape == ((rows, cols, 3) if channels == 3 else (rows, cols))
        out, log = TC.image_want(family, rows, cols, channels, v, alpha)
        assert sum(_crossed(rs) for rs in out) >= 3, (v, "rank order equals slot order")
        assert _resumed(out), (v, "no id resumes")
        assert max(r["id"] for rs in out for r in rs) >= 3
    every = [TC.image_want(family, rows, cols, channels, v, alpha)[1] for v in range(3)]
    assert any(l["expired"] for log in every for l in log), "no id expires"


# ------------------------------------------------------------------------------------- header, library, binding, binary ----

@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(ROOT, "oat_amd", "lib", "liboatgpu.so")):
        subprocess.check_call(["make", "-s", "-j4", "-C", ROOT, "oat_amd/lib/liboatgpu.so"])
    from oat_amd import ffi
    return ffi.load()


def test_tracks_are_declared_exported_and_bound(lib, tmp_path):
    from oat_amd import ffi
    header = open(os.path.join(ROOT, "include", "oatgpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(lib, name) and name in ffi.SIGNATURES
    assert ffi.SIGNATURES["oatgpu_set_tracks"][1] == [C.c_void_p, C.POINTER(ffi.MarkerFilters), C.c_double]
    assert ffi.SIGNATURES["oatgpu_tracks"][1] == [C.c_void_p, C.POINTER(ffi.Track), C.c_int32]
    assert ffi.SIGNATURES["oatgpu_tracks_update"][1] == [C.c_void_p, C.POINTER(ffi.Position), C.POINTER(ffi.Track)]
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "oatgpu.h"\nint main(){printf("%zu %zu %zu %zu %d\\n",'
                   'sizeof(oatgpu_track),offsetof(oatgpu_track,id),offsetof(oatgpu_track,rank),offsetof(oatgpu_track,missed),'
                   'OATGPU_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert [int(x) for x in subprocess.check_output([str(exe)]).split()] == [96, 72, 80, 88, 9]
    assert C.sizeof(ffi.Track) == 96 and ffi.Track.id.offset == 72 and ffi.Track.rank.offset == 80 and ffi.Track.missed.offset == 88
    assert ffi.ABI_VERSION == 9 == lib.oatgpu_abi_version()


def test_the_header_states_the_semantics():
    header = open(os.path.join(ROOT, "include", "oatgpu.h")).read()
    text = " ".join(header.split())
    for words in ("NOT LIVE AT THE START OF THIS FRAME", "break equal costs by the smaller slot index, then by the smaller rank",
                  "A NaN cost is inadmissible", "carries the covariance filter_step leaves behind", "do NOT advance tracks"):
        assert words in text.replace("* ", ""), words


def test_every_detector_class_has_tracks():
    import oat_amd.components as comp
    for cls in ("HotPath", "MotionTracker", "SubtractionTracker", "HSVDetector", "SimpleThreshold", "DifferenceDetector"):
        k = getattr(comp, cls)
        assert all(callable(getattr(k, m, None)) for m in ("set_tracks", "tracks", "update_tracks")), cls


@pytest.fixture(scope="module")
def host_bins():
    if not os.path.exists(os.path.join(BIN, "oat-posidet-hip")):
        subprocess.check_call(["make", "-s", "-j4", "-C", ROOT, "host"])
    return BIN


K = ["--kalman"]
REFUSALS = [
    (["diff", "src", "snk", "--track-sinks", "a,b"], "--track-sinks needs --kalman"),
    (["diff", "src", "snk", "--track-sinks", "1,2,3,4,5,6,7,8,9"] + K, "names 9 sinks, at most 8"),
    (["diff", "src", "snk", "--track-sinks", "a,b,a"] + K, "sink 'a' is named twice"),
    (["diff", "src", "snk", "--track-sinks", "a,snk"] + K, "sink 'snk' is named twice"),
    (["diff", "src", "snk", "--target-sinks", "a,b", "--track-sinks", "c,a"] + K, "sink 'a' is named twice"),
    (["diff", "src", "snk", "--track-sinks", "a,b", "--marker", "H=[0,10]"] + K, "--track-sinks does not go with --marker"),
    (["diff", "src", "snk", "--target-sinks", "a", "--track-sinks", "b,c"] + K, "--track-sinks names 2 sinks, --target-sinks 1"),
    (["thresh", "src", "snk", "--track-sinks", "a,b"], "--track-sinks with TYPE thresh needs --bsub"),
    (["hsv", "src", "snk", "--track-sinks", "a,b"], "--track-sinks with TYPE hsv needs --bsub"),
    (["diff", "src", "snk", "--track-gate", "4"] + K, "--track-gate is a parameter of --track-sinks"),
    (["diff", "src", "snk", "--track-sinks", "a,b", "--track-gate", "-1"] + K, "--track-gate: expected pixels >= 0"),
    (["diff", "src", "snk", "--track-sinks", "a,b", "--track-gate", "nan"] + K, "--track-gate: expected pixels >= 0"),
]


@pytest.mark.parametrize("args,text", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_posidet_refuses_wrong_track_sinks(host_bins, args, text):
    r = subprocess.run([os.path.join(host_bins, "oat-posidet-hip")] + args, capture_output=True, text=True, timeout=20)
    assert r.returncode != 0 and text in r.stderr, (r.returncode, r.stderr)


def test_track_sinks_in_a_config_file_are_checked_the_same_way(host_bins, tmp_path):
    cfg = tmp_path / "c.toml"
    cfg.write_text('[det]\ntrack-sinks = "a,b,a"\nkalman = true\n')
    r = subprocess.run([os.path.join(host_bins, "oat-posidet-hip"), "diff", "src", "snk", "-c", str(cfg), "det"], capture_output=True,
                       text=True, timeout=20)
    assert r.returncode != 0 and "sink 'a' is named twice" in r.stderr, r.stderr
