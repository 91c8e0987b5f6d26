"""The blob stage's LDS-kernel limits, on the CPU: tests/blob_load.py restates what k_blob_lds counts; here it is checked
on hand-counted masks and against scipy, its constants against the kernel sources, and every GPU edge case
(tests/test_blob_limits_gpu.py) against the counts it is meant to land on."""
import os
import re

import numpy as np
import pytest

import blob_load as B
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oat_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _final(raw, ero, dil):
    f = raw * np.uint8(255)
    if ero:
        f = O.erode(f, ero)
    if dil:
        f = O.dilate(f, dil)
    return f


# ------------------------------------------------------------------------------------- the sources' limits ---

def test_kernel_constants_are_the_edge_tables():
    s, rs = _src("kernels_bloblds.hip"), _src("kernels_rowscan.hip")
    consts = {k: int(v) for k, v in re.findall(r"\b(kLds(?:Rows|Runs|Roots|Block|Trip))\s*=\s*(\d+)", s)}
    assert consts == dict(kLdsRows=B.LDS_ROWS, kLdsRuns=B.LDS_RUNS, kLdsRoots=B.LDS_ROOTS, kLdsBlock=B.LDS_BLOCK,
                          kLdsTrip=B.LDS_TRIP)
    # phase A: row counts in registers while a thread owns <= 4 rows; phase E: 16 / 8 / 4 threads a run
    assert set(re.findall(r"if \(per <= (\d+)\)", s)) == {str(B.PHASE_A_ROWS)}
    assert re.search(r"int ric\[(\d+)\]", s).group(1) == str(B.PHASE_A_ROWS)
    assert re.findall(r"NF \* (\d+)u <= \(unsigned\)kLdsBlock \? (\d) :", s) == [("16", "4"), ("8", "3")]
    # k_rowscan: one lane per word, chunks of 64 words
    assert len(re.findall(r"for \(int c0 = 0; c0 < g\.words; c0 \+= 64\)", rs)) == 2
    assert B.ROWSCAN_CHUNK_PX == 64 * 64


def test_lds_geometry_rule_is_stated_alike_in_both_places():
    rule = re.compile(r"const bool (lds_able|lds_geom) = ([^;]*);")
    found = dict(rule.findall(_src("kernels_blob.hip")))
    found.update(rule.findall(_src("api_track.hip")))
    assert set(found) == {"lds_able", "lds_geom"}
    a, g = (" ".join(found[k].split()) for k in ("lds_able", "lds_geom"))
    assert a == g, (a, g)
    assert a == f"g.H > 2 && g.H <= {B.GEOM_MAX} && g.W <= {B.GEOM_MAX}", a


def test_edge_table_straddles_every_limit():
    cases = B.edge_cases()
    exp = {n: c[5] for n, c in cases.items()}

    def values(key, **where):
        return {e[key]: e["path"] for e in exp.values() if key in e and all(e.get(k) == v for k, v in where.items())}
    assert {B.LDS_RUNS - 1: "lds", B.LDS_RUNS: "lds", B.LDS_RUNS + 1: "global"}.items() <= values("R").items()
    assert {B.LDS_ROOTS - 1: "lds", B.LDS_ROOTS: "lds", B.LDS_ROOTS + 1: "global"}.items() <= values("NR").items()
    assert {B.LDS_ROWS: "lds", B.LDS_ROWS + 1: "global"}.items() <= values("D").items()
    assert exp[f"rows_{B.LDS_ROWS}"]["R"] == B.LDS_RUNS                 # the D edge is also the R edge
    nf = {e["NF"]: (e["lanes"], e["passes"]) for e in exp.values() if "lanes" in e}
    blk = B.LDS_BLOCK
    assert nf == {blk // 16: (16, 1), blk // 16 + 1: (8, 1), blk // 8: (8, 1), blk // 8 + 1: (4, 1),
                  blk // 4: (4, 1), blk // 4 + 1: (4, 2)}
    per_trip = B.LDS_TRIP * B.LDS_BLOCK // 64
    assert {1, 2} == {e["trips"] for e in exp.values() if "trips" in e}
    assert {per_trip, per_trip + 1} <= {e["D"] for e in exp.values() if "trips" in e}
    tall = B.PHASE_A_ROWS * B.LDS_BLOCK
    heights = {c[0]: (c[5]["path"], c[5]["phase_a"]) for n, c in cases.items() if n.startswith("height_")}
    assert heights == {3: ("lds", "registers"), tall: ("lds", "registers"), tall + 1: ("lds", "loop"),
                       B.GEOM_MAX: ("lds", "loop"), 2: ("global", "registers"), B.GEOM_MAX + 1: ("global", "loop")}
    widths = {c[1]: c[5]["path"] for n, c in cases.items() if n.startswith("width_")}
    assert widths[B.GEOM_MAX] == "lds" and widths[B.GEOM_MAX + 1] == "global"
    assert {B.ROWSCAN_CHUNK_PX, B.ROWSCAN_CHUNK_PX + 1} <= set(widths)


# ------------------------------------------------------------------------------------- the restatement ---

def _mask(h, w, pix):
    m = np.zeros((h, w), np.uint8)
    for y, x in pix:
        m[y, x] = 1
    return m


def test_blob_load_on_hand_counted_masks():
    def counts(m):
        L = B.blob_load(m)
        return L["D"], L["R"], L["NF"], L["NR"]
    assert counts(np.zeros((5, 5), np.uint8)) == (0, 0, 0, 0)
    assert counts(_mask(5, 5, [(2, 2)])) == (1, 3, 1, 1)
    assert counts(_mask(6, 6, [(2, 2), (3, 3)])) == (2, 6, 2, 1)              # 8-connected diagonal
    assert counts(_mask(6, 6, [(2, 3), (3, 2)])) == (2, 6, 2, 1)              # ... both ways
    assert counts(_mask(7, 7, [(2, 2), (4, 2)])) == (2, 6, 2, 2)              # a row apart: two
    assert counts(np.ones((6, 6), np.uint8)) == (4, 12, 4, 1)                 # the frame is zeroed first
    ring = np.zeros((11, 11), np.uint8)
    ring[2:9, 2:9] = 1
    ring[3:8, 3:8] = 0
    ring[5, 5] = 1                                                            # a component inside the hole
    # rows 2 and 8: one run; rows 3, 4, 6, 7: two walls; row 5: wall, dot, wall
    assert counts(ring) == (7, 33, 13, 2)
    comb = np.zeros((8, 20), np.uint8)
    comb[1:5, 2:4] = 1
    comb[1:3, 6:9] = 1
    comb[2, 11] = 1                                                            # rows 1..4: 2, 3, 1, 1 fg runs
    assert counts(comb) == (4, 2 * 7 + 4, 7, 3)
    L = B.blob_load(comb)
    assert (L["path"], L["lanes"], L["passes"], L["phase_a"], L["trips"], L["chunks"]) == ("lds", 16, 1, "registers", 1, 1)


def test_blob_load_branches_follow_the_kernels_thresholds():
    tall = np.zeros((4 * 1024 + 1, 8), np.uint8)
    assert B.blob_load(tall[:-1])["phase_a"] == "registers" and B.blob_load(tall)["phase_a"] == "loop"
    assert B.blob_load(np.zeros((2, 8), np.uint8))["path"] == "global"
    assert B.blob_load(np.zeros((3, 8), np.uint8))["path"] == "lds"
    assert B.blob_load(np.zeros((4, 16384), np.uint8))["path"] == "global"
    assert B.blob_load(np.zeros((4, 16383), np.uint8))["chunks"] == 4


@pytest.mark.parametrize("seed", range(6))
def test_blob_load_components_match_scipy(seed):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(seed)
    h, w = int(rng.integers(3, 120)), int(rng.integers(3, 300))
    for dens in (0.05, 0.3, 0.5, 0.7):
        m = B.frame_zeroed(rng.random((h, w)) < dens)
        if seed % 2:
            m = B.frame_zeroed(O.dilate(m * np.uint8(255), 2))
        n = ndimage.label(m, structure=np.ones((3, 3), int))[1]
        assert B.blob_load(m)["NR"] == n, (seed, dens)


# ------------------------------------------------------------------------------------- the GPU cases' masks ---

@pytest.mark.parametrize("name", sorted(B.edge_cases()))
def test_edge_case_lands_on_its_counts(name):
    ndimage = pytest.importorskip("scipy.ndimage")
    H, W, ero, dil, build, exp = B.edge_cases()[name]
    raw = build()
    assert raw.shape == (H, W) and raw.dtype == np.uint8 and set(np.unique(raw)) <= {0, 1}
    final = B.frame_zeroed(_final(raw, ero, dil))
    L = B.blob_load(final)
    assert {k: L[k] for k in exp} == exp, (name, L)
    assert L["NR"] == ndimage.label(final, structure=np.ones((3, 3), int))[1]


@pytest.mark.parametrize("shape", B.PIPELINE_SHAPES)
def test_pipeline_masks_land_on_their_counts(shape):
    for kind, (m, exp) in B.pipeline_masks(*shape).items():
        assert m.shape == shape
        assert (B.frame_zeroed(m) == m).all(), kind                          # nothing on the frame: thr == final
        L = B.blob_load(m)
        assert {k: L[k] for k in exp} == exp, (kind, L)
