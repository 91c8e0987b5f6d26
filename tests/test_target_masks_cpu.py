"""Conditions on the model and the cases of target masks alone (tests/target_masks_ref.py, tests/target_masks_cases.py):
no GPU.  The labelling against scipy and against a scalar restatement; what every designed sequence must hold for the GPU tests to
mean anything; twelve planted wrong implementations, each of which must differ from the model on a case; the header's text, the
binding, the exports."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import crops_cases as CC
import crops_ref as R
import target_masks_cases as MC
import target_masks_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("oatgpu_set_target_mask_tensor", "oatgpu_target_mask_tensor_sets")
COND_K, COND_HW = 4, (16, 12)                # the setting the designed sequences' conditions are checked at


def _case_masks():
    """every mask a GPU run labels: (tag, mask)"""
    seen = set()
    for kind, family, alpha, rows, cols, n, k, h, w in MC.RUNS:
        for v in {MC.variant_of(s) for s in range(n)}:
            key = (kind, family, rows, cols, v, alpha)
            if key not in seen:
                seen.add(key)
                for t, m in enumerate(MC.sequence_masks(*key)):
                    yield key + (t,), m


# ------------------------------------------------------------------------------------------------------------ the model ----

def test_label8_is_scipys_labelling_on_every_case_mask():
    ndimage = pytest.importorskip("scipy.ndimage")
    count = 0
    for tag, m in _case_masks():
        first = MR.label8(m)
        lab, n = ndimage.label(MR.zero_frame(m), structure=np.ones((3, 3), int))
        assert ((first >= 0) == (lab > 0)).all(), tag
        for i in range(1, n + 1):
            ys, xs = np.nonzero(lab == i)
            seed = int(ys[0]) * m.shape[1] + int(xs[np.nonzero(ys == ys[0])[0][0]])      # np.nonzero is in raster order
            assert (first[lab == i] == seed).all(), (tag, i)
        count += n
    assert count > 500


def test_the_designs_hold_what_membership_can_get_wrong():
    for rows, cols in MC.GEOMETRIES:
        d = MC.design(rows, cols, "full", 0).astype(np.uint8)
        first, four = MR.label8(d), MR.labels_for(d, "four_connected")
        comps = {int(s): first == s for s in np.unique(first[first >= 0])}
        # the two squares: one component under 8-connectivity, two under 4
        assert first[2, 14] == first[7, 19] >= 0 and four[2, 14] != four[7, 19]
        # the ring's hole holds a blob of another component
        assert first[9, 2] >= 0 and first[12, 5] >= 0 and first[12, 5] != first[9, 2] and first[10, 3] < 0
        # the blob on the edge lost its first row and column
        assert d[0, 0] and d[0, 5] and first[0, 5] < 0 and first[3, 0] < 0 and first[1, 1] == 1 * cols + 1
        # two ranked blobs one column apart, and a blob below the area window beside them
        ranks, found = MC.T.reference(d * 255, MC.AREA, 8)
        fps = {r["first_pixel"] for r in ranks if r["valid"]}
        assert int(first[11, 12]) in fps and int(first[11, 18]) in fps and first[11, 12] != first[11, 18] and first[11, 17] < 0
        assert first[18, 14] >= 0 and int(first[18, 14]) not in fps
        assert found == (8 if cols >= 140 else 7)
        # the comb and the staircase: run heads in more than three rows (or teeth) that meet only further down
        comb, stair = comps[int(first[1, 24])], comps[int(first[10, 44])]
        assert comb[1, 24] and comb[1, 32] and not comb[1, 25] and comb[8, 28]
        heads = [int(np.nonzero(stair[y])[0][0]) for y in range(10, 18)]
        assert heads == sorted(heads, reverse=True) and len(set(heads)) == 8
        if cols >= 140:
            # a run through both word boundaries, and a component that is one only through it
            run = first[4, 62:130]
            assert (run == first[2, 58]).all() and first[2, 58] == first[6, 133] >= 0
            cut = d.copy()
            cut[4, 64] = 0
            assert MR.label8(cut)[2, 58] != MR.label8(cut)[6, 133]
            assert (MR.labels_for(d, "head_in_word")[4, 64:128] < 0).all()
    few = MC.design(21, 150, "few", 2).astype(np.uint8) * 255
    assert MC.T.reference(few, MC.AREA, 4)[1] == 2


def test_a_scalar_restatement_of_one_element_is_the_array_form():
    rng = np.random.default_rng(77)
    checked = on = 0
    for kind, family, rows, cols, zoom, axis, t in (("designed", "motion", 21, 150, 1.37, True, 1), ("designed", "subtraction", 37, 61, 1.0, False, 2),
                                                    ("designed", "subtraction", 48, 64, 0.5, True, 3), ("designed", "motion", 37, 61, 2.0, False, 6),
                                                    ("mix", "motion", 48, 64, 1.37, True, 5), ("mix", "subtraction", 37, 61, 2.0, True, 6)):
        h, w = COND_HW
        mask = MC.sequence_masks(kind, family, rows, cols, 1, 0.0)[t]
        ranks = MC.sequence_targets(kind, family, rows, cols, 1, 0.0, COND_K)[t][0]
        wins = MC.sequence_windows(kind, family, rows, cols, 1, 0.0, COND_K, axis, zoom)[t]
        got = MR.windows_mask(mask, ranks, wins, h, w, "uint8")
        assert np.array_equal(got != 0, MC.sequence_on(kind, family, rows, cols, 1, 0.0, COND_K, axis, zoom, h, w)[t])
        for j in range(COND_K):
            for i, x in zip(rng.integers(0, h, 40), rng.integers(0, w, 40)):
                want = MR.element_scalar(mask, ranks[j], wins[j], h, w, int(i), int(x))
                assert bool(got[j, i, x]) == want and got[j, i, x] in (0, 255), (kind, family, t, j, i, x)
                checked += 1
                on += want
    assert checked > 900 and 50 < on < checked - 50


def test_values_by_dtype():
    on = np.array([[True, False]])
    assert MR.to_dtype(on, "uint8").tolist() == [[255, 0]] and MR.to_dtype(on, "uint8").dtype == np.uint8
    for d in ("float16", "float32"):
        v = MR.to_dtype(on, d)
        assert v.tolist() == [[1.0, 0.0]] and v.dtype == np.dtype(d)


# -------------------------------------------------------------------------------------------- conditions on the sequences ----

def _window_facts(kind, family, rows, cols, zoom, axis, t):
    """of frame t at the conditions' setting: (a window with ON and with foreground OFF elements, a valid window the frame clips, an
    invalid rank behind a valid one)"""
    h, w = COND_HW
    first = MC.sequence_labels(kind, family, rows, cols, 0, 0.0)[t]
    ranks = MC.sequence_targets(kind, family, rows, cols, 0, 0.0, COND_K)[t][0]
    wins = MC.sequence_windows(kind, family, rows, cols, 0, 0.0, COND_K, axis, zoom)[t]
    both = clipped = False
    for rank, win in zip(ranks, wins):
        if not rank["valid"] or not R.is_valid(win):
            continue
        x, y, ok = MR.source_pixels(win, h, w)
        inside = ok & (x >= 0) & (x < cols) & (y >= 0) & (y < rows)
        fg = inside & (first[np.clip(y, 0, rows - 1), np.clip(x, 0, cols - 1)] >= 0)
        on = MR.window_on(first, rank, win, h, w)
        both |= bool(on.any() and (fg & ~on).any())
        clipped |= bool((~inside).any() and inside.any())
    valid = [r["valid"] for r in ranks]
    return both, clipped, any(valid[j] and not valid[j + 1] for j in range(COND_K - 1))


@pytest.mark.parametrize("family", MC.FAMILIES)
@pytest.mark.parametrize("rows,cols", MC.GEOMETRIES)
def test_every_designed_sequence_has_the_three_conditions_in_one_entry(family, rows, cols):
    for zoom in MC.ZOOMS:
        for axis in (False, True):
            facts = [_window_facts("designed", family, rows, cols, zoom, axis, t) for t in range(MC.N_FRAMES)]
            assert any(all(f) for f in facts), (family, rows, cols, zoom, axis, facts)


def test_at_zoom_1_37_rint_and_the_contract_part():
    """a sampled position whose fraction lies in [15.5/32, 0.5): rint(X) is the pixel below, the nearest 1/32 step rounds to the one above"""
    h, w = COND_HW
    hits = 0
    jj, ii = np.arange(w) - w // 2, np.arange(h) - h // 2
    for kind, family, alpha, rows, cols, n, k, _, _ in MC.RUNS:
        for v in sorted({MC.variant_of(s) for s in range(n)}):
            for axis in (False, True):
                for wins in MC.sequence_windows(kind, family, rows, cols, v, alpha, k, axis, 1.37):
                    for win in wins:
                        if not R.is_valid(win):
                            continue
                        _, _, cx, cy, ax, ay = win
                        X = (cx + jj[None, :] * ax) - ii[:, None] * ay
                        Y = (cy + jj[None, :] * ay) + ii[:, None] * ax
                        x, y, _ = MR.source_pixels(win, h, w)
                        xr, yr, _ = MR.source_pixels(win, h, w, "rint_x")
                        for pos, got, plain in ((X, x, xr), (Y, y, yr)):
                            frac = pos - np.floor(pos)
                            part = (frac >= 15.5 / 32) & (frac < 0.5)
                            assert ((got != plain) >= part).all()      # wherever the fraction lies there, the two rules part
                            hits += int(part.sum())
    assert hits >= 1


# ------------------------------------------------------------------------------------------- planted wrong implementations ----

def _runs_for(wrong):
    if wrong == "head_in_word":
        return [r for r in MC.DESIGNED_RUNS if r[4] >= 140]
    return MC.DESIGNED_RUNS + MC.MIX_RUNS[:2]


@pytest.mark.parametrize("wrong", MR.WRONG_LABEL + MR.WRONG_PIXEL + MR.WRONG_VALUE)
def test_a_planted_wrong_rule_differs_from_the_model(wrong):
    differs = 0
    for run in _runs_for(wrong):
        for axis, (zoom, dtype) in ((False, (1.0, "uint8")), (True, (1.37, "uint8"))):
            if wrong in MR.WRONG_PIXEL and zoom == 1.0:
                continue
            for t in range(1, 5):
                differs += not np.array_equal(MC.entry(run, t, axis, zoom, dtype), MC.entry(run, t, axis, zoom, dtype, wrong))
    assert differs >= 1, wrong


@pytest.mark.parametrize("wrong", MR.WRONG_ENTRY)
def test_a_planted_wrong_delivery_differs_from_the_model(wrong):
    differs = 0
    for run in MC.DESIGNED_RUNS[:3] + MC.MIX_RUNS[3:5]:
        family = run[1]
        pairs = tuple(sorted(CC.paired_second(family, MC.PLAN_LONG)))
        assert pairs
        sets = [MC.entry(run, t, False, 1.0, "uint8") for t in range(MC.N_FRAMES)]
        bad = [MC.entry(run, t, False, 1.0, "uint8", wrong, pairs) for t in range(MC.N_FRAMES)] if wrong == "first_of_pair" else sets
        valid = [np.broadcast_to(MC.entry_valid(run, t)[..., None, None], sets[t].shape) for t in range(MC.N_FRAMES)]
        want = MR.deliver(MC.RUN_CALLS, sets, valid, MC.CAPACITY)
        got = MR.deliver(MC.RUN_CALLS, bad, valid, MC.CAPACITY, wrong)
        differs += any(not np.array_equal(a, b) for a, b in zip(want, got))
    assert differs >= 1, wrong


def test_twelve_wrong_implementations_are_planted():
    assert len(MR.WRONG) == 12 == len(set(MR.WRONG))


def test_every_zoom_meets_every_dtype_in_both_modes_over_the_runs():
    for axis in (False, True):
        seen = {s for case in range(len(MC.RUNS)) for s in MC.settings_of(case, axis)}
        assert seen == set(MC.COMBOS) and len(MC.COMBOS) == 12
    assert {r[7:] for r in MC.RUNS} == set(MC.MASK_SIZES)
    assert {r[6] for r in MC.RUNS} == {1, 4, 8} and {r[5] for r in MC.RUNS} == {1, 3, 66}
    assert {(r[1], r[3], r[4]) for r in MC.DESIGNED_RUNS} == {(f, *g) for f in MC.FAMILIES for g in MC.GEOMETRIES}


# --------------------------------------------------------------------------------------------- header, library, binding ----

@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(os.path.join(ROOT, "oat_amd", "lib", "liboatgpu.so")):
        subprocess.check_call(["make", "-s", "-j4", "-C", ROOT, "oat_amd/lib/liboatgpu.so"])
    from oat_amd import ffi
    return ffi.load()


def test_target_masks_are_declared_exported_and_bound(lib):
    from oat_amd import ffi
    header = open(os.path.join(ROOT, "include", "oatgpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(lib, name) and name in ffi.SIGNATURES
    assert ffi.SIGNATURES["oatgpu_set_target_mask_tensor"][1] == [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32,
                                                                  C.c_void_p, C.c_int32]
    assert ffi.SIGNATURES["oatgpu_target_mask_tensor_sets"][1] == [C.c_void_p]
    assert re.search(r"#define\s+OATGPU_ABI_VERSION\s+9\b", header)
    assert ffi.ABI_VERSION == 9 == lib.oatgpu_abi_version()                     # additive entries: the version stays


def test_the_header_states_the_semantics():
    header = open(os.path.join(ROOT, "include", "oatgpu.h")).read()
    text = " ".join(" ".join(re.sub(r"^\s*\*\s", "", line) for line in header.splitlines()).split())
    assert "target masks:" in text
    for words in ("(rint(cx) - w/2 + j, rint(cy) - h/2 + i)", "qx = rint(32 * X), qy = rint(32 * Y)", "((qx + 16) >> 5, (qy + 16) >> 5)",
                  "arithmetic shifts", "a mask and a crop tensor of the same setting are aligned", "the source pixel is inside the frame",
                  "with the one-pixel frame zeroed", "8-connected component whose first pixel in raster order is this rank's first_pixel",
                  "a blob inside this blob's hole", "255 / 0 for OATGPU_TENSOR_U8", "1.0 / 0.0 for OATGPU_TENSOR_F16 and OATGPU_TENSOR_F32",
                  "[sets][n][K][h][w]", "There is no channel axis", "goes into entry t, not into the tracker's slot",
                  "entries past the delivered count are not touched", "before anything is launched and with nothing changed",
                  "independent of oatgpu_set_target_crops and oatgpu_set_target_crop_tensor", "it is NOT refused with either front end",
                  "deliver none and reset the count", "the switch allocates nothing"):
        assert words.lower() in text.lower(), words


def test_every_detector_class_has_target_masks():
    import oat_amd.components as comp
    for cls in ("HotPath", "MotionTracker", "SubtractionTracker", "HSVDetector", "SimpleThreshold", "DifferenceDetector"):
        k = getattr(comp, cls)
        assert all(callable(getattr(k, m, None)) for m in ("set_target_mask_tensor", "target_mask_tensor")), cls
    for name in ("ffi.py", "components.py"):
        src = open(os.path.join(ROOT, "oat_amd", name)).read()
        assert not re.search(r"^(import torch|from torch)", src, flags=re.M), name


def test_the_new_units_are_in_the_makefile_lists_and_share_one_definition():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    kernels = re.search(r"^KERNELS\s*=(.*)$", mk, flags=re.M).group(1).split()
    api = re.search(r"^API\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "kernels_targetmask" in kernels and "api_targetmask" in api
    csrc = os.path.join(ROOT, "oat_amd", "csrc")
    defs = {}
    for f in (f for f in os.listdir(csrc) if f.endswith((".hip", ".h"))):
        for fn in re.findall(r"^__device__ __forceinline__ \w+ (run_head|run_head_w|uf_root|msb64|low_mask_incl)\(", open(os.path.join(csrc, f)).read(), flags=re.M):
            defs.setdefault(fn, []).append(f)
    assert defs == {fn: ["blobruns_inline.h"] for fn in ("run_head", "run_head_w", "uf_root", "msb64", "low_mask_incl")}, defs
