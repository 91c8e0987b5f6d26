"""CPU tests of the subtraction tracker's test material and bindings (no GPU): the numpy model of the front end
(tests/bsub_cases.py) equals the oracle chain `framefilt mask -> bsub -> col HSV -> inRange` (GREY: bsub -> inRange) on every
shared case and frame -- the subtracted image byte for byte, the window bits --, the cases see detections, they tell each planted
wrong front end from the right one, and the seven entries are declared, exported and bound.  The oracle does not show its fp32
accumulator: the model's `acc`, which the GPU tests compare bit for bit, is checked here only through what it does to the
subtracted image and, on the planted half-way pixels, by value; beyond that the model is its own reference."""
import os
import re

import numpy as np
import pytest

import bsub_cases as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"oatgpu_set_bsub_tracker": 2, "oatgpu_bsub_reset": 2, "oatgpu_bsub_track_batch_dev": 4, "oatgpu_bsub_track_batch": 5,
           "oatgpu_bsub_track_sequence_dev": 5, "oatgpu_bsub_get_state": 4, "oatgpu_read_bsub_mask": 4}   # name -> arguments


def _model_run(c, wrong=None):
    """[t][s] -> (bits, bg, acc, d) of a model of every stream"""
    ms = []
    for s in range(c.n_streams):
        m = B.Model(c.alpha, wrong)
        if s in c.background:
            m.set_background(c.background[s])
        ms.append(m)
    return [[ms[s].front(f, c.roi_at(t, s)) for s, f in enumerate(fs)] for t, fs in enumerate(c.frames)]


@pytest.fixture(scope="module")
def runs():
    """Every case through the oracle chain and the right model, once: [(case, oracle [t][s], model [t][s])]."""
    out = []
    for c in B.cpu_cases():
        orcs = [B.Oracle(c, c.background.get(s)) for s in range(c.n_streams)]
        want = [[orcs[s].step(f, c.roi_at(t, s)) for s, f in enumerate(fs)] for t, fs in enumerate(c.frames)]
        out.append((c, want, _model_run(c)))
    return out


def test_the_model_equals_the_oracle_on_every_case_and_frame(runs):
    for c, want, got in runs:
        for t in range(len(c.frames)):
            for s in range(c.n_streams):
                (bits, bg, acc, d), (_, sub, thr, _) = got[t][s], want[t][s]
                assert (d == sub).all(), (c.name, t, s)
                assert ((thr > 0) == bits).all(), (c.name, t, s)
                assert bg.dtype == np.uint8 and (acc is None) == (s in c.background), (c.name, t, s)
                if acc is not None:
                    assert acc.dtype == np.float32


def test_the_cases_see_detections_and_the_planted_pixels_do_what_they_say(runs):
    for c, want, got in runs:
        hits = [want[t][s][0]["valid"] for t in range(1, len(c.frames)) for s in range(c.n_streams)]
        if c.alpha <= 0.05:
            assert 2 * sum(hits) >= len(hits), (c.name, sum(hits), len(hits))
        if c.alpha == 1.0:                        # the background IS the frame: nothing is left
            assert not any(w[2].any() for ws in want for w in ws), c.name
        if c.cols < 16 or c.roi is not None or c.background:
            continue
        plants = B.PLANTS_BGR if c.channels == 3 else B.PLANTS_GREY
        pos = B.plant_positions(c.rows, c.cols, len(plants))
        bits, bg, acc, d = got[1][0]
        if c.alpha == 0.0:
            one = (1,) * 3 if c.channels == 3 else 1
            assert not np.any(d[pos[0]]) and np.all(d[pos[1]] == one) and not np.any(d[pos[2]]), c.name
            if c.channels == 3:
                for p, (_, inside) in zip(pos[5:], B.EDGES_BGR):
                    assert bits[p] == inside, (c.name, p)
            else:
                assert [bool(bits[p]) for p in pos[5:]] == [True, False, True, False], c.name
        if c.alpha == 0.5:                        # 10.5 -> 10 and 11.5 -> 12: round half to even
            assert np.all(acc[pos[3]] == 10.5) and np.all(bg[pos[3]] == 10) and np.all(acc[pos[4]] == 11.5) and np.all(bg[pos[4]] == 12)


def _differs(a, b, state=True):
    for ta, tb in zip(a, b):
        for (bits, bg, acc, _), (bits2, bg2, acc2, _) in zip(ta, tb):
            if (bits != bits2).any():
                return True
            if state and ((bg != bg2).any() or (acc is not None and (acc != acc2).any())):
                return True
    return False


@pytest.mark.parametrize("wrong", B.WRONG)
def test_the_cases_tell_a_wrong_front_end_apart(runs, wrong):
    """In what the GPU tests compare: the window bits of every frame, and the background and its accumulator."""
    assert any(_differs(_model_run(c, wrong), got) for c, _, got in runs), wrong


@pytest.mark.parametrize("wrong", [w for w in B.WRONG if w not in ("half_up", "acc_on_bg", "first_not_acc", "fused")])
def test_the_window_bits_alone_tell_these_apart(runs, wrong):
    assert any(_differs(_model_run(c, wrong), got, state=False) for c, _, got in runs), wrong


def test_the_right_model_is_not_told_apart(runs):
    assert not any(_differs(_model_run(c), got) for c, _, got in runs)


def test_only_the_accumulator_shows_a_contracted_multiply_add():
    """accumulateWeighted rounds the two products and the sum separately; a fused multiply-add rounds once.  On 12 noise frames
    of 90 x 200 x 3 at alpha 0.01 most ACCUMULATORS differ between the two (39 812 of 54 000; 36 045 at alpha 0.05) and no
    background byte does: a short test sees a contraction only in the fp32 state, which is why the GPU tests compare it bit for
    bit."""
    rng = np.random.default_rng(5)
    frames = [rng.integers(0, 256, (90, 200, 3)).astype(np.uint8) for _ in range(12)]
    for alpha in (0.01, 0.05):
        right, fused = B.Model(alpha), B.Model(alpha, "fused")
        for f in frames:
            _, bg, acc, _ = right.front(f)
            _, bg2, acc2, _ = fused.front(f)
        n_acc, n_bg = int((acc != acc2).sum()), int((bg != bg2).sum())
        print(f"alpha {alpha}: {n_acc} of {acc.size} accumulators differ, {n_bg} background bytes")
        # what the GPU tests rely on: the accumulators show a contraction; and why they must: the bytes all but hide it (a byte
        # changes only where the accumulator sits within an ulp of a half, 2^-17 of the pixels at these magnitudes)
        assert n_acc > 0, (alpha, n_acc)
        assert 100 * n_bg < n_acc, (alpha, n_bg, n_acc)


def test_the_header_declares_the_entries_and_the_binding_binds_them():
    from oat_amd import ffi
    src = open(os.path.join(ROOT, "include", "oatgpu.h")).read()
    listed = src[src.index("Further additive entries"):src.index("enum {")]
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in ENTRIES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, f"{name} is not declared in include/oatgpu.h"
        assert len(m.group(1).split(",")) == nargs, name
        assert name in listed, f"{name} is not in the header's list of additive entries"
        assert name in ffi.SIGNATURES, f"{name} is not bound"
        assert len(ffi.SIGNATURES[name][1]) == nargs, name
    lib = ffi.load()                              # (AttributeError for a symbol the built library does not export)
    for name in ENTRIES:
        assert len(getattr(lib, name).argtypes) == ENTRIES[name]


def test_subtraction_tracker_is_exported():
    import oat_amd
    assert hasattr(oat_amd, "SubtractionTracker") and "SubtractionTracker" in oat_amd.__all__
    for m in ("track", "track_dev", "track_sequence_dev", "reset", "set_background", "state", "read_mask", "set_roi_mask"):
        assert callable(getattr(oat_amd.SubtractionTracker, m)), m
