"""CPU tests of the motion tracker's test material and bindings (no GPU): the numpy model of the front end
(tests/diff_cases.py) equals the oracle chain `framefilt mask -> col GREY -> posidet diff` on every shared case, the cases
see detections and empty frames, they tell each planted wrong front end from the right one, and the six entries are declared,
exported and bound."""
import os
import re

import numpy as np
import pytest

import diff_cases as D
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"oatgpu_set_diff_tracker": 2, "oatgpu_diff_reset": 2, "oatgpu_diff_batch_dev": 3, "oatgpu_diff_batch": 4,
           "oatgpu_diff_sequence_dev": 4, "oatgpu_read_diff_mask": 4}      # name -> number of arguments


@pytest.fixture(scope="module")
def runs():
    """Every case through the oracle, once: [(case, [t][s] -> (detection, thr image))]."""
    out = []
    for c in D.cpu_cases():
        orcs = [O.Diff(c.rows, c.cols, c.diff_threshold, c.blur, *D.AREA) for _ in range(c.n_streams)]
        res = [[orcs[s].detect(D.oracle_frame(f, c.roi_at(t, s))) for s, f in enumerate(fs)] for t, fs in enumerate(c.frames)]
        out.append((c, res))
    return out


def _model_run(c, wrong=None):
    ms = [D.Model(c.diff_threshold, c.blur, wrong=wrong) for _ in range(c.n_streams)]
    return [[ms[s].detect(f, c.roi_at(t, s)) for s, f in enumerate(fs)] for t, fs in enumerate(c.frames)]


def _differs(c, got, want):
    """Does a model run differ from the oracle's anywhere -- in a detection or in the mask the contours are taken from?"""
    for t in range(len(c.frames)):
        for s in range(c.n_streams):
            (det, _, mask), (odet, othr) = got[t][s], want[t][s]
            if not D.same_dict(det, odet) or ((othr > 0) != mask).any():
                return True
    return False


def test_the_model_equals_the_oracle_on_every_case(runs):
    for c, want in runs:
        got = _model_run(c)
        for t in range(len(c.frames)):
            for s in range(c.n_streams):
                (det, _, mask), (odet, othr) = got[t][s], want[t][s]
                assert ((othr > 0) == mask).all(), (c.name, t, s)
                assert D.same_dict(det, odet), (c.name, t, s, det, odet)


def test_the_cases_see_detections_and_empty_frames(runs):
    empty = 0
    for c, want in runs:
        later = [want[t][s][0]["valid"] for t in range(1, len(c.frames)) for s in range(c.n_streams)]
        if c.diff_threshold == 255:
            assert not any(later), c.name       # no difference of two bytes exceeds 255: nothing can be found after frame 0
        else:
            assert 2 * sum(later) >= len(later), (c.name, sum(later), len(later))
        empty += len(later) - sum(later)
        for t in D.STILL:                        # the rectangle has not moved: the difference is empty
            for s in range(c.n_streams):
                assert not want[t][s][0]["valid"] and not want[t][s][1].any(), (c.name, t, s)
    assert empty > 0


@pytest.mark.parametrize("wrong", D.WRONG)
def test_the_cases_tell_a_wrong_front_end_apart(runs, wrong):
    assert any(_differs(c, _model_run(c, wrong), want) for c, want in runs), wrong


def test_the_right_model_is_not_told_apart(runs):
    assert not any(_differs(c, _model_run(c), want) for c, want in runs)


def test_the_header_declares_the_entries_and_the_binding_binds_them():
    from oat_amd import ffi
    src = open(os.path.join(ROOT, "include", "oatgpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in ENTRIES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert m, f"{name} is not declared in include/oatgpu.h"
        assert len(m.group(1).split(",")) == nargs, name
        assert name in ffi.SIGNATURES, f"{name} is not bound"
        assert len(ffi.SIGNATURES[name][1]) == nargs, name
    lib = ffi.load()
    for name in ENTRIES:
        assert len(getattr(lib, name).argtypes) == ENTRIES[name]


def test_motion_tracker_is_exported():
    import oat_amd
    assert hasattr(oat_amd, "MotionTracker") and "MotionTracker" in oat_amd.__all__
    for m in ("track", "track_dev", "track_sequence_dev", "reset", "read_mask", "set_roi_mask"):
        assert callable(getattr(oat_amd.MotionTracker, m)), m
