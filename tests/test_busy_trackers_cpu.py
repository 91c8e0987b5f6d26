"""The busy-frame cases of the two batched trackers (tests/busy_tracker_cases.py) held to the models and the oracle, without
a GPU: every exact construction gives the intended final mask bit for bit and blob_load puts it on the declared side of
k_blob_lds' capacity; the schedules meet the conditions the GPU file counts on; the expected detections tell a right back half
from a stale or mis-indexed one -- shown on four planted wrong back halves, run on the oracle's results alone.

(That the oracle -- O.Diff, bsub_cases.Oracle -- and the numpy models agree on every frame is asserted where the cases are
built: DiffRun.step_masks, BsubRun.step_masks.)"""
import numpy as np
import pytest

import blob_load as L
import busy_tracker_cases as K
import diff_cases as D

ALL_SHAPES = K.SHAPES + (K.MANY,)
STD = [(r, c, ch, n) for r, c in ALL_SHAPES for ch in (3, 1) for n in (1, 3)]


def _diff(a, b):
    return not D.same_dict(a, b)


def _all_steps():
    """every list of Steps the GPU file runs, by name"""
    out = {}
    for r, c, ch, n in STD:
        out[f"diff-{r}x{c}-ch{ch}-n{n}"] = K.diff_standard(r, c, ch, n)
        out[f"bsub-{r}x{c}-ch{ch}-n{n}"] = K.bsub_standard(r, c, ch, n)[1]
    for ch in (3, 1):
        out[f"diff-reset-ch{ch}"] = K.diff_reset_in_front(ch)
        out[f"bsub-reset-ch{ch}"] = K.bsub_reset_in_front(ch)[1]
    for n in K.MIXED:
        out[f"diff-mixed-n{n}"] = [st for _, st in K.diff_mixed(n, 0)]
    out["diff-many"] = K.diff_many()
    out["bsub-many"] = K.bsub_many()[1]
    out["shared"] = list(K.shared_steps()[1].values())
    return out


# ------------------------------------------------------------------------------------------------- the constructions ----

@pytest.mark.parametrize("rows,cols", ALL_SHAPES)
def test_the_tag_changes_neither_the_counts_nor_the_path(rows, cols):
    masks = L.pipeline_masks(rows, cols)
    for kind in K.TAGGED:
        plain = K.load_of(K._bases(rows, cols)[kind][0])
        if kind in masks:
            exp = masks[kind][1]
            assert {q: plain[q] for q in exp} == exp, (kind, plain)
        seen = set()
        for s, t in ((0, 0), (1, 0), (0, 1), (2, 5), (65, 6), (19, 0), (7, 15)):
            m = K.mask_of(rows, cols, kind, s, t)
            got = K.load_of(m)
            assert got == plain, (kind, s, t, got, plain)
            assert m.sum() > K._bases(rows, cols)[kind][0].sum()
            seen.add(m.tobytes())
        assert len(seen) == 7, kind
    assert K.load_of(K.mask_of(rows, cols, "empty", 1, 2))["D"] == 0
    noise = K.load_of(K.mask_of(rows, cols, "noise", 1, 2))
    assert noise["path"] == "global" and noise["R"] >= 4 * L.LDS_RUNS, noise


def test_tags_are_distinct_where_the_cases_need_them():
    for t in range(K.N_STANDARD + 4):
        assert len({K.tag(s, t) for s in range(K.N_MANY)}) == K.N_MANY
        for s in (0, 1, 2, 65):
            assert K.tag(s, t) != K.tag(s, t + 1) and K.tag(s, t) != K.tag(s, t + 4)


def test_exact_cases_give_the_intended_mask_on_the_declared_path():
    n_global = n_lds = 0
    for name, steps in _all_steps().items():
        for st in steps:
            for s, kind in enumerate(st.kinds):
                assert st.intended[s] is not None, (name, st.t, s)
                assert (st.final[s] == st.intended[s]).all(), (name, st.t, s, kind)
                assert st.path[s] == K.DECLARED[kind], (name, st.t, s, kind, K.load_of(st.final[s]))
                n_global += st.path[s] == "global"
                n_lds += st.path[s] == "lds"
    assert n_global > 500 and n_lds > 500


@pytest.mark.parametrize("channels", [3, 1])
def test_first_frames_of_the_subtraction_tracker_are_the_background(channels):
    _, steps = K.bsub_reset_in_front(channels)
    t0, s0 = K.RESET_FRONT["before"], K.RESET_FRONT["reset"]
    assert [st.first[s0] for st in steps] == [t == t0 for t in range(len(steps))]
    assert steps[t0].kinds[s0] == "empty" and not steps[t0].final[s0].any()
    assert not any(st.first[s] for st in steps for s in (0, 2))
    dsteps = K.diff_reset_in_front(channels)
    assert [st.first for st in dsteps] == [[t == 0, t in (0, t0), t == 0] for t in range(len(dsteps))]


def test_blurred_cases_stay_on_the_global_route():
    """blur 2: the final mask is the model's dilation of the intended mask; what was over capacity stays over it"""
    for r, c in K.SHAPES:
        steps = K.diff_standard(r, c, 3, 3, 2)
        for st in steps:
            for s, kind in enumerate(st.kinds):
                assert st.intended[s] is None
                if st.first[s]:
                    assert (st.final[s] == K.mask_of(r, c, kind, s, st.t)).all() and st.path[s] == K.DECLARED[kind]
                elif kind.endswith("_over"):
                    assert st.path[s] == "global" and st.final[s].sum() > K.mask_of(r, c, kind, s, st.t).sum()
        assert K.load_of(K.diff_standard(200, 360, 3, 3, 2)[1].final[0])["R"] > L.LDS_RUNS
    for n in K.MIXED:
        for _, st in K.diff_mixed(n, 2):
            assert st.path == ["global"] * n


@pytest.mark.parametrize("which", ["bsub-bgr", "bsub-grey", "bsub-raw", "diff-raw"])
def test_noise_forms_are_global_by_a_wide_margin(which):
    steps = {"bsub-bgr": lambda: K.bsub_standard(*K.SHAPES[0], 3, 3, 0.05)[1], "bsub-grey": lambda: K.bsub_standard(*K.SHAPES[1], 1, 3, 0.05)[1],
             "bsub-raw": lambda: K.bsub_raw()[1], "diff-raw": lambda: K.diff_raw()[1]}[which]()
    busy = quiet = 0
    for st in steps:
        for s, kind in enumerate(st.kinds):
            load = K.load_of(st.final[s])
            if kind == "noise":
                assert st.path[s] == "global" and load["R"] >= 2 * L.LDS_RUNS, (which, st.t, s, load)
                assert st.want[s]["valid"]
                busy += 1
            else:
                assert st.path[s] == "lds" and load["R"] <= L.LDS_RUNS // 8, (which, st.t, s, kind, load)
                assert st.want[s]["valid"] == (kind == "rect")
                quiet += 1
    assert busy >= 8 and quiet >= 8


def test_area_cases_over_capacity():
    cases = K.area_cases()
    for name, (mask, area) in cases.items():
        for ch in (3, 1):
            ds, (_, bs) = K.diff_area(name, ch), K.bsub_area(name, ch)
            for st in (ds, bs):
                assert (st.final[0] == mask).all() and st.path == ["global"], name
                assert D.same_dict(st.want[0], K.largest(mask, area))
    assert not K.diff_area("max_area_equal", 1).want[0]["valid"] and not K.diff_area("max_area_under", 1).want[0]["valid"]
    assert K.diff_area("min_area_equal", 1).want[0]["valid"]
    # the tie: the selected square is not the first in raster order
    ties = K.diff_area("ties", 1).want[0]
    assert ties["valid"] and ties["area"] == 1.0 and ties["first_pixel"] > int(np.argmax(cases["ties"][0].reshape(-1)))


# ------------------------------------------------------------------------------------------------------ the schedules ----

def _transitions(paths):
    """{slot: set of (previous occupant's path, path)} of a stream's frames in the sequence call's slots t % 4"""
    out = {q: set() for q in range(4)}
    for t in range(4, len(paths)):
        out[t % 4].add((paths[t - 4], paths[t]))
    return out


@pytest.mark.parametrize("tracker", ["diff", "bsub"])
@pytest.mark.parametrize("rows,cols,ch,n", STD)
def test_standard_schedule_conditions_counted_from_the_data(tracker, rows, cols, ch, n):
    steps = K.diff_standard(rows, cols, ch, n) if tracker == "diff" else K.bsub_standard(rows, cols, ch, n)[1]
    assert len(steps) >= 12
    for s in range(n):
        paths = [st.path[s] for st in steps]
        kinds = [st.kinds[s] for st in steps]
        for q, seen in _transitions(paths).items():
            assert {("lds", "global"), ("global", "lds"), ("global", "global")} <= seen, (s, q, seen)
        assert any(kinds[t] == "empty" and paths[t - 1] == "global" and paths[t - 4] == "global" for t in range(4, len(steps))), s
        assert {"runs_over", "roots_over"} <= {k for k, p in zip(kinds, paths) if p == "global"}
        # the prefixes the sequence tests run, from frame 0 and from frame 3: global behind lds and behind global in a slot
        for start in (0, 3):
            for nf in (8, 12, 13):
                flat = set().union(*_transitions(paths[start:start + nf]).values())
                assert {("lds", "global"), ("global", "lds"), ("global", "global")} <= flat, (s, start, nf)
    if n > 1:
        assert all(len(set(st.path)) == 2 for st in steps), "every frame set mixes global and lds streams"


def test_many_stream_case_layout():
    for steps in (K.diff_many(), K.bsub_many()[1]):
        assert len(steps) == K.MANY_FRAMES
        for st in steps:
            busy = [st.kinds[s] for s in K.MANY_BUSY]
            assert busy[0] != busy[1] and busy[2] != busy[3] and set(busy) == {"runs_over", "roots_over"}
            assert [s for s in range(K.N_MANY) if st.path[s] == "global"] == list(K.MANY_BUSY)
            assert all(st.kinds[s].endswith("_at") for s in K.MANY_AT)
            assert all(w["valid"] for w in st.want)
        for s in K.MANY_BUSY:
            assert {st.kinds[s] for st in steps} == {"runs_over", "roots_over"}


def test_mixed_first_frame_cases_issue_two_to_four_launches():
    for n, want in ((3, {2, 3}), (5, {2, 3, 4})):
        for blur in (0, 2):
            runs = K.diff_mixed(n, blur)
            counts = set()
            firsts = set()
            for t, (resets, st) in enumerate(runs):
                assert st.first == [t == 0 or s in resets for s in range(n)]
                la = K.launches(st.first)
                if t:
                    counts.add(len(la))
                    firsts |= {s0 for s0, _ in la}
            assert counts == want, (n, counts)
            assert firsts == set(range(n)), "every stream is once the first of a launch"
            assert any(st.first == [False] * (n - 1) + [True] for _, st in runs), "only the last stream fresh"


# ------------------------------------------------------------------------------------------------------- non-vacuity ----

@pytest.mark.parametrize("blur", [0, 2])
def test_every_global_frame_differs_from_what_a_wrong_back_half_could_hand_out(blur):
    cases = _all_steps()
    if blur:
        cases = {f"blur-{r}x{c}": K.diff_standard(r, c, 3, 3, 2) for r, c in K.SHAPES}
        cases.update({f"blur-mixed-n{n}": [st for _, st in K.diff_mixed(n, 2)] for n in K.MIXED})
    checked = 0
    for name, steps in cases.items():
        for i, st in enumerate(steps):
            for s, p in enumerate(st.path):
                if p != "global":
                    continue
                w = st.want[s]
                if not w["valid"]:
                    continue                                # (none in these cases; the area cases have a test of their own)
                if i >= 4 and "shared" not in name:
                    assert _diff(w, steps[i - 4].want[s]), (name, st.t, s, "the slot's previous occupant")
                if i >= 1:
                    assert _diff(w, steps[i - 1].want[s]), (name, st.t, s, "the frame before")
                for o in range(len(st.path)):
                    if o != s:
                        assert _diff(w, st.want[o]), (name, st.t, s, o, "another stream of the set")
                if s:
                    assert _diff(w, K.largest(st.final[0])), (name, st.t, s, "stream 0's mask")
                checked += 1
    assert checked > (50 if blur else 500)


# ------------------------------------------------------------------------------------------ planted wrong back halves ----
# Each takes the oracle's results of a scenario and hands out what a back half with ONE mistake on the global route would;
# the cases must catch every one of them (a mutant that equals the oracle everywhere would make the GPU test vacuous).

INVALID = dict(valid=False, area=0.0)


def _slot_of(i, in_flight):
    return i % 4 if in_flight else 0


def _previous_occupant(steps, i, s, in_flight):
    j = i - 4 if in_flight else i - 1
    return steps[j].want[s] if j >= 0 else INVALID


def stale_slot(steps, in_flight, launches=None):
    """a global frame gets what the slot's previous occupant left in the result record"""
    return [[_previous_occupant(steps, i, s, in_flight) if p == "global" else st.want[s] for s, p in enumerate(st.path)]
            for i, st in enumerate(steps)]


def lds_ok_of_first(steps, in_flight, launches):
    """lds_ok[first_stream + 0] decides for every stream of a launch: behind an lds stream the global kernels leave, and the
    declined streams keep the slot's previous result"""
    out = []
    for i, st in enumerate(steps):
        row = list(st.want)
        for s0, n in launches(st):
            if st.path[s0] == "lds":
                for s in range(s0, s0 + n):
                    if st.path[s] == "global":
                        row[s] = _previous_occupant(steps, i, s, in_flight)
        out.append(row)
    return out


def first_stream_ignored(steps, in_flight, launches):
    """k_merge / k_green_select without first_stream: stream s0 + i gets the result for stream i"""
    out = []
    for st in steps:
        row = list(st.want)
        for s0, n in launches(st):
            for i in range(n):
                if st.path[s0 + i] == "global":
                    row[s0 + i] = K.largest(st.final[i])
        out.append(row)
    return out


def _caught(steps, got):
    return any(_diff(g, w) for st, row in zip(steps, got) for g, w in zip(row, st.want))


def _one_launch(st):
    return [(0, len(st.path))]


def _diff_launches(st):
    return K.launches(st.first)


def test_planted_stale_slot_is_caught():
    for name, steps in _all_steps().items():
        if name == "shared":
            continue
        for in_flight in (False, True):
            if len(steps) > (4 if in_flight else 1):
                assert _caught(steps, stale_slot(steps, in_flight)), (name, in_flight)


def test_planted_lds_ok_of_the_first_stream_is_caught():
    for r, c, ch, n in STD:
        if n == 1:
            continue
        for in_flight in (False, True):
            assert _caught(K.diff_standard(r, c, ch, n), lds_ok_of_first(K.diff_standard(r, c, ch, n), in_flight, _diff_launches))
            steps = K.bsub_standard(r, c, ch, n)[1]
            assert _caught(steps, lds_ok_of_first(steps, in_flight, _one_launch))
    for steps in (K.diff_many(), K.bsub_many()[1]):
        # (stream 0 is busy there: the mistake shows on no stream -- which is why the standard schedule rotates)
        assert not _caught(steps, lds_ok_of_first(steps, True, _one_launch))


def test_planted_first_stream_ignored_is_caught():
    for n in K.MIXED:
        for blur in (0, 2):
            steps = [st for _, st in K.diff_mixed(n, blur)]
            got = first_stream_ignored(steps, False, _diff_launches)
            assert _caught(steps, got), (n, blur)
            # ... on every step with more than one launch, and for every launch behind the first
            for st, row in zip(steps[1:], got[1:]):
                for s0, cnt in K.launches(st.first)[1:]:
                    assert any(_diff(row[s], st.want[s]) for s in range(s0, s0 + cnt)), (n, blur, st.t, s0)
    steps = K.diff_reset_in_front(3)
    assert _caught(steps, first_stream_ignored(steps, True, _diff_launches))
    # a single launch from stream 0 cannot show it
    steps = K.diff_standard(*K.SHAPES[0], 3, 3)
    assert not _caught(steps[1:], first_stream_ignored(steps[1:], False, _diff_launches))


def test_planted_context_plane_instead_of_the_trackers_is_caught():
    """`fin` of the context's own scratch set read where the tracker's plane belongs: the global kernels see the mask of the
    previous ordinary call"""
    masks = K.shared_masks()
    _, steps = K.shared_steps()
    plane = [None] * K.SHARED_N
    caught = {"diff": 0, "bsub": 0}
    for i, (op, kinds) in enumerate(K.SHARED_OPS):
        if op in K.ORDINARY:
            for s, m in enumerate(masks[i]):
                if m is not None:
                    plane[s] = m
            continue
        st = steps[i]
        for s, p in enumerate(st.path):
            if p == "global":
                assert plane[s] is not None
                assert _diff(K.largest(plane[s]), st.want[s]), (i, op, s)
                caught[op] += 1
    assert caught["diff"] >= 4 and caught["bsub"] >= 3
    # the interleaving the GPU file runs: busy and quiet calls of each form follow each other in set 0
    ops = [op for op, _ in K.SHARED_OPS]
    busy = [any(k is not None and K.DECLARED[k] == "global" for k in ks) for _, ks in K.SHARED_OPS]
    assert ops[1] == "track" and busy[1] and ops[2] == "diff" and not busy[2]
    assert ops[5] == "bsub" and busy[5] and ops[6] == "track" and not busy[6] and ops[7] == "diff" and busy[7]
