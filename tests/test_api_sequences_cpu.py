"""The sequence driver of tests/api_sequences.py without a GPU: a GPU visit must not be the first time the generator, the
model and the driver execute, and the GPU tests must be able to FAIL for the bugs they are there for.

  * FakeHotPath -- HotPath's methods on the oracle alone, following include/oatgpu.h and reading the caller's buffers as
    late as the header allows -- passes every committed small seed, the interleaved pairs and the two-thread pairs;
  * each of its five mutants fails at least one committed seed;
  * the committed seeds reach the interleavings the tests exist for (counted, not hoped for).
"""
import collections

import pytest

import api_sequences as S


@pytest.fixture(scope="module")
def runs():
    """Every committed small seed through the driver on the fake, once: seed -> Runner."""
    return {seed: S.run_scenario(S.scenario(seed), S.FakeHotPath) for seed in S.SMALL_SEEDS}


def test_generator_is_deterministic():
    for seed in S.SMALL_SEEDS[:6]:
        a, b = S.scenario(seed), S.scenario(seed)
        assert a["cfg"] == b["cfg"] and a["ops"] == b["ops"]
    for case in S.LARGE_CASES:
        assert S.scenario(case, "large") == S.scenario(case, "large")
    a, b = S.pair_scenarios(S.PAIR_SEEDS[0]), S.pair_scenarios(S.PAIR_SEEDS[0])
    assert a[2] == b[2] and a[0]["ops"] == b[0]["ops"] and a[1]["ops"] == b[1]["ops"]
    assert S.scenario(1)["ops"] != S.scenario(2)["ops"]


def test_seed_counts_and_sequence_lengths():
    assert (len(S.SMALL_SEEDS), len(S.PAIR_SEEDS), len(S.THREAD_SEEDS), len(S.LARGE_CASES)) == (24, 6, 4, 3)
    for seed in S.SMALL_SEEDS:
        assert 40 <= len(S.scenario(seed)["ops"]) <= 70, seed
    for seed in S.PAIR_SEEDS + S.THREAD_SEEDS:
        a, b, order = S.pair_scenarios(seed)
        ca, cb = a["cfg"], b["cfg"]
        assert (ca["rows"], ca["cols"]) != (cb["rows"], cb["cols"]) and ca["ring"] != cb["ring"], seed
        assert sorted(order) == [0] * len(a["ops"]) + [1] * len(b["ops"])


def test_small_scenarios_draw_what_the_issue_lists():
    cfgs = [S.scenario(seed)["cfg"] for seed in S.SMALL_SEEDS]
    geoms = {(c["rows"], c["cols"]) for c in cfgs}
    assert {(240, 320), (150, 203), (33, 70)} <= geoms
    assert {c["n"] for c in cfgs} == {1, 2, 3} and {c["channels"] for c in cfgs} == {1, 3}
    assert {c["ring"] for c in cfgs} == {1, 2, 3, 4, 5} and {c["restore"] for c in cfgs} == {0, 1}
    assert sum(c["ring"] % 2 for c in cfgs) * 2 >= len(cfgs)                  # odd depths well represented
    assert any(c["roi"] for c in cfgs) and any(c["kalman"] for c in cfgs)
    dets = [c["det"] for c in cfgs] + [a["det"] for seed in S.SMALL_SEEDS for k, a in S.scenario(seed)["ops"] if k == "set_detector"]
    assert 0 in {d["erode"] for d in dets} and 0 in {d["dilate"] for d in dets}
    assert any(d["erode"] and d["erode"] % 2 == 0 for d in dets) and any(d["dilate"] and d["dilate"] % 2 == 0 for d in dets)
    # ... and windows that keep the blob as well as one that leaves it out: a window applied to the wrong frame shows
    assert sum(d["h_lo"] == 0 if "s_lo" in d else d["h_hi"] < 250 for d in dets) >= 5
    assert sum(d["h_lo"] > 0 if "s_lo" in d else d["h_hi"] == 256 for d in dets) >= 5
    rates = {a["lr"] for seed in S.SMALL_SEEDS for k, a in S.scenario(seed)["ops"] if k == "set_lr"}
    assert rates == {0.0, 0.01, 0.2, -1.0}


def test_fake_context_passes_every_small_seed(runs):
    for seed, r in runs.items():
        assert r.model.collected == r.model.enqueued and r.i == len(r.ops), seed


@pytest.mark.parametrize("seed", S.PAIR_SEEDS)
def test_fake_contexts_interleaved(seed):
    for st in S.run_interleaved(seed, S.FakeHotPath):
        assert st["collected"] >= 12


def test_fake_contexts_on_two_threads():
    for st in S.run_on_two_threads(S.THREAD_SEEDS[0], S.FakeHotPath):
        assert st["collected"] >= 12


def test_a_failure_names_seed_operation_and_replay_line():
    scn = S.scenario(3)
    with pytest.raises((AssertionError, RuntimeError)) as e:
        for seed in S.SMALL_SEEDS:
            scn = S.scenario(seed)
            S.run_scenario(scn, S.FakeHotPath, mutant="owes_result_after_stage_abort")
    msg = str(e.value)
    assert f"seed {scn['seed']} " in msg and ("operation" in msg or "at the end" in msg)
    assert f"replay: python tools/fuzz_api.py --seed {scn['seed']} --sequences 1 --only 0 --size small" in msg


@pytest.mark.parametrize("mutant", S.MUTANTS)
def test_driver_catches_mutant(mutant):
    """Each deliberate bug of the fake fails at least one committed seed -- with an assertion of the driver, not a crash."""
    caught = []
    for seed in S.SMALL_SEEDS:
        try:
            S.run_scenario(S.scenario(seed), S.FakeHotPath, mutant=mutant)
        except AssertionError:
            caught.append(seed)
            break
    assert caught, f"no committed seed notices the mutant '{mutant}'"


def test_coverage_of_the_committed_seeds(runs):
    total = collections.Counter()
    for r in runs.values():
        total.update(r.stats)
    for kind in S.KINDS + S.REFUSALS:
        assert total[kind] >= 10, (kind, total[kind])
    for tag in ("single_stage_busy_outstanding", "detector_with_registered", "fusion_switch_outstanding",
                "early_or_k1_switch_outstanding", "stage_abort_after_stage", "overwrite_after_consumed_uncollected",
                "fusion2_odd_ring_full"):
        assert total[tag] >= 3, (tag, total[tag])
    assert sum(r.cfg["ring"] == 1 for r in runs.values()) >= 3
    for seed, r in runs.items():
        assert r.stats["refusals"] <= 0.15 * r.stats["ops"], (seed, r.stats["refusals"], r.stats["ops"])
        assert r.stats["collected"] >= 12, (seed, r.stats["collected"])
    assert sum(r.stats["busy_sets"] > 0 for r in runs.values()) * 2 >= len(runs)


def test_busy_frames_are_over_the_lds_kernels_run_capacity():
    """Counted on the CPU in the oracle's morph mask, as tests/blob_load.py counts; a calm frame is far below."""
    import numpy as np
    import oracle_lib as O
    from blob_load import LDS_RUNS, blob_load
    scn = S.scenario(1)
    c = dict(scn["cfg"], n=1)
    assert c["channels"] == 3
    c["det"] = dict(zip(("h_lo", "h_hi", "s_lo", "s_hi", "v_lo", "v_hi"), S.BGR_WINDOWS[0]), erode=0, dilate=2, min_area=4.0, max_area=1e9)
    fr = S.Frames(dict(scn, cfg=c))
    mog = O.Mog2(c["rows"], c["cols"], c["channels"])
    p = O.hsv_params(**c["det"])
    for k in range(4):
        O.chain_step(mog, fr.get(k)[0], 0.01, p)
    calm = O.chain_step(mog, fr.get(4)[0], 0.01, p)[1]
    busy = O.chain_step(mog, fr.get(5, True)[0], 0.01, p)[1]
    assert blob_load(busy)["R"] > LDS_RUNS and blob_load(busy)["path"] == "global" and S.runs_over_capacity(busy)
    assert blob_load(calm)["path"] == "lds" and not S.runs_over_capacity(calm)
    assert np.count_nonzero(calm) > 0


def test_large_scenarios_are_what_their_test_says():
    shapes = []
    for case in S.LARGE_CASES:
        scn = S.scenario(case, "large")
        c, kinds = scn["cfg"], [k for k, _ in scn["ops"]]
        shapes.append((c["n"], c["rows"], c["cols"], c["ring"]))
        assert c["n"] * c["rows"] * c["cols"] >= 4_000_000 and c["nthreads"] == 8
        assert "set_early_blob" not in kinds                                 # the early order runs un-forced
        assert set(kinds) <= {"enqueue_dev", "collect", "ready", "ready_poll", "input_consumed", "detect", "mog_state",
                              "set_fusion", "set_k1_workgroup", "set_stage_copy"}
        enq = [a for k, a in scn["ops"] if k == "enqueue_dev"]
        assert len(enq) == 14 and [a["busy"] for a in enq].count(True) == 1 and enq[7]["busy"]
        assert kinds[-c["n"]:] == ["mog_state"] * c["n"]
    assert shapes == [(2, 1080, 1920, 4), (1, 2000, 2048, 4), (2, 1080, 1920, 3)]
    assert S.scenario(2, "large")["ops"][0] == ("set_fusion", dict(frames=2))
