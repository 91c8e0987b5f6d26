"""Random call sequences of the host API on the GPU against the oracle (tests/api_sequences.py has the generator, the model,
the driver and THE BUFFER RULE; tests/test_api_sequences_cpu.py shows that the driver catches the bugs it is there for).

Every result, mask and MOG2 model is compared with the CPU oracle, never with another context of the library.  A failing
assertion names the seed, the operation and one command that replays the sequence (tools/fuzz_api.py).
"""
import pytest

import api_sequences as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    import oat_amd
    return oat_amd


@pytest.mark.parametrize("seed", S.SMALL_SEEDS)
def test_sequence_small(A, seed):
    """One context, 40-70 operations: the four launch orders, registered frames, staging, repairs, single-stage calls and
    settings in whatever interleaving the seed draws; buffers overwritten as soon as include/oatgpu.h allows."""
    r = S.run_scenario(S.scenario(seed), A.HotPath)
    assert r.model.collected == r.model.enqueued >= 12


@pytest.mark.parametrize("seed", S.PAIR_SEEDS)
def test_two_contexts_interleaved(A, seed):
    """Two contexts of different geometry and ring depth on ONE thread, their operations merged at random: they share the
    process's A, B and copy streams, and each must still match its own oracle."""
    for st in S.run_interleaved(seed, A.HotPath):
        assert st["collected"] >= 12


@pytest.mark.parametrize("seed", S.THREAD_SEEDS)
def test_two_contexts_on_two_threads(A, seed):
    """One context per host thread (the header's rule), both started behind a barrier; ctypes releases the GIL inside the
    library.  A thread still running after 60 s fails the test."""
    for st in S.run_on_two_threads(seed, A.HotPath, cap=60.0):
        assert st["collected"] >= 12


@pytest.mark.parametrize("case", S.LARGE_CASES)
def test_sequence_large(A, case):
    """Device frames at 4 MP a step and more, where the shipped early order runs UN-FORCED (oatgpu_set_early_blob stays at
    -1): 2 x 1080x1920, 1 x 2000x2048, 2 x 1080x1920 with two frames a launch and a ring of 3.  One busy set in the middle:
    the parked blob workgroup declines it, the global kernels repair it, and later sets go the early way again."""
    scn = S.scenario(case, "large")
    r = S.run_scenario(scn, A.HotPath)
    assert r.stats["busy_sets"] == 1, "the busy set is not over the LDS kernel's capacity"
    assert r.early_steps >= 1, "no step of the sequence was dispatched early (oatgpu_last_step_shape)"
    assert r.busy_then_collected, "no result was collected behind the busy set"
    assert r.model.collected == r.model.enqueued == 14


def test_device_and_host_frame_in_one_step_after_a_decline(A):
    """What seed 22 found, by hand: after a declined frame the steps take the plain order; a small two-frame step then puts
    both back halves on ONE B stream -- also when one frame is a registered host frame and the other a device frame, whose
    B streams are counted differently (slot % 2 and slot % 3).  Host then device under the default fusion, device then host
    under oatgpu_set_fusion(2), with the step's first frame in every ring slot."""
    det = dict(h_lo=100, h_hi=125, s_lo=150, s_hi=256, v_lo=100, v_hi=256, erode=0, dilate=2, min_area=4.0, max_area=1e9)
    cfg = dict(rows=240, cols=320, n=1, channels=3, ring=4, restore=1, det=det, roi=None, kalman=None, lr=0.01, nthreads=1)
    ops = [("track_dev", dict(frame=k, busy=False)) for k in range(4)] + [("track_dev", dict(frame=4, busy=True))]
    k = 5
    for first, second in (("enqueue", "enqueue_dev"), ("enqueue_dev", "enqueue")):
        if first == "enqueue_dev":
            ops.append(("set_fusion", dict(frames=2)))
        for rep in range(7):
            if rep in (3, 5):                                   # shift the parity of the slots the steps start in
                ops.append(("track_dev", dict(frame=k, busy=False)))
                k += 1
            for kind in (first, second):
                ops.append((kind, dict(frame=k, busy=False, mem="host", reuse=False)))
                k += 1
            ops += [("collect", {}), ("collect", {})]
    r = S.run_scenario(dict(seed=22, size="small", cfg=cfg, ops=ops), A.HotPath)
    assert r.stats["busy_sets"] == 1, "frame 4 is not over the LDS kernel's capacity"       # (counted by the model, on the CPU)
    assert r.model.collected == r.model.enqueued == k


def test_read_mask_after_a_repaired_frame(A):
    """What tools/fuzz_api.py --seed 1459 found, by hand: a busy frame in the middle of oatgpu_track_sequence_dev is repaired
    when it is collected, AFTER the frames behind it were launched; the morph and final taps of oatgpu_read_mask must still be
    those of the frame processed last, as the threshold tap is -- also when the busy frame is that last one."""
    det = dict(h_lo=180, h_hi=256, erode=0, dilate=3, min_area=20.0, max_area=1e5)
    cfg = dict(rows=240, cols=320, n=2, channels=1, ring=5, restore=0, det=det, roi=None, kalman=None, lr=0.0, nthreads=1)
    taps = [("read_mask", dict(stream=s, which=w)) for s in range(2) for w in range(3)]
    ops = [("track_sequence_dev", dict(frames=[0, 1, 2, 3], busy=[False, False, True, False]))] + taps
    ops += [("track_sequence_dev", dict(frames=list(range(4, 24)), busy=[False] * 20))] + taps          # 16 calm ones: speculation is back
    ops += [("track_sequence_dev", dict(frames=[24, 25, 26], busy=[False, False, True]))] + taps
    ops += [("enqueue_dev", dict(frame=27 + k, busy=k == 1, reuse=False)) for k in range(3)] + [("collect", {})] * 3 + taps
    r = S.run_scenario(dict(seed=1459, size="small", cfg=cfg, ops=ops), A.HotPath)
    assert r.stats["busy_sets"] == 3, "the busy frames are not over the LDS kernel's capacity"       # (counted by the model, on the CPU)
    assert r.model.collected == r.model.enqueued == 30


@pytest.mark.parametrize("seed", [1459, 1567])
def test_sequences_the_fuzz_run_found(A, seed):
    """Seeds of tools/fuzz_api.py that failed on their first run and stay: 1459 -- read_mask behind a repaired frame (by hand
    above); 1567 -- the per-pixel kernel at learning rate 0 after 0.2: a mode behind a pruned slot fits again and bubbles in
    front of it, no weight VALUE changes, and the exchanged weights were not stored (kernels_mog.hip, the store-back)."""
    r = S.run_scenario(S.scenario(seed), A.HotPath)
    assert r.model.collected == r.model.enqueued >= 12
