"""Multi-GPU readiness on ONE GPU: the N > 1 control flow of bench.py and an RCCL
import/initialisation check, so that a problem shows up before the driver's 8-GPU SCALE run.  What these
cannot show is scaling: that stays "unmeasured on hardware" until a SCALE record exists."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _launch(cmd_of_port, env, timeout):
    """ONE launch (no second attempt: VERDICT r04 weak-12 -- the product tolerates a transient device-open failure itself,
    with a bounded, counted retry: oatgpu_create / bench.py open_device_with_retry).  A launch that dies leaves its stderr
    under gpurun_out/ for the driver to pull."""
    r = subprocess.run(cmd_of_port(_free_port()), cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        try:
            os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
            with open(os.path.join(ROOT, "gpurun_out", "multirank_failure_%d.txt" % os.getpid()), "a") as f:
                f.write("rc %d\n--- stderr\n%s\n--- stdout\n%s\n" % (r.returncode, r.stderr[-20000:], r.stdout[-4000:]))
        except OSError:
            pass
    return r


def _detail():
    with open(os.path.join(ROOT, "bench_detail.json")) as f:
        return json.load(f)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_bench_two_ranks_over_gloo_share_one_gpu():
    """`torch.distributed.run --nproc-per-node 2 bench.py --gpus 2 --backend gloo --full`: both ranks run the hot path on
    the one GPU, barriers and max-over-ranks timing work, rank 0 alone prints one line whose value counts BOTH
    ranks' streams, and every position of both ranks was found."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = lambda port: [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo",
                        "--workload", "vga1", "--steps", "60", "--warmup", "10", "--check-steps", "8", "--scatter-steps", "24", "--full"]
    r = _launch(cmd, env, 600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and len(lines[0]) <= 4096, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["steps"] == 60 and j["scaling"] == "weak"
    d = _detail()                                       # everything else the run measured
    timed = d["timing"]["steps_timed"]                 # exactly --steps timed steps, one block, max over the ranks
    assert timed == 60 and d["timing"]["blocks"] == 1 and j["timed_region_ms"] == pytest.approx(60 * j["ms_per_step"], rel=1e-3)
    assert j["positions_expected"] == 2 * timed and j["positions_found"] >= 0.95 * 2 * timed   # (the oracle gate checks WHICH)
    assert abs(j["value"] - 2 * 60 / (j["ms_per_step"] * 60 / 1e3)) < 1e-5 * j["value"]
    assert j["parity"] == "ok"
    assert j["cpu_baseline"] is None and j["roofline"]["frac"] is None      # N = 1-only legs are skipped, and say so
    assert [q[:5] for q in j["partition"]["ranks"]] == [[0, 0, 0, 1, "ok"], [1, 0, 1, 2, "ok"]]
    # the scatter leg: all frames from rank 0 through FrameScatterPipe, gated against the oracle on what ARRIVED
    sc = j["scatter_ingest"]
    assert sc["parity"] == "ok" and sc["fps"] > 0 and sc["bytes_per_peer"] == 480 * 640 * 3 and sc["backend"] == "gloo"
    assert [q["parity"] for q in d["scatter_ingest"]["per_rank"]] == ["ok", "ok"]
    assert j["rccl"] == {"ranks": 2, "backend": "gloo", "version": None}


def test_bench_gpus_2_as_a_plain_process_starts_two_ranks():
    """`python3 bench.py --gpus 2 ...` the way the driver may run it -- NO launcher in front: the script starts its two ranks
    itself (torch.distributed.run) and the one line says n_gpus 2 (VERDICT r04 missing-2: it used to bench ONE GPU and
    print n_gpus 1)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    cmd = lambda port: [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--workload", "vga1",
                        "--steps", "40", "--warmup", "10", "--check-steps", "4", "--scatter-steps", "16", "--full"]
    r = _launch(cmd, env, 600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and len(lines[0]) <= 4096, r.stdout[-2000:]
    j = json.loads(lines[-1])
    assert j["n_gpus"] == 2 and j["steps"] == 40 and j["parity"] == "ok" and j["config"]["workload"] == "vga1"
    assert len(j["partition"]["ranks"]) == 2 and j["scatter_ingest"]["parity"] == "ok"
    assert j["fps_per_gpu"] * 2 == pytest.approx(j["value"], rel=1e-4)


def test_bench_gpus_2_without_full_times_both_ranks_and_runs_nothing_else():
    """`python3 bench.py --gpus 2` without --full: both ranks time their shard, rank 0 prints one line whose value counts both
    ranks' streams, and no gate, second workload or scatter leg runs."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    cmd = lambda port: [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--workload", "vga1",
                        "--steps", "40", "--warmup", "10"]
    r = _launch(cmd, env, 600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and len(lines[0]) <= 4096, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["steps"] == 40 and j["full_run"] is False and j["parity"] == "skipped"
    assert abs(j["value"] - 2 * 40 / (j["ms_per_step"] * 40 / 1e3)) < 1e-5 * j["value"]
    assert j["positions_expected"] == 80 and j["positions_found"] >= 0.95 * 80
    assert j["scatter_ingest"] is None and j["extra_workloads"] is None and j["cpu_baseline"] is None
    assert [q[:5] for q in j["partition"]["ranks"]] == [[0, 0, 0, 1, "skipped"], [1, 0, 1, 2, "skipped"]]


# Ranks of the multi-rank runs that share the one GPU: with the test process (it opens the device first) and the launcher
# in front of the ranks, no more than six processes have the device open at once.
RANKS = 3


@pytest.mark.parametrize("workload,per_rank", [("1080p8", 8), ("4k1", 1)])
def test_bench_three_ranks_on_one_gpu_run_configs_3_and_4(workload, per_rank):
    """BASELINE configs[3] (8 x 1080p a rank) and configs[4] (one 4K stream a rank) in their multi-rank form on the one GPU
    there is: `torch.distributed.run --nproc-per-node 3 bench.py --gpus 3 --backend gloo --full`.  Three
    processes, three contexts on device 0.  Asserted: SURVEY 8e's partition (rank r owns global streams r*per .. r*per +
    per - 1), BOTH parity gates green on EVERY rank for every stream of its shard, one JSON line from rank 0 whose value
    counts all ranks' streams, the N = 1-only legs absent.  What this cannot show is scaling over xGMI: that stays
    unmeasured until a SCALE record exists."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    K = 20
    N = RANKS
    cmd = lambda port: [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(N), "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", str(N), "--backend", "gloo",
                        "--workload", workload, "--steps", str(K), "--warmup", "5", "--age", "40", "--pool", "8", "--check-steps", "4",
                        "--no-spin-up", "--scatter-steps", "12", "--no-extra", "--full"]
    r = _launch(cmd, env, 900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and len(lines[0]) <= 4096, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["n_gpus"] == N and j["steps"] == K and j["scaling"] == "weak" and j["config"]["workload"] == workload
    assert j["config"]["streams_per_gpu"] == per_rank
    part = _detail()["partition"]
    assert part["streams_total"] == N * per_rank and len(part["per_rank"]) == N
    for rk, rec in enumerate(part["per_rank"]):
        assert rec["rank"] == rk and rec["streams"] == [rk * per_rank, (rk + 1) * per_rank], rec
        assert rec["parity"] == "ok", rec                      # every rank gated its own shard
        assert rec["positions_found"] > 0, rec
    assert [q[:5] for q in j["partition"]["ranks"]] == [[rk, 0, rk * per_rank, (rk + 1) * per_rank, "ok"] for rk in range(N)]
    assert j["parity"] == "ok", j["parity"]
    timed = _detail()["timing"]["steps_timed"]
    assert timed == K and j["positions_expected"] == N * per_rank * timed
    assert j["positions_found"] >= 0.7 * j["positions_expected"]       # (young models, 40 frames: the gates check WHICH)
    assert abs(j["value"] - N * per_rank * K / (j["ms_per_step"] * K / 1e3)) < 1e-5 * j["value"]
    assert j["cpu_baseline"] is None and j["roofline"]["frac"] is None and j.get("extra_workloads") is None
    assert j["scatter_ingest"]["parity"] == "ok" and j["scatter_ingest"]["bytes_per_peer"] == per_rank * (1080 * 1920 if per_rank == 8 else 2160 * 3840) * 3


def test_the_drivers_multi_gpu_command_at_three_ranks_yields_the_whole_record_on_one_gpu():
    """`python3 bench.py --gpus 3 --steps 20 --warmup 5 --full` -- the driver's argv for its one-shot SCALE run (there with
    --gpus 8) with everything beyond the headline, plus `--backend gloo` so that the ranks can share the one GPU there is
    (VERDICT r05 next-1).  ONE invocation, no launcher in front, default ageing / pool / gates: one line <= 4 KB with n_gpus 3 that carries BOTH north-star sizes at N GPUs -- `value` on
    configs[4]'s shard (one 4K stream a rank) and `extra_workloads.1080p8` on configs[3]'s (8 x 1080p a rank), both parity
    gates green on every rank for both --, the benched per-pixel launch as a fraction of the HBM peak from the slowest
    rank's HIP events (no profiler child at N > 1), the per-rank kernel times, and the stream->rank scatter for both sizes."""
    import time
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    N = RANKS
    cmd = lambda port: [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(N), "--steps", "20", "--warmup", "5", "--backend", "gloo",
                        "--full"]
    t0 = time.perf_counter()
    r = _launch(cmd, env, 900)
    wall = time.perf_counter() - t0
    try:
        os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
        with open(os.path.join(ROOT, "gpurun_out", "drivers_multi_gpu_command_stderr.txt"), "w") as f:
            f.write(r.stderr[-60000:])
    except OSError:
        pass
    assert r.returncode == 0, r.stderr[-3000:]
    assert wall < 900
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and len(lines[0]) <= 4096, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["n_gpus"] == N and j["steps"] == 20 and j["warmup"] == 5 and j["config"]["workload"] == "4k1"
    assert j["parity"] == "ok" and [q[4] for q in j["partition"]["ranks"]] == ["ok"] * N
    assert set(j["extra_workloads"]) == {"1080p8"} and j["extra_workloads"]["1080p8"] > 0 and j["extra_parity"] == "ok"
    d = _detail()
    ex = d["extra_workloads"]["1080p8"]
    assert ex["streams_total"] == 8 * N and [q["parity"] for q in ex["per_rank"]] == ["ok"] * N and ex["timed_region_ms"] >= 50.0
    assert ex["value"] == pytest.approx(8 * N * 20 / (ex["ms_per_step"] * 20 / 1e3), rel=1e-6)
    rf = j["roofline"]
    assert rf["frac"] is None and rf["frac_benched"] is not None and 0.0 < rf["frac_benched"] < 1.0 and rf["frac_benched_source"] == "audit"
    assert rf["benched_launch_ms"] == pytest.approx(rf["k1_ms_ranks"][1], rel=1e-3) and rf["k1_ms_ranks"][0] <= rf["k1_ms_ranks"][1]
    assert all(q[5] and q[5] > 0 for q in j["partition"]["ranks"])                 # every rank's k_mog_fused ms
    sc = j["scatter_ingest"]
    assert sc["parity"] == "ok" and sc["bytes_per_peer"] == 2160 * 3840 * 3
    assert sc["also"]["workload"] == "1080p8" and sc["also"]["parity"] == "ok" and sc["also"]["bytes_per_peer"] == 8 * 1080 * 1920 * 3
    assert j["rccl"] == {"ranks": N, "backend": "gloo", "version": None}
    assert j["value_mean"] > 0 and j["positions_with_target"] <= j["positions_expected"]
    with open(os.path.join(ROOT, "gpurun_out", "drivers_multi_gpu_command_wall_s.txt"), "w") as f:
        f.write("%.1f s wall, line %d bytes\n%s\n" % (wall, len(lines[0]), lines[0]))


def test_rccl_single_rank_init_allreduce_teardown():
    """backend "nccl" IS RCCL on ROCm: a world of one must initialise, reduce on the GPU and tear down."""
    code = r"""
import os, torch, torch.distributed as dist
os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
dist.init_process_group(backend="nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
t = torch.arange(8, dtype=torch.float64, device="cuda")
dist.all_reduce(t, op=dist.ReduceOp.MAX)
dist.barrier()
assert t.tolist() == list(range(8))
import oat_amd.dist as od
blk = od.scatter_frames(torch.arange(2 * 24, dtype=torch.uint8).view(2, 2, 4, 3), 2, (2, 4, 3), torch.device("cuda", 0))
assert blk.shape == (2, 2, 4, 3) and int(blk.sum()) == sum(range(48))
pipe = od.FrameScatterPipe(2, (2, 4, 3), torch.device("cuda", 0))
pipe.post(0, torch.full((2, 2, 4, 3), 7, dtype=torch.uint8))
assert int(pipe.take(0).sum()) == 7 * 48
# ... with the hot path as consumer: take() orders the consumer's HIP stream behind the transfer (no host sync),
# post() waits for the kernel that read the slot before it reuses it (oatgpu_track_input_consumed)
import numpy as np, oat_amd
rows, cols = 64, 128
hp = oat_amd.HotPath(rows, cols, n_streams=2, ring_depth=4, adaptation_coeff=0.0, erode=0, dilate=0, v_thresh=(200, 256), area=(0.5, 1e9))
pipe = od.FrameScatterPipe(2, (rows, cols, 3), torch.device("cuda", 0), depth=2, consumer=hp)
def frames(k):
    f = np.zeros((2, rows, cols, 3), np.uint8)
    if k:
        f[0, 10:12 + k, 10:14] = 255
        f[1, 20:24, 30:32 + k] = 255
    return torch.from_numpy(f)
got = []
pipe.post(0, frames(0))
for t in range(7):
    if t + 1 < 7: pipe.post(t + 1, frames(t + 1))
    local = pipe.take(t)
    hp.enqueue_dev(local.data_ptr())
    if hp.outstanding() == 3: got.append(hp.collect())
while hp.outstanding(): got.append(hp.collect())
assert [r[0].area for r in got[1:]] == [(k + 1) * 3.0 for k in range(1, 7)], [r[0].area for r in got]
assert [r[1].area for r in got[1:]] == [3.0 * (k + 1) for k in range(1, 7)]
hp.close()
dist.destroy_process_group()
print("rccl ok")
"""
    env = dict(os.environ, MASTER_PORT=str(_free_port()), HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "rccl ok" in r.stdout, r.stderr[-3000:]
