"""Random, legal call sequences of the tracker's host API, an oracle-backed model of what every call must return, and the
driver that runs one against the other (TEST INFRASTRUCTURE, as tests/mog_matrix.py and tests/blob_load.py are).

What is under test is the machinery BETWEEN the kernels in oat_amd/csrc/api_track.hip and api_context.hip: launch orders, scratch sets by
frame parity, frames that are only registered under oatgpu_set_fusion(2), speculation and repair, staging camera by
camera, the quiesce() in front of every synchronous call, HIP streams shared by the contexts of a process.

  scenario(seed, size)   a context configuration and a list of operations, drawn by a random walk over an abstract state of
                         the context (ring, staging, fusion, ...), so that the generator knows whether each operation is
                         legal; refusals are drawn on purpose and must leave the context as it was.
  Model                  one oracle MOG2 (and Kalman filter) per stream, the detector in force, a FIFO of expected results.
  Runner                 runs the operations on a context -- oat_amd.HotPath, or FakeHotPath below -- and checks every
                         return value, the masks and the whole MOG2 model against the Model.  Never library against library.
  FakeHotPath            HotPath's methods on the oracle alone, reading the caller's buffers as LATE as include/oatgpu.h
                         allows; its mutants are the bugs the driver is there to catch (tests/test_api_sequences_cpu.py).

THE BUFFER RULE.  The Runner owns every frame buffer it hands over and overwrites it with random bytes as soon as the header
allows: a host frame after oatgpu_track_input_consumed returned, after oatgpu_track_input_consumed_stream for its stream, or
after its set was collected; a staged frame after input_consumed_stream(s) or oatgpu_track_stage_abort; a device frame after
input_consumed returned or its set was collected.  Expected results come from the Model's own copy of the frame.  While
device frames are launched inside oatgpu_track_enqueue_dev (default fusion, or 1) the Runner also reuses ONE device buffer,
refilled in stream order on the context's HIP stream.

Left out on purpose: marker sets, undistort, homography (but for its refusal), checkpoints and deferred mode have sequence
tests of their own; more than one device has none.
"""
import collections
import threading
import time

import numpy as np

import oracle_lib as O
from blob_load import frame_zeroed, over_run_capacity
from oat_amd.components import Position2D
from oat_amd.ffi import OatGpuError
from parity_asserts import _same_detection, _same_state

SMALL_SEEDS = tuple(range(24))
PAIR_SEEDS = tuple(range(100, 106))
THREAD_SEEDS = tuple(range(200, 204))
LARGE_CASES = (0, 1, 2)

GEOMETRIES = [(240, 320), (240, 320), (240, 320), (150, 203), (150, 203), (150, 203), (33, 70), (96, 200)]
RATES = [0.0, 0.01, 0.2, -1.0]
# the blob is BGR (255, 64, 0) = HSV (112, 255, 255), GREY 250: the LAST window of each list leaves it out, so that a window
# applied to the wrong frame changes the result (the others differ in what they keep of the noise alone)
BGR_WINDOWS = [(100, 125, 150, 256, 100, 256), (95, 130, 100, 256, 80, 256), (105, 120, 150, 256, 100, 256), (0, 100, 0, 256, 100, 256)]
GREY_WINDOWS = [(200, 256), (180, 256), (220, 256), (100, 240)]
KALMAN = dict(dt=0.01, timeout=0.08, sigma_accel=30.0, sigma_noise=1.5)
IDENTITY9 = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
REFUSALS = ("r_enqueue_full", "r_stage_full", "r_collect_empty", "r_sync_outstanding", "r_set_kalman", "r_set_homography",
            "r_enqueue_staging", "r_staged_short", "r_stage_twice", "r_stream_range")
KINDS = ("enqueue", "enqueue_dev", "stage", "enqueue_staged", "stage_abort", "collect", "ready", "ready_poll", "outstanding",
         "input_consumed", "input_consumed_stream", "set_lr", "track", "track_dev", "track_sequence_dev", "detect",
         "mog_state", "read_mask", "set_detector", "set_fusion", "set_early_blob", "set_k1_workgroup", "set_stage_copy",
         "set_kalman")
SINGLE_STAGE = ("detect", "mog_state", "read_mask")


# ---------------------------------------------------------------------------------------------------- scenarios ---

def _draw_detector(rng, channels, busy_friendly):
    d = {}
    if channels == 3:
        w = BGR_WINDOWS[min(int(rng.integers(3 if busy_friendly else 6)), 3)]      # (not friendly: half leave the blob out)
        d.update(h_lo=w[0], h_hi=w[1], s_lo=w[2], s_hi=w[3], v_lo=w[4], v_hi=w[5])
    else:
        w = GREY_WINDOWS[min(int(rng.integers(3 if busy_friendly else 6)), 3)]
        d.update(h_lo=w[0], h_hi=w[1])
    if busy_friendly:                        # specks survive: a busy frame stays over the LDS kernel's run capacity
        d.update(erode=0, dilate=int(rng.choice([0, 2, 3])))
    else:
        d.update(erode=int(rng.choice([0, 0, 2, 3])), dilate=int(rng.choice([0, 2, 3, 4, 7])))
    d.update(min_area=float(rng.choice([0.0, 4.0, 20.0])), max_area=float(rng.choice([1e9, 1e5, 400.0])))
    return d


def _busy_friendly(det, rows):
    sees_blob = det["h_lo"] > 0 if "s_lo" in det else det["h_hi"] == 256
    return sees_blob and det["erode"] == 0 and det["dilate"] <= 3 and rows >= 150


class _Walk:
    """The generator's abstract state of the context: enough to know what is legal, and to tag the interleavings the
    coverage conditions of tests/test_api_sequences_cpu.py count."""

    def __init__(self, cfg):
        self.n, self.ring = cfg["n"], cfg["ring"]
        self.out = []                 # outstanding sets: dict(busy=, dev=)
        self.staged = []              # streams staged of the open set
        self.fusion = 0               # 0: the default (host frames pair, device frames do not), 1, 2
        self.pend = False             # the newest outstanding set is only registered (include/oatgpu.h, oatgpu_set_fusion)
        self.early, self.k1, self.stage_copy = -1, 0, 0
        self.kalman = cfg["kalman"] is not None
        self.det = dict(cfg["det"])
        self.lr = cfg["lr"]
        self.k = 0                    # frame sets drawn so far
        self.collected = 0
        self.ics_next = None          # next stream of input_consumed_stream for the latest host set
        self.taps = False             # read_mask is defined: the last thing processed was a frame set
        self.since_busy = 99
        self.stage_frame = None       # (frame index, busy) of the set being staged
        self.dev_unconsumed = False   # a device frame was handed over since the last input_consumed: that call launches a registered frame

    def registered(self, host):
        pair = self.fusion == 2 or (self.fusion == 0 and host)
        if self.pend:
            self.pend = False
        elif pair and self.ring >= 2:
            self.pend = True

    def quiesce(self):
        self.pend = False

    def consumed(self):
        """oatgpu_track_input_consumed, also reached through input_consumed_stream: with device frames unconsumed it
        launches the registered frame before it waits."""
        if self.dev_unconsumed:
            self.pend = False
        self.dev_unconsumed = False


def _small_config(rng, avoid=None):
    geoms = [g for g in GEOMETRIES if g != avoid]
    rows, cols = geoms[int(rng.integers(len(geoms)))]
    n = int(rng.choice([1, 2, 2, 3]))
    channels = int(rng.choice([3, 3, 1]))
    ring = int(rng.choice([1, 1, 2, 3, 3, 4, 5, 5]))
    det = _draw_detector(rng, channels, rng.random() < 0.85)
    roi = None
    if rng.random() < 0.3:
        roi = dict(stream=int(rng.integers(n)), y0=rows // 8, y1=rows - rows // 10, x0=cols // 9, x1=cols - cols // 7)
    kalman = dict(KALMAN) if rng.random() < 0.3 else None
    return dict(rows=rows, cols=cols, n=n, channels=channels, ring=ring, restore=int(rng.integers(2)), det=det, roi=roi,
                kalman=kalman, lr=float(rng.choice(RATES)), nthreads=1)


def scenario(seed, size="small", avoid_geometry=None):
    """-> dict(seed, size, cfg, ops); ops = [(kind, args)].  Deterministic in its arguments."""
    if size == "large":
        return _large_scenario(seed)
    rng = np.random.default_rng([0x5E9, int(seed)])
    cfg = _small_config(rng, avoid_geometry)
    w = _Walk(cfg)
    n, ring = w.n, w.ring
    total = int(rng.integers(44, 63))
    ops, used = [], collections.Counter()

    def emit(kind, tags=(), **args):
        if tags:
            args["tags"] = tuple(tags)
        ops.append((kind, args))
        used[kind] += 1

    def new_set(dev):
        busy = bool(w.k > 1 and _busy_friendly(w.det, cfg["rows"]) and w.since_busy > 3 and rng.random() < 0.6)
        w.since_busy = 0 if busy else w.since_busy + 1
        k = w.k
        w.k += 1
        return k, busy

    def enqueued(busy, host):
        w.out.append(dict(busy=busy, dev=not host))
        w.registered(host)
        if not host:
            w.dev_unconsumed = True
        w.ics_next = 0 if host else None
        w.taps = True
        tags = []
        if w.fusion == 2 and ring % 2 == 1 and len(w.out) == ring:
            tags.append("fusion2_odd_ring_full")
        return tags

    while len(ops) < total or (w.collected + len(w.out) < 14 and len(ops) < 70):
        full, staging, out = len(w.out) == ring, bool(w.staged), len(w.out)
        # ---- a deliberate refusal?
        closing = len(ops) >= total        # short of result sets: nothing but frames in and results out from here on
        if not closing and rng.random() < (0.3 if staging else 0.3 if full else 0.08) and sum(used[r] for r in REFUSALS) < 0.13 * total:
            avail = ["r_staged_short" if len(w.staged) < n else None, "r_stream_range"]
            if full and not staging:
                avail += ["r_enqueue_full", "r_stage_full"]
            if out == 0:
                avail.append("r_collect_empty")
            if out > 0:
                avail += ["r_sync_outstanding", "r_set_kalman", "r_set_homography"]
            if staging:
                avail += ["r_enqueue_staging", "r_stage_twice"]
            avail = [a for a in avail if a]
            rare = {"r_enqueue_full": 8, "r_stage_full": 14, "r_collect_empty": 5, "r_enqueue_staging": 5, "r_stage_twice": 5,
                    "r_sync_outstanding": 5, "r_set_kalman": 3, "r_set_homography": 3, "r_staged_short": 3, "r_stream_range": 2}
            p = np.array([rare.get(a, 1) / (1.0 + used[a]) for a in avail])
            kind = avail[int(rng.choice(len(avail), p=p / p.sum()))]
            args = {}
            if kind in ("r_enqueue_full", "r_enqueue_staging"):
                args["form"] = str(rng.choice(["host", "dev"]))
            elif kind == "r_sync_outstanding":
                args["form"] = str(rng.choice(["track", "track_dev", "track_sequence_dev"]))
            elif kind == "r_stage_twice":
                args["stream"] = int(rng.choice(w.staged))
            elif kind == "r_stream_range":
                args["form"] = str(rng.choice(["stage", "input_consumed_stream"]))
                args["stream"] = int(rng.choice([-1, n, n + 3]))
            emit(kind, **args)
            continue
        # ---- a legal operation, by weight
        busy_out = any(s["busy"] for s in w.out)
        cand = {}
        if not full and not staging:
            cand["enqueue"] = 3.0
            cand["enqueue_dev"] = 3.0
            cand["stage"] = 2.6
        if staging:
            if len(w.staged) < n:
                cand["stage"] = 6.0
            else:
                cand["enqueue_staged"] = 9.0
            cand["stage_abort"] = 3.5 if len(w.staged) < n else 1.5
            cand["input_consumed_stream"] = 1.5
        if out:
            cand["collect"] = 1.5 + 3.0 * out / ring + (4.0 if full else 0.0)
            cand["ready_poll"] = 0.8
            cand["input_consumed"] = 1.3
            if not staging and w.ics_next is not None and w.ics_next < n:
                cand["input_consumed_stream"] = 1.5
        cand["ready"] = 0.7
        cand["outstanding"] = 0.6
        cand["set_lr"] = 0.8
        if out == 0 and not staging:
            cand.update(track=2.5, track_dev=2.5, track_sequence_dev=3.5, set_kalman=1.6)
            if w.taps:
                cand["read_mask"] = 3.0
        single = 3.0 if busy_out else 1.0
        cand["detect"] = 1.0 * single
        cand["mog_state"] = 0.6 * single
        cand["set_detector"] = 1.0 * (3.0 if (w.pend and w.fusion == 2) else 1.0)
        cand["set_fusion"] = 0.6 * (2.0 if out else 1.0)
        cand["set_early_blob"] = 0.3 * (2.0 if out else 1.0)
        cand["set_k1_workgroup"] = 0.3 * (2.0 if out else 1.0)
        cand["set_stage_copy"] = 0.45
        if closing:
            cand = {k: v for k, v in cand.items() if k in ("enqueue", "enqueue_dev", "collect", "enqueue_staged", "track") or (k == "stage" and staging)}
        names = sorted(cand)
        p = np.array([cand[k] for k in names])
        kind = names[int(rng.choice(len(names), p=p / p.sum()))]

        if kind == "enqueue":
            k, busy = new_set(False)
            emit(kind, enqueued(busy, True), frame=k, busy=busy, mem="pinned" if rng.random() < 0.35 else "host")
        elif kind == "enqueue_dev":
            k, busy = new_set(True)
            reuse = bool(w.fusion != 2 and rng.random() < 0.5)
            emit(kind, enqueued(busy, False), frame=k, busy=busy, reuse=reuse)
        elif kind == "stage":
            if not w.staged:
                w.stage_frame = new_set(False)
                w.ics_next = None
            s = int(rng.choice([s for s in range(n) if s not in w.staged]))
            w.staged.append(s)
            emit(kind, stream=s, frame=w.stage_frame[0], busy=w.stage_frame[1], mem="pinned" if rng.random() < 0.5 else "host")
        elif kind == "enqueue_staged":
            w.staged = []
            tags = enqueued(w.stage_frame[1], True)
            w.ics_next = None                 # (its frames were waited for stream by stream, or are by input_consumed)
            emit(kind, tags)
        elif kind == "stage_abort":
            w.staged = []
            w.k -= 1                          # the set is given up: its frame index is drawn again
            emit(kind, ("stage_abort_after_stage",))
        elif kind == "collect":
            w.out.pop(0)
            w.collected += 1
            if not w.out:
                w.pend = False
            emit(kind)
        elif kind in ("ready", "ready_poll"):
            if len(w.out) == 1:
                w.pend = False
            emit(kind)
        elif kind == "outstanding":
            emit(kind)
        elif kind == "input_consumed":
            w.consumed()
            w.ics_next = None
            emit(kind)
        elif kind == "input_consumed_stream":
            if staging:
                emit(kind, stream=int(rng.choice(w.staged)))
            else:
                if w.dev_unconsumed or w.ics_next + 1 == n:      # falls through to oatgpu_track_input_consumed
                    w.consumed()
                emit(kind, stream=w.ics_next)
                w.ics_next += 1
        elif kind == "set_lr":
            w.lr = float(rng.choice(RATES))
            emit(kind, lr=w.lr)
        elif kind in ("track", "track_dev"):
            k, busy = new_set(kind == "track_dev")
            w.collected += 1
            w.taps = True
            w.quiesce()
            w.dev_unconsumed = True           # (both go through oatgpu_track_enqueue_dev)
            emit(kind, frame=k, busy=busy)
        elif kind == "track_sequence_dev":
            sets = [new_set(True) for _ in range(int(rng.integers(2, 6)))]
            w.collected += len(sets)
            w.taps = True
            w.quiesce()
            w.dev_unconsumed = False
            emit(kind, frames=[k for k, _ in sets], busy=[b for _, b in sets])
        elif kind == "detect":
            tags = ["single_stage_outstanding"] if out else []
            w.quiesce()
            w.taps = False
            emit(kind, tags, stream=int(rng.integers(n)), probe=int(rng.integers(2)))
        elif kind == "mog_state":
            w.quiesce()
            emit(kind, ["single_stage_outstanding"] if out else [], stream=int(rng.integers(n)))
        elif kind == "read_mask":
            w.quiesce()
            emit(kind, stream=int(rng.integers(n)), which=int(rng.integers(3)))
        elif kind == "set_detector":
            tags = ["detector_with_registered"] if (w.pend and w.fusion == 2) else []
            w.det = _draw_detector(rng, cfg["channels"], rng.random() < 0.75)
            w.quiesce()
            emit(kind, tags, det=dict(w.det))
        elif kind == "set_fusion":
            f = int(rng.choice([1, 2, 2]))
            tags = ["fusion_switch_outstanding"] if (out and f != w.fusion) else []
            w.quiesce()
            w.fusion = f
            emit(kind, tags, frames=f)
        elif kind == "set_early_blob":
            v = int(rng.choice([x for x in (-1, 0, 1) if x != w.early]))
            w.early = v
            emit(kind, ["early_or_k1_switch_outstanding"] if out else [], on=v)
        elif kind == "set_k1_workgroup":
            v = int(rng.choice([x for x in (0, 64, 256) if x != w.k1]))
            w.k1 = v
            emit(kind, ["early_or_k1_switch_outstanding"] if out else [], threads=v)
        elif kind == "set_stage_copy":
            w.stage_copy ^= 1
            emit(kind, mode=w.stage_copy)
        elif kind == "set_kalman":
            w.kalman = not w.kalman if rng.random() < 0.5 else w.kalman
            w.quiesce()
            emit(kind, enable=w.kalman)
    assert 40 <= len(ops) <= 70, len(ops)
    return dict(seed=int(seed), size="small", cfg=cfg, ops=ops)


LARGE_SHAPES = [dict(n=2, rows=1080, cols=1920, ring=4, fusion=None), dict(n=1, rows=2000, cols=2048, ring=4, fusion=None),
                dict(n=2, rows=1080, cols=1920, ring=3, fusion=2)]


def _large_scenario(case):
    """Device frames at sizes where the shipped early order runs un-forced (oatgpu_set_early_blob stays at -1): about 14
    frame sets, one busy set in the middle; enqueue_dev, collect, ready, input_consumed, detect, the switches, mog_state at
    the end."""
    sh = LARGE_SHAPES[case]
    rng = np.random.default_rng([0x1A9, int(case)])
    det = dict(h_lo=100, h_hi=125, s_lo=150, s_hi=256, v_lo=100, v_hi=256, erode=0, dilate=2, min_area=4.0, max_area=1e9)
    cfg = dict(rows=sh["rows"], cols=sh["cols"], n=sh["n"], channels=3, ring=sh["ring"], restore=1, det=det, roi=None,
               kalman=None, lr=0.01, nthreads=8)
    ops, out, fusion, k1, sc = [], 0, sh["fusion"] or 0, 0, 0
    if sh["fusion"]:
        ops.append(("set_fusion", dict(frames=sh["fusion"])))
    nsets, busy_at = 14, 7
    for k in range(nsets):
        while out == cfg["ring"] or (out and rng.random() < 0.25):
            if rng.random() < 0.3:
                ops.append(("ready_poll", {}))
            ops.append(("collect", {}))
            out -= 1
        ops.append(("enqueue_dev", dict(frame=k, busy=k == busy_at, reuse=False)))
        out += 1
        r = rng.random()
        if r < 0.15:
            ops.append(("input_consumed", {}))
        elif r < 0.3:
            ops.append(("ready", {}))
        elif r < 0.42 or k == busy_at:            # a single-stage call with the busy set outstanding
            ops.append(("detect", dict(stream=int(rng.integers(cfg["n"])), probe=int(rng.integers(2)),
                                        tags=("single_stage_outstanding",))))
        elif r < 0.52 and not sh["fusion"]:
            fusion = 2 if fusion != 2 else 1
            ops.append(("set_fusion", dict(frames=fusion)))
        elif r < 0.6:
            k1 = int(rng.choice([x for x in (0, 64, 256) if x != k1]))
            ops.append(("set_k1_workgroup", dict(threads=k1)))
        elif r < 0.66:
            sc ^= 1
            ops.append(("set_stage_copy", dict(mode=sc)))
    while out:
        ops.append(("collect", {}))
        out -= 1
    ops += [("mog_state", dict(stream=s)) for s in range(cfg["n"])]
    return dict(seed=int(case), size="large", cfg=cfg, ops=ops)


def pair_scenarios(seed):
    """Two scenarios of different geometry and ring depth, and the order their operations are merged in."""
    a = scenario(seed)
    for j in range(1, 50):
        b = scenario(seed + 1000 * j, avoid_geometry=(a["cfg"]["rows"], a["cfg"]["cols"]))
        if b["cfg"]["ring"] != a["cfg"]["ring"]:
            break
    rng = np.random.default_rng([0x3E6, int(seed)])
    order = np.array([0] * len(a["ops"]) + [1] * len(b["ops"]))
    rng.shuffle(order)
    return a, b, [int(x) for x in order]


def replay_line(scn, contexts=1, threads=False):
    s = f"python tools/fuzz_api.py --seed {scn['seed']} --sequences 1 --only 0 --size {scn['size']}"
    if contexts == 2:
        s += " --contexts 2" + (" --threads" if threads else "")
    return s


# ------------------------------------------------------------------------------------------------------- frames ---

class Frames:
    """The scenario's frame sets, by index: noisy background, a moving blob from set 1 on and, on a BUSY set, specks of the
    blob's colour all over (the pattern of test_back_half_speculation_and_repair).  Deterministic in (seed, index)."""

    def __init__(self, scn):
        c = scn["cfg"]
        self.seed, self.n, self.rows, self.cols, self.ch = scn["seed"], c["n"], c["rows"], c["cols"], c["channels"]
        rng = np.random.default_rng([0xF2A, self.seed, 0 if scn["size"] == "small" else 1])
        shape = (self.n, self.rows, self.cols, self.ch)
        self.base = rng.integers(90, 140, shape).astype(np.int16)
        self.noise = rng.integers(-5, 6, shape).astype(np.int16)
        self.colour = np.array([255, 64, 0], np.uint8) if self.ch == 3 else np.array([250], np.uint8)
        self._cache = {}

    def shape1(self):
        return (self.rows, self.cols, 3) if self.ch == 3 else (self.rows, self.cols)

    def get(self, k, busy=False):
        """-> uint8 (n,) + frame shape; the Model's own copy (never handed to the context)."""
        key = (k, busy)
        if key not in self._cache:
            f = self.base + np.roll(self.noise, (5 * k + 1, 11 * k + 3), axis=(1, 2))
            f = np.clip(f, 0, 255).astype(np.uint8)
            if k > 0:
                bh, bw = max(4, self.rows // 12), max(5, self.cols // 12)
                rng = np.random.default_rng([0xB5E, self.seed, k])
                for s in range(self.n):
                    cy = 2 + (self.rows // 6 + 7 * k + 30 * s) % (self.rows - bh - 4)
                    cx = 2 + (self.cols // 6 + 11 * k + 40 * s) % (self.cols - bw - 4)
                    f[s, cy:cy + bh, cx:cx + bw] = self.colour
                    if busy:
                        f[s][rng.random((self.rows, self.cols)) < 0.08] = self.colour
            if len(self._cache) > 8:
                self._cache.clear()
            self._cache[key] = f.reshape((self.n,) + self.shape1())
        return self._cache[key]

    def probe(self, i):
        """A calm frame of stream 0 as the single-stage detectors take it: HSV for BGR contexts, GREY as it is."""
        f = self.get(1 + i)[0]
        return O.bgr2hsv(f) if self.ch == 3 else f


def runs_over_capacity(morph):
    """The LDS blob kernel declines this mask: more runs (or dirty rows) than it holds, counted by tests/blob_load.py."""
    return over_run_capacity(morph)


# -------------------------------------------------------------------------------------------------------- model ---

def _hsv_params(det):
    return O.hsv_params(**det)


def threshold_mask(work, det, rows, cols, ch):
    """The inRange output of a filtered frame (OATGPU_TAP_THRESHOLD) under detector `det`."""
    if ch == 3:
        hsv = O.bgr2hsv(work.reshape(rows, cols, 3))
        return O.inrange3(hsv, (det["h_lo"], det["s_lo"], det["v_lo"]), (det["h_hi"], det["s_hi"], det["v_hi"]))
    return O.inrange1(work.reshape(rows, cols), det["h_lo"], det["h_hi"])


def tap(last, which):
    """Tap `which` of one stream's remembered (threshold mask, morph mask): both made with the detector in force when the
    set was handed over, as the bits in the library's ring slot are."""
    thr, morph = last
    return thr if which == 0 else morph if which == 1 else frame_zeroed(morph) * 255


class Model:
    """What the reference chain gives for the calls made so far."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.n, self.rows, self.cols, self.ch = cfg["n"], cfg["rows"], cfg["cols"], cfg["channels"]
        self.mog = [O.Mog2(self.rows, self.cols, self.ch, params=dict(restore_nmodes=cfg["restore"])) for _ in range(self.n)]
        self.det = dict(cfg["det"])
        self.kal = [O.Kalman(**cfg["kalman"]) for _ in range(self.n)] if cfg["kalman"] else None
        self.roi = None
        if cfg["roi"]:
            self.roi = (cfg["roi"]["stream"], roi_mask(cfg))
        self.fifo = []
        self.last = None              # per stream (threshold mask, morph mask) of the latest set
        self.enqueued = self.collected = 0
        self.nthreads = cfg["nthreads"]

    def set_kalman(self, enable):
        self.kal = [O.Kalman(**KALMAN) for _ in range(self.n)] if enable else None

    def push(self, frames, lr):
        """One frame set through the chain with the parameters and rate in force NOW -> the expected result set."""
        p = _hsv_params(self.det)
        want, last, busy = [], [], False
        for s in range(self.n):
            f = frames[s]
            if self.roi and self.roi[0] == s:
                f = f.copy()
                f[self.roi[1] == 0] = 0
            d, morph = O.chain_step(self.mog[s], f, lr, p, nthreads=self.nthreads)
            k = self.kal[s].filter(d["valid"], d["x"], d["y"]) if self.kal else None
            want.append((d, k))
            last.append((threshold_mask(self.mog[s]._work[0], self.det, self.rows, self.cols, self.ch), morph))
            busy = busy or runs_over_capacity(morph)
        self.last = last
        self.enqueued += 1
        rec = dict(want=want, busy=busy, id=self.enqueued)
        self.fifo.append(rec)
        return rec

    def pop(self):
        self.collected += 1
        return self.fifo.pop(0)

    def mask(self, which, s):
        return tap(self.last[s], which)


def roi_mask(cfg):
    r = cfg["roi"]
    m = np.zeros((cfg["rows"], cfg["cols"]), np.uint8)
    m[r["y0"]:r["y1"], r["x0"]:r["x1"]] = 255
    return m


def same_result(got, want, tag):
    """One stream's collected Position2D against (detection, filtered) of the Model; with the filter on, the fields
    test_kalman_filter_on_the_batch_matches_oracle compares, bit for bit."""
    d, k = want
    if k is None:
        _same_detection(got, d, tag)
        return
    assert got.raw_valid == d["valid"], (tag, got, d)
    if d["valid"]:
        assert (got.raw_x, got.raw_y, got.a00) == (d["x"], d["y"], d["a00"]), (tag, got, d)
    assert got.position_valid == k["position_valid"] and got.velocity_valid == k["velocity_valid"], (tag, got, k)
    assert (got.x, got.y, got.vx, got.vy) == (k["x"], k["y"], k["vx"], k["vy"]), (tag, got, k)


# ------------------------------------------------------------------------------------------------------ buffers ---

class _HostBuf:
    def __init__(self, arr, free=None):
        self.arr, self.free = arr, free

    def scribble(self, junk):
        self.arr[...] = junk


class CpuMemory:
    """'Device' memory of a FakeHotPath: numpy arrays it finds by address."""

    def __init__(self, hp):
        self.hp = hp

    class _Dev(_HostBuf):
        @property
        def ptr(self):
            return self.arr.ctypes.data

    def pinned(self, shape):
        return _HostBuf(np.empty(shape, np.uint8))

    def dev_new(self, frames):
        b = CpuMemory._Dev(frames.copy())
        self.hp.device_memory[b.ptr] = b.arr
        return b

    def dev_refill(self, b, frames):
        b.arr[...] = frames              # (the fake read the previous frame inside enqueue_dev: stream order)

    def release(self):
        pass


class GpuMemory:
    """Device memory through torch; host frames in oatgpu_host_alloc memory.  Fills of a buffer of its own and every
    overwrite run on a side stream that is waited for (so nothing but the library's own ordering protects a frame); the
    refill of the REUSED buffer runs in stream order on the context's HIP stream and is not waited for."""

    def __init__(self, hp):
        import torch
        self.torch, self.hp = torch, hp
        self.dev = torch.device("cuda:0")
        self.side = torch.cuda.Stream(device=self.dev)
        self.ext = torch.cuda.ExternalStream(hp.get_stream(), device=self.dev)
        self.keep, self.allocs = [], []

    class _Dev:
        def __init__(self, mem, t):
            self.mem, self.t, self.ptr = mem, t, t.data_ptr()

        def scribble(self, junk):
            torch = self.mem.torch
            with torch.cuda.stream(self.mem.side):
                self.t.random_(0, 256)
            self.mem.side.synchronize()

    def pinned(self, shape):
        import ctypes as C
        nbytes = int(np.prod(shape))
        p = self.hp.lib.oatgpu_host_alloc(nbytes)
        assert p, "oatgpu_host_alloc failed"
        self.allocs.append(p)
        arr = np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(p)).reshape(shape)
        return _HostBuf(arr)

    def dev_new(self, frames):
        torch = self.torch
        t = torch.empty(frames.shape, dtype=torch.uint8, device=self.dev)
        with torch.cuda.stream(self.side):
            t.copy_(torch.from_numpy(np.ascontiguousarray(frames)))
        self.side.synchronize()
        return GpuMemory._Dev(self, t)

    def dev_refill(self, b, frames):
        torch = self.torch
        src = torch.from_numpy(frames.copy()).pin_memory()
        self.keep.append(src)                     # until the context is closed: the copy is asynchronous
        with torch.cuda.stream(self.ext):
            b.t.copy_(src, non_blocking=True)

    def release(self):
        self.torch.cuda.synchronize()
        for p in self.allocs:
            self.hp.lib.oatgpu_host_free(p)
        self.allocs, self.keep = [], []


# ------------------------------------------------------------------------------------------------------- driver ---

def open_context(scn, factory, **extra):
    """The scenario's context: factory is oat_amd.HotPath or FakeHotPath (same arguments)."""
    c, d = scn["cfg"], scn["cfg"]["det"]
    kw = dict(n_streams=c["n"], ring_depth=c["ring"], channels=c["channels"], adaptation_coeff=c["lr"],
              h_thresh=(d["h_lo"], d["h_hi"]), erode=d["erode"], dilate=d["dilate"], area=(d["min_area"], d["max_area"]),
              mog_restore_nmodes=c["restore"])
    if c["channels"] == 3:
        kw.update(s_thresh=(d["s_lo"], d["s_hi"]), v_thresh=(d["v_lo"], d["v_hi"]))
    kw.update(extra)
    hp = factory(c["rows"], c["cols"], **kw)
    if c["roi"]:
        hp.set_roi_mask(roi_mask(c), stream=c["roi"]["stream"])
    if c["kalman"]:
        hp.set_kalman(True, **c["kalman"])
    return hp


class Runner:
    """Runs a scenario's operations on a context, one step() at a time, and checks every result against the Model."""

    def __init__(self, hp, scn, memory=None, log=None, contexts=1, threads=False):
        self.hp, self.scn, self.cfg, self.ops = hp, scn, scn["cfg"], scn["ops"]
        self.mem = memory or (GpuMemory(hp) if hasattr(hp, "ctx") else CpuMemory(hp))
        self.model = Model(self.cfg)
        self.frames = Frames(scn)
        self.n = self.cfg["n"]
        self.log = log
        self.replay = replay_line(scn, contexts, threads)
        self.lr = self.cfg["lr"]
        self.live = []                 # buffers handed over and not yet overwritten: dict(buf, set, stream, state)
        self.staging = []              # ... of the set being staged
        self.shared = None             # the reused device buffer
        self.fusion = 0
        self.latest_dev = False
        self.junk = np.random.default_rng([0x7C, scn["seed"]]).integers(0, 256, (self.n,) + self.frames.shape1(), np.uint8)
        self.stats = collections.Counter()
        self.early_steps = 0
        self.busy_then_collected = False
        self.busy_id = 0
        self.i = 0

    # -- buffers
    def _host_set(self, frames, mem):
        bufs = []
        for s in range(self.n):
            b = self.mem.pinned(frames[s].shape) if mem == "pinned" else _HostBuf(np.empty_like(frames[s]))
            b.arr[...] = frames[s]
            bufs.append(b)
        return bufs

    def _scribble(self, recs, because_consumed=False):
        for r in recs:
            if because_consumed and r["set"] is not None and any(f["id"] == r["set"] for f in self.model.fifo):
                self.stats["overwrite_after_consumed_uncollected"] += 1
            r["buf"].scribble(self.junk[r["stream"] or 0] if r["stream"] is not None else self.junk)
        ids = {id(r) for r in recs}
        self.live = [r for r in self.live if id(r) not in ids]

    def _handed(self, bufs, rec):
        for s, b in enumerate(bufs):
            self.live.append(dict(buf=b, set=rec["id"], stream=s))

    def _push(self, k, busy):
        f = self.frames.get(k, busy)
        rec = self.model.push(f, self.lr)
        if rec["busy"]:
            self.stats["busy_sets"] += 1
        return f, rec

    def _check_set(self, got, rec, tag):
        assert len(got) == self.n, (tag, len(got))
        for s in range(self.n):
            same_result(got[s], rec["want"][s], (tag, "stream", s, "set", rec["id"], "busy", rec["busy"]))

    def _collect(self, tag):
        got = self.hp.collect()
        rec = self.model.pop()
        if rec["busy"]:
            self.busy_id = rec["id"]
        elif self.busy_id and rec["id"] > self.busy_id:
            self.busy_then_collected = True
        self._scribble([r for r in self.live if r["set"] == rec["id"]])
        self._check_set(got, rec, tag)
        self._say(tag, got, rec["want"])
        self._shape()

    def _shape(self):
        if hasattr(self.hp, "last_step_shape") and self.hp.last_step_shape()[1]:
            self.early_steps += 1

    def _say(self, what, got=None, want=None):
        if self.log:
            self.log(f"  [{self.i}] {what}: got {got} | want {want}")

    def _refused(self, call):
        out = self.hp.outstanding()
        try:
            call()
        except OatGpuError as e:
            self._say("refused", str(e))
        else:
            raise AssertionError("the call was accepted; include/oatgpu.h refuses it")
        assert self.hp.outstanding() == out == len(self.model.fifo), (self.hp.outstanding(), out, len(self.model.fifo))

    def _dev(self, frames, reuse):
        if reuse and self.fusion != 2:
            if self.shared is None:
                self.shared = self.mem.dev_new(frames)
            else:
                self.mem.dev_refill(self.shared, frames)
            return self.shared, False
        return self.mem.dev_new(frames), True

    # -- one operation
    def step(self):
        kind, a = self.ops[self.i]
        try:
            self._step(kind, a)
        except AssertionError as e:
            raise AssertionError(f"seed {self.scn['seed']} ({self.scn['size']}) operation {self.i} {kind} {a}: {e}\n"
                                 f"replay: {self.replay}") from e
        except Exception as e:
            raise RuntimeError(f"seed {self.scn['seed']} ({self.scn['size']}) operation {self.i} {kind} {a}: "
                               f"{type(e).__name__}: {e}\nreplay: {self.replay}") from e
        self.stats[kind] += 1
        for t in a.get("tags", ()):
            self.stats[t] += 1
        if kind in SINGLE_STAGE and any(f["busy"] for f in self.model.fifo):
            self.stats["single_stage_busy_outstanding"] += 1
        self.i += 1

    def _step(self, kind, a):
        hp, model, n = self.hp, self.model, self.n
        hp.learning_coeff_ = self.lr
        if kind == "enqueue":
            f, rec = self._push(a["frame"], a["busy"])
            bufs = self._host_set(f, a["mem"])
            hp.enqueue([b.arr for b in bufs])
            self._handed(bufs, rec)
            self.latest_dev = False
            self._say(kind, None, rec["want"])
            self._shape()
        elif kind == "enqueue_dev":
            f, rec = self._push(a["frame"], a["busy"])
            b, own = self._dev(f, a["reuse"])
            hp.enqueue_dev(b.ptr, keepalive=b)
            if own:
                self.live.append(dict(buf=b, set=rec["id"], stream=None))
            self.latest_dev = True
            self._say(kind, None, rec["want"])
            self._shape()
        elif kind == "stage":
            f = self.frames.get(a["frame"], a["busy"])[a["stream"]]
            b = self.mem.pinned(f.shape) if a["mem"] == "pinned" else _HostBuf(np.empty_like(f))
            b.arr[...] = f
            hp.stage(a["stream"], b.arr)
            self.staging.append(dict(buf=b, set=None, stream=a["stream"], frame=(a["frame"], a["busy"])))
        elif kind == "enqueue_staged":
            k, busy = self.staging[0]["frame"]
            _, rec = self._push(k, busy)
            hp.enqueue_staged()
            for r in self.staging:
                r["set"] = rec["id"]
                self.live.append(r)
            self.staging = []
            self.latest_dev = False
            self._say(kind, None, rec["want"])
        elif kind == "stage_abort":
            hp.stage_abort()
            self._scribble(self.staging)
            self.staging = []
            assert hp.outstanding() == len(model.fifo), "a given-up set owes no result"
        elif kind == "collect":
            self._collect(kind)
        elif kind == "ready":
            got = hp.ready()
            if not model.fifo:
                assert got is False, "ready with nothing outstanding"
            self._say(kind, got, "False" if not model.fifo else "either")
        elif kind == "ready_poll":
            t0 = time.perf_counter()
            while not hp.ready():
                assert time.perf_counter() - t0 < 10.0, "the oldest result was not ready within 10 s"
        elif kind == "outstanding":
            got = hp.outstanding()
            assert got == len(model.fifo), (got, len(model.fifo))
        elif kind == "input_consumed":
            hp.input_consumed()
            self._scribble(list(self.live), because_consumed=True)
        elif kind == "input_consumed_stream":
            hp.input_consumed_stream(a["stream"])
            if self.staging:
                recs = [r for r in self.staging if r["stream"] == a["stream"] and not r.get("done")]
                for r in recs:
                    r["buf"].scribble(self.junk[a["stream"]])
                    r["done"] = True
            elif self.latest_dev:           # "for device frames it is oatgpu_track_input_consumed"
                self._scribble(list(self.live), because_consumed=True)
            else:
                latest = model.enqueued
                self._scribble([r for r in self.live if r["set"] == latest and r["stream"] == a["stream"]], because_consumed=True)
        elif kind == "set_lr":
            self.lr = a["lr"]
        elif kind == "track":
            f, rec = self._push(a["frame"], a["busy"])
            bufs = self._host_set(f, "host")
            got = hp.track([b.arr for b in bufs])
            for b in bufs:
                b.scribble(self.junk[0])
            self._check_set(got, model.pop(), kind)
            self._say(kind, got, rec["want"])
        elif kind == "track_dev":
            f, rec = self._push(a["frame"], a["busy"])
            b = self.mem.dev_new(f)
            got = hp.track_dev(b.ptr)
            b.scribble(self.junk)
            self._check_set(got, model.pop(), kind)
            self._say(kind, got, rec["want"])
        elif kind == "track_sequence_dev":
            recs, bufs = [], []
            for k, busy in zip(a["frames"], a["busy"]):
                f, rec = self._push(k, busy)
                recs.append(rec)
                bufs.append(self.mem.dev_new(f))
            got = hp.track_sequence_dev([b.ptr for b in bufs])
            for b in bufs:
                b.scribble(self.junk)
            assert len(got) == len(recs), (len(got), len(recs))
            for t, g in enumerate(got):
                self._check_set(g, model.pop(), (kind, t))
            self._say(kind, got, [r["want"] for r in recs])
        elif kind == "detect":
            probe = self.frames.probe(a["probe"])
            p = _hsv_params(model.det)
            if self.cfg["channels"] == 3:
                got, want = hp.detect_hsv(probe.copy(), a["stream"]), O.detect_hsv(probe, p)[0]
            else:
                got, want = hp.detect_thresh(probe.copy(), a["stream"]), O.detect_thresh(probe, p)[0]
            _same_detection(got, want, kind)
            self._say(kind, got, want)
        elif kind == "mog_state":
            _same_state(hp.mog_state(a["stream"]), model.mog[a["stream"]].state(), (kind, a["stream"]))
        elif kind == "read_mask":
            got, want = hp.read_mask(a["which"], a["stream"]), model.mask(a["which"], a["stream"])
            assert (got == want).all(), f"tap {a['which']} of stream {a['stream']}: {int((got != want).sum())} pixels differ"
        elif kind == "set_detector":
            hp._set(**a["det"])
            model.det = dict(a["det"])
        elif kind == "set_fusion":
            hp.set_fusion(a["frames"])
            self.fusion = a["frames"]
            if self.fusion == 2:
                self.shared = None            # back to one buffer a frame
        elif kind == "set_early_blob":
            hp.set_early_blob(None if a["on"] < 0 else bool(a["on"]))
        elif kind == "set_k1_workgroup":
            hp.set_k1_workgroup(a["threads"])
        elif kind == "set_stage_copy":
            hp.set_stage_copy(a["mode"])
        elif kind == "set_kalman":
            hp.set_kalman(a["enable"], **KALMAN)
            model.set_kalman(a["enable"])
        # ---- deliberate refusals: OatGpuError, and nothing has moved
        elif kind in ("r_enqueue_full", "r_enqueue_staging"):
            if a["form"] == "host":
                self._refused(lambda: hp.enqueue([self.junk[s].copy() for s in range(n)]))
            else:
                b = self.mem.dev_new(self.junk)
                self._refused(lambda: hp.enqueue_dev(b.ptr))
        elif kind == "r_stage_full":
            self._refused(lambda: hp.stage(0, self.junk[0].copy()))
        elif kind == "r_collect_empty":
            self._refused(hp.collect)
        elif kind == "r_sync_outstanding":
            if a["form"] == "track":
                self._refused(lambda: hp.track([self.junk[s].copy() for s in range(n)]))
            else:
                b = self.mem.dev_new(self.junk)
                self._refused((lambda: hp.track_dev(b.ptr)) if a["form"] == "track_dev" else
                              (lambda: hp.track_sequence_dev([b.ptr, b.ptr])))
        elif kind == "r_set_kalman":
            self._refused(lambda: hp.set_kalman(True, **KALMAN))
        elif kind == "r_set_homography":
            self._refused(lambda: hp.set_homography(IDENTITY9))
        elif kind == "r_staged_short":
            self._refused(hp.enqueue_staged)
        elif kind == "r_stage_twice":
            self._refused(lambda: hp.stage(a["stream"], self.junk[0].copy()))
        elif kind == "r_stream_range":
            if a["form"] == "stage":
                self._refused(lambda: hp.stage(a["stream"], self.junk[0].copy()))
            else:
                self._refused(lambda: hp.input_consumed_stream(a["stream"]))
        else:
            raise AssertionError(f"unknown operation {kind}")

    def finish(self):
        """Collect what is outstanding, compare every stream's whole model, one token out per token in."""
        self.i = len(self.ops)
        try:
            if self.staging:
                self.hp.stage_abort()
                self.staging = []
            while self.model.fifo:
                self._collect("final collect")
            assert self.hp.outstanding() == 0, f"{self.hp.outstanding()} result sets outstanding after the last collect"
            with_error = None
            try:
                self.hp.collect()
            except OatGpuError as e:
                with_error = e
            assert with_error is not None, "collect with nothing outstanding was accepted"
            for s in range(self.n):
                _same_state(self.hp.mog_state(s), self.model.mog[s].state(), ("final model", s))
            assert self.model.collected == self.model.enqueued, (self.model.collected, self.model.enqueued)
        except AssertionError as e:
            raise AssertionError(f"seed {self.scn['seed']} ({self.scn['size']}) at the end: {e}\nreplay: {self.replay}") from e
        finally:
            self.mem.release()
        self.stats["collected"] = self.model.collected
        self.stats["ops"] = len(self.ops)
        self.stats["refusals"] = sum(self.stats[r] for r in REFUSALS)
        return self.stats

    def run(self):
        while self.i < len(self.ops):
            if self.log:
                self.log(f"[{self.i}] {self.ops[self.i][0]} {self.ops[self.i][1]}")
            self.step()
        return self.finish()


def run_scenario(scn, factory, log=None, **extra):
    hp = open_context(scn, factory, **extra)
    try:
        r = Runner(hp, scn, log=log)
        r.run()
        return r
    finally:
        hp.close()


def run_interleaved(seed, factory, log=None):
    """Two contexts of different scenarios on ONE thread, their operations merged at random."""
    a, b, order = pair_scenarios(seed)
    hps = [open_context(a, factory), open_context(b, factory)]
    try:
        rs = [Runner(hps[i], scn, contexts=2, log=(lambda m, i=i: log(f"ctx {i} {m}")) if log else None) for i, scn in enumerate((a, b))]
        for r in rs:
            r.replay = replay_line(a, 2)
        for which in order:
            if log:
                log(f"ctx {which} [{rs[which].i}] {rs[which].ops[rs[which].i][0]} {rs[which].ops[rs[which].i][1]}")
            rs[which].step()
        return [r.finish() for r in rs]
    finally:
        for hp in hps:
            hp.close()


def run_on_two_threads(seed, factory, cap=60.0, log=None):
    """One context per thread ("one context per host thread"), both started behind a barrier.  A thread still alive after
    `cap` seconds is a failure (reported, never retried); exceptions of the threads are raised here."""
    a, b, _ = pair_scenarios(seed)
    barrier = threading.Barrier(2)
    errors, stats = [None, None], [None, None]

    def work(i, scn):
        try:
            hp = open_context(scn, factory)
            try:
                r = Runner(hp, scn, contexts=2, threads=True, log=(lambda m: log(f"thread {i} {m}")) if log else None)
                r.replay = replay_line(a, 2, True)
                barrier.wait(timeout=cap)
                stats[i] = r.run()
            finally:
                hp.close()
        except BaseException as e:              # noqa: BLE001  (handed to the test's thread)
            errors[i] = e
            barrier.abort()

    ts = [threading.Thread(target=work, args=(i, s), daemon=True) for i, s in enumerate((a, b))]
    t0 = time.perf_counter()
    for t in ts:
        t.start()
    for t in ts:
        t.join(max(0.0, cap - (time.perf_counter() - t0)))
    alive = [i for i, t in enumerate(ts) if t.is_alive()]
    for e in errors:
        if e is not None and not isinstance(e, threading.BrokenBarrierError):
            raise e
    assert not alive, f"seed {seed}: thread(s) {alive} still running after {cap} s\nreplay: {replay_line(a, 2, True)}"
    for e in errors:
        if e is not None:
            raise e
    return stats


# ------------------------------------------------------------------------------------------------- fake context ---

E_INVALID, E_RING_FULL, E_RING_EMPTY = -1, -4, -5
MUTANTS = ("reads_frame_at_collect", "detector_applies_to_enqueued_frame", "pair_results_swapped",
           "single_stage_before_outstanding", "owes_result_after_stage_abort")


class FakeHotPath:
    """oat_amd.HotPath's methods on oracle_lib alone, following include/oatgpu.h: ring, staging, refusals -- and reading a
    caller's buffer at the LAST moment the header allows (a registered frame when its result is asked for, when
    input_consumed is called or when a synchronous call drains), so that a driver that overwrites a buffer too early fails.
    `mutant` names one deliberate bug (MUTANTS)."""

    def __init__(self, rows, cols, n_streams=1, ring_depth=4, channels=3, adaptation_coeff=0.0, h_thresh=(0, 256),
                 s_thresh=(0, 256), v_thresh=(0, 256), erode=0, dilate=10, area=(0.0, 1e300), mog_restore_nmodes=1,
                 mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.rows, self.cols, self.n_streams, self.ring, self.channels = rows, cols, n_streams, ring_depth, channels
        self.learning_coeff_ = float(adaptation_coeff)
        self.mutant = mutant
        self.det = dict(h_lo=h_thresh[0], h_hi=h_thresh[1], erode=erode, dilate=dilate, min_area=area[0], max_area=area[1])
        if channels == 3:
            self.det.update(s_lo=s_thresh[0], s_hi=s_thresh[1], v_lo=v_thresh[0], v_hi=v_thresh[1])
        self.mog = [O.Mog2(rows, cols, channels, params=dict(restore_nmodes=mog_restore_nmodes)) for _ in range(n_streams)]
        self.nframes = [0] * n_streams
        self.kal = None
        self.roi = {}
        self.sets = []                 # outstanding: dict(src, frames, det, lr, kal, result)
        self.staged = {}               # stream -> [source array, copy or None]
        self.fusion = 0
        self.last = None
        self.device_memory = {}        # address -> numpy array (CpuMemory)

    def close(self):
        self.sets = []

    # -- plumbing
    def _fail(self, code, msg):
        raise OatGpuError(code, msg)

    def _read(self, st, streams=None):
        for s in (range(self.n_streams) if streams is None else streams):
            if st["frames"][s] is None:
                st["frames"][s] = st["src"][s].copy()

    def _run(self, frames, det, lr, kal_on):
        p = _hsv_params(det)
        res, last = [], []
        for s in range(self.n_streams):
            f = frames[s]
            if s in self.roi:
                f = f.copy()
                f[self.roi[s] == 0] = 0
            d, morph = O.chain_step(self.mog[s], f, lr, p)
            self.nframes[s] += 1
            pos = Position2D(d["valid"], d["x"], d["y"], d["area"], d["a00"], d["a10"], d["a01"], d["first_pixel"])
            if kal_on and self.kal:
                k = self.kal[s].filter(d["valid"], d["x"], d["y"])
                pos = Position2D(k["position_valid"], k["x"], k["y"], d["area"], d["a00"], d["a10"], d["a01"], d["first_pixel"],
                                 k["velocity_valid"], k["vx"], k["vy"], d["valid"], d["x"], d["y"])
            res.append(pos)
            last.append((threshold_mask(self.mog[s]._work[0], det, self.rows, self.cols, self.channels), morph))
        self.last = last
        return res

    def _compute(self, upto=None):
        todo = [st for st in (self.sets if upto is None else self.sets[:upto]) if st["result"] is None]
        for st in todo:
            self._read(st)
            det = self.det if self.mutant == "detector_applies_to_enqueued_frame" else st["det"]
            st["result"] = self._run(st["frames"], det, st["lr"], st["kal"])
            for s, pos in st.get("spoiled", {}).items():
                st["result"][s] = pos
        if self.mutant == "pair_results_swapped" and len(todo) >= 2:
            todo[0]["result"], todo[1]["result"] = todo[1]["result"], todo[0]["result"]

    def _quiesce(self):
        self._compute()

    def _refuse_pipelined(self, staging=True, full=True):
        if staging and self.staged:
            self._fail(E_INVALID, "a frame set is being staged")
        if full and len(self.sets) == self.ring:
            self._fail(E_RING_FULL, "result ring full: collect first")

    def _register(self, src, frames, dev=False):
        self.sets.append(dict(src=src, frames=frames, det=dict(self.det), lr=self.learning_coeff_, kal=self.kal is not None,
                              result=None, dev=dev))

    def _shape(self, f):
        shape = (self.rows, self.cols, 3) if self.channels == 3 else (self.rows, self.cols)
        assert f.shape == shape and f.dtype == np.uint8 and f.flags.c_contiguous
        return f

    def _device(self, ptr):
        if ptr not in self.device_memory:
            self._fail(E_INVALID, "unknown device address")
        return self.device_memory[ptr]

    # -- pipelined entry points
    def enqueue(self, frames):
        if len(frames) != self.n_streams:
            self._fail(E_INVALID, "expected n frames")
        self._refuse_pipelined()
        self._register([self._shape(f) for f in frames], [None] * self.n_streams)

    def enqueue_dev(self, dev_ptr, keepalive=None):
        self._refuse_pipelined()
        a = self._device(dev_ptr)
        if self.fusion == 2 and self.ring >= 2:       # registered: read when it is launched
            self._register(list(a), [None] * self.n_streams, dev=True)
        else:                                         # the kernel is queued inside the call: stream order
            self._register(None, [f.copy() for f in a], dev=True)

    def stage(self, stream, frame):
        if not 0 <= stream < self.n_streams:
            self._fail(E_INVALID, "stream index out of range")
        if not self.staged:
            self._refuse_pipelined(staging=False)
        if stream in self.staged:
            self._fail(E_INVALID, "stream is already staged for this frame set")
        self.staged[stream] = [self._shape(frame), None]

    def enqueue_staged(self):
        if len(self.staged) != self.n_streams:
            self._fail(E_INVALID, f"{len(self.staged)} of {self.n_streams} streams staged")
        self._register([self.staged[s][0] for s in range(self.n_streams)], [self.staged[s][1] for s in range(self.n_streams)])
        self.staged = {}

    def stage_abort(self):
        if self.mutant == "owes_result_after_stage_abort" and self.staged:
            zero = np.zeros((self.rows, self.cols, 3) if self.channels == 3 else (self.rows, self.cols), np.uint8)
            self._register(None, [self.staged[s][0].copy() if s in self.staged else zero for s in range(self.n_streams)])
        self.staged = {}

    def collect(self):
        if not self.sets:
            self._fail(E_RING_EMPTY, "nothing outstanding")
        self._compute(upto=2 if self.mutant == "pair_results_swapped" else 1)
        return self.sets.pop(0)["result"]

    def ready(self):
        if not self.sets:
            return False
        self._compute(upto=1)
        return True

    def outstanding(self):
        return len(self.sets)

    def input_consumed(self):
        if self.mutant == "reads_frame_at_collect":
            return
        for st in self.sets:
            self._read(st)

    def input_consumed_stream(self, stream):
        if not 0 <= stream < self.n_streams:
            self._fail(E_INVALID, "stream index out of range")
        if self.mutant == "reads_frame_at_collect":
            return
        if self.staged:
            if stream not in self.staged:
                self._fail(E_INVALID, "stream is not staged")
            if self.staged[stream][1] is None:
                self.staged[stream][1] = self.staged[stream][0].copy()
        elif self.sets:
            st = self.sets[-1]
            if st["dev"]:
                self.input_consumed()
            else:
                self._read(st, [stream])

    # -- synchronous entry points
    def _sync_refusals(self, what):
        if self.sets:
            self._fail(E_INVALID, f"{what} while enqueued results are outstanding")
        if self.staged:
            self._fail(E_INVALID, "a frame set is being staged")

    def track(self, frames):
        if len(frames) != self.n_streams:
            self._fail(E_INVALID, "expected n frames")
        self._sync_refusals("track_batch")
        return self._run([self._shape(f) for f in frames], self.det, self.learning_coeff_, True)

    def track_dev(self, dev_ptr):
        self._sync_refusals("track_batch")
        return self._run(list(self._device(dev_ptr)), self.det, self.learning_coeff_, True)

    def track_sequence_dev(self, dev_ptrs):
        self._sync_refusals("track_sequence")
        return [self._run(list(self._device(p)), self.det, self.learning_coeff_, True) for p in dev_ptrs]

    # -- single-stage calls
    def _detect(self, img, stream, fn):
        if not 0 <= stream < self.n_streams:
            self._fail(E_INVALID, "stream index out of range")
        d = fn(img, _hsv_params(self.det))[0]
        pos = Position2D(d["valid"], d["x"], d["y"], d["area"], d["a00"], d["a10"], d["a01"], d["first_pixel"])
        if self.mutant == "single_stage_before_outstanding":
            for st in self.sets:              # its threshold bits land in an outstanding frame's slot
                if st["result"] is None:
                    st.setdefault("spoiled", {})[stream] = pos
                    break
        else:
            self._quiesce()
        return pos

    def detect_hsv(self, hsv, stream=0):
        return self._detect(hsv, stream, O.detect_hsv)

    def detect_thresh(self, grey, stream=0):
        return self._detect(grey, stream, O.detect_thresh)

    def mog_state(self, stream=0):
        self._quiesce()
        return self.mog[stream].state() + (self.nframes[stream],)

    def read_mask(self, which=1, stream=0):
        self._quiesce()
        return tap(self.last[stream], which)

    # -- settings
    def _set(self, **kw):
        if self.mutant != "detector_applies_to_enqueued_frame":
            self._quiesce()
        self.det.update(kw)

    def set_fusion(self, frames_per_launch):
        if frames_per_launch not in (1, 2):
            self._fail(E_INVALID, "frames_per_launch must be 1 or 2")
        self._quiesce()
        self.fusion = frames_per_launch

    def set_early_blob(self, on=True):
        pass

    def set_k1_workgroup(self, threads=0):
        if threads not in (0, 64, 256):
            self._fail(E_INVALID, "k1 workgroup must be 0 (by path), 64 or 256")

    def set_stage_copy(self, mode):
        if mode not in (0, 1):
            self._fail(E_INVALID, "stage copy mode must be 0 (DMA) or 1 (kernel)")

    def set_kalman(self, enable=True, dt=0.02, timeout=0.0, sigma_accel=5.0, sigma_noise=0.0):
        if self.sets:
            self._fail(E_INVALID, "set_kalman while enqueued results are outstanding")
        self.kal = [O.Kalman(dt, timeout, sigma_accel, sigma_noise) for _ in range(self.n_streams)] if enable else None

    def set_homography(self, h=None):
        if self.sets:
            self._fail(E_INVALID, "set_homography while enqueued results are outstanding")
        if h is not None:
            raise NotImplementedError("the sequence tests leave the homography out")

    def set_roi_mask(self, mask, stream=0):
        self._quiesce()
        if mask is None:
            self.roi.pop(stream, None)
        else:
            self.roi[stream] = np.array(mask, np.uint8)

    def get_stream(self):
        return 0
