"""Every instantiation of the per-pixel MOG2 kernel (k_mog_fused<CH, AUDIT, NTLD, NF, FROZEN, WG>, oat_amd/csrc/kernels_mog.hip)
and how the pipelined track path is made to launch it, restated in Python.  No GPU and no product code here.

  * SCENARIOS: one row per instantiation the library holds, with a readable id and the settings that reach it -- channels,
    oatgpu_set_fusion, oatgpu_set_k1_workgroup, the rate schedule, the kind of frames and the traffic audit;
  * the launcher's choice, restated: launch_mog_fused / launch_mog_pick / launch_mog_ch / rate_in_range (kernels_mog.hip),
    the workgroup rule of plan_step, the pairing rule of launch_front, frozen_ok of mog_launch_opts, the density switch and
    the probe schedule of launch_front, what k_density_probe counts (api_track.hip);
  * frame generators for the regimes: sparse (SyntheticStream discs), dense (five well separated levels a pixel, own
    phase: five live modes), mixed (sparse with a tenth of the pixels cycling through six levels: full mixtures that keep
    replacing their last mode, while the mean stays well below the density switch) and shadows (a moving patch at 0.7 x
    the frame).

tests/test_mog_matrix_cpu.py checks the table against the symbols of the built library, the restated rules against the
sources, and every regime against the C oracle; tests/test_mog_matrix_gpu.py runs every row on the device.
"""
from dataclasses import dataclass, field

import numpy as np

FIELDS = ("CH", "AUDIT", "NTLD", "NF", "FROZEN", "WG")

# ---- constants of the sources (test_mog_matrix_cpu.py reads them back out of the sources) ----
COUNT_MASK, LIVE_SHIFT = 7, 2            # counter byte: mode count in bits 0..2, live hint of slot k >= 1 in bit 2 + k
DENSE_NUM, DENSE_DEN = 5, 2              # nt_loads = 2 * live >= 5 * samples: mean live modes >= 2.5
PROBE_SAMPLES = 16384                    # k_density_probe: one workgroup, a coarse lattice of 16 384 counter bytes
RATE_MIN, PRUNE_MIN = 2.0 ** -40, 2.0 ** -60     # rate_in_range
WARM_RATE = 0.02                         # every scenario's learning rate; frozen ones switch to 0 after WARM_FRAMES
WARM_FRAMES = 10


def inst_id(inst):
    ch, audit, ntld, nf, frozen, wg = inst
    kind = "audit" if audit else "stream" if ntld else "frozen" if frozen else "plain"
    return f"{'grey' if ch == 1 else 'bgr'}-{kind}-nf{nf}-wg{wg}"


def mangled(inst):
    """The template-argument part of k_mog_fused's mangled name."""
    ch, audit, ntld, nf, frozen, wg = inst
    return f"ILi{ch}ELb{int(audit)}ELb{int(ntld)}ELi{nf}ELb{int(frozen)}ELi{wg}E"


def parse_mangled(name):
    """-> (CH, AUDIT, NTLD, NF, FROZEN, WG) of a k_mog_fused symbol, None for any other name."""
    import re
    m = re.search(r"k_mog_fusedILi(\d+)ELb([01])ELb([01])ELi(\d+)ELb([01])ELi(\d+)E", name)
    return tuple(int(v) for v in m.groups()) if m else None


# ------------------------------------------------------------------------------------------------ scenarios ---

@dataclass
class Scenario:
    inst: tuple                   # (CH, AUDIT, NTLD, NF, FROZEN, WG) it exists to reach
    channels: int
    fusion: int                   # oatgpu_set_fusion
    wg_force: int                 # oatgpu_set_k1_workgroup from the start: 0 (by path), 64 or 256
    data: str                     # "sparse" | "dense"
    audit: bool = False           # oatgpu_traffic_audit
    frozen: bool = False          # WARM_FRAMES at WARM_RATE, then 0
    wg_after_switch: int = 0      # dense: forced once the switch to the streaming loads has been seen (0: none)
    nframes: int = 36
    shape: tuple = field(default=(40, 101))

    @property
    def id(self):
        return inst_id(self.inst)

    def rate(self, t):
        return 0.0 if (self.frozen and t >= WARM_FRAMES) else WARM_RATE


def _scenarios():
    out = []
    for ch in (3, 1):
        for nf in (1, 2):
            for wg in (64, 256):
                shape = (40, 101) if (nf + wg // 64) % 2 else (48, 128)          # odd and even widths, both channel counts
                # plain: sparse frames at a rate; 256 is the path's own choice there (and the sparse control of the switch)
                out.append(Scenario((ch, 0, 0, nf, 0, wg), ch, nf, 64 if wg == 64 else 0, "sparse", shape=shape))
                # streaming loads: a dense model; the path switches itself to 64 -- 256 is forced once it has
                out.append(Scenario((ch, 0, 1, nf, 0, wg), ch, nf, 0, "dense", wg_after_switch=256 if wg == 256 else 0,
                                    nframes=40, shape=shape))
                # frozen: warm-up at a rate, then 0
                out.append(Scenario((ch, 0, 0, nf, 1, wg), ch, nf, 64 if wg == 64 else 0, "sparse", frozen=True, shape=shape))
    # audited: always 256 threads; GREY is never paired under the audit
    out.append(Scenario((3, 1, 0, 2, 0, 256), 3, 2, 0, "sparse", audit=True))
    out.append(Scenario((3, 1, 0, 1, 0, 256), 3, 1, 0, "sparse", audit=True, shape=(48, 128)))
    out.append(Scenario((1, 1, 0, 1, 0, 256), 1, 2, 0, "sparse", audit=True))
    return out


SCENARIOS = _scenarios()
INSTANTIATIONS = {sc.inst for sc in SCENARIOS}


# ------------------------------------------------------------------------------------ the launcher, restated ---

def mog_begin(nframes, lr, history=500, ct=0.05):
    """BackgroundSubtractorMOG2Impl::apply's prologue (api_track.hip mog_begin): -> (fresh, nframes after, alphaT, prune)."""
    fresh = nframes == 0 or lr >= 1
    nf = (0 if fresh else nframes) + 1
    lim = 2 * nf if 2 * nf < history else history
    lr = lr if (lr >= 0 and nf > 1) else 1.0 / lim
    return fresh, nf, np.float32(lr), np.float32(-lr * float(np.float32(ct)))


def frozen_ok(var_init=15.0, var_min=4.0, var_max=75.0):
    vi, lo, hi = np.float32(var_init), np.float32(var_min), np.float32(var_max)
    return bool(lo <= vi <= hi and lo > 0)


def rate_in_range(aT, prune):
    aT, prune = np.float32(aT), np.float32(prune)
    if aT == 0:
        return True
    return bool(np.float32(RATE_MIN) <= aT <= 1 and np.float32(PRUNE_MIN) <= -prune <= np.float32(0.5) * aT)


def _pick(ch, nf, audit, ntld, frozen, wg):
    """launch_mog_pick + launch_mog_ch for one launch."""
    if nf == 2 and audit:
        return (3, 1, 0, 2, 0, 256)               # (audited pairs are BGR: the pairing rule's business)
    if audit:
        return (ch, 1, 0, 1, 0, 256)
    wg = 64 if wg == 64 else 256
    if ntld:
        return (ch, 0, 1, nf, 0, wg)
    return (ch, 0, 0, nf, 1 if frozen else 0, wg)


def k1_launches(ch, rates, fresh, nt_loads, frozen_ok_, wild, audit, wg):
    """launch_mog_fused: the instantiations ONE per-pixel launch runs.  rates: [(alphaT, prune)] of its frame, or of its
    two frames (a paired launch); fresh: the first frame builds the model anew."""
    aT, pr = rates[0]
    two = len(rates) == 2
    aT2, pr2 = rates[1] if two else (None, None)
    frozen = frozen_ok_ and not nt_loads and aT == 0 and (aT2 == 0 if two else not fresh)
    in_range = not wild and rate_in_range(aT, pr) and (not two or rate_in_range(aT2, pr2))
    if not audit and not in_range:
        if two:                          # split into two one-frame launches through the audit instantiations
            f1 = frozen_ok_ and not nt_loads and aT == 0 and not fresh
            f2 = frozen_ok_ and not nt_loads and aT2 == 0
            return [_pick(ch, 1, True, nt_loads, f1, 256), _pick(ch, 1, True, nt_loads, f2, 256)]
        audit = True
    return [_pick(ch, 2 if two else 1, audit, nt_loads, frozen, wg)]


def step_workgroup(force, nt_loads, early=False, lone_early=False):
    """plan_step's k1_wg: forced, else 64 on the early layout, on a dense model (streaming loads) or for a lone frame of
    the early shape, else 256."""
    return force if force else (64 if (early or nt_loads or lone_early) else 256)


def paired(nj, fresh1, fresh2, audit, channels):
    """launch_front: the two frames of a step go into ONE launch unless one of them is fresh; GREY is never paired under
    the audit."""
    return nj == 2 and not fresh1 and not fresh2 and not (audit and channels != 3)


def may_fuse(fuse, ring_depth, audit, channels, frames_ready=False, in_sequence=False):
    """enqueue_frames: whether a host frame set is held back to be launched with the next one."""
    want = fuse == 2 or (fuse == 0 and (frames_ready or in_sequence))
    return want and ring_depth >= 2 and not (audit and channels != 3)


def probe_at(t):
    """launch_front: density probes at frames 8, 16, 32, then every 64th."""
    return (8 <= t < 64 and (t & (t - 1)) == 0) or (t >= 64 and t % 64 == 0)


def dense_flag(live, samples):
    return DENSE_DEN * live >= DENSE_NUM * samples


def counter_bytes(nm, w):
    """The counter byte k_mog_fused stores for an oracle state: the count, and the live hint of every slot k >= 1 below
    it whose weight has a nonzero bit pattern."""
    nm = np.asarray(nm, np.int64)
    c = nm.copy()
    bits = np.asarray(w, np.float32).view(np.uint32) != 0
    for k in range(1, w.shape[1]):
        c |= ((k < nm) & bits[:, k]).astype(np.int64) << (LIVE_SHIFT + k)
    return c.astype(np.uint8)


def density_probe(counters, rows, cols):
    """k_density_probe over the streams' counter planes (each padded to Palloc pixels of rows x Wp):
    -> (sum of 1 + live hints over sampled bytes with a nonzero count, samples with a nonzero count)."""
    wp = (cols + 63) // 64 * 64
    palloc = (rows * wp + 1023) // 1024 * 1024
    plane = np.zeros((len(counters), palloc), np.uint8)
    for s, c in enumerate(counters):
        plane[s, :rows * wp].reshape(rows, wp)[:, :cols] = np.asarray(c).reshape(rows, cols)
    flat = plane.reshape(-1)
    stride = flat.size // PROBE_SAMPLES if flat.size > PROBE_SAMPLES else 1
    smp = flat[np.arange(0, flat.size, stride)]
    smp = smp[np.arange(smp.size) * stride < flat.size]
    live = smp[(smp & COUNT_MASK) != 0].astype(np.int64)
    hints = sum(((live >> (LIVE_SHIFT + k)) & 1) for k in range(1, 5))
    return int((1 + hints).sum()), int(live.size)


# ------------------------------------------------------------------------------------------------ frames ---

BGR_LEVELS = np.array([[20, 30, 40], [90, 200, 60], [200, 60, 120], [240, 240, 230], [40, 130, 220]], np.int16)  # tools/state_check.py
GREY_LEVELS = np.array([20, 70, 120, 170, 230], np.int16)
SHADOW_FACTOR = 0.7


def sparse_frames(n_streams, rows, cols, ch, nframes, seed=0):
    """SyntheticStream: gradient, noise of +-4, a flickering 64th of the pixels, a moving disc from frame 1 on (GREY: channel 1)."""
    from oat_amd.synth import SyntheticStream
    st = [SyntheticStream(rows, cols, seed + s, n_discs=1, noise=4) for s in range(n_streams)]
    out = []
    for t in range(nframes):
        fs = [x.frame(t, with_discs=t > 0) for x in st]
        out.append([f if ch == 3 else np.ascontiguousarray(f[:, :, 1]) for f in fs])
    return out


def dense_frames(n_streams, rows, cols, ch, nframes, seed=0):
    """Every pixel steps through five well separated levels, each pixel with its own phase (BGR: state_check.py's table,
    +-5; GREY: 20/70/120/170/230 +-3): five live modes everywhere after five frames."""
    rng = np.random.default_rng(0xD0 + seed)
    phase = rng.integers(0, 5, (n_streams, rows, cols))
    out = []
    for t in range(nframes):
        fs = []
        for s in range(n_streams):
            if ch == 3:
                f = BGR_LEVELS[(phase[s] + t) % 5] + rng.integers(-5, 6, (rows, cols, 3))
            else:
                f = GREY_LEVELS[(phase[s] + t) % 5] + rng.integers(-3, 4, (rows, cols))
            fs.append(np.clip(f, 0, 255).astype(np.uint8))
        out.append(fs)
    return out


def mixed_frames(n_streams, rows, cols, ch, nframes, seed=0):
    """Sparse frames in which every tenth pixel cycles through six levels (own phase): those hold full mixtures of any
    size and replace their last mode again and again; the mean stays far below the density switch."""
    base = sparse_frames(n_streams, rows, cols, ch, nframes, seed)
    rng = np.random.default_rng(0x3E + seed)
    cyc = (np.arange(rows * cols).reshape(rows, cols) % 10) == 3
    phase = rng.integers(0, 6, (n_streams, rows, cols))
    levels = np.array([10, 55, 100, 145, 190, 235], np.int16)
    for t, fs in enumerate(base):
        for s, f in enumerate(fs):
            v = levels[(phase[s] + t) % 6]
            if ch == 3:
                f[cyc] = np.stack([v, 255 - v, (v + 90) % 256], -1)[cyc]
            else:
                f[cyc] = v[cyc]
    return base


def shadow_box(t, rows, cols, s=0):
    """The patch that turns into a shadow at frame t (None before frame 3): 6 x 10 pixels, moving."""
    if t < 3:
        return None
    h, w = min(6, rows - 2), min(10, cols - 2)
    y = 1 + (3 * t + 5 * s) % (rows - h - 1)
    x = 1 + (7 * t + 11 * s) % (cols - w - 1)
    return y, x, h, w


def shadow_frames(n_streams, rows, cols, ch, nframes, seed=0, mixed=False):
    """Sparse (or mixed) frames with a moving patch of SHADOW_FACTOR x the frame from frame 3 on."""
    gen = mixed_frames if mixed else sparse_frames
    out = gen(n_streams, rows, cols, ch, nframes, seed)
    for t, fs in enumerate(out):
        for s, f in enumerate(fs):
            b = shadow_box(t, rows, cols, s)
            if b:
                y, x, h, w = b
                f[y:y + h, x:x + w] = (f[y:y + h, x:x + w] * SHADOW_FACTOR).astype(np.uint8)
    return out


def two_level_frames(n_streams, rows, cols, ch, nframes, seed=0):
    """Every pixel has a level A (grey-ish in BGR) and a brighter one B = 4/3 A; over six frames it shows A, A + d, A, B, A,
    A + d (d = 6..9 a channel in BGR, 10..14 in GREY).  Two frames a launch pair frames (even, odd): the first matches
    mode 0 as background, and with varThresholdGen 20 against varThreshold 2 at a rate of 0.1 the second often fits
    mode 0 without being background, is no shadow of mode 0 and, mode 0 weighing less than backgroundRatio, a shadow of
    mode B (mode 1) -- the one place where frame 2 reads a record of mode 1 after fitting mode 0."""
    rng = np.random.default_rng(0x7B + seed)
    g = rng.integers(60, 150, (n_streams, rows, cols)).astype(np.int16)
    a = np.stack([g, g + 5, g - 5], -1) if ch == 3 else g
    b = (a * 4 + 1) // 3
    out = []
    for t in range(nframes):
        ph = t % 6
        d = (6 + (t // 6) % 4) if ch == 3 else (10 + (t // 6) % 5)
        fs = []
        for s in range(n_streams):
            f = b[s] if ph == 3 else a[s] + d if ph in (1, 5) else a[s] + rng.integers(-1, 2, a[s].shape)
            fs.append(np.clip(f, 0, 255).astype(np.uint8))
        out.append(fs)
    return out


def frames_of(kind, n_streams, rows, cols, ch, nframes, seed=0):
    return dict(sparse=sparse_frames, dense=dense_frames, mixed=mixed_frames, two_level=two_level_frames,
                shadow=lambda *a, **k: shadow_frames(*a, **k, mixed=True))[kind](n_streams, rows, cols, ch, nframes, seed)


# ------------------------------------------------------------------------------- the parameter grid (GPU 3C) ---

# name -> (oatgpu_config overrides, rate schedule, what the HSV / threshold window must do, kind of frames)
#   window "default": the usual window; "black": contains black (0,0,0) but not the shadows' colours; "shadow": contains the
#   shadows' colours but not black -- only where a shadow pixel is zeroed or not can the threshold tell
PARAM_GRID = {
    "nmix1": (dict(nmixtures=1), "rate", "default", "shadow"),
    "nmix2": (dict(nmixtures=2), "rate", "default", "shadow"),
    "nmix4": (dict(nmixtures=4), "rate", "default", "shadow"),
    "nmix2-shrink": (dict(nmixtures=2, mog_restore_nmodes=0), "rate", "default", "shadow"),
    "no-shadows": (dict(detect_shadows=0), "rate", "default", "shadow"),
    "shadow0-black": (dict(shadow_value=0), "rate", "black", "shadow"),
    "shadow0-noblack": (dict(shadow_value=0), "rate", "shadow", "shadow"),
    "shadow200": (dict(shadow_value=200), "rate", "default", "shadow"),
    "tau0.2": (dict(tau=0.2), "rate", "default", "shadow"),
    "tau0.95": (dict(tau=0.95), "rate", "default", "shadow"),
    "tg20-tb2": (dict(var_threshold=2.0, var_threshold_gen=20.0), "fast", "default", "two_level"),
    "tg20-tb2-shadow0": (dict(var_threshold=2.0, var_threshold_gen=20.0, shadow_value=0), "fast", "shadow", "two_level"),
    "bgratio0.3": (dict(background_ratio=0.3), "rate", "default", "shadow"),
    "bgratio1.0": (dict(background_ratio=1.0), "rate", "default", "shadow"),
    "varinit-outside": (dict(var_init=100.0), "rate-then-0", "default", "shadow"),
    "varmin-eq-varmax": (dict(var_init=10.0, var_min=10.0, var_max=10.0), "rate-then-0", "default", "shadow"),
    "ct0.49": (dict(ct=0.49), "rate", "default", "shadow"),
    "history6": (dict(history=6), "auto", "default", "shadow"),
}
SHADOW_GRID = ("shadow0-black", "shadow0-noblack", "shadow200", "tau0.2", "tau0.95", "tg20-tb2-shadow0", "no-shadows")


FAST_RATE = 0.1


def grid_rate(schedule, t):
    if schedule == "auto":
        return -1.0
    if schedule == "fast":
        return FAST_RATE
    if schedule == "rate-then-0" and t >= WARM_FRAMES:
        return 0.0
    return WARM_RATE


def oracle_params(over):
    """oatgpu_config overrides -> the C oracle's parameter names."""
    m = dict(over)
    if "mog_restore_nmodes" in m:
        m["restore_nmodes"] = m.pop("mog_restore_nmodes")
    return m


# ------------------------------------------------------------------------------- a whole run, restated ---

@dataclass
class Step:
    frames: tuple                 # frame indices of the step (one, or two consecutive)
    wg: int                       # what oatgpu_last_step_shape reports for it
    launches: list                # instantiations of its per-pixel launches, in order
    nt_loads: bool                # the context's streaming-load flag while it was launched


def plan(channels, fusion, rates, dense_after, audit=False, wg_force=0, wg_after_switch=0, frozen_ok_=True, ring_depth=4,
         history=500, ct=0.05):
    """The steps the pipelined host-frame path (enqueue one frame set at a time, fusion `fusion`, streams sharing one rate
    schedule) launches for frames 0..len(rates)-1.  dense_after(t): whether the density probe launched behind the step
    that ends with frame t reads >= 2.5 live modes (the oracle's model after frame t, tests/test_mog_matrix_cpu.py).
    Assumes every probe's numbers have arrived when the next probe is launched (they have on small frames: a frame is
    collected only behind its step's probe)."""
    nf, nt, probes, prev = 0, False, 0, None
    force, total, steps, pend = wg_force, 0, [], None

    def run(job):
        nonlocal nf, nt, probes, prev, force, total
        wg = step_workgroup(force, nt)
        rs = []
        for t in job:
            fresh, nf, aT, pr = mog_begin(nf, rates[t], history, ct)
            rs.append((fresh, aT, pr))
        if paired(len(job), rs[0][0], rs[-1][0], audit, channels):
            ls = k1_launches(channels, [(rs[0][1], rs[0][2]), (rs[1][1], rs[1][2])], False, nt, frozen_ok_, False, audit, wg)
        else:
            ls = [i for f, aT, pr in rs for i in k1_launches(channels, [(aT, pr)], f, nt, frozen_ok_, False, audit, wg)]
        steps.append(Step(tuple(job), wg, ls, nt))
        for i in range(len(job)):
            if probe_at(total + i):
                if probes and prev is not None:
                    nt = prev
                prev = dense_after(job[-1])
                probes += 1
        total += len(job)
        if wg_after_switch and wg == 64 and not force:
            force = wg_after_switch

    fuse = may_fuse(fusion, ring_depth, audit, channels)
    for t in range(len(rates)):
        if pend is not None:
            job, pend = (pend, t), None
            run(job)
        elif fuse:
            pend = t
        else:
            run((t,))
    if pend is not None:
        run((pend,))
    return steps


def shapes_after_enqueue(steps, nframes):
    """oatgpu_last_step_shape's workgroup after each enqueue: the latest step launched so far (0 before the first)."""
    last = {s.frames[-1]: s.wg for s in steps}
    out, cur = [], 0
    for t in range(nframes):
        cur = last.get(t, cur)
        out.append(cur)
    return out
