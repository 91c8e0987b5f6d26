"""The per-pixel MOG2 kernel's instantiation matrix, on the CPU (tests/mog_matrix.py): the scenario table against the
k_mog_fused symbols of the built library, the launcher's rules as restated against the sources, every scenario's data
against the regime it is meant to produce on the C oracle, and the Python restatement of MOG2 (tests/golden/make_golden.py)
against the C oracle away from OpenCV's default parameters."""
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import mog_matrix as M
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oat_amd", "csrc")
LIB = os.path.join(ROOT, "oat_amd", "lib", "liboatgpu.so")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_hazard_check as H  # noqa: E402

READELF = os.path.join(os.path.dirname(H.OBJDUMP), "llvm-readelf")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _flat(s):
    return " ".join(s.split())


def _function(src, head):
    """The text of the function whose definition starts with `head`, up to its closing brace at column 0."""
    i = src.index(head)
    return src[i:src.index("\n}\n", i) + 2]


# ------------------------------------------------------------------------------------ the table and the binary ---

def _kernel_names():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-s", "-j4", "-C", ROOT, "oat_amd/lib/liboatgpu.so"])
    names = set()
    with tempfile.TemporaryDirectory() as tmp:
        for co in H.code_objects(LIB, tmp):
            txt = subprocess.run([READELF, "--notes", co], check=True, capture_output=True, text=True).stdout
            names.update(re.findall(r"\.name:\s+(\S*k_mog_fused\S*)", txt))
    return names


def table_mismatch(table, names):
    """-> (instantiations in the library the table lacks, table rows the library lacks, names that do not parse)."""
    got = {M.parse_mangled(n) for n in names}
    odd = sorted(n for n in names if M.parse_mangled(n) is None)
    got.discard(None)
    return sorted(got - set(table)), sorted(set(table) - got), odd


@pytest.mark.skipif(not (os.path.exists(H.OBJDUMP) and os.path.exists(READELF)), reason="llvm tools of ROCm not found")
def test_table_matches_the_binary():
    names = _kernel_names()
    assert len(names) == len(M.SCENARIOS) == 27, sorted(names)
    assert table_mismatch(M.INSTANTIATIONS, names) == ([], [], [])
    assert len({sc.id for sc in M.SCENARIOS}) == len(M.SCENARIOS)
    for n in names:                                                  # the id names the mangled arguments it stands for
        assert M.mangled(M.parse_mangled(n)) in n
    # the comparison itself notices a row too few and a kernel too many
    some = sorted(M.INSTANTIATIONS)[5]
    assert table_mismatch(M.INSTANTIATIONS - {some}, names)[0] == [some]
    fake = "_Z11k_mog_fusedILi1ELb0ELb1ELi2ELb1ELi64EEv4Geom9MogLaunchi"
    assert table_mismatch(M.INSTANTIATIONS, names | {fake})[0] == [(1, 0, 1, 2, 1, 64)]


def test_every_scenario_reaches_its_instantiation_by_the_restated_launcher():
    """The restated launcher, run over each scenario's schedule with its data's regime on the oracle, launches the row's
    instantiation; the workgroup by path is 256 on sparse models and switches to 64 on dense ones."""
    for sc in M.SCENARIOS:
        rates = [sc.rate(t) for t in range(sc.nframes)]
        dense = sc.data == "dense"
        steps = M.plan(sc.channels, sc.fusion, rates, lambda t: dense and t >= 5, audit=sc.audit, wg_force=sc.wg_force,
                       wg_after_switch=sc.wg_after_switch)
        got = [i for s in steps for i in s.launches]
        assert sc.inst in got, (sc.id, sorted(set(map(M.inst_id, got))))
        assert {i[0] for i in got} == {sc.channels} and {i[1] for i in got} == {int(sc.audit)}, sc.id
        assert sum(len(s.frames) for s in steps) == sc.nframes
        if dense:
            wgs = [s.wg for s in steps]
            k = wgs.index(64)
            assert set(wgs[:k]) == {256} and max(s.frames[-1] for s in steps[:k]) >= 16, (sc.id, wgs)
            assert set(wgs[k + 1:]) == ({sc.wg_after_switch} if sc.wg_after_switch else {64}), (sc.id, wgs)
        elif not sc.wg_force:
            assert {s.wg for s in steps} == {256}, sc.id


def test_restated_launcher_corner_cases():
    ok = M.frozen_ok()
    r = M.mog_begin(3, 0.02)[2:]
    z = M.mog_begin(3, 0.0)[2:]
    # a pair at rate 0 is frozen; a pair with one frame at a rate is not; a dense model never runs the frozen kernels
    assert M.k1_launches(3, [z, z], False, False, ok, False, False, 256) == [(3, 0, 0, 2, 1, 256)]
    assert M.k1_launches(3, [r, z], False, False, ok, False, False, 256) == [(3, 0, 0, 2, 0, 256)]
    assert M.k1_launches(1, [z, z], False, True, ok, False, False, 64) == [(1, 0, 1, 2, 0, 64)]
    # var_init outside [var_min, var_max]: rate 0 takes the learning kernels
    assert not M.frozen_ok(var_init=100.0) and M.frozen_ok(10.0, 10.0, 10.0) and not M.frozen_ok(1.0, 0.0, 5.0)
    assert M.k1_launches(3, [z], False, False, False, False, False, 64) == [(3, 0, 0, 1, 0, 64)]
    # a fresh frame at rate 0 is not frozen
    assert M.k1_launches(3, [z], True, False, ok, False, False, 256) == [(3, 0, 0, 1, 0, 256)]
    # outside the in-range division: one-frame audit launches of 256, a pair split in two
    tiny = M.mog_begin(3, 1e-14)[2:]
    assert M.k1_launches(3, [tiny, tiny], False, False, ok, False, False, 64) == [(3, 1, 0, 1, 0, 256)] * 2
    assert M.k1_launches(1, [r], False, True, ok, True, False, 64) == [(1, 1, 0, 1, 0, 256)]
    # the audit ignores the workgroup; GREY is never paired under it
    assert M.k1_launches(3, [r, r], False, False, ok, False, True, 64) == [(3, 1, 0, 2, 0, 256)]
    assert not M.paired(2, False, False, True, 1) and M.paired(2, False, False, True, 3)
    assert not M.may_fuse(2, 4, True, 1) and M.may_fuse(2, 4, True, 3) and not M.may_fuse(2, 1, False, 3)
    # rate 1.0 re-initialises every frame (a first frame's rate: 1/2): never paired
    f1, n1, a1, _ = M.mog_begin(7, 1.0)
    assert f1 and n1 == 1 and a1 == 0.5
    # history caps the automatic rate: 1/min(2n, history)
    assert [float(M.mog_begin(n, -1.0, history=6)[2]) for n in range(5)] == [np.float32(v) for v in (1 / 2, 1 / 4, 1 / 6, 1 / 6, 1 / 6)]
    assert M.rate_in_range(1.0, -0.05) and not M.rate_in_range(1.0, -0.6) and not M.rate_in_range(2.0 ** -41, 0.0)
    assert M.rate_in_range(0.0, 0.0) and not M.rate_in_range(0.02, 0.0)        # ct 0: prune 0 is below 2^-60
    assert [t for t in range(300) if M.probe_at(t)] == [8, 16, 32, 64, 128, 192, 256]


# ------------------------------------------------------------------------------- the rules, read from the sources ---

def test_density_switch_and_probe_schedule_are_the_sources():
    api = _flat(_function(_src("api_track.hip"), "static int launch_front("))
    assert "if ((t >= 8 && t < 64 && (t & (t - 1)) == 0) || (t >= 64 && (t & 63) == 0)) {" in api
    assert f"if (c->dens_probes && prev[1]) c->nt_loads = {M.DENSE_DEN}ull * prev[0] >= {M.DENSE_NUM}ull * prev[1];" in api
    assert "const unsigned *prev = c->dens.host() + 2 * (ds ^ 1);" in api           # the previous probe's numbers
    assert "c->launched_total += (unsigned long long)nj;" in api
    mog = _src("kernels_mog.hip")
    probe = _flat(_function(mog, "void launch_density_probe("))
    assert f"const size_t samples = {M.PROBE_SAMPLES};" in probe
    assert "const size_t stride = total > samples ? total / samples : 1;" in probe
    k = _flat(_function(mog, "__global__ __launch_bounds__(1024) void k_density_probe("))
    assert "for (size_t j = threadIdx.x; j * stride < total; j += 1024) {" in k
    assert "if (c & kCountMask) { live += 1u + (unsigned)__popc((c >> (kLiveShift + 1)) & 0xfu); n += 1; }" in k
    h = _src("oatgpu_internal.h")
    assert re.search(r"constexpr int kCountMask = (\d+);", h).group(1) == str(M.COUNT_MASK)
    assert re.search(r"constexpr int kLiveShift = (\d+);", h).group(1) == str(M.LIVE_SHIFT)
    # the counter byte's live hints, as counter_bytes restates them
    assert "if (k >= 1 && k < nnew && __float_as_uint(pm.w[k]) != 0u) newcnt |= 1 << (kLiveShift + k);" in _flat(mog)


def test_workgroup_pairing_and_frozen_rules_are_the_sources():
    api = _flat(_src("api_track.hip"))
    assert ("p.k1_wg = c->k1_wg_force ? c->k1_wg_force : (p.early || c->nt_loads || (lone && c->lone_plain && early_wanted "
            "&& step_px >= c->early_min_px)) ? 64 : 256;") in api
    assert ("const bool pair = nj == 2 && !rates[s0].fresh && !rates[(size_t)n + s0].fresh && "
            "!(c->audit_on && c->cfg.channels != 3);") in api
    assert ("const bool may_fuse = want_pair && c->cfg.ring_depth >= 2 && !(c->audit_on && c->cfg.channels != 3);") in api
    assert ("o.frozen_ok = c->cfg.var_min <= c->cfg.var_init && c->cfg.var_init <= c->cfg.var_max && c->cfg.var_min > 0.f;"
            in api)
    assert "const int lim = 2 * nf < c->cfg.history ? 2 * nf : c->cfg.history;" in api
    assert "const bool needToInitialize = nf == 0 || learningRate >= 1;" in api
    # the one density flag decides both the loads and the workgroup; the switch is read only there
    assert api.count("c->nt_loads =") == 1 and "a.nt_loads = c->nt_loads ? 1 : 0;" in api


def test_launcher_dispatch_is_the_sources():
    mog = _src("kernels_mog.hip")
    rr = _flat(_function(mog, "static bool rate_in_range("))
    assert "if (aT == 0.f) return true;" in rr
    assert "return aT >= 0x1p-40f && aT <= 1.f && -prune >= 0x1p-60f && -prune <= 0.5f * aT;" in rr
    assert M.RATE_MIN == 2.0 ** -40 and M.PRUNE_MIN == 2.0 ** -60
    fused = _flat(_function(mog, "void launch_mog_fused("))
    assert ("a.audit_frozen = (o.frozen_ok && !a.nt_loads && a.alphaT == 0.f && (a.frames2 ? a.alphaT2 == 0.f : !a.fresh)) "
            "? 1 : 0;") in fused
    assert ("const bool in_range = !o.wild_model && rate_in_range(a.alphaT, a.prune) && (!a.frames2 || "
            "rate_in_range(a.alphaT2, a.prune2));") in fused
    assert "launch_mog_pick(g, a1, first_stream, n_streams, st, nullptr, 256);" in fused
    assert "launch_mog_pick(g, a, first_stream, n_streams, st, stop, o.wg);" in fused
    ch = _flat(_function(mog, "static void launch_mog_ch("))
    assert "if constexpr (!AUDIT) { if (wg == 64) { launch_mog_wg<CH, AUDIT, NTLD, NF, FROZEN, 64>" in ch
    # launch_mog_pick, branch by branch: the condition chain and the instantiation each branch launches
    pick = _flat(_function(mog, "static void launch_mog_pick("))
    calls = re.findall(r"launch_mog_ch<(\d), (true|false), (true|false), (\d)(?:, (true))?>", pick)
    got = [(int(c), int(a == "true"), int(n == "true"), int(f), int(z == "true")) for c, a, n, f, z in calls]
    assert got == [(3, 1, 0, 2, 0), (1, 0, 1, 2, 0), (3, 0, 1, 2, 0), (1, 0, 0, 2, 1), (3, 0, 0, 2, 1), (1, 0, 0, 2, 0),
                   (3, 0, 0, 2, 0), (1, 1, 0, 1, 0), (3, 1, 0, 1, 0), (1, 0, 1, 1, 0), (3, 0, 1, 1, 0), (1, 0, 0, 1, 1),
                   (3, 0, 0, 1, 1), (1, 0, 0, 1, 0), (3, 0, 0, 1, 0)], got
    conds = re.findall(r"(if \(a\.frames2\)|if \(a\.audit\)|else if \(a\.nt_loads\)|else if \(a\.audit_frozen\)|"
                       r"else if \(a\.audit\))", pick)
    assert conds == ["if (a.frames2)", "if (a.audit)", "else if (a.nt_loads)", "else if (a.audit_frozen)", "else if (a.audit)",
                     "else if (a.nt_loads)", "else if (a.audit_frozen)"], conds
    # ... and the restatement picks the same for every combination
    for nf in (1, 2):
        for ch in (1, 3):
            for audit in (0, 1):
                for nt in (0, 1):
                    for fr in (0, 1):
                        want = ((3, 1, 0, 2, 0) if nf == 2 else (ch, 1, 0, 1, 0)) if audit else \
                            (ch, 0, 1, nf, 0) if nt else (ch, 0, 0, nf, fr)
                        assert M._pick(ch, nf, audit, nt, fr, 64)[:5] == want


# ------------------------------------------------------------------------------------- the regimes on the oracle ---

def _probe_means(kind, ch, rows, cols, nframes=33, over=None, rate=M.WARM_RATE, streams=2):
    fr = M.frames_of(kind, streams, rows, cols, ch, nframes)
    orcs = [O.Mog2(rows, cols, ch, params=over) for _ in range(streams)]
    means = {}
    for t, fs in enumerate(fr):
        for o, f in zip(orcs, fs):
            o.apply(f, rate if callable(rate) is False else rate(t))
        if M.probe_at(t):
            live, n = M.density_probe([M.counter_bytes(*o.state()[:2]) for o in orcs], rows, cols)
            means[t] = live / n
    return means


@pytest.mark.parametrize("ch", [3, 1])
@pytest.mark.parametrize("shape", [(40, 101), (48, 128)])
def test_dense_and_sparse_data_sit_far_from_the_switch(ch, shape):
    dense = _probe_means("dense", ch, *shape)
    sparse = _probe_means("sparse", ch, *shape)
    assert min(dense.values()) >= 4.0, dense
    assert max(sparse.values()) <= 1.5, sparse
    # the restated probe and a direct count agree on these frames (the lattice takes every counter byte)
    o = O.Mog2(*shape, ch)
    for f in M.frames_of("dense", 1, *shape, ch, 6):
        o.apply(f[0], M.WARM_RATE)
    nm, w = o.state()[:2]
    assert M.density_probe([M.counter_bytes(nm, w)], *shape) == (int(((w != 0).sum(1)).sum()), nm.size)


def test_density_probe_lattice_on_large_planes():
    """Beyond 16 384 counter bytes the probe samples a lattice: every stride-th byte of the padded planes."""
    rows, cols = 300, 200                              # Wp 256, Palloc 76 800 a stream
    c = np.zeros(rows * cols, np.uint8)
    c[::7] = 1 | (1 << (M.LIVE_SHIFT + 1))
    live, n = M.density_probe([c, c], rows, cols)
    plane = np.zeros(2 * 76800, np.uint8)
    for s in range(2):
        plane[s * 76800:s * 76800 + rows * 256].reshape(rows, 256)[:, :cols] = c.reshape(rows, cols)
    smp = plane[::plane.size // M.PROBE_SAMPLES]
    assert n == int((smp != 0).sum()) and live == 2 * n and n > 0


@pytest.mark.parametrize("ch", [3, 1])
def test_shadow_data_yields_shadows(ch):
    rows, cols = 40, 101
    fr = M.shadow_frames(1, rows, cols, ch, 12)
    o = O.Mog2(rows, cols, ch)
    hit = 0
    for t, fs in enumerate(fr):
        m = o.apply(fs[0], M.WARM_RATE)
        b = M.shadow_box(t, rows, cols)
        if b:
            y, x, h, w = b
            hit += int((m[y:y + h, x:x + w] == 127).sum())
    assert hit >= 200, hit


@pytest.mark.parametrize("ch", [3, 1])
@pytest.mark.parametrize("nmix", [1, 2, 4])
def test_nmixtures_cases_fill_and_replace_their_last_mode(ch, nmix):
    rows, cols = 40, 101
    fr = M.frames_of("shadow", 1, rows, cols, ch, 24)
    o = O.Mog2(rows, cols, ch, params=dict(nmixtures=nmix))
    full = replaced = 0
    for fs in fr:
        nm0 = o.state()[0]
        o.apply(fs[0], M.WARM_RATE)
        nm, w, v, mu = o.state()
        x = fs[0].reshape(rows * cols, ch).astype(np.float32)
        new = ((mu == x[:, None, :]).all(-1) & (v == np.float32(15.0))).any(1)     # a slot holds this frame's pixel anew
        full = max(full, int((nm == nmix).sum()))
        replaced += int((new & (nm0 == nmix) & (nm == nmix)).sum())
    assert full > rows * cols // 20 and replaced > 100, (full, replaced)


GRID_SHAPE = (40, 101)


@pytest.mark.parametrize("name", sorted(M.PARAM_GRID))
def test_parameter_grid_stays_below_the_density_switch(name):
    """The GPU parameter grid runs plain (and frozen) instantiations only: its data must stay clear of 2.5 live modes."""
    over, sched, _, kind = M.PARAM_GRID[name]
    for ch in (3, 1):
        means = _probe_means(kind, ch, *GRID_SHAPE, nframes=33, over=M.oracle_params(over),
                             rate=lambda t: M.grid_rate(sched, t))
        assert max(means.values()) <= 2.1, (name, ch, means)


@pytest.mark.parametrize("ch", [3, 1])
def test_two_level_data_fits_mode_0_without_being_background(ch):
    """tg20-tb2's frames: in the second frame of a pair (odd t), pixels that matched mode 0 as background in the first
    fit mode 0 without being background, are no shadow of mode 0, and the oracle marks them as shadows -- of mode 1: the
    two-frame kernel must have fetched mode 1's record for them in its first frame (want2, kernels_mog.hip)."""
    rows, cols = GRID_SHAPE
    over = M.oracle_params(M.PARAM_GRID["tg20-tb2"][0])
    tb, tg = np.float32(over["var_threshold"]), np.float32(over["var_threshold_gen"])
    tau, TB = np.float32(0.5), np.float32(0.9)                                  # OpenCV's, not overridden here
    o = O.Mog2(rows, cols, ch, params=over)
    hits = 0
    for t, fs in enumerate(M.two_level_frames(1, rows, cols, ch, 30, seed=17)):
        x = fs[0].reshape(rows * cols, ch).astype(np.float32)
        nm, w, v, mu = o.state()
        m = o.apply(fs[0], M.grid_rate("fast", t)).reshape(-1)
        if t >= 2 and t % 2 == 1:
            d2 = ((mu[:, 0] - x) ** 2).sum(1)
            fit_not_bg = (d2 < tg * v[:, 0]) & ~(d2 < tb * v[:, 0]) & (nm >= 2)
            num, den = (x * mu[:, 0]).sum(1), (mu[:, 0] ** 2).sum(1)
            a = num / np.where(den == 0, 1, den)
            shadow0 = (num <= den) & (num >= tau * den) & (((a[:, None] * mu[:, 0] - x) ** 2).sum(1) < tb * v[:, 0] * a * a)
            hits += int((fit_not_bg & ~shadow0 & (w[:, 0] <= TB) & (m == 127)).sum())
    assert hits >= 1000, hits


# ------------------------------------------------------------- the Python restatement off the default parameters ---

def _make_golden():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(ROOT, "tests", "golden", "make_golden.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    return G


RESTATED_GRID = {
    "defaults": {},
    "nmix1": dict(nmixtures=1), "nmix2": dict(nmixtures=2), "nmix4": dict(nmixtures=4),
    "nmix2-shrink": dict(nmixtures=2, restore_nmodes=0),
    "no-shadows": dict(detect_shadows=0), "shadow0": dict(shadow_value=0), "shadow200": dict(shadow_value=200),
    "tau0.2": dict(tau=0.2), "tau0.95": dict(tau=0.95),
    "tg20-tb6": dict(var_threshold=6.0, var_threshold_gen=20.0), "tg20-tb2": dict(var_threshold=2.0, var_threshold_gen=20.0),
    "bgratio0.3": dict(background_ratio=0.3), "bgratio1.0": dict(background_ratio=1.0),
    "varinit-outside": dict(var_init=100.0), "varmin-eq-varmax": dict(var_init=10.0, var_min=10.0, var_max=10.0),
    "ct0.49": dict(ct=0.49), "history6": dict(history=6),
}
_KW = dict(var_threshold="Tb", background_ratio="TB", var_threshold_gen="Tg", var_init="var_init", var_min="var_min",
           var_max="var_max", ct="ct", tau="tau", detect_shadows="detect_shadows", shadow_value="shadow_value",
           history="history", nmixtures="nmix", restore_nmodes="restore")


@pytest.mark.parametrize("name", sorted(RESTATED_GRID))
def test_restatement_against_the_c_oracle_off_the_defaults(name):
    """make_golden.mog2_pixel_trace with the parameters as keywords against oracle/mog2.c on random pixel histories --
    flicker between two colours, slow drift, shadows (0.7 x the pixel), outliers -- mask, count, weights, variances and
    means of every pixel and frame, bit for bit; automatic, fixed and rate-0 phases."""
    G = _make_golden()
    over = RESTATED_GRID[name]
    kw = {_KW[k]: (bool(v) if k in ("detect_shadows", "restore_nmodes") else v) for k, v in over.items()}
    rng = np.random.default_rng(sum(map(ord, name)))
    npx, nfr = 24, 36
    base = rng.integers(40, 220, (npx, 3))
    alt = rng.integers(0, 256, (npx, 3))
    frames = np.empty((nfr, npx, 3), np.uint8)
    for t in range(nfr):
        f = base + rng.integers(-6, 7, (npx, 3)) + (t // 9)
        flip = rng.random(npx) < 0.25
        f[flip] = alt[flip] + rng.integers(-3, 4, (int(flip.sum()), 3))
        shade = rng.random(npx) < 0.15
        f[shade] = (base[shade] * 0.7).astype(np.int64)
        wild = rng.random(npx) < 0.05
        f[wild] = rng.integers(0, 256, (int(wild.sum()), 3))
        frames[t] = np.clip(f, 0, 255)
    rates = [-1.0] * 8 + [0.3] * 6 + [0.02] * 14 + [0.0] * 8
    m = O.Mog2(1, npx, 3, params=over)
    got = []
    for t in range(nfr):
        mask = m.apply(frames[t].reshape(1, npx, 3), rates[t])
        nm, w, v, mu = m.state()
        got.append((mask[0].copy(), nm.copy(), w.copy(), v.copy(), mu.copy()))
    masks = set()
    for p in range(npx):
        tr = G.mog2_pixel_trace([tuple(int(c) for c in frames[t, p]) for t in range(nfr)], rates, **kw)
        for t, want in enumerate(tr):
            mask, nm, w, v, mu = got[t]
            k = want["nmodes"]
            assert int(mask[p]) == want["mask"] and int(nm[p]) == k, (p, t)
            # (a NaN equals a NaN: a pruned slot matched again at rate 0 has k = 0 / 0, on both sides)
            assert np.array_equal(w[p, :k], np.float32(want["weight"]), equal_nan=True), (p, t)
            assert np.array_equal(v[p, :k], np.float32(want["variance"]), equal_nan=True), (p, t)
            assert np.array_equal(mu[p, :k], np.float32(want["mean"]).reshape(k, 3), equal_nan=True), (p, t)
            masks.add(want["mask"])
    counts = np.stack([g[1] for g in got])
    nmix = over.get("nmixtures", 5)
    assert counts.max() == nmix
    shadow = over.get("shadow_value", 127) if over.get("detect_shadows", 1) else None
    assert 255 in masks and 0 in masks
    if shadow is not None and name not in ("tau0.95",):
        assert shadow in masks, (name, masks)             # the histories really met the shadow test's outcome
    if shadow is None:
        assert masks <= {0, 255}


def test_restatement_defaults_are_the_oracles():
    """The keywords' defaults are OpenCV's, as the C oracle's defaults are."""
    G = _make_golden()
    import inspect
    d = {k: v.default for k, v in inspect.signature(G.mog2_pixel_trace).parameters.items() if v.default is not inspect._empty}
    p = O.Mog2Params()
    O.lib.oat_mog2_default_params(p)
    for k, kw in _KW.items():
        want = getattr(p, k)
        if k == "shadow_value":
            want = int(want)
        assert np.float32(d[kw]) == np.float32(want), (k, d[kw], want)
