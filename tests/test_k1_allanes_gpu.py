"""What all 64 lanes of a wave of the per-pixel MOG2 kernel execute, against the C oracle (tests/oracle_lib.py), bit for bit:

* the pixel fetch -- one unaligned 32-bit load a pixel in the two-frame default-policy BGR kernel -- at widths round the
  64-pixel tile, on frames at every byte alignment, with different garbage round the frames;
* the quotient alphaT / weight at mode 0's fit site on imported weights that are, are next to, and are far from the weight
  a settled single-mode pixel holds (1.0f, and the W = (alpha1 * 1.0f + prune) + alphaT it becomes), whole waves and
  mixtures, at three rates and on the automatic rate schedule -- the cases a shortcut for the settled weight would have to
  get right (measured and not adopted, LABNOTES; the fit site runs on every lane since, fitting or not);
* the load predicates of slots 1..4 -- every mode count crossed with every pattern of live slots an import can produce, on
  lanes that match mode 0, lanes that do not, and lanes that match it in the first frame of a launch only."""
import numpy as np
import pytest

import oracle_lib as O
from parity_asserts import _same_detection, _same_state

pytestmark = pytest.mark.gpu

F = np.float32
CT = F(0.05)
AREA = (2.0, 1e9)
WIN = dict(h=(20, 150), s=(30, 256), v=(40, 256))          # a window all three channels of a pixel decide
TAP_THRESHOLD = 0


@pytest.fixture(scope="module")
def A():
    import oat_amd
    return oat_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _context(A, rows, cols, n, fusion, ring=8):
    hp = A.HotPath(rows, cols, n_streams=n, ring_depth=ring, erode=0, dilate=0, area=AREA, h_thresh=WIN["h"],
                   s_thresh=WIN["s"], v_thresh=WIN["v"])
    hp.set_fusion(fusion)
    return hp


def _hsv_params():
    return O.hsv_params(erode=0, dilate=0, min_area=AREA[0], max_area=AREA[1], h_lo=WIN["h"][0], h_hi=WIN["h"][1],
                        s_lo=WIN["s"][0], s_hi=WIN["s"][1], v_lo=WIN["v"][0], v_hi=WIN["v"][1])


def _state_bytes(st):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in st[:4])


# ------------------------------------------------------------------------------------------------- pixel fetch ---

NFETCH = 5                                  # frame 0 re-initialises (rate 1, never paired); 1..4 are two pairs under fusion 2
FETCH_RATES = [1.0, 0.05, 0.05, 0.05, 0.05]
_fetch_ref = {}


def _fetch_frames(rows, cols, n):
    rng = np.random.default_rng(1000 * rows + 10 * cols + n)
    base = rng.integers(0, 256, (n, rows, cols, 3)).astype(np.int16)
    out = []
    for t in range(NFETCH):
        f = np.clip(base + rng.integers(-6, 7, base.shape), 0, 255).astype(np.uint8)
        jump = rng.random((n, rows, cols)) < 0.3                # pixels that leave the background: later modes, foreground
        f[jump] = rng.integers(0, 256, (int(jump.sum()), 3)).astype(np.uint8)
        out.append(f)
    return out


def _fetch_reference(rows, cols, n):
    """frames, and the oracle's (detections, last threshold image, final model) of every stream: computed once a shape"""
    key = (rows, cols, n)
    if key not in _fetch_ref:
        frames, p = _fetch_frames(rows, cols, n), _hsv_params()
        per = []
        for s in range(n):
            orc, dets, thr = O.Mog2(rows, cols, 3), [], None
            for t in range(NFETCH):
                want, thr = O.chain_step(orc, frames[t][s], FETCH_RATES[t], p)
                dets.append(want)
            per.append((dets, thr.copy(), orc.state()))
        _fetch_ref[key] = (frames, per)
    return _fetch_ref[key]


@pytest.mark.parametrize("fusion", [1, 2])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("cols", [1, 63, 64, 65, 67, 130])
def test_pixel_fetch(A, torch, cols, rows, n, fusion):
    """Frames are views into a larger device tensor at byte offsets 0..3, with two different fillings of the bytes in front of
    and behind them: the results are the oracle's and do not depend on the filling.  (The bytes behind the last pixel lie
    inside this test's own tensor: it proves that the fourth byte of a load is ignored, not that the byte behind a caller's
    buffer is not read -- that is argued where the kernel branches on the wave's word index, kernels_mog.hip.)"""
    frames, per = _fetch_reference(rows, cols, n)
    nb = n * rows * cols * 3
    pad = 16
    pitch = (pad + 3 + nb + pad + 3) // 4 * 4
    hp = _context(A, rows, cols, n, fusion)
    seen = set()
    for off in range(4):
        for fill in (0xA5, None):
            if fill is None:
                host = np.random.default_rng(off + 17).integers(1, 256, (NFETCH, pitch)).astype(np.uint8)
            else:
                host = np.full((NFETCH, pitch), fill, np.uint8)
            for t in range(NFETCH):
                host[t, pad + off:pad + off + nb] = frames[t].reshape(-1)
            buf = torch.from_numpy(host).cuda()
            assert buf.data_ptr() % 4 == 0
            got = []
            for t in range(NFETCH):
                hp.learning_coeff_ = FETCH_RATES[t]
                hp.enqueue_dev(buf.data_ptr() + t * pitch + pad + off, keepalive=buf)
            for t in range(NFETCH):
                got.append(hp.collect())
            for s in range(n):
                dets, thr, state = per[s]
                for t in range(NFETCH):
                    _same_detection(got[t][s], dets[t], (off, fill, t, s))
                assert (hp.read_mask(TAP_THRESHOLD, s) == thr).all(), (off, fill, s)
                _same_state(hp.mog_state(s), state, (off, fill, s))
            seen.add(b"".join(_state_bytes(hp.mog_state(s)) for s in range(n)))
    assert len(seen) == 1
    hp.close()


# -------------------------------------------------------------------------------------------- settled quotient ---

def _rate(lr):
    aT = F(lr)
    return aT, F(1) - aT, F(-float(lr) * float(CT))


def _settled_w(lr):
    aT, a1, prune = _rate(lr)
    return F(F(F(a1 * F(1)) + prune) + aT)


ALPHA_DEFAULT = 0.01            # the benchmark's rate: 1.0f IS a fixed point of (decay, fit, renormalise)
ALPHA_NOT_FIXED = 0.006         # ... and here it is not: W * (1 / W) rounds to 1 - 2^-24 (checked below)


def test_the_named_rates_are_what_they_are_named_for():
    for lr, fixed in ((ALPHA_DEFAULT, True), (ALPHA_NOT_FIXED, False)):
        w = _settled_w(lr)
        assert (F(w * F(F(1) / w)) == F(1)) == fixed, (lr, w)


def _quotient_models(cols, lr):
    """{name: mode-0 weight of every pixel}: whole waves of each value, and mixtures inside a wave"""
    one = F(1)
    vals = [one, np.nextafter(one, F(0)), np.nextafter(one, F(2)), F(0.5), _settled_w(lr) if lr > 0 else F(0.75)]
    out = {f"all_{i}": np.full(cols, v, F) for i, v in enumerate(vals)}
    out["by_lane"] = np.array([vals[i % 5] for i in range(cols)], F)
    out["random"] = np.array(vals, F)[np.random.default_rng(3).integers(0, 5, cols)]
    lone = np.full(cols, one, F); lone[37 % cols] = vals[3]; lone[cols - 1] = vals[1]       # one or two lanes off the settled weight
    out["lone"] = lone
    if cols > 64:
        out["by_wave"] = np.where(np.arange(cols) < 64, one, vals[3]).astype(F)
    return out


@pytest.mark.parametrize("fusion", [1, 2])
@pytest.mark.parametrize("lr", [ALPHA_DEFAULT, ALPHA_NOT_FIXED, 0.0])
@pytest.mark.parametrize("cols", [64, 128])
def test_settled_quotient_on_imported_weights(A, cols, lr, fusion):
    rng = np.random.default_rng(cols + int(lr * 1000))
    base = rng.integers(30, 220, (1, cols, 3)).astype(np.int16)
    frames = []
    for t in range(3):
        f = np.clip(base + rng.integers(-3, 4, base.shape), 0, 255).astype(np.uint8)
        far = np.arange(cols) % 11 == 5 + t                     # a few lanes that do not fit mode 0: not in the fit site's mask
        f[0, far] = 255 - f[0, far]
        frames.append(f)
    hp, p = _context(A, 1, cols, 1, fusion), _hsv_params()
    orc = O.Mog2(1, cols, 3)
    hp.learning_coeff_ = lr
    hp.track([frames[0]]); O.chain_step(orc, frames[0], lr, p)              # (a first frame: geometry, frame counter)
    for name, w0 in _quotient_models(cols, lr).items():
        nm = np.ones(cols, np.uint8)
        w = np.zeros((cols, 5), F); w[:, 0] = w0
        v = np.zeros((cols, 5), F); v[:, 0] = 15.0
        m = np.zeros((cols, 5, 3), F); m[:, 0] = base.reshape(cols, 3)
        hp.set_mog_state(nm, w, v, m, 5)
        orc.set_state(nm, w, v, m, 5)
        for f in frames[1:]:
            hp.enqueue([f])
        got = [hp.collect() for _ in frames[1:]]
        for t, f in enumerate(frames[1:]):
            want, thr = O.chain_step(orc, f, lr, p)
            _same_detection(got[t][0], want, (name, t))
        assert (hp.read_mask(TAP_THRESHOLD, 0) == thr).all(), name
        _same_state(hp.mog_state(0), orc.state(), name)
    hp.close()


@pytest.mark.parametrize("cols", [64, 128])
def test_settled_quotient_on_the_automatic_schedule(A, cols):
    """A fresh context, twelve pipelined frames at the automatic rate 1 / min(2 n, history): the two frames of a launch carry
    different rates, each with its own W and K.  The whole model is the oracle's after every pair."""
    rng = np.random.default_rng(cols)
    base = rng.integers(30, 220, (1, cols, 3)).astype(np.int16)
    hp, p = _context(A, 1, cols, 1, 2), _hsv_params()
    orc = O.Mog2(1, cols, 3)
    hp.learning_coeff_ = -1.0
    for pair in range(6):
        fs = [np.clip(base + rng.integers(-3, 4, base.shape), 0, 255).astype(np.uint8) for _ in range(2)]
        for f in fs:
            hp.enqueue([f])
        got = [hp.collect() for _ in fs]
        for t, f in enumerate(fs):
            want, _ = O.chain_step(orc, f, -1.0, p)
            _same_detection(got[t][0], want, (pair, t))
        _same_state(hp.mog_state(0), orc.state(), pair)
    hp.close()


# ------------------------------------------------------------------------------------------ phase-2 predicates ---

def _predicate_model(nold):
    """One wave.  Lane = (pattern of live slots among 1..nold-1) x (kind): kind 0 matches mode 0 in both frames, 1 matches no
    live mode's mean but the LAST slot's (mode 0's when there is no other: then it is far from everything), 2 matches mode 0 in
    frame 1 only.  -> (nm, w, v, m, frame 1, frame 2)"""
    cols = 64
    npat = 1 << (nold - 1)
    nm = np.full(cols, nold, np.uint8)
    w = np.zeros((cols, 5), F); v = np.zeros((cols, 5), F); m = np.zeros((cols, 5, 3), F)
    f1 = np.zeros((1, cols, 3), np.uint8); f2 = np.zeros((1, cols, 3), np.uint8)
    for lane in range(cols):
        pat, kind = (lane // 3) % npat, lane % 3
        live = [0] + [k for k in range(1, nold) if (pat >> (k - 1)) & 1]
        for k in range(nold):                                   # a dead slot keeps its record, as a pruned mode does
            v[lane, k] = 15.0 + k
            m[lane, k] = (20 + 45 * k, 30 + 40 * k, 240 - 45 * k)
        rest = 0.4 / max(len(live) - 1, 1)
        for i, k in enumerate(live):
            w[lane, k] = 0.6 if k == 0 else rest - 0.01 * i     # descending, as the reference keeps them
        if len(live) == 1:
            w[lane, 0] = 1.0
        own = m[lane, 0].astype(np.uint8)
        other = m[lane, nold - 1].astype(np.uint8) if nold > 1 else np.array([250, 5, 128], np.uint8)
        f1[0, lane] = other if kind == 1 else own
        f2[0, lane] = own if kind == 0 else other
    return nm, w, v, m, f1, f2


@pytest.mark.parametrize("fusion", [1, 2])
@pytest.mark.parametrize("nold", [1, 2, 3, 4, 5])
def test_phase2_predicates(A, nold, fusion):
    nm, w, v, m, f1, f2 = _predicate_model(nold)
    if nold == 5:
        assert all(len({(lane // 3) % 16 for lane in range(64) if lane % 3 == k}) == 16 for k in range(3))   # every pattern, every kind
    hp, p = _context(A, 1, 64, 1, fusion), _hsv_params()
    orc = O.Mog2(1, 64, 3)
    lr = 0.01
    hp.learning_coeff_ = lr
    hp.track([f1]); O.chain_step(orc, f1, lr, p)
    hp.set_mog_state(nm, w, v, m, 5)
    orc.set_state(nm, w, v, m, 5)
    hp.enqueue([f1]); hp.enqueue([f2])
    got = [hp.collect(), hp.collect()]
    for t, f in enumerate((f1, f2)):
        want, thr = O.chain_step(orc, f, lr, p)
        _same_detection(got[t][0], want, (nold, t))
    assert (hp.read_mask(TAP_THRESHOLD, 0) == thr).all()
    gs, os_ = hp.mog_state(0), orc.state()
    assert (gs[0] == os_[0]).all()                              # the counter bytes, as exported
    _same_state(gs, os_, nold)
    # ... and once more from the model the kernel stored (its own live hints now, not the importer's)
    hp.enqueue([f2]); hp.enqueue([f1])
    hp.collect(); hp.collect()
    O.chain_step(orc, f2, lr, p); O.chain_step(orc, f1, lr, p)
    _same_state(hp.mog_state(0), orc.state(), (nold, "again"))
    hp.close()
