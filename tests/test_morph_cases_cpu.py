"""The morphology case table (tests/morph_cases.py), on the CPU: its constants and route predicates against the kernel
sources, every edge geometry against the edge it is meant to straddle, the oracle against scipy's window filters on every
case, the closed-form results of the impulse / hole / probe cases -- and whether the cases DISCRIMINATE: for every case
the right result must differ from five wrong morphologies (mutant references below), or the GPU test that compares the
kernels with the oracle on these cases would pass a kernel with that very mistake."""
import functools
import os
import re

import numpy as np
from scipy import ndimage

import morph_cases as M
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oat_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _flat(s):
    return " ".join(s.split())


# ------------------------------------------------------------------------------------- the sources' constants ---

def test_constants_are_the_kernels():
    blob, api, hdr = _flat(_src("kernels_rowscan.hip")), _flat(_src("api_context.hip")), _flat(_src("oatgpu_internal.h"))
    assert re.search(r"constexpr int kRsWaves = \d+, kRsRows = (\d+);", blob).group(1) == str(M.RS_ROWS)
    m = re.search(r"constexpr size_t kRowscanLdsMax = (\d+) \* (\d+);", hdr)
    assert int(m.group(1)) * int(m.group(2)) == M.ROWSCAN_LDS_MAX
    # 64-pixel words, planes padded to 1024
    assert "g.Wp = (cfg->cols + 63) / 64 * 64; g.words = g.Wp / 64;" in api and M.WORD == 64
    assert "g.Palloc = (g.P + 1023) / 1024 * 1024;" in api and M.PLANE_ALIGN == 1024
    # 64-word chunks: both loops of k_rowscan
    assert blob.count("for (int c0 = 0; c0 < g.words; c0 += 64)") == 2 and M.CHUNK_WORDS == 64
    # k <= 63
    assert f"if (k.erode > {M.K_MAX} || k.dilate > {M.K_MAX})" in api
    assert M.SIZES[-1] == M.K_MAX and all(0 <= k <= M.K_MAX for k in M.SIZES)


def test_route_predicates_are_the_sources():
    blob, api = _flat(_src("kernels_rowscan.hip")), _flat(_src("api_track.hip"))
    markers, ctx = _flat(_src("api_markers.hip")), _flat(_src("oatgpu_ctx.h"))
    # rowscan_lds_bytes(): (kRsRows + max(dil, 1) - 1) rows of g.words 8-byte words
    assert "return (size_t)(kRsRows + (dil_k > 1 ? dil_k : 1) - 1) * g.words * sizeof(u64);" in blob
    assert M.rowscan_lds_bytes(12, 129, 0) == M.rowscan_lds_bytes(12, 129, 1) == 4 * 3 * 8
    assert M.rowscan_lds_bytes(12, 129, 5) == 8 * 3 * 8
    # plan_morph(): sizes of 0 and 1 do nothing; the erosion is apart when the fused form's LDS is over the budget
    assert "m.dil = dilate > 1 ? dilate : 0; m.ero = erode > 1 ? erode : 0; " \
           "m.ero_apart = m.ero && rowscan_lds_bytes(g, m.dil) > kRowscanLdsMax;" in api
    assert not M.ero_apart(12, 1 << 14, 1, 63) and M.ero_apart(12, 1 << 14, 2, 63)
    # the fused form is taken from an erosion of 2 on; the marker table and the pair need the LDS kernel's geometry
    assert "if (ero_k > 1) hipLaunchKernelGGL(k_rowscan<true>" in blob
    assert "mkp.table = g.H > 2 && g.H <= 16383 && g.W <= 16383 && rowscan_lds_bytes(g, max_dil) <= kRowscanLdsMax;" in markers
    assert "const bool lds_geom = g.H > 2 && g.H <= 16383 && g.W <= 16383;" in api
    # a two-frame step whose erosion is apart is not paired (no public call tells: the GPU file runs both sides alike)
    assert "p.paired = nj == 2 && !p.early && c->pair_back && c->lds_spec && !c->kal_on && lds_geom && !p.ero_apart;" in api
    assert re.search(r"size_t early_min_px = \d+;", ctx)
    assert not M.lds_able(2, 64) and M.lds_able(3, 64)
    # the row group's LDS rows and the shortcut's source rows, as group_rows() restates them
    assert "const int r0 = grp * ROWS - dk / 2;" in blob and "const int dk = dil_k > 1 ? dil_k : 1;" in blob
    assert "const int ya = max(r0 - ero_k / 2, 0), yb = min(r0 + (ROWS + dk - 1) - ero_k / 2 + ero_k - 1, g.H);" in blob
    for H, g, e, d in ((9, 0, 3, 2), (9, 2, 4, 4), (40, 3, 7, 9), (12, 1, 2, 63)):
        dk = max(d, 1)
        r0 = g * 4 - dk // 2
        assert M.group_rows(H, g, e, d) == (r0, r0 + 4 + dk - 2, max(r0 - e // 2, 0), min(r0 + (4 + dk - 1) - e // 2 + e - 1, H))


def test_edge_geometries_straddle_their_edges():
    geoms = M.geometries()
    # word edges: no padding / 1, 7, 63 valid bits in the last word; one, two, three words; one row group and more
    assert {(H, W) for H in M.WORD_H for W in M.WORD_W} <= set(geoms)
    assert {W % 64 for W in M.WORD_W} == {0, 1, 7, 63} and {M.words(W) for W in M.WORD_W} == {1, 2, 3}
    assert {-(-H // M.RS_ROWS) for H in M.WORD_H} == {1, 2, 3} and {H % M.RS_ROWS for H in M.WORD_H} == {0, 1, 2, 3}
    assert {M.lds_able(H, 64) for H in M.WORD_H} == {False, True}
    # Palloc-padded stream planes and unpadded ones
    assert all(H * M.words(W) * 64 < 1024 < M.palloc(H, W) + 1 for H in M.WORD_H for W in M.WORD_W if H * M.words(W) < 16)
    assert M.palloc(*M.CHUNK_GEOMS[0]) == M.CHUNK_GEOMS[0][0] * M.CHUNK_GEOMS[0][1]
    # chunk edge: 64 and 65 words
    assert [M.words(W) for _, W in M.CHUNK_GEOMS] == [64, 65] and set(M.CHUNK_GEOMS) <= set(geoms)
    # LDS budget edge: the first width fuses, one word more (one pixel more already) does not; an erosion of 1 never is apart
    for dil in M.LDS_DILS:
        fuse, word = M.lds_edge_widths(dil)
        assert not M.ero_apart(M.LDS_H, fuse, 2, dil) and M.ero_apart(M.LDS_H, fuse + 1, 2, dil) and M.ero_apart(M.LDS_H, word, 2, dil)
        assert M.rowscan_lds_bytes(M.LDS_H, fuse, dil) <= M.ROWSCAN_LDS_MAX < M.rowscan_lds_bytes(M.LDS_H, word, dil)
        assert M.words(word) == M.words(fuse) + 1 and word == fuse + 64
        for W in (fuse, word):
            on = {M.route(c.H, c.W, c.e, c.d) for c in geoms[(M.LDS_H, W)]}
            assert on == {"k_morph + dilate_word" if W != fuse else "erode_word + dilate_word_lds"}, (W, on)
    assert M.lds_edge_widths(63)[0] == 124 * 64 and M.lds_edge_widths(62)[0] == 126 * 64      # (the source's formula, by hand)


def test_table_covers_what_it_promises():
    C = M.CASES
    assert len({c.name for c in C}) == len(C) and 300 <= len(C) <= 600
    assert 24 <= len(M.PIPELINED) <= 72 and {(c.H, c.W, c.e, c.d) for c in M.PIPELINED} == set(M.PIPE_SETS)
    assert all(M.lds_able(H, W) for H, W, _, _ in M.PIPE_SETS)
    # paired back halves are not formed where the erosion is apart: the subset holds both sides
    assert {M.ero_apart(*s) for s in M.PIPE_SETS} == {False, True}
    sizes = {(c.e, c.d) for c in C}
    assert {(e, 0) for e in M.SIZES} | {(0, d) for d in M.SIZES} <= sizes
    assert {(2, 3), (3, 2), (2, 2), (4, 4), (32, 32), (63, 63), (1, 1)} <= sizes
    # every route at every geometry class it can occur in
    for cls in ("word", "chunk"):
        assert {M.route(c.H, c.W, c.e, c.d) for c in C if c.cls == cls} == {"copy", "dilate_word", "erode_word + dilate_word_lds"} - \
            ({"copy"} if cls == "chunk" else set())
    # windows that see only border: k > W, k > H, k >= 2 H, for the erosion and for the dilation
    for k in ("e", "d"):
        assert any(getattr(c, k) > c.W for c in C) and any(c.H < getattr(c, k) < 2 * c.H for c in C)
        assert any(getattr(c, k) >= 2 * c.H and getattr(c, k) >= 2 * c.W for c in C)
    # impulses: every x of the list at a three-word row, every y mod kRsRows, the four corners
    imp = [c for c in C if c.kind == "impulse" and (c.H, c.W) == (9, 129)]
    assert {c.arg[1] for c in imp} >= {0, 1, 62, 63, 64, 65, 127, 128}
    assert {c.arg[0] % M.RS_ROWS for c in imp} == set(range(M.RS_ROWS))
    assert {c.arg for c in C if c.kind == "impulse"} >= {(0, 0)}
    assert any(len(M.impulse_rects(c)) == 5 for c in imp)
    assert {c.arg[1] for c in C if c.kind == "impulse" and c.cls == "chunk"} >= {4095, 4096}
    # shortcut probes: first, inner and last group, a square row on the first / the last row of [ya, yb) and one outside
    pr = {(c.arg) for c in C if c.kind == "probe" and c.H == 9}
    assert pr >= {(g, w) for g in (0, 1, 2) for w in ("first_in", "last_in")}      # (but where the pixel would lie outside the frame)
    assert {w for _, w in pr} == {"first_in", "last_in", "first_out", "last_out"}
    for c in C:
        if c.kind != "probe":
            continue
        assert c.e > 1 and not M.ero_apart(c.H, c.W, c.e, c.d)
        rects = M.probe_rects(c)
        g, which = c.arg
        r0, L, ya, yb = M.group_rows(c.H, g % -(-c.H // M.RS_ROWS), c.e, c.d)
        if not rects:
            continue
        y0, y1 = rects[0][:2]
        inside = [y for y in range(y0, y1 + 1) if ya <= y < yb]
        if which.endswith("_out"):
            assert len(inside) == 1 and inside[0] == (ya if which == "first_out" else yb - 1), c.name
        else:
            assert len(inside) == y1 - y0 + 1 and (y0 == ya if which == "first_in" else y1 == yb - 1), c.name


def test_streams_differ_and_stream_two_is_set_where_stream_zero_is_empty():
    for c in M.CASES:
        s = [M.build(c, k) for k in range(3)]
        assert all(m.shape == (c.H, c.W) and m.dtype == np.uint8 and set(np.unique(m)) <= {0, 255} for m in s), c.name
        if (s[0] == 0).any():
            assert ((s[2] != 0) & (s[0] == 0)).any(), c.name
        else:
            assert (s[2] != s[0]).any(), c.name


# ---------------------------------------------------------------------------- references, right and wrong ---

def _filt(img, k, erosion, variant=None):
    """One stage with scipy's window filters (the formulation of tests/test_independent_crosscheck.py): window
    [x - k // 2, x - k // 2 + k - 1], outside the image 255 for the erosion and 0 for the dilation -- or one of the
    mutants: "anchor" (k - 1) / 2, "border" the other constant, "reflect" reflect-101, "shrunk" a window of k - 1."""
    if k <= 1:
        return img
    f = ndimage.minimum_filter if erosion else ndimage.maximum_filter
    cval = 255 if erosion else 0
    if variant == "anchor":
        return f(img, size=k, mode="constant", cval=cval, origin=-1 if k % 2 == 0 else 0)
    if variant == "border":
        return f(img, size=k, mode="constant", cval=255 - cval, origin=0)
    if variant == "reflect":
        return f(img, size=k, mode="mirror", origin=0)
    if variant == "shrunk":
        return f(img, size=k - 1, mode="constant", cval=cval, origin=0)
    return f(img, size=k, mode="constant", cval=cval, origin=0)


# mutant -> (variant of the erosion, variant of the dilation).  The anchor and the window are properties of one function
# (erode_word, dilate_word, dilate_word_lds and k_morph each have their own), so each stage is wrong on its own: both at
# once would cancel on lone squares (k - 1 for both stages of sizes of opposite parity gives the right answer there).  The
# border rule is one rule of the whole operation.
MUTANTS = {"anchor (erosion)": ("anchor", None), "anchor (dilation)": (None, "anchor"),
           "erosion border 0": ("border", None), "dilation border 1": (None, "border"),
           "reflect-101 border": ("reflect", "reflect"),
           "window k - 1 (erosion)": ("shrunk", None), "window k - 1 (dilation)": (None, "shrunk")}


def _morph(img, e, d, variants=(None, None)):
    return _filt(_filt(img, e, True, variants[0]), d, False, variants[1])


def _interval(N, p, k, variant):
    """What index p of one stage reads along an axis of N pixels: (lo, hi) inside the image, and whether the window
    reaches outside it."""
    a, kk = k // 2, k
    if variant == "anchor":
        a = (k - 1) // 2
    if variant == "shrunk":
        kk, a = k - 1, (k - 1) // 2
    lo, hi = p - a, p - a + kk - 1
    out = lo < 0 or hi > N - 1
    if variant == "reflect" and out and N > 1:
        per = 2 * (N - 1)
        idx = [i % per if i % per < N else per - i % per for i in range(lo, hi + 1)]
        return (min(idx), max(idx)), out            # (a reflected window is still a run of pixels)
    return (max(lo, 0), min(hi, N - 1)), out


@functools.lru_cache(maxsize=None)
def _family(N, e, d, ve, vd):
    """erode e -> dilate d along one axis as a monotone function of the pixels: for every output index (all of a short
    axis, both ends of a long one: away from the borders the operation is the same at every index) the minimal runs of
    pixels that, all set, set it -- or True where the dilation's border value alone does."""
    fam = []
    near = 2 * (e + d) + 4
    for q in (range(N) if N <= 2 * near else list(range(near)) + list(range(N - near, N))):
        if d > 1:
            (plo, phi), out = _interval(N, q, d, vd)
            if vd == "border" and out:
                fam.append(True)
                continue
        else:
            plo = phi = q
        terms = set()
        for p in range(plo, phi + 1):
            if e > 1:
                t, out = _interval(N, p, e, ve)
                if ve == "border" and out:
                    continue                         # (this pixel never survives)
                terms.add(t)
            else:
                terms.add((p, p))
        keep, least = [], None                       # minimal runs: those that hold no other one
        for lo, hi in sorted(terms, key=lambda t: (-t[0], t[1])):
            if least is None or hi < least:
                keep.append((lo, hi))
                least = hi
        fam.append(frozenset(keep))
    return tuple(fam)


def _exempt(c, variants):
    """The geometry and the sizes alone make this form of a mutant the right operation: along both axes it is the same
    function of the pixels (odd k for the anchor, e <= 1 for the erosion's border, an axis every window covers, a reflected
    border behind an odd erosion whose survivors it cannot tell from the right one's, ...)."""
    ve, vd = variants
    return all(_family(N, c.e, c.d, ve, vd) == _family(N, c.e, c.d, None, None) for N in (c.H, c.W))


@functools.lru_cache(maxsize=None)
def _right(name):
    c = M.BY_NAME[name]
    return _morph(M.build(c), c.e, c.d)


def test_oracle_equals_scipy_window_filters_on_every_case_and_stream():
    for c in M.CASES:
        for s in range(3):
            img = M.build(c, s)
            want = _right(c.name) if s == 0 else _morph(img, c.e, c.d)
            got = O.dilate(O.erode(img, c.e) if c.e else img, c.d) if c.d else (O.erode(img, c.e) if c.e else img)
            assert (got == want).all(), (c.name, s)
            if c.e and c.d:                                   # each stage on its own too
                assert (O.erode(img, c.e) == _filt(img, c.e, True)).all(), (c.name, s)


def test_closed_form_results_and_no_trivial_ones():
    for c in M.CASES:
        want = _right(c.name)
        pred = M.predicted(c)
        if pred is not None:
            assert (pred == want).all(), c.name
        if c.kind == "probe":
            # one pixel survives the erosion where the square is whole (clipped only by the frame), and dilates to d x d
            rects = M.probe_rects(c)
            n = 0
            for y0, y1, x0, x1 in rects:
                ys = M.dilate_1d(c.H, M.erode_1d(c.H, y0, y1, c.e), c.d)
                xs = M.dilate_1d(c.W, M.erode_1d(c.W, x0, x1, c.e), c.d)
                n += len(ys) * len(xs)
            assert int((want != 0).sum()) == n, c.name
            if rects and c.arg[1].endswith("_in") and c.H >= c.e:
                assert n > 0, c.name
            continue
        k = max(c.e, c.d)
        if k <= c.H and k <= c.W and (c.H, c.W) != (1, 1):
            assert want.any() and not want.all(), c.name


def test_cases_tell_every_mutant_apart():
    """>= 90 % of the cases a mutant applies to, and at least one case of every geometry class, give another result under
    the mutant than under the right operation.  The figures are printed."""
    for mutant, v in MUTANTS.items():
        told = {cls: [0, 0] for cls in ("word", "chunk", "lds")}
        missed = []
        for c in M.CASES:
            wrong = _morph(M.build(c), c.e, c.d, v)
            if _exempt(c, v):
                assert (wrong == _right(c.name)).all(), (mutant, c.name)
                continue
            differs = bool((wrong != _right(c.name)).any())
            told[c.cls][0] += differs
            told[c.cls][1] += 1
            if not differs:
                missed.append(c.name)
        hit, of = sum(t[0] for t in told.values()), sum(t[1] for t in told.values())
        print(f"{mutant}: told apart by {hit} of {of} cases it applies to ({100 * hit / of:.1f} %); by class {told}; not by {missed}")
        assert of >= 100 and hit >= 0.9 * of, (mutant, hit, of, missed)
        assert all(t[0] > 0 for t in told.values()), (mutant, told)
