"""The case table of the bit-packed morphology (k_morph, erode_word / dilate_word / dilate_word_lds and k_rowscan in
oat_amd/csrc/kernels_rowscan.hip), shared by tests/test_morph_cases_cpu.py and tests/test_morph_routes_gpu.py.

The kernel's constants are held here once; the CPU file reads them out of the sources and fails when the two disagree.
rowscan_lds_bytes() and ero_apart() restate the sources' formulas (kernels_rowscan.hip, plan_morph in api_track.hip), and
every geometry "on an edge" is DERIVED from them:

  mechanism                                     one side                          other side
  --------------------------------------------  --------------------------------  ---------------------------------------
  last word's padding bits (valid_bits, vlast)  W = 64, 128 (no padding)          W = 1, 7, 63, 65, 129 (1..63 valid bits)
  one / two / three words a row (pw, cw, nw)    W <= 64                           W = 65, 128 | W = 129
  row group of kRsRows rows (r0, [ya, yb))      H = 1 .. 4 (one group)            H = 5 (group + 1 row), 9 (two + 1 row)
  the LDS kernel's geometry (H > 2)             H = 1, 2 (global union-find)      H >= 3
  Palloc padding of the stream planes           H * Wp < 1024 (H * words < 16)    9 x 4096: H * Wp = 36 * 1024, no padding
  64-word chunk of the row scan                 W = 64 * 64 (64 words)            W = 64 * 64 + 1 (65 words)
  LDS budget of the fused erosion (ero_apart)   widest W that fuses at dil 63/62  that W + one word (k_morph)
  anchor k / 2 of an even window                e, d in {2, 4, 32, 62} ...        ... beside {3, 31, 33, 63}
  window against the frame                      k <= min(H, W)                    k > W, k > H, k >= 2 H (only border)
  erosion shortcut (no bit in [ya, yb))         probes with a square row ON the   probes one row outside of it
                                                first / last row of the range

Inputs are 0 / 255 masks built from the case alone (no global random state): build(case, stream).
"""
from collections import namedtuple

import numpy as np

RS_ROWS = 4                       # kRsRows: image rows a row-scan workgroup takes
ROWSCAN_LDS_MAX = 64 * 1024       # kRowscanLdsMax
WORD = 64                         # pixels a mask word
CHUNK_WORDS = 64                  # words a row-scan chunk (one lane per word)
K_MAX = 63                        # largest erode / dilate size
PLANE_ALIGN = 1024                # Palloc = P rounded up to this

SIZES = (0, 1, 2, 3, 4, 31, 32, 33, 62, 63)


def words(W):
    return -(-W // WORD)


def palloc(H, W):
    P = H * words(W) * WORD
    return -(-P // PLANE_ALIGN) * PLANE_ALIGN


def rowscan_lds_bytes(H, W, dil):
    """kernels_rowscan.hip, rowscan_lds_bytes(): the eroded rows a workgroup's dilation windows touch, 8 bytes a word."""
    return (RS_ROWS + (dil if dil > 1 else 1) - 1) * words(W) * 8


def ero_apart(H, W, ero, dil):
    """api_track.hip, plan_morph(): the erosion is a k_morph launch of its own (sizes of 0 and 1 do nothing)."""
    ero, dil = (ero if ero > 1 else 0), (dil if dil > 1 else 0)
    return bool(ero) and rowscan_lds_bytes(H, W, dil) > ROWSCAN_LDS_MAX


def route(H, W, ero, dil):
    """Which code computes the rectangle on the single-stage and plain routes."""
    if ero > 1:
        return "k_morph + dilate_word" if ero_apart(H, W, ero, dil) else "erode_word + dilate_word_lds"
    return "dilate_word" if dil > 1 else "copy"


def lds_able(H, W):
    return 2 < H <= 16383 and W <= 16383


def lds_edge_widths(dil):
    """(widest W whose erosion still fuses at this dilation, that W + one word)."""
    w_max = ROWSCAN_LDS_MAX // ((RS_ROWS + dil - 1) * 8)
    return w_max * WORD, (w_max + 1) * WORD


def group_rows(H, g, ero, dil):
    """Row group g of the fused row scan: (r0, L, ya, yb) = first and last eroded row it keeps in LDS and the source-row
    range [ya, yb) its shortcut looks at (k_rowscan<true>)."""
    dk = dil if dil > 1 else 1
    r0 = g * RS_ROWS - dk // 2
    L = r0 + RS_ROWS + dk - 2
    a = ero // 2
    return r0, L, max(r0 - a, 0), min(L - a + ero, H)


# --------------------------------------------------------------------------------- the rectangle, in one dimension ---
# A third statement of the operation beside the oracle's and scipy's, on index sets: good for inputs made of rectangles
# that do not interact (impulses, holes, probes), whose result is then known in closed form.

def _win(p, k):
    a = k // 2
    return p - a, p - a + k - 1


def erode_1d(N, lo, hi, k):
    """Survivors of the set interval [lo, hi] (inclusive) under a window of k; outside [0, N) reads as set."""
    if k <= 1:
        return set(range(max(lo, 0), min(hi, N - 1) + 1))
    return {p for p in range(N) if max(_win(p, k)[0], 0) >= lo and min(_win(p, k)[1], N - 1) <= hi}


def dilate_1d(N, pts, k):
    if k <= 1 or not pts:
        return set(pts)
    return {q for q in range(N) if any(_win(q, k)[0] <= p <= _win(q, k)[1] for p in pts)}


def rect_result(H, W, rects, e, d):
    """erode e -> dilate d of a union of non-interacting rectangles (y0, y1, x0, x1), inclusive: 0 / 255 image."""
    out = np.zeros((H, W), np.uint8)
    for y0, y1, x0, x1 in rects:
        ys = dilate_1d(H, erode_1d(H, y0, y1, e), d)
        xs = dilate_1d(W, erode_1d(W, x0, x1, e), d)
        if ys and xs:
            out[np.ix_(sorted(ys), sorted(xs))] = 255
    return out


def hole_result(H, W, y, x, e, d):
    """erode e -> dilate d of a full frame with one zero pixel: the erosion opens the reflected window around it, the
    dilation closes what its own window bridges (outside the frame reads 0 for it, so the border never helps)."""
    a = e // 2
    zy = (max(y + a - e + 1, 0), min(y + a, H - 1)) if e > 1 else (y, y)
    zx = (max(x + a - e + 1, 0), min(x + a, W - 1)) if e > 1 else (x, x)
    out = np.full((H, W), 255, np.uint8)
    ys, xs = erode_1d(H, zy[0], zy[1], d), erode_1d(W, zx[0], zx[1], d)
    if ys and xs:
        out[np.ix_(sorted(ys), sorted(xs))] = 0
    return out


# ------------------------------------------------------------------------------------------------------ the inputs ---

Case = namedtuple("Case", "name cls H W e d kind arg pipelined")
# cls: "word" | "chunk" | "lds" (the geometry class); kind: "dense" | "impulse" | "hole" | "probe"
# arg: dense: seed; impulse / hole: (y, x) of the surviving / the zero pixel; probe: (group, which)


def _square(N, p, k):
    """The interval that erodes to exactly p (clipped to the frame: what lies outside reads as set)."""
    if k <= 1:
        return p, p
    lo, hi = _win(p, k)
    return max(lo, 0), min(hi, N - 1)


def _apart(r, s, gap):
    return r[0] - s[1] > gap or s[0] - r[1] > gap or r[2] - s[3] > gap or s[2] - r[3] > gap


def impulse_rects(c, stream=0):
    """The case's square -- the window of the pixel c.arg, clipped to the frame, so that this pixel survives the erosion --
    then more of the kind where they stay clear of it and of each other by more than e + d (no window then sees two of them,
    and rect_result() is the result): one in the middle of the frame (free of every border where the frame is large enough:
    what a window one too small changes), the corners, and one each on the top and on the left border.  Streams 1 and 2
    move the case's square to the mirrored position."""
    y, x = c.arg
    if stream == 1:
        x = c.W - 1 - x
    elif stream == 2:
        y, x = c.H - 1 - y, c.W - 1 - x
    rects = [_square(c.H, y, c.e) + _square(c.W, x, c.e)]
    # the top left one: an even erosion's square there is k / 2 wide and high, which is what a reflected border would get
    # wrong; without one, an even dilation's pixel sits k / 2 off both borders, for the same reason
    t = c.d // 2 if (c.e <= 1 or c.e % 2) and c.d > 1 and c.d % 2 == 0 else 0
    for cy, cx in ((c.H // 2, c.W // 2), (min(t, c.H - 1), min(t, c.W - 1)), (0, c.W - 1), (c.H - 1, 0), (c.H - 1, c.W - 1),
                   (min(t, c.H - 1), c.W // 2), (c.H // 2, min(t, c.W - 1))):
        r = _square(c.H, cy, c.e) + _square(c.W, cx, c.e)
        if all(_apart(r, s, c.e + c.d) for s in rects):
            rects.append(r)
    return rects


def probe_rects(c, stream=0):
    """One e x e square against the shortcut range [ya, yb) of row group g = c.arg[0] (fused erosion, e > 1):
      first_in  its FIRST row is row ya, it erodes to a pixel in the group's first eroded row r0 (first row of its LDS);
      last_in   its LAST row is row yb - 1, it erodes to a pixel in the group's last eroded row L;
      first_out its LAST row is row ya: one row inside the range, the pixel belongs to the rows above;
      last_out  its FIRST row is row yb - 1: one row inside, the pixel belongs to the rows below.
    Clipped to the frame where the range is (the frame's outside reads as set for the erosion).  (A range one row short at
    either end would still see e - 1 >= 1 rows of a square whose pixel lies in the group's rows: it shows only where the
    window is one row -- on one-row frames, and behind the table form's erosion of 1.  The probes pin where the range's ends
    are all the same.)  Streams 1 and 2 take the
    next groups (mod the number of groups) and another x."""
    g, which = c.arg
    groups = -(-c.H // RS_ROWS)
    g = (g + stream) % groups
    r0, L, ya, yb = group_rows(c.H, g, c.e, c.d)
    a = c.e // 2
    top = {"first_in": r0 - a, "last_in": L - a, "first_out": ya - c.e + 1, "last_out": yb - 1}[which]
    y0, y1 = max(top, 0), min(top + c.e - 1, c.H - 1)
    if y1 < y0:
        return []
    # stream 0: against the left border, clipped by it (what a wrong border value or a reflected border would change);
    # streams 1 and 2: across the first word edge
    px = 0 if stream == 0 else min(WORD - 2 + stream, c.W - 1)
    return [(y0, y1) + _square(c.W, px, c.e)]


def _paint(H, W, rects):
    m = np.zeros((H, W), np.uint8)
    for y0, y1, x0, x1 in rects:
        m[y0:y1 + 1, x0:x1 + 1] = 255
    return m


def _dense(c, stream):
    """A union of rectangles with pinholes, sized by the case.  The core rectangle, painted last, is e x e and a little more
    where the frame is (the erosion leaves something of it, a run of pixels, not one), free of the left and right borders
    more often than not (a window one too small shows on a free edge); the others are anywhere and carry the pinholes.  All keep to the left W - 1 - d / 2 columns, so that the
    dilation leaves the last column empty where the frame is wider than its window; every other seed and stream is
    mirrored, which puts the core on the right border (padding bits) and the free column on the left."""
    H, W, e, d = c.H, c.W, max(c.e, 1), max(c.d, 1)
    rng = np.random.default_rng(1000 * c.arg + 17 * stream + 3)
    m = np.zeros((H, W), np.uint8)
    room = W - 1 - d // 2 if W - 1 - d // 2 >= 1 else W

    def extra(N, most):
        return int(rng.integers(0, min(most, max(N - max(e, d) - 1, 0)) + 1))
    for i in range(int(rng.integers(1, 4))):
        h, w = min(H, int(rng.integers(1, e + 4))), min(room, int(rng.integers(1, e + 9)))
        y0, x0 = int(rng.integers(0, H - h + 1)), int(rng.integers(0, room - w + 1))
        m[y0:y0 + h, x0:x0 + w] = 255
        if h * w > 2:
            for _ in range(int(rng.integers(1, 3))):
                m[y0 + int(rng.integers(0, h)), x0 + int(rng.integers(0, w))] = 0
    def core(N, most):                                     # a window above the axis: all but the last pixel where the
        if e > N:                                          # window of pixel 0 ends before it, else the whole axis
            return N - 1 if (e + 1) // 2 <= N - 1 else N
        return e + extra(N, most)
    h, w = core(H, 2), min(room, core(W, 5))
    y0 = 0 if e > H or H < h + 2 else (0, H - h, int(rng.integers(1, H - h)), int(rng.integers(1, H - h)))[int(rng.integers(0, 4))]
    x0 = 0 if e > W or room < w + 2 or rng.random() < 0.3 else int(rng.integers(1, room - w))
    m[y0:y0 + h, x0:x0 + w] = 255
    if m.all() and max(e, d) <= min(H, W) and m.size > 1:
        m[-1, -1] = 0                                      # (a tiny frame the rectangles filled)
    m = m[:, ::-1].copy() if (c.arg + stream) % 2 else m
    _tab(m, c)
    return m


def _tab(m, c):
    """What a reflected (reflect-101) border would get wrong, put on the top border, or on the left one where the frame is
    not high enough.  Even erosion: a tab k / 2 pixels deep -- it survives on the border line only while the border reads
    as set, not as the pixel k / 2 in, which is cleared.  Otherwise, even dilation: a square that erodes to the pixel
    k / 2 off the border, with nothing between it and the border -- the border line must stay empty."""
    H, W = m.shape
    e, d = c.e, c.d
    if e > 1 and e % 2 == 0:
        a = e // 2
        if a < H:
            x0 = max((W - e - 1) // 2, 0)
            m[0:a, x0:x0 + e + 1] = 255
            m[a, x0:x0 + e + 1] = 0
        elif a < W:
            m[:, 0:a] = 255
            m[:, a] = 0
    elif d > 1 and d % 2 == 0 and d // 2 - max(e, 1) // 2 >= 1:
        ad, ae = d // 2, max(e, 1) // 2
        if ad < H:
            x0 = max((W - e - 1) // 2, 0)
            m[0:ad + ae + 2, max(x0 - d, 0):x0 + max(e, 1) + d] = 0
            m[ad - ae:ad + ae + 1, x0:x0 + max(e, 1)] = 255
        elif ad < W:
            m[:, 0:ad + ae + 2 + d] = 0
            m[:, ad - ae:ad + ae + 1] = 255


def _build(c, stream):
    if c.kind == "dense":
        return _dense(c, stream)
    if c.kind == "impulse":
        return _paint(c.H, c.W, impulse_rects(c, stream))
    if c.kind == "probe":
        return _paint(c.H, c.W, probe_rects(c, stream))
    y, x = c.arg                                           # hole; stream 2: the complement, a lone pixel
    m = np.full((c.H, c.W), 255, np.uint8)
    if stream == 1:
        x = c.W - 1 - x
    m[y, x] = 0
    return 255 - m if stream == 2 else m


def build(c, stream=0):
    """The 0 / 255 input of stream 0, 1 or 2 of a case.  Stream 2's is set somewhere stream 0's is empty (a full stream 0:
    differs from it), so that a stream read at another stream's offset cannot give the right answer."""
    m = _build(c, stream)
    if stream == 2:
        s0 = _build(c, 0)
        if not ((m != 0) & (s0 == 0)).any() and not ((s0 != 0).all() and (m != s0).any()):
            m = 255 - s0
    return m


def predicted(c):
    """Stream 0's result in closed form, or None (dense: the oracle and scipy are the statement)."""
    if c.kind == "impulse":
        return rect_result(c.H, c.W, impulse_rects(c), c.e, c.d)
    if c.kind == "probe":
        return rect_result(c.H, c.W, probe_rects(c), c.e, c.d)
    if c.kind == "hole":
        return hole_result(c.H, c.W, c.arg[0], c.arg[1], c.e, c.d)
    return None


# ------------------------------------------------------------------------------------------------------- the table ---

WORD_H = (1, 2, 3, 4, 5, 9)
WORD_W = (1, 7, 63, 64, 65, 128, 129)
CHUNK_GEOMS = ((9, CHUNK_WORDS * WORD), (9, CHUNK_WORDS * WORD + 1))
LDS_H = 12
LDS_DILS = (63, 62)

ERO_ONLY = tuple((e, 0) for e in SIZES if e)
DIL_ONLY = tuple((0, d) for d in SIZES if d)
# e < d, e > d, both even, both odd, both 63; small against large; k > W, k > H, k >= 2 H come with the geometries
PAIRS = ((1, 1), (2, 3), (3, 2), (2, 2), (2, 4), (4, 2), (3, 3), (3, 31), (31, 3), (32, 32), (4, 62), (62, 4), (33, 32),
         (31, 33), (2, 63), (63, 2), (32, 62), (62, 32), (33, 63), (63, 63))
ROTATED = ERO_ONLY + DIL_ONLY + PAIRS
IMPULSE_X = (0, 1, 62, 63, 64, 65, -2, -1, CHUNK_WORDS * WORD - 1, CHUNK_WORDS * WORD)      # negative: from W

# (H, W, e, d) of the pipelined routes (fused tracker, paired back half): LDS-able geometries, tiny Palloc-padded planes,
# every word shape, both sides of the LDS budget; each gets a dense, an impulse, a hole (e > 1, d <= e) and a probe (fused) case
PIPE_SETS = ((3, 65, 2, 3), (4, 7, 3, 2), (5, 129, 4, 4), (9, 63, 2, 2), (9, 64, 31, 33), (9, 129, 0, 63), (9, 128, 63, 0)) + \
    tuple((LDS_H, w, 3, 63) for w in lds_edge_widths(63))


def impulse_xs(W):
    return sorted({x % W if x < 0 else x for x in IMPULSE_X if -W <= x < W})


def _cases():
    out, seen = [], set()

    def add(cls, H, W, e, d, kind, arg):
        if kind == "hole" and (e <= 1 or d > e):           # (a dilation above the erosion closes the hole again)
            kind, arg = "dense", (arg[0] * 131 + arg[1]) % 997
        if kind == "probe" and (e <= 1 or ero_apart(H, W, e, d)):
            return
        if kind == "probe" and not rect_result(H, W, probe_rects(Case("", cls, H, W, e, d, kind, arg, False)), e, d).any():
            return                                         # (the square's pixel would lie outside the frame)
        if kind == "hole" and e % 2 and W > e + 2:          # an odd erosion's hole: free of the left and right borders, where a
            arg = (arg[0], W // 2)                         # window one too small opens it less
        if kind == "hole" and e % 2 == 0 and e // 2 < W:   # k / 2 off the left border: a reflected border would see it from x = 0;
            arg = (0, e // 2)                              # in row 0: the hole stays open on the border, where a dilation's border value shows
        name = f"{cls}-{H}x{W}-e{e}d{d}-{kind}-" + ("_".join(map(str, arg)) if isinstance(arg, tuple) else str(arg))
        if name in seen:
            return
        seen.add(name)
        out.append(Case(name, cls, H, W, e, d, kind, arg, (H, W, e, d) in PIPE_SETS))

    def pos(H, W, i):
        xs = impulse_xs(W)
        return i % H, xs[i % len(xs)]

    # word edges: two fixed cases a geometry (the even anchor on the fused form; e > d impulses), two or five rotated ones
    gi = 0
    for H in WORD_H:
        for W in WORD_W:
            if W > 1:
                add("word", H, W, 4, 4, "dense", gi)
            if W > 7:
                add("word", H, W, 3, 2, "impulse", pos(H, W, gi))
            for j in range(2 if W <= 7 else 5):            # (a frame of a few pixels tells few sizes apart: fewer there)
                e, d = ROTATED[((gi * 5 + j) * 7) % len(ROTATED)]
                kind = ("dense", "impulse", "hole")[(gi + j) % 3]
                add("word", H, W, e, d, kind, gi + 50 * j if kind == "dense" else pos(H, W, gi + 3 * j + 1))
            gi += 1
    add("word", 9, 129, 0, 0, "dense", 1)
    add("word", 1, 1, 0, 0, "dense", 2)
    # every impulse x, and every y mod kRsRows, at one three-word geometry: an odd pair, an even pair, e alone, d alone
    for i, x in enumerate(impulse_xs(129)):
        for e, d in ((3, 2), (4, 4), (2, 0), (0, 4)):
            add("word", 9, 129, e, d, "impulse", ((i + e) % 9, x))
    # the erosion shortcut: first, inner and last row group (H = 9: groups 0, 1, 2)
    for e, d in ((2, 3), (4, 2), (3, 0)):
        for g in (0, 1, 2):
            for which in ("first_in", "last_in", "first_out", "last_out"):
                add("word", 9, 129 if (e + g) % 2 else 65, e, d, "probe", (g, which))
    for e, d in ((4, 4), (2, 33), (3, 3)):
        for which in ("first_in", "last_in"):
            add("word", 9, 129, e, d, "probe", (1, which))
    # chunk edge
    for H, W in CHUNK_GEOMS:
        for k, (e, d) in enumerate(((4, 4), (0, 63), (63, 0), (33, 32), (2, 63), (3, 2))):
            add("chunk", H, W, e, d, "dense", 7 + k)
        for i, x in enumerate(impulse_xs(W)[2:]):
            e, d = ((3, 2), (4, 4), (2, 62), (31, 3))[i % 4]
            add("chunk", H, W, e, d, "impulse", (i % H, x))
        add("chunk", H, W, 32, 2, "hole", (4, CHUNK_WORDS * WORD - 1))
        add("chunk", H, W, 2, 3, "probe", (1, "last_in"))
    # LDS budget edge: the fused erosion on one side, k_morph on the other (e > 1 or the budget does not matter)
    for dil in LDS_DILS:
        for W in lds_edge_widths(dil):
            for k, e in enumerate((2, 3, 4, 31, 32, 33, 62, 63)):
                add("lds", LDS_H, W, e, dil, "dense", 11 + k)
            add("lds", LDS_H, W, 4, dil, "impulse", (5, W - 1))
            add("lds", LDS_H, W, 33, dil, "impulse", (11, WORD))
            add("lds", LDS_H, W, 62, dil, "hole", (6, W - 2))
    # the pipelined subset: every kind at every set
    for H, W, e, d in PIPE_SETS:
        cls = "lds" if H == LDS_H else "word"
        add(cls, H, W, e, d, "dense", 5)
        add(cls, H, W, e, d, "impulse", pos(H, W, 3))
        add(cls, H, W, e, d, "hole", (H // 2, W - 1))
        add(cls, H, W, e, d, "probe", (-(-H // RS_ROWS) - 1, "last_in"))
    return tuple(out)


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
PIPELINED = tuple(c for c in CASES if c.pipelined)


def geometries():
    """{(H, W): [cases]} in table order: the GPU file keeps one context a geometry."""
    g = {}
    for c in CASES:
        g.setdefault((c.H, c.W), []).append(c)
    return g
