"""What the blob stage's single-workgroup kernel (k_blob_lds, oat_amd/csrc/kernels_bloblds.hip) counts on a final mask,
restated in numpy, and masks that land exactly on a requested count.

The final mask is the threshold mask after erode / dilate with the image frame zeroed, as O.sift_contours sees it.
The counts are the kernel's:
  * k_rowscan's rowinfo: the run count of a row that holds foreground, else 0.  A run starts at x = 0 and wherever
    the pixel value changes; with columns 0 and W-1 zeroed a dirty row holds 2 * fg_runs + 1 runs;
  * D = dirty rows, R = runs of the dirty rows, NF = (R - D) / 2 foreground runs (phase A, phase E);
  * NR = 8-connected foreground components, those inside holes included (phase D gives each an accumulator slot).
k_blob_lds takes a frame only when H > 2, H <= 16383, W <= 16383, D <= LDS_ROWS, R <= LDS_RUNS and NR <= LDS_ROOTS; the
global union-find (k_merge + k_green_select) takes every other frame.

The limits below are the kernel's constants; tests/test_blob_limits_cpu.py reads them out of the sources and fails when
the two disagree, so the GPU edge cases cannot drift away from the edges they are meant to straddle.
"""
import numpy as np

LDS_ROWS, LDS_RUNS, LDS_ROOTS = 1024, 3072, 768      # kLdsRows, kLdsRuns, kLdsRoots
LDS_BLOCK, LDS_TRIP = 1024, 8                        # kLdsBlock, kLdsTrip (words a thread has in flight per phase-B trip)
GEOM_MAX = 16383                                     # lds_able / lds_geom: H <= 16383 and W <= 16383
ROWSCAN_CHUNK_PX = 64 * 64                           # k_rowscan: one lane per word, 64-word chunks
PHASE_A_ROWS = 4                                     # phase A keeps row counts in registers while a thread owns <= 4 rows


def frame_zeroed(mask):
    """0/1 copy of mask with the image frame zeroed (cvStartFindContours in OpenCV 3.1, k_rowscan)."""
    m = (np.asarray(mask) != 0).astype(np.uint8)
    m[0, :] = 0
    m[-1, :] = 0
    m[:, 0] = 0
    m[:, -1] = 0
    return m


def _fg_runs(m):
    """(row, start, end) of every foreground run, end inclusive, in raster order."""
    H, W = m.shape
    p = np.zeros((H, W + 2), np.int8)
    p[:, 1:-1] = m
    d = np.diff(p, axis=1)
    ys, xs = np.nonzero(d == 1)
    ye, xe = np.nonzero(d == -1)
    return ys, xs, xe - 1


def _components(ys, xs, xe):
    """8-connected components over foreground runs: a run joins the runs of the row above that it overlaps once
    widened by one pixel.  Plain union-find, run index = node."""
    n = len(ys)
    par = list(range(n))

    def find(i):
        while par[i] != i:
            par[i] = par[par[i]]
            i = par[i]
        return i
    starts = np.searchsorted(ys, np.arange(ys[-1] + 2)) if n else np.zeros(1, np.int64)
    for i in range(n):
        y = ys[i]
        if y == 0:
            continue
        j, je = starts[y - 1], starts[y]
        # runs of a row are sorted by x: skip those that end left of this one's widened extent
        j = j + np.searchsorted(xe[j:je], xs[i] - 1)
        while j < je and xs[j] <= xe[i] + 1:
            a, b = find(i), find(j)
            if a != b:
                par[max(a, b)] = min(a, b)
            j += 1
    return len({find(i) for i in range(n)})


def run_counts(m):
    """(D, R) of a frame-zeroed 0/1 mask: dirty rows and the runs of the dirty rows, as k_rowscan's rowinfo counts them."""
    trans = np.count_nonzero(m[:, 1:] != m[:, :-1], axis=1)
    dirty = m.any(axis=1)
    return int(dirty.sum()), int(np.where(dirty, 1 + trans, 0).sum())


def over_run_capacity(final):
    """k_blob_lds declines this mask for its rows or runs alone (D > LDS_ROWS or R > LDS_RUNS): the cheap half of
    blob_load()'s verdict, without the component count -- for callers that ask once a frame at full size."""
    D, R = run_counts(frame_zeroed(final))
    return D > LDS_ROWS or R > LDS_RUNS


def blob_load(final):
    """Counts and branch choices of k_blob_lds for one final mask (frame zeroed here again; idempotent)."""
    m = frame_zeroed(final)
    H, W = m.shape
    words = (W + 63) // 64
    D, R = run_counts(m)
    NF = (R - D) // 2
    ys, xs, xe = _fg_runs(m)
    assert len(ys) == NF, "a dirty row holds 2 * fg_runs + 1 runs"
    NR = _components(ys, xs, xe)
    geom = H > 2 and H <= GEOM_MAX and W <= GEOM_MAX
    lds = geom and D <= LDS_ROWS and R <= LDS_RUNS and NR <= LDS_ROOTS
    lanes = 16 if NF * 16 <= LDS_BLOCK else (8 if NF * 8 <= LDS_BLOCK else 4)
    per = -(-H // LDS_BLOCK)
    return dict(D=D, R=R, NF=NF, NR=NR, path="lds" if lds else "global", lanes=lanes,
                passes=-(-NF // (LDS_BLOCK // lanes)), phase_a="registers" if per <= PHASE_A_ROWS else "loop",
                trips=-(-(D * words) // (LDS_TRIP * LDS_BLOCK)), chunks=-(-W // ROWSCAN_CHUNK_PX))


# ------------------------------------------------------------------------------------------------ constructors ---
# Each paints 1s into a 0/1 uint8 mask, never on the image frame, and returns the first row below what it painted
# plus one blank row, so that constructions stacked with it stay separate components.

def paint_comb(m, y0, R, k=16, x0=2, rw=2, gap=2):
    """Exactly R runs: D consecutive dirty rows with f_i foreground runs each, sum(2 f_i + 1) = R, f_i non-increasing,
    f_i <= k.  Run j of every row sits at the same x, so column j is one component: NR = f_0 = ceil(NF / D)."""
    D = 1 if R % 2 else 2
    while (R - D) // 2 > k * D:
        D += 2
    assert 3 * D <= R, "R too small for a comb"
    NF = (R - D) // 2
    f = [NF // D + (1 if i < NF % D else 0) for i in range(D)]
    for i, fi in enumerate(f):
        for j in range(fi):
            x = x0 + j * (rw + gap)
            m[y0 + i, x:x + rw] = 1
    assert x0 + f[0] * (rw + gap) < m.shape[1] - 1
    return y0 + D + 1


def paint_dashes(m, y0, n, x0=2, widths=(1, 3), gap=2):
    """n one-row components (single pixels and one-pixel lines, area 0), a row of them every other row."""
    W = m.shape[1]
    y, x, i = y0, x0, 0
    while i < n:
        w = widths[i % len(widths)]
        if x + w >= W - 1:
            y, x = y + 2, x0
            continue
        m[y, x:x + w] = 1
        x += w + gap
        i += 1
    return y + 2


def paint_squares(m, y0, n, size=2, x0=2, gap=2, rows_of=None):
    """n size x size squares (equal areas), a band of them every size + 1 rows (rows_of: at most that many a band)."""
    W = m.shape[1]
    y, x, i, inband = y0, x0, 0, 0
    while i < n:
        if x + size >= W - 1 or (rows_of and inband == rows_of):
            y, x, inband = y + size + 1, x0, 0
            continue
        m[y:y + size, x:x + size] = 1
        x += size + gap
        i += 1
        inband += 1
    return y + size + 1


def paint_jagged(m, y0, n, w0=70, x0=5, gap=9):
    """n three-row blobs, three runs each, of widths w0 + b (distinct areas), rows of different extents at offsets that
    cross 64-bit words differently: every lane share of phase E meets left / right / top / bottom border bits."""
    W = m.shape[1]
    y, x = y0, x0
    for b in range(n):
        w = w0 + b
        if x + w + 4 + gap >= W - 1:
            y, x = y + 4, x0
        m[y, x + 2:x + w - 1] = 1
        m[y + 1, x:x + w + 3] = 1
        m[y + 2, x + 5:x + w - 5] = 1
        x += w + 4 + gap + (b % 7)
    return y + 4


def paint_bar(m, y0, h, x=3, w=4):
    """A w-wide bar over h rows: h dirty rows, one run each."""
    m[y0:y0 + h, x:x + w] = 1
    return y0 + h + 1


def paint_rect(m, y0, y1, x0, x1):
    m[y0:y1, x0:x1] = 1
    return y1 + 1


# ------------------------------------------------------------------------------------------------ the edge table ---
# name -> (H, W, erode, dilate, builder, expected counts).  The builder returns the RAW mask (0/1) that the detector is
# given; the final mask is the oracle's erode / dilate of it with the frame zeroed.

def _blank(H, W):
    return np.zeros((H, W), np.uint8)


def _runs_case(R):
    def build():
        m = _blank(120, 96)
        y = paint_comb(m, 2, R - 3, k=16)
        paint_rect(m, y, y + 1, 4, 40)                   # one more dirty row, one run: R exactly
        return m
    return build


def _roots_case(NR):
    def build():
        m = _blank(40, 1000)
        paint_rect(m, 2, 9, 3, 30)                       # the one real blob
        paint_dashes(m, 11, NR - 1, widths=(1, 3, 1, 6))  # zero-area contours: single pixels and one-pixel lines
        return m
    return build


def _bar_case(D):
    def build():
        m = _blank(D + 4, 16)
        paint_bar(m, 1, D, x=3, w=4)
        return m
    return build


def _nf_case(NF):
    def build():
        m = _blank(80, 1300)
        nb = NF // 3
        y = paint_jagged(m, 2, nb)
        paint_dashes(m, y, NF - 3 * nb, widths=(40,))
        return m
    return build


def _trips_case(D):
    def build():
        m = _blank(D + 8, 4096)                          # 64 words a row: D * 64 words against kLdsTrip * kLdsBlock
        paint_bar(m, 1, D, x=1990, w=110)                # across a word boundary
        paint_rect(m, 3, 9, 4000, 4095)                  # ... and up to the last pixel before the zeroed column
        return m
    return build


def _ties_case(H, W, NR, band):
    def build():
        m = _blank(H, W)
        y = paint_squares(m, 2, 300, size=2, rows_of=band)
        paint_dashes(m, y, NR - 300)
        return m
    return build


def _tall_case(H):
    def build():
        W = 24
        m = _blank(H, W)
        if H <= 3:
            m[1, 2:9] = 1
            return m
        paint_rect(m, 1, min(4, H - 1), 2, 7)
        for b in (1023, 1024, 4095, 4096, 4100, 16380):  # the stretches of rows the threads of phase A own
            if b + 3 < H - 1:
                paint_rect(m, b - 1, b + 2, 9, 13 + (b % 5))
        paint_rect(m, max(H - 5, 1), H - 1, 14, 22)      # down to the last row before the zeroed one
        return m
    return build


def _wide_case(W):
    def build():
        m = _blank(12, W)
        paint_rect(m, 1, 4, 1, 70)
        for i, c in enumerate(range(ROWSCAN_CHUNK_PX, W, ROWSCAN_CHUNK_PX)):   # across every 4096-px chunk boundary
            paint_rect(m, 2 + i % 3, 7 + i % 3, c - 40 - i, min(c + 41 + 3 * i, W - 1))
        paint_rect(m, 4, 11, W - 1 - 67, W - 1)          # the last word, up to the last pixel before the zeroed column
        return m
    return build


def edge_cases():
    """{name: (H, W, erode, dilate, builder, expected)}: every pair straddles one edge of k_blob_lds or k_rowscan."""
    c = {}
    for R in (LDS_RUNS - 1, LDS_RUNS, LDS_RUNS + 1):
        c[f"runs_{R}"] = (120, 96, 0, 0, _runs_case(R), dict(R=R, path="lds" if R <= LDS_RUNS else "global"))
    for NR in (LDS_ROOTS - 1, LDS_ROOTS, LDS_ROOTS + 1):
        c[f"roots_{NR}"] = (40, 1000, 0, 0, _roots_case(NR), dict(NR=NR, path="lds" if NR <= LDS_ROOTS else "global"))
    for D in (LDS_ROWS, LDS_ROWS + 1):
        c[f"rows_{D}"] = (D + 4, 16, 0, 0, _bar_case(D), dict(D=D, R=3 * D, path="lds" if D <= LDS_ROWS else "global"))
    for NF, lanes, passes in ((64, 16, 1), (65, 8, 1), (128, 8, 1), (129, 4, 1), (256, 4, 1), (257, 4, 2)):
        c[f"fgruns_{NF}"] = (80, 1300, 0, 0, _nf_case(NF), dict(NF=NF, lanes=lanes, passes=passes, path="lds"))
    per_trip = LDS_TRIP * LDS_BLOCK // 64
    for D, trips in ((per_trip - 7, 1), (per_trip, 1), (per_trip + 1, 2)):
        c[f"trips_{D}"] = (D + 8, 4096, 0, 0, _trips_case(D), dict(D=D, trips=trips, path="lds"))
    tall = PHASE_A_ROWS * LDS_BLOCK
    for H, path, mode in ((3, "lds", "registers"), (tall, "lds", "registers"), (tall + 1, "lds", "loop"),
                          (GEOM_MAX, "lds", "loop"), (2, "global", "registers"), (GEOM_MAX + 1, "global", "loop")):
        c[f"height_{H}"] = (H, 24, 0, 0, _tall_case(H), dict(path=path, phase_a=mode))
    for W, path in ((ROWSCAN_CHUNK_PX, "lds"), (ROWSCAN_CHUNK_PX + 1, "lds"), (2 * ROWSCAN_CHUNK_PX, "lds"),
                    (GEOM_MAX, "lds"), (GEOM_MAX + 1, "global"), (GEOM_MAX + 2, "global")):
        c[f"width_{W}"] = (12, W, 0, 0, _wide_case(W), dict(path=path, chunks=-(-W // ROWSCAN_CHUNK_PX)))
    # a morphology in front: single pixels dilated into 3 x 3 squares, the counts are the final mask's
    def dil_squares():
        m = _blank(40, 1000)
        n, y, x = 0, 3, 3
        while n < 300:
            m[y, x] = 1
            n += 1
            x += 4 + (n % 3 == 0)
            if x >= 996:
                y, x = y + 5, 3
        return m
    c["dilated_squares_300"] = (40, 1000, 0, 3, dil_squares, dict(NR=300, NF=900, path="lds"))
    # equal areas: hundreds of 2 x 2 squares beside zero-area dashes, at the root limit and one over it; the squares' first
    # pixels in one row, or in bands of seven (the last band shorter: the latest first pixel is not the largest x)
    for NR in (LDS_ROOTS, LDS_ROOTS + 1):
        for band, H, W in ((None, 40, 1300), (7, 160, 1000)):
            c[f"ties_{'row' if band is None else 'bands'}_{NR}"] = (H, W, 0, 0, _ties_case(H, W, NR, band),
                                                                    dict(NR=NR, path="lds" if NR <= LDS_ROOTS else "global"))
    return c


# the pipelined tests' frames: each stream's final mask is one of these (threshold mask = the painted pixels; erode 0,
# dilate 0), at the LDS kernel's capacity or one over it
PIPELINE_SHAPES = ((200, 360), (1080, 1920))


def pipeline_masks(H, W):
    """{kind: (mask, expected)} for one frame geometry."""
    def runs(R):
        m = _blank(H, W)
        y = paint_comb(m, 3, R - 3, k=16, x0=H % 7 + 2)
        paint_rect(m, y, y + 1, 5, 60)
        return m

    def roots(NR):
        m = _blank(H, W)
        paint_rect(m, 3, 12, 4, 41)
        paint_dashes(m, 14, NR - 1, widths=(1, 3, 1, 6))
        return m
    return {"runs_at": (runs(LDS_RUNS), dict(R=LDS_RUNS, path="lds")),
            "runs_over": (runs(LDS_RUNS + 1), dict(R=LDS_RUNS + 1, path="global")),
            "roots_at": (roots(LDS_ROOTS), dict(NR=LDS_ROOTS, path="lds")),
            "roots_over": (roots(LDS_ROOTS + 1), dict(NR=LDS_ROOTS + 1, path="global")),
            "empty": (_blank(H, W), dict(D=0, path="lds"))}
