"""Masks whose contours cross every seam of the blob kernels' shared border rule (oat_amd/csrc/blobedges_inline.h)
(TEST INFRASTRUCTURE, no GPU imports: tests/test_blob_seams_cpu.py checks on the masks alone that every listed position holds a
border pixel, tests/test_blob_seams_gpu.py runs them through k_blob_lds, k_green_select + k_blob_rank and k_blob_shape).

The rule is indexed by bit position in a 64-pixel mask word, and a thread of the global kernels owns a quarter of a word
(kGreenChunks = 4), a thread of the LDS kernel a quarter, an eighth or a sixteenth.  The frame is 12 rows x 200 columns: four mask
words a row, the last one of 8 pixels.  Every case holds, in its final mask (the frame's outermost pixels zeroed),
  a border pixel on bit 0 and on bit 63 of a word; on both sides of bits 15 | 16, 31 | 32 and 47 | 48; in the first and in the last
  word of a row; in rows 1 and H - 2; a hole (sides that face background which is not OUTSIDE); and two squares that touch only at
  a corner, across a word boundary (one 8-connected blob).
A border pixel is a foreground pixel with a background 4-neighbour: what the kernels walk.

Every blob's record must reach a comparison, on every path: the plain step hands out one blob, so it is run once per area window
of windows() -- each blob is the only candidate of one of them -- and the ranked steps take K = 4 (the issue's) and K = 8, which
holds all five blobs of a case.  seams() names the border pixels of every listed seam, so that the CPU test can say which blob each
lies on."""
import functools

import numpy as np

H, W = 12, 200
WORD = 64
SEAM_BITS = (0, 63, 15, 16, 31, 32, 47, 48)
AREA = (0.5, 1e6)
KS = (4, 8)


def _case_rows():
    """long horizontal edges: every seam bit of word 0 lies on the top row (row 1) of a bar that runs on into word 1"""
    m = np.zeros((H, W), np.uint8)
    m[1:4, 10:71] = 255                       # rows 1 .. 3, x 10 .. 70: bits 10 .. 63 of word 0, 0 .. 6 of word 1
    m[5:7, 60:64] = 255                       # two squares, corner to corner across x = 63 | 64
    m[7:9, 64:68] = 255
    m[5:10, 100:141] = 255                    # a ring across x = 127 | 128 ...
    m[6:9, 104:137] = 0                       # ... and its hole
    m[6:11, 190:199] = 255                    # the last word (x 192 .. 198), down to row H - 2
    m[8:11, 1:6] = 255                        # the first word from x = 1, down to row H - 2
    return m


def _case_columns():
    """vertical edges on the seams: a block from bit 0 to bit 63 of word 1 whose hole's walls stand on the chunk boundaries"""
    m = np.zeros((H, W), np.uint8)
    m[2:10, 64:128] = 255                     # word 1 exactly: left edge on bit 0, right edge on bit 63
    m[4:8, 80:112] = 0                        # the hole: x 80 .. 111 -- walls at bits 15 | 16 and 47 | 48
    m[4:8, 95:97] = 255                       # a bar through the hole at bits 31 | 32 (joins the block above and below)
    m[1:11, 1:21] = 255                       # the first word, rows 1 .. H - 2
    m[1:4, 192:199] = 255                     # the last word from its bit 0
    m[5:7, 188:192] = 255                     # two squares, corner to corner across x = 191 | 192
    m[7:9, 192:196] = 255
    m[9:11, 150:160] = 255                    # a fifth blob: more than K = 4
    return m


@functools.lru_cache(maxsize=None)
def cases():
    out = {"rows": _case_rows(), "columns": _case_columns()}
    for m in out.values():
        m.setflags(write=False)
    return out


def final(mask):
    """the mask the contour stage analyses: the frame's outermost rows and columns zeroed"""
    f = np.array(mask)
    f[0, :] = f[-1, :] = 0
    f[:, 0] = f[:, -1] = 0
    return f


def border(fin):
    """foreground pixels with a background 4-neighbour (bool)"""
    fg = fin != 0
    p = np.pad(fg, 1)
    inner = p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    return fg & ~inner


def corner_contacts(fin):
    """[(y, x)]: (x, y) and (x + 1, y + 1) are foreground, (x + 1, y) and (x, y + 1) background, x the last pixel of a word"""
    fg = fin != 0
    out = []
    for y in range(fin.shape[0] - 1):
        for x in range(WORD - 1, fin.shape[1] - 1, WORD):
            if fg[y, x] and fg[y + 1, x + 1] and not fg[y, x + 1] and not fg[y + 1, x]:
                out.append((y, x))
    return out


def windows(fin):
    """[(min_area, max_area)]: one window a contour area of the mask, selecting the blobs of exactly that area (the areas of a case
    are distinct: one blob a window), and AREA itself"""
    import oracle_lib as O
    areas = sorted({c["m00"] for c in O.find_contours(fin) if c["m00"] > 0})
    return [AREA] + [(a, areas[i + 1] if i + 1 < len(areas) else AREA[1]) for i, a in enumerate(areas)]


def seams(fin):
    """{seam name: [(y, x)]}: the border pixels of the final mask on every listed seam"""
    bd = border(fin)
    fg = fin != 0
    ys, xs = np.nonzero(bd)
    px = list(zip(ys.tolist(), xs.tolist()))
    out = {f"bit {b}": [(y, x) for y, x in px if x % WORD == b] for b in SEAM_BITS}
    out["first word"] = [(y, x) for y, x in px if x // WORD == 0]
    out["last word"] = [(y, x) for y, x in px if x // WORD == (fin.shape[1] - 1) // WORD]
    out["row 1"] = [(y, x) for y, x in px if y == 1]
    out["row H - 2"] = [(y, x) for y, x in px if y == fin.shape[0] - 2]
    import shapes_ref as R
    hole = np.pad(~fg & ~R.outside_background(fg), 1)
    out["beside a hole"] = [(y, x) for y, x in px if hole[y, x + 1] or hole[y + 2, x + 1] or hole[y + 1, x] or hole[y + 1, x + 2]]
    out["corner contact"] = [p for y, x in corner_contacts(fin) for p in ((y, x), (y + 1, x + 1))]
    return out
