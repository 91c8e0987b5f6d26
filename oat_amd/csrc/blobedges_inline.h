// blobedges_inline.h -- ONE definition of the rules that turn a final mask into OpenCV's contour moments and the step's result
// (cv::findContours(RETR_EXTERNAL) + cv::moments + the largest area in the window): the contour-edge rule and the
// neighbour ring it reads, the Green terms of an edge, the global path's walk over the border pixels of a word chunk, the area
// window with the ranking key, a thread's bits of a word and a workgroup's arrival at its stream's counter.  For kernels_blob.hip
// (k_green_select, k_blob_rank, k_blob_shape) and kernels_bloblds.hip (k_blob_lds: it decides OUTSIDE from its run list in LDS, so
// it keeps its own loop round the edge rule).  These rules ARE the bit-exact parity with the reference.  No state, all inlined.
#pragma once
#include "blobruns_inline.h"

namespace oatgpu {

// ------------------------------------------------------------ the contour-edge rule ----
// The eight neighbours of every pixel of a word slice, one mask a direction: bit i of L is the pixel left of bit i of the slice.
template <typename M> struct Ring { M L, R, U, D, UL, UR, DL, DR; };
// the word whose bit i is the pixel left / right of bit i of word v (vP / vN: the previous / next word of v's row)
__device__ __forceinline__ u64 left_of(u64 v, u64 vP) { return (v << 1) | (vP >> 63); }
__device__ __forceinline__ u64 right_of(u64 v, u64 vN) { return (v >> 1) | (vN << 63); }
// ... from the nine words round a word: the row's own (the word, the previous and the next one), the row above's, the row below's
__device__ __forceinline__ Ring<u64> ring_of(u64 cur, u64 curP, u64 curN, u64 U, u64 upP, u64 upN, u64 D, u64 dnP, u64 dnN)
{
    return Ring<u64>{left_of(cur, curP), right_of(cur, curN), U, D, left_of(U, upP), right_of(U, upN), left_of(D, dnP), right_of(D, dnN)};
}

// The sides of a pixel in the order they are visited.  A side whose neighbour is OUTSIDE background yields at most one directed
// edge from the pixel (x, y): to the DIAGONAL neighbour of the side if that is foreground, else to the STRAIGHT one if that is,
// else none --   left: DL, then D      bottom: DR, then R      right: UR, then U      top: UL, then L
// (the outer border followed with the background on the left hand, as cv::findContours does).
enum { kSideLeft = 0, kSideBottom = 1, kSideRight = 2, kSideTop = 3 };
template <int SIDE, typename M>
__device__ __forceinline__ bool edge_end(const Ring<M> &n, M bit, int x, int y, int &qx, int &qy)
{
    const M diag = SIDE == kSideLeft ? n.DL : SIDE == kSideBottom ? n.DR : SIDE == kSideRight ? n.UR : n.UL;
    const M strt = SIDE == kSideLeft ? n.D : SIDE == kSideBottom ? n.R : SIDE == kSideRight ? n.U : n.L;
    constexpr int ddx = (SIDE == kSideBottom || SIDE == kSideRight) ? 1 : -1, ddy = (SIDE == kSideLeft || SIDE == kSideBottom) ? 1 : -1;
    constexpr int sdx = SIDE == kSideBottom ? 1 : SIDE == kSideTop ? -1 : 0, sdy = SIDE == kSideLeft ? 1 : SIDE == kSideRight ? -1 : 0;
    if (diag & bit) { qx = x + ddx; qy = y + ddy; return true; }
    if (strt & bit) { qx = x + sdx; qy = y + sdy; return true; }
    return false;
}

// ------------------------------------------------------------ the Green terms of an edge (x, y) -> (qx, qy) ----
// Order <= 1 (contourMoments: a00, a10, a01), d = x qy - qx y.  P: the type the two products are formed in -- int where the
// caller has shown that they fit (k_blob_lds), long long otherwise; the sums are int64 either way.
template <typename P>
__device__ __forceinline__ void green1(int x, int y, int qx, int qy, long long &s00, long long &s10, long long &s01)
{
    const int d = x * qy - qx * y;
    s00 += d; s10 += (P)d * (x + qx); s01 += (P)d * (y + qy);
}
// Order 2 (a20, a11, a02): the products are formed in 64 bits, a term passes 2^31 from x ~ 900 on
__device__ __forceinline__ void green2(int x, int y, int qx, int qy, long long &s20, long long &s11, long long &s02)
{
    const long long d = (long long)(x * qy - qx * y), sy = y + qy;
    s20 += d * ((long long)x * (x + qx) + (long long)qx * qx);
    s11 += d * ((long long)x * (sy + y) + (long long)qx * (sy + qy));
    s02 += d * ((long long)y * (y + qy) + (long long)qy * qy);
}

// ------------------------------------------------------------ the global path: a thread's chunk of a mask word ----
// kGreenChunks threads a mask word of an interior row (1 .. H-2), thread tt of the stream's grid: the bits of the word that are its
__device__ __forceinline__ u64 chunk_bits(int tt)
{
    return (kGreenChunks == 1 ? ~0ull : ((1ull << (64 / kGreenChunks)) - 1ull)) << ((tt % kGreenChunks) * (64 / kGreenChunks));
}
struct BorderChunk {
    int y, w;          // the word's row and index (0, 0 behind the last interior row)
    u64 bits, cur;     // chunk_bits; the word (0 behind the last interior row)
    __device__ __forceinline__ bool any() const { return (cur & bits) != 0ull; }      // foreground among the thread's bits
};
__device__ __forceinline__ BorderChunk border_chunk(const Geom &g, const u64 *fin, int tt)
{
    BorderChunk c{0, 0, chunk_bits(tt), 0ull};
    const int t = tt / kGreenChunks;
    if (t < (g.H - 2) * g.words) {
        c.y = 1 + t / g.words; c.w = t % g.words;
        c.cur = fin[(size_t)c.y * g.words + c.w];
    }
    return c;
}
// The border pixels among the chunk's bits (a foreground pixel with a background 4-neighbour), and the straight half of the ring
// they are read from.  (In two steps because k_blob_shape decides on these bits, workgroup-wide, whether it goes on at all.)
__device__ __forceinline__ u64 border_bits(const Geom &g, const u64 *fin, const BorderChunk &c, Ring<u64> &n)
{
    const size_t rc = (size_t)c.y * g.words;
    const u64 curP = c.w > 0 ? fin[rc + c.w - 1] : 0ull, curN = c.w + 1 < g.words ? fin[rc + c.w + 1] : 0ull;
    n.U = fin[rc - g.words + c.w]; n.D = fin[rc + g.words + c.w];
    n.L = left_of(c.cur, curP); n.R = right_of(c.cur, curN);
    return c.cur & ~(n.L & n.R & n.U & n.D) & c.bits;
}
// The walk over those border pixels `cand`, lowest bit first.  Tc: the row's run starts in this word (trans).  Roots are found by
// walking parent[] (uf_root, no flatten pass); consecutive border pixels of one edge look at the same runs, so the last
// (run head -> root) pair per lookup class is memoised and a straight edge costs one walk.  The callables:
//   wanted(root) -> bool   the pixel's root is not the previous pixel's: is its contour wanted?  (If not, no side is tested.)
//   edge(x, y, qx, qy)     a side that faces OUTSIDE background (root 0) yields this edge
//   outside(x, y)          the pixel has a side facing OUTSIDE background
template <typename Wanted, typename Edge, typename Outside>
__device__ __forceinline__ void walk_border(const Geom &g, const u64 *fin, const u64 *trans, const int *carry, const int *parent,
                                            const BorderChunk &c, Ring<u64> &n, u64 cand, u64 Tc, Wanted wanted, Edge edge, Outside outside)
{
    const int y = c.y, w = c.w;
    const size_t rc = (size_t)y * g.words, ru = rc - g.words, rd = rc + g.words;
    const bool hp = w > 0, hn = w + 1 < g.words;
    const u64 upP = hp ? fin[ru + w - 1] : 0ull, upN = hn ? fin[ru + w + 1] : 0ull;
    const u64 dnP = hp ? fin[rd + w - 1] : 0ull, dnN = hn ? fin[rd + w + 1] : 0ull;
    n.UL = left_of(n.U, upP); n.UR = right_of(n.U, upN);
    n.DL = left_of(n.D, dnP); n.DR = right_of(n.D, dnN);
    const u64 Tu = trans[ru + w], Td = trans[rd + w];
    const int cc = carry[rc + w], cu = carry[ru + w], cd = carry[rd + w];

    struct Memo { int head, root; };
    Memo mo{-1, 0}, ml{-1, 0}, mb{-1, 0}, mr{-1, 0}, mt{-1, 0};
    auto root_of = [&](Memo &m, int head) -> int {
        if (head != m.head) { m.head = head; m.root = uf_root(parent, head); }
        return m.root;
    };
    int label = -1;
    bool want = false;      // the contour of root `label` is wanted
    while (cand) {
        const int i = lsb64(cand);
        cand &= cand - 1;
        const int x = w * 64 + i;
        const u64 bit = 1ull << i;
        const int lab = root_of(mo, run_head_w(g, Tc, cc, y, w, i));
        if (lab != label) { label = lab; want = wanted(lab); }
        if (!want) continue;
        int qx, qy;
        bool out = false;
        if (!(n.L & bit)) {
            const int h = i > 0 ? run_head_w(g, Tc, cc, y, w, i - 1) : run_head(g, trans, carry, y, x - 1);
            if (root_of(ml, h) == 0) { out = true; if (edge_end<kSideLeft>(n, bit, x, y, qx, qy)) edge(x, y, qx, qy); }
        }
        if (!(n.D & bit) && root_of(mb, run_head_w(g, Td, cd, y + 1, w, i)) == 0) {
            out = true; if (edge_end<kSideBottom>(n, bit, x, y, qx, qy)) edge(x, y, qx, qy);
        }
        if (!(n.R & bit)) {
            const int h = i < 63 ? run_head_w(g, Tc, cc, y, w, i + 1) : run_head(g, trans, carry, y, x + 1);
            if (root_of(mr, h) == 0) { out = true; if (edge_end<kSideRight>(n, bit, x, y, qx, qy)) edge(x, y, qx, qy); }
        }
        if (!(n.U & bit) && root_of(mt, run_head_w(g, Tu, cu, y - 1, w, i)) == 0) {
            out = true; if (edge_end<kSideTop>(n, bit, x, y, qx, qy)) edge(x, y, qx, qy);
        }
        if (out) outside(x, y);
    }
}

// ------------------------------------------------------------ the area window and the ranking key ----
// A root with Green sum a00 and (padded) first pixel `first` is a candidate if a00 != 0 (a blob inside another blob's hole never
// faces the outside background: its sums stay 0) and min_area <= |a00| / 2 < max_area; its key is |a00| << 32 | first pixel, larger
// first: ties go to the later first pixel -- the reference walks its reversed contour list with a strict '>'.  0: no candidate.
__device__ __forceinline__ u64 area_key(long long a00, unsigned first, double min_area, double max_area)
{
    if (a00 == 0) return 0ull;
    const u64 mag = (u64)(a00 < 0 ? -a00 : a00);
    const double area = (double)mag * 0.5;            // m00 = a00 * (+-0.5), exact
    if (!(area >= min_area && area < max_area)) return 0ull;
    return (mag << 32) | (u64)first;
}
__device__ __forceinline__ unsigned key_first(u64 key) { return (unsigned)(key & 0xffffffffull); }
// a record's first_pixel (y * W + x) from the padded index h (y * Wp + x); I: int or unsigned, the division the caller had
template <typename I>
__device__ __forceinline__ int first_pixel_of(const Geom &g, I h)
{
    const I yy = h / (I)g.Wp, xx = h - yy * (I)g.Wp;
    return (int)(yy * (I)g.W + xx);
}

// ------------------------------------------------------------ the arrival ----
// Every workgroup of a stream's grid (gridDim.x of them) arrives once at the stream's counter; true, in all its threads, in the last to
// arrive.  What that one reads of the others' writes goes through agent-scope atomics: each wave drains vmcnt first.  is_last: in LDS.
__device__ __forceinline__ bool arrive_last(unsigned *counter, int *is_last)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned prev = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *is_last = (prev == gridDim.x - 1) ? 1 : 0;
    }
    __syncthreads();
    return *is_last != 0;
}

}  // namespace oatgpu
