// debayer_inline.h -- the arithmetic of the Bayer RAW8 -> BGR stage, shared by the stage itself
// (kernels_debayer.hip) and the front kernels that demosaic in registers (kernels_diff.hip, kernels_bsubtrack.hip).
//
// OpenCV 3.1's bilinear Bayer2RGB_ in 32-bit integers.  At an R or B site: own colour = the sample,
// G = (N + S + W + E + 2) >> 2, opposite colour = (NW + NE + SW + SE + 2) >> 2.  At a G site: G = the sample, the colour of the
// horizontal neighbours = (W + E + 1) >> 1, of the vertical ones = (N + S + 1) >> 1.  Output (y, x) is the triple of
// (clamp(y, 1, H - 2), clamp(x, 1, W - 2)) with THAT pixel's site colours: first / last column and row repeat their neighbours.
//
// A pattern is two parity bits: the row and the column of the R sample of the 2 x 2 tile.
#pragma once
#include "oatgpu_internal.h"

namespace oatgpu {

// the five candidate values of a pixel from its 3 x 3 neighbourhood -> (B, G, R) packed as B | G << 8 | R << 16.
// row_r / col_r: the pixel's row / column holds R samples
__device__ __forceinline__ unsigned site_bgr(unsigned nw, unsigned n, unsigned ne, unsigned w, unsigned c, unsigned e,
                                             unsigned sw, unsigned s, unsigned se, bool row_r, bool col_r)
{
    const unsigned h = (w + e + 1u) >> 1, v = (n + s + 1u) >> 1;
    const unsigned p = (n + s + w + e + 2u) >> 2, d = (nw + ne + sw + se + 2u) >> 2;
    unsigned b, g, r;
    if (row_r == col_r) {                // an R or a B site
        g = p;
        r = row_r ? c : d;
        b = row_r ? d : c;
    } else {                             // a G site: in an R row the horizontal neighbours are R, the vertical ones B
        g = c;
        r = row_r ? h : v;
        b = row_r ? v : h;
    }
    return b | g << 8 | r << 16;
}

// bytes x0 - 1 .. x0 + 4 of a raw row as one little-endian 48-bit window (l, c, r: the dwords at x0 - 4, x0, x0 + 4)
__device__ __forceinline__ u64 window(unsigned l, unsigned c, unsigned r)
{
    return (u64)(l >> 24) | (u64)c << 8 | (u64)(r & 255u) << 40;
}
__device__ __forceinline__ unsigned wbyte(u64 w, int j) { return (unsigned)(w >> (8 * j)) & 255u; }

// the four BGR triples of one output row of a wide lane from the windows of the raw rows above, at and below it
__device__ __forceinline__ void row4(u64 up, u64 at, u64 dn, bool row_r, bool col0_r, unsigned px[4])
{
#pragma unroll
    for (int i = 0; i < 4; ++i)          // pixel i sits at window byte i + 1; x0 % 4 == 0: its column parity is i & 1
        px[i] = site_bgr(wbyte(up, i), wbyte(up, i + 1), wbyte(up, i + 2), wbyte(at, i), wbyte(at, i + 1), wbyte(at, i + 2),
                         wbyte(dn, i), wbyte(dn, i + 1), wbyte(dn, i + 2), row_r, (i & 1) ? !col0_r : col0_r);
}

// 4 triples as the 12 bytes of 4 packed BGR pixels, three little-endian dwords
__device__ __forceinline__ void pack_bgr4(const unsigned px[4], unsigned (&d)[3])
{
    d[0] = px[0] | px[1] << 24;
    d[1] = px[1] >> 8 | px[2] << 16;
    d[2] = px[2] >> 16 | px[3] << 8;
}

// The triples of output pixels (y, x0 .. x0 + 3) of one raw plane with dword loads: x0 % 4 == 0, W % 4 == 0, the plane 4-byte
// aligned, H >= 3.  The dwords at x0 - 4, x0, x0 + 4 of the three raw rows around clamp(y, 1, H - 2); the neighbour columns are
// clamped into the row (the values they give at the first and last column are not used: those repeat their neighbours).
__device__ __forceinline__ void debayer_px4(const uint8_t *in, int H, int W, int y, int x0, bool r_row, bool r_col, unsigned px[4])
{
    const int cy = min(max(y, 1), H - 2);
    const int xl = x0 > 0 ? x0 - 4 : x0, xr = x0 + 4 < W ? x0 + 4 : x0;
    u64 w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint8_t *row = in + (size_t)(cy - 1 + k) * W;
        w[k] = window(*(const unsigned *)(row + xl), *(const unsigned *)(row + x0), *(const unsigned *)(row + xr));
    }
    row4(w[0], w[1], w[2], ((cy & 1) != 0) == r_row, r_col == false, px);     // x0 is even: it holds R iff the R column parity is 0
    if (x0 == 0) px[0] = px[1];
    if (x0 + 4 == W) px[3] = px[2];
}

// The triple of output pixel (y, x) of one raw plane with byte loads: H, W >= 3
__device__ __forceinline__ unsigned debayer_px1(const uint8_t *in, int H, int W, int y, int x, bool r_row, bool r_col)
{
    const int cy = min(max(y, 1), H - 2), cx = min(max(x, 1), W - 2);
    const uint8_t *r0 = in + (size_t)(cy - 1) * W + cx, *r1 = r0 + W, *r2 = r1 + W;
    return site_bgr(r0[-1], r0[0], r0[1], r1[-1], r1[0], r1[1], r2[-1], r2[0], r2[1], ((cy & 1) != 0) == r_row,
                    ((cx & 1) != 0) == r_col);
}

// patterns[n] (OATGPU_BAYER_* 1..4, n <= 64) as the two parity words of a launch, bit i = stream i of the launch.
// R sits at (row, column) parity: RGGB (0, 0), BGGR (1, 1), GRBG (0, 1), GBRG (1, 0)
inline void bayer_parity_bits(const int *patterns, int n, u64 &r_row, u64 &r_col)
{
    r_row = r_col = 0;
    for (int i = 0; i < n; ++i) {
        const int p = patterns[i];
        r_row |= (u64)(p == 2 || p == 4) << i;
        r_col |= (u64)(p == 2 || p == 3) << i;
    }
}

}  // namespace oatgpu
