// hsv_inline.h -- BGR -> HSV of ONE pixel and the inRange test, the one implementation of every kernel that converts: the
// per-pixel MOG2 kernel (kernels_mog.hip), the marker sets (kernels_markers.hip), the subtraction tracker (kernels_bsubtrack.hip)
// and the single stage k_bgr2hsv (kernels_stages.hip) produce the same HSV triple for the same pixel, bit for bit.
#pragma once

#include "oatgpu_internal.h"

namespace oatgpu {

// RGB2HSV_b's table entries sdiv[i] = cvRound((255<<12)/i), hdiv[i] = cvRound((180<<12)/(6 i)), computed on the spot: a pixel
// needs two of them, K1 for FOREGROUND pixels only, and 256-entry tables in LDS would cost every workgroup 512 quotients and a
// barrier.  Neither quotient ever lands on .5 (255<<12 = 2^12*255, 180<<12/6 = 2^13*15), so round-half-even == floor(q + 1/2)
// == floor((2n + i) / (2i)).  The quotient is taken in fp32: numerator < 2^22 and denominator <= 510 are exact floats, and the
// exact quotient is at least 1/(2i) away from the next integer, so floor() of an fp32 quotient good to a few ulp is exact.
// (r05) the quotient as numerator * v_rcp_f32(denominator), 2 vector instructions instead of the 11 of an IEEE division:
// v_rcp_f32 is good to 1 ulp and the product rounds once more, so the result is within 1.5 * 2^-23 of the exact quotient
// q <= 2^20 / i + 1/2, i.e. off by < 0.19 / i, while q lies at least 1 / (2i) away from the next integer (above): floor()
// still lands on the same integer.  tests/test_abi_exports.py checks every entry with the reciprocal off by one ulp either
// way, test_bgr2hsv_exhaustive_256cubed runs all 2^24 colours through k_bgr2hsv, that is through these very functions.
__device__ __forceinline__ int hsv_sdiv(int i) { return i ? (int)floorf((float)(2 * (255 << 12) + i) * __builtin_amdgcn_rcpf((float)(2 * i))) : 0; }
__device__ __forceinline__ int hsv_hdiv(int i) { return i ? (int)floorf((float)(2 * ((180 << 12) / 6) + i) * __builtin_amdgcn_rcpf((float)(2 * i))) : 0; }
__device__ __forceinline__ void bgr2hsv_inline(int b, int g, int r, int &h, int &s, int &v)
{
    v = max(b, max(g, r));
    const int vmin = min(b, min(g, r));
    const int diff = v - vmin;
    s = (diff * hsv_sdiv(v) + (1 << 11)) >> 12;
    int hh = (v == r) ? (g - b) : (v == g) ? (b - r + 2 * diff) : (r - g + 4 * diff);
    hh = (hh * hsv_hdiv(diff) + (1 << 11)) >> 12;   // arithmetic shift, as the reference
    hh += hh < 0 ? 180 : 0;
    h = hh;
}

__device__ __forceinline__ bool in_range3(int a, int b, int c, const RangeParams &rp)
{
    return a >= rp.lo[0] && a <= rp.hi[0] && b >= rp.lo[1] && b <= rp.hi[1] &&
           c >= rp.lo[2] && c <= rp.hi[2];
}

}  // namespace oatgpu
