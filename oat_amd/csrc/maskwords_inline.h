// maskwords_inline.h -- a wave's mask words out of four pixels a lane, shared by the front kernels that own 4 consecutive pixels
// of a row per lane (kernels_diff.hip, kernels_bsubtrack.hip).
#pragma once

#include "oatgpu_internal.h"

namespace oatgpu {

// bits 0..15 of x to bits 0, 4, 8, .. 60
__device__ __forceinline__ u64 spread4(u64 x)
{
    x = (x | x << 24) & 0x000000ff000000ffull;
    x = (x | x << 12) & 0x000f000f000f000full;
    x = (x | x << 6) & 0x0303030303030303ull;
    x = (x | x << 3) & 0x1111111111111111ull;
    return x;
}

// the wave's 4 mask words out of every lane's nibble (bit k = pixel k of the lane): lane w < 4 stores word w
__device__ __forceinline__ void store_words(unsigned nib, int lane, u64 *dst)
{
    const u64 b0 = __ballot(nib & 1u), b1 = __ballot(nib & 2u), b2 = __ballot(nib & 4u), b3 = __ballot(nib & 8u);
    if (lane < 4) {
        const int sh = lane * 16;
        dst[lane] = spread4((b0 >> sh) & 0xffffull) | spread4((b1 >> sh) & 0xffffull) << 1 | spread4((b2 >> sh) & 0xffffull) << 2 |
                    spread4((b3 >> sh) & 0xffffull) << 3;
    }
}

}  // namespace oatgpu
