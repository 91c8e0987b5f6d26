// blobruns_inline.h -- ONE definition of how a pixel of the final mask finds its connected component in what a global back half
// leaves in its scratch set (kernels_rowscan.hip: k_rowscan's run starts `trans` / `carry`; kernels_blob.hip: k_merge's union-find
// `parent`): the run that holds the pixel, and the read-only walk from the run's head to its root.  Used by the blob kernels
// (kernels_blob.hip: k_merge; blobedges_inline.h: the border walk of k_green_select and k_blob_shape) and by the target-mask
// kernel (crops_inline.h, kernels_targetmask.hip).  The bit helpers of the mask words stand here too: every unit
// of the blob stage (kernels_rowscan.hip, kernels_bloblds.hip, kernels_blob.hip) takes them from this header.
#pragma once
#include "oatgpu_internal.h"

namespace oatgpu {

__device__ __forceinline__ int msb64(u64 v) { return 63 - __clzll((long long)v); }
__device__ __forceinline__ int lsb64(u64 v) { return __ffsll((long long)v) - 1; }
__device__ __forceinline__ u64 low_mask_incl(int i) { return (i >= 63) ? ~0ull : ((2ull << i) - 1ull); }

// bits of word w that are real pixels (x < W)
__device__ __forceinline__ u64 valid_bits(const Geom &g, int w)
{
    const int rem = g.W - w * 64;
    return rem >= 64 ? ~0ull : (rem <= 0 ? 0ull : ((1ull << rem) - 1ull));
}

// head (first pixel, padded index) of the run that contains pixel (x, y)
__device__ __forceinline__ int run_head(const Geom &g, const u64 *trans, const int *carry, int y, int x)
{
    const int w = x >> 6, i = x & 63;
    const u64 t = trans[(size_t)y * g.words + w] & low_mask_incl(i);
    const int sx = t ? (w * 64 + msb64(t)) : carry[(size_t)y * g.words + w];
    return y * g.Wp + sx;
}
// same, with this word's T / carry already in registers
__device__ __forceinline__ int run_head_w(const Geom &g, u64 Tw, int cw, int y, int w, int i)
{
    const u64 t = Tw & low_mask_incl(i);
    const int sx = t ? (w * 64 + msb64(t)) : cw;
    return y * g.Wp + sx;
}

// read-only walk to the root (after the merge kernel has completed: plain loads)
__device__ __forceinline__ int uf_root(const int *parent, int i)
{
    int p = parent[i];
    while (p != i) { i = p; p = parent[i]; }
    return i;
}

}  // namespace oatgpu
