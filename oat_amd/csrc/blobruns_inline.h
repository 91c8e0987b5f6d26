// blobruns_inline.h -- ONE definition of how a pixel of the final mask finds its connected component in what a global back half
// leaves in its scratch set (kernels_blob.hip: k_rowscan's run starts `trans` / `carry`, k_merge's union-find `parent`): the run
// that holds the pixel, and the read-only walk from the run's head to its root.  Used by the blob kernels (kernels_blob.hip:
// k_merge, k_green_select, k_blob_shape) and by the target-mask kernel (crops_inline.h, kernels_targetmask.hip).
// The functions stand here as they stood in kernels_blob.hip, word for word.
#pragma once
#include "oatgpu_internal.h"

namespace oatgpu {

__device__ __forceinline__ int msb64(u64 v) { return 63 - __clzll((long long)v); }
__device__ __forceinline__ u64 low_mask_incl(int i) { return (i >= 63) ? ~0ull : ((2ull << i) - 1ull); }

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
