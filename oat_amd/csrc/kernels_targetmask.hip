// kernels_targetmask.hip -- target masks: each ranked blob's own pixels in the window of its crop tensor, in the caller's device
// memory (oatgpu_set_target_mask_tensor).  The text in include/oatgpu.h ("target masks") is the contract.
//
// k_target_mask<DTYPE> is the crop kernel of crops_inline.h -- k_crop_tensor's grid, lane mapping, record fetch, window and zoom,
// one definition each -- with the pixel fetch replaced: an element's source pixel is looked up in what the slot's global back half
// left in its scratch set (the final mask, the run starts, the merged union-find; blobruns_inline.h) and the element is ON where
// that pixel belongs to the rank's component.  One plane [h][w] a window: 255 / 0 in bytes, 1.0 / 0.0 in halves and floats; plain
// stores to device memory, at most 64 bits each.  It reads the scratch set and the target and shape sets and writes only `out`.
#include "crops_inline.h"

namespace oatgpu {

template <int DTYPE> constexpr auto k_target_mask = k_crop_windows<1, kCropOutMask + DTYPE>;

void launch_target_mask(const MaskTensorLaunch &a, int dtype, int n_streams, hipStream_t st)
{
    dim3 grid, block;
    crop_grid(a, n_streams, grid, block);
    if (dtype == kCropOutU8) hipLaunchKernelGGL(k_target_mask<kCropOutU8>, grid, block, 0, st, a.g.H, a.g.W, a);
    else if (dtype == kCropOutF16) hipLaunchKernelGGL(k_target_mask<kCropOutF16>, grid, block, 0, st, a.g.H, a.g.W, a);
    else hipLaunchKernelGGL(k_target_mask<kCropOutF32>, grid, block, 0, st, a.g.H, a.g.W, a);
}

}  // namespace oatgpu
