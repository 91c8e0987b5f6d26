// kernels_croptensor.hip -- crop tensors: the windows of target crops, zoomed and converted for a network, in the caller's device
// memory (oatgpu_set_target_crop_tensor, oatgpu_crop_tensor_windows_dev).  The text in include/oatgpu.h ("crop
// tensors") is the contract.
//
// k_crop_tensor<CH, DTYPE> is the crop kernel of crops_inline.h -- k_target_crops' grid, lane mapping, record fetch, window and
// pixel rules, one definition each -- with the other outputs: DTYPE = kCropOutU8 the window's bytes [h][w][CH], kCropOutF16 /
// kCropOutF32 planar [CH][h][w] values fl32(fl32((float)p * scale[c]) + bias[c]), rounded to nearest even to half for F16.  A rank's
// window takes the launch's zoom: at 1.0 it is k_target_crops' window, the copy where the rank is upright.  The stores go to device
// memory, plain, at most 64 bits each.
#include "crops_inline.h"

namespace oatgpu {

template <int CH, int DTYPE> constexpr auto k_crop_tensor = k_crop_windows<CH, DTYPE>;

template <int DTYPE> static void launch_of(const Geom &g, const CropTensorLaunch &a, const dim3 &grid, const dim3 &block, hipStream_t st)
{
    if (a.channels == 3) hipLaunchKernelGGL((k_crop_tensor<3, DTYPE>), grid, block, 0, st, g.H, g.W, a);
    else hipLaunchKernelGGL((k_crop_tensor<1, DTYPE>), grid, block, 0, st, g.H, g.W, a);
}

void launch_crop_tensor(const Geom &g, const CropTensorLaunch &a, int dtype, int n_streams, hipStream_t st)
{
    dim3 grid, block;
    crop_grid(a, n_streams, grid, block);
    if (dtype == kCropOutU8) launch_of<kCropOutU8>(g, a, grid, block, st);
    else if (dtype == kCropOutF16) launch_of<kCropOutF16>(g, a, grid, block, st);
    else launch_of<kCropOutF32>(g, a, grid, block, st);
}

}  // namespace oatgpu
