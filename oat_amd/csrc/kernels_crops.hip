// kernels_crops.hip -- target crops: an h x w window of the input frame around every ranked blob, upright or turned so that the
// blob's body axis lies along the window's +x (oatgpu_set_target_crops, oatgpu_crop_windows_dev).  The text in
// include/oatgpu.h ("target crops") is the contract; crops_inline.h is its one implementation on the device, shared with crop
// tensors (kernels_croptensor.hip).
//
// k_target_crops is ONE body for both sources of windows: a target set with the shape set beside it (launched behind k_blob_rank
// / k_blob_shape on the same HIP stream, api_crops.hip), or an explicit table (oatgpu_crop_windows_dev).  It is the crop kernel
// with the output it always had: the window's bytes, 32-bit stores into a crop set that may be host-mapped memory.
#include "crops_inline.h"

namespace oatgpu {

template <int CH> constexpr auto k_target_crops = k_crop_windows<CH, kCropOutBytes>;

void launch_target_crops(const Geom &g, const CropLaunch &a, int n_streams, hipStream_t st)
{
    dim3 grid, block;
    crop_grid(a, n_streams, grid, block);
    if (a.channels == 3) hipLaunchKernelGGL(k_target_crops<3>, grid, block, 0, st, g.H, g.W, a);
    else hipLaunchKernelGGL(k_target_crops<1>, grid, block, 0, st, g.H, g.W, a);
}

}  // namespace oatgpu
