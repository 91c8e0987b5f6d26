// api_targetmask.hip -- target masks: which pixels of a ranked blob's window are that blob, in the caller's device memory (DESIGN.md
// 9o).  A rider of the slots of the motion and the subtraction tracker: tracker_tail launches k_target_mask
// (kernels_targetmask.hip) behind k_crop_tensor on the slot's HIP stream, on the scratch set the slot's global back half has just
// left -- frame set t of a call goes into entry t of the caller's memory, whichever slot it sat in.  The slot's ev_done already
// follows the launch, so the entry is complete when the call returns.  Nothing is allocated, copied or kept here: the memory is the
// caller's.  The window is the crop tensor's (crop_launch_from_slot, check_crop_mode / _size / _zoom, check_window_riders:
// api_crops.hip); the mask is cut from the tracker's own final mask, not from the caller's frames, so -- unlike the two crop
// switches -- it rides behind the RAW8 and the undistorting front end as well.
#include "oatgpu_ctx.h"

int mask_tensor_launch(oatgpu_ctx *c, const BatchedTrackerState &bt, const BlobBuffers &bb, int slot, hipStream_t st)
{
    const MaskTensor &mt = c->tg.mt;
    if (!mt.mode) return OATGPU_OK;
    const int entry = bt.entry[slot];
    if (entry < 0 || entry >= mt.capacity)         // (mask_tensor_room refused the call before anything was launched)
        return fail(c, OATGPU_E_INVALID, "target masks: frame set %d of the call has no entry (capacity %d)", entry, mt.capacity);
    MaskTensorLaunch a{};
    crop_launch_from_slot(a, c, bt, slot, mt.mode, mt.h, mt.w);
    a.frames = nullptr;                            // (no pixel of a frame is read)
    a.channels = 1;
    a.out = mt.out + (size_t)entry * mt.entry_bytes;
    a.zoom = mt.zoom;
    a.g = c->g;
    a.b = bb;
    launch_target_mask(a, mt.dtype, c->cfg.n_streams, st);
    HIPCHK(c, hipGetLastError());
    return OATGPU_OK;
}

void mask_tensor_keep(oatgpu_ctx *c)
{
    if (c->tg.mt.mode) c->tg.mt.last_sets++;
}

int mask_tensor_room(oatgpu_ctx *c, int n_frames, const char *what)
{
    const MaskTensor &mt = c->tg.mt;
    if (mt.mode && n_frames > mt.capacity)
        return fail(c, OATGPU_E_INVALID, "%s: %d frames, the mask tensor has %d entries (oatgpu_set_target_mask_tensor)", what, n_frames,
                    mt.capacity);
    return OATGPU_OK;
}

extern "C" int oatgpu_set_target_mask_tensor(oatgpu_ctx *c, int32_t mode, int32_t h, int32_t w, double zoom, int32_t dtype,
                                             void *out_dev, int32_t capacity_sets)
{
    if (!c) return OATGPU_E_INVALID;
    const char *what = "set_target_mask_tensor";
    int rc = check_crop_mode(c, what, mode);
    if (rc) return rc;
    if (mode != OATGPU_CROP_OFF) {
        rc = check_crop_size(c, what, h, w);
        if (!rc) rc = check_crop_zoom(c, what, zoom);
        if (rc) return rc;
        if (dtype != OATGPU_TENSOR_U8 && dtype != OATGPU_TENSOR_F16 && dtype != OATGPU_TENSOR_F32)
            return fail(c, OATGPU_E_INVALID, "%s: the dtype must be OATGPU_TENSOR_U8, _F16 or _F32 (got %d)", what, dtype);
        if (!out_dev) return fail(c, OATGPU_E_INVALID, "%s: null output", what);
        if ((uintptr_t)out_dev % 16 != 0) return fail(c, OATGPU_E_INVALID, "%s: the output must be 16-byte aligned (got %p)", what, out_dev);
        if (capacity_sets < 1) return fail(c, OATGPU_E_INVALID, "%s: room for at least one frame set is needed (got %d)", what, capacity_sets);
    }
    if (c->ring_count || c->staged_count) return fail(c, OATGPU_E_INVALID, "%s while enqueued results are outstanding", what);
    if (mode != OATGPU_CROP_OFF && (rc = check_window_riders(c, what, mode))) return rc;
    rc = open_sync(c);
    if (rc) return rc;
    MaskTensor &mt = c->tg.mt;
    mt = {};
    if (mode == OATGPU_CROP_OFF) return OATGPU_OK;
    mt.mode = mode; mt.h = h; mt.w = w; mt.zoom = zoom; mt.dtype = dtype;
    mt.out = (uint8_t *)out_dev;
    mt.capacity = capacity_sets;
    mt.entry_bytes = (size_t)c->cfg.n_streams * (size_t)c->tg.k * (size_t)h * (size_t)w *
                     (dtype == OATGPU_TENSOR_U8 ? 1u : dtype == OATGPU_TENSOR_F16 ? 2u : 4u);
    return OATGPU_OK;
}

extern "C" int oatgpu_target_mask_tensor_sets(oatgpu_ctx *c)
{
    if (!c) return OATGPU_E_INVALID;
    const MaskTensor &mt = c->tg.mt;
    if (!mt.mode) return fail(c, OATGPU_E_INVALID, "target masks are off (oatgpu_set_target_mask_tensor)");
    if (mt.last_sets == 0) return fail(c, OATGPU_E_INVALID, "no call has delivered a mask tensor entry since target masks were switched on");
    return mt.last_sets;
}
