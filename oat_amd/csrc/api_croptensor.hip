// api_croptensor.hip -- crop tensors: the windows of target crops in the caller's device memory, zoomed and converted for a network
// (DESIGN.md 9m).  A rider of the slots of the motion and the subtraction tracker, whose front launches leave the
// slot's frame set and its place in the call there (tracker_front): tracker_tail launches k_crop_tensor (kernels_croptensor.hip)
// behind k_target_crops on the same HIP stream -- frame set t of a call goes into entry t of the caller's memory, whichever slot it
// sat in.  The slot's ev_done already follows the launch, so the entry is complete when the call returns.  Nothing is allocated,
// copied or kept here: the memory is the caller's.  oatgpu_crop_tensor_windows_dev is the same kernel on an explicit table of
// windows.  What is the same as for target crops -- the launch's base, the switch's preconditions, the explicit call's path, the
// table -- is api_crops.hip's.
#include "oatgpu_ctx.h"

#include <cmath>

static_assert(OATGPU_TENSOR_U8 == kCropOutU8 && OATGPU_TENSOR_F16 == kCropOutF16 && OATGPU_TENSOR_F32 == kCropOutF32,
              "the header's dtypes are the kernel's");
static_assert(sizeof(oatgpu_crop_tensor_fmt) == 32, "oatgpu_crop_tensor_fmt's layout");

static size_t element_bytes(int dtype) { return dtype == OATGPU_TENSOR_U8 ? 1 : dtype == OATGPU_TENSOR_F16 ? 2 : 4; }

static void fill(CropTensorLaunch &a, const oatgpu_crop_tensor_fmt &f)
{
    for (int i = 0; i < 3; ++i) { a.scale[i] = f.scale[i]; a.bias[i] = f.bias[i]; }
}

int crop_tensor_launch(oatgpu_ctx *c, const BatchedTrackerState &bt, int slot, hipStream_t st)
{
    const CropTensor &ct = c->tg.ct;
    if (!ct.mode) return OATGPU_OK;
    const int entry = bt.entry[slot];
    if (entry < 0 || entry >= ct.capacity)         // (crop_tensor_room refused the call before anything was launched)
        return fail(c, OATGPU_E_INVALID, "crop tensor: frame set %d of the call has no entry (capacity %d)", entry, ct.capacity);
    CropTensorLaunch a{};
    crop_launch_from_slot(a, c, bt, slot, ct.mode, ct.h, ct.w);
    a.out = ct.out + (size_t)entry * ct.entry_bytes;
    a.zoom = ct.zoom;
    fill(a, ct.fmt);
    launch_crop_tensor(c->g, a, ct.fmt.dtype, c->cfg.n_streams, st);
    HIPCHK(c, hipGetLastError());
    return OATGPU_OK;
}

void crop_tensor_keep(oatgpu_ctx *c)
{
    if (c->tg.ct.mode) c->tg.ct.last_sets++;
}

int crop_tensor_room(oatgpu_ctx *c, int n_frames, const char *what)
{
    const CropTensor &ct = c->tg.ct;
    if (ct.mode && n_frames > ct.capacity)
        return fail(c, OATGPU_E_INVALID, "%s: %d frames, the crop tensor has %d entries (oatgpu_set_target_crop_tensor)", what, n_frames,
                    ct.capacity);
    return OATGPU_OK;
}

static int check_fmt(oatgpu_ctx *c, const char *what, const oatgpu_crop_tensor_fmt *f, const void *out_dev)
{
    if (!f) return fail(c, OATGPU_E_INVALID, "%s: null format", what);
    if (f->dtype != OATGPU_TENSOR_U8 && f->dtype != OATGPU_TENSOR_F16 && f->dtype != OATGPU_TENSOR_F32)
        return fail(c, OATGPU_E_INVALID, "%s: the dtype must be OATGPU_TENSOR_U8, _F16 or _F32 (got %d)", what, f->dtype);
    if (f->reserved != 0) return fail(c, OATGPU_E_INVALID, "%s: the format's reserved field must be 0 (got %d)", what, f->reserved);
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(f->scale[i]) || !std::isfinite(f->bias[i]))
            return fail(c, OATGPU_E_INVALID, "%s: scale and bias must be finite (channel %d: %g, %g)", what, i, (double)f->scale[i],
                        (double)f->bias[i]);
    if (!out_dev) return fail(c, OATGPU_E_INVALID, "%s: null output", what);
    if ((uintptr_t)out_dev % 16 != 0) return fail(c, OATGPU_E_INVALID, "%s: the output must be 16-byte aligned (got %p)", what, out_dev);
    return OATGPU_OK;
}

extern "C" int oatgpu_set_target_crop_tensor(oatgpu_ctx *c, int32_t mode, int32_t h, int32_t w, double zoom,
                                             const oatgpu_crop_tensor_fmt *fmt, void *out_dev, int32_t capacity_sets)
{
    if (!c) return OATGPU_E_INVALID;
    const char *what = "set_target_crop_tensor";
    int rc = check_crop_mode(c, what, mode);
    if (rc) return rc;
    if (mode != OATGPU_CROP_OFF) {
        rc = check_crop_size(c, what, h, w);
        if (rc) return rc;
        rc = check_crop_zoom(c, what, zoom);
        if (rc) return rc;
        rc = check_fmt(c, what, fmt, out_dev);
        if (rc) return rc;
        if (capacity_sets < 1) return fail(c, OATGPU_E_INVALID, "%s: room for at least one frame set is needed (got %d)", what, capacity_sets);
    }
    if (c->ring_count || c->staged_count) return fail(c, OATGPU_E_INVALID, "%s while enqueued results are outstanding", what);
    if (mode != OATGPU_CROP_OFF && (rc = check_crop_switch(c, what, mode))) return rc;
    rc = open_sync(c);
    if (rc) return rc;
    CropTensor &ct = c->tg.ct;
    ct = {};
    if (mode == OATGPU_CROP_OFF) return OATGPU_OK;
    ct.mode = mode; ct.h = h; ct.w = w; ct.zoom = zoom; ct.fmt = *fmt;
    ct.out = (uint8_t *)out_dev;
    ct.capacity = capacity_sets;
    ct.entry_bytes = (size_t)c->cfg.n_streams * (size_t)c->tg.k * (size_t)h * (size_t)w * (size_t)c->cfg.channels * element_bytes(fmt->dtype);
    return OATGPU_OK;
}

extern "C" int oatgpu_target_crop_tensor_sets(oatgpu_ctx *c)
{
    if (!c) return OATGPU_E_INVALID;
    const CropTensor &ct = c->tg.ct;
    if (!ct.mode) return fail(c, OATGPU_E_INVALID, "crop tensors are off (oatgpu_set_target_crop_tensor)");
    if (ct.last_sets == 0) return fail(c, OATGPU_E_INVALID, "no call has delivered a crop tensor entry since crop tensors were switched on");
    return ct.last_sets;
}

extern "C" int oatgpu_crop_tensor_windows_dev(oatgpu_ctx *c, const void *frames_dev, const oatgpu_crop_window *win, int32_t per_stream,
                                              int32_t h, int32_t w, const oatgpu_crop_tensor_fmt *fmt, void *out_dev)
{
    if (!c) return OATGPU_E_INVALID;
    const char *what = "crop_tensor_windows";
    if (!frames_dev || !win) return fail(c, OATGPU_E_INVALID, "null argument");
    int rc = check_windows(c, what, per_stream, h, w);
    if (!rc) rc = check_fmt(c, what, fmt, out_dev);
    if (!rc) rc = load_windows(c, what, win, per_stream);
    if (rc) return rc;
    CropTensorLaunch a{};
    crop_launch_from_table(a, c, frames_dev, per_stream, h, w);
    a.out = (uint8_t *)out_dev;
    a.zoom = 1.0;                                           // (an explicit window carries its zoom in (ax, ay))
    fill(a, *fmt);
    launch_crop_tensor(c->g, a, fmt->dtype, c->cfg.n_streams, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OATGPU_OK;
}
