// api_croptensor.hip -- crop tensors: the windows of target crops in the caller's device memory, zoomed and converted for a network
// (DESIGN.md 9m).  While the switch is on, targets_launch (api_targets.hip) launches k_crop_tensor (kernels_croptensor.hip) behind
// k_blob_rank, k_blob_shape and k_target_crops on the same HIP stream -- for the target sets of the motion and the subtraction
// tracker, whose front launches leave the slot's frame set and its place in the call there (tracker_front): frame set t of a call
// goes into entry t of the caller's memory, whichever slot it sat in.  The slot's ev_done already follows the launch, so the entry
// is complete when the call returns.  Nothing is allocated, copied or kept here: the memory is the caller's.
// oatgpu_crop_tensor_windows_dev is the same kernel on an explicit table of windows.
#include "oatgpu_ctx.h"

#include <cmath>

static_assert(OATGPU_TENSOR_U8 == kCropOutU8 && OATGPU_TENSOR_F16 == kCropOutF16 && OATGPU_TENSOR_F32 == kCropOutF32,
              "the header's dtypes are the kernel's");
static_assert(sizeof(oatgpu_crop_tensor_fmt) == 32, "oatgpu_crop_tensor_fmt's layout");

static size_t element_bytes(int dtype) { return dtype == OATGPU_TENSOR_U8 ? 1 : dtype == OATGPU_TENSOR_F16 ? 2 : 4; }

// a batched tracker's target sets: the only ones whose slots remember a frame set
static bool of_a_batched_tracker(const oatgpu_ctx *c, const TargetSets &ts) { return &ts == &c->df.tgt || &ts == &c->bs.tgt; }

static void fill(CropTensorLaunch &a, const oatgpu_crop_tensor_fmt &f)
{
    for (int i = 0; i < 3; ++i) { a.scale[i] = f.scale[i]; a.bias[i] = f.bias[i]; }
}

int crop_tensor_launch(oatgpu_ctx *c, const TargetSets &ts, int slot, int s0, int n, hipStream_t st)
{
    const Targets &tg = c->tg;
    const CropTensor &ct = tg.ct;
    if (!ct.mode || !of_a_batched_tracker(c, ts)) return OATGPU_OK;
    const int entry = ts.crp.entry[slot];
    if (entry < 0 || entry >= ct.capacity)         // (crop_tensor_room refused the call before anything was launched)
        return fail(c, OATGPU_E_INVALID, "crop tensor: frame set %d of the call has no entry (capacity %d)", entry, ct.capacity);
    const size_t k = (size_t)tg.k, win_bytes = (size_t)ct.h * ct.w * c->cfg.channels * element_bytes(ct.fmt.dtype);
    CropTensorLaunch a{};
    a.frames = ts.crp.frame[slot] + (size_t)s0 * c->g.H * c->g.W * c->cfg.channels;
    a.channels = c->cfg.channels;
    a.h = ct.h; a.w = ct.w; a.k = tg.k;
    a.axis = ct.mode == OATGPU_CROP_AXIS;
    a.recs = ts.rec_dev(slot) + (size_t)s0 * k;
    a.shp = a.axis ? ts.shp.rec_dev(slot) + (size_t)s0 * k : nullptr;
    a.out = ct.out + (size_t)entry * ct.entry_bytes + (size_t)s0 * k * win_bytes;
    a.zoom = ct.zoom;
    fill(a, ct.fmt);
    launch_crop_tensor(c->g, a, ct.fmt.dtype, n, st);
    HIPCHK(c, hipGetLastError());
    return OATGPU_OK;
}

void crop_tensor_begin(oatgpu_ctx *c) { c->tg.ct.last_sets = 0; }

void crop_tensor_keep(oatgpu_ctx *c, const TargetSets &ts)
{
    if (c->tg.ct.mode && of_a_batched_tracker(c, ts)) c->tg.ct.last_sets++;
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
    if (mode != OATGPU_CROP_OFF && mode != OATGPU_CROP_UPRIGHT && mode != OATGPU_CROP_AXIS)
        return fail(c, OATGPU_E_INVALID, "%s: the mode must be OATGPU_CROP_OFF, _UPRIGHT or _AXIS (got %d)", what, mode);
    Targets &tg = c->tg;
    if (mode != OATGPU_CROP_OFF) {
        int rc = check_crop_size(c, what, h, w);
        if (rc) return rc;
        if (!(zoom >= 1.0 / 16 && zoom <= 16.0))          // (false for a NaN)
            return fail(c, OATGPU_E_INVALID, "%s: the zoom must be in 1/16 .. 16 (got %g)", what, zoom);
        rc = check_fmt(c, what, fmt, out_dev);
        if (rc) return rc;
        if (capacity_sets < 1) return fail(c, OATGPU_E_INVALID, "%s: room for at least one frame set is needed (got %d)", what, capacity_sets);
    }
    if (c->ring_count || c->staged_count) return fail(c, OATGPU_E_INVALID, "%s while enqueued results are outstanding", what);
    if (mode != OATGPU_CROP_OFF) {
        if (!tg.k) return fail(c, OATGPU_E_INVALID, "%s: targets are off (oatgpu_set_targets)", what);
        if (mode == OATGPU_CROP_AXIS && !tg.shapes)
            return fail(c, OATGPU_E_INVALID, "%s: windows along the body axis need target shapes (oatgpu_set_target_shapes)", what);
        if (c->tb_on) return fail(c, OATGPU_E_INVALID, "%s with Bayer frames on (oatgpu_set_tracker_bayer) is not supported", what);
        if (c->tu_on) return fail(c, OATGPU_E_INVALID, "%s with undistortion on (oatgpu_set_tracker_undistort) is not supported", what);
    }
    const int rc = open_sync(c);
    if (rc) return rc;
    CropTensor &ct = tg.ct;
    HostMem<CropWin> table = std::move(ct.win);            // (the explicit form's table outlives the switch)
    ct = {};
    ct.win = std::move(table);
    if (mode == OATGPU_CROP_OFF) return OATGPU_OK;
    ct.mode = mode; ct.h = h; ct.w = w; ct.zoom = zoom; ct.fmt = *fmt;
    ct.out = (uint8_t *)out_dev;
    ct.capacity = capacity_sets;
    ct.entry_bytes = (size_t)c->cfg.n_streams * (size_t)tg.k * (size_t)h * (size_t)w * (size_t)c->cfg.channels * element_bytes(fmt->dtype);
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
    if (per_stream < 1 || per_stream > kCropMaxWindows)
        return fail(c, OATGPU_E_INVALID, "%s: 1..%d windows a stream (got %d)", what, kCropMaxWindows, per_stream);
    int rc = check_crop_size(c, what, h, w);
    if (rc) return rc;
    rc = check_fmt(c, what, fmt, out_dev);
    if (rc) return rc;
    if (c->ring_count || c->staged_count) return fail(c, OATGPU_E_INVALID, "%s while enqueued results are outstanding", what);
    rc = open_sync(c);
    if (rc) return rc;
    CropTensor &ct = c->tg.ct;
    const size_t n = (size_t)c->cfg.n_streams, count = n * (size_t)per_stream;
    if (!ct.win.host()) {                                   // built aside: a failed allocation leaves the context as it was
        HostMem<CropWin> table;
        if (table.alloc(n * kCropMaxWindows * sizeof(CropWin), hipHostMallocMapped) != hipSuccess)
            return fail(c, OATGPU_E_NOMEM, "%s: allocation failed: %s", what, hipGetErrorString(hipGetLastError()));
        ct.win = std::move(table);
    }
    memcpy(ct.win.host(), win, count * sizeof(CropWin));
    CropTensorLaunch a{};
    a.frames = (const uint8_t *)frames_dev;
    a.channels = c->cfg.channels;
    a.h = h; a.w = w; a.k = per_stream;
    a.win = ct.win.dev();
    a.out = (uint8_t *)out_dev;
    a.zoom = 1.0;                                           // (an explicit window carries its zoom in (ax, ay))
    fill(a, *fmt);
    launch_crop_tensor(c->g, a, fmt->dtype, (int)n, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OATGPU_OK;
}
