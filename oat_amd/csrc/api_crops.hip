// api_crops.hip -- target crops: a window of the input frame around every ranked blob of every camera.
// Crops ride on the slots of the motion and the subtraction tracker, whose front launches leave the slot's frame set
// there (tracker_front): tracker_tail launches k_target_crops (kernels_crops.hip) behind k_blob_rank and k_blob_shape on the same
// HIP stream, into the crop set that stands beside the slot's target set (TargetSets::crp); the slot's ev_done already follows the
// launch, and tracker_hand_out keeps the crop sets of what a call delivered beside its target sets.  oatgpu_crop_windows_dev is the
// same kernel on an explicit table of windows.  What crop tensors (api_croptensor.hip) do the same way is defined here, once.
#include "oatgpu_ctx.h"

static_assert(sizeof(oatgpu_crop_window) == sizeof(CropWin) && sizeof(CropWin) == 40, "k_target_crops reads oatgpu_crop_window's layout");
static_assert(OATGPU_CROP_MAX_SIDE == kCropMaxSide && OATGPU_CROP_MAX_WINDOWS == kCropMaxWindows, "the header's limits are the kernel's");

bool CropSets::alloc(size_t slots, size_t n_streams, int k, int h, int w, int channels)
{
    set_bytes = n_streams * (size_t)k * (size_t)h * (size_t)w * (size_t)channels;
    if (mem.alloc(slots * set_bytes, hipHostMallocMapped) != hipSuccess) return false;
    memset(mem.host(), 0, slots * set_bytes);
    return true;
}

// --- behind the ranking of a tracker's slot ---

// what both crop launches take from the slot: its frame set, target set and -- for windows along the body axis -- shape set
void crop_launch_from_slot(CropLaunch &a, const oatgpu_ctx *c, const BatchedTrackerState &bt, int slot, int mode, int h, int w)
{
    a.frames = bt.frame[slot];
    a.channels = c->cfg.channels;
    a.h = h; a.w = w; a.k = c->tg.k;
    a.axis = mode == OATGPU_CROP_AXIS;
    a.recs = bt.tgt.rec_dev(slot);
    a.shp = a.axis ? bt.tgt.shp.rec_dev(slot) : nullptr;
}

int crops_launch(oatgpu_ctx *c, const BatchedTrackerState &bt, int slot, hipStream_t st)
{
    const Targets &tg = c->tg;
    if (!tg.crop_mode) return OATGPU_OK;
    CropLaunch a{};
    crop_launch_from_slot(a, c, bt, slot, tg.crop_mode, tg.crop_h, tg.crop_w);
    a.out = bt.tgt.crp.set_dev(slot);
    launch_target_crops(c->g, a, c->cfg.n_streams, st);
    HIPCHK(c, hipGetLastError());
    return OATGPU_OK;
}

void crops_keep(oatgpu_ctx *c, const BatchedTrackerState &bt, int slot)
{
    if (c->tg.crop_mode) c->tg.last_crops.keep(bt.tgt.crp.set_bytes, bt.tgt.crp.set_host(slot));
}

// --- what the two switches and the two explicit calls share (what: the call, in the refusal's text) ---

int check_crop_mode(oatgpu_ctx *c, const char *what, int mode)
{
    if (mode != OATGPU_CROP_OFF && mode != OATGPU_CROP_UPRIGHT && mode != OATGPU_CROP_AXIS)
        return fail(c, OATGPU_E_INVALID, "%s: the mode must be OATGPU_CROP_OFF, _UPRIGHT or _AXIS (got %d)", what, mode);
    return OATGPU_OK;
}

int check_crop_size(oatgpu_ctx *c, const char *what, int h, int w)
{
    if (h < 1 || h > kCropMaxSide || w < 4 || w > kCropMaxSide || w % 4 != 0)
        return fail(c, OATGPU_E_INVALID, "%s: a window is 1..%d rows by 4..%d columns, the columns a multiple of 4 (got %d x %d)", what,
                    kCropMaxSide, kCropMaxSide, h, w);
    return OATGPU_OK;
}

// a zoom of crop tensors and of target masks
int check_crop_zoom(oatgpu_ctx *c, const char *what, double zoom)
{
    if (!(zoom >= 1.0 / 16 && zoom <= 16.0))          // (false for a NaN)
        return fail(c, OATGPU_E_INVALID, "%s: the zoom must be in 1/16 .. 16 (got %g)", what, zoom);
    return OATGPU_OK;
}

// what every switch that puts a window around a ranked blob needs of the target family
int check_window_riders(oatgpu_ctx *c, const char *what, int mode)
{
    if (!c->tg.k) return fail(c, OATGPU_E_INVALID, "%s: targets are off (oatgpu_set_targets)", what);
    if (mode == OATGPU_CROP_AXIS && !c->tg.shapes)
        return fail(c, OATGPU_E_INVALID, "%s: windows along the body axis need target shapes (oatgpu_set_target_shapes)", what);
    return OATGPU_OK;
}

// what the context must be for a crop switch to go on: that, and a front end whose frames are the caller's own (the windows are cut
// from the caller's frame set; target masks, cut from the tracker's own mask, do not share these two: api_targetmask.hip)
int check_crop_switch(oatgpu_ctx *c, const char *what, int mode)
{
    const int rc = check_window_riders(c, what, mode);
    if (rc) return rc;
    if (c->tb_on) return fail(c, OATGPU_E_INVALID, "%s with Bayer frames on (oatgpu_set_tracker_bayer) is not supported", what);
    if (c->tu_on) return fail(c, OATGPU_E_INVALID, "%s with undistortion on (oatgpu_set_tracker_undistort) is not supported", what);
    return OATGPU_OK;
}

int check_windows(oatgpu_ctx *c, const char *what, int per_stream, int h, int w)
{
    if (per_stream < 1 || per_stream > kCropMaxWindows)
        return fail(c, OATGPU_E_INVALID, "%s: 1..%d windows a stream (got %d)", what, kCropMaxWindows, per_stream);
    return check_crop_size(c, what, h, w);
}

int load_windows(oatgpu_ctx *c, const char *what, const oatgpu_crop_window *win, int per_stream)
{
    if (c->ring_count || c->staged_count) return fail(c, OATGPU_E_INVALID, "%s while enqueued results are outstanding", what);
    const int rc = open_sync(c);
    if (rc) return rc;
    const size_t n = (size_t)c->cfg.n_streams;
    if (!c->tg.win.host()) {
        HostMem<CropWin> table;
        if (table.alloc(n * kCropMaxWindows * sizeof(CropWin), hipHostMallocMapped) != hipSuccess)
            return fail(c, OATGPU_E_NOMEM, "%s: allocation failed: %s", what, hipGetErrorString(hipGetLastError()));
        c->tg.win = std::move(table);
    }
    memcpy(c->tg.win.host(), win, n * (size_t)per_stream * sizeof(CropWin));
    return OATGPU_OK;
}

void crop_launch_from_table(CropLaunch &a, const oatgpu_ctx *c, const void *frames_dev, int per_stream, int h, int w)
{
    a.frames = (const uint8_t *)frames_dev;
    a.channels = c->cfg.channels;
    a.h = h; a.w = w; a.k = per_stream;
    a.win = c->tg.win.dev();
}

// --- target crops ---

extern "C" int oatgpu_set_target_crops(oatgpu_ctx *c, int32_t mode, int32_t h, int32_t w)
{
    if (!c) return OATGPU_E_INVALID;
    const char *what = "set_target_crops";
    int rc = check_crop_mode(c, what, mode);
    if (!rc && mode != OATGPU_CROP_OFF) rc = check_crop_size(c, what, h, w);
    if (rc) return rc;
    if (c->ring_count || c->staged_count) return fail(c, OATGPU_E_INVALID, "%s while enqueued results are outstanding", what);
    if (mode != OATGPU_CROP_OFF && (rc = check_crop_switch(c, what, mode))) return rc;
    rc = open_sync(c);
    if (rc) return rc;
    Targets &tg = c->tg;
    if (mode == OATGPU_CROP_OFF) {
        tg.crop_mode = tg.crop_h = tg.crop_w = 0;
        tg.last_crops = {};
        for_each_target_home(c, [](TargetSets &ts, size_t, bool, bool) { ts.crp = {}; });
        return OATGPU_OK;
    }
    TargetWants wants = wants_of(c);
    wants.crop_mode = mode; wants.crop_h = h; wants.crop_w = w;
    rc = rebuild_target_sets(c, wants, "target crops");
    if (rc) return rc;
    tg.crop_mode = mode; tg.crop_h = h; tg.crop_w = w;
    targets_begin(c);                    // a target set kept from before has no crop set beside it
    tg.last_crops.items.reserve((size_t)c->cfg.n_streams * (size_t)tg.k * (size_t)h * (size_t)w * (size_t)c->cfg.channels);
    return OATGPU_OK;
}

extern "C" int oatgpu_target_crops(oatgpu_ctx *c, uint8_t *out, int32_t max_sets)
{
    if (!c || !out) return fail(c, OATGPU_E_INVALID, "null argument");
    return delivered_to(c, c->tg.last_crops, c->tg.crop_mode != 0, "target crops are off (oatgpu_set_target_crops)",
                        "no call has delivered a crop set since target crops were switched on", out, max_sets);
}

extern "C" int oatgpu_crop_windows_dev(oatgpu_ctx *c, const void *frames_dev, const oatgpu_crop_window *win, int32_t per_stream,
                                       int32_t h, int32_t w, uint8_t *out)
{
    if (!c) return OATGPU_E_INVALID;
    if (!frames_dev || !win || !out) return fail(c, OATGPU_E_INVALID, "null argument");
    int rc = check_windows(c, "crop_windows", per_stream, h, w);
    if (!rc) rc = load_windows(c, "crop_windows", win, per_stream);
    if (rc) return rc;
    Targets &tg = c->tg;
    const size_t n = (size_t)c->cfg.n_streams;
    const size_t bytes = n * (size_t)per_stream * (size_t)h * (size_t)w * (size_t)c->cfg.channels;
    if (tg.cw_bytes < bytes) {                               // built aside: a failed allocation leaves the context as it was
        HostMem<uint8_t> set;
        if (set.alloc(bytes, hipHostMallocMapped) != hipSuccess)
            return fail(c, OATGPU_E_NOMEM, "crop_windows: allocation failed: %s", hipGetErrorString(hipGetLastError()));
        tg.cw_out = std::move(set);
        tg.cw_bytes = bytes;
    }
    CropLaunch a{};
    crop_launch_from_table(a, c, frames_dev, per_stream, h, w);
    a.out = tg.cw_out.dev();
    launch_target_crops(c->g, a, (int)n, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memcpy(out, tg.cw_out.host(), bytes);
    return OATGPU_OK;
}
