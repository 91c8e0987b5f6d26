// api_crops.hip -- target crops: a window of the input frame around every ranked blob of every camera.
// While crops are on, targets_launch (api_targets.hip) launches k_target_crops (kernels_crops.hip) behind k_blob_rank and
// k_blob_shape on the same HIP stream, into the crop set that stands beside the slot's target set (TargetSets::crp) -- for the
// target sets of the motion and the subtraction tracker, whose front launches leave the slot's frame set there (tracker_front);
// the slot's ev_done already follows the launch.  targets_begin / targets_keep keep the crop sets of what a call delivered beside
// its target sets.  oatgpu_crop_windows_dev is the same kernel on an explicit table of windows.
#include "oatgpu_ctx.h"

static_assert(sizeof(oatgpu_crop_window) == sizeof(CropWin) && sizeof(CropWin) == 40, "k_target_crops reads oatgpu_crop_window's layout");
static_assert(kSeqSlots == 4, "CropSets::frame has one entry a slot");
static_assert(OATGPU_CROP_MAX_SIDE == kCropMaxSide && OATGPU_CROP_MAX_WINDOWS == kCropMaxWindows, "the header's limits are the kernel's");

bool CropSets::alloc(size_t slots, size_t n_streams, int k, int h, int w, int channels)
{
    set_bytes = n_streams * (size_t)k * (size_t)h * (size_t)w * (size_t)channels;
    if (mem.alloc(slots * set_bytes, hipHostMallocMapped) != hipSuccess) return false;
    memset(mem.host(), 0, slots * set_bytes);
    return true;
}

int crops_launch(oatgpu_ctx *c, const TargetSets &ts, int slot, int s0, int n, hipStream_t st)
{
    const Targets &tg = c->tg;
    if (!tg.crop_mode || !ts.crp.on()) return OATGPU_OK;
    const size_t k = (size_t)tg.k, win_bytes = (size_t)tg.crop_h * tg.crop_w * c->cfg.channels;
    CropLaunch a{};
    a.frames = ts.crp.frame[slot] + (size_t)s0 * c->g.H * c->g.W * c->cfg.channels;
    a.channels = c->cfg.channels;
    a.h = tg.crop_h; a.w = tg.crop_w; a.k = tg.k;
    a.axis = tg.crop_mode == OATGPU_CROP_AXIS;
    a.recs = ts.rec_dev(slot) + (size_t)s0 * k;
    a.shp = a.axis ? ts.shp.rec_dev(slot) + (size_t)s0 * k : nullptr;
    a.out = ts.crp.set_dev(slot) + (size_t)s0 * k * win_bytes;
    launch_target_crops(c->g, a, n, st);
    HIPCHK(c, hipGetLastError());
    return OATGPU_OK;
}

void crops_begin(oatgpu_ctx *c) { c->tg.last_crop_sets = 0; }

void crops_keep(oatgpu_ctx *c, const TargetSets &ts, int slot)
{
    Targets &tg = c->tg;
    if (!tg.crop_mode || !ts.crp.on()) return;
    const size_t at = (size_t)tg.last_crop_sets, bytes = ts.crp.set_bytes;
    tg.last_crops.resize((at + 1) * bytes);
    memcpy(tg.last_crops.data() + at * bytes, ts.crp.set_host(slot), bytes);
    tg.last_crop_sets++;
}

int check_crop_size(oatgpu_ctx *c, const char *what, int h, int w)
{
    if (h < 1 || h > kCropMaxSide || w < 4 || w > kCropMaxSide || w % 4 != 0)
        return fail(c, OATGPU_E_INVALID, "%s: a window is 1..%d rows by 4..%d columns, the columns a multiple of 4 (got %d x %d)", what,
                    kCropMaxSide, kCropMaxSide, h, w);
    return OATGPU_OK;
}

extern "C" int oatgpu_set_target_crops(oatgpu_ctx *c, int32_t mode, int32_t h, int32_t w)
{
    if (!c) return OATGPU_E_INVALID;
    if (mode != OATGPU_CROP_OFF && mode != OATGPU_CROP_UPRIGHT && mode != OATGPU_CROP_AXIS)
        return fail(c, OATGPU_E_INVALID, "set_target_crops: the mode must be OATGPU_CROP_OFF, _UPRIGHT or _AXIS (got %d)", mode);
    if (mode != OATGPU_CROP_OFF) {
        const int rc = check_crop_size(c, "set_target_crops", h, w);
        if (rc) return rc;
    }
    if (c->ring_count || c->staged_count) return fail(c, OATGPU_E_INVALID, "set_target_crops while enqueued results are outstanding");
    Targets &tg = c->tg;
    if (mode != OATGPU_CROP_OFF) {
        if (!tg.k) return fail(c, OATGPU_E_INVALID, "set_target_crops: targets are off (oatgpu_set_targets)");
        if (mode == OATGPU_CROP_AXIS && !tg.shapes)
            return fail(c, OATGPU_E_INVALID, "set_target_crops: windows along the body axis need target shapes (oatgpu_set_target_shapes)");
        if (c->tb_on) return fail(c, OATGPU_E_INVALID, "set_target_crops with Bayer frames on (oatgpu_set_tracker_bayer) is not supported");
        if (c->tu_on) return fail(c, OATGPU_E_INVALID, "set_target_crops with undistortion on (oatgpu_set_tracker_undistort) is not supported");
    }
    const int rc = open_sync(c);
    if (rc) return rc;
    if (mode == OATGPU_CROP_OFF) {
        tg.crop_mode = tg.crop_h = tg.crop_w = 0;
        tg.last_crop_sets = 0;
        tg.last_crops = {};
        c->df.tgt.crp = {}; c->bs.tgt.crp = {};
        return OATGPU_OK;
    }
    // everything is built aside: a failed allocation leaves the context as it was
    const size_t n = (size_t)c->cfg.n_streams;
    CropSets df, bs;
    bool ok = !c->df.on || df.alloc(kSeqSlots, n, tg.k, h, w, c->cfg.channels);
    ok = ok && (!c->bs.on || bs.alloc(kSeqSlots, n, tg.k, h, w, c->cfg.channels));
    if (!ok) return fail(c, OATGPU_E_NOMEM, "target crops: allocation failed: %s", hipGetErrorString(hipGetLastError()));
    c->df.tgt.crp = std::move(df);
    c->bs.tgt.crp = std::move(bs);
    tg.crop_mode = mode; tg.crop_h = h; tg.crop_w = w;
    // the lists start over, for targets and shapes too: a target set kept from before has no crop set beside it
    tg.last_sets = 0;
    tg.last_shapes.clear();
    tg.last_crop_sets = 0;
    tg.last_crops.clear();
    tg.last_crops.reserve(n * (size_t)tg.k * (size_t)h * (size_t)w * (size_t)c->cfg.channels);
    return OATGPU_OK;
}

extern "C" int oatgpu_target_crops(oatgpu_ctx *c, uint8_t *out, int32_t max_sets)
{
    if (!c || !out) return fail(c, OATGPU_E_INVALID, "null argument");
    const Targets &tg = c->tg;
    if (!tg.crop_mode) return fail(c, OATGPU_E_INVALID, "target crops are off (oatgpu_set_target_crops)");
    if (tg.last_crop_sets == 0) return fail(c, OATGPU_E_INVALID, "no call has delivered a crop set since target crops were switched on");
    if (max_sets < tg.last_crop_sets)
        return fail(c, OATGPU_E_INVALID, "room for %d frame sets, the latest call delivered %d", max_sets, tg.last_crop_sets);
    memcpy(out, tg.last_crops.data(), tg.last_crops.size());
    return tg.last_crop_sets;
}

extern "C" int oatgpu_crop_windows_dev(oatgpu_ctx *c, const void *frames_dev, const oatgpu_crop_window *win, int32_t per_stream,
                                       int32_t h, int32_t w, uint8_t *out)
{
    if (!c) return OATGPU_E_INVALID;
    if (!frames_dev || !win || !out) return fail(c, OATGPU_E_INVALID, "null argument");
    if (per_stream < 1 || per_stream > kCropMaxWindows)
        return fail(c, OATGPU_E_INVALID, "crop_windows: 1..%d windows a stream (got %d)", kCropMaxWindows, per_stream);
    int rc = check_crop_size(c, "crop_windows", h, w);
    if (rc) return rc;
    if (c->ring_count || c->staged_count) return fail(c, OATGPU_E_INVALID, "crop_windows while enqueued results are outstanding");
    rc = open_sync(c);
    if (rc) return rc;
    Targets &tg = c->tg;
    const size_t n = (size_t)c->cfg.n_streams, count = n * (size_t)per_stream;
    const size_t bytes = count * (size_t)h * (size_t)w * (size_t)c->cfg.channels;
    if (!tg.cw_win.host() || tg.cw_bytes < bytes) {          // built aside: a failed allocation leaves the context as it was
        HostMem<CropWin> table;
        HostMem<uint8_t> set;
        if (table.alloc(n * kCropMaxWindows * sizeof(CropWin), hipHostMallocMapped) != hipSuccess ||
            set.alloc(bytes, hipHostMallocMapped) != hipSuccess)
            return fail(c, OATGPU_E_NOMEM, "crop_windows: allocation failed: %s", hipGetErrorString(hipGetLastError()));
        tg.cw_win = std::move(table);
        tg.cw_out = std::move(set);
        tg.cw_bytes = bytes;
    }
    memcpy(tg.cw_win.host(), win, count * sizeof(CropWin));
    CropLaunch a{};
    a.frames = (const uint8_t *)frames_dev;
    a.channels = c->cfg.channels;
    a.h = h; a.w = w; a.k = per_stream;
    a.win = tg.cw_win.dev();
    a.out = tg.cw_out.dev();
    launch_target_crops(c->g, a, (int)n, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memcpy(out, tg.cw_out.host(), bytes);
    return OATGPU_OK;
}
