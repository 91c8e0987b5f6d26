// api_stages.hip -- the single-stage calls: one `framefilt` / `posidet` component a call, and the taps.
#include "oatgpu_ctx.h"

// the input of a single-stage call on its way to the device; deferred: with an event behind it
static int stage_in(oatgpu_ctx *c, void *dst, const void *src, size_t bytes)
{
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    if (c->deferred) {
        if (!c->ev_h2d) HIPCHK(c, c->ev_h2d.create(hipEventDisableTiming | hipEventDisableSystemFence));
        HIPCHK(c, hipEventRecord(c->ev_h2d, c->stream));
    }
    return OATGPU_OK;
}
// the output frame of a single-stage call: copied out and waited for -- or, deferred, left on the device once the INPUT
// has been read (FrameFilter.cpp:73-80: the reference posts its SOURCE right after its memcpy)
static int finish_frame(oatgpu_ctx *c, uint8_t *out, const uint8_t *dev, size_t bytes)
{
    if (c->deferred) {
        HIPCHK(c, hipEventSynchronize(c->ev_h2d));
        c->defer_kind = 1; c->defer_dev = dev; c->defer_bytes = bytes;       // (only once the wait succeeded: a failed call owes no fetch)
        return OATGPU_OK;
    }
    HIPCHK(c, hipMemcpyAsync(out, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OATGPU_OK;
}

extern "C" int oatgpu_fetch_frame(oatgpu_ctx *c, uint8_t *out)
{
    if (!c || !out) return fail(c, OATGPU_E_INVALID, "null argument");
    if (c->defer_kind != 1) return fail(c, OATGPU_E_INVALID, "no deferred frame is waiting");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipMemcpyAsync(out, c->defer_dev, c->defer_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->defer_kind = 0;                  // (cleared once the frame has arrived: a failed fetch can be repeated)
    return OATGPU_OK;
}

static int mog_single(oatgpu_ctx *c, int s, const uint8_t *bgr_in, uint8_t *mask_out, uint8_t *bgr_out, double lr)
{
    int rc = check_stream_ix(c, s);
    if (rc) return rc;
    if (!bgr_in) return fail(c, OATGPU_E_INVALID, "null frame");
    rc = open_sync(c);
    if (rc) return rc;
    const size_t npx = (size_t)c->g.H * c->g.W;
    const size_t ch = c->cfg.channels;
    uint8_t *slot = c->frames + (size_t)s * npx * ch;
    rc = stage_in(c, slot, bgr_in, npx * ch);
    if (rc) return rc;
    const Rate r = mog_begin(c, s, lr);
    MogLaunch a = mog_launch_base(c, c->frames, r);
    a.out_base = s;
    if (mask_out) a.out_mask = c->aux_a;
    if (bgr_out) a.out_bgr = c->aux_b;
    launch_mog_fused(c->g, a, s, 1, c->stream, nullptr, mog_launch_opts(c, s, s + 1, 256));
    HIPCHK(c, hipGetLastError());
    if (bgr_out && !mask_out) return finish_frame(c, bgr_out, c->aux_b, npx * ch);       // (deferrable: the filter form)
    if (mask_out) HIPCHK(c, hipMemcpyAsync(mask_out, c->aux_a, npx, hipMemcpyDeviceToHost, c->stream));
    if (bgr_out) HIPCHK(c, hipMemcpyAsync(bgr_out, c->aux_b, npx * ch, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OATGPU_OK;
}

extern "C" int oatgpu_set_kalman(oatgpu_ctx *c, int32_t enable, double dt, double timeout, double sigma_accel,
                                 double sigma_noise)
{
    if (!c) return OATGPU_E_INVALID;
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (c->ring_count) return fail(c, OATGPU_E_INVALID, "set_kalman while enqueued results are outstanding");
    if (enable && c->mkp.on)
        return fail(c, OATGPU_E_INVALID, "the marker pipeline is on and does not take the position filter: oatgpu_set_marker_pipeline(0) first");
    int rc = quiesce(c);
    if (rc) return rc;
    if (!enable) { c->kal_on = false; return OATGPU_OK; }
    if (!(dt > 0) || !(timeout >= 0) || !(sigma_accel >= 0) || !(sigma_noise >= 0) || !(timeout / dt < 2147483647.0))
        return fail(c, OATGPU_E_INVALID, "kalman: dt must be > 0, timeout / sigma-accel / sigma-noise >= 0");
    if (!c->kal_state) HIPCHK(c, c->kal_state.alloc((size_t)c->cfg.n_streams * sizeof(KalmanState)));
    c->kal.state = c->kal_state;
    c->kal.dt = dt; c->kal.sig_accel = sigma_accel; c->kal.sig_noise = sigma_noise;
    c->kal.threshold = (int)(timeout / dt);                     // KalmanFilter2D.cpp:74-76
    launch_kalman_reset(c->kal.state, c->cfg.n_streams, c->kal_ticket, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->kal_on = true;
    return OATGPU_OK;
}

extern "C" int oatgpu_set_homography(oatgpu_ctx *c, int32_t enable, const double *h9)
{
    if (!c) return OATGPU_E_INVALID;
    if (enable && !h9) return fail(c, OATGPU_E_INVALID, "null homography");
    if (c->ring_count) return fail(c, OATGPU_E_INVALID, "set_homography while enqueued results are outstanding");
    if (enable && c->mkp.on)
        return fail(c, OATGPU_E_INVALID, "the marker pipeline is on and does not take a homography: oatgpu_set_marker_pipeline(0) first");
    c->homo_on = enable != 0;
    if (enable) for (int i = 0; i < 9; ++i) c->homo[i] = h9[i];
    return OATGPU_OK;
}

extern "C" int oatgpu_set_roi_mask(oatgpu_ctx *c, int32_t s, const uint8_t *roi_mask)
{
    int rc = check_stream_ix(c, s);
    if (rc) return rc;
    rc = open_sync(c);
    if (rc) return rc;
    const Geom &g = c->g;
    const size_t NW = g.Palloc >> 6, n = c->cfg.n_streams, npx = (size_t)g.H * g.W;
    if (!c->roi) {
        if (!roi_mask) return OATGPU_OK;                       // nothing to clear
        HIPCHK(c, c->roi.alloc(n * NW * 8));
        HIPCHK(c, hipMemsetAsync(c->roi, 0xff, n * NW * 8, c->stream));   // other streams keep everything
    }
    if (!roi_mask) {
        HIPCHK(c, hipMemsetAsync(c->roi + (size_t)s * NW, 0xff, NW * 8, c->stream));
    } else {
        HIPCHK(c, hipMemcpyAsync(c->aux_a, roi_mask, npx, hipMemcpyHostToDevice, c->stream));
        launch_pack_bits(g, c->aux_a, c->roi + (size_t)s * NW, c->stream);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OATGPU_OK;
}

extern "C" int oatgpu_mog_apply(oatgpu_ctx *c, int32_t s, const uint8_t *bgr_in, uint8_t *fgmask_out, double lr)
{
    if (!fgmask_out) return fail(c, OATGPU_E_INVALID, "null mask buffer");
    return mog_single(c, s, bgr_in, fgmask_out, nullptr, lr);
}

extern "C" int oatgpu_mog_filter(oatgpu_ctx *c, int32_t s, const uint8_t *bgr_in, uint8_t *bgr_out, double lr)
{
    if (!bgr_out) return fail(c, OATGPU_E_INVALID, "null output frame");
    return mog_single(c, s, bgr_in, nullptr, bgr_out, lr);
}

// framefilt bsub's background and its fp32 accumulator, made on first use
int ensure_bsub(oatgpu_ctx *c, size_t nb)
{
    if (c->bsub_bg) return OATGPU_OK;
    DevMem<uint8_t> bg; DevMem<float> f;
    HIPCHK(c, bg.alloc((size_t)c->cfg.n_streams * nb));
    HIPCHK(c, f.alloc((size_t)c->cfg.n_streams * nb * sizeof(float)));
    c->bsub_bg = std::move(bg); c->bsub_f = std::move(f);
    return OATGPU_OK;
}

extern "C" int oatgpu_bsub_filter(oatgpu_ctx *c, int32_t s, const uint8_t *in, uint8_t *out, double alpha)
{
    int rc = check_stream_ix(c, s);
    if (rc) return rc;
    if (!in || !out) return fail(c, OATGPU_E_INVALID, "null argument");
    if (!(alpha >= 0.0 && alpha <= 1.0)) return fail(c, OATGPU_E_INVALID, "adaptation-coeff must be in [0,1]");
    rc = open_sync(c);
    if (rc) return rc;
    const size_t nb = (size_t)c->g.H * c->g.W * c->cfg.channels;
    { const int arc = ensure_bsub(c, nb); if (arc) return arc; }
    if (c->bsub_have[s] == 2 && alpha > 0.0)        // the reference's accumulateWeighted asserts on its empty fp32 image
        return fail(c, OATGPU_E_INVALID, "a background image from a file cannot adapt (adaptation-coeff must be 0)");
    rc = stage_in(c, c->aux_a, in, nb);
    if (rc) return rc;
    const float a = (float)alpha, b = 1 - a;              // accW_: AT a = (AT)alpha, b = 1 - a
    launch_bsub(c->aux_a, c->aux_b, c->bsub_bg + (size_t)s * nb, c->bsub_f + (size_t)s * nb, nb, a, b,
                c->bsub_have[s] ? 0 : 1, alpha > 0.0 ? 1 : 0, c->stream);
    HIPCHK(c, hipGetLastError());
    if (!c->bsub_have[s]) c->bsub_have[s] = 1;
    return finish_frame(c, out, c->aux_b, nb);
}

extern "C" int oatgpu_bsub_set_background(oatgpu_ctx *c, int32_t s, const uint8_t *image)
{
    int rc = check_stream_ix(c, s);
    if (rc) return rc;
    if (!image) return fail(c, OATGPU_E_INVALID, "null argument");
    rc = open_sync(c);
    if (rc) return rc;
    const size_t nb = (size_t)c->g.H * c->g.W * c->cfg.channels;
    { const int arc = ensure_bsub(c, nb); if (arc) return arc; }
    HIPCHK(c, hipMemcpyAsync(c->bsub_bg + (size_t)s * nb, image, nb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->bsub_have[s] = 2;          // from a file: the fp32 accumulator does not exist (BackgroundSubtractor.cpp:63-71)
    return OATGPU_OK;
}

extern "C" int oatgpu_mask_filter(oatgpu_ctx *c, int32_t s, const uint8_t *in, uint8_t *out)
{
    int rc = check_stream_ix(c, s);
    if (rc) return rc;
    if (!in || !out) return fail(c, OATGPU_E_INVALID, "null argument");
    rc = open_sync(c);
    if (rc) return rc;
    const size_t nb = (size_t)c->g.H * c->g.W * c->cfg.channels;
    if (!c->roi) {                                   // no mask set: FrameMasker::filter leaves the frame alone
        if (c->deferred) {                           // (through the device, so that the fetch finds it)
            rc = stage_in(c, c->aux_b, in, nb);
            return rc ? rc : finish_frame(c, out, c->aux_b, nb);
        }
        if (out != in) memcpy(out, in, nb);
        return OATGPU_OK;
    }
    rc = stage_in(c, c->aux_a, in, nb);
    if (rc) return rc;
    launch_apply_roi(c->g, c->aux_a, c->aux_b, c->cfg.channels, c->roi + (size_t)s * (c->g.Palloc >> 6), c->stream);
    HIPCHK(c, hipGetLastError());
    return finish_frame(c, out, c->aux_b, nb);
}

extern "C" int oatgpu_thresh_filter(oatgpu_ctx *c, const uint8_t *in, uint8_t *out, int32_t i_min, int32_t i_max)
{
    if (!c || !in || !out) return fail(c, OATGPU_E_INVALID, "null argument");
    if (i_min < 0 || i_min > 256 || i_max < 0 || i_max > 256)      // Threshold.cpp:62-63
        return fail(c, OATGPU_E_INVALID, "Values of intensity should be between 0 and 256.");
    int rc = open_sync(c);
    if (rc) return rc;
    const size_t npx = (size_t)c->g.H * c->g.W, nb = npx * c->cfg.channels;
    int lo, hi;
    norm_range(i_min, i_max, lo, hi);
    rc = stage_in(c, c->aux_a, in, nb);
    if (rc) return rc;
    launch_thresh_filter(c->aux_a, c->aux_b, npx, c->cfg.channels, lo, hi, c->stream);
    HIPCHK(c, hipGetLastError());
    return finish_frame(c, out, c->aux_b, nb);
}

// ------------------------------------------------------- framefilt undistort (Undistorter.cpp:83-88) ----

static int check_undistort_args(oatgpu_ctx *c, const double *K, const double *dist, int n_dist)
{
    const char *why = nullptr;
    if (!K || !dist) return fail(c, OATGPU_E_INVALID, "null argument");
    if (undistort_check_coeffs(n_dist, &why)) return fail(c, OATGPU_E_INVALID, "%s", why);
    return OATGPU_OK;
}

extern "C" int oatgpu_undistort_map(int32_t rows, int32_t cols, const double K[9], const double *dist, int32_t n_dist,
                                    int16_t *map1, uint16_t *map2)
{
    if (rows < 1 || cols < 1) return fail(nullptr, OATGPU_E_INVALID, "rows and cols must be >= 1");
    if (!map1 || !map2) return fail(nullptr, OATGPU_E_INVALID, "null argument");
    const int rc = check_undistort_args(nullptr, K, dist, n_dist);
    if (rc) return rc;
    undistort_build_map(rows, cols, K, dist, n_dist, map1, map2);
    return OATGPU_OK;
}

extern "C" int oatgpu_set_undistort(oatgpu_ctx *c, int32_t s, const double K[9], const double *dist, int32_t n_dist)
{
    int rc = check_stream_ix(c, s);
    if (rc) return rc;
    if (n_dist == 0) {
        if (c->ud_track)                // (the fused track calls remap every stream: each needs its map while the switch is on)
            return fail(c, OATGPU_E_INVALID, "stream %d: the map cannot be removed while the tracker undistorts (oatgpu_set_track_undistort)", s);
        if (c->tu_on)                   // (and so do the motion and the subtraction tracker's front kernels)
            return fail(c, OATGPU_E_INVALID, "stream %d: the map cannot be removed while the diff and bsub trackers undistort (oatgpu_set_tracker_undistort)", s);
        c->ud_have[(size_t)s] = 0;      // (nothing on the device reads a stream without a map)
        return OATGPU_OK;
    }
    rc = check_undistort_args(c, K, dist, n_dist);
    if (rc) return rc;
    const Geom &g = c->g;
    const size_t npx = (size_t)g.H * g.W, n = c->cfg.n_streams;
    std::vector<int16_t> m1(npx * 2);
    std::vector<uint16_t> m2(npx);
    undistort_build_map(g.H, g.W, K, dist, n_dist, m1.data(), m2.data());
    rc = open_sync(c);                  // an undistortion still in flight may be reading the old map
    if (rc) return rc;
    if (!c->ud_map1) {                  // first use: both maps built aside, moved in when everything worked
        const size_t stride = undistort_map_stride(g.H, g.W);
        DevMem<uint32_t> map1; DevMem<uint16_t> map2;
        HIPCHK(c, map1.alloc(n * stride * sizeof(uint32_t)));
        if (map2.alloc(n * stride * sizeof(uint16_t)) != hipSuccess)
            return fail(c, OATGPU_E_NOMEM, "device allocation of the undistortion maps failed");
        HIPCHK(c, hipMemsetAsync(map1, 0, n * stride * sizeof(uint32_t), c->stream));   // (the padding is read)
        HIPCHK(c, hipMemsetAsync(map2, 0, n * stride * sizeof(uint16_t), c->stream));
        c->ud_stride = stride; c->ud_map1 = std::move(map1); c->ud_map2 = std::move(map2);
    }
    HIPCHK(c, hipMemcpyAsync(c->ud_map1 + (size_t)s * c->ud_stride, m1.data(), npx * sizeof(uint32_t), hipMemcpyHostToDevice,
                             c->stream));
    HIPCHK(c, hipMemcpyAsync(c->ud_map2 + (size_t)s * c->ud_stride, m2.data(), npx * sizeof(uint16_t), hipMemcpyHostToDevice,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->ud_have[(size_t)s] = 1;
    return OATGPU_OK;
}

extern "C" int oatgpu_set_track_undistort(oatgpu_ctx *c, int32_t on)
{
    if (!c) return OATGPU_E_INVALID;
    if (on != 0 && on != 1) return fail(c, OATGPU_E_INVALID, "track undistort must be 0 (off) or 1 (on)");
    if (on)
        for (int s = 0; s < c->cfg.n_streams; ++s)
            if (!c->ud_have[(size_t)s]) return fail(c, OATGPU_E_INVALID, "stream %d has no undistortion map (oatgpu_set_undistort)", s);
    const int rc = open_sync(c);        // frames registered or in flight were handed over under the old setting
    if (rc) return rc;
    if (on && !c->ud_frames[0]) {       // (allocated here, never in the middle of a step)
        const size_t sb = (size_t)c->g.H * c->g.W * c->cfg.channels * c->cfg.n_streams;
        DevMem<uint8_t> fr[2];
        if (fr[0].alloc(sb) != hipSuccess || fr[1].alloc(sb) != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, OATGPU_E_NOMEM, "device allocation of the undistorted-frame buffers (2 x %zu bytes) failed", sb);
        }
        c->ud_frames[0] = std::move(fr[0]); c->ud_frames[1] = std::move(fr[1]);
    }
    c->ud_track = on != 0;
    return OATGPU_OK;
}

// The motion and the subtraction tracker on distorted frames (api_diff.hip, api_bsubtrack.hip): their front kernels remap in
// registers with the maps of oatgpu_set_undistort, so the switch is a flag alone -- no buffer, and the trackers' state stays in
// the undistorted domain.
extern "C" int oatgpu_set_tracker_undistort(oatgpu_ctx *c, int32_t on)
{
    if (!c) return OATGPU_E_INVALID;
    if (on != 0 && on != 1) return fail(c, OATGPU_E_INVALID, "tracker undistort must be 0 (off) or 1 (on)");
    if (on) {
        for (int s = 0; s < c->cfg.n_streams; ++s)
            if (!c->ud_have[(size_t)s]) return fail(c, OATGPU_E_INVALID, "stream %d has no undistortion map (oatgpu_set_undistort)", s);
        if (c->tb_on)
            return fail(c, OATGPU_E_INVALID, "set_tracker_undistort with Bayer frames on (oatgpu_set_tracker_bayer) is not supported");
        if (c->tg.crop_mode)
            return fail(c, OATGPU_E_INVALID, "set_tracker_undistort with target crops on (oatgpu_set_target_crops) is not supported");
        if (c->tg.ct.mode)
            return fail(c, OATGPU_E_INVALID, "set_tracker_undistort with crop tensors on (oatgpu_set_target_crop_tensor) is not supported");
    }
    if (c->ring_count) return fail(c, OATGPU_E_INVALID, "set_tracker_undistort while enqueued results are outstanding");
    if (c->staged_count)
        return fail(c, OATGPU_E_INVALID, "set_tracker_undistort while a frame set is being staged (oatgpu_track_stage): finish it with oatgpu_track_enqueue_staged or give it up");
    c->tu_on = on != 0;
    return OATGPU_OK;
}

extern "C" int oatgpu_undistort_filter(oatgpu_ctx *c, int32_t s, const uint8_t *in, uint8_t *out)
{
    int rc = check_stream_ix(c, s);
    if (rc) return rc;
    if (!in || !out) return fail(c, OATGPU_E_INVALID, "null argument");
    if (!c->ud_have[(size_t)s]) return fail(c, OATGPU_E_INVALID, "stream %d has no undistortion map (oatgpu_set_undistort)", s);
    rc = open_sync(c);
    if (rc) return rc;
    const size_t nb = (size_t)c->g.H * c->g.W * c->cfg.channels;
    rc = stage_in(c, c->aux_a, in, nb);             // (the reference clones first: out == in is fine, the kernel reads aux_a)
    if (rc) return rc;
    launch_undistort(c->aux_a, c->aux_b, c->ud_map1 + (size_t)s * c->ud_stride, c->ud_map2 + (size_t)s * c->ud_stride,
                     c->ud_stride, c->g.H, c->g.W, c->cfg.channels, 1, c->stream);
    HIPCHK(c, hipGetLastError());
    return finish_frame(c, out, c->aux_b, nb);
}

extern "C" int oatgpu_undistort_dev(oatgpu_ctx *c, const void *frames_dev, void *out_dev)
{
    if (!c) return OATGPU_E_INVALID;
    if (!frames_dev || !out_dev) return fail(c, OATGPU_E_INVALID, "null argument");
    if (frames_dev == out_dev) return fail(c, OATGPU_E_INVALID, "undistort_dev cannot work in place");
    for (int s = 0; s < c->cfg.n_streams; ++s)
        if (!c->ud_have[(size_t)s]) return fail(c, OATGPU_E_INVALID, "stream %d has no undistortion map (oatgpu_set_undistort)", s);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    launch_undistort((const uint8_t *)frames_dev, (uint8_t *)out_dev, c->ud_map1, c->ud_map2, c->ud_stride, c->g.H, c->g.W,
                     c->cfg.channels, c->cfg.n_streams, c->stream);
    HIPCHK(c, hipGetLastError());
    return OATGPU_OK;
}

// ------------------------------------- Bayer RAW8 -> BGR (the frame server's conversion, PointGreyCam.cpp:48-50, :729) ----

static int check_bayer_args(oatgpu_ctx *c, const int32_t *patterns, int n_patterns)
{
    if (c->g.H < 3 || c->g.W < 3) return fail(c, OATGPU_E_INVALID, "demosaicing needs frames of at least 3 x 3 pixels (have %d x %d)", c->g.H, c->g.W);
    if (!patterns) return fail(c, OATGPU_E_INVALID, "null argument");
    if (n_patterns != 1 && n_patterns != c->cfg.n_streams)
        return fail(c, OATGPU_E_INVALID, "%d Bayer patterns for %d streams (give one, or one a stream)", n_patterns, c->cfg.n_streams);
    for (int i = 0; i < n_patterns; ++i)
        if (patterns[i] < OATGPU_BAYER_RGGB || patterns[i] > OATGPU_BAYER_GBRG)
            return fail(c, OATGPU_E_INVALID, "Bayer pattern %d (stream %d) is not one of 1 RGGB, 2 BGGR, 3 GRBG, 4 GBRG", patterns[i], i);
    return OATGPU_OK;
}

extern "C" int oatgpu_debayer_filter(oatgpu_ctx *c, int32_t pattern, const uint8_t *raw_in, uint8_t *bgr_out)
{
    if (!c) return OATGPU_E_INVALID;
    if (!raw_in || !bgr_out) return fail(c, OATGPU_E_INVALID, "null argument");
    int rc = check_bayer_args(c, &pattern, 1);
    if (rc) return rc;
    rc = open_sync(c);
    if (rc) return rc;
    const size_t npx = (size_t)c->g.H * c->g.W;
    rc = stage_in(c, c->aux_a, raw_in, npx);
    if (rc) return rc;
    const uint8_t *in[1] = {c->aux_a};
    uint8_t *const out[1] = {c->aux_b};
    const int pat[1] = {pattern};
    launch_debayer_frames(in, out, 1, pat, c->g.H, c->g.W, 1, c->stream);
    HIPCHK(c, hipGetLastError());
    return finish_frame(c, bgr_out, c->aux_b, npx * 3);
}

extern "C" int oatgpu_debayer_dev(oatgpu_ctx *c, const int32_t *patterns, int32_t n_patterns, const void *raw_dev, void *bgr_dev)
{
    if (!c) return OATGPU_E_INVALID;
    if (!raw_dev || !bgr_dev) return fail(c, OATGPU_E_INVALID, "null argument");
    if (raw_dev == bgr_dev) return fail(c, OATGPU_E_INVALID, "debayer_dev cannot work in place");
    { const int rc = check_bayer_args(c, patterns, n_patterns); if (rc) return rc; }
    HIPCHK(c, hipSetDevice(c->cfg.device));
    std::vector<int> pat((size_t)c->cfg.n_streams);
    for (int s = 0; s < c->cfg.n_streams; ++s) pat[(size_t)s] = patterns[n_patterns == 1 ? 0 : s];
    const uint8_t *in[1] = {(const uint8_t *)raw_dev};
    uint8_t *const out[1] = {(uint8_t *)bgr_dev};
    launch_debayer_frames(in, out, 1, pat.data(), c->g.H, c->g.W, c->cfg.n_streams, c->stream);
    HIPCHK(c, hipGetLastError());
    return OATGPU_OK;
}

extern "C" int oatgpu_set_track_bayer(oatgpu_ctx *c, const int32_t *patterns, int32_t n_patterns)
{
    if (!c) return OATGPU_E_INVALID;
    const bool on = patterns != nullptr || n_patterns != 0;
    if (on) {
        if (c->cfg.channels != 3) return fail(c, OATGPU_E_INVALID, "Bayer frames need a BGR context (channels = 3, have %d)", c->cfg.channels);
        const int rc = check_bayer_args(c, patterns, n_patterns);
        if (rc) return rc;
    }
    // (the staged copies were sized under the old setting)
    if (c->staged_count)
        return fail(c, OATGPU_E_INVALID, "a frame set is being staged (oatgpu_track_stage): finish it with oatgpu_track_enqueue_staged or give it up");
    const int rc = open_sync(c);        // frames registered or in flight were handed over under the old setting
    if (rc) return rc;
    if (on && !c->by_frames[0]) {       // (allocated here, never in the middle of a step)
        const size_t sb = (size_t)c->g.H * c->g.W * 3 * c->cfg.n_streams;
        DevMem<uint8_t> fr[2];
        if (fr[0].alloc(sb) != hipSuccess || fr[1].alloc(sb) != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, OATGPU_E_NOMEM, "device allocation of the demosaiced-frame buffers (2 x %zu bytes) failed", sb);
        }
        c->by_frames[0] = std::move(fr[0]); c->by_frames[1] = std::move(fr[1]);
    }
    if (on) {
        c->by_pat.resize((size_t)c->cfg.n_streams);
        for (int s = 0; s < c->cfg.n_streams; ++s) c->by_pat[(size_t)s] = patterns[n_patterns == 1 ? 0 : s];
    }
    c->by_track = on;
    return OATGPU_OK;
}

// The motion and the subtraction tracker on RAW8 frames (api_diff.hip, api_bsubtrack.hip): their front kernels demosaic in
// registers, so the switch is the pattern table alone -- no buffer, and the trackers' state stays in the demosaiced domain.
extern "C" int oatgpu_set_tracker_bayer(oatgpu_ctx *c, const int32_t *patterns, int32_t n_patterns)
{
    if (!c) return OATGPU_E_INVALID;
    const bool on = patterns != nullptr || n_patterns != 0;
    std::vector<int> pat;               // built aside: the context takes it when nothing was refused
    if (on) {
        if (c->cfg.channels != 3) return fail(c, OATGPU_E_INVALID, "Bayer frames need a BGR context (channels = 3, have %d)", c->cfg.channels);
        const int rc = check_bayer_args(c, patterns, n_patterns);
        if (rc) return rc;
        if (c->tu_on)                   // (the gather would demosaic four corners a pixel)
            return fail(c, OATGPU_E_INVALID, "set_tracker_bayer with undistortion on (oatgpu_set_tracker_undistort) is not supported");
        if (c->tg.crop_mode)
            return fail(c, OATGPU_E_INVALID, "set_tracker_bayer with target crops on (oatgpu_set_target_crops) is not supported");
        if (c->tg.ct.mode)
            return fail(c, OATGPU_E_INVALID, "set_tracker_bayer with crop tensors on (oatgpu_set_target_crop_tensor) is not supported");
        pat.resize((size_t)c->cfg.n_streams);
        for (int s = 0; s < c->cfg.n_streams; ++s) pat[(size_t)s] = patterns[n_patterns == 1 ? 0 : s];
    }
    if (c->ring_count) return fail(c, OATGPU_E_INVALID, "set_tracker_bayer while enqueued results are outstanding");
    if (c->staged_count)
        return fail(c, OATGPU_E_INVALID, "set_tracker_bayer while a frame set is being staged (oatgpu_track_stage): finish it with oatgpu_track_enqueue_staged or give it up");
    c->tb_pat = std::move(pat);
    c->tb_on = on;
    return OATGPU_OK;
}

extern "C" int oatgpu_bgr2hsv(oatgpu_ctx *c, const uint8_t *bgr_in, uint8_t *hsv_out)
{
    if (!c || !bgr_in || !hsv_out) return fail(c, OATGPU_E_INVALID, "null argument");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (c->defer_kind) return fail(c, OATGPU_E_INVALID, "a deferred result is waiting: fetch it first");
    const size_t npx = (size_t)c->g.H * c->g.W;
    { const int rc = stage_in(c, c->aux_a, bgr_in, npx * 3); if (rc) return rc; }
    launch_bgr2hsv(c->aux_a, c->aux_b, npx, c->stream);
    HIPCHK(c, hipGetLastError());
    return finish_frame(c, hsv_out, c->aux_b, npx * 3);
}

// ColorConvert::filter for any pair of oat::PixelColor values: oat::color_conv_table (Color.h:45-51) picks the
// cvtColor code, color_conv_code (Color.h:88-95) refuses the impossible pairs and ColorConvert::connectToNode
// (ColorConvert.cpp:79-85) the ones with nothing to do -- same texts here.
extern "C" int oatgpu_cvt_color(oatgpu_ctx *c, int32_t from_color, int32_t to_color, const uint8_t *in, uint8_t *out)
{
    if (!c || !in || !out) return fail(c, OATGPU_E_INVALID, "null argument");
    static const char *const names[4] = {"BINARY", "GREY", "BGR", "HSV"};
    if (from_color < 0 || from_color > 3 || to_color < 0 || to_color > 3) return fail(c, OATGPU_E_INVALID, "Invalid color.");
    //                       to: BINARY GREY BGR HSV        -1 nothing to do, -2 not possible, 3 = BGR -> HSV
    static const int table[4][4] = {{-1, -1, 1, -2},      // from BINARY
                                    {-1, -1, 1, -2},      // from GREY
                                    {0, 0, -1, 3},        // from BGR
                                    {-2, -2, 2, -1}};     // from HSV
    const int code = table[from_color][to_color];
    if (code == -2) return fail(c, OATGPU_E_INVALID, "Requested color conversion is not possible.");
    if (code == -1)
        return fail(c, OATGPU_E_INVALID, "Nothing to be done for %s to %s conversion.", names[from_color], names[to_color]);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const size_t npx = (size_t)c->g.H * c->g.W;
    const size_t nin = npx * (from_color >= 2 ? 3 : 1), nout = npx * (to_color >= 2 ? 3 : 1);
    if (c->defer_kind) return fail(c, OATGPU_E_INVALID, "a deferred result is waiting: fetch it first");
    { const int rc = stage_in(c, c->aux_a, in, nin); if (rc) return rc; }
    if (code == 3) launch_bgr2hsv(c->aux_a, c->aux_b, npx, c->stream);
    else launch_cvt_color(code, c->aux_a, c->aux_b, npx, c->stream);
    HIPCHK(c, hipGetLastError());
    return finish_frame(c, out, c->aux_b, nout);
}

// The back half of a synchronous detector on the bits it has just put into slot 0's buffer, into the extra result slot, and
// the position handed out -- or, deferred, left with the device once the frame has been read (oatgpu_fetch_position)
static int detect_tail(oatgpu_ctx *c, int s, int erode_k, int dilate_k, oatgpu_position *out)
{
    const int slot = c->ring_slots;       // the extra slot
    const int rc = back_half(c, c->bb[0].b, thr_buf(c, 0), s, 1, slot, c->stream, nullptr, erode_k, dilate_k);
    if (rc) return rc;
    c->last_slot = 0;
    if (c->deferred) {
        HIPCHK(c, hipEventSynchronize(c->ev_h2d));
        c->defer_kind = 2; c->defer_s = s;
        return OATGPU_OK;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    to_position(c->res.host()[(size_t)slot * c->cfg.n_streams + s], out);
    targets_begin(c);
    targets_keep(c, c->tg.ring, slot, s);
    return OATGPU_OK;
}

static int detect_single(oatgpu_ctx *c, int s, const uint8_t *in, int channels, oatgpu_position *out)
{
    int rc = check_stream_ix(c, s);
    if (rc) return rc;
    if (!in || (!out && !c->deferred)) return fail(c, OATGPU_E_INVALID, "null argument");
    rc = open_sync(c);
    if (rc) return rc;
    const Geom &g = c->g;
    const size_t npx = (size_t)g.H * g.W;
    rc = stage_in(c, c->aux_a, in, npx * channels);
    if (rc) return rc;
    RangeParams rp = range_of(detector_of(c->cfg));
    launch_inrange_bits(g, c->aux_a, channels, rp, thr_buf(c, 0) + (size_t)s * (g.Palloc >> 6), c->stream);
    return detect_tail(c, s, -1, -1, out);
}

extern "C" int oatgpu_detect_diff(oatgpu_ctx *c, int32_t s, const uint8_t *grey_in, oatgpu_position *out)
{
    int rc = check_stream_ix(c, s);
    if (rc) return rc;
    if (!grey_in || (!out && !c->deferred)) return fail(c, OATGPU_E_INVALID, "null argument");
    rc = open_sync(c);
    if (rc) return rc;
    const Geom &g = c->g;
    const size_t npx = (size_t)g.H * g.W;
    if (!c->diff_last) HIPCHK(c, c->diff_last.alloc((size_t)c->cfg.n_streams * npx));
    rc = stage_in(c, c->aux_a, grey_in, npx);
    if (rc) return rc;
    const int have = c->diff_have[s];
    launch_absdiff_bits(g, c->aux_a, c->diff_last + (size_t)s * npx, c->cfg.diff_threshold, have,
                        thr_buf(c, 0) + (size_t)s * (g.Palloc >> 6), c->stream);
    c->diff_have[s] = 1;
    // the first frame is analysed unblurred (DifferenceDetector.cpp:167-171); afterwards blur == dilation
    return detect_tail(c, s, 0, have ? c->cfg.blur : 0, out);
}

extern "C" int oatgpu_detect_hsv(oatgpu_ctx *c, int32_t s, const uint8_t *hsv_in, oatgpu_position *out)
{
    return detect_single(c, s, hsv_in, 3, out);
}
extern "C" int oatgpu_detect_thresh(oatgpu_ctx *c, int32_t s, const uint8_t *grey_in, oatgpu_position *out)
{
    return detect_single(c, s, grey_in, 1, out);
}

extern "C" int oatgpu_fetch_position(oatgpu_ctx *c, oatgpu_position *out)
{
    if (!c || !out) return fail(c, OATGPU_E_INVALID, "null argument");
    if (c->defer_kind != 2) return fail(c, OATGPU_E_INVALID, "no deferred position is waiting");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->defer_kind = 0;
    to_position(c->res.host()[(size_t)c->ring_slots * c->cfg.n_streams + c->defer_s], out);
    return OATGPU_OK;
}

// ------------------------------------------------------------------ taps ----

// one camera's bit plane as a byte mask on the host: unpack, copy, wait
int read_plane(oatgpu_ctx *c, const u64 *plane, uint8_t *out)
{
    launch_unpack_bits(c->g, plane, c->aux_b, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, c->aux_b, (size_t)c->g.H * c->g.W, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OATGPU_OK;
}

extern "C" int oatgpu_read_mask(oatgpu_ctx *c, int32_t s, int32_t which, uint8_t *out)
{
    int rc = check_stream_ix(c, s);
    if (rc) return rc;
    if (!out) return fail(c, OATGPU_E_INVALID, "null argument");
    rc = open_sync(c);
    if (rc) return rc;
    const u64 *last_thr = thr_buf(c, c->last_slot);
    const u64 *base = which == OATGPU_TAP_THRESHOLD ? last_thr
                    : which == OATGPU_TAP_MORPH ? c->last_morph
                    : which == OATGPU_TAP_FINAL ? c->last_fin : nullptr;
    if (!base) return fail(c, OATGPU_E_INVALID, "unknown tap %d", which);
    return read_plane(c, base + (size_t)s * (c->g.Palloc >> 6), out);
}
