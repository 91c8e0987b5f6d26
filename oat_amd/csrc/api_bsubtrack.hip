// api_bsubtrack.hip -- the subtraction tracker.
// `framefilt bsub` -> `framefilt col -C HSV` -> `posidet hsv` (GREY contexts: `framefilt bsub` -> `posidet thresh`) for every camera
// of the context (kernels_bsubtrack.hip).  The per-stream state -- bsub_bg, bsub_f, bsub_have -- is
// oatgpu_bsub_filter's: the two forms continue each other, oatgpu_bsub_set_background serves both.
#include "oatgpu_ctx.h"

static size_t frame_bytes(const oatgpu_ctx *c) { return (size_t)c->g.H * c->g.W * c->cfg.channels; }

extern "C" int oatgpu_set_bsub_tracker(oatgpu_ctx *c, int32_t on)
{
    if (!c) return OATGPU_E_INVALID;
    if (c->ring_count || c->staged_count) return fail(c, OATGPU_E_INVALID, "set_bsub_tracker while enqueued results are outstanding");
    if (!on) {
        if (!c->bs.on) return OATGPU_OK;
        const int rc = open_sync(c);
        if (rc) return rc;
        c->bs = {};
        return OATGPU_OK;
    }
    if (c->bs.on) return OATGPU_OK;
    int rc = open_sync(c);
    if (rc) return rc;
    rc = ensure_bsub(c, frame_bytes(c));          // (the background planes stay the context's: they outlive the tracker)
    if (rc) return rc;
    const Geom &g = c->g;
    const size_t n = c->cfg.n_streams, NW = (size_t)g.Palloc / 64, K = BsubTracker::kSlots;
    BsubTracker bs;                      // built aside: the context takes it when everything worked
    bool ok = bs.bits.alloc(K * n * NW * 8) == hipSuccess;
    ok = ok && bs.masks.alloc(K * 3 * n * NW * 8) == hipSuccess;
    ok = ok && bs.rec.alloc(K * n * sizeof(ResultRec), hipHostMallocMapped) == hipSuccess;
    // (the taps: words beyond the frame are never written by the back half)
    ok = ok && hipMemsetAsync(bs.bits, 0, K * n * NW * 8, c->stream) == hipSuccess;
    ok = ok && hipMemsetAsync(bs.masks, 0, K * 3 * n * NW * 8, c->stream) == hipSuccess;
    for (auto &e : bs.ev_front) ok = ok && e.create(hipEventDisableTiming | hipEventDisableSystemFence) == hipSuccess;
    for (auto &e : bs.ev_done) ok = ok && e.create(hipEventDisableTiming) == hipSuccess;
    ok = ok && hipStreamSynchronize(c->stream) == hipSuccess;
    if (!ok) return fail(c, OATGPU_E_NOMEM, "bsub tracker: allocation failed: %s", hipGetErrorString(hipGetLastError()));
    bs.on = true;
    c->bs = std::move(bs);
    return OATGPU_OK;
}

extern "C" int oatgpu_bsub_reset(oatgpu_ctx *c, int32_t s)
{
    if (!c) return OATGPU_E_INVALID;
    if (s < -1 || s >= c->cfg.n_streams) return fail(c, OATGPU_E_INVALID, "stream index %d out of range", s);
    if (s < 0) c->bsub_have.assign((size_t)c->cfg.n_streams, 0);
    else c->bsub_have[(size_t)s] = 0;
    return OATGPU_OK;
}

// what a step refuses, checked before anything is read or has moved
static int bsub_refusals(oatgpu_ctx *c, const char *what, double alpha)
{
    if (!c->bs.on) return fail(c, OATGPU_E_INVALID, "the bsub tracker is off (oatgpu_set_bsub_tracker)");
    if (c->ring_count || c->staged_count) return fail(c, OATGPU_E_INVALID, "%s while enqueued results are outstanding", what);
    if (c->kal_on) return fail(c, OATGPU_E_INVALID, "%s with the position filter on (oatgpu_set_kalman) is not supported", what);
    if (c->homo_on) return fail(c, OATGPU_E_INVALID, "%s with a homography on (oatgpu_set_homography) is not supported", what);
    if (c->ud_track) return fail(c, OATGPU_E_INVALID, "%s with undistortion on (oatgpu_set_track_undistort) is not supported", what);
    if (c->by_track) return fail(c, OATGPU_E_INVALID, "%s with Bayer frames on (oatgpu_set_track_bayer) is not supported", what);
    if (!(alpha >= 0.0 && alpha <= 1.0)) return fail(c, OATGPU_E_INVALID, "adaptation-coeff must be in [0,1]");
    if (alpha > 0.0)                    // the reference's accumulateWeighted asserts on its empty fp32 image
        for (int s = 0; s < c->cfg.n_streams; ++s)
            if (c->bsub_have[(size_t)s] == 2)
                return fail(c, OATGPU_E_INVALID, "stream %d: a background image from a file cannot adapt (adaptation-coeff must be 0)", s);
    return OATGPU_OK;
}

static u64 *bsub_bits(oatgpu_ctx *c, int slot) { return c->bs.bits + (size_t)slot * c->cfg.n_streams * (c->g.Palloc >> 6); }
static u64 *bsub_mask(oatgpu_ctx *c, int slot, int which) { return c->bs.masks + ((size_t)slot * 3 + which) * c->cfg.n_streams * (c->g.Palloc >> 6); }

// The front kernel of one frame set (f2: and the next) on stream A into the bits of `slot` (and slot2).  bsub_have is the state
// the first frame met; it moves on.
static int bsub_front(oatgpu_ctx *c, const void *f1, const void *f2, double alpha, int slot, int slot2)
{
    BsubLaunch a{};
    a.frames = (const uint8_t *)f1; a.frames2 = (const uint8_t *)f2; a.channels = c->cfg.channels;
    a.bg = c->bsub_bg; a.acc = c->bsub_f; a.have = c->bsub_have.data();
    a.bits = bsub_bits(c, slot); a.bits2 = f2 ? bsub_bits(c, slot2) : nullptr;
    a.roi = c->roi; a.rp = range_of(detector_of(c->cfg));
    a.bayer = tracker_bayer(c);
    tracker_undistort(c, a);
    a.learn = alpha > 0.0; a.a = (float)alpha; a.b = 1 - a.a;        // accW_: AT a = (AT)alpha, b = 1 - a
    launch_bsubtrack_front(c->g, a, c->cfg.n_streams, c->stream);
    HIPCHK(c, hipGetLastError());
    for (auto &h : c->bsub_have) if (!h) h = 1;
    return OATGPU_OK;
}

// The back half of the frame in `slot` on stream st, every stream in one launch sequence: the context's erode / dilate and area
// window.  Touches neither last_slot nor last_morph / last_fin: those stay with the ordinary calls.  Behind it the filter chain
// on the slot's records, where one is configured (prev_slot: tracker_filters_launch).
static int bsub_back(oatgpu_ctx *c, int slot, hipStream_t st, int prev_slot = -1)
{
    const Geom &g = c->g;
    const int n = c->cfg.n_streams;
    BlobBuffers bb = c->bb[slot].b;
    bb.tmp = bsub_mask(c, slot, 0);
    bb.morph = bsub_mask(c, slot, 1);
    bb.fin = bsub_mask(c, slot, 2);
    const MorphPlan mp = plan_morph(g, c->cfg.erode, c->cfg.dilate);
    const MorphIssued m = issue_morph(g, mp, bb, bsub_bits(c, slot), 0, n, st);
    ResultRec *rd = c->bs.rec.dev() + (size_t)slot * n;
    launch_blob(g, bb, m.src, m.ero, mp.dil, c->cfg.min_area, c->cfg.max_area, rd, 0, n, st, kBlobFull);
    HIPCHK(c, hipGetLastError());
    c->bs.last = slot;
    c->bs.last_tap = m.tap;
    return tracker_filters_launch(c, rd, slot, prev_slot, st);
}

static void bsub_hand_out(oatgpu_ctx *c, int slot, oatgpu_position *out)
{
    const int n = c->cfg.n_streams;
    for (int s = 0; s < n; ++s) to_position(c->bs.rec.host()[(size_t)slot * n + s], out + s);
    tracker_filters_keep(c, slot);
}

// one synchronous step on frames in device memory; the context is drained (open_sync)
static int bsub_step(oatgpu_ctx *c, const void *frames_dev, double alpha, oatgpu_position *out)
{
    tracker_filters_begin(c);
    int rc = bsub_front(c, frames_dev, nullptr, alpha, 0, 0);
    if (rc) return rc;
    rc = bsub_back(c, 0, c->stream);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    bsub_hand_out(c, 0, out);
    return OATGPU_OK;
}

extern "C" int oatgpu_bsub_track_batch_dev(oatgpu_ctx *c, const void *frames_dev, double alpha, oatgpu_position *out)
{
    if (!c) return OATGPU_E_INVALID;
    if (!frames_dev || !out) return fail(c, OATGPU_E_INVALID, "null argument");
    int rc = bsub_refusals(c, "bsub_track_batch", alpha);
    if (rc) return rc;
    rc = open_sync(c);
    if (rc) return rc;
    return bsub_step(c, frames_dev, alpha, out);
}

extern "C" int oatgpu_bsub_track_batch(oatgpu_ctx *c, const uint8_t *const *frames_host, int32_t n, double alpha, oatgpu_position *out)
{
    if (!c) return OATGPU_E_INVALID;
    if (!frames_host || !out) return fail(c, OATGPU_E_INVALID, "null argument");
    if (n != c->cfg.n_streams) return fail(c, OATGPU_E_INVALID, "expected %d frames, got %d", c->cfg.n_streams, n);
    for (int s = 0; s < n; ++s) if (!frames_host[s]) return fail(c, OATGPU_E_INVALID, "null frame %d", s);
    int rc = bsub_refusals(c, "bsub_track_batch", alpha);
    if (rc) return rc;
    rc = open_sync(c);
    if (rc) return rc;
    rc = upload_frames(c, frames_host, tracker_in_bytes(c));
    if (rc) return rc;
    return bsub_step(c, c->frames, alpha, out);
}

// A recorded sequence: up to four frames in flight.  Front launches on stream A -- two frames a launch wherever a next frame
// exists, a first frame may be the first of a pair --, frame t's back half on B[t % 3] behind the front launch's event, in slot
// t % 4 (scratch set, bits, masks, records); a slot is reused only after its result has been collected.  Everything is collected
// before the call returns.
extern "C" int oatgpu_bsub_track_sequence_dev(oatgpu_ctx *c, const void *const *frames_dev, int32_t n_frames, double alpha,
                                              oatgpu_position *out)
{
    if (!c) return OATGPU_E_INVALID;
    if (n_frames < 0) return fail(c, OATGPU_E_INVALID, "n_frames must be >= 0");
    if (!frames_dev || (!out && n_frames > 0)) return fail(c, OATGPU_E_INVALID, "null argument");
    for (int t = 0; t < n_frames; ++t) if (!frames_dev[t]) return fail(c, OATGPU_E_INVALID, "null frame set %d", t);
    int rc = bsub_refusals(c, "bsub_track_sequence", alpha);
    if (rc) return rc;
    if (n_frames == 0) return OATGPU_OK;
    rc = open_sync(c);
    if (rc) return rc;
    static_assert(BsubTracker::kSlots == kSeqSlots, "the sequence loop's slots are the tracker's");
    const int n = c->cfg.n_streams;
    int prev = -1;                         // slot of the frame before (the filter chain's order)
    tracker_filters_begin(c);
    return run_sequence_in_flight(
        c, n_frames, c->bs.ev_front, c->bs.ev_done, [&](int t) { return t + 1 < n_frames ? 2 : 1; },
        [&](int t, int nf, int q, int q2) { return bsub_front(c, frames_dev[t], nf == 2 ? frames_dev[t + 1] : nullptr, alpha, q, q2); },
        [&](int q, int, hipStream_t B) { return bsub_back(c, q, B, std::exchange(prev, q)); },
        [&](int q, int frame) { bsub_hand_out(c, q, out + (size_t)frame * n); });
}

extern "C" int oatgpu_bsub_get_state(oatgpu_ctx *c, int32_t s, uint8_t *bg, float *acc)
{
    int rc = check_stream_ix(c, s);
    if (rc) return rc;
    const int have = c->bsub_bg ? c->bsub_have[(size_t)s] : 0;
    if (!have) return fail(c, OATGPU_E_INVALID, "stream %d has no background yet", s);
    if (acc && have == 2) return fail(c, OATGPU_E_INVALID, "stream %d: a background image from a file has no accumulator", s);
    rc = open_sync(c);
    if (rc) return rc;
    const size_t nb = frame_bytes(c);
    if (bg) HIPCHK(c, hipMemcpyAsync(bg, c->bsub_bg + (size_t)s * nb, nb, hipMemcpyDeviceToHost, c->stream));
    if (acc) HIPCHK(c, hipMemcpyAsync(acc, c->bsub_f + (size_t)s * nb, nb * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return OATGPU_OK;
}

extern "C" int oatgpu_read_bsub_mask(oatgpu_ctx *c, int32_t s, int32_t which, uint8_t *out)
{
    int rc = check_stream_ix(c, s);
    if (rc) return rc;
    if (!out) return fail(c, OATGPU_E_INVALID, "null argument");
    if (!c->bs.on) return fail(c, OATGPU_E_INVALID, "the bsub tracker is off (oatgpu_set_bsub_tracker)");
    if (c->bs.last < 0) return fail(c, OATGPU_E_INVALID, "no bsub tracker step has run yet");
    if (which != OATGPU_TAP_THRESHOLD && which != OATGPU_TAP_MORPH && which != OATGPU_TAP_FINAL)
        return fail(c, OATGPU_E_INVALID, "unknown tap %d", which);
    rc = open_sync(c);
    if (rc) return rc;
    const int q = c->bs.last;
    const u64 *base = which == OATGPU_TAP_FINAL ? bsub_mask(c, q, 2) : which == OATGPU_TAP_MORPH ? c->bs.last_tap : bsub_bits(c, q);
    return read_plane(c, base + (size_t)s * (c->g.Palloc >> 6), out);
}
