// api_trackfilt.hip -- what the motion and the subtraction tracker share on the host, and the filter chain on the host.
// `posifilt kalman` -> `posifilt homography` -> `posifilt region` has ONE owner here for both of its users, the marker sets'
// combined record (api_markers.hip) and the trackers' own result records: the checked parameters (chain_params),
// and the hand-out of the list a delivering call keeps (chain_hand_out; delivered_refusals for every such list of the library);
// the setters' body is configure_chain (oatgpu_ctx.h).  The trackers' chain runs one launch a frame behind the slot's back half,
// in frame order (kernels_trackfilt.hip).  A step of either tracker is tracker_begin, its own front and blob launches,
// tracker_tail -- everything that rides on the slot, the chain last -- and tracker_hand_out.
#include "oatgpu_ctx.h"

static_assert(sizeof(oatgpu_filtered) == sizeof(MarkerFiltered), "k_marker_filters and k_tracker_filters write oatgpu_filtered's layout");

// --- what the two trackers' entry points have in common (BatchedTrackerState, oatgpu_ctx.h) ---

bool BatchedTrackerState::alloc(const oatgpu_ctx *c)
{
    n = (size_t)c->cfg.n_streams;
    words = n * ((size_t)c->g.Palloc / 64);
    const size_t K = kSeqSlots;
    bool ok = bits.alloc(K * words * 8) == hipSuccess;
    ok = ok && masks.alloc(K * planes * words * 8) == hipSuccess;
    ok = ok && rec.alloc(K * n * sizeof(ResultRec), hipHostMallocMapped) == hipSuccess;
    ok = ok && tgt.alloc(wants_of(c), K, n, c->cfg.channels, true);
    // (the taps: words beyond the frame are never written by the back half)
    ok = ok && hipMemsetAsync(bits, 0, K * words * 8, c->stream) == hipSuccess;
    ok = ok && hipMemsetAsync(masks, 0, K * planes * words * 8, c->stream) == hipSuccess;
    for (auto &e : ev_front) ok = ok && e.create(hipEventDisableTiming | hipEventDisableSystemFence) == hipSuccess;
    for (auto &e : ev_done) ok = ok && e.create(hipEventDisableTiming) == hipSuccess;
    ok = ok && hipStreamSynchronize(c->stream) == hipSuccess;
    on = ok;
    return ok;
}

// what a step of either tracker refuses, checked before anything is read or has moved
int tracker_refusals(oatgpu_ctx *c, const BatchedTrackerState &bt, const char *name, const char *what)
{
    if (!bt.on) return fail(c, OATGPU_E_INVALID, "the %s tracker is off (oatgpu_set_%s_tracker)", name, name);
    if (c->ring_count || c->staged_count) return fail(c, OATGPU_E_INVALID, "%s while enqueued results are outstanding", what);
    if (c->kal_on) return fail(c, OATGPU_E_INVALID, "%s with the position filter on (oatgpu_set_kalman) is not supported", what);
    if (c->homo_on) return fail(c, OATGPU_E_INVALID, "%s with a homography on (oatgpu_set_homography) is not supported", what);
    if (c->ud_track) return fail(c, OATGPU_E_INVALID, "%s with undistortion on (oatgpu_set_track_undistort) is not supported", what);
    if (c->by_track) return fail(c, OATGPU_E_INVALID, "%s with Bayer frames on (oatgpu_set_track_bayer) is not supported", what);
    return OATGPU_OK;
}

// the arguments of the *_batch_dev, *_batch and *_sequence_dev entry points
int check_batch_dev(oatgpu_ctx *c, const void *frames_dev, const oatgpu_position *out)
{
    if (!c) return OATGPU_E_INVALID;
    if (!frames_dev || !out) return fail(c, OATGPU_E_INVALID, "null argument");
    return OATGPU_OK;
}
int check_batch(oatgpu_ctx *c, const uint8_t *const *frames_host, int n, const oatgpu_position *out)
{
    if (!c) return OATGPU_E_INVALID;
    if (!frames_host || !out) return fail(c, OATGPU_E_INVALID, "null argument");
    if (n != c->cfg.n_streams) return fail(c, OATGPU_E_INVALID, "expected %d frames, got %d", c->cfg.n_streams, n);
    for (int s = 0; s < n; ++s) if (!frames_host[s]) return fail(c, OATGPU_E_INVALID, "null frame %d", s);
    return OATGPU_OK;
}
int check_sequence_dev(oatgpu_ctx *c, const void *const *frames_dev, int n_frames, const oatgpu_position *out)
{
    if (!c) return OATGPU_E_INVALID;
    if (n_frames < 0) return fail(c, OATGPU_E_INVALID, "n_frames must be >= 0");
    if (!frames_dev || (!out && n_frames > 0)) return fail(c, OATGPU_E_INVALID, "null argument");
    for (int t = 0; t < n_frames; ++t) if (!frames_dev[t]) return fail(c, OATGPU_E_INVALID, "null frame set %d", t);
    return OATGPU_OK;
}

// oatgpu_read_diff_mask / oatgpu_read_bsub_mask up to the read itself: the arguments, a frame to read from (none_yet: the text
// where there is none), the context drained
int open_tap(oatgpu_ctx *c, const BatchedTrackerState &bt, const char *name, const char *none_yet, int s, int which, const uint8_t *out)
{
    const int rc = check_stream_ix(c, s);
    if (rc) return rc;
    if (!out) return fail(c, OATGPU_E_INVALID, "null argument");
    if (!bt.on) return fail(c, OATGPU_E_INVALID, "the %s tracker is off (oatgpu_set_%s_tracker)", name, name);
    if (bt.last < 0) return fail(c, OATGPU_E_INVALID, "%s", none_yet);
    if (which != OATGPU_TAP_THRESHOLD && which != OATGPU_TAP_MORPH && which != OATGPU_TAP_FINAL)
        return fail(c, OATGPU_E_INVALID, "unknown tap %d", which);
    return open_sync(c);
}

// oatgpu_diff_reset / oatgpu_bsub_reset: stream s (-1: every stream) starts over with its next frame
int reset_have(oatgpu_ctx *c, std::vector<char> &have, int s)
{
    if (s < -1 || s >= c->cfg.n_streams) return fail(c, OATGPU_E_INVALID, "stream index %d out of range", s);
    if (s < 0) have.assign((size_t)c->cfg.n_streams, 0);
    else have[(size_t)s] = 0;
    return OATGPU_OK;
}

// --- a step of either tracker around its front and blob launches (the declarations in oatgpu_ctx.h say what each does) ---

void tracker_begin(oatgpu_ctx *c)
{
    c->tf.last.begin();
    targets_begin(c);
    c->tk.last.begin();
}

int tracker_tail(oatgpu_ctx *c, const BatchedTrackerState &bt, const BlobBuffers &bb, const ResultRec *rd, int slot, int prev_slot, hipStream_t st)
{
    int rc = targets_launch(c, bb, bt.tgt, slot, 0, c->cfg.n_streams, st);      // (every stream's roots and sums are still in the set)
    if (!rc) rc = crops_launch(c, bt, slot, st);
    if (!rc) rc = crop_tensor_launch(c, bt, slot, st);
    if (!rc) rc = mask_tensor_launch(c, bt, bb, slot, st);
    if (!rc) rc = tracks_launch(c, bt.tgt, slot, prev_slot, st);
    return rc ? rc : tracker_filters_launch(c, rd, slot, prev_slot, st);      // (the caller records the slot's "done" event behind this)
}

void tracker_hand_out(oatgpu_ctx *c, const BatchedTrackerState &bt, int slot, oatgpu_position *out)
{
    for (size_t s = 0; s < bt.n; ++s) to_position(bt.rec.host()[(size_t)slot * bt.n + s], out + s);
    if (c->tf.on) c->tf.last.keep(bt.n, c->tf.out.host() + (size_t)slot * bt.n);
    targets_keep(c, bt.tgt, slot);
    crops_keep(c, bt, slot);
    crop_tensor_keep(c);
    mask_tensor_keep(c);
    if (c->tk.on) c->tk.last.keep(bt.n * (size_t)c->tk.k, bt.tgt.trk_host(slot));
}

int tracker_filters_launch(oatgpu_ctx *c, const ResultRec *rec_dev, int slot, int prev_slot, hipStream_t st)
{
    TrackerFilters &tf = c->tf;
    if (!tf.on) return OATGPU_OK;
    const int n = c->cfg.n_streams;
    if (prev_slot >= 0) HIPCHK(c, hipStreamWaitEvent(st, tf.ev[prev_slot], 0));
    launch_tracker_filters(tf.params, tf.state, rec_dev, tf.out.dev() + (size_t)slot * n, n, st);
    HIPCHK(c, hipGetLastError());
    if (st != c->stream) HIPCHK(c, hipEventRecord(tf.ev[slot], st));
    return OATGPU_OK;
}

// --- the filter chain, for the marker sets and the trackers alike ---

// The parameters of a chain kalman -> homography -> region as the kernels take them, checked: oatgpu_set_marker_filters' and
// oatgpu_set_tracker_filters' limits and messages.  Nothing of the context changes.
int chain_params(oatgpu_ctx *c, const oatgpu_marker_filters *f, MarkerFilterParams &p)
{
    memset(&p, 0, sizeof p);
    if (f->kalman) {
        if (!(f->dt > 0) || !(f->timeout >= 0) || !(f->sigma_accel >= 0) || !(f->sigma_noise >= 0) || !(f->timeout / f->dt < 2147483647.0))
            return fail(c, OATGPU_E_INVALID, "kalman: dt must be > 0, timeout / sigma-accel / sigma-noise >= 0");
        p.kalman = 1;
        p.dt = f->dt; p.sig_accel = f->sigma_accel; p.sig_noise = f->sigma_noise;
        p.threshold = (int)(f->timeout / f->dt);                 // KalmanFilter2D.cpp:74-76
    }
    if (f->homography) {
        p.homography = 1;
        for (int i = 0; i < 9; ++i) p.h[i] = f->h[i];
    }
    if (f->n_regions < 0 || f->n_regions > kMaxRegions) return fail(c, OATGPU_E_INVALID, "at most %d regions (got %d)", kMaxRegions, f->n_regions);
    if (f->n_regions > 0 && !f->regions) return fail(c, OATGPU_E_INVALID, "null argument");
    p.n_regions = f->n_regions;
    int at = 0;
    for (int r = 0; r < f->n_regions; ++r) {
        const oatgpu_region &g = f->regions[r];
        if (!memchr(g.name, 0, sizeof g.name))
            return fail(c, OATGPU_E_INVALID, "region %d: a name takes at most %d bytes", r, (int)sizeof g.name - 1);
        if (g.n_points < 0 || g.n_points > kMaxRegionPoints)
            return fail(c, OATGPU_E_INVALID, "region %d (%s): at most %d points (got %d)", r, g.name, kMaxRegionPoints, g.n_points);
        if (g.n_points > 0 && !g.xy) return fail(c, OATGPU_E_INVALID, "null argument");
        p.region[r][0] = at; p.region[r][1] = g.n_points;
        for (int i = 0; i < g.n_points; ++i, ++at)
            for (int k = 0; k < 2; ++k) {
                const double v = nearbyint(g.xy[2 * i + k]);     // (cv::Point)cv::Point2d: cvRound, ties to even
                if (!(fabs(v) <= 32767.0)) return fail(c, OATGPU_E_INVALID, "region %d (%s): point %d is beyond +-32767", r, g.name, i);
                p.verts[at][k] = (int)v;
            }
    }
    return OATGPU_OK;
}

// What a reader of a Delivered list refuses (oatgpu_ctx.h): its switch is off, no call has delivered since, too little room
int delivered_refusals(oatgpu_ctx *c, bool on, const char *off, const char *none_yet, int sets, int max_sets)
{
    if (!on) return fail(c, OATGPU_E_INVALID, "%s", off);
    if (sets == 0) return fail(c, OATGPU_E_INVALID, "%s", none_yet);
    if (max_sets < sets) return fail(c, OATGPU_E_INVALID, "room for %d frame sets, the latest call delivered %d", max_sets, sets);
    return OATGPU_OK;
}

// oatgpu_marker_filtered / oatgpu_tracker_filtered behind their null checks; none_yet: the text where nothing was delivered yet
int chain_hand_out(oatgpu_ctx *c, const PosfiltChain &ch, const char *who, const char *none_yet, oatgpu_filtered *out, int max_sets)
{
    const std::string off = std::string("no filter chain is configured (oatgpu_set_") + who + "_filters)";
    return delivered_to(c, ch.last, ch.on, off.c_str(), none_yet, out, max_sets);
}

extern "C" int oatgpu_set_tracker_filters(oatgpu_ctx *c, const oatgpu_marker_filters *f)
{
    if (!c) return OATGPU_E_INVALID;
    return configure_chain(c, c->tf, f, "tracker", nullptr, [](TrackerFilters &tf, size_t n) {
        bool ok = tf.out.alloc(kSeqSlots * n * sizeof(MarkerFiltered), hipHostMallocMapped) == hipSuccess;
        for (auto &e : tf.ev) ok = ok && e.create(hipEventDisableTiming | hipEventDisableSystemFence) == hipSuccess;
        return ok;
    });
}

extern "C" int oatgpu_tracker_filtered(oatgpu_ctx *c, oatgpu_filtered *out, int32_t max_sets)
{
    if (!c || !out) return fail(c, OATGPU_E_INVALID, "null argument");
    return chain_hand_out(c, c->tf, "tracker", "no tracker call has run since the filter chain was configured", out, max_sets);
}
