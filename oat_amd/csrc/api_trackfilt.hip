// api_trackfilt.hip -- what the motion and the subtraction tracker share on the host, and the filter chain behind them.
// `posifilt kalman` -> `posifilt homography` -> `posifilt region` on the trackers' own result records (kernels_trackfilt.hip,
// DESIGN.md 9h): one launch a frame behind the slot's back half, in frame order.  api_diff.hip and api_bsubtrack.hip call the
// three helpers below from their steps; with no chain configured they do nothing.
#include "oatgpu_ctx.h"

// --- what the two trackers' entry points have in common (BatchedTrackerState, oatgpu_ctx.h) ---

bool BatchedTrackerState::alloc(const oatgpu_ctx *c)
{
    n = (size_t)c->cfg.n_streams;
    words = n * ((size_t)c->g.Palloc / 64);
    const size_t K = kSeqSlots;
    bool ok = bits.alloc(K * words * 8) == hipSuccess;
    ok = ok && masks.alloc(K * planes * words * 8) == hipSuccess;
    ok = ok && rec.alloc(K * n * sizeof(ResultRec), hipHostMallocMapped) == hipSuccess;
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

// the finished frame in `slot` to the caller: its records as positions, its filtered set into the call's
void tracker_hand_out(oatgpu_ctx *c, const BatchedTrackerState &bt, int slot, oatgpu_position *out)
{
    for (size_t s = 0; s < bt.n; ++s) to_position(bt.rec.host()[(size_t)slot * bt.n + s], out + s);
    tracker_filters_keep(c, slot);
}

// --- the filter chain ---

// The chain on the frame whose result records are rec_dev (the tracker's slot `slot`), on stream st right behind that frame's
// back half.  Inside a sequence call (st is a B stream) consecutive frames sit on different HIP streams: the launch waits for
// the filter event of the frame before it (prev_slot; -1: the first frame of the call, everything before it has drained) and
// records its own.  The synchronous step runs on stream A alone and needs neither.  The caller records the slot's "done" event
// behind this.
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

// a tracker call starts: what oatgpu_tracker_filtered hands out is this call's
void tracker_filters_begin(oatgpu_ctx *c)
{
    if (c->tf.on) c->tf.last_sets = 0;
}

// the frame in `slot` has finished: its filtered set joins the call's
void tracker_filters_keep(oatgpu_ctx *c, int slot)
{
    static_assert(sizeof(oatgpu_filtered) == sizeof(MarkerFiltered), "k_tracker_filters writes oatgpu_filtered's layout");
    TrackerFilters &tf = c->tf;
    if (!tf.on) return;
    const size_t n = (size_t)c->cfg.n_streams;
    tf.last.resize((size_t)(tf.last_sets + 1) * n);
    memcpy(tf.last.data() + (size_t)tf.last_sets * n, tf.out.host() + (size_t)slot * n, n * sizeof(oatgpu_filtered));
    tf.last_sets++;
}

// Everything is checked before anything changes.
extern "C" int oatgpu_set_tracker_filters(oatgpu_ctx *c, const oatgpu_marker_filters *f)
{
    if (!c) return OATGPU_E_INVALID;
    if (c->ring_count || c->staged_count) return fail(c, OATGPU_E_INVALID, "set_tracker_filters while enqueued results are outstanding");
    const bool on = f && (f->kalman || f->homography || f->n_regions > 0);
    std::vector<MarkerFilterParams> hp(on ? 1 : 0);      // (8 KiB: not on the stack)
    if (on) {
        const int prc = chain_params(c, f, hp[0]);
        if (prc) return prc;
    }
    int rc = open_sync(c);
    if (rc) return rc;
    if (!on) { c->tf = {}; return OATGPU_OK; }
    const size_t n = (size_t)c->cfg.n_streams;
    TrackerFilters made;                    // first use: built aside, moved in when everything worked
    const bool first = !c->tf.params;
    TrackerFilters &tf = first ? made : c->tf;
    if (first) {
        bool ok = tf.params.alloc(sizeof(MarkerFilterParams)) == hipSuccess;
        ok = ok && tf.state.alloc(n * sizeof(KalmanState)) == hipSuccess;
        ok = ok && tf.out.alloc(kSeqSlots * n * sizeof(MarkerFiltered), hipHostMallocMapped) == hipSuccess;
        for (auto &e : tf.ev) ok = ok && e.create(hipEventDisableTiming | hipEventDisableSystemFence) == hipSuccess;
        if (!ok) return fail(c, OATGPU_E_NOMEM, "tracker filters: allocation failed: %s", hipGetErrorString(hipGetLastError()));
        tf.last.reserve(n);
    }
    HIPCHK(c, hipMemcpy(tf.params, hp.data(), sizeof(MarkerFilterParams), hipMemcpyHostToDevice));
    launch_kalman_reset(tf.state, (int)n, 0u, c->stream);          // every stream's filter from the reference's initial state
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (first) c->tf = std::move(made);
    c->tf.on = true;
    c->tf.last_sets = 0;
    return OATGPU_OK;
}

extern "C" int oatgpu_tracker_filtered(oatgpu_ctx *c, oatgpu_filtered *out, int32_t max_sets)
{
    if (!c || !out) return fail(c, OATGPU_E_INVALID, "null argument");
    if (!c->tf.on) return fail(c, OATGPU_E_INVALID, "no filter chain is configured (oatgpu_set_tracker_filters)");
    if (c->tf.last_sets == 0) return fail(c, OATGPU_E_INVALID, "no tracker call has run since the filter chain was configured");
    if (max_sets < c->tf.last_sets) return fail(c, OATGPU_E_INVALID, "room for %d frame sets, the latest call delivered %d", max_sets, c->tf.last_sets);
    memcpy(out, c->tf.last.data(), (size_t)c->tf.last_sets * c->cfg.n_streams * sizeof(oatgpu_filtered));
    return c->tf.last_sets;
}
