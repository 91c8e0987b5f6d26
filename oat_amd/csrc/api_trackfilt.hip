// api_trackfilt.hip -- the filter chain behind the motion and the subtraction tracker.
// `posifilt kalman` -> `posifilt homography` -> `posifilt region` on the trackers' own result records (kernels_trackfilt.hip,
// DESIGN.md 9h): one launch a frame behind the slot's back half, in frame order.  api_diff.hip and api_bsubtrack.hip call the
// three helpers below from their steps; with no chain configured they do nothing.
#include "oatgpu_ctx.h"

static_assert(TrackerFilters::kSlots == kSeqSlots && TrackerFilters::kSlots == DiffTracker::kSlots &&
              TrackerFilters::kSlots == BsubTracker::kSlots, "a filtered set for every slot of the trackers");

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
        ok = ok && tf.out.alloc(TrackerFilters::kSlots * n * sizeof(MarkerFiltered), hipHostMallocMapped) == hipSuccess;
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
