// api_tracks.hip -- target tracks: identity across frames for the K ranked blobs of every camera.
// While tracks are on, the tail of a step of the motion and the subtraction tracker (tracker_tail, api_trackfilt.hip) launches
// k_target_tracks (kernels_tracks.hip) behind the ranking on the same HIP stream, into the track set of the frame's slot
// (TargetSets::trk); inside the sequence calls the host orders consecutive frames with an event per slot, exactly like
// tracker_filters_launch.  tracker_hand_out keeps the sets a call delivered for oatgpu_tracks.
// oatgpu_tracks_update is the same kernel on positions from the host.
#include "oatgpu_ctx.h"

static_assert(sizeof(oatgpu_track) == sizeof(TrackRec), "k_target_tracks writes oatgpu_track's layout");

int tracks_launch(oatgpu_ctx *c, const TargetSets &ts, int slot, int prev_slot, hipStream_t st)
{
    Tracks &tk = c->tk;
    if (!tk.on) return OATGPU_OK;
    const int n = c->cfg.n_streams;
    if (prev_slot >= 0) HIPCHK(c, hipStreamWaitEvent(st, tk.ev[prev_slot], 0));
    launch_target_tracks(tk.launch(), ts.rec_dev(slot), nullptr, ts.trk_dev(slot), n, st);
    HIPCHK(c, hipGetLastError());
    if (st != c->stream) HIPCHK(c, hipEventRecord(tk.ev[slot], st));
    return OATGPU_OK;
}

extern "C" int oatgpu_set_tracks(oatgpu_ctx *c, const oatgpu_marker_filters *f, double gate)
{
    if (!c) return OATGPU_E_INVALID;
    if (c->ring_count || c->staged_count) return fail(c, OATGPU_E_INVALID, "set_tracks while enqueued results are outstanding");
    if (!f) {
        const int rc = open_sync(c);
        if (rc) return rc;
        c->tk = {};
        for_each_target_home(c, [](TargetSets &ts, size_t, bool, bool) { ts.trk = {}; });
        return OATGPU_OK;
    }
    if (!c->tg.k) return fail(c, OATGPU_E_INVALID, "set_tracks: targets are off (oatgpu_set_targets)");
    if (!f->kalman) return fail(c, OATGPU_E_INVALID, "set_tracks: the kalman member of the chain is required");
    if (!(gate >= 0.0)) return fail(c, OATGPU_E_INVALID, "set_tracks: the gate must be >= 0 (+inf: no gate)");
    std::vector<MarkerFilterParams> hp(1);               // (8 KiB: not on the stack)
    int rc = chain_params(c, f, hp[0]);
    if (rc) return rc;
    rc = open_sync(c);
    if (rc) return rc;
    // everything is built aside: a failed allocation leaves the context as it was
    const size_t n = (size_t)c->cfg.n_streams, k = (size_t)c->tg.k;
    Tracks made;
    bool ok = made.params.alloc(sizeof(MarkerFilterParams)) == hipSuccess;
    ok = ok && made.state.alloc(n * k * sizeof(KalmanState)) == hipSuccess;
    ok = ok && made.meta.alloc(n * k * sizeof(TrackMeta)) == hipSuccess;
    ok = ok && made.next_id.alloc(n * sizeof(long long)) == hipSuccess;
    ok = ok && made.upd_in.alloc(n * k * sizeof(TrackTriple), hipHostMallocMapped) == hipSuccess;
    ok = ok && made.upd_out.alloc(n * k * sizeof(TrackRec), hipHostMallocMapped) == hipSuccess;
    for (auto &e : made.ev) ok = ok && e.create(hipEventDisableTiming | hipEventDisableSystemFence) == hipSuccess;
    if (!ok) return fail(c, OATGPU_E_NOMEM, "tracks: allocation failed: %s", hipGetErrorString(hipGetLastError()));
    TargetWants w = wants_of(c);
    w.tracks = true;
    memset(made.upd_out.host(), 0, n * k * sizeof(TrackRec));
    const std::vector<long long> first(n, 1);
    HIPCHK(c, hipMemcpy(made.params, hp.data(), sizeof(MarkerFilterParams), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(made.next_id, first.data(), n * sizeof(long long), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemsetAsync(made.meta, 0, n * k * sizeof(TrackMeta), c->stream));
    launch_kalman_reset(made.state, (int)(n * k), 0u, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    rc = rebuild_target_sets(c, w, "tracks");            // (last: nothing after it can fail)
    if (rc) return rc;
    made.on = true;
    made.k = (int)k;
    made.gate2 = gate * gate;
    made.last.items.reserve(n * k);
    c->tk = std::move(made);
    return OATGPU_OK;
}

extern "C" int oatgpu_tracks(oatgpu_ctx *c, oatgpu_track *out, int32_t max_sets)
{
    if (!c || !out) return fail(c, OATGPU_E_INVALID, "null argument");
    return delivered_to(c, c->tk.last, c->tk.on, "tracks are off (oatgpu_set_tracks)",
                        "no call has delivered a track set since tracks were switched on", out, max_sets);
}

extern "C" int oatgpu_tracks_update(oatgpu_ctx *c, const oatgpu_position *targets, oatgpu_track *out)
{
    if (!c || !targets || !out) return fail(c, OATGPU_E_INVALID, "null argument");
    Tracks &tk = c->tk;
    if (!tk.on) return fail(c, OATGPU_E_INVALID, "tracks are off (oatgpu_set_tracks)");
    if (c->ring_count || c->staged_count) return fail(c, OATGPU_E_INVALID, "tracks_update while enqueued results are outstanding");
    const int rc = open_sync(c);
    if (rc) return rc;
    const int n = c->cfg.n_streams;
    const size_t per = (size_t)n * (size_t)tk.k;
    TrackTriple *in = tk.upd_in.host();
    for (size_t i = 0; i < per; ++i) {
        in[i].valid = targets[i].valid != 0;
        in[i].x = targets[i].x; in[i].y = targets[i].y;
    }
    launch_target_tracks(tk.launch(), nullptr, tk.upd_in.dev(), tk.upd_out.dev(), n, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memcpy(out, tk.upd_out.host(), per * sizeof(oatgpu_track));
    tk.last.begin();
    tk.last.keep(per, tk.upd_out.host());
    return OATGPU_OK;
}
