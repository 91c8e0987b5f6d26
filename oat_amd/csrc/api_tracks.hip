// api_tracks.hip -- target tracks: identity across frames for the K ranked blobs of every camera.
// While tracks are on, the back halves of the motion and the subtraction tracker (diff_back, api_diff.hip; bsub_back,
// api_bsubtrack.hip) launch k_target_tracks (kernels_tracks.hip) behind targets_launch on the same HIP stream, into the track set
// of the frame's slot; inside the sequence calls the host orders consecutive frames with an event per slot, exactly like
// tracker_filters_launch (api_trackfilt.hip).  The calls that hand results out keep the sets they delivered (tracks_begin,
// tracks_keep) for oatgpu_tracks, the way targets_keep does.  oatgpu_tracks_update is the same kernel on positions from the host.
#include "oatgpu_ctx.h"

static_assert(sizeof(oatgpu_track) == sizeof(TrackRec), "k_target_tracks writes oatgpu_track's layout");

bool tracks_alloc_sets(const oatgpu_ctx *c, HostMem<TrackRec> &sets, int k)
{
    const size_t bytes = (size_t)kSeqSlots * (size_t)c->cfg.n_streams * (size_t)k * sizeof(TrackRec);
    if (sets.alloc(bytes, hipHostMallocMapped) != hipSuccess) return false;
    memset(sets.host(), 0, bytes);
    return true;
}

int tracks_launch(oatgpu_ctx *c, const TargetRec *recs, TrackRec *sets, int slot, int prev_slot, hipStream_t st)
{
    Tracks &tk = c->tk;
    if (!tk.on) return OATGPU_OK;
    const int n = c->cfg.n_streams;
    if (prev_slot >= 0) HIPCHK(c, hipStreamWaitEvent(st, tk.ev[prev_slot], 0));
    launch_target_tracks(tk.launch(), recs, nullptr, sets + (size_t)slot * n * (size_t)tk.k, n, st);
    HIPCHK(c, hipGetLastError());
    if (st != c->stream) HIPCHK(c, hipEventRecord(tk.ev[slot], st));
    return OATGPU_OK;
}

void tracks_begin(oatgpu_ctx *c) { c->tk.last_sets = 0; }

void tracks_keep(oatgpu_ctx *c, const TrackRec *set)
{
    Tracks &tk = c->tk;
    if (!tk.on) return;
    const size_t per = (size_t)c->cfg.n_streams * (size_t)tk.k;
    tk.last.resize((size_t)(tk.last_sets + 1) * per);
    memcpy(tk.last.data() + (size_t)tk.last_sets * per, set, per * sizeof(oatgpu_track));
    tk.last_sets++;
}

extern "C" int oatgpu_set_tracks(oatgpu_ctx *c, const oatgpu_marker_filters *f, double gate)
{
    if (!c) return OATGPU_E_INVALID;
    if (c->ring_count || c->staged_count) return fail(c, OATGPU_E_INVALID, "set_tracks while enqueued results are outstanding");
    if (!f) {
        const int rc = open_sync(c);
        if (rc) return rc;
        c->tk = {};
        c->df.trk = {}; c->bs.trk = {};
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
    HostMem<TrackRec> df, bs;
    bool ok = made.params.alloc(sizeof(MarkerFilterParams)) == hipSuccess;
    ok = ok && made.state.alloc(n * k * sizeof(KalmanState)) == hipSuccess;
    ok = ok && made.meta.alloc(n * k * sizeof(TrackMeta)) == hipSuccess;
    ok = ok && made.next_id.alloc(n * sizeof(long long)) == hipSuccess;
    ok = ok && made.upd_in.alloc(n * k * sizeof(TrackTriple), hipHostMallocMapped) == hipSuccess;
    ok = ok && made.upd_out.alloc(n * k * sizeof(TrackRec), hipHostMallocMapped) == hipSuccess;
    for (auto &e : made.ev) ok = ok && e.create(hipEventDisableTiming | hipEventDisableSystemFence) == hipSuccess;
    ok = ok && (!c->df.on || tracks_alloc_sets(c, df, (int)k));
    ok = ok && (!c->bs.on || tracks_alloc_sets(c, bs, (int)k));
    if (!ok) return fail(c, OATGPU_E_NOMEM, "tracks: allocation failed: %s", hipGetErrorString(hipGetLastError()));
    memset(made.upd_out.host(), 0, n * k * sizeof(TrackRec));
    const std::vector<long long> first(n, 1);
    HIPCHK(c, hipMemcpy(made.params, hp.data(), sizeof(MarkerFilterParams), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(made.next_id, first.data(), n * sizeof(long long), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemsetAsync(made.meta, 0, n * k * sizeof(TrackMeta), c->stream));
    launch_kalman_reset(made.state, (int)(n * k), 0u, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    made.on = true;
    made.k = (int)k;
    made.gate2 = gate * gate;
    made.last.reserve(n * k);
    c->tk = std::move(made);
    c->df.trk = std::move(df);
    c->bs.trk = std::move(bs);
    return OATGPU_OK;
}

extern "C" int oatgpu_tracks(oatgpu_ctx *c, oatgpu_track *out, int32_t max_sets)
{
    if (!c || !out) return fail(c, OATGPU_E_INVALID, "null argument");
    const Tracks &tk = c->tk;
    if (!tk.on) return fail(c, OATGPU_E_INVALID, "tracks are off (oatgpu_set_tracks)");
    if (tk.last_sets == 0) return fail(c, OATGPU_E_INVALID, "no call has delivered a track set since tracks were switched on");
    if (max_sets < tk.last_sets) return fail(c, OATGPU_E_INVALID, "room for %d frame sets, the latest call delivered %d", max_sets, tk.last_sets);
    memcpy(out, tk.last.data(), (size_t)tk.last_sets * c->cfg.n_streams * (size_t)tk.k * sizeof(oatgpu_track));
    return tk.last_sets;
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
    tracks_begin(c);
    tracks_keep(c, tk.upd_out.host());
    return OATGPU_OK;
}
