// api_markers.hip -- marker sets.
// Several colour windows per camera behind ONE model pass, and `posicom mean` behind them (kernels_markers.hip).
#include "oatgpu_ctx.h"

// the context's own window is the NON-ZERO window: its threshold plane is then Z (kernels_markers.hip)
bool own_window_is_nonzero(const oatgpu_config &k)
{
    const RangeParams r = range_of(detector_of(k));
    if (k.channels == 1) return r.lo[0] == 1 && r.hi[0] == 255;
    return r.lo[0] == 0 && r.hi[0] == 255 && r.lo[1] == 0 && r.hi[1] == 255 && r.lo[2] == 1 && r.hi[2] == 255;
}

extern "C" int oatgpu_set_markers(oatgpu_ctx *c, int32_t n_markers, const oatgpu_marker *defaults, int32_t heading_anchor)
{
    if (!c) return OATGPU_E_INVALID;
    if (n_markers < 0 || n_markers > kMaxMarkers) return fail(c, OATGPU_E_INVALID, "n_markers must be in 0..%d", kMaxMarkers);
    if (n_markers > 0 && !defaults) return fail(c, OATGPU_E_INVALID, "null argument");
    if (n_markers > 0 && (heading_anchor < -1 || heading_anchor >= n_markers))      // MeanPosition.cpp:55-57
        return fail(c, OATGPU_E_INVALID, "heading anchor %d out of range: -1 (none) or a marker index below %d", heading_anchor, n_markers);
    for (int m = 0; m < n_markers; ++m) { const int rc = check_detector(c, defaults[m]); if (rc) return rc; }
    if (n_markers > 0 && c->tg.k) return fail(c, OATGPU_E_INVALID, "set_markers with targets on (oatgpu_set_targets) is not supported");
    if (c->mkp.on)       // (its planes, scratch and records are sized by M: refused, like everything that would pull them from under it)
        return fail(c, OATGPU_E_INVALID, "the marker pipeline is on: oatgpu_set_marker_pipeline(0) before the marker set changes");
    int rc = open_sync(c);
    if (rc) return rc;
    c->mkp = {}; c->mf = {}; c->mk = {};      // the old set goes BEFORE the new one is made: peak memory does not double
    if (n_markers == 0) return OATGPU_OK;

    const size_t n = c->cfg.n_streams, M = (size_t)n_markers, NW = (size_t)c->g.Palloc / 64;
    const size_t res_bytes = M * n * sizeof(ResultRec) + n * sizeof(MarkerCombined);
    MarkerSet &mk = c->mk;
    bool ok = mk.win.alloc(n * M * sizeof(RangeParams)) == hipSuccess;
    ok = ok && mk.planes.alloc(M * n * NW * 8) == hipSuccess;
    ok = ok && mk.masks.alloc(M * 3 * n * NW * 8) == hipSuccess;
    ok = ok && mk.res.alloc(res_bytes) == hipSuccess;
    ok = ok && mk.res_host.alloc(res_bytes, hipHostMallocDefault) == hipSuccess;
    ok = ok && mk.bb.alloc(c);
    // (the taps read these before the first step; words beyond the frame are never written by the back half)
    ok = ok && hipMemsetAsync(mk.planes, 0, M * n * NW * 8, c->stream) == hipSuccess;
    ok = ok && hipMemsetAsync(mk.masks, 0, M * 3 * n * NW * 8, c->stream) == hipSuccess;
    if (ok) {
        mk.win_host.resize(n * M);
        for (size_t s = 0; s < n; ++s)
            for (size_t m = 0; m < M; ++m) mk.win_host[s * M + m] = range_of(defaults[m]);
        ok = hipMemcpy(mk.win, mk.win_host.data(), n * M * sizeof(RangeParams), hipMemcpyHostToDevice) == hipSuccess;
    }
    ok = ok && hipStreamSynchronize(c->stream) == hipSuccess;
    if (!ok) {
        const hipError_t e = hipGetLastError();
        mk = {};
        return fail(c, OATGPU_E_NOMEM, "marker sets: device allocation failed: %s", hipGetErrorString(e));
    }
    mk.n = n_markers;
    mk.anchor = heading_anchor;
    mk.def.assign(defaults, defaults + n_markers);
    mk.tap_morph.resize(M);
    for (size_t m = 0; m < M; ++m) mk.tap_morph[m] = mk.planes + m * n * NW;
    return OATGPU_OK;
}

static int check_marker_ix(oatgpu_ctx *c, int s, int m)
{
    const int rc = check_stream_ix(c, s);
    if (rc) return rc;
    if (c->mk.n == 0) return fail(c, OATGPU_E_INVALID, "marker sets are not configured (oatgpu_set_markers)");
    if (m < 0 || m >= c->mk.n) return fail(c, OATGPU_E_INVALID, "marker index %d out of range (have %d)", m, c->mk.n);
    return OATGPU_OK;
}

extern "C" int oatgpu_set_marker_window(oatgpu_ctx *c, int32_t s, int32_t marker, const oatgpu_marker *m)
{
    int rc = check_marker_ix(c, s, marker);
    if (rc) return rc;
    if (!m) return fail(c, OATGPU_E_INVALID, "null argument");
    oatgpu_marker w = c->mk.def[(size_t)marker];      // erode / dilate / area stay the marker's: only the window is checked and taken
    w.h_lo = m->h_lo; w.h_hi = m->h_hi; w.s_lo = m->s_lo; w.s_hi = m->s_hi; w.v_lo = m->v_lo; w.v_hi = m->v_hi;
    rc = check_detector(c, w);
    if (rc) return rc;
    rc = open_sync(c);
    if (rc) return rc;
    const size_t i = (size_t)s * c->mk.n + marker;
    c->mk.win_host[i] = range_of(w);
    HIPCHK(c, hipMemcpy(c->mk.win + i, &c->mk.win_host[i], sizeof(RangeParams), hipMemcpyHostToDevice));
    return OATGPU_OK;
}

// what a marker step refuses, checked before anything has moved
static int marker_step_refusals(oatgpu_ctx *c, const char *what = "track_markers")
{
    if (c->ring_count || c->staged_count) return fail(c, OATGPU_E_INVALID, "%s while enqueued results are outstanding", what);
    if (c->mk.n == 0) return fail(c, OATGPU_E_INVALID, "marker sets are not configured (oatgpu_set_markers)");
    if (!own_window_is_nonzero(c->cfg))
        return fail(c, OATGPU_E_INVALID, "%s needs the context's own window to be the non-zero window: %s", what,
                    c->cfg.channels == 1 ? "intensity [1,256]" : "H [0,256], S [0,256], V [1,256]");
    if (c->kal_on) return fail(c, OATGPU_E_INVALID, "%s with the position filter on (oatgpu_set_kalman) is not supported", what);
    if (c->homo_on) return fail(c, OATGPU_E_INVALID, "%s with a homography on (oatgpu_set_homography) is not supported", what);
    return OATGPU_OK;
}

// The pipelined marker path, on or off (default off).  On: the refusals of the synchronous step, then EVERYTHING the path needs
// is allocated here (oatgpu.h has the sizes); a failed allocation is reported here and leaves an ordinary context.
extern "C" int oatgpu_set_marker_pipeline(oatgpu_ctx *c, int32_t on)
{
    if (!c) return OATGPU_E_INVALID;
    if (!on) {
        if (!c->mkp.on) return OATGPU_OK;
        if (c->ring_count || c->staged_count)
            return fail(c, OATGPU_E_INVALID, "set_marker_pipeline while enqueued results are outstanding");
        const int rc = open_sync(c);
        if (rc) return rc;
        c->mkp = {};
        return OATGPU_OK;
    }
    { const int rrc = marker_step_refusals(c, "set_marker_pipeline"); if (rrc) return rrc; }
    if (c->mkp.on) return OATGPU_OK;
    int rc = open_sync(c);
    if (rc) return rc;
    const Geom &g = c->g;
    const size_t n = c->cfg.n_streams, M = (size_t)c->mk.n, NW = (size_t)g.Palloc / 64, planes = M * n, ring = (size_t)c->ring_slots;
    // the one-launch back half: a geometry the LDS kernel takes, and a row scan whose LDS holds the largest dilation of the set
    std::vector<BlobTab> tab(planes);
    int max_dil = 0;
    for (size_t m = 0; m < M; ++m) {
        const oatgpu_marker &k = c->mk.def[m];
        const MorphPlan mp = plan_morph(g, k.erode, k.dilate);
        max_dil = std::max(max_dil, mp.dil);
        for (size_t s = 0; s < n; ++s) tab[m * n + s] = BlobTab{mp.ero ? mp.ero : 1, mp.dil, k.min_area, k.max_area};
    }
    MarkerPipeline mkp;                  // built aside: the context takes it when everything worked
    mkp.max_dil = max_dil;
    mkp.table = g.H > 2 && g.H <= 16383 && g.W <= 16383 && rowscan_lds_bytes(g, max_dil) <= kRowscanLdsMax;
    mkp.set_bytes = planes * sizeof(ResultRec) + n * (sizeof(MarkerCombined) + sizeof(MarkerFiltered));
    bool ok = mkp.planes.alloc(ring * planes * NW * 8) == hipSuccess;
    ok = ok && mkp.masks.alloc(ring * 3 * planes * NW * 8) == hipSuccess;
    ok = ok && mkp.tab.alloc(planes * sizeof(BlobTab)) == hipSuccess;
    ok = ok && mkp.res.alloc(2 * planes * sizeof(ResultRec)) == hipSuccess;
    ok = ok && mkp.rec.alloc(ring * mkp.set_bytes, hipHostMallocMapped) == hipSuccess;
    for (auto &b : mkp.bb) ok = ok && b.alloc(c, planes);
    // (the taps may be read before a slot's first step; words beyond the frame are never written by the back half)
    ok = ok && hipMemsetAsync(mkp.planes, 0, ring * planes * NW * 8, c->stream) == hipSuccess;
    ok = ok && hipMemsetAsync(mkp.masks, 0, ring * 3 * planes * NW * 8, c->stream) == hipSuccess;
    ok = ok && hipMemcpy(mkp.tab, tab.data(), planes * sizeof(BlobTab), hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && make_events(mkp.ev, ring, hipEventDisableTiming) == hipSuccess;
    ok = ok && mkp.bits_ev.create(hipEventDisableTiming | hipEventDisableSystemFence) == hipSuccess;
    ok = ok && hipStreamSynchronize(c->stream) == hipSuccess;
    if (!ok) return fail(c, OATGPU_E_NOMEM, "marker pipeline: allocation failed: %s", hipGetErrorString(hipGetLastError()));
    mkp.ev_of.assign(ring, 0);
    mkp.tap_morph.assign(ring * M, nullptr);
    mkp.on = true;
    c->mkp = std::move(mkp);
    return OATGPU_OK;
}

// The marker work of a step (oatgpu_set_marker_pipeline), queued with the step on every launch order.  It depends on the
// step's per-pixel kernel and on nothing of the foreground back half:
//   stream A, right behind the per-pixel launches: k_marker_bits, ONE launch for the step's frames (grid z = frame), on the
//     frames K1 read and the slots' Z planes, into the slots' own bit planes.  On A because everything that orders itself
//     against K1's reads then covers this kernel's as well, with nothing added: oatgpu_track_input_consumed's event, the next
//     step's remap into the two undistort buffers, the reuse of a host-frame staging slot;
//   stream B2 behind an event on A (a lone frame: stream A itself, no cross-queue dependency): the back half of all M x n
//     planes of the step's frames -- launch_blob_table, whose launch count does not depend on M; marker by marker where the
//     row scan's LDS cannot take the set (mkp.table) -- then k_marker_combine, ONE launch, which writes the frame sets' marker
//     records and combined records into the slots' host-mapped record sets; then the slots' marker event.
// ONE scratch set a frame of the step serves every step: the marker work of consecutive steps runs in order on B2, and a
// lone frame is launched with nothing outstanding -- every earlier frame set was collected, its marker event waited for.
int launch_marker_work(oatgpu_ctx *c, const oatgpu_ctx::FrameJob *j, int nj, const StepPlan &plan)
{
    const Geom &g = c->g;
    const int n = c->cfg.n_streams, M = c->mk.n;
    const size_t NW = (size_t)g.Palloc / 64, planes = (size_t)M * n;
    hipStream_t A = c->stream, S = plan.inline_back ? A : c->stream_b[oatgpu_ctx::kNB - 1];
    const uint8_t *fr[2] = {};
    const u64 *z[2] = {}, *src[2] = {};
    u64 *bits[2] = {};
    BlobBuffers bbs[2];
    const ResultRec *res_c[2] = {};
    ResultRec *res[2] = {}, *rec[2] = {};
    MarkerCombined *comb[2] = {};
    MarkerFiltered *filt[2] = {};
    for (int i = 0; i < nj; ++i) {
        const int slot = j[i].slot;
        fr[i] = step_frame(c, i, j[i].frames);
        z[i] = thr_buf(c, slot);
        src[i] = bits[i] = c->mkp.planes + (size_t)slot * planes * NW;
        u64 *own = c->mkp.masks + (size_t)slot * 3 * planes * NW;
        bbs[i] = c->mkp.bb[i].b;
        bbs[i].tmp = own; bbs[i].morph = own + planes * NW; bbs[i].fin = own + 2 * planes * NW;
        res_c[i] = res[i] = c->mkp.res + (size_t)i * planes;
        rec[i] = (ResultRec *)((char *)c->mkp.rec.dev() + (size_t)slot * c->mkp.set_bytes);
        comb[i] = (MarkerCombined *)(rec[i] + planes);
        filt[i] = (MarkerFiltered *)(comb[i] + n);
        c->mkp.ev_of[(size_t)slot] = j[nj - 1].slot;
    }
    launch_marker_bits_frames(g, fr, c->cfg.channels, z, c->mk.win, M, bits, n, nj, A);
    HIPCHK(c, hipGetLastError());
    if (S != A) {
        HIPCHK(c, hipEventRecord(c->mkp.bits_ev, A));
        HIPCHK(c, hipStreamWaitEvent(S, c->mkp.bits_ev, 0));
        c->b_used[oatgpu_ctx::kNB - 1] = true;
    }
    if (c->mkp.table) {
        launch_blob_table(g, bbs, src, c->mkp.tab, c->mkp.max_dil, res, (int)planes, nj, S);
        for (int i = 0; i < nj; ++i)
            for (int m = 0; m < M; ++m) c->mkp.tap_morph[(size_t)j[i].slot * M + m] = bbs[i].morph + (size_t)m * n * NW;
    } else {
        for (int i = 0; i < nj; ++i)
            for (int m = 0; m < M; ++m) {                     // marker m's planes are "streams" m n .. m n + n - 1 of the set
                const oatgpu_marker &k = c->mk.def[(size_t)m];
                const MorphPlan mp = plan_morph(g, k.erode, k.dilate);
                const MorphIssued mi = issue_morph(g, mp, bbs[i], src[i], m * n, n, S);
                c->mkp.tap_morph[(size_t)j[i].slot * M + m] = mi.tap + (size_t)m * n * NW;
                launch_blob(g, bbs[i], mi.src, mi.ero, mp.dil, k.min_area, k.max_area, res[i], m * n, n, S, kBlobFull);
            }
    }
    HIPCHK(c, hipGetLastError());
    launch_marker_combine_frames(res_c, M, c->mk.anchor, n, comb, rec, nj, S);
    HIPCHK(c, hipGetLastError());
    if (c->mf.on) {       // the chain, behind the combiner and before the event: the filtered records are final when it fires
        launch_marker_filters(c->mf.params, c->mf.state, comb, filt, n, nj, S);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(c->mkp.ev[(size_t)j[nj - 1].slot], S));
    return OATGPU_OK;
}

extern "C" int oatgpu_track_markers_dev(oatgpu_ctx *c, const void *frames_dev, double lr, oatgpu_position *fg,
                                        oatgpu_position *markers, oatgpu_combined *mean)
{
    static_assert(sizeof(oatgpu_combined) == sizeof(MarkerCombined), "k_marker_combine writes oatgpu_combined's layout");
    if (!c) return OATGPU_E_INVALID;
    if (!frames_dev || !markers) return fail(c, OATGPU_E_INVALID, "null argument");
    // ---- 1. refusals, before anything has moved ----
    { const int rrc = marker_step_refusals(c); if (rrc) return rrc; }
    const Geom &g = c->g;
    const int n = c->cfg.n_streams, M = c->mk.n;
    const size_t NW = (size_t)g.Palloc / 64;
    // ---- 2. the existing step, unchanged: enqueue + collect ----
    std::vector<oatgpu_position> fg_own;
    if (!fg) { fg_own.resize((size_t)n); fg = fg_own.data(); }
    const bool pipe = c->mkp.on;          // (the step's own marker work follows: nothing of the pipelined path's for this frame)
    c->mkp.on = false;
    int rc = oatgpu_track_batch_dev(c, frames_dev, lr, fg);
    c->mkp.on = pipe;
    if (rc) return rc;
    c->mkp.last_slot = -1;
    // ---- 3. every marker's mask from the frames the per-pixel kernel read and the Z plane it has just written ----
    hipStream_t A = c->stream;
    const uint8_t *seen = step_frame(c, 0, frames_dev);
    launch_marker_bits(g, seen, c->cfg.channels, thr_buf(c, c->last_slot), c->mk.win, M, c->mk.planes, n, A);
    HIPCHK(c, hipGetLastError());
    // ---- 4. each marker's back half on its plane, with its erode / dilate / area ----
    for (int m = 0; m < M; ++m) {
        const oatgpu_marker &k = c->mk.def[(size_t)m];
        BlobBuffers bb = c->mk.bb.b;
        u64 *own = c->mk.masks + (size_t)m * 3 * n * NW;
        bb.tmp = own; bb.morph = own + (size_t)n * NW; bb.fin = own + 2 * (size_t)n * NW;
        const MorphPlan mp = plan_morph(g, k.erode, k.dilate);
        const MorphIssued mi = issue_morph(g, mp, bb, c->mk.planes + (size_t)m * n * NW, 0, n, A);
        c->mk.tap_morph[(size_t)m] = mi.tap;
        launch_blob(g, bb, mi.src, mi.ero, mp.dil, k.min_area, k.max_area, c->mk.res + (size_t)m * n, 0, n, A, kBlobFull);
        HIPCHK(c, hipGetLastError());
    }
    // ---- 5. posicom mean, one copy back, one synchronisation ----
    MarkerCombined *comb_dev = (MarkerCombined *)(c->mk.res + (size_t)M * n);
    launch_marker_combine(c->mk.res, M, c->mk.anchor, n, comb_dev, A);
    HIPCHK(c, hipGetLastError());
    if (c->mf.on) {       // the chain, behind the combiner and before the copy back
        const MarkerCombined *comb_c = comb_dev;
        MarkerFiltered *filt = c->mf.out;
        launch_marker_filters(c->mf.params, c->mf.state, &comb_c, &filt, n, 1, A);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(c->mf.out_host.host(), c->mf.out, (size_t)n * sizeof(MarkerFiltered), hipMemcpyDeviceToHost, A));
    }
    const size_t res_bytes = (size_t)M * n * sizeof(ResultRec) + (size_t)n * sizeof(MarkerCombined);
    HIPCHK(c, hipMemcpyAsync(c->mk.res_host.host(), c->mk.res, res_bytes, hipMemcpyDeviceToHost, A));
    HIPCHK(c, hipStreamSynchronize(A));
    const ResultRec *r = c->mk.res_host.host();
    for (int s = 0; s < n; ++s)
        for (int m = 0; m < M; ++m) to_position(r[(size_t)m * n + s], &markers[(size_t)s * M + m]);
    if (mean) memcpy(mean, r + (size_t)M * n, (size_t)n * sizeof(oatgpu_combined));
    if (c->mf.on) { c->mf.last.begin(); c->mf.last.keep((size_t)c->cfg.n_streams, c->mf.out_host.host()); }
    return OATGPU_OK;
}

// The filter chain behind the combined record: `posifilt kalman` -> `posifilt homography` -> `posifilt region` (oatgpu.h).  The
// chain's host side is api_trackfilt.hip's and configure_chain's (oatgpu_ctx.h); the marker chain's own: its precondition, the
// synchronous step's output buffers, its texts.
extern "C" int oatgpu_set_marker_filters(oatgpu_ctx *c, const oatgpu_marker_filters *f)
{
    if (!c) return OATGPU_E_INVALID;
    const char *refused = c->mk.n == 0 ? "marker sets are not configured (oatgpu_set_markers)" : nullptr;
    return configure_chain(c, c->mf, f, "marker", refused, [](MarkerFilters &mf, size_t n) {
        return mf.out.alloc(n * sizeof(MarkerFiltered)) == hipSuccess &&
               mf.out_host.alloc(n * sizeof(MarkerFiltered), hipHostMallocDefault) == hipSuccess;
    });
}

extern "C" int oatgpu_marker_filtered(oatgpu_ctx *c, oatgpu_filtered *out, int32_t max_sets)
{
    if (!c || !out) return fail(c, OATGPU_E_INVALID, "null argument");
    return chain_hand_out(c, c->mf, "marker", "no marker result has been delivered since the filter chain was configured", out, max_sets);
}

extern "C" int oatgpu_track_markers(oatgpu_ctx *c, const uint8_t *const *frames_host, int32_t n, double lr, oatgpu_position *fg,
                                    oatgpu_position *markers, oatgpu_combined *mean)
{
    if (!c || !frames_host || !markers) return fail(c, OATGPU_E_INVALID, "null argument");
    if (n != c->cfg.n_streams) return fail(c, OATGPU_E_INVALID, "expected %d frames, got %d", c->cfg.n_streams, n);
    { const int rrc = marker_step_refusals(c); if (rrc) return rrc; }           // (before the staging buffer is written)
    for (int s = 0; s < n; ++s) if (!frames_host[s]) return fail(c, OATGPU_E_INVALID, "null frame %d", s);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    { const int rc = upload_frames(c, frames_host, track_in_bytes(c)); if (rc) return rc; }
    return oatgpu_track_markers_dev(c, c->frames, lr, fg, markers, mean);
}

extern "C" int oatgpu_read_marker_mask(oatgpu_ctx *c, int32_t s, int32_t marker, int32_t which, uint8_t *out)
{
    int rc = check_marker_ix(c, s, marker);
    if (rc) return rc;
    if (!out) return fail(c, OATGPU_E_INVALID, "null argument");
    rc = open_sync(c);
    if (rc) return rc;
    const size_t n = c->cfg.n_streams, NW = (size_t)c->g.Palloc / 64;
    // the planes of the frame set collected last: a ring slot's (the pipelined path), or the synchronous step's
    const size_t M = (size_t)c->mk.n, slot = (size_t)(c->mkp.last_slot < 0 ? 0 : c->mkp.last_slot);
    const bool piped = c->mkp.on && c->mkp.last_slot >= 0;
    const u64 *base = which == OATGPU_TAP_THRESHOLD ? (piped ? c->mkp.planes + (slot * M + marker) * n * NW : c->mk.planes + (size_t)marker * n * NW)
                    : which == OATGPU_TAP_MORPH ? (piped ? c->mkp.tap_morph[slot * M + marker] : c->mk.tap_morph[(size_t)marker])
                    : which == OATGPU_TAP_FINAL ? (piped ? c->mkp.masks + ((slot * 3 + 2) * M + marker) * n * NW
                                                         : c->mk.masks + ((size_t)marker * 3 + 2) * n * NW) : nullptr;
    if (!base) return fail(c, OATGPU_E_INVALID, "unknown tap %d", which);
    return read_plane(c, base + (size_t)s * NW, out);
}
