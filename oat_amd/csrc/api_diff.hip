// api_diff.hip -- the motion tracker.
// `framefilt col -C GREY` -> `posidet diff` for every camera of the context (kernels_diff.hip).  The per-stream
// state -- diff_last, diff_have -- is oatgpu_detect_diff's: the two forms continue each other.
#include "oatgpu_ctx.h"

extern "C" int oatgpu_set_diff_tracker(oatgpu_ctx *c, int32_t on)
{
    if (!c) return OATGPU_E_INVALID;
    if (c->ring_count || c->staged_count) return fail(c, OATGPU_E_INVALID, "set_diff_tracker while enqueued results are outstanding");
    if (!on) {
        if (!c->df.on) return OATGPU_OK;
        const int rc = open_sync(c);
        if (rc) return rc;
        c->df = {};
        return OATGPU_OK;
    }
    if (c->df.on) return OATGPU_OK;
    const int rc = open_sync(c);
    if (rc) return rc;
    const Geom &g = c->g;
    const size_t n = c->cfg.n_streams, NW = (size_t)g.Palloc / 64, K = DiffTracker::kSlots, npx = (size_t)g.H * g.W;
    DiffTracker df;                      // built aside: the context takes it when everything worked
    DevMem<uint8_t> last;
    bool ok = c->diff_last || last.alloc(n * npx) == hipSuccess;
    ok = ok && df.bits.alloc(K * n * NW * 8) == hipSuccess;
    ok = ok && df.masks.alloc(K * 2 * n * NW * 8) == hipSuccess;
    ok = ok && df.rec.alloc(K * n * sizeof(ResultRec), hipHostMallocMapped) == hipSuccess;
    // (the taps: words beyond the frame are never written by the back half)
    ok = ok && hipMemsetAsync(df.bits, 0, K * n * NW * 8, c->stream) == hipSuccess;
    ok = ok && hipMemsetAsync(df.masks, 0, K * 2 * n * NW * 8, c->stream) == hipSuccess;
    for (auto &e : df.ev_front) ok = ok && e.create(hipEventDisableTiming | hipEventDisableSystemFence) == hipSuccess;
    for (auto &e : df.ev_done) ok = ok && e.create(hipEventDisableTiming) == hipSuccess;
    ok = ok && hipStreamSynchronize(c->stream) == hipSuccess;
    if (!ok) return fail(c, OATGPU_E_NOMEM, "diff tracker: allocation failed: %s", hipGetErrorString(hipGetLastError()));
    df.last_dilated.assign(n, 0);
    df.on = true;
    if (!c->diff_last) c->diff_last = std::move(last);
    c->df = std::move(df);
    return OATGPU_OK;
}

extern "C" int oatgpu_diff_reset(oatgpu_ctx *c, int32_t s)
{
    if (!c) return OATGPU_E_INVALID;
    if (s < -1 || s >= c->cfg.n_streams) return fail(c, OATGPU_E_INVALID, "stream index %d out of range", s);
    if (s < 0) c->diff_have.assign((size_t)c->cfg.n_streams, 0);
    else c->diff_have[(size_t)s] = 0;
    return OATGPU_OK;
}

// what a diff step refuses, checked before anything is read or has moved
static int diff_refusals(oatgpu_ctx *c, const char *what)
{
    if (!c->df.on) return fail(c, OATGPU_E_INVALID, "the diff tracker is off (oatgpu_set_diff_tracker)");
    if (c->ring_count || c->staged_count) return fail(c, OATGPU_E_INVALID, "%s while enqueued results are outstanding", what);
    if (c->kal_on) return fail(c, OATGPU_E_INVALID, "%s with the position filter on (oatgpu_set_kalman) is not supported", what);
    if (c->homo_on) return fail(c, OATGPU_E_INVALID, "%s with a homography on (oatgpu_set_homography) is not supported", what);
    if (c->ud_track) return fail(c, OATGPU_E_INVALID, "%s with undistortion on (oatgpu_set_track_undistort) is not supported", what);
    if (c->by_track) return fail(c, OATGPU_E_INVALID, "%s with Bayer frames on (oatgpu_set_track_bayer) is not supported", what);
    return OATGPU_OK;
}

static u64 *diff_bits(oatgpu_ctx *c, int slot) { return c->df.bits + (size_t)slot * c->cfg.n_streams * (c->g.Palloc >> 6); }
static u64 *diff_mask(oatgpu_ctx *c, int slot, int which) { return c->df.masks + ((size_t)slot * 2 + which) * c->cfg.n_streams * (c->g.Palloc >> 6); }

// The front kernel of one frame set (f2: and the next, every stream has a last image) on stream A into the bits of `slot`
// (and slot2).  have[] is the state the frame(s) met; diff_have moves on.
static int diff_front(oatgpu_ctx *c, const void *f1, const void *f2, int slot, int slot2)
{
    DiffLaunch a{};
    a.frames = (const uint8_t *)f1; a.frames2 = (const uint8_t *)f2; a.channels = c->cfg.channels; a.last = c->diff_last;
    a.have_last = c->diff_have.data(); a.bits = diff_bits(c, slot); a.bits2 = f2 ? diff_bits(c, slot2) : nullptr;
    a.roi = c->roi; a.thr = c->cfg.diff_threshold; a.bayer = tracker_bayer(c);
    tracker_undistort(c, a);
    launch_diff_front(c->g, a, c->cfg.n_streams, c->stream);
    HIPCHK(c, hipGetLastError());
    return OATGPU_OK;
}

// The back half of the frame in `slot` on stream st: once for each maximal run of consecutive streams in the same first-frame
// state (have[s] != 0: blur as dilation; 0: the first frame is analysed as it is), erode never.  Touches neither last_slot nor
// last_morph / last_fin: those stay with the ordinary calls.  Behind it the filter chain on the slot's records, where one is
// configured (prev_slot: tracker_filters_launch).
static int diff_back(oatgpu_ctx *c, int slot, const char *have, hipStream_t st, int prev_slot = -1)
{
    const Geom &g = c->g;
    const int n = c->cfg.n_streams;
    BlobBuffers bb = c->bb[slot].b;
    bb.morph = diff_mask(c, slot, 0);
    bb.fin = diff_mask(c, slot, 1);
    const u64 *src = diff_bits(c, slot);
    ResultRec *rd = c->df.rec.dev() + (size_t)slot * n;
    for (int s0 = 0; s0 < n;) {
        int s1 = s0 + 1;
        while (s1 < n && (have[s1] != 0) == (have[s0] != 0)) ++s1;
        const MorphPlan mp = plan_morph(g, 0, have[s0] ? c->cfg.blur : 0);
        launch_blob(g, bb, src, 0, mp.dil, c->cfg.min_area, c->cfg.max_area, rd, s0, s1 - s0, st, kBlobFull);
        for (int s = s0; s < s1; ++s) c->df.last_dilated[(size_t)s] = mp.dil != 0;
        s0 = s1;
    }
    HIPCHK(c, hipGetLastError());
    c->df.last = slot;
    return tracker_filters_launch(c, rd, slot, prev_slot, st);
}

static void diff_hand_out(oatgpu_ctx *c, int slot, oatgpu_position *out)
{
    const int n = c->cfg.n_streams;
    for (int s = 0; s < n; ++s) to_position(c->df.rec.host()[(size_t)slot * n + s], out + s);
    tracker_filters_keep(c, slot);
}

// one synchronous step on frames in device memory; the context is drained (open_sync)
static int diff_step(oatgpu_ctx *c, const void *frames_dev, oatgpu_position *out)
{
    const std::vector<char> have = c->diff_have;
    tracker_filters_begin(c);
    int rc = diff_front(c, frames_dev, nullptr, 0, 0);
    if (rc) return rc;
    c->diff_have.assign(have.size(), 1);
    rc = diff_back(c, 0, have.data(), c->stream);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    diff_hand_out(c, 0, out);
    return OATGPU_OK;
}

extern "C" int oatgpu_diff_batch_dev(oatgpu_ctx *c, const void *frames_dev, oatgpu_position *out)
{
    if (!c) return OATGPU_E_INVALID;
    if (!frames_dev || !out) return fail(c, OATGPU_E_INVALID, "null argument");
    int rc = diff_refusals(c, "diff_batch");
    if (rc) return rc;
    rc = open_sync(c);
    if (rc) return rc;
    return diff_step(c, frames_dev, out);
}

extern "C" int oatgpu_diff_batch(oatgpu_ctx *c, const uint8_t *const *frames_host, int32_t n, oatgpu_position *out)
{
    if (!c) return OATGPU_E_INVALID;
    if (!frames_host || !out) return fail(c, OATGPU_E_INVALID, "null argument");
    if (n != c->cfg.n_streams) return fail(c, OATGPU_E_INVALID, "expected %d frames, got %d", c->cfg.n_streams, n);
    for (int s = 0; s < n; ++s) if (!frames_host[s]) return fail(c, OATGPU_E_INVALID, "null frame %d", s);
    int rc = diff_refusals(c, "diff_batch");
    if (rc) return rc;
    rc = open_sync(c);
    if (rc) return rc;
    rc = upload_frames(c, frames_host, tracker_in_bytes(c));
    if (rc) return rc;
    return diff_step(c, c->frames, out);
}

// A recorded sequence: up to four frames in flight.  Front launches on stream A -- two frames a launch wherever both have a last
// image --, frame t's back half on B[t % 3] behind the front launch's event, in slot t % 4 (scratch set, bits, masks, records);
// a slot is reused only after its result has been collected.  Everything is collected before the call returns.
extern "C" int oatgpu_diff_sequence_dev(oatgpu_ctx *c, const void *const *frames_dev, int32_t n_frames, oatgpu_position *out)
{
    if (!c) return OATGPU_E_INVALID;
    if (n_frames < 0) return fail(c, OATGPU_E_INVALID, "n_frames must be >= 0");
    if (!frames_dev || (!out && n_frames > 0)) return fail(c, OATGPU_E_INVALID, "null argument");
    for (int t = 0; t < n_frames; ++t) if (!frames_dev[t]) return fail(c, OATGPU_E_INVALID, "null frame set %d", t);
    int rc = diff_refusals(c, "diff_sequence");
    if (rc) return rc;
    if (n_frames == 0) return OATGPU_OK;
    rc = open_sync(c);
    if (rc) return rc;
    static_assert(DiffTracker::kSlots == kSeqSlots, "the sequence loop's slots are the tracker's");
    const int n = c->cfg.n_streams;
    const std::vector<char> all(c->diff_have.size(), 1);
    std::vector<char> have;                // the state the launch's first frame met
    int prev = -1;                         // slot of the frame before (the filter chain's order)
    tracker_filters_begin(c);
    return run_sequence_in_flight(
        c, n_frames, c->df.ev_front, c->df.ev_done,
        [&](int t) {
            const bool every = std::all_of(c->diff_have.begin(), c->diff_have.end(), [](char h) { return h != 0; });
            return every && t + 1 < n_frames ? 2 : 1;
        },
        [&](int t, int nf, int q, int q2) {
            have = c->diff_have;
            const int r = diff_front(c, frames_dev[t], nf == 2 ? frames_dev[t + 1] : nullptr, q, q2);
            if (!r) c->diff_have.assign(have.size(), 1);
            return r;
        },
        [&](int q, int i, hipStream_t B) { return diff_back(c, q, i ? all.data() : have.data(), B, std::exchange(prev, q)); },
        [&](int q, int frame) { diff_hand_out(c, q, out + (size_t)frame * n); });
}

extern "C" int oatgpu_read_diff_mask(oatgpu_ctx *c, int32_t s, int32_t which, uint8_t *out)
{
    int rc = check_stream_ix(c, s);
    if (rc) return rc;
    if (!out) return fail(c, OATGPU_E_INVALID, "null argument");
    if (!c->df.on) return fail(c, OATGPU_E_INVALID, "the diff tracker is off (oatgpu_set_diff_tracker)");
    if (c->df.last < 0) return fail(c, OATGPU_E_INVALID, "no diff step has run yet");
    if (which != OATGPU_TAP_THRESHOLD && which != OATGPU_TAP_MORPH && which != OATGPU_TAP_FINAL)
        return fail(c, OATGPU_E_INVALID, "unknown tap %d", which);
    rc = open_sync(c);
    if (rc) return rc;
    const int q = c->df.last;
    const u64 *base = which == OATGPU_TAP_FINAL ? diff_mask(c, q, 1)
                    : which == OATGPU_TAP_MORPH && c->df.last_dilated[(size_t)s] ? diff_mask(c, q, 0) : diff_bits(c, q);
    return read_plane(c, base + (size_t)s * (c->g.Palloc >> 6), out);
}
