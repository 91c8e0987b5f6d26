// api_diff.hip -- the motion tracker.
// `framefilt col -C GREY` -> `posidet diff` for every camera of the context (kernels_diff.hip).  The per-stream
// state -- diff_last, diff_have -- is oatgpu_detect_diff's: the two forms continue each other.
#include "oatgpu_ctx.h"

extern "C" int oatgpu_set_diff_tracker(oatgpu_ctx *c, int32_t on)
{
    if (!c) return OATGPU_E_INVALID;
    const size_t n = c->cfg.n_streams, npx = (size_t)c->g.H * c->g.W;
    DevMem<uint8_t> last;                // built aside like the tracker; diff_last stays the context's: it outlives the tracker
    const int rc = set_batched_tracker(c, c->df, on, "diff", [&](DiffTracker &df, bool &ok) {
        ok = c->diff_last || last.alloc(n * npx) == hipSuccess;
        df.last_dilated.assign(n, 0);
        return OATGPU_OK;
    });
    if (!rc && last) c->diff_last = std::move(last);
    return rc;
}

extern "C" int oatgpu_diff_reset(oatgpu_ctx *c, int32_t s)
{
    if (!c) return OATGPU_E_INVALID;
    return reset_have(c, c->diff_have, s);
}

// The front kernel of one frame set (f2: and the next, every stream has a last image) on stream A into the bits of `slot`
// (and slot2).  have[] is the state the frame(s) met; diff_have moves on.  entry: f1's place in the call (tracker_front).
static int diff_front(oatgpu_ctx *c, const void *f1, const void *f2, int slot, int slot2, int entry)
{
    DiffLaunch a{};
    tracker_front(c, c->df, f1, f2, slot, slot2, entry, a);
    a.last = c->diff_last; a.have_last = c->diff_have.data(); a.thr = c->cfg.diff_threshold;
    launch_diff_front(c->g, a, c->cfg.n_streams, c->stream);
    HIPCHK(c, hipGetLastError());
    return OATGPU_OK;
}

// The back half of the frame in `slot` on stream st: once for each maximal run of consecutive streams in the same first-frame
// state (have[s] != 0: blur as dilation; 0: the first frame is analysed as it is), erode never.  Touches neither last_slot nor
// last_morph / last_fin: those stay with the ordinary calls.  Behind it whatever rides on the slot (tracker_tail; prev_slot: the
// slot of the frame before).  With targets on every run takes the global route and ONE k_blob_rank launch behind the last of them
// ranks all streams into the slot's target set.
static int diff_back(oatgpu_ctx *c, int slot, const char *have, hipStream_t st, int prev_slot = -1)
{
    const Geom &g = c->g;
    const int n = c->cfg.n_streams;
    BlobBuffers bb = c->bb[slot].b;
    bb.morph = c->df.mask(slot, 0);
    bb.fin = c->df.mask(slot, 1);
    const u64 *src = c->df.bits_of(slot);
    ResultRec *rd = c->df.rec_dev(slot);
    for (int s0 = 0; s0 < n;) {
        int s1 = s0 + 1;
        while (s1 < n && (have[s1] != 0) == (have[s0] != 0)) ++s1;
        const MorphPlan mp = plan_morph(g, 0, have[s0] ? c->cfg.blur : 0);
        launch_blob(g, bb, src, 0, mp.dil, c->cfg.min_area, c->cfg.max_area, rd, s0, s1 - s0, st, c->tg.k ? kBlobGlobal : kBlobFull);
        for (int s = s0; s < s1; ++s) c->df.last_dilated[(size_t)s] = mp.dil != 0;
        s0 = s1;
    }
    HIPCHK(c, hipGetLastError());
    c->df.last = slot;
    return tracker_tail(c, c->df, bb, rd, slot, prev_slot, st);
}

// one synchronous step on frames in device memory; the context is drained (open_sync)
static int diff_step(oatgpu_ctx *c, const void *frames_dev, oatgpu_position *out)
{
    const std::vector<char> have = c->diff_have;
    tracker_begin(c);
    int rc = diff_front(c, frames_dev, nullptr, 0, 0, 0);
    if (rc) return rc;
    c->diff_have.assign(have.size(), 1);
    rc = diff_back(c, 0, have.data(), c->stream);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    tracker_hand_out(c, c->df, 0, out);
    return OATGPU_OK;
}

extern "C" int oatgpu_diff_batch_dev(oatgpu_ctx *c, const void *frames_dev, oatgpu_position *out)
{
    int rc = check_batch_dev(c, frames_dev, out);
    if (rc) return rc;
    rc = tracker_refusals(c, c->df, "diff", "diff_batch");
    if (rc) return rc;
    rc = open_sync(c);
    if (rc) return rc;
    return diff_step(c, frames_dev, out);
}

extern "C" int oatgpu_diff_batch(oatgpu_ctx *c, const uint8_t *const *frames_host, int32_t n, oatgpu_position *out)
{
    int rc = check_batch(c, frames_host, n, out);
    if (rc) return rc;
    rc = tracker_refusals(c, c->df, "diff", "diff_batch");
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
    int rc = check_sequence_dev(c, frames_dev, n_frames, out);
    if (rc) return rc;
    rc = tracker_refusals(c, c->df, "diff", "diff_sequence");
    if (rc) return rc;
    rc = crop_tensor_room(c, n_frames, "diff_sequence");
    if (!rc) rc = mask_tensor_room(c, n_frames, "diff_sequence");
    if (rc) return rc;
    if (n_frames == 0) return OATGPU_OK;
    rc = open_sync(c);
    if (rc) return rc;
    const int n = c->cfg.n_streams;
    const std::vector<char> all(c->diff_have.size(), 1);
    std::vector<char> have;                // the state the launch's first frame met
    int prev = -1;                         // slot of the frame before (the order of the tracks and of the filter chain)
    tracker_begin(c);
    return run_sequence_in_flight(
        c, n_frames, c->df.ev_front, c->df.ev_done,
        [&](int t) {
            const bool every = std::all_of(c->diff_have.begin(), c->diff_have.end(), [](char h) { return h != 0; });
            return every && t + 1 < n_frames ? 2 : 1;
        },
        [&](int t, int nf, int q, int q2) {
            have = c->diff_have;
            const int r = diff_front(c, frames_dev[t], nf == 2 ? frames_dev[t + 1] : nullptr, q, q2, t);
            if (!r) c->diff_have.assign(have.size(), 1);
            return r;
        },
        [&](int q, int i, hipStream_t B) { return diff_back(c, q, i ? all.data() : have.data(), B, std::exchange(prev, q)); },
        [&](int q, int frame) { tracker_hand_out(c, c->df, q, out + (size_t)frame * n); });
}

extern "C" int oatgpu_read_diff_mask(oatgpu_ctx *c, int32_t s, int32_t which, uint8_t *out)
{
    if (!c) return OATGPU_E_INVALID;
    const int rc = open_tap(c, c->df, "diff", "no diff step has run yet", s, which, out);
    if (rc) return rc;
    const int q = c->df.last;
    const u64 *base = which == OATGPU_TAP_FINAL ? c->df.mask(q, 1)
                    : which == OATGPU_TAP_MORPH && c->df.last_dilated[(size_t)s] ? c->df.mask(q, 0) : c->df.bits_of(q);
    return read_plane(c, base + (size_t)s * (c->g.Palloc >> 6), out);
}
