// api_bsubtrack.hip -- the subtraction tracker.
// `framefilt bsub` -> `framefilt col -C HSV` -> `posidet hsv` (GREY contexts: `framefilt bsub` -> `posidet thresh`) for every camera
// of the context (kernels_bsubtrack.hip).  The per-stream state -- bsub_bg, bsub_f, bsub_have -- is
// oatgpu_bsub_filter's: the two forms continue each other, oatgpu_bsub_set_background serves both.
#include "oatgpu_ctx.h"

static size_t frame_bytes(const oatgpu_ctx *c) { return (size_t)c->g.H * c->g.W * c->cfg.channels; }

extern "C" int oatgpu_set_bsub_tracker(oatgpu_ctx *c, int32_t on)
{
    if (!c) return OATGPU_E_INVALID;
    // (the background planes stay the context's: they outlive the tracker)
    return set_batched_tracker(c, c->bs, on, "bsub", [&](BsubTracker &, bool &) { return ensure_bsub(c, frame_bytes(c)); });
}

extern "C" int oatgpu_bsub_reset(oatgpu_ctx *c, int32_t s)
{
    if (!c) return OATGPU_E_INVALID;
    return reset_have(c, c->bsub_have, s);
}

// what a step refuses, checked before anything is read or has moved
static int bsub_refusals(oatgpu_ctx *c, const char *what, double alpha)
{
    const int rc = tracker_refusals(c, c->bs, "bsub", what);
    if (rc) return rc;
    if (!(alpha >= 0.0 && alpha <= 1.0)) return fail(c, OATGPU_E_INVALID, "adaptation-coeff must be in [0,1]");
    if (alpha > 0.0)                    // the reference's accumulateWeighted asserts on its empty fp32 image
        for (int s = 0; s < c->cfg.n_streams; ++s)
            if (c->bsub_have[(size_t)s] == 2)
                return fail(c, OATGPU_E_INVALID, "stream %d: a background image from a file cannot adapt (adaptation-coeff must be 0)", s);
    return OATGPU_OK;
}

// The front kernel of one frame set (f2: and the next) on stream A into the bits of `slot` (and slot2).  bsub_have is the state
// the first frame met; it moves on.  entry: f1's place in the call (tracker_front).
static int bsub_front(oatgpu_ctx *c, const void *f1, const void *f2, double alpha, int slot, int slot2, int entry)
{
    BsubLaunch a{};
    tracker_front(c, c->bs, f1, f2, slot, slot2, entry, a);
    a.bg = c->bsub_bg; a.acc = c->bsub_f; a.have = c->bsub_have.data();
    a.rp = range_of(detector_of(c->cfg));
    a.learn = alpha > 0.0; a.a = (float)alpha; a.b = 1 - a.a;        // accW_: AT a = (AT)alpha, b = 1 - a
    launch_bsubtrack_front(c->g, a, c->cfg.n_streams, c->stream);
    HIPCHK(c, hipGetLastError());
    for (auto &h : c->bsub_have) if (!h) h = 1;
    return OATGPU_OK;
}

// The back half of the frame in `slot` on stream st, every stream in one launch sequence: the context's erode / dilate and area
// window.  Touches neither last_slot nor last_morph / last_fin: those stay with the ordinary calls.  Behind it whatever rides on
// the slot (tracker_tail; prev_slot: the slot of the frame before).
static int bsub_back(oatgpu_ctx *c, int slot, hipStream_t st, int prev_slot = -1)
{
    const Geom &g = c->g;
    const int n = c->cfg.n_streams;
    BlobBuffers bb = c->bb[slot].b;
    bb.tmp = c->bs.mask(slot, 0);
    bb.morph = c->bs.mask(slot, 1);
    bb.fin = c->bs.mask(slot, 2);
    const MorphPlan mp = plan_morph(g, c->cfg.erode, c->cfg.dilate);
    const MorphIssued m = issue_morph(g, mp, bb, c->bs.bits_of(slot), 0, n, st);
    ResultRec *rd = c->bs.rec_dev(slot);
    launch_blob(g, bb, m.src, m.ero, mp.dil, c->cfg.min_area, c->cfg.max_area, rd, 0, n, st, c->tg.k ? kBlobGlobal : kBlobFull);
    HIPCHK(c, hipGetLastError());
    c->bs.last = slot;
    c->bs.last_tap = m.tap;
    return tracker_tail(c, c->bs, bb, rd, slot, prev_slot, st);
}

// one synchronous step on frames in device memory; the context is drained (open_sync)
static int bsub_step(oatgpu_ctx *c, const void *frames_dev, double alpha, oatgpu_position *out)
{
    tracker_begin(c);
    int rc = bsub_front(c, frames_dev, nullptr, alpha, 0, 0, 0);
    if (rc) return rc;
    rc = bsub_back(c, 0, c->stream);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    tracker_hand_out(c, c->bs, 0, out);
    return OATGPU_OK;
}

extern "C" int oatgpu_bsub_track_batch_dev(oatgpu_ctx *c, const void *frames_dev, double alpha, oatgpu_position *out)
{
    int rc = check_batch_dev(c, frames_dev, out);
    if (rc) return rc;
    rc = bsub_refusals(c, "bsub_track_batch", alpha);
    if (rc) return rc;
    rc = open_sync(c);
    if (rc) return rc;
    return bsub_step(c, frames_dev, alpha, out);
}

extern "C" int oatgpu_bsub_track_batch(oatgpu_ctx *c, const uint8_t *const *frames_host, int32_t n, double alpha, oatgpu_position *out)
{
    int rc = check_batch(c, frames_host, n, out);
    if (rc) return rc;
    rc = bsub_refusals(c, "bsub_track_batch", alpha);
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
    int rc = check_sequence_dev(c, frames_dev, n_frames, out);
    if (rc) return rc;
    rc = bsub_refusals(c, "bsub_track_sequence", alpha);
    if (rc) return rc;
    rc = crop_tensor_room(c, n_frames, "bsub_track_sequence");
    if (!rc) rc = mask_tensor_room(c, n_frames, "bsub_track_sequence");
    if (rc) return rc;
    if (n_frames == 0) return OATGPU_OK;
    rc = open_sync(c);
    if (rc) return rc;
    const int n = c->cfg.n_streams;
    int prev = -1;                         // slot of the frame before (the order of the tracks and of the filter chain)
    tracker_begin(c);
    return run_sequence_in_flight(
        c, n_frames, c->bs.ev_front, c->bs.ev_done, [&](int t) { return t + 1 < n_frames ? 2 : 1; },
        [&](int t, int nf, int q, int q2) { return bsub_front(c, frames_dev[t], nf == 2 ? frames_dev[t + 1] : nullptr, alpha, q, q2, t); },
        [&](int q, int, hipStream_t B) { return bsub_back(c, q, B, std::exchange(prev, q)); },
        [&](int q, int frame) { tracker_hand_out(c, c->bs, q, out + (size_t)frame * n); });
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
    if (!c) return OATGPU_E_INVALID;
    const int rc = open_tap(c, c->bs, "bsub", "no bsub tracker step has run yet", s, which, out);
    if (rc) return rc;
    const int q = c->bs.last;
    const u64 *base = which == OATGPU_TAP_FINAL ? c->bs.mask(q, 2) : which == OATGPU_TAP_MORPH ? c->bs.last_tap : c->bs.bits_of(q);
    return read_plane(c, base + (size_t)s * (c->g.Palloc >> 6), out);
}
