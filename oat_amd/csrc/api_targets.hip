// api_targets.hip -- multi-target detection: the K largest blobs of every camera, ranked, and their shapes: second
// moments, extents and body axis.
// While targets are on, every back half that delivers a foreground result takes the global blob route (kBlobGlobal) with
// k_blob_rank (kernels_blob.hip) behind it on the same HIP stream, into the target set of the result's slot, and -- while shapes
// are on -- k_blob_shape behind that into the shape set beside it: back_half (api_track.hip: the fused tracker and the single-stage
// detectors) and the batched trackers' tracker_tail (api_trackfilt.hip) call targets_launch; the calls that hand results out keep
// the sets they delivered (targets_begin, targets_keep), so every call that delivers targets delivers shapes.  The derived fields
// of a shape are shape_of's (posfilt_inline.h), on the host.  This unit also owns what stands beside the slots of every home of
// target sets (TargetSets::alloc, rebuild_target_sets) for the whole family: the rider convention is DESIGN.md 9n.
#include "oatgpu_ctx.h"

static_assert(sizeof(oatgpu_shape) == 104, "oatgpu_shape is thirteen 64-bit words");

bool ShapeSets::alloc(size_t slots, size_t n_streams, int k_)
{
    n = n_streams; k = (size_t)k_;
    const size_t recs = slots * n * k;
    bool ok = mem.alloc(recs * sizeof(ShapeRec), hipHostMallocMapped) == hipSuccess;
    ok = ok && accum.alloc(recs * kShapeAccWords * sizeof(u64)) == hipSuccess;
    ok = ok && arrived.alloc(slots * n * sizeof(unsigned)) == hipSuccess;
    ok = ok && hipMemset(accum, 0, recs * kShapeAccWords * sizeof(u64)) == hipSuccess;
    ok = ok && hipMemset(arrived, 0, slots * n * sizeof(unsigned)) == hipSuccess;
    if (ok) memset(mem.host(), 0, recs * sizeof(ShapeRec));
    return ok;
}

bool TargetSets::alloc(const TargetWants &w, size_t slots, size_t n_streams, int channels, bool of_tracker)
{
    if (!w.k) return true;
    n = n_streams; k = (size_t)w.k;
    set_bytes = n * k * sizeof(TargetRec) + n * sizeof(long long);
    if (mem.alloc(slots * set_bytes, hipHostMallocMapped) != hipSuccess) return false;
    memset(mem.host(), 0, slots * set_bytes);
    if (w.shapes && !shp.alloc(slots, n, w.k)) return false;
    if (of_tracker && w.crop_mode && !crp.alloc(slots, n, w.k, w.crop_h, w.crop_w, channels)) return false;
    if (of_tracker && w.tracks) {
        const size_t bytes = slots * n * k * sizeof(TrackRec);
        if (trk.alloc(bytes, hipHostMallocMapped) != hipSuccess) return false;
        memset(trk.host(), 0, bytes);
    }
    return true;
}

int rebuild_target_sets(oatgpu_ctx *c, const TargetWants &w, const char *what)
{
    TargetSets made[3];
    bool ok = true;
    int i = 0;
    for_each_target_home(c, [&](TargetSets &, size_t slots, bool of_tracker, bool on) {
        ok = ok && (!on || made[i].alloc(w, slots, (size_t)c->cfg.n_streams, c->cfg.channels, of_tracker));
        ++i;
    });
    if (!ok) return fail(c, OATGPU_E_NOMEM, "%s: allocation failed: %s", what, hipGetErrorString(hipGetLastError()));
    i = 0;
    for_each_target_home(c, [&](TargetSets &ts, size_t, bool, bool) { ts = std::move(made[i++]); });
    return OATGPU_OK;
}

int targets_launch(oatgpu_ctx *c, const BlobBuffers &bb, const TargetSets &ts, int slot, int s0, int n, hipStream_t st)
{
    if (!c->tg.k) return OATGPU_OK;
    launch_blob_rank(c->g, bb, c->cfg.min_area, c->cfg.max_area, c->tg.k, ts.rec_dev(slot), ts.found_dev(slot), s0, n, st);
    HIPCHK(c, hipGetLastError());
    if (!c->tg.shapes) return OATGPU_OK;
    launch_blob_shape(c->g, bb, c->tg.k, ts.rec_dev(slot), ts.shp.accum_of(slot), ts.shp.arrived_of(slot), ts.shp.rec_dev(slot), s0, n, st);
    HIPCHK(c, hipGetLastError());
    return OATGPU_OK;
}

// the target family's lists start over
void targets_begin(oatgpu_ctx *c)
{
    Targets &tg = c->tg;
    tg.last.begin(); tg.last_found.begin(); tg.last_shapes.begin(); tg.last_crops.begin();
    tg.ct.last_sets = 0;
    tg.mt.last_sets = 0;
}

static oatgpu_shape shape_out(const TargetRec &t, const ShapeRec &r)
{
    oatgpu_shape o{};
    if (!t.valid || !r.valid) return o;
    ShapeDerived d;
    shape_of(t.a00, t.a10, t.a01, r.a20, r.a11, r.a02, d);
    o.valid = 1;
    o.axis_valid = d.axis_valid;
    o.a20 = r.a20; o.a11 = r.a11; o.a02 = r.a02;
    o.x_min = r.x_min; o.y_min = r.y_min; o.x_max = r.x_max; o.y_max = r.y_max;
    o.mu20 = d.mu20; o.mu11 = d.mu11; o.mu02 = d.mu02;
    o.axis_x = d.axis_x; o.axis_y = d.axis_y;
    o.major = d.major; o.minor = d.minor;
    return o;
}

void targets_keep(oatgpu_ctx *c, const TargetSets &ts, int slot, int only)
{
    Targets &tg = c->tg;
    if (!tg.k) return;
    const size_t n = (size_t)c->cfg.n_streams, k = (size_t)tg.k;
    oatgpu_position *pos = tg.last.keep(n * k);
    int32_t *n_found = tg.last_found.keep(n);
    oatgpu_shape *shapes = tg.shapes ? tg.last_shapes.keep(n * k) : nullptr;
    const TargetRec *rec = ts.rec_host(slot);
    const long long *found = ts.found_host(slot);
    for (size_t s = 0; s < n; ++s) {
        const bool have = only < 0 || (size_t)only == s;          // (a single-stage detector analyses one stream: the others are empty)
        n_found[s] = have ? (int32_t)found[s] : 0;
        for (size_t j = 0; j < k; ++j) {
            const TargetRec t = have ? rec[s * k + j] : TargetRec{};
            ResultRec r{};
            r.a00 = t.a00; r.a10 = t.a10; r.a01 = t.a01; r.first_pixel = t.first_pixel; r.valid = t.valid;
            to_position(r, &pos[s * k + j]);
            if (shapes) shapes[s * k + j] = shape_out(t, ts.shp.rec_host(slot)[s * k + j]);
        }
    }
}

extern "C" int oatgpu_set_targets(oatgpu_ctx *c, int32_t k)
{
    if (!c) return OATGPU_E_INVALID;
    if (k < 0 || k > kMaxTargets) return fail(c, OATGPU_E_INVALID, "targets must be in 0..%d", kMaxTargets);
    if (c->ring_count || c->staged_count) return fail(c, OATGPU_E_INVALID, "set_targets while enqueued results are outstanding");
    if (c->tk.on) return fail(c, OATGPU_E_INVALID, "set_targets while tracks are on: switch tracks off first (oatgpu_set_tracks)");
    if (c->tg.shapes) return fail(c, OATGPU_E_INVALID, "set_targets while target shapes are on: switch them off first (oatgpu_set_target_shapes)");
    if (c->tg.crop_mode) return fail(c, OATGPU_E_INVALID, "set_targets while target crops are on: switch them off first (oatgpu_set_target_crops)");
    if (c->tg.ct.mode) return fail(c, OATGPU_E_INVALID, "set_targets while crop tensors are on: switch them off first (oatgpu_set_target_crop_tensor)");
    if (c->tg.mt.mode) return fail(c, OATGPU_E_INVALID, "set_targets while target masks are on: switch them off first (oatgpu_set_target_mask_tensor)");
    if (k > 0 && c->deferred) return fail(c, OATGPU_E_INVALID, "set_targets with deferred completion on (oatgpu_set_deferred) is not supported");
    if (k > 0 && c->mk.n) return fail(c, OATGPU_E_INVALID, "set_targets with marker sets configured (oatgpu_set_markers) is not supported");
    int rc = open_sync(c);
    if (rc) return rc;
    TargetWants w{};                     // (every rider is off, see above)
    w.k = k;
    rc = rebuild_target_sets(c, w, "targets");
    if (rc) return rc;
    TargetSets ring = std::move(c->tg.ring);
    c->tg = {};
    c->tg.k = k;
    c->tg.ring = std::move(ring);
    c->tg.last.items.reserve((size_t)c->cfg.n_streams * (size_t)k);
    c->tg.last_found.items.reserve((size_t)c->cfg.n_streams);
    return OATGPU_OK;
}

extern "C" int oatgpu_targets(oatgpu_ctx *c, oatgpu_position *out, int32_t *n_found, int32_t max_sets)
{
    if (!c || !out || !n_found) return fail(c, OATGPU_E_INVALID, "null argument");
    const Targets &tg = c->tg;
    const int sets = delivered_to(c, tg.last, tg.k != 0, "targets are off (oatgpu_set_targets)",
                                  "no call has delivered a result since targets were switched on", out, max_sets);
    if (sets > 0) memcpy(n_found, tg.last_found.items.data(), (size_t)sets * tg.last_found.per * sizeof(int32_t));     // (kept set for set with last)
    return sets;
}

extern "C" int oatgpu_set_target_shapes(oatgpu_ctx *c, int32_t on)
{
    if (!c) return OATGPU_E_INVALID;
    if (c->ring_count || c->staged_count) return fail(c, OATGPU_E_INVALID, "set_target_shapes while enqueued results are outstanding");
    if (!c->tg.k) return fail(c, OATGPU_E_INVALID, "set_target_shapes: targets are off (oatgpu_set_targets)");
    int rc = open_sync(c);
    if (rc) return rc;
    Targets &tg = c->tg;
    if (!on && tg.crop_mode == OATGPU_CROP_AXIS)
        return fail(c, OATGPU_E_INVALID, "set_target_shapes(0) while target crops follow the body axis: switch them off first (oatgpu_set_target_crops)");
    if (!on && tg.ct.mode == OATGPU_CROP_AXIS)
        return fail(c, OATGPU_E_INVALID, "set_target_shapes(0) while crop tensors follow the body axis: switch them off first (oatgpu_set_target_crop_tensor)");
    if (!on && tg.mt.mode == OATGPU_CROP_AXIS)
        return fail(c, OATGPU_E_INVALID, "set_target_shapes(0) while target masks follow the body axis: switch them off first (oatgpu_set_target_mask_tensor)");
    if (!on) {
        tg.shapes = false;
        tg.last_shapes.begin();
        for_each_target_home(c, [](TargetSets &ts, size_t, bool, bool) { ts.shp = {}; });
        return OATGPU_OK;
    }
    TargetWants w = wants_of(c);
    w.shapes = true;
    rc = rebuild_target_sets(c, w, "target shapes");
    if (rc) return rc;
    tg.shapes = true;
    targets_begin(c);                    // a target set kept from before has no shape set beside it
    tg.last_shapes.items.reserve((size_t)c->cfg.n_streams * (size_t)tg.k);
    return OATGPU_OK;
}

extern "C" int oatgpu_target_shapes(oatgpu_ctx *c, oatgpu_shape *out, int32_t max_sets)
{
    if (!c || !out) return fail(c, OATGPU_E_INVALID, "null argument");
    return delivered_to(c, c->tg.last_shapes, c->tg.shapes, "target shapes are off (oatgpu_set_target_shapes)",
                        "no call has delivered a result since target shapes were switched on", out, max_sets);
}
