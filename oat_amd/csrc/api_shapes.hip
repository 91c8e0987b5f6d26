// api_shapes.hip -- target shapes: second moments, extents and body axis of the K ranked blobs of every camera.
// While shapes are on, targets_launch (api_targets.hip) -- the one place every back half ranks from -- launches k_blob_shape
// (kernels_blob.hip) behind k_blob_rank on the same HIP stream and scratch set, into the shape set that stands beside the slot's
// target set (TargetSets::shp); targets_begin / targets_keep keep the shape sets of what a call delivered beside its target sets,
// so every call that delivers targets delivers shapes.  The derived fields are shape_of's (posfilt_inline.h), on the host.
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

int shapes_launch(oatgpu_ctx *c, const BlobBuffers &bb, const TargetSets &ts, int slot, int s0, int n, hipStream_t st)
{
    if (!c->tg.shapes) return OATGPU_OK;
    launch_blob_shape(c->g, bb, c->tg.k, ts.rec_dev(slot), ts.shp.accum_of(slot), ts.shp.arrived_of(slot), ts.shp.rec_dev(slot), s0, n, st);
    HIPCHK(c, hipGetLastError());
    return OATGPU_OK;
}

void shapes_begin(oatgpu_ctx *c) { c->tg.last_shapes.clear(); }

// (called with tg.last_sets still the index of the set being kept)
void shapes_keep(oatgpu_ctx *c, const TargetSets &ts, int slot, int only)
{
    Targets &tg = c->tg;
    if (!tg.shapes) return;
    const size_t n = (size_t)c->cfg.n_streams, k = (size_t)tg.k, at = (size_t)tg.last_sets;
    tg.last_shapes.resize((at + 1) * n * k);
    const TargetRec *rec = ts.rec_host(slot);
    const ShapeRec *shp = ts.shp.rec_host(slot);
    for (size_t s = 0; s < n; ++s) {
        const bool have = only < 0 || (size_t)only == s;
        for (size_t j = 0; j < k; ++j) {
            oatgpu_shape o{};
            const TargetRec &t = rec[s * k + j];
            const ShapeRec &r = shp[s * k + j];
            if (have && t.valid && r.valid) {
                ShapeDerived d;
                shape_of(t.a00, t.a10, t.a01, r.a20, r.a11, r.a02, d);
                o.valid = 1;
                o.axis_valid = d.axis_valid;
                o.a20 = r.a20; o.a11 = r.a11; o.a02 = r.a02;
                o.x_min = r.x_min; o.y_min = r.y_min; o.x_max = r.x_max; o.y_max = r.y_max;
                o.mu20 = d.mu20; o.mu11 = d.mu11; o.mu02 = d.mu02;
                o.axis_x = d.axis_x; o.axis_y = d.axis_y;
                o.major = d.major; o.minor = d.minor;
            }
            tg.last_shapes[(at * n + s) * k + j] = o;
        }
    }
}

extern "C" int oatgpu_set_target_shapes(oatgpu_ctx *c, int32_t on)
{
    if (!c) return OATGPU_E_INVALID;
    if (c->ring_count || c->staged_count) return fail(c, OATGPU_E_INVALID, "set_target_shapes while enqueued results are outstanding");
    if (!c->tg.k) return fail(c, OATGPU_E_INVALID, "set_target_shapes: targets are off (oatgpu_set_targets)");
    const int rc = open_sync(c);
    if (rc) return rc;
    Targets &tg = c->tg;
    if (!on && tg.crop_mode == OATGPU_CROP_AXIS)
        return fail(c, OATGPU_E_INVALID, "set_target_shapes(0) while target crops follow the body axis: switch them off first (oatgpu_set_target_crops)");
    if (!on && tg.ct.mode == OATGPU_CROP_AXIS)
        return fail(c, OATGPU_E_INVALID, "set_target_shapes(0) while crop tensors follow the body axis: switch them off first (oatgpu_set_target_crop_tensor)");
    if (!on) {
        tg.shapes = false;
        tg.last_shapes.clear();
        tg.ring.shp = {}; c->df.tgt.shp = {}; c->bs.tgt.shp = {};
        return OATGPU_OK;
    }
    // everything is built aside: a failed allocation leaves the context as it was
    const size_t n = (size_t)c->cfg.n_streams;
    ShapeSets ring, df, bs;
    bool ok = ring.alloc((size_t)c->ring_slots + 1, n, tg.k);
    ok = ok && (!c->df.on || df.alloc(kSeqSlots, n, tg.k));
    ok = ok && (!c->bs.on || bs.alloc(kSeqSlots, n, tg.k));
    if (!ok) return fail(c, OATGPU_E_NOMEM, "target shapes: allocation failed: %s", hipGetErrorString(hipGetLastError()));
    tg.ring.shp = std::move(ring);
    c->df.tgt.shp = std::move(df);
    c->bs.tgt.shp = std::move(bs);
    tg.shapes = true;
    // the list starts over, for targets too: a target set kept from before has no shape set beside it
    tg.last_sets = 0;
    tg.last_shapes.clear();
    tg.last_shapes.reserve(n * (size_t)tg.k);
    return OATGPU_OK;
}

extern "C" int oatgpu_target_shapes(oatgpu_ctx *c, oatgpu_shape *out, int32_t max_sets)
{
    if (!c || !out) return fail(c, OATGPU_E_INVALID, "null argument");
    const Targets &tg = c->tg;
    if (!tg.shapes) return fail(c, OATGPU_E_INVALID, "target shapes are off (oatgpu_set_target_shapes)");
    if (tg.last_sets == 0) return fail(c, OATGPU_E_INVALID, "no call has delivered a result since target shapes were switched on");
    if (max_sets < tg.last_sets) return fail(c, OATGPU_E_INVALID, "room for %d frame sets, the latest call delivered %d", max_sets, tg.last_sets);
    memcpy(out, tg.last_shapes.data(), (size_t)tg.last_sets * (size_t)c->cfg.n_streams * (size_t)tg.k * sizeof(oatgpu_shape));
    return tg.last_sets;
}
