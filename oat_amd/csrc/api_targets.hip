// api_targets.hip -- multi-target detection: the K largest blobs of every camera, ranked.
// While targets are on, every back half that delivers a foreground result takes the global blob route (kBlobGlobal) with
// k_blob_rank (kernels_blob.hip) behind it on the same HIP stream, into the target set of the result's slot: back_half
// (api_track.hip: the fused tracker and the single-stage detectors), diff_back (api_diff.hip) and bsub_back (api_bsubtrack.hip)
// call targets_launch; the calls that hand results out keep the sets they delivered (targets_begin, targets_keep) for
// oatgpu_targets, the way the filter chains do (api_trackfilt.hip).  Target shapes (api_shapes.hip) ride on these
// three: targets_launch launches k_blob_shape behind the ranking, targets_begin / targets_keep keep the shape sets beside the target sets.
// Target crops (api_crops.hip) ride on them the same way, behind the shapes, and crop tensors (api_croptensor.hip,
// DESIGN.md 9m) behind those.
#include "oatgpu_ctx.h"

bool TargetSets::alloc(size_t slots, size_t n_streams, int k_)
{
    n = n_streams; k = (size_t)k_;
    set_bytes = n * k * sizeof(TargetRec) + n * sizeof(long long);
    if (mem.alloc(slots * set_bytes, hipHostMallocMapped) != hipSuccess) return false;
    memset(mem.host(), 0, slots * set_bytes);
    return true;
}

int targets_launch(oatgpu_ctx *c, const BlobBuffers &bb, const TargetSets &ts, int slot, int s0, int n, hipStream_t st)
{
    if (!c->tg.k) return OATGPU_OK;
    launch_blob_rank(c->g, bb, c->cfg.min_area, c->cfg.max_area, c->tg.k, ts.rec_dev(slot), ts.found_dev(slot), s0, n, st);
    HIPCHK(c, hipGetLastError());
    int rc = shapes_launch(c, bb, ts, slot, s0, n, st);
    if (rc) return rc;
    rc = crops_launch(c, ts, slot, s0, n, st);
    return rc ? rc : crop_tensor_launch(c, ts, slot, s0, n, st);
}

void targets_begin(oatgpu_ctx *c) { c->tg.last_sets = 0; shapes_begin(c); crops_begin(c); crop_tensor_begin(c); }

void targets_keep(oatgpu_ctx *c, const TargetSets &ts, int slot, int only)
{
    Targets &tg = c->tg;
    if (!tg.k) return;
    const size_t n = (size_t)c->cfg.n_streams, k = (size_t)tg.k, at = (size_t)tg.last_sets;
    tg.last.resize((at + 1) * n * k);
    tg.last_found.resize((at + 1) * n);
    const TargetRec *rec = ts.rec_host(slot);
    const long long *found = ts.found_host(slot);
    for (size_t s = 0; s < n; ++s) {
        const bool have = only < 0 || (size_t)only == s;          // (a single-stage detector analyses one stream: the others are empty)
        tg.last_found[at * n + s] = have ? (int32_t)found[s] : 0;
        for (size_t j = 0; j < k; ++j) {
            ResultRec r{};
            if (have) {
                const TargetRec &t = rec[s * k + j];
                r.a00 = t.a00; r.a10 = t.a10; r.a01 = t.a01; r.first_pixel = t.first_pixel; r.valid = t.valid;
            }
            to_position(r, &tg.last[(at * n + s) * k + j]);
        }
    }
    shapes_keep(c, ts, slot, only);
    crops_keep(c, ts, slot);
    crop_tensor_keep(c, ts);
    tg.last_sets++;
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
    if (k > 0 && c->deferred) return fail(c, OATGPU_E_INVALID, "set_targets with deferred completion on (oatgpu_set_deferred) is not supported");
    if (k > 0 && c->mk.n) return fail(c, OATGPU_E_INVALID, "set_targets with marker sets configured (oatgpu_set_markers) is not supported");
    int rc = open_sync(c);
    if (rc) return rc;
    Targets &tg = c->tg;
    if (k == 0) {
        tg = {};
        c->df.tgt = {}; c->bs.tgt = {};
        return OATGPU_OK;
    }
    // everything is built aside: a failed allocation leaves the context as it was
    const size_t n = (size_t)c->cfg.n_streams;
    TargetSets ring, df, bs;
    bool ok = ring.alloc((size_t)c->ring_slots + 1, n, k);
    ok = ok && (!c->df.on || df.alloc(kSeqSlots, n, k));
    ok = ok && (!c->bs.on || bs.alloc(kSeqSlots, n, k));
    if (!ok) return fail(c, OATGPU_E_NOMEM, "targets: allocation failed: %s", hipGetErrorString(hipGetLastError()));
    tg = {};
    tg.k = k;
    tg.ring = std::move(ring);
    tg.last.reserve(n * (size_t)k);
    tg.last_found.reserve(n);
    c->df.tgt = std::move(df);
    c->bs.tgt = std::move(bs);
    return OATGPU_OK;
}

extern "C" int oatgpu_targets(oatgpu_ctx *c, oatgpu_position *out, int32_t *n_found, int32_t max_sets)
{
    if (!c || !out || !n_found) return fail(c, OATGPU_E_INVALID, "null argument");
    const Targets &tg = c->tg;
    if (!tg.k) return fail(c, OATGPU_E_INVALID, "targets are off (oatgpu_set_targets)");
    if (tg.last_sets == 0) return fail(c, OATGPU_E_INVALID, "no call has delivered a result since targets were switched on");
    if (max_sets < tg.last_sets) return fail(c, OATGPU_E_INVALID, "room for %d frame sets, the latest call delivered %d", max_sets, tg.last_sets);
    const size_t n = (size_t)c->cfg.n_streams;
    memcpy(out, tg.last.data(), (size_t)tg.last_sets * n * (size_t)tg.k * sizeof(oatgpu_position));
    memcpy(n_found, tg.last_found.data(), (size_t)tg.last_sets * n * sizeof(int32_t));
    return tg.last_sets;
}
