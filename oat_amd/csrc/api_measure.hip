// api_measure.hip -- measurement: the bandwidth probe, the traffic audit, the step profile.
#include "oatgpu_ctx.h"

extern "C" int oatgpu_measure_hbm(oatgpu_ctx *c, size_t bytes, int32_t reps, double *read_gbps, double *copy_gbps)
{
    if (!c || bytes < (1u << 20) || reps < 1) return fail(c, OATGPU_E_INVALID, "bad argument");
    int rc = open_sync(c);
    if (rc) return rc;
    const size_t n16 = bytes / 16;
    DevMem<void> a_own, b_own; DevMem<unsigned> sink_own; Event e0, e1;
    hipError_t e = a_own.alloc(n16 * 16);
    if (e == hipSuccess) e = b_own.alloc(n16 * 16);
    if (e == hipSuccess) e = sink_own.alloc(4);
    void *a = a_own, *b = b_own; unsigned *sink = sink_own;
    if (e == hipSuccess) e = hipMemsetAsync(a, 0x5a, n16 * 16, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(b, 0, n16 * 16, c->stream);
    if (e == hipSuccess) e = e0.create(hipEventDefault);
    if (e == hipSuccess) e = e1.create(hipEventDefault);
    double best_r = 0, best_c = 0;
    for (int i = 0; i < reps + 1 && e == hipSuccess; ++i) {          // first iteration warms up
        float ms = 0;
        hipEventRecord(e0, c->stream);
        launch_stream_read(a, n16, sink, c->stream);
        hipEventRecord(e1, c->stream);
        e = hipEventSynchronize(e1);
        if (e == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess && i && ms > 0)
            best_r = std::max(best_r, (double)(n16 * 16) / (ms * 1e-3) / 1e9);
        hipEventRecord(e0, c->stream);
        launch_stream_copy(a, b, n16, c->stream);
        hipEventRecord(e1, c->stream);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        if (e == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess && i && ms > 0)
            best_c = std::max(best_c, (double)(2 * n16 * 16) / (ms * 1e-3) / 1e9);
    }
    if (e != hipSuccess) return fail(c, OATGPU_E_HIP, "bandwidth probe failed: %s", hipGetErrorString(e));
    if (read_gbps) *read_gbps = best_r;
    if (copy_gbps) *copy_gbps = best_c;
    return OATGPU_OK;
}

extern "C" int oatgpu_traffic_audit(oatgpu_ctx *c, int32_t on)
{
    if (!c) return OATGPU_E_INVALID;
    int rc = open_sync(c);
    if (rc) return rc;
    if (on) {
        if (!c->audit_dev) HIPCHK(c, c->audit_dev.alloc(8 * sizeof(unsigned long long)));
        HIPCHK(c, hipMemsetAsync(c->audit_dev, 0, 8 * sizeof(unsigned long long), c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->audit_launches = 0;
    }
    c->audit_on = on != 0;
    return OATGPU_OK;
}
extern "C" int oatgpu_traffic_read(oatgpu_ctx *c, oatgpu_traffic *out)
{
    if (!c || !out) return OATGPU_E_INVALID;
    memset(out, 0, sizeof *out);
    if (!c->audit_dev) return OATGPU_OK;
    int rc = open_sync(c);
    if (rc) return rc;
    unsigned long long h[8];
    HIPCHK(c, hipMemcpy(h, c->audit_dev, sizeof h, hipMemcpyDeviceToHost));
    out->launches = c->audit_launches;
    out->pixels = (int64_t)h[0];
    out->lane_bytes_read = (int64_t)h[1]; out->lane_bytes_written = (int64_t)h[2];
    out->sector32_bytes_read = (int64_t)h[3]; out->sector32_bytes_written = (int64_t)h[4];
    out->sector64_bytes_read = (int64_t)h[5]; out->sector64_bytes_written = (int64_t)h[6];
    return OATGPU_OK;
}

extern "C" int oatgpu_profile_enable(oatgpu_ctx *c, int32_t on)
{
    if (!c) return OATGPU_E_INVALID;
    { const int frc = flush_pending(c); if (frc) return frc; }
    if (!on) prof_fold(c);
    if (on && !c->prof) {
        // calibrate: what an event pair measures on stream A around a launch that does nothing
        // (event processing + dispatch latency; the empty wave itself runs ~1 us)
        HIPCHK(c, hipStreamSynchronize(c->stream));
        Event e0, e1;
        HIPCHK(c, e0.create(hipEventDisableSystemFence));
        HIPCHK(c, e1.create(hipEventDisableSystemFence));
        float best = 1e30f;
        for (int i = 0; i < 16; ++i) {
            HIPCHK(c, hipEventRecord(e0, c->stream));
            launch_nop(c->stream);
            HIPCHK(c, hipEventRecord(e1, c->stream));
            HIPCHK(c, hipEventSynchronize(e1));
            float ms = 0;
            if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess && ms < best) best = ms;
        }
        c->event_pair_ms = best < 1e29f ? best : 0.0;
    }
    c->prof = on != 0;
    c->prof_every = on > 1 ? on : 1;
    c->prof_tick = 0;
    return OATGPU_OK;
}
extern "C" int oatgpu_profile_read(oatgpu_ctx *c, oatgpu_profile *out)
{
    if (!c || !out) return OATGPU_E_INVALID;
    { const int frc = flush_pending(c); if (frc) return frc; }
    prof_fold(c);
    *out = c->prof_sum;
    out->event_pair_ms = c->event_pair_ms;
    return OATGPU_OK;
}
extern "C" int oatgpu_profile_reset(oatgpu_ctx *c)
{
    if (!c) return OATGPU_E_INVALID;
    { const int frc = flush_pending(c); if (frc) return frc; }
    prof_fold(c);
    c->prof_sum = oatgpu_profile{};
    c->prof_drop_streak = 0;
    return OATGPU_OK;
}

void prof_fold(oatgpu_ctx *c)
{
    if (!c->prof_used) return;
    hipStreamSynchronize(c->stream);
    drain_b(c);
    for (size_t i = 0; i < c->prof_used; ++i) {
        float a = 0, b = 0, d = 0, t = 0;
        ProfStep &p = c->prof_steps[i];
        hipEventElapsedTime(&a, p.e[0], p.e[1]);   // fused per-pixel kernel (stream A)
        hipEventElapsedTime(&b, p.e[2], p.e[3]);   // erode (stream B)
        hipEventElapsedTime(&d, p.e[3], p.e[4]);   // dilate + labelling + sums + selection (stream B)
        hipEventElapsedTime(&t, p.e[0], p.e[4]);   // latency of the frame through both streams
        // (a host thread descheduled between the first event's record and the launch call puts its absence INTO the event
        // pair: one 10 ms sample among 145 turned a 100 us average into 238 us, profiles/r07z run of the driver's arguments.  A
        // sample eight times the average of those taken so far is the host's, not the kernel's: dropped.)
        // (the drops are COUNTED -- oatgpu_profile.dropped -- and bounded: four in a row are no host hiccup but a
        // change of regime, e.g. one-frame steps on a sparse model followed by two-frame steps on a dense one; the sample is
        // then taken and the streak starts anew, so the profile cannot freeze on its first eight samples.)
        // ... and a host stall is a millisecond or more: on a 70 x 200 frame, whose launch takes 5 us, ordinary jitter is "eight
        // times the average" (a dropped sample failed test_two_frames_a_launch_... once in this round's runs)
        const double mean_ms = c->prof_sum.steps ? c->prof_sum.mog_ms / (double)c->prof_sum.steps : 0.0;
        if (c->prof_sum.steps >= 8 && a > 8.0 * mean_ms && a > mean_ms + 1.0 && c->prof_drop_streak < 4) {
            c->prof_sum.dropped += 1;
            c->prof_drop_streak++;
            continue;
        }
        c->prof_drop_streak = 0;
        c->prof_sum.steps += 1;
        c->prof_sum.mog_frames += p.frames;
        c->prof_sum.mog_ms += a; c->prof_sum.morph_ms += b; c->prof_sum.blob_ms += d; c->prof_sum.total_ms += t;
    }
    c->prof_used = 0;
}
