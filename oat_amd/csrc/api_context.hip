// api_context.hip -- the C ABI of include/oatgpu.h over the gfx950 kernels: the context, its device and its streams.
#include "oatgpu_ctx.h"

thread_local std::string g_last_error;

int fail(oatgpu_ctx *c, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    if (c) c->err = buf;
    return code;
}

// wait for the B streams this context has launched on (all of them, whatever one of them answers)
hipError_t drain_b(oatgpu_ctx *c)
{
    hipError_t first = hipSuccess;
    for (int q = 0; q < oatgpu_ctx::kNB; ++q)
        if (c->stream_b[q] && c->b_used[q]) {
            const hipError_t e = hipStreamSynchronize(c->stream_b[q]);
            if (first == hipSuccess) first = e;
        }
    return first;
}

extern "C" int oatgpu_abi_version(void) { return OATGPU_ABI_VERSION; }

extern "C" int oatgpu_default_config(oatgpu_config *c)
{
    if (!c) return OATGPU_E_INVALID;
    memset(c, 0, sizeof *c);
    c->device = 0; c->n_streams = 1; c->rows = 0; c->cols = 0; c->ring_depth = 4; c->channels = 3;
    // cv::createBackgroundSubtractorMOG2() defaults (bgfg_gaussmix2.cpp)
    c->history = 500; c->nmixtures = 5; c->var_threshold = 16.f; c->background_ratio = 0.9f;
    c->var_threshold_gen = 9.f; c->var_init = 15.f; c->var_min = 4.f; c->var_max = 75.f;
    c->ct = 0.05f; c->tau = 0.5f; c->detect_shadows = 1; c->shadow_value = 127;
    // HSVDetector.h:77-94, HSVDetector.cpp:42-43
    c->h_lo = 0; c->h_hi = 256; c->s_lo = 0; c->s_hi = 256; c->v_lo = 0; c->v_hi = 256;
    c->erode = 0; c->dilate = 10; c->min_area = 0.0; c->max_area = DBL_MAX;
    c->diff_threshold = 10; c->blur = 2;       // DifferenceDetector.h:74, DifferenceDetector.cpp:41
    c->mog_restore_nmodes = 1;                 // bgfg_gaussmix2.cpp MOG2Invoker: nmodes = nNewModes
    return OATGPU_OK;
}

int check_detector(oatgpu_ctx *c, const oatgpu_marker &k, int blur)
{
    const int v[6] = { k.h_lo, k.h_hi, k.s_lo, k.s_hi, k.v_lo, k.v_hi };
    for (int i = 0; i < 6; ++i)
        if (v[i] < 0 || v[i] > 256)   // HSVDetector.cpp:87,98,109
            return fail(c, OATGPU_E_INVALID, "threshold values should be between 0 and 256");
    if (k.erode < 0 || k.dilate < 0) return fail(c, OATGPU_E_INVALID, "erode/dilate must be >= 0");
    if (k.erode > 63 || k.dilate > 63)
        return fail(c, OATGPU_E_INVALID, "erode/dilate kernel sizes above 63 are not supported");
    if (blur < 0 || blur > 22)
        return fail(c, OATGPU_E_INVALID, "blur must be in 0..22 (above that a box blur is no longer a dilation)");
    if (!(k.min_area < k.max_area))   // HSVDetector.cpp:135
        return fail(c, OATGPU_E_INVALID, "Max area should be larger than min area.");
    return OATGPU_OK;
}

// The HIP streams are shared by all contexts of a device in this process, and they are created
// together, in a fixed order.  Measured on MI355X / ROCm 7.2: the runtime
// spreads the streams of a process over FOUR hardware queues in the order they are created (the
// null stream counts from its first use; priorities and GPU_MAX_HW_QUEUES make no difference), and
// two streams on one hardware queue execute strictly one after the other.  A fifth stream therefore
// lands on the first one's queue: with private streams the second context's B0 shared a queue with
// the first context's A, and every K1 waited for the other context's back halves (18.9k fps for two
// contexts, against 38.3k for one context holding both cameras).  So: A, B0, B1, B2 are created
// back to back (any four consecutive streams sit on four different queues) and shared by all
// contexts; the host-frame copy stream is created right behind them (the host-frame path leaves B2
// unused, which keeps it at four active streams).
namespace {
struct DeviceStreams {
    int refs = 0;
    hipStream_t a = nullptr, b[oatgpu_ctx::kNB] = {}, copy = nullptr, copy2 = nullptr;
};
std::mutex g_streams_mutex;
std::map<int, DeviceStreams> g_streams;      // by device ordinal

hipStream_t create_b_stream()
{
    // the B streams carry short latency-bound kernels that must slip in between the big
    // bandwidth-bound launches of stream A: highest priority
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { least = greatest = 0; }
    hipStream_t st = nullptr;
    if (hipStreamCreateWithPriority(&st, hipStreamNonBlocking, greatest) != hipSuccess) st = nullptr;
    return st;
}

bool acquire_streams(int device, hipStream_t *a, hipStream_t *b)
{
    std::lock_guard<std::mutex> lk(g_streams_mutex);
    DeviceStreams &d = g_streams[device];
    if (!d.a) {
        // (measurement builds: OATGPU_A_RESERVE=n keeps stream A -- the per-pixel kernel -- off the last n compute units)
        int reserve = 0;
        if (const char *e = measure_env("OATGPU_A_RESERVE")) reserve = atoi(e);
        if (reserve > 0) {
            hipDeviceProp_t prop;
            if (hipGetDeviceProperties(&prop, device) != hipSuccess) return false;
            const int ncu = prop.multiProcessorCount;
            std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, 0u);
            for (int i = 0; i < ncu - reserve; ++i) mask[(size_t)i >> 5] |= 1u << (i & 31);
            if (hipExtStreamCreateWithCUMask(&d.a, (uint32_t)mask.size(), mask.data()) != hipSuccess) { d.a = nullptr; return false; }
        } else
        if (hipStreamCreateWithFlags(&d.a, hipStreamNonBlocking) != hipSuccess) { d.a = nullptr; return false; }
        for (int q = 0; q < oatgpu_ctx::kNB; ++q)                // A + 3 B streams = the four queues
            if (!(d.b[q] = create_b_stream())) return false;
        // ... and, in the same breath, the host-frame copy stream.  Where it lands relative to A
        // decides who yields while host frames are copied: right behind the B streams (no padding)
        // the copies win and K1 waits for them, which is the better trade on a PCIe-bound path
        // (7.8k fps at 1080p with K1 stretched to 62 us, against 5.6-7.0k fps with K1 at 26 us when
        // 1..3 idle streams were put in front of it).
        if (hipStreamCreateWithFlags(&d.copy, hipStreamNonBlocking) != hipSuccess) d.copy = nullptr;
    }
    d.refs++;
    *a = d.a;
    for (int q = 0; q < oatgpu_ctx::kNB; ++q) b[q] = d.b[q];
    return true;
}

}  // namespace
// A second copy stream (created on first use: the camera-by-camera path alternates between the two, so that one copy's
// set-up and completion signalling hide behind the other's transfer)
hipStream_t acquire_copy_stream2(int device)
{
    std::lock_guard<std::mutex> lk(g_streams_mutex);
    DeviceStreams &d = g_streams[device];
    if (!d.copy2 && hipStreamCreateWithFlags(&d.copy2, hipStreamNonBlocking) != hipSuccess) d.copy2 = nullptr;
    return d.copy2;
}
hipStream_t acquire_copy_stream(int device)
{
    std::lock_guard<std::mutex> lk(g_streams_mutex);
    return g_streams[device].copy;
}
void release_streams(int device)
{
    // The device's streams are NOT destroyed with the last context: the runtime places streams on its four hardware
    // queues in creation order, so a later context that had to create its streams afresh may find A and a B stream
    // on one queue (bench.py's fourth leg in a row ran 1080p at 15.8 k instead of 27.9 k fps).  They live as long as
    // the process; the runtime reclaims them at exit.
    std::lock_guard<std::mutex> lk(g_streams_mutex);
    auto it = g_streams.find(device);
    if (it != g_streams.end() && it->second.refs > 0) --it->second.refs;
}

// Opening the device.  Several processes that open one freshly booted device in the same instant (the ranks of a job, the
// components of a pipeline started by one script) can see the first runtime calls fail transiently -- no device yet, the
// device busy being initialised by a sibling.  Bounded retry with back-off (50 ms doubling, ~1.5 s in all); an ordinal that
// does not exist is not transient.  Retries are counted (oatgpu_device_open_retries) so that a caller can report them
// instead of hiding them.
static std::atomic<int> g_open_retries{0};
static hipError_t open_device(int device, int *ndev)
{
    hipError_t e = hipSuccess;
    for (int attempt = 0; attempt < 6; ++attempt) {
        *ndev = 0;
        e = hipGetDeviceCount(ndev);
        if (e == hipSuccess && *ndev > 0) {
            if (device < 0 || device >= *ndev) return hipErrorInvalidDevice;
            e = hipSetDevice(device);
            if (e == hipSuccess) e = hipFree(nullptr);             // forces the context into being here, not in the first hipMalloc
            if (e == hipSuccess) return hipSuccess;
        } else if (e == hipSuccess) {
            e = hipErrorNoDevice;
        }
        (void)hipGetLastError();
        // (a box WITHOUT a device says so at the first call -- hipErrorNoDevice, or a count of 0 -- and is not kept
        // waiting 1.5 s for one on every oatgpu_create; what the retry absorbs is a device that exists and is busy being
        // initialised by a sibling process: any other error, or "no device" after a first attempt that saw one)
        if (attempt == 0 && e == hipErrorNoDevice) break;
        if (attempt == 5) break;
        g_open_retries++;
        usleep(50000u << attempt);
    }
    return e;
}
extern "C" int oatgpu_device_open_retries(void) { return g_open_retries.load(); }

// a table of `count` events: made aside, put in place only when every one of them exists
hipError_t make_events(std::vector<Event> &table, size_t count, unsigned flags)
{
    std::vector<Event> made(count);
    for (auto &e : made) { const hipError_t r = e.create(flags); if (r != hipSuccess) return r; }
    table = std::move(made);
    return hipSuccess;
}

template <class T> static bool dev_malloc(T *&p, size_t bytes) { return hipMalloc((void **)&p, bytes) == hipSuccess; }
// One scratch set of the back half (BlobBuffers; about 30 bytes a pixel and stream), its counters zeroed.  ALL sets a context
// can come to use are made with it (oatgpu_create): the three of the plain order, the fourth of the early and
// the paired layout, and the repair set -- 150 bytes a pixel and stream in all.  An allocation in the middle of a pipelined
// step would stall a camera-paced caller for as long as hipMalloc takes, and its failure would come after the model had
// moved.
bool Scratch::alloc(const oatgpu_ctx *c, size_t planes)
{
    const Geom &g = c->g;
    const size_t n = planes ? planes : (size_t)c->cfg.n_streams, PA = g.Palloc, NW = PA / 64;
    reset();
    b.thr = c->thr;
    b.nopark = c->nopark;
    bool ok = dev_malloc(b.tmp, n * NW * 8);
    ok = ok && dev_malloc(b.morph, n * NW * 8);
    ok = ok && dev_malloc(b.fin, n * NW * 8);
    ok = ok && dev_malloc(b.trans, n * NW * 8);
    ok = ok && dev_malloc(b.carry, n * (size_t)g.H * g.words * sizeof(int));
    ok = ok && dev_malloc(b.parent, n * PA * sizeof(int));
    ok = ok && dev_malloc(b.acc, n * PA * 3 * sizeof(long long));
    ok = ok && dev_malloc(b.done, n * sizeof(unsigned));
    ok = ok && dev_malloc(b.roots, n * (PA / 2) * sizeof(int));
    ok = ok && dev_malloc(b.nroots, n * sizeof(unsigned));
    ok = ok && dev_malloc(b.wpre, n * (size_t)g.H * g.words * sizeof(unsigned short));
    ok = ok && dev_malloc(b.rowinfo, n * (size_t)g.H * sizeof(int));
    ok = ok && dev_malloc(b.lds_ok, n * sizeof(unsigned));
    ok = ok && dev_malloc(b.ready, n * sizeof(unsigned));
    for (unsigned *p : {b.done, b.nroots, b.lds_ok, b.ready})
        ok = ok && hipMemsetAsync(p, 0, n * sizeof(unsigned), c->stream) == hipSuccess;
    return ok;
}

extern "C" oatgpu_ctx *oatgpu_create(const oatgpu_config *cfg)
{
    if (!cfg) { fail(nullptr, OATGPU_E_INVALID, "null config"); return nullptr; }
    if (cfg->rows < 1 || cfg->cols < 1 || cfg->n_streams < 1 || cfg->ring_depth < 1) {
        fail(nullptr, OATGPU_E_INVALID, "rows, cols, n_streams and ring_depth must be >= 1");
        return nullptr;
    }
    if (cfg->channels != 1 && cfg->channels != 3) {
        fail(nullptr, OATGPU_E_INVALID, "channels must be 3 (BGR) or 1 (GREY)");
        return nullptr;
    }
    if (cfg->nmixtures < 1 || cfg->nmixtures > kMaxMix) {
        fail(nullptr, OATGPU_E_INVALID, "nmixtures must be in 1..5");
        return nullptr;
    }
    if (!(cfg->ct >= 0.f && cfg->ct < 0.5f)) {      // a matched mode must never be prunable (kernels_mog.hip mog2_mode)
        fail(nullptr, OATGPU_E_INVALID, "ct (complexity reduction) must be in [0, 0.5)");
        return nullptr;
    }
    if ((long long)cfg->rows * (((long long)cfg->cols + 63) / 64 * 64) > 0x7fff0000ll) {
        fail(nullptr, OATGPU_E_INVALID, "frame too large");
        return nullptr;
    }
    if (check_detector(nullptr, detector_of(*cfg), cfg->blur) != OATGPU_OK) return nullptr;

    int ndev = 0;
    const hipError_t oe = open_device(cfg->device, &ndev);
    if (oe == hipErrorInvalidDevice && ndev > 0) {
        fail(nullptr, OATGPU_E_INVALID, "device %d out of range (have %d)", cfg->device, ndev);
        return nullptr;
    }
    if (oe != hipSuccess) {
        if (ndev < 1) fail(nullptr, OATGPU_E_NODEVICE, "no HIP device available");
        else fail(nullptr, OATGPU_E_HIP, "hipSetDevice(%d) failed: %s", cfg->device, hipGetErrorString(oe));
        return nullptr;
    }

    oatgpu_ctx *c = new oatgpu_ctx();
    c->cfg = *cfg;
    Geom &g = c->g;
    g.H = cfg->rows; g.W = cfg->cols; g.Wp = (cfg->cols + 63) / 64 * 64; g.words = g.Wp / 64;
    g.P = g.H * g.Wp; g.Palloc = (g.P + 1023) / 1024 * 1024; g.n_streams = cfg->n_streams;
    g.words_magic = (unsigned)((0x100000000ull + (unsigned)g.words - 1) / (unsigned)g.words);
    // (i * magic) >> 32 == i / words needs i * (magic * words - 2^32) < 2^32; the error term is < words
    if ((unsigned long long)(g.Palloc / 64) * (unsigned long long)g.words >= 0x100000000ull ||
        (unsigned long long)mog_stream_floats(g.Palloc) * 4ull >= 0x100000000ull) {     // 32-bit plane offsets in K1
        fail(nullptr, OATGPU_E_INVALID, "frame too large");
        delete c;
        return nullptr;
    }
    const size_t n = cfg->n_streams, npx = (size_t)g.H * g.W, PA = g.Palloc, NW = PA / 64;
    c->nframes.assign(n, 0);
    c->wild_model.assign(n, 0);
    c->diff_have.assign(n, 0);
    c->bsub_have.assign(n, 0);
    c->ud_have.assign(n, 0);

    bool ok = acquire_streams(cfg->device, &c->stream, c->stream_b);
    if (ok) c->lease.device = cfg->device;
    c->ring_slots = cfg->ring_depth;                  // slot = threshold buffer; on the plain path slot % 3 = scratch set / stream
    for (auto &e : c->ev_k1) ok = ok && e.create(hipEventDisableTiming | hipEventDisableSystemFence) == hipSuccess;
    for (auto &e : c->ev_blob) ok = ok && e.create(hipEventDisableTiming | hipEventDisableSystemFence) == hipSuccess;
    if (const char *e = measure_env("OATGPU_EARLY_BLOB")) c->early_blob = atoi(e);
    if (const char *e = measure_env("OATGPU_EARLY_MIN_PX")) c->early_min_px = (size_t)atoll(e);
    if (const char *e = measure_env("OATGPU_LONE_PLAIN")) c->lone_plain = atoi(e) != 0;
    if (const char *e = measure_env("OATGPU_PAIR_BACK")) c->pair_back = atoi(e) != 0;
    if (const char *e = measure_env("OATGPU_RS_DEEP_ROWS")) { const int v = atoi(e); if (v == kRsRowsDeep || v == kRsRowsDeepAlt) c->rs_rows_deep = v; }
    if (const char *e = measure_env("OATGPU_K1_WG")) { const int v = atoi(e); if (v == 64 || v == 256) c->k1_wg_force = v; }

    if (const char *e = measure_env("OATGPU_K1_STOP_EVENT")) c->k1_stop_event = atoi(e) != 0 ? 1 : 0;

    ok = ok && c->state.alloc(n * mog_stream_floats(g.Palloc) * sizeof(float)) == hipSuccess;
    ok = ok && c->nmodes.alloc(n * PA) == hipSuccess;
    ok = ok && c->frames.alloc(n * npx * cfg->channels) == hipSuccess;
    ok = ok && c->aux_a.alloc(npx * 3) == hipSuccess;
    ok = ok && c->aux_b.alloc(npx * 3) == hipSuccess;
    // One threshold-bit buffer per ring slot: a slot is only reused after its result was collected,
    // i.e. after the back half that read its buffer has finished -- stream A never waits for a B stream.
    ok = ok && c->thr.alloc((size_t)c->ring_slots * n * NW * 8) == hipSuccess;
    ok = ok && c->nopark.alloc(sizeof(unsigned)) == hipSuccess;
    ok = ok && hipMemsetAsync(c->nopark, 0, sizeof(unsigned), c->stream) == hipSuccess;
    for (int q = 0; q < oatgpu_ctx::kSets && ok; ++q) ok = c->bb[q].alloc(c);   // (an out-of-memory shows HERE, as OATGPU_E_NOMEM from oatgpu_create)
    const size_t slots = (size_t)c->ring_slots + 1;
    ok = ok && c->res.alloc(slots * n * sizeof(ResultRec), hipHostMallocMapped) == hipSuccess;
    ok = ok && c->dens.alloc(4 * sizeof(unsigned), hipHostMallocMapped) == hipSuccess;
    if (ok) memset(c->dens.host(), 0, 4 * sizeof(unsigned));
    ok = ok && c->wild_sink.alloc(8 * sizeof(unsigned long long)) == hipSuccess;
    ok = ok && hipMemset(c->wild_sink, 0, 8 * sizeof(unsigned long long)) == hipSuccess;
    if (ok) {
        c->slots.assign(c->ring_slots, oatgpu_ctx::Slot{});
        for (int i = 0; i < c->ring_slots; ++i) c->slots[i].ev = i;
        ok = make_events(c->ring_ev, (size_t)c->ring_slots, hipEventDisableTiming) == hipSuccess;
    }
    // the model's mode counters start at zero; everything else is written before it is read
    ok = ok && hipMemsetAsync(c->nmodes, 0, n * PA, c->stream) == hipSuccess;
    ok = ok && hipMemsetAsync(c->state, 0, n * mog_stream_floats(g.Palloc) * sizeof(float), c->stream) == hipSuccess;
    ok = ok && hipMemsetAsync(c->thr, 0, (size_t)c->ring_slots * n * NW * 8, c->stream) == hipSuccess;
    ok = ok && hipStreamSynchronize(c->stream) == hipSuccess;
    if (!ok) {
        fail(nullptr, OATGPU_E_NOMEM, "device allocation failed: %s", hipGetErrorString(hipGetLastError()));
        delete c;
        return nullptr;
    }
    c->last_morph = c->thr;
    c->last_fin = c->bb[0].b.fin;
    return c;
}

extern "C" void oatgpu_destroy(oatgpu_ctx *c)
{
    if (!c) return;
    hipSetDevice(c->cfg.device);
    c->pend_valid = false;            // a registered frame nobody collected: nothing to launch for
    if (c->stream) hipStreamSynchronize(c->stream);
    drain_b(c);
    delete c;           // every member releases what it holds; the stream lease, declared first, goes last
}

extern "C" const char *oatgpu_last_error(const oatgpu_ctx *c)
{
    return c ? c->err.c_str() : g_last_error.c_str();
}

extern "C" int oatgpu_device_count(void)
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

extern "C" int oatgpu_device_numa_node(int32_t device)
{
    char bus[32] = {0};
    if (device < 0 || device >= oatgpu_device_count()) return -1;             // (never hand HIP a bad ordinal: its error is sticky)
    if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, device) != hipSuccess) { (void)hipGetLastError(); return -1; }
    for (char *p = bus; *p; ++p) if (*p >= 'A' && *p <= 'F') *p = (char)(*p - 'A' + 'a');      // sysfs spells it in lower case
    char path[96];
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
    FILE *f = fopen(path, "r");
    if (!f) return -1;
    int node = -1;
    if (fscanf(f, "%d", &node) != 1) node = -1;
    fclose(f);
    return node;
}

extern "C" int oatgpu_host_register(void *ptr, size_t bytes)
{
    if (!ptr || !bytes) return fail(nullptr, OATGPU_E_INVALID, "null argument");
    hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterDefault);
    if (e != hipSuccess) return fail(nullptr, OATGPU_E_HIP, "hipHostRegister failed: %s", hipGetErrorString(e));
    return OATGPU_OK;
}
extern "C" int oatgpu_host_unregister(void *ptr)
{
    if (!ptr) return OATGPU_E_INVALID;
    return hipHostUnregister(ptr) == hipSuccess ? OATGPU_OK : OATGPU_E_HIP;
}
extern "C" void *oatgpu_host_alloc(size_t bytes)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
extern "C" void oatgpu_host_free(void *ptr) { if (ptr) hipHostFree(ptr); }

extern "C" int oatgpu_set_stream(oatgpu_ctx *c, void *s)
{
    if (!c) return OATGPU_E_INVALID;
    { const int frc = flush_pending(c); if (frc) return frc; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, drain_b(c));
    c->stream = (hipStream_t)s;
    return OATGPU_OK;
}
extern "C" void *oatgpu_get_stream(oatgpu_ctx *c) { return c ? (void *)c->stream : nullptr; }
extern "C" int oatgpu_synchronize(oatgpu_ctx *c)
{
    if (!c) return OATGPU_E_INVALID;
    return quiesce(c);
}
extern "C" int oatgpu_set_stage_copy(oatgpu_ctx *c, int32_t mode)
{
    if (!c || (mode != 0 && mode != 1)) return fail(c, OATGPU_E_INVALID, "stage copy mode must be 0 (DMA) or 1 (kernel)");
    c->stage_kernel = mode == 1;
    return OATGPU_OK;
}

extern "C" int oatgpu_set_early_blob(oatgpu_ctx *c, int32_t on)
{
    if (!c) return OATGPU_E_INVALID;
    c->early_blob = on < 0 ? -1 : on != 0;
    return OATGPU_OK;
}

#ifdef OATGPU_MEASURE
// measurement builds only (tools/dense_placement_probe.py): where the context's model, counters and frames landed
extern "C" __attribute__((visibility("default"))) int oatgpu_debug_addresses(oatgpu_ctx *c, unsigned long long *out4)
{
    if (!c || !out4) return OATGPU_E_INVALID;
    out4[0] = (unsigned long long)(uintptr_t)c->state.get(); out4[1] = (unsigned long long)(uintptr_t)c->nmodes.get();
    out4[2] = (unsigned long long)(uintptr_t)c->thr.get(); out4[3] = (unsigned long long)(mog_stream_floats(c->g.Palloc) * 4);
    return OATGPU_OK;
}
#endif

extern "C" int oatgpu_set_k1_workgroup(oatgpu_ctx *c, int32_t threads)
{
    if (!c || (threads != 0 && threads != 64 && threads != 256)) return fail(c, OATGPU_E_INVALID, "k1 workgroup must be 0 (by path), 64 or 256");
    c->k1_wg_force = threads;
    return OATGPU_OK;
}

extern "C" int oatgpu_last_step_shape(const oatgpu_ctx *c, int32_t *k1_workgroup, int32_t *early_blob)
{
    if (!c) return OATGPU_E_INVALID;
    if (k1_workgroup) *k1_workgroup = c->last_k1_wg;
    if (early_blob) *early_blob = c->last_step_early ? 1 : 0;
    return OATGPU_OK;
}

extern "C" int oatgpu_set_rowscan_rows(oatgpu_ctx *c, int32_t rows)
{
    if (!c || (rows != 0 && rows != kRsRowsNarrow && rows != c->rs_rows_deep))
        return fail(c, OATGPU_E_INVALID, "row-scan rows must be 0 (by pipeline depth), %d or %d", kRsRowsNarrow, c ? c->rs_rows_deep : kRsRowsDeep);
    c->rs_rows_force = rows;
    return OATGPU_OK;
}

extern "C" int oatgpu_last_step_rowscan_rows(const oatgpu_ctx *c) { return c ? c->last_rs_rows : 0; }

extern "C" int64_t oatgpu_early_blob_timeouts(const oatgpu_ctx *c) { return c ? (int64_t)c->early_timeouts : 0; }

extern "C" int oatgpu_set_fusion(oatgpu_ctx *c, int32_t frames_per_launch)
{
    if (!c) return OATGPU_E_INVALID;
    if (frames_per_launch != 1 && frames_per_launch != 2) return fail(c, OATGPU_E_INVALID, "frames_per_launch must be 1 or 2");
    const int rc = quiesce(c);
    if (rc) return rc;
    c->fuse = frames_per_launch;
    return OATGPU_OK;
}

extern "C" int oatgpu_set_detector(oatgpu_ctx *c, int32_t h_lo, int32_t h_hi, int32_t s_lo, int32_t s_hi,
                                   int32_t v_lo, int32_t v_hi, int32_t erode, int32_t dilate,
                                   double min_area, double max_area)
{
    if (!c) return OATGPU_E_INVALID;
    oatgpu_config k = c->cfg;
    k.h_lo = h_lo; k.h_hi = h_hi; k.s_lo = s_lo; k.s_hi = s_hi; k.v_lo = v_lo; k.v_hi = v_hi;
    k.erode = erode; k.dilate = dilate; k.min_area = min_area; k.max_area = max_area;
    int rc = check_detector(c, detector_of(k), k.blur);
    if (rc) return rc;
    if (c->mkp.on && !own_window_is_nonzero(k))
        return fail(c, OATGPU_E_INVALID, "the marker pipeline is on and needs the non-zero window: oatgpu_set_marker_pipeline(0) first");
    rc = quiesce(c);
    if (rc) return rc;
    c->cfg = k;
    return OATGPU_OK;
}

// The single-stage calls are synchronous and share scratch with the pipelined path:
// wait until both HIP streams have drained.
int quiesce(oatgpu_ctx *c)
{
    if (c->defer_kind) return fail(c, OATGPU_E_INVALID, "a deferred result is waiting: fetch it first (oatgpu_fetch_frame / oatgpu_fetch_position)");
    const int frc = flush_pending(c);
    if (frc) return frc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, drain_b(c));
    // Outstanding frames whose speculative back half declined them are redone NOW, while their threshold bits are still
    // in their ring slots: the single-stage calls that follow a quiesce() write theirs into slot 0's buffer.
    return repair_outstanding(c);
}

// ... which is how every synchronous call opens, once its own arguments are in order
int open_sync(oatgpu_ctx *c)
{
    HIPCHK(c, hipSetDevice(c->cfg.device));
    return quiesce(c);
}

int check_stream_ix(oatgpu_ctx *c, int s)
{
    if (!c) return OATGPU_E_INVALID;
    if (s < 0 || s >= c->cfg.n_streams) return fail(c, OATGPU_E_INVALID, "stream index %d out of range", s);
    return OATGPU_OK;
}

extern "C" int oatgpu_set_deferred(oatgpu_ctx *c, int32_t on)
{
    if (!c) return OATGPU_E_INVALID;
    if (c->defer_kind) return fail(c, OATGPU_E_INVALID, "a deferred result is waiting: fetch it first");
    if (on && c->tg.k) return fail(c, OATGPU_E_INVALID, "set_deferred with targets on (oatgpu_set_targets) is not supported");
    c->deferred = on != 0;
    return OATGPU_OK;
}
