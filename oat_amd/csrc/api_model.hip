// api_model.hip -- the MOG2 model of a camera stream, out and in: export, import, checkpoint.
#include "oatgpu_ctx.h"

namespace {
struct ModelBufs {          // one stream's model in the logical layout of oatgpu_mog_get_state: modes used, weights, variances, means
    DevMem<uint8_t> mu; DevMem<float> w, v, m;
    hipError_t alloc(size_t npx, size_t k, size_t mean_bytes)
    {
        hipError_t e = mu.alloc(npx);
        if (e == hipSuccess) e = w.alloc(npx * k * 4);
        if (e == hipSuccess) e = v.alloc(npx * k * 4);
        if (e == hipSuccess) e = m.alloc(npx * k * mean_bytes);
        return e;
    }
};
}  // namespace

extern "C" int oatgpu_mog_get_state(oatgpu_ctx *c, int32_t s, uint8_t *modes_used, float *weight, float *variance,
                                    float *mean, int32_t *nframes)
{
    int rc = check_stream_ix(c, s);
    if (rc) return rc;
    rc = open_sync(c);
    if (rc) return rc;
    const Geom &g = c->g;
    const size_t npx = (size_t)g.H * g.W, k = c->cfg.nmixtures, mb = 4 * (size_t)c->cfg.channels;
    ModelBufs b;                         // freed on every return path
    HIPCHK(c, b.alloc(npx, k, mb));
    uint8_t *d_mu = b.mu; float *d_w = b.w, *d_v = b.v, *d_m = b.m;
    launch_state_export(g, c->state + (size_t)s * mog_stream_floats(g.Palloc), c->nmodes + (size_t)s * g.Palloc, (int)k,
                        c->cfg.channels, d_mu, d_w, d_v, d_m, c->stream);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && modes_used) e = hipMemcpyAsync(modes_used, d_mu, npx, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && weight) e = hipMemcpyAsync(weight, d_w, npx * k * 4, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && variance) e = hipMemcpyAsync(variance, d_v, npx * k * 4, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && mean) e = hipMemcpyAsync(mean, d_m, npx * k * mb, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, OATGPU_E_HIP, "state export failed: %s", hipGetErrorString(e));
    if (nframes) *nframes = c->nframes[s];
    return OATGPU_OK;
}

extern "C" int oatgpu_mog_set_state(oatgpu_ctx *c, int32_t s, const uint8_t *modes_used, const float *weight,
                                    const float *variance, const float *mean, int32_t nframes)
{
    int rc = check_stream_ix(c, s);
    if (rc) return rc;
    if (!modes_used || !weight || !variance || !mean || nframes < 0)
        return fail(c, OATGPU_E_INVALID, "null argument");
    rc = open_sync(c);
    if (rc) return rc;
    const Geom &g = c->g;
    const size_t npx = (size_t)g.H * g.W, k = c->cfg.nmixtures, mb = 4 * (size_t)c->cfg.channels;
    ModelBufs b;                         // freed on every return path
    HIPCHK(c, b.alloc(npx, k, mb));
    uint8_t *d_mu = b.mu; float *d_w = b.w, *d_v = b.v, *d_m = b.m;
    hipError_t e = hipMemcpyAsync(d_mu, modes_used, npx, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_w, weight, npx * k * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_v, variance, npx * k * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_m, mean, npx * k * mb, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        launch_state_import(g, c->state + (size_t)s * mog_stream_floats(g.Palloc), c->nmodes + (size_t)s * g.Palloc, (int)k,
                            c->cfg.channels, d_mu, d_w, d_v, d_m, c->stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, OATGPU_E_HIP, "state import failed: %s", hipGetErrorString(e));
    c->nframes[s] = nframes;
    // The product kernels rely on what a run of the kernel leaves in a model (kernels_mog.hip): a weight that is 0 or in
    // [2^-62, 4] (div_inrange), means that are finite, below 2^20 and not -0.f and variances inside [var_min, var_max] (at
    // rate 0 the update of a fitted mode is then the identity and is not computed).  A model holding anything else
    // (hand-made, NaN, a weight of 1e-30, a variance outside the clamp) is taken as it is and advanced by the
    // instantiations that keep the compiler's division and compute every update.
    bool wild = false;
    const size_t chn = (size_t)c->cfg.channels;
    for (size_t p = 0; p < npx && !wild; ++p) {
        const size_t used = modes_used[p] < k ? modes_used[p] : k;
        for (size_t m = 0; m < used && !wild; ++m) {
            const float w = weight[p * k + m], v = variance[p * k + m];
            if (!(w == 0.f || (w >= 0x1p-62f && w <= 4.f))) wild = true;
            if (!(v >= c->cfg.var_min && v <= c->cfg.var_max)) wild = true;
            for (size_t ch = 0; ch < chn; ++ch) {
                const float mu = mean[(p * k + m) * chn + ch];
                uint32_t bits;
                memcpy(&bits, &mu, sizeof bits);
                if (!(mu > -0x1p20f && mu < 0x1p20f) || bits == 0x80000000u) wild = true;
            }
        }
    }
    c->wild_model[(size_t)s] = wild ? 1 : 0;
    return OATGPU_OK;
}

// ------------------------------------------------------- model checkpoint ----
// File: 64-byte header, then modes_used u8[npx], weight f32[npx*k], variance f32[npx*k],
// mean f32[npx*k*channels] in the logical layout of oatgpu_mog_get_state; entries of unused modes
// are written as zeros so that equal models give equal files.
namespace {
struct CkptHeader {
    char magic[8];          // "OATMOG2\0"
    uint32_t version;       // 1
    uint32_t rows, cols, channels, nmixtures;
    int32_t nframes;
    uint64_t payload_bytes;
    uint8_t reserved[24];
};
static_assert(sizeof(CkptHeader) == 64, "checkpoint header layout");
const char kCkptMagic[8] = {'O', 'A', 'T', 'M', 'O', 'G', '2', 0};
}  // namespace

extern "C" int oatgpu_mog_save(oatgpu_ctx *c, int32_t s, const char *path)
{
    int rc = check_stream_ix(c, s);
    if (rc) return rc;
    if (!path || !*path) return fail(c, OATGPU_E_INVALID, "null path");
    const size_t npx = (size_t)c->g.H * c->g.W, k = c->cfg.nmixtures, ch = c->cfg.channels;
    std::vector<uint8_t> mu(npx);
    std::vector<float> w(npx * k), v(npx * k), m(npx * k * ch);
    int32_t nf = 0;
    rc = oatgpu_mog_get_state(c, s, mu.data(), w.data(), v.data(), m.data(), &nf);
    if (rc) return rc;
    for (size_t p = 0; p < npx; ++p)
        for (size_t j = mu[p]; j < k; ++j) {
            w[p * k + j] = 0.f; v[p * k + j] = 0.f;
            for (size_t q = 0; q < ch; ++q) m[(p * k + j) * ch + q] = 0.f;
        }
    CkptHeader h{};
    memcpy(h.magic, kCkptMagic, 8);
    h.version = 1; h.rows = c->g.H; h.cols = c->g.W; h.channels = (uint32_t)ch; h.nmixtures = (uint32_t)k;
    h.nframes = nf;
    h.payload_bytes = npx + (w.size() + v.size() + m.size()) * sizeof(float);
    const std::string tmp = std::string(path) + ".tmp";
    FILE *f = fopen(tmp.c_str(), "wb");
    if (!f) return fail(c, OATGPU_E_INVALID, "cannot open '%s' for writing", tmp.c_str());
    bool ok = fwrite(&h, sizeof h, 1, f) == 1 && fwrite(mu.data(), 1, npx, f) == npx &&
              fwrite(w.data(), 4, w.size(), f) == w.size() && fwrite(v.data(), 4, v.size(), f) == v.size() &&
              fwrite(m.data(), 4, m.size(), f) == m.size();
    ok = (fclose(f) == 0) && ok;
    if (ok) ok = rename(tmp.c_str(), path) == 0;      // readers never see a half-written file
    if (!ok) { remove(tmp.c_str()); return fail(c, OATGPU_E_INVALID, "writing '%s' failed", path); }
    return OATGPU_OK;
}

extern "C" int oatgpu_mog_load(oatgpu_ctx *c, int32_t s, const char *path)
{
    int rc = check_stream_ix(c, s);
    if (rc) return rc;
    if (!path || !*path) return fail(c, OATGPU_E_INVALID, "null path");
    FILE *f = fopen(path, "rb");
    if (!f) return fail(c, OATGPU_E_INVALID, "cannot open '%s'", path);
    CkptHeader h{};
    const size_t npx = (size_t)c->g.H * c->g.W, k = c->cfg.nmixtures, ch = c->cfg.channels;
    if (fread(&h, sizeof h, 1, f) != 1 || memcmp(h.magic, kCkptMagic, 8) != 0 || h.version != 1) {
        fclose(f);
        return fail(c, OATGPU_E_INVALID, "'%s' is not a MOG2 model checkpoint", path);
    }
    if (h.rows != (uint32_t)c->g.H || h.cols != (uint32_t)c->g.W || h.channels != ch || h.nmixtures != k ||
        h.nframes < 0 || h.payload_bytes != npx + (2 * npx * k + npx * k * ch) * sizeof(float)) {
        fclose(f);
        return fail(c, OATGPU_E_INVALID, "checkpoint '%s' is %ux%ux%u with %u mixtures; this context is %dx%dx%d with %d",
                    path, h.rows, h.cols, h.channels, h.nmixtures, c->g.H, c->g.W, (int)ch, (int)k);
    }
    std::vector<uint8_t> mu(npx);
    std::vector<float> w(npx * k), v(npx * k), m(npx * k * ch);
    const bool ok = fread(mu.data(), 1, npx, f) == npx && fread(w.data(), 4, w.size(), f) == w.size() &&
                    fread(v.data(), 4, v.size(), f) == v.size() && fread(m.data(), 4, m.size(), f) == m.size();
    fclose(f);
    if (!ok) return fail(c, OATGPU_E_INVALID, "checkpoint '%s' is truncated", path);
    for (size_t p = 0; p < npx; ++p)
        if (mu[p] > k) return fail(c, OATGPU_E_INVALID, "checkpoint '%s' is corrupt (mode count %u)", path, mu[p]);
    return oatgpu_mog_set_state(c, s, mu.data(), w.data(), v.data(), m.data(), h.nframes);
}
