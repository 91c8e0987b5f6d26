// kernels_markers.hip -- marker sets: several colour windows per camera behind ONE MOG2 pass, and `posicom mean`.
//
// Reference: one `posidet hsv` per colour (HSVDetector.cpp:142-173) behind one `framefilt mog` + `framefilt col`, and
// oat::MeanPosition::combine (src/positioncombiner/MeanPosition.cpp:60-118) behind them.
//
// The per-pixel kernel (kernels_mog.hip) is not touched.  A context whose OWN window is H [0,256], S [0,256], V [1,256]
// (GREY: intensity [1,256]) leaves, as its threshold plane, Z = "the pixel of the frame `framefilt mog` published is
// non-zero".  A foreground pixel that is pure black is a zero in that frame like any background pixel, so Z ? px : 0 IS that
// frame, byte for byte, and every marker's inRange mask is a function of (the frame K1 read, Z):
//
//     bits_m(p) = inRange_m(hsv(Z(p) ? px(p) : 0)),   hsv(0) = (0,0,0)
//
// k_marker_bits evaluates it for all markers and all streams of a step in one launch: C + 1/8 bytes read and M/8 bytes
// written per pixel, no LDS, no scratch.  The M planes go through the ordinary back half (launch_blob), one marker at a
// time; k_marker_combine then folds each stream's M centroids into the combined position and heading.
#include "oatgpu_internal.h"
#include "hsv_inline.h"
#include "posfilt_inline.h"

namespace oatgpu {

namespace {

constexpr int kWordsPerWave = 4;                      // mask words (of 64 pixels) a wave takes: their loads are in flight together
constexpr int kWavesPerGroup = 4;
static_assert(kWordsPerWave * kMaxMarkers <= kWavePx, "one lane stores one (word, marker) pair");
static_assert(1024 % (kWavePx * kWordsPerWave * kWavesPerGroup) == 0, "Palloc is a multiple of a workgroup's span: no tail");

}  // namespace

// grid (Palloc / 1024, n_streams, frames of the step), 256 threads; wave w of workgroup b takes mask words (4 b + w) * 4 .. + 3
// of stream blockIdx.y.  Lane l of word i owns pixel 64 * word + l.  planes: [M][n_streams][Palloc / 64].  blockIdx.z selects
// one of the TWO frames of a paired step, each with its own frames, Z plane and output planes (as k_undistort_frames does).
template <int CH>
__global__ __launch_bounds__(kWavePx *kWavesPerGroup) void k_marker_bits(Geom g, const uint8_t *__restrict__ frames0,
                                                                        const uint8_t *__restrict__ frames1,
                                                                        const u64 *__restrict__ zbits0, const u64 *__restrict__ zbits1,
                                                                        const RangeParams *__restrict__ win, int M,
                                                                        u64 *__restrict__ planes0, u64 *__restrict__ planes1)
{
    const bool second = blockIdx.z != 0;
    const uint8_t *__restrict__ frames = second ? frames1 : frames0;
    const u64 *__restrict__ zbits = second ? zbits1 : zbits0;
    u64 *__restrict__ planes = second ? planes1 : planes0;
    const unsigned s = blockIdx.y, n = gridDim.y;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned nwords = (unsigned)g.Palloc >> 6, pwords = (unsigned)g.P >> 6;     // P is a multiple of 64 (Wp is)
    // (uniform over the wave: scalar registers, and the Z words and windows below come in through scalar loads)
    const unsigned w0 = __builtin_amdgcn_readfirstlane((blockIdx.x * (unsigned)kWavesPerGroup + (threadIdx.x >> 6)) * (unsigned)kWordsPerWave);
    if (w0 >= nwords) return;
    const uint8_t *frame = frames + (size_t)s * (size_t)g.H * (size_t)g.W * CH;
    const u64 *zs = zbits + (size_t)s * nwords;
    const RangeParams *ws = win + (size_t)s * (unsigned)M;

    // ---- the loads of all four words first: Z (one word a wave), then the pixels of the lanes whose Z bit is set ----
    bool valid[kWordsPerWave], on[kWordsPerWave];
    int c0[kWordsPerWave], c1[kWordsPerWave], c2[kWordsPerWave];
#pragma unroll
    for (int i = 0; i < kWordsPerWave; ++i) {
        const unsigned widx = w0 + (unsigned)i;
        const bool inside = widx < pwords;
        const u64 z = inside ? zs[widx] : 0ull;
        // a word's 64 pixels lie in one row: row = widx / words by multiply-high (Geom::words_magic)
        const unsigned y = g.words == 1 ? widx : (unsigned)(((u64)widx * g.words_magic) >> 32);
        const unsigned x = (widx - y * (unsigned)g.words) * 64u + lane;
        valid[i] = inside && x < (unsigned)g.W;
        on[i] = valid[i] && ((z >> lane) & 1ull);
        c0[i] = 0; c1[i] = 0; c2[i] = 0;
        if (on[i]) {
            const unsigned fi = (y * (unsigned)g.W + x) * CH;                // frames stay below 4 GiB per stream
            c0[i] = frame[fi];
            if (CH == 3) { c1[i] = frame[fi + 1]; c2[i] = frame[fi + 2]; }
        }
    }
    // ---- BGR -> HSV once per pixel, only where Z is set: everything else is the zeroed pixel, HSV (0,0,0) ----
    if (CH == 3) {
#pragma unroll
        for (int i = 0; i < kWordsPerWave; ++i)
            if (on[i]) {
                int hh, ss, vv;
                bgr2hsv_inline(c0[i], c1[i], c2[i], hh, ss, vv);
                c0[i] = hh; c1[i] = ss; c2[i] = vv;
            }
    }
    // ---- M windows, a ballot each: lane 8 i + m keeps the word of (word i, marker m) ----
    u64 mine = 0ull;
    for (int m = 0; m < M; ++m) {
        const RangeParams rp = ws[m];
#pragma unroll
        for (int i = 0; i < kWordsPerWave; ++i) {
            const bool t = valid[i] && (CH == 3 ? in_range3(c0[i], c1[i], c2[i], rp) : (c0[i] >= rp.lo[0] && c0[i] <= rp.hi[0]));
            const u64 w = __ballot(t);
            if (lane == (unsigned)(i * kMaxMarkers + m)) mine = w;
        }
    }
    // one 64-bit store instruction a wave (nothing wider than 64 bits)
    const unsigned mi = lane & (unsigned)(kMaxMarkers - 1), wi = lane / (unsigned)kMaxMarkers;
    if (wi < (unsigned)kWordsPerWave && mi < (unsigned)M)
        planes[((size_t)mi * n + s) * nwords + w0 + wi] = mine;
}

void launch_marker_bits_frames(const Geom &g, const uint8_t *const *frames, int channels, const u64 *const *zbits,
                               const RangeParams *win, int M, u64 *const *planes, int n_streams, int nf, hipStream_t st)
{
    const int k = nf > 1 ? 1 : 0;
    const dim3 grid((unsigned)(g.Palloc / (kWavePx * kWordsPerWave * kWavesPerGroup)), (unsigned)n_streams, (unsigned)nf);
    const dim3 block(kWavePx * kWavesPerGroup);
    if (channels == 3)
        hipLaunchKernelGGL(k_marker_bits<3>, grid, block, 0, st, g, frames[0], frames[k], zbits[0], zbits[k], win, M, planes[0], planes[k]);
    else
        hipLaunchKernelGGL(k_marker_bits<1>, grid, block, 0, st, g, frames[0], frames[k], zbits[0], zbits[k], win, M, planes[0], planes[k]);
}
void launch_marker_bits(const Geom &g, const uint8_t *frames, int channels, const u64 *zbits, const RangeParams *win, int M,
                        u64 *planes, int n_streams, hipStream_t st)
{
    launch_marker_bits_frames(g, &frames, channels, &zbits, win, M, &planes, n_streams, 1, st);
}

// MeanPosition::combine (MeanPosition.cpp:60-118), one lane per camera stream, fp64, every product and sum rounded on its own
// (the library is built with -ffp-contract=off), in the reference's order.  results: [M][n_streams] records of the blob stage.
// Kept as the reference has them: an invalid marker leaves the mean a partial sum and clears position_valid; with an anchor
// the heading takes pos_m - pos_anchor only while the running position_valid is still set (and loses heading_valid
// otherwise); the sum is divided by its length even when that is 0 (one marker, coincident markers: NaN, heading_valid 1).
// Detectors never set a heading or a velocity, so without an anchor heading_valid is 0, and velocity_valid always is.
// blockIdx.y selects one of the TWO frames of a paired step.  copy (nullptr: none): where the lane also leaves its stream's M
// result records as they are -- the pipelined path's host-mapped record set, so that a frame set's marker results and its
// combined record reach the host by this kernel's stores alone.
__global__ __launch_bounds__(64) void k_marker_combine(const ResultRec *__restrict__ results0, const ResultRec *__restrict__ results1,
                                                       int M, int anchor, int n_streams, MarkerCombined *__restrict__ out0,
                                                       MarkerCombined *__restrict__ out1, ResultRec *__restrict__ copy0,
                                                       ResultRec *__restrict__ copy1)
{
    const bool second = blockIdx.y != 0;
    const ResultRec *__restrict__ results = second ? results1 : results0;
    MarkerCombined *__restrict__ out = second ? out1 : out0;
    ResultRec *__restrict__ copy = second ? copy1 : copy0;
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_streams) return;
    if (copy) {
        static_assert(sizeof(ResultRec) % 8 == 0, "a record is copied as 64-bit words");
        for (int m = 0; m < M; ++m) {
            const u64 *src = reinterpret_cast<const u64 *>(results + (size_t)m * n_streams + s);
            u64 *dst = reinterpret_cast<u64 *>(copy + (size_t)m * n_streams + s);
#pragma unroll
            for (int i = 0; i < (int)(sizeof(ResultRec) / 8); ++i)       // 64-bit stores (nothing wider)
                __hip_atomic_store(dst + i, src[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    // posidet's centroid of marker m: the host epilogue's and k_kalman's (centroid_of, posfilt_inline.h)
    auto centroid = [&](int m, double &x, double &y) { return centroid_of(results[(size_t)m * n_streams + s], x, y); };
    const double mean_denom = 1.0 / (double)M;
    double px = 0.0, py = 0.0, hx = 0.0, hy = 0.0, ax = 0.0, ay = 0.0;
    int position_valid = 1, heading_valid = 1, n_valid = 0;
    if (anchor >= 0) centroid(anchor, ax, ay);
    for (int m = 0; m < M; ++m) {
        double x, y;
        if (centroid(m, x, y)) {
            px += mean_denom * x;
            py += mean_denom * y;
            ++n_valid;
        } else {
            position_valid = 0;
        }
        if (anchor >= 0) {
            if (position_valid) {
                hx += x - ax;
                hy += y - ay;
            } else {
                heading_valid = 0;
            }
        } else {
            heading_valid = 0;
        }
    }
    if (heading_valid) {
        const double mag = sqrt(hx * hx + hy * hy);
        hx = hx / mag;
        hy = hy / mag;
    }
    // 64-bit stores, one field (or pair of flags) each (nothing wider than 64 bits)
    u64 *o = reinterpret_cast<u64 *>(out + s);
    auto put = [&](int i, u64 v) { __hip_atomic_store(o + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    put(0, (u64)(unsigned)position_valid | (u64)(unsigned)heading_valid << 32);
    put(1, (u64)(unsigned)n_valid << 32);                          // velocity_valid = 0: the filter chain writes a record of its own (k_marker_filters)
    put(2, (u64)__double_as_longlong(px));
    put(3, (u64)__double_as_longlong(py));
    put(4, (u64)__double_as_longlong(hx));
    put(5, (u64)__double_as_longlong(hy));
}

void launch_marker_combine_frames(const ResultRec *const *results, int M, int anchor, int n_streams, MarkerCombined *const *out,
                                  ResultRec *const *copy, int nf, hipStream_t st)
{
    const int k = nf > 1 ? 1 : 0;
    hipLaunchKernelGGL(k_marker_combine, dim3((n_streams + 63) / 64, nf), dim3(64), 0, st, results[0], results[k], M, anchor,
                       n_streams, out[0], out[k], copy[0], copy[k]);
}
void launch_marker_combine(const ResultRec *results, int M, int anchor, int n_streams, MarkerCombined *out, hipStream_t st)
{
    ResultRec *const none = nullptr;
    launch_marker_combine_frames(&results, M, anchor, n_streams, &out, &none, 1, st);
}

}  // namespace oatgpu
