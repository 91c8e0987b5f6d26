// kernels_bsubtrack.hip -- the front end of the subtraction tracker (`framefilt bsub` -> `framefilt col -C HSV` -> `posidet hsv`
// for BGR frames, `framefilt bsub` -> `posidet thresh` for GREY ones) for every camera stream of a context in one
// launch (grid y = stream).
//
// Per pixel and channel bsub_elem, k_bsub's rule (BackgroundSubtractor.cpp:79-100): x = the frame byte, 0 where the stream's ROI bit is
// 0 (framefilt mask in front of bsub); on a stream's first frame acc = (float)x, bg = x; with LEARN acc = x * a + acc * b in
// separate roundings (cv::accumulateWeighted, the unit is built with -ffp-contract=off) and bg = saturate(round-half-even(acc));
// d = x > bg ? x - bg : 0.  Then bit = inRange(hsv(d_b, d_g, d_r)) (hsv_inline.h) or lo <= d <= hi (GREY).
//   LEARN false: acc is neither read nor written and bg only read -- except on a first frame, which makes both.
//   LEARN true:  bg is not read (it is a function of acc) but written: the state is oatgpu_bsub_filter's.
//   PAIR:        the stream's next frame in the same launch; acc and bg stay in registers between the two and are stored once.
//
// Two instantiations of the lane mapping (kernels_diff.hip's):
//   wide   (W % 4 == 0, frames and bg 4-byte, acc 16-byte aligned): a lane owns 4 consecutive pixels of one row -- CH dwords of
//          the frame, CH dwords of bg, CH 16-byte accesses of acc (a wave's 64 * 16 * CH bytes of acc are one contiguous run).
//          The accumulator leaves in 128-bit stores: each is followed by `s_nop 1` with its data registers live.
//   narrow (everything else): one pixel a lane with byte and dword accesses, the ballot is the word.
// Both write EVERY word of Palloc / 64 (zero bits for x >= W and p >= P): the row scan reads them.
//
// Where the pixels come from is a template argument of the lane code (pixel_source_inline.h): packed frames (k_bsubtrack_wide /
// k_bsubtrack_narrow), Bayer RAW8 demosaiced in registers into the 12 bytes a BGR frame would have held (FrontLaunch::bayer,
// k_bsubtrack_raw_*, the BGR lanes) or packed frames remapped in registers with the stream's undistortion map into
// the bytes an undistorted frame would have held (FrontLaunch::ud_map1, DESIGN.md 9g: k_bsubtrack_remap_*).  The ROI falls on the
// pixel the source hands back; bg and acc are BGR images, with a map in undistorted coordinates.
#include "oatgpu_internal.h"
#include "hsv_inline.h"
#include "maskwords_inline.h"
#include "pixel_rules_inline.h"
#include "pixel_source_inline.h"

namespace oatgpu {

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct BsubArgs {
    const uint8_t *frames, *frames2;     // [n][H*W*CH] stream-major (raw kernels: [n][H*W]); frames2: the second frame of a paired launch
    uint8_t *bg;                         // [n][H*W*CH]
    float *acc;                          // [n][H*W*CH]
    u64 *bits, *bits2;                   // [n][Palloc/64]
    const u64 *roi;                      // [n][Palloc/64]
    u64 first;                           // bit (stream - first_stream): this is the stream's first frame
    RangeParams rp;
    float a, b;                          // accW_: a = (float)alpha, b = 1 - a
    int first_stream;
};

template <int CH> __device__ __forceinline__ bool window(const int (&d)[CH], const RangeParams &rp)
{
    if constexpr (CH == 1) {
        return d[0] >= rp.lo[0] && d[0] <= rp.hi[0];
    } else {
        // V of the triple is its maximum: outside the V window -- every background pixel of a quiet scene -- H and S are not needed
        const int vmax = max(d[0], max(d[1], d[2]));
        if (vmax < rp.lo[2] || vmax > rp.hi[2]) return false;
        int h, s, v;
        bgr2hsv_inline(d[0], d[1], d[2], h, s, v);
        return in_range3(h, s, v, rp);
    }
}

// 4 pixels of one frame held as CH little-endian dwords: bg (CH dwords) and acc (4 * CH floats) move on; -> the 4 window bits
template <int CH, bool LEARN>
__device__ __forceinline__ unsigned frame4(const unsigned (&f)[CH], unsigned keep, bool first, unsigned (&bgw)[CH], float (&acc)[4 * CH],
                                           const BsubArgs &a)
{
    unsigned nib = 0, out[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) out[j] = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int d[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int e = k * CH + c, w = e >> 2, sh = (e & 3) * 8;
            const int x = (keep >> k) & 1u ? (int)((f[w] >> sh) & 255u) : 0;
            int bg = (int)((bgw[w] >> sh) & 255u);
            d[c] = bsub_elem<LEARN>(x, first, bg, acc[e], a.a, a.b);
            out[w] |= (unsigned)bg << sh;
        }
        nib |= window<CH>(d, a.rp) ? 1u << k : 0u;
    }
#pragma unroll
    for (int j = 0; j < CH; ++j) bgw[j] = out[j];
    return nib;
}

template <int CH, bool ROI, bool PAIR, bool LEARN, class SRC>
__device__ __forceinline__ void bsubtrack_wide(const Geom &g, const BsubArgs &a, SRC src)
{
    const int s = a.first_stream + (int)blockIdx.y;
    const bool first = (a.first >> blockIdx.y) & 1ull;               // uniform
    const QuadLane ql(g);
    const int y = ql.y, x = ql.x;
    const size_t npx = (size_t)g.H * g.W, NW = (size_t)(g.Palloc >> 6);
    unsigned n1 = 0, n2 = 0;
    if (ql.inside(g)) {
        const size_t e0 = ((size_t)s * npx + (size_t)y * g.W + x) * CH;          // the lane's first element: a multiple of 4
        unsigned keep = 15u;
        if (ROI) keep = ql.nibble(a.roi + (size_t)s * NW);
        unsigned f[CH], bgw[CH];
        float acc[4 * CH] = {};
        unsigned *bp = (unsigned *)(a.bg + e0);
        float4 *ap = (float4 *)(a.acc + e0);
        src.begin4(g, s, y, x);
        src.four(a.frames, g, s, y, x, f);
#pragma unroll
        for (int j = 0; j < CH; ++j) bgw[j] = 0;
        if (!first) {
            if (LEARN) {
#pragma unroll
                for (int j = 0; j < CH; ++j) { const float4 q = ap[j]; acc[4 * j] = q.x; acc[4 * j + 1] = q.y; acc[4 * j + 2] = q.z; acc[4 * j + 3] = q.w; }
            } else {
#pragma unroll
                for (int j = 0; j < CH; ++j) bgw[j] = bp[j];
            }
        }
        n1 = frame4<CH, LEARN>(f, keep, first, bgw, acc, a);
        if (PAIR) {
            src.four(a.frames2, g, s, y, x, f);
            n2 = frame4<CH, LEARN>(f, keep, false, bgw, acc, a);
        }
        if (LEARN || first) {
#pragma unroll
            for (int j = 0; j < CH; ++j) bp[j] = bgw[j];
#pragma unroll
            for (int j = 0; j < CH; ++j) {
                u32x4 q;
                q.x = __float_as_uint(acc[4 * j]); q.y = __float_as_uint(acc[4 * j + 1]);
                q.z = __float_as_uint(acc[4 * j + 2]); q.w = __float_as_uint(acc[4 * j + 3]);
                *(u32x4 *)(ap + j) = q;
                // a store of more than 64 bits reads its data registers after issue: two wait states, the registers live
                asm volatile("s_nop 1" :: "v"(q) : "memory");
            }
        }
    }
    store_words(n1, ql.lane, a.bits + (size_t)s * NW + (size_t)ql.wave * 4);
    if (PAIR) store_words(n2, ql.lane, a.bits2 + (size_t)s * NW + (size_t)ql.wave * 4);
}

template <int CH, bool ROI, bool PAIR, bool LEARN, class SRC>
__device__ __forceinline__ void bsubtrack_narrow(const Geom &g, const BsubArgs &a, SRC src)
{
    const int s = a.first_stream + (int)blockIdx.y;
    const bool first = (a.first >> blockIdx.y) & 1ull;               // uniform
    const WordLane l(g);                                             // Palloc % 256 == 0: every word of the grid exists
    const int y = l.y, x = l.x;
    const size_t npx = (size_t)g.H * g.W, NW = (size_t)(g.Palloc >> 6);
    bool on1 = false, on2 = false;
    if (l.inside(g)) {
        const size_t e0 = ((size_t)s * npx + (size_t)y * g.W + x) * CH;
        const bool keep = !ROI || ((a.roi[(size_t)s * NW + l.word] >> l.lane) & 1ull);
        int bg[CH], d[CH], v[CH];
        float acc[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) v[c] = 0;
        if (keep) { src.begin1(g, s, y, x); src.one(a.frames, g, s, y, x, v); }
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            bg[c] = 0; acc[c] = 0.f;
            if (!first) { if (LEARN) acc[c] = a.acc[e0 + c]; else bg[c] = a.bg[e0 + c]; }
            d[c] = bsub_elem<LEARN>(v[c], first, bg[c], acc[c], a.a, a.b);
        }
        on1 = window<CH>(d, a.rp);
        if (PAIR) {
            if (keep) src.one(a.frames2, g, s, y, x, v);
#pragma unroll
            for (int c = 0; c < CH; ++c) d[c] = bsub_elem<LEARN>(v[c], false, bg[c], acc[c], a.a, a.b);
            on2 = window<CH>(d, a.rp);
        }
        if (LEARN || first) {
#pragma unroll
            for (int c = 0; c < CH; ++c) { a.bg[e0 + c] = (uint8_t)bg[c]; a.acc[e0 + c] = acc[c]; }
        }
    }
    store_word(on1, l.lane, a.bits, (size_t)s * NW + l.word);
    if (PAIR) store_word(on2, l.lane, a.bits2, (size_t)s * NW + l.word);
}

// One kernel name a source and lane mapping; the raw and the remap kernels take what their source is built from
template <int CH, bool ROI, bool PAIR, bool LEARN> __global__ __launch_bounds__(256) void k_bsubtrack_wide(Geom g, BsubArgs a)
{
    bsubtrack_wide<CH, ROI, PAIR, LEARN>(g, a, PackedSource<CH, true>{});
}
template <int CH, bool ROI, bool PAIR, bool LEARN> __global__ __launch_bounds__(256) void k_bsubtrack_narrow(Geom g, BsubArgs a)
{
    bsubtrack_narrow<CH, ROI, PAIR, LEARN>(g, a, PackedSource<CH, true>{});
}
template <bool ROI, bool PAIR, bool LEARN> __global__ __launch_bounds__(256) void k_bsubtrack_raw_wide(Geom g, BsubArgs a, u64 r_row, u64 r_col)
{
    bsubtrack_wide<3, ROI, PAIR, LEARN>(g, a, RawSource(r_row, r_col));
}
template <bool ROI, bool PAIR, bool LEARN> __global__ __launch_bounds__(256) void k_bsubtrack_raw_narrow(Geom g, BsubArgs a, u64 r_row, u64 r_col)
{
    bsubtrack_narrow<3, ROI, PAIR, LEARN>(g, a, RawSource(r_row, r_col));
}
template <int CH, bool ROI, bool PAIR, bool LEARN>
__global__ __launch_bounds__(256) void k_bsubtrack_remap_wide(Geom g, BsubArgs a, const uint32_t *map1, const uint16_t *map2, size_t map_stride)
{
    bsubtrack_wide<CH, ROI, PAIR, LEARN>(g, a, RemapSource<CH>(a.first_stream, map1, map2, map_stride));
}
template <int CH, bool ROI, bool PAIR, bool LEARN>
__global__ __launch_bounds__(256) void k_bsubtrack_remap_narrow(Geom g, BsubArgs a, const uint32_t *map1, const uint16_t *map2, size_t map_stride)
{
    bsubtrack_narrow<CH, ROI, PAIR, LEARN>(g, a, RemapSource<CH>(a.first_stream, map1, map2, map_stride));
}

}  // namespace

// With a map (ud_map1) the frames are gathered with unaligned loads, so their own alignment does not count (the rule of
// diff_front_is_wide): bg, CH dwords a lane, and acc, CH 16-byte accesses a lane, still have to be aligned.
bool bsubtrack_front_is_wide(const Geom &g, const BsubLaunch &a)
{
    const uintptr_t m = a.ud_map1 ? (uintptr_t)a.bg : (uintptr_t)a.frames | (uintptr_t)a.frames2 | (uintptr_t)a.bg;
    return g.W % 4 == 0 && (m & 3u) == 0 && ((uintptr_t)a.acc & 15u) == 0;
}

void launch_bsubtrack_front(const Geom &g, const BsubLaunch &a, int n_streams, hipStream_t st)
{
    const bool wide = bsubtrack_front_is_wide(g, a);
    for (int s0 = 0; s0 < n_streams; s0 += 64) {         // the first-frame mask and the parity bits of a launch are 64-bit kernel arguments
        const int n = n_streams - s0 < 64 ? n_streams - s0 : 64;
        BsubArgs k{a.frames, a.frames2, a.bg, a.acc, a.bits, a.bits2, a.roi, 0ull, a.rp, a.a, a.b, s0};
        for (int i = 0; i < n; ++i) k.first |= (u64)(a.have[s0 + i] == 0) << i;
        // the source, then CH, ROI, PAIR and LEARN pick the kernel pair; `wide` picks of the pair and sets the grid
        auto launch = [&](auto *k_wide, auto *k_narrow, auto... source_args) {
            hipLaunchKernelGGL(wide ? k_wide : k_narrow, dim3(g.Palloc / (wide ? 1024 : 256), n), dim3(256), 0, st, g, k, source_args...);
        };
        const bool ch3 = a.channels == 3, roi = a.roi != nullptr, pair = a.frames2 != nullptr;
        if (a.bayer) {
            u64 r_row, r_col;
            bayer_parity_bits(a.bayer + s0, n, r_row, r_col);
            lift_bools([&](auto ROI, auto PAIR, auto LEARN) {
                launch(k_bsubtrack_raw_wide<ROI, PAIR, LEARN>, k_bsubtrack_raw_narrow<ROI, PAIR, LEARN>, r_row, r_col);
            }, roi, pair, a.learn);
        } else if (a.ud_map1) {
            lift_bools([&](auto CH3, auto ROI, auto PAIR, auto LEARN) {
                launch(k_bsubtrack_remap_wide<CH3 ? 3 : 1, ROI, PAIR, LEARN>, k_bsubtrack_remap_narrow<CH3 ? 3 : 1, ROI, PAIR, LEARN>,
                       a.ud_map1, a.ud_map2, a.ud_stride);
            }, ch3, roi, pair, a.learn);
        } else {
            lift_bools([&](auto CH3, auto ROI, auto PAIR, auto LEARN) {
                launch(k_bsubtrack_wide<CH3 ? 3 : 1, ROI, PAIR, LEARN>, k_bsubtrack_narrow<CH3 ? 3 : 1, ROI, PAIR, LEARN>);
            }, ch3, roi, pair, a.learn);
        }
    }
}

}  // namespace oatgpu
