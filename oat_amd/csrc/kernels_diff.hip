// kernels_diff.hip -- the front end of the motion tracker (`framefilt col -C GREY` -> `posidet diff`) for every
// camera stream of a context in one launch (grid y = stream).
//
// Per pixel: g = grey(B, G, R) (3 channels, RGB2Gray<uchar>'s integers) or the pixel itself (1 channel); g = 0 where the
// stream's ROI bit is 0 (framefilt mask in front of col: grey(0, 0, 0) = 0); bit = have_last ? |g - last| > thr : g != 0
// (cv::absdiff + cv::threshold(THRESH_BINARY), DifferenceDetector.cpp:156-171); last = g.  With a second frame in the launch
// (PAIR) the first frame's grey stays in registers: bits2 = |g2 - g| > thr, last = g2.
//
// Two instantiations of the lane mapping:
//   wide   (W % 4 == 0, frame and `last` 4-byte aligned): a lane owns 4 consecutive pixels of one row -- one dword load and one
//          dword store of `last`, one dword (GREY) or three dwords (BGR, 12 bytes) of the frame.  A wave covers 256 pixels = 4
//          mask words; bit k of every lane is gathered by one ballot, and lane w < 4 interleaves the four 16-bit fields of its
//          word out of the four ballots and stores it: every word is stored once, 64 bits a lane.
//   narrow (everything else): one pixel a lane with byte accesses, the ballot is the word (k_absdiff_bits' mapping).
// Both write EVERY word of Palloc / 64 (zero bits for x >= W and p >= P): the row scan reads them.
//
// Where the pixels come from is a template argument of the lane code (pixel_source_inline.h): packed frames (k_diff_wide /
// k_diff_narrow), Bayer RAW8 demosaiced in registers (FrontLaunch::bayer, DESIGN.md 9f: k_diff_raw_*) or packed frames remapped in
// registers with the stream's undistortion map (FrontLaunch::ud_map1, DESIGN.md 9g: k_diff_remap_*).  The grey is taken of what
// the source hands back -- of the demosaiced or the remapped triple, the chain's order: undistort, mask, col GREY -- and the ROI
// falls on that pixel.
#include "oatgpu_internal.h"
#include "maskwords_inline.h"
#include "pixel_rules_inline.h"
#include "pixel_source_inline.h"

namespace oatgpu {

namespace {

// col GREY of one pixel's values
template <class T, int CH> __device__ __forceinline__ int grey_of(const T (&v)[CH])
{
    if constexpr (CH == 1) return (int)v[0];
    else return (int)grey_bgr(v[0], v[1], v[2]);
}
// the greys of a source's 4 pixels from (y, x) on as one little-endian dword, and the grey of its pixel (y, x)
template <class SRC> __device__ __forceinline__ unsigned grey4(const SRC &src, const uint8_t *frames, const Geom &g, int s, int y, int x)
{
    unsigned gr = 0;
    src.each4(frames, g, s, y, x, [&](int k, const unsigned (&v)[SRC::kCH]) { gr |= (unsigned)grey_of(v) << (8 * k); });
    return gr;
}
template <class SRC> __device__ __forceinline__ int grey1(const SRC &src, const uint8_t *frames, const Geom &g, int s, int y, int x)
{
    int v[SRC::kCH];
    src.one(frames, g, s, y, x, v);
    return grey_of(v);
}

struct DiffArgs {
    const uint8_t *frames, *frames2;     // [n][H*W*CH] stream-major (raw kernels: [n][H*W]); frames2: the second frame of a paired launch
    uint8_t *last;                       // [n][H*W]
    u64 *bits, *bits2;                   // [n][Palloc/64]
    const u64 *roi;                      // [n][Palloc/64]
    u64 have;                            // bit (stream - first_stream): the stream has a last image
    int thr, first_stream;
};

template <bool ROI, bool PAIR, class SRC> __device__ __forceinline__ void diff_wide(const Geom &g, const DiffArgs &a, SRC src)
{
    const int s = a.first_stream + (int)blockIdx.y;
    const bool have = PAIR || ((a.have >> blockIdx.y) & 1ull);      // uniform
    const QuadLane ql(g);
    const int y = ql.y, x = ql.x;
    const size_t npx = (size_t)g.H * g.W, NW = (size_t)(g.Palloc >> 6);
    unsigned n1 = 0, n2 = 0;
    if (ql.inside(g)) {
        const size_t i = (size_t)y * g.W + x;
        unsigned *lp = (unsigned *)(a.last + (size_t)s * npx + i);
        unsigned keep = 0xffffffffu;
        if (ROI) {
            const unsigned r = ql.nibble(a.roi + (size_t)s * NW);
            keep = (r & 1u ? 0xffu : 0u) | (r & 2u ? 0xff00u : 0u) | (r & 4u ? 0xff0000u : 0u) | (r & 8u ? 0xff000000u : 0u);
        }
        src.begin4(g, s, y, x);
        const unsigned g1 = grey4(src, a.frames, g, s, y, x) & keep;
        if (have) {                                                  // (uniform: one branch, not one a pixel)
            const unsigned l = *lp;
#pragma unroll
            for (int k = 0; k < 4; ++k) n1 |= motion_bit((g1 >> (8 * k)) & 255u, (l >> (8 * k)) & 255u, true, a.thr) ? 1u << k : 0u;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) n1 |= motion_bit((g1 >> (8 * k)) & 255u, 0, false, a.thr) ? 1u << k : 0u;
        }
        unsigned out = g1;
        if (PAIR) {
            const unsigned g2 = grey4(src, a.frames2, g, s, y, x) & keep;
#pragma unroll
            for (int k = 0; k < 4; ++k) n2 |= differs((g2 >> (8 * k)) & 255u, (g1 >> (8 * k)) & 255u, a.thr) ? 1u << k : 0u;
            out = g2;
        }
        *lp = out;
    }
    store_words(n1, ql.lane, a.bits + (size_t)s * NW + (size_t)ql.wave * 4);
    if (PAIR) store_words(n2, ql.lane, a.bits2 + (size_t)s * NW + (size_t)ql.wave * 4);
}

template <bool ROI, bool PAIR, class SRC> __device__ __forceinline__ void diff_narrow(const Geom &g, const DiffArgs &a, SRC src)
{
    const int s = a.first_stream + (int)blockIdx.y;
    const bool have = PAIR || ((a.have >> blockIdx.y) & 1ull);
    const WordLane l(g);                                             // Palloc % 256 == 0: every word of the grid exists
    const int y = l.y, x = l.x;
    const size_t npx = (size_t)g.H * g.W, NW = (size_t)(g.Palloc >> 6);
    bool on1 = false, on2 = false;
    if (l.inside(g)) {
        const size_t i = (size_t)y * g.W + x;
        uint8_t *lp = a.last + (size_t)s * npx + i;
        const bool keep = !ROI || ((a.roi[(size_t)s * NW + l.word] >> l.lane) & 1ull);
        if (keep) src.begin1(g, s, y, x);
        const int g1 = keep ? grey1(src, a.frames, g, s, y, x) : 0;
        on1 = motion_bit(g1, have ? *lp : 0, have, a.thr);
        int out = g1;
        if (PAIR) {
            const int g2 = keep ? grey1(src, a.frames2, g, s, y, x) : 0;
            on2 = differs(g2, g1, a.thr);
            out = g2;
        }
        *lp = (uint8_t)out;
    }
    store_word(on1, l.lane, a.bits, (size_t)s * NW + l.word);
    if (PAIR) store_word(on2, l.lane, a.bits2, (size_t)s * NW + l.word);
}

// One kernel name a source and lane mapping; the raw and the remap kernels take what their source is built from
template <int CH, bool ROI, bool PAIR> __global__ __launch_bounds__(256) void k_diff_wide(Geom g, DiffArgs a)
{
    diff_wide<ROI, PAIR>(g, a, PackedSource<CH>{});
}
template <int CH, bool ROI, bool PAIR> __global__ __launch_bounds__(256) void k_diff_narrow(Geom g, DiffArgs a)
{
    diff_narrow<ROI, PAIR>(g, a, PackedSource<CH>{});
}
template <bool ROI, bool PAIR> __global__ __launch_bounds__(256) void k_diff_raw_wide(Geom g, DiffArgs a, u64 r_row, u64 r_col)
{
    diff_wide<ROI, PAIR>(g, a, RawSource(r_row, r_col));
}
template <bool ROI, bool PAIR> __global__ __launch_bounds__(256) void k_diff_raw_narrow(Geom g, DiffArgs a, u64 r_row, u64 r_col)
{
    diff_narrow<ROI, PAIR>(g, a, RawSource(r_row, r_col));
}
template <int CH, bool ROI, bool PAIR>
__global__ __launch_bounds__(256) void k_diff_remap_wide(Geom g, DiffArgs a, const uint32_t *map1, const uint16_t *map2, size_t map_stride)
{
    diff_wide<ROI, PAIR>(g, a, RemapSource<CH>(a.first_stream, map1, map2, map_stride));
}
template <int CH, bool ROI, bool PAIR>
__global__ __launch_bounds__(256) void k_diff_remap_narrow(Geom g, DiffArgs a, const uint32_t *map1, const uint16_t *map2, size_t map_stride)
{
    diff_narrow<ROI, PAIR>(g, a, RemapSource<CH>(a.first_stream, map1, map2, map_stride));
}

}  // namespace

// With a map (ud_map1) the frames are gathered with unaligned loads, so their own alignment does not count: W % 4 == 0 keeps a
// lane's 4 pixels in one row and its map index a multiple of 4, and only `last`, still one dword a lane, has to be aligned.
bool diff_front_is_wide(const Geom &g, const DiffLaunch &a)
{
    const uintptr_t m = a.ud_map1 ? (uintptr_t)a.last : (uintptr_t)a.frames | (uintptr_t)a.frames2 | (uintptr_t)a.last;
    return g.W % 4 == 0 && (m & 3u) == 0;
}

void launch_diff_front(const Geom &g, const DiffLaunch &a, int n_streams, hipStream_t st)
{
    const bool wide = diff_front_is_wide(g, a);
    for (int s0 = 0; s0 < n_streams; s0 += 64) {         // the have-last mask and the parity bits of a launch are 64-bit kernel arguments
        const int n = n_streams - s0 < 64 ? n_streams - s0 : 64;
        DiffArgs k{a.frames, a.frames2, a.last, a.bits, a.bits2, a.roi, 0ull, a.thr, s0};
        for (int i = 0; i < n; ++i) k.have |= (u64)(a.have_last[s0 + i] != 0) << i;
        // the source, then CH, ROI and PAIR pick the kernel pair; `wide` picks of the pair and sets the grid
        auto launch = [&](auto *k_wide, auto *k_narrow, auto... source_args) {
            hipLaunchKernelGGL(wide ? k_wide : k_narrow, dim3(g.Palloc / (wide ? 1024 : 256), n), dim3(256), 0, st, g, k, source_args...);
        };
        const bool ch3 = a.channels == 3, roi = a.roi != nullptr, pair = a.frames2 != nullptr;
        if (a.bayer) {
            u64 r_row, r_col;
            bayer_parity_bits(a.bayer + s0, n, r_row, r_col);
            lift_bools([&](auto ROI, auto PAIR) { launch(k_diff_raw_wide<ROI, PAIR>, k_diff_raw_narrow<ROI, PAIR>, r_row, r_col); }, roi, pair);
        } else if (a.ud_map1) {
            lift_bools([&](auto CH3, auto ROI, auto PAIR) {
                launch(k_diff_remap_wide<CH3 ? 3 : 1, ROI, PAIR>, k_diff_remap_narrow<CH3 ? 3 : 1, ROI, PAIR>, a.ud_map1, a.ud_map2, a.ud_stride);
            }, ch3, roi, pair);
        } else {
            lift_bools([&](auto CH3, auto ROI, auto PAIR) { launch(k_diff_wide<CH3 ? 3 : 1, ROI, PAIR>, k_diff_narrow<CH3 ? 3 : 1, ROI, PAIR>); }, ch3, roi, pair);
        }
    }
}

}  // namespace oatgpu

