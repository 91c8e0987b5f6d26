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
// Bayer RAW8 frames (DiffLaunch::bayer): k_diff_raw_wide / k_diff_raw_narrow are the same lanes with another pixel
// source -- the lane demosaics its pixels in registers (debayer_inline.h: the dwords at x0 - 4, x0, x0 + 4 of raw rows y - 1, y,
// y + 1, or 9 byte loads) and takes the grey of the triples; the ROI falls on the demosaiced pixel.  The pattern is run-time
// data, two parity bits a stream in two 64-bit kernel arguments.
//
// Lens undistortion (DiffLaunch::ud_map1): k_diff_remap_wide / k_diff_remap_narrow are the same lanes with a third
// pixel source -- the lane loads the map entries of its own pixels (raster index y * W + x of the stream's planes: one 16-byte
// and one 8-byte load for 4 pixels, or one entry of each plane), keeps them in registers for both frames of a paired launch, and
// gathers each pixel's 2 x 2 neighbourhood from the caller's frame with undistort_inline.h's remap_px.  B, G and R are remapped
// each on its own and the grey is taken of the remapped triple (the chain's order: undistort, mask, col GREY); the ROI falls on
// the undistorted pixel.
#include "oatgpu_internal.h"
#include "debayer_inline.h"
#include "maskwords_inline.h"
#include "undistort_inline.h"

namespace oatgpu {

namespace {

__device__ __forceinline__ int grey_bgr(unsigned b, unsigned g, unsigned r)
{
    return (int)((1868u * b + 9617u * g + 4899u * r + 8192u) >> 14);
}
__device__ __forceinline__ bool differs(int a, int b, int thr) { return (a > b ? a - b : b - a) > thr; }

// byte k of three little-endian dwords
__device__ __forceinline__ unsigned byte_of(const unsigned (&d)[3], int k) { return (d[k >> 2] >> ((k & 3) * 8)) & 255u; }

// the four greys of the 4 pixels at raster index i (a multiple of 4) of one frame, as one little-endian dword
template <int CH> __device__ __forceinline__ unsigned grey4(const uint8_t *frame, size_t i)
{
    if (CH == 1) return *(const unsigned *)(frame + i);
    const unsigned *q = (const unsigned *)(frame + 3 * i);
    const unsigned d[3] = {q[0], q[1], q[2]};
    unsigned g = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) g |= (unsigned)grey_bgr(byte_of(d, 3 * k), byte_of(d, 3 * k + 1), byte_of(d, 3 * k + 2)) << (8 * k);
    return g;
}
template <int CH> __device__ __forceinline__ int grey1(const uint8_t *frame, size_t i)
{
    if (CH == 1) return frame[i];
    return grey_bgr(frame[3 * i], frame[3 * i + 1], frame[3 * i + 2]);
}

// Where a lane's greys come from: `frames` is a frame set of the launch (stream-major), s the stream, (y, x) the pixel
// (four: x % 4 == 0, the four pixels from x on as one little-endian dword).  begin4 / begin1 run once a lane ahead of the
// first four / one: what the lane keeps for every frame of the launch.
template <int CH> struct PackedSource {                  // packed BGR (3) or GREY (1) frames
    __device__ __forceinline__ void begin4(const Geom &, int, int, int) {}
    __device__ __forceinline__ void begin1(const Geom &, int, int, int) {}
    __device__ __forceinline__ unsigned four(const uint8_t *frames, const Geom &g, int s, int y, int x) const
    {
        return grey4<CH>(frames + (size_t)s * g.H * g.W * CH, (size_t)y * g.W + x);
    }
    __device__ __forceinline__ int one(const uint8_t *frames, const Geom &g, int s, int y, int x) const
    {
        return grey1<CH>(frames + (size_t)s * g.H * g.W * CH, (size_t)y * g.W + x);
    }
};
struct RawSource {                                       // Bayer RAW8 frames, demosaiced in registers
    bool r_row, r_col;                                   // parity of the row / the column of the stream's R sample (uniform)
    __device__ __forceinline__ void begin4(const Geom &, int, int, int) {}
    __device__ __forceinline__ void begin1(const Geom &, int, int, int) {}
    __device__ __forceinline__ unsigned four(const uint8_t *frames, const Geom &g, int s, int y, int x) const
    {
        unsigned px[4], v = 0;
        debayer_px4(frames + (size_t)s * g.H * g.W, g.H, g.W, y, x, r_row, r_col, px);
#pragma unroll
        for (int k = 0; k < 4; ++k) v |= (unsigned)grey_bgr(px[k] & 255u, (px[k] >> 8) & 255u, px[k] >> 16) << (8 * k);
        return v;
    }
    __device__ __forceinline__ int one(const uint8_t *frames, const Geom &g, int s, int y, int x) const
    {
        const unsigned p = debayer_px1(frames + (size_t)s * g.H * g.W, g.H, g.W, y, x, r_row, r_col);
        return grey_bgr(p & 255u, (p >> 8) & 255u, p >> 16);
    }
};

template <int CH> struct RemapSource {                   // packed frames seen through the stream's undistortion map
    const uint32_t *map1;                                // the STREAM's planes (uniform)
    const uint16_t *map2;
    uint32_t m1[4], m2[4];                               // the lane's map entries: loaded once, used for every frame of the launch
    __device__ __forceinline__ void begin4(const Geom &g, int, int y, int x) { load_map4(map1, map2, (size_t)y * g.W + x, m1, m2); }
    __device__ __forceinline__ void begin1(const Geom &g, int, int y, int x)
    {
        const size_t i = (size_t)y * g.W + x;
        m1[0] = map1[i]; m2[0] = map2[i];
    }
    __device__ __forceinline__ int grey(const uint8_t *frame, const Geom &g, int k) const
    {
        uint32_t v[CH];
        remap_px<CH>(frame, g.H, g.W, m1[k], m2[k], v);
        if constexpr (CH == 1) return (int)v[0];
        else return grey_bgr(v[0], v[1], v[2]);
    }
    __device__ __forceinline__ unsigned four(const uint8_t *frames, const Geom &g, int s, int, int) const
    {
        const uint8_t *frame = frames + (size_t)s * g.H * g.W * CH;
        unsigned v = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) v |= (unsigned)grey(frame, g, k) << (8 * k);
        return v;
    }
    __device__ __forceinline__ int one(const uint8_t *frames, const Geom &g, int s, int, int) const
    {
        return grey(frames + (size_t)s * g.H * g.W * CH, g, 0);
    }
};

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
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);            // 256 pixels = words 4 * wave .. 4 * wave + 3; Palloc % 1024 == 0
    const int p0 = wave * 256 + lane * 4;
    const int y = p0 / g.Wp, x = p0 - y * g.Wp;
    const size_t npx = (size_t)g.H * g.W, NW = (size_t)(g.Palloc >> 6);
    unsigned n1 = 0, n2 = 0;
    if (p0 < g.P && x < g.W) {                                       // W % 4 == 0: the lane's 4 pixels are inside together
        const size_t i = (size_t)y * g.W + x;
        unsigned *lp = (unsigned *)(a.last + (size_t)s * npx + i);
        unsigned keep = 0xffffffffu;
        if (ROI) {
            const unsigned r = (((const uint8_t *)(a.roi + (size_t)s * NW))[p0 >> 3] >> (p0 & 4)) & 15u;
            keep = (r & 1u ? 0xffu : 0u) | (r & 2u ? 0xff00u : 0u) | (r & 4u ? 0xff0000u : 0u) | (r & 8u ? 0xff000000u : 0u);
        }
        src.begin4(g, s, y, x);
        const unsigned g1 = src.four(a.frames, g, s, y, x) & keep;
        if (have) {
            const unsigned l = *lp;
#pragma unroll
            for (int k = 0; k < 4; ++k) n1 |= differs((g1 >> (8 * k)) & 255u, (l >> (8 * k)) & 255u, a.thr) ? 1u << k : 0u;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) n1 |= ((g1 >> (8 * k)) & 255u) ? 1u << k : 0u;
        }
        unsigned out = g1;
        if (PAIR) {
            const unsigned g2 = src.four(a.frames2, g, s, y, x) & keep;
#pragma unroll
            for (int k = 0; k < 4; ++k) n2 |= differs((g2 >> (8 * k)) & 255u, (g1 >> (8 * k)) & 255u, a.thr) ? 1u << k : 0u;
            out = g2;
        }
        *lp = out;
    }
    store_words(n1, lane, a.bits + (size_t)s * NW + (size_t)wave * 4);
    if (PAIR) store_words(n2, lane, a.bits2 + (size_t)s * NW + (size_t)wave * 4);
}

template <bool ROI, bool PAIR, class SRC> __device__ __forceinline__ void diff_narrow(const Geom &g, const DiffArgs &a, SRC src)
{
    const int s = a.first_stream + (int)blockIdx.y;
    const bool have = PAIR || ((a.have >> blockIdx.y) & 1ull);
    const int lane = threadIdx.x & 63;
    const int word = blockIdx.x * 4 + (threadIdx.x >> 6);            // Palloc % 256 == 0: every word of the grid exists
    const int p = word * 64 + lane;
    const int y = p / g.Wp, x = p - y * g.Wp;
    const size_t npx = (size_t)g.H * g.W, NW = (size_t)(g.Palloc >> 6);
    bool on1 = false, on2 = false;
    if (p < g.P && x < g.W) {
        const size_t i = (size_t)y * g.W + x;
        uint8_t *lp = a.last + (size_t)s * npx + i;
        const bool keep = !ROI || ((a.roi[(size_t)s * NW + word] >> lane) & 1ull);
        if (keep) src.begin1(g, s, y, x);
        const int g1 = keep ? src.one(a.frames, g, s, y, x) : 0;
        on1 = have ? differs(g1, *lp, a.thr) : g1 != 0;
        int out = g1;
        if (PAIR) {
            const int g2 = keep ? src.one(a.frames2, g, s, y, x) : 0;
            on2 = differs(g2, g1, a.thr);
            out = g2;
        }
        *lp = (uint8_t)out;
    }
    const u64 w1 = __ballot(on1);
    if (lane == 0) a.bits[(size_t)s * NW + word] = w1;
    if (PAIR) {
        const u64 w2 = __ballot(on2);
        if (lane == 0) a.bits2[(size_t)s * NW + word] = w2;
    }
}

template <int CH, bool ROI, bool PAIR> __global__ __launch_bounds__(256) void k_diff_wide(Geom g, DiffArgs a)
{
    diff_wide<ROI, PAIR>(g, a, PackedSource<CH>{});
}
template <int CH, bool ROI, bool PAIR> __global__ __launch_bounds__(256) void k_diff_narrow(Geom g, DiffArgs a)
{
    diff_narrow<ROI, PAIR>(g, a, PackedSource<CH>{});
}
// r_row, r_col: bit (stream - first_stream), the parity of the row / the column of the stream's R sample
template <bool ROI, bool PAIR> __global__ __launch_bounds__(256) void k_diff_raw_wide(Geom g, DiffArgs a, u64 r_row, u64 r_col)
{
    diff_wide<ROI, PAIR>(g, a, RawSource{(bool)((r_row >> blockIdx.y) & 1ull), (bool)((r_col >> blockIdx.y) & 1ull)});
}
template <bool ROI, bool PAIR> __global__ __launch_bounds__(256) void k_diff_raw_narrow(Geom g, DiffArgs a, u64 r_row, u64 r_col)
{
    diff_narrow<ROI, PAIR>(g, a, RawSource{(bool)((r_row >> blockIdx.y) & 1ull), (bool)((r_col >> blockIdx.y) & 1ull)});
}

// map1, map2: plane 0 of the context's maps; the stream's planes start map_stride entries a stream further on
template <int CH, bool ROI, bool PAIR>
__global__ __launch_bounds__(256) void k_diff_remap_wide(Geom g, DiffArgs a, const uint32_t *map1, const uint16_t *map2, size_t map_stride)
{
    const size_t off = (size_t)(a.first_stream + (int)blockIdx.y) * map_stride;
    diff_wide<ROI, PAIR>(g, a, RemapSource<CH>{map1 + off, map2 + off, {}, {}});
}
template <int CH, bool ROI, bool PAIR>
__global__ __launch_bounds__(256) void k_diff_remap_narrow(Geom g, DiffArgs a, const uint32_t *map1, const uint16_t *map2, size_t map_stride)
{
    const size_t off = (size_t)(a.first_stream + (int)blockIdx.y) * map_stride;
    diff_narrow<ROI, PAIR>(g, a, RemapSource<CH>{map1 + off, map2 + off, {}, {}});
}

template <int CH, bool ROI, bool PAIR> void launch_one(const Geom &g, const DiffArgs &a, bool wide, int n, hipStream_t st)
{
    if (wide) hipLaunchKernelGGL((k_diff_wide<CH, ROI, PAIR>), dim3(g.Palloc / 1024, n), dim3(256), 0, st, g, a);
    else hipLaunchKernelGGL((k_diff_narrow<CH, ROI, PAIR>), dim3(g.Palloc / 256, n), dim3(256), 0, st, g, a);
}
template <int CH> void launch_ch(const Geom &g, const DiffArgs &a, bool wide, int n, hipStream_t st)
{
    const bool roi = a.roi != nullptr, pair = a.frames2 != nullptr;
    if (roi) { if (pair) launch_one<CH, true, true>(g, a, wide, n, st); else launch_one<CH, true, false>(g, a, wide, n, st); }
    else { if (pair) launch_one<CH, false, true>(g, a, wide, n, st); else launch_one<CH, false, false>(g, a, wide, n, st); }
}

template <bool ROI, bool PAIR> void launch_raw_one(const Geom &g, const DiffArgs &a, u64 r_row, u64 r_col, bool wide, int n, hipStream_t st)
{
    if (wide) hipLaunchKernelGGL((k_diff_raw_wide<ROI, PAIR>), dim3(g.Palloc / 1024, n), dim3(256), 0, st, g, a, r_row, r_col);
    else hipLaunchKernelGGL((k_diff_raw_narrow<ROI, PAIR>), dim3(g.Palloc / 256, n), dim3(256), 0, st, g, a, r_row, r_col);
}
void launch_raw(const Geom &g, const DiffArgs &a, u64 r_row, u64 r_col, bool wide, int n, hipStream_t st)
{
    const bool roi = a.roi != nullptr, pair = a.frames2 != nullptr;
    if (roi) { if (pair) launch_raw_one<true, true>(g, a, r_row, r_col, wide, n, st); else launch_raw_one<true, false>(g, a, r_row, r_col, wide, n, st); }
    else { if (pair) launch_raw_one<false, true>(g, a, r_row, r_col, wide, n, st); else launch_raw_one<false, false>(g, a, r_row, r_col, wide, n, st); }
}

struct MapPlanes { const uint32_t *map1; const uint16_t *map2; size_t stride; };
template <int CH, bool ROI, bool PAIR> void launch_remap_one(const Geom &g, const DiffArgs &a, MapPlanes m, bool wide, int n, hipStream_t st)
{
    if (wide) hipLaunchKernelGGL((k_diff_remap_wide<CH, ROI, PAIR>), dim3(g.Palloc / 1024, n), dim3(256), 0, st, g, a, m.map1, m.map2, m.stride);
    else hipLaunchKernelGGL((k_diff_remap_narrow<CH, ROI, PAIR>), dim3(g.Palloc / 256, n), dim3(256), 0, st, g, a, m.map1, m.map2, m.stride);
}
template <int CH> void launch_remap(const Geom &g, const DiffArgs &a, MapPlanes m, bool wide, int n, hipStream_t st)
{
    const bool roi = a.roi != nullptr, pair = a.frames2 != nullptr;
    if (roi) { if (pair) launch_remap_one<CH, true, true>(g, a, m, wide, n, st); else launch_remap_one<CH, true, false>(g, a, m, wide, n, st); }
    else { if (pair) launch_remap_one<CH, false, true>(g, a, m, wide, n, st); else launch_remap_one<CH, false, false>(g, a, m, wide, n, st); }
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
        if (a.bayer) {
            u64 r_row, r_col;
            bayer_parity_bits(a.bayer + s0, n, r_row, r_col);
            launch_raw(g, k, r_row, r_col, wide, n, st);
        } else if (a.ud_map1) {
            const MapPlanes m{a.ud_map1, a.ud_map2, a.ud_stride};
            if (a.channels == 3) launch_remap<3>(g, k, m, wide, n, st);
            else launch_remap<1>(g, k, m, wide, n, st);
        } else if (a.channels == 3) launch_ch<3>(g, k, wide, n, st);
        else launch_ch<1>(g, k, wide, n, st);
    }
}

}  // namespace oatgpu

