// pixel_source_inline.h -- where a lane of the two batched trackers' front kernels (kernels_diff.hip, kernels_bsubtrack.hip) takes
// its pixels from.  Three sources, one contract:
//   PackedSource<CH>  packed BGR (3) or GREY (1) frames as the caller gave them
//   RawSource         Bayer RAW8 frames, demosaiced in registers (debayer_inline.h): BGR pixels
//   RemapSource<CH>   packed frames seen through the stream's undistortion map (undistort_inline.h)
// A source is built from the launch's kernel arguments (the stream is blockIdx.y).  `frames` is a frame set of the launch
// (stream-major), s the stream, (y, x) the pixel; kCH is the number of channels of a pixel.
//   begin4 / begin1   once a lane, ahead of the first four / each4 / one: what the lane keeps for every frame of the launch
//   four              x % 4 == 0: the 4 pixels from x on as the kCH little-endian dwords a packed frame holds
//   each4             the same 4 pixels one by one: use(k, v) with v[c] = channel c of pixel x + k
//   one               the kCH values of the pixel
// four and each4 are two views of the same loads: a kernel uses the one its arithmetic wants (the subtraction tracker the
// dwords, the motion tracker, which takes a grey of every pixel, the values).  RemapSource::four repeats each4's loop instead
// of calling it: the compiler gives the subtraction tracker's kernels other code otherwise (profiles/front_kernels_refactor.txt).
#pragma once
#include "oatgpu_internal.h"
#include "debayer_inline.h"
#include "undistort_inline.h"

namespace oatgpu {

// byte k of CH little-endian dwords
template <int CH> __device__ __forceinline__ unsigned byte_of(const unsigned (&d)[CH], int k) { return (d[k >> 2] >> ((k & 3) * 8)) & 255u; }

// STREAM_IN_LANE: the stream joins the lane's 64-bit index arithmetic (kernels_bsubtrack.hip) instead of moving the uniform base
// pointer (kernels_diff.hip, and the other two sources).  The same address: each unit keeps the form its registers were counted with.
template <int CH, bool STREAM_IN_LANE = false> struct PackedSource {
    static constexpr int kCH = CH;
    __device__ __forceinline__ const uint8_t *at(const uint8_t *frames, const Geom &g, int s, int y, int x) const
    {
        if constexpr (STREAM_IN_LANE) return frames + (((size_t)s * g.H + y) * g.W + x) * CH;
        else return frames + (size_t)s * g.H * g.W * CH + ((size_t)y * g.W + x) * CH;
    }
    __device__ __forceinline__ void begin4(const Geom &, int, int, int) {}
    __device__ __forceinline__ void begin1(const Geom &, int, int, int) {}
    __device__ __forceinline__ void four(const uint8_t *frames, const Geom &g, int s, int y, int x, unsigned (&f)[CH]) const
    {
        const unsigned *fp = (const unsigned *)at(frames, g, s, y, x);
#pragma unroll
        for (int j = 0; j < CH; ++j) f[j] = fp[j];
    }
    template <class F> __device__ __forceinline__ void each4(const uint8_t *frames, const Geom &g, int s, int y, int x, F &&use) const
    {
        unsigned f[CH];
        four(frames, g, s, y, x, f);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            unsigned v[CH];
#pragma unroll
            for (int c = 0; c < CH; ++c) v[c] = byte_of(f, k * CH + c);
            use(k, v);
        }
    }
    __device__ __forceinline__ void one(const uint8_t *frames, const Geom &g, int s, int y, int x, int (&v)[CH]) const
    {
        const uint8_t *fp = at(frames, g, s, y, x);
#pragma unroll
        for (int c = 0; c < CH; ++c) v[c] = fp[c];
    }
};

struct RawSource {
    static constexpr int kCH = 3;
    bool r_row, r_col;                                   // parity of the row / the column of the stream's R sample (uniform)
    // r_row, r_col: bit (stream - first_stream) of the launch's two parity words (bayer_parity_bits)
    __device__ __forceinline__ RawSource(u64 r_row, u64 r_col) : r_row((r_row >> blockIdx.y) & 1ull), r_col((r_col >> blockIdx.y) & 1ull) {}
    __device__ __forceinline__ void begin4(const Geom &, int, int, int) {}
    __device__ __forceinline__ void begin1(const Geom &, int, int, int) {}
    __device__ __forceinline__ void px4(const uint8_t *frames, const Geom &g, int s, int y, int x, unsigned (&px)[4]) const
    {
        debayer_px4(frames + (size_t)s * g.H * g.W, g.H, g.W, y, x, r_row, r_col, px);
    }
    __device__ __forceinline__ void four(const uint8_t *frames, const Geom &g, int s, int y, int x, unsigned (&f)[3]) const
    {
        unsigned px[4];
        px4(frames, g, s, y, x, px);
        pack_bgr4(px, f);
    }
    template <class F> __device__ __forceinline__ void each4(const uint8_t *frames, const Geom &g, int s, int y, int x, F &&use) const
    {
        unsigned px[4];
        px4(frames, g, s, y, x, px);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned v[3] = {px[k] & 255u, (px[k] >> 8) & 255u, px[k] >> 16};
            use(k, v);
        }
    }
    __device__ __forceinline__ void one(const uint8_t *frames, const Geom &g, int s, int y, int x, int (&v)[3]) const
    {
        const unsigned p = debayer_px1(frames + (size_t)s * g.H * g.W, g.H, g.W, y, x, r_row, r_col);
        v[0] = p & 255u; v[1] = (p >> 8) & 255u; v[2] = p >> 16;
    }
};

template <int CH> struct RemapSource {
    static constexpr int kCH = CH;
    const uint32_t *map1;                                // the STREAM's planes (uniform)
    const uint16_t *map2;
    uint32_t m1[4], m2[4];                               // the lane's map entries: loaded once, used for every frame of the launch
    // map1, map2: plane 0 of the context's maps; the stream's planes start map_stride entries a stream further on
    __device__ __forceinline__ RemapSource(int first_stream, const uint32_t *map1, const uint16_t *map2, size_t map_stride)
        : map1(map1 + (size_t)(first_stream + (int)blockIdx.y) * map_stride),
          map2(map2 + (size_t)(first_stream + (int)blockIdx.y) * map_stride), m1{}, m2{} {}
    __device__ __forceinline__ void begin4(const Geom &g, int, int y, int x) { load_map4(map1, map2, (size_t)y * g.W + x, m1, m2); }
    __device__ __forceinline__ void begin1(const Geom &g, int, int y, int x)
    {
        const size_t i = (size_t)y * g.W + x;
        m1[0] = map1[i]; m2[0] = map2[i];
    }
    template <class F> __device__ __forceinline__ void each4(const uint8_t *frames, const Geom &g, int s, int, int, F &&use) const
    {
        const uint8_t *frame = frames + (size_t)s * g.H * g.W * CH;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t v[CH];
            remap_px<CH>(frame, g.H, g.W, m1[k], m2[k], v);
            use(k, v);
        }
    }
    __device__ __forceinline__ void four(const uint8_t *frames, const Geom &g, int s, int y, int x, unsigned (&f)[CH]) const
    {
        const uint8_t *frame = frames + (size_t)s * g.H * g.W * CH;
        unsigned px[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t v[CH];
            remap_px<CH>(frame, g.H, g.W, m1[k], m2[k], v);
            if constexpr (CH == 1) px[k] = v[0];
            else px[k] = v[0] | v[1] << 8 | v[2] << 16;
        }
        if constexpr (CH == 1) f[0] = px[0] | px[1] << 8 | px[2] << 16 | px[3] << 24;
        else pack_bgr4(px, f);
    }
    __device__ __forceinline__ void one(const uint8_t *frames, const Geom &g, int s, int, int, int (&v)[CH]) const
    {
        uint32_t u[CH];
        remap_px<CH>(frames + (size_t)s * g.H * g.W * CH, g.H, g.W, m1[0], m2[0], u);
#pragma unroll
        for (int c = 0; c < CH; ++c) v[c] = (int)u[c];
    }
};

}  // namespace oatgpu
