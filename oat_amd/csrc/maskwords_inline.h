// maskwords_inline.h -- which pixels of the padded index space a lane owns and how a wave's mask words leave it, shared by the
// kernels that write a bit plane with 256 threads a workgroup and blockIdx.x along the plane: one pixel a lane (kernels_stages.hip,
// the narrow front kernels) or 4 consecutive pixels of a row a lane (the wide front kernels; kernels_diff.hip, kernels_bsubtrack.hip).
#pragma once

#include "oatgpu_internal.h"

namespace oatgpu {

// one wave = one mask word: pixel p = y * Wp + x of word `word` is this lane's; inside(): it is a pixel of the frame
struct WordLane {
    int lane, word, p, y, x;
    // the wave's word alone, for a kernel that leaves before anything else when its grid may overshoot the plane
    static __device__ __forceinline__ int this_word() { return blockIdx.x * 4 + (threadIdx.x >> 6); }
    __device__ __forceinline__ explicit WordLane(const Geom &g)
        : lane(threadIdx.x & 63), word(this_word()), p(word * 64 + lane), y(p / g.Wp), x(p - y * g.Wp) {}
    __device__ __forceinline__ bool inside(const Geom &g) const { return p < g.P && x < g.W; }
};

// the wave's word out of every lane's bit: lane 0 stores it as words[index]
__device__ __forceinline__ void store_word(bool on, int lane, u64 *words, size_t index)
{
    const u64 w = __ballot(on);
    if (lane == 0) words[index] = w;
}

// four pixels a lane: p0 .. p0 + 3 from (y, x) on, of words 4 * wave .. 4 * wave + 3 (Palloc % 1024 == 0); W % 4 == 0: inside together
struct QuadLane {
    int lane, wave, p0, y, x;
    __device__ __forceinline__ explicit QuadLane(const Geom &g)
        : lane(threadIdx.x & 63), wave(blockIdx.x * 4 + (threadIdx.x >> 6)), p0(wave * 256 + lane * 4), y(p0 / g.Wp), x(p0 - y * g.Wp) {}
    __device__ __forceinline__ bool inside(const Geom &g) const { return p0 < g.P && x < g.W; }
    // the 4 pixels' bits of a stream's bit plane (bit k = pixel k of the lane)
    __device__ __forceinline__ unsigned nibble(const u64 *plane) const { return (((const uint8_t *)plane)[p0 >> 3] >> (p0 & 4)) & 15u; }
};

// bits 0..15 of x to bits 0, 4, 8, .. 60
__device__ __forceinline__ u64 spread4(u64 x)
{
    x = (x | x << 24) & 0x000000ff000000ffull;
    x = (x | x << 12) & 0x000f000f000f000full;
    x = (x | x << 6) & 0x0303030303030303ull;
    x = (x | x << 3) & 0x1111111111111111ull;
    return x;
}

// the wave's 4 mask words out of every lane's nibble (bit k = pixel k of the lane): lane w < 4 stores word w
__device__ __forceinline__ void store_words(unsigned nib, int lane, u64 *dst)
{
    const u64 b0 = __ballot(nib & 1u), b1 = __ballot(nib & 2u), b2 = __ballot(nib & 4u), b3 = __ballot(nib & 8u);
    if (lane < 4) {
        const int sh = lane * 16;
        dst[lane] = spread4((b0 >> sh) & 0xffffull) | spread4((b1 >> sh) & 0xffffull) << 1 | spread4((b2 >> sh) & 0xffffull) << 2 |
                    spread4((b3 >> sh) & 0xffffull) << 3;
    }
}

}  // namespace oatgpu
