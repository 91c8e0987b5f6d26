// undistort_inline.h -- the per-pixel arithmetic of `framefilt undistort`'s remap (INTER_LINEAR, BORDER_CONSTANT 0, OpenCV's fixed
// point: dst = (sum S * BilinearTab_i + 16384) >> 15 == (sum S * p + 512) >> 10 with p = w / 32), shared by the stand-alone
// remap (kernels_undistort.hip) and the front kernels of the motion and the subtraction tracker, which remap their pixels in
// registers (kernels_diff.hip, kernels_bsubtrack.hip).  One definition: the fused kernels are bit-identical to the
// stand-alone remap by construction.
//
// A stream's map is two planes indexed by the OUTPUT pixel's raster position: map1 one u32 (sx | sy << 16, signed shorts), map2
// one u16 (fy * 32 + fx, 1/32 px).  Corner pairs (sx, sx + 1) are read as one unaligned dword + ushort (BGR) or one ushort (GREY)
// per source row when all four corners are inside the frame -- sx < W - 1 and sy < H - 1, so the 6 (2) bytes of either row end
// inside the frame; border pixels read each corner that is inside byte by byte and take 0 for the others.
#pragma once
#include "oatgpu_internal.h"

namespace oatgpu {

struct __attribute__((packed)) ua_u32 { uint32_t v; };
struct __attribute__((packed)) ua_u16 { uint16_t v; };

__device__ __forceinline__ uint32_t ld_u32(const uint8_t *p) { return ((const ua_u32 *)p)->v; }
__device__ __forceinline__ uint32_t ld_u16(const uint8_t *p) { return ((const ua_u16 *)p)->v; }

// one output pixel of an H x W frame of CH interleaved channels from the source corner (sx, sy) and the fractions (fx, fy) in
// 1/32 px, 0..31: the rule itself, for remap_px below and for k_target_crops (kernels_crops.hip), whose windows compute their
// own source positions
template <int CH>
__device__ __forceinline__ void remap_core(const uint8_t *__restrict__ src, int H, int W, int sx, int sy, int fx, int fy, uint32_t out[CH])
{
    const int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;   // BilinearTab_i / 32
    uint32_t s00[CH], s01[CH], s10[CH], s11[CH];
    if ((unsigned)sx < (unsigned)(W - 1) && (unsigned)sy < (unsigned)(H - 1)) {
        const uint8_t *r0 = src + ((size_t)sy * W + sx) * CH, *r1 = r0 + (size_t)W * CH;
        if constexpr (CH == 3) {
            const uint32_t a0 = ld_u32(r0), b0 = ld_u16(r0 + 4), a1 = ld_u32(r1), b1 = ld_u16(r1 + 4);
            s00[0] = a0 & 255; s00[1] = (a0 >> 8) & 255; s00[2] = (a0 >> 16) & 255;
            s01[0] = a0 >> 24; s01[1] = b0 & 255;        s01[2] = b0 >> 8;
            s10[0] = a1 & 255; s10[1] = (a1 >> 8) & 255; s10[2] = (a1 >> 16) & 255;
            s11[0] = a1 >> 24; s11[1] = b1 & 255;        s11[2] = b1 >> 8;
        } else {
            const uint32_t a0 = ld_u16(r0), a1 = ld_u16(r1);
            s00[0] = a0 & 255; s01[0] = a0 >> 8; s10[0] = a1 & 255; s11[0] = a1 >> 8;
        }
    } else if (sx >= W || sx + 1 < 0 || sy >= H || sy + 1 < 0) {
        for (int c = 0; c < CH; ++c) out[c] = 0;
        return;
    } else {
        const bool x0 = sx >= 0, x1 = sx + 1 < W, y0 = sy >= 0, y1 = sy + 1 < H;
        for (int c = 0; c < CH; ++c) {
            s00[c] = (x0 && y0) ? src[((size_t)sy * W + sx) * CH + c] : 0;
            s01[c] = (x1 && y0) ? src[((size_t)sy * W + sx + 1) * CH + c] : 0;
            s10[c] = (x0 && y1) ? src[((size_t)(sy + 1) * W + sx) * CH + c] : 0;
            s11[c] = (x1 && y1) ? src[((size_t)(sy + 1) * W + sx + 1) * CH + c] : 0;
        }
    }
    for (int c = 0; c < CH; ++c)
        out[c] = (s00[c] * w00 + s01[c] * w01 + s10[c] * w10 + s11[c] * w11 + 512u) >> 10;
}

// ... from its map entry (m1, m2)
template <int CH>
__device__ __forceinline__ void remap_px(const uint8_t *__restrict__ src, int H, int W, uint32_t m1, uint32_t m2, uint32_t out[CH])
{
    remap_core<CH>(src, H, W, (int)(int16_t)(m1 & 0xffffu), (int)(int16_t)(m1 >> 16), (int)(m2 & 31u), (int)((m2 >> 5) & 31u), out);
}

// The map entries of the 4 output pixels from raster position i on: one 16-byte and one 8-byte load.  i % 4 == 0; the planes
// are padded to a multiple of kMapAlign entries a stream (undistort_map_stride), so the loads are aligned and end inside the
// stream's padded plane even when fewer than 4 pixels of the frame are left.
__device__ __forceinline__ void load_map4(const uint32_t *__restrict__ map1, const uint16_t *__restrict__ map2, size_t i,
                                          uint32_t (&m1v)[4], uint32_t (&m2v)[4])
{
    const uint4 m1 = *(const uint4 *)(map1 + i);
    const uint2 m2 = *(const uint2 *)(map2 + i);
    m1v[0] = m1.x; m1v[1] = m1.y; m1v[2] = m1.z; m1v[3] = m1.w;
    m2v[0] = m2.x & 0xffffu; m2v[1] = m2.x >> 16; m2v[2] = m2.y & 0xffffu; m2v[3] = m2.y >> 16;
}

}  // namespace oatgpu
