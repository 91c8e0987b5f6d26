// crops_inline.h -- the crop kernel: ONE definition of a window, of its two pixel rules and of the lane mapping for both kernels
// that cut windows out of frames -- k_target_crops (kernels_crops.hip: bytes into a crop set that may be host-mapped memory,
// DESIGN.md 9l) and k_crop_tensor (kernels_croptensor.hip: bytes, halves or floats into the caller's device memory).
// A third kernel takes the window and nothing of the pixels: k_target_mask (kernels_targetmask.hip) writes, for the
// crop tensor's window, which source pixels are the rank's own blob.
// The text in include/oatgpu.h ("target crops", "crop tensors", "target masks") is the contract.
//
// The body is one kernel template, k_crop_windows<CH, OUT>, and the two kernels are its instantiations by OUT: the rules are
// written once, and what differs -- the zoom of a rank's window, the conversion, the stores -- stands under `if constexpr`.  Helper
// functions were tried first and dropped: however they were cut (by value, by reference, with the LDS inside or outside), hipcc
// ordered k_target_crops' instructions differently from the kernel it was; this form compiles OUT = kCropOutBytes to the very
// listing k_target_crops had, but for the symbol's name and the compilation unit's id.
//
// Grid: (row block, window, stream); a lane takes 4 output pixels of one row, w / 4 lanes a row, blockDim.x / (w / 4) rows a
//   workgroup.  The window's record -- 4 + 6 words of TargetRec and ShapeRec, or the 5 words of a CropWin -- may live in
//   host-mapped memory, where every dependent read is a round trip over the link (profiles/shapes_bench.txt): it is fetched once a
//   workgroup, one lane a word, and lane 0 derives the window from the words in LDS with centroid_of / shape_of
//   (posfilt_inline.h), the very functions the host hands positions and shapes out with.
// Upright: a copy with unaligned source rows -- 4 pixels are one (GREY) or three (BGR) unaligned dword loads where they lie inside
//   the frame, byte loads with 0 for what lies outside otherwise.  Axis: a gather, fp64 source position per pixel (one rounding per
//   operation: the units are built with -ffp-contract=off), then remap_core (undistort_inline.h): `framefilt undistort`'s fixed-point
//   bilinear rule with BORDER_CONSTANT 0.
// Stores, consecutive lanes consecutive addresses, every element of every window by every launch (an invalid window is zeros, or
//   bias[c] behind the conversion):
//   kCropOutBytes  32-bit, one to three a lane (nothing wider than 64 bits; the crop set may be host-mapped memory)
//   kCropOutU8     the same dwords, plain stores into device memory
//   kCropOutF16    planar, one 64-bit store a channel;  kCropOutF32  planar, two 64-bit stores a channel
//   kCropOutMask + one of the three: one plane [h][w], the same stores -- one dword, one 64-bit store, two 64-bit stores a lane
// Target masks (OUT >= kCropOutMask; CH = 1): the pixel fetch is replaced.  The source pixel of an element is where the copy reads,
//   or the pixel nearest to where the gather samples -- ((qx + 16) >> 5, (qy + 16) >> 5) --; the element is ON where that pixel lies
//   inside the frame, its bit of the final mask `fin` is set, and the root of its run is the rank's (the padded index of
//   TargetRec.first_pixel, as k_blob_shape forms it).  Only a set bit costs lookups: run_head, then uf_root (blobruns_inline.h),
//   the last (head -> root) pair kept across the lane's four pixels -- consecutive pixels of a row mostly share a run.  Plain loads:
//   what is read is final from the end of k_merge to the set's next row scan (kernels_blob.hip, k_blob_shape's comment).
#pragma once
#include "oatgpu_internal.h"
#include "posfilt_inline.h"
#include "blobruns_inline.h"
#include "undistort_inline.h"

namespace oatgpu {

constexpr int kCropBlock = 256;
static_assert(sizeof(TargetRec) == 32 && sizeof(ShapeRec) == 48 && sizeof(CropWin) == 40, "the record words the crop kernel fetches");
static_assert(kCropMaxSide / 4 <= 64, "a row's lanes fit the smallest workgroup");

// Between two plain stores to neighbouring addresses: hipcc fuses them into one store of 96 or 128 bits otherwise, and DESIGN.md 3b
// keeps this library's stores at 64 bits unless they are padded.  No instruction; the compiler only may not move stores across it.
__device__ __forceinline__ void crop_keep_stores_apart() { asm volatile("" ::: "memory"); }

// what a launch takes by OUT: k_target_crops its CropLaunch as it always did, k_crop_tensor the CropTensorLaunch around it
// ... and k_target_mask the MaskTensorLaunch around that
template <int OUT> struct CropLaunchOf { typedef std::conditional_t<(OUT >= kCropOutMask), MaskTensorLaunch, CropTensorLaunch> type; };
template <> struct CropLaunchOf<kCropOutBytes> { typedef CropLaunch type; };

template <int CH, int OUT>
__global__ __launch_bounds__(kCropBlock) void k_crop_windows(int H, int W, typename CropLaunchOf<OUT>::type a)
{
    __shared__ u64 word[10];
    __shared__ CropWin win;
    const size_t at = (size_t)blockIdx.z * a.k + blockIdx.y;       // the window: stream blockIdx.z, rank blockIdx.y
    const unsigned t = threadIdx.x;
    if (a.recs) {
        if (t < 4) word[t] = reinterpret_cast<const u64 *>(a.recs + at)[t];
        else if (t < 10) word[t] = a.shp ? reinterpret_cast<const u64 *>(a.shp + at)[t - 4] : 0ull;
    } else if (t < 5) {
        word[t] = reinterpret_cast<const u64 *>(a.win + at)[t];
    }
    __syncthreads();
    if (t == 0) {
        CropWin v{};
        if (a.recs) {
            ResultRec r{};
            r.a00 = (long long)word[0]; r.a10 = (long long)word[1]; r.a01 = (long long)word[2];
            r.valid = (int)(word[3] >> 32) != 0;
            v.valid = centroid_of(r, v.cx, v.cy) ? 1 : 0;
            v.upright = 1;
            if (v.valid && a.axis && (unsigned)word[9] != 0u) {
                ShapeDerived d;
                shape_of(r.a00, r.a10, r.a01, (long long)word[4], (long long)word[5], (long long)word[6], d);
                if (d.axis_valid) { v.upright = 0; v.ax = d.axis_x; v.ay = d.axis_y; }
            }
            if constexpr (OUT != kCropOutBytes) {
                // zoom, source pixels an output pixel: 1.0 leaves the window as it is -- the copy where the rank is upright; any
                // other value makes it a gather along the zoomed axis, one fp64 multiply a component, used as given
                if (a.zoom != 1.0) {
                    if (v.upright) { v.ax = a.zoom; v.ay = 0.0; }
                    else { v.ax = a.zoom * v.ax; v.ay = a.zoom * v.ay; }
                    v.upright = 0;
                }
            }
        } else {
            v.valid = (unsigned)word[0] != 0u;
            v.upright = (unsigned)(word[0] >> 32) != 0u;
            v.cx = __longlong_as_double((long long)word[1]); v.cy = __longlong_as_double((long long)word[2]);
            v.ax = __longlong_as_double((long long)word[3]); v.ay = __longlong_as_double((long long)word[4]);
        }
        // a centre or an axis that is not finite, or a centre beyond +-1e6: no window (the comparisons are false for a NaN)
        if (!(fabs(v.cx) <= 1e6 && fabs(v.cy) <= 1e6 && fabs(v.ax) <= DBL_MAX && fabs(v.ay) <= DBL_MAX)) v.valid = 0;
        win = v;
    }
    __syncthreads();

    const int lpr = a.w >> 2, rows_wg = (int)blockDim.x / lpr;
    const int ri = (int)t / lpr, i = (int)blockIdx.x * rows_wg + ri, j0 = ((int)t - ri * lpr) * 4;
    if (ri >= rows_wg || i >= a.h) return;

    uint32_t px[4][CH];
#pragma unroll
    for (int q = 0; q < 4; ++q)
        for (int c = 0; c < CH; ++c) px[q][c] = 0u;
    if constexpr (OUT < kCropOutMask) {
        const uint8_t *src = a.frames + (size_t)blockIdx.z * H * W * CH;
        if (win.valid && win.upright) {
            const int x = (int)rint(win.cx) - a.w / 2 + j0, y = (int)rint(win.cy) - a.h / 2 + i;
            if ((unsigned)y < (unsigned)H) {
                const uint8_t *p = src + ((ptrdiff_t)y * W + x) * CH;
                if (x >= 0 && x + 3 < W) {
                    uint32_t w[CH];
#pragma unroll
                    for (int c = 0; c < CH; ++c) w[c] = ld_u32(p + 4 * c);
#pragma unroll
                    for (int b = 0; b < 4 * CH; ++b) px[b / CH][b % CH] = (w[b >> 2] >> ((b & 3) * 8)) & 255u;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if ((unsigned)(x + q) < (unsigned)W)
                            for (int c = 0; c < CH; ++c) px[q][c] = p[q * CH + c];
                }
            }
        } else if (win.valid) {
            const double cx = win.cx, cy = win.cy, ax = win.ax, ay = win.ay;
            const double v = (double)(i - a.h / 2);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double u = (double)(j0 + q - a.w / 2);
                const double X = (cx + u * ax) - v * ay, Y = (cy + u * ay) + v * ax;
                const double qxd = rint(X * 32.0), qyd = rint(Y * 32.0);
                // (a position that is not finite or beyond 2^25 pixels lies outside every frame; the comparison is false for a NaN)
                if (fabs(qxd) < 1073741824.0 && fabs(qyd) < 1073741824.0) {
                    const int qx = (int)qxd, qy = (int)qyd;
                    remap_core<CH>(src, H, W, qx >> 5, qy >> 5, qx & 31, qy & 31, px[q]);
                }
            }
        }
    } else {
        // a target mask: px[q][0] = 1 where the element's source pixel is the rank's own
        static_assert(CH == 1, "a mask has no channel axis");
        if (win.valid) {
            const Geom &g = a.g;
            const size_t soff = (size_t)blockIdx.z * (g.Palloc >> 6);
            const u64 *fin = a.b.fin + soff, *trans = a.b.trans + soff;
            const int *carry = a.b.carry + (size_t)blockIdx.z * g.H * g.words;
            const int *parent = a.b.parent + (size_t)blockIdx.z * g.Palloc;
            const int fp = (int)(unsigned)word[3], fy = fp / W;            // TargetRec.first_pixel -> the rank's root, a padded index
            const int root_j = fy * g.Wp + (fp - fy * W);
            const double cx = win.cx, cy = win.cy, ax = win.ax, ay = win.ay;
            const double v = (double)(i - a.h / 2);
            int m_head = -1, m_root = -1;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                int x = -1, y = -1;
                if (win.upright) {
                    x = (int)rint(cx) - a.w / 2 + j0 + q; y = (int)rint(cy) - a.h / 2 + i;
                } else {
                    const double u = (double)(j0 + q - a.w / 2);
                    const double X = (cx + u * ax) - v * ay, Y = (cy + u * ay) + v * ax;
                    const double qxd = rint(X * 32.0), qyd = rint(Y * 32.0);
                    if (fabs(qxd) < 1073741824.0 && fabs(qyd) < 1073741824.0) {      // (as the gather: outside every frame otherwise)
                        x = ((int)qxd + 16) >> 5; y = ((int)qyd + 16) >> 5;
                    }
                }
                if ((unsigned)x < (unsigned)W && (unsigned)y < (unsigned)H &&
                    ((fin[(size_t)y * g.words + (x >> 6)] >> (x & 63)) & 1ull) != 0ull) {
                    const int head = run_head(g, trans, carry, y, x);
                    if (head != m_head) { m_head = head; m_root = uf_root(parent, head); }
                    px[q][0] = m_root == root_j ? 1u : 0u;
                }
            }
        }
    }
    if constexpr (OUT == kCropOutBytes) {
        uint32_t w[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) w[c] = 0u;
#pragma unroll
        for (int b = 0; b < 4 * CH; ++b) w[b >> 2] |= px[b / CH][b % CH] << ((b & 3) * 8);
        uint32_t *o = reinterpret_cast<uint32_t *>(a.out + ((at * a.h + i) * a.w + j0) * CH);
#pragma unroll
        for (int c = 0; c < CH; ++c) __hip_atomic_store(o + c, w[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if constexpr (OUT == kCropOutU8) {
        // the same bytes, [h][w][CH], into device memory: plain stores
        uint32_t w[CH];
#pragma unroll
        for (int c = 0; c < CH; ++c) w[c] = 0u;
#pragma unroll
        for (int b = 0; b < 4 * CH; ++b) w[b >> 2] |= px[b / CH][b % CH] << ((b & 3) * 8);
        uint32_t *o = reinterpret_cast<uint32_t *>(a.out + ((at * a.h + i) * a.w + j0) * CH);
#pragma unroll
        for (int c = 0; c < CH; ++c) { o[c] = w[c]; crop_keep_stores_apart(); }
    } else if constexpr (OUT >= kCropOutMask) {
        // a mask plane [h][w]: ON / OFF are 255 / 0 in bytes, 1.0 / 0.0 in halves and floats
        const size_t e = (at * a.h + i) * a.w + j0;
        if constexpr (OUT == kCropOutMask + kCropOutU8) {
            *reinterpret_cast<uint32_t *>(a.out + e) = (px[0][0] | px[1][0] << 8 | px[2][0] << 16 | px[3][0] << 24) * 255u;
        } else if constexpr (OUT == kCropOutMask + kCropOutF16) {
            *reinterpret_cast<uint2 *>(reinterpret_cast<unsigned short *>(a.out) + e) =
                make_uint2((px[0][0] | px[1][0] << 16) * 0x3c00u, (px[2][0] | px[3][0] << 16) * 0x3c00u);
        } else {
            static_assert(OUT == kCropOutMask + kCropOutF32, "the three tensor dtypes");
            float2 *o = reinterpret_cast<float2 *>(reinterpret_cast<float *>(a.out) + e);
            o[0] = make_float2((float)px[0][0], (float)px[1][0]);
            crop_keep_stores_apart();
            o[1] = make_float2((float)px[2][0], (float)px[3][0]);
        }
    } else {
        // planar [CH][h][w]: fl32(fl32((float)p * scale[c]) + bias[c]), two roundings (__fmul_rn / __fadd_rn never contract), then
        // to nearest even to half for kCropOutF16; 4 values a lane a channel: one 64-bit store of halves, two of floats
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            float f[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) f[q] = __fadd_rn(__fmul_rn((float)px[q][c], a.scale[c]), a.bias[c]);
            const size_t e = ((at * CH + c) * a.h + i) * a.w + j0;
            if (c) crop_keep_stores_apart();
            if constexpr (OUT == kCropOutF16) {
                uint32_t hw[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) hw[q] = __builtin_bit_cast(unsigned short, (_Float16)f[q]);
                *reinterpret_cast<uint2 *>(reinterpret_cast<unsigned short *>(a.out) + e) = make_uint2(hw[0] | hw[1] << 16, hw[2] | hw[3] << 16);
            } else {
                float2 *o = reinterpret_cast<float2 *>(reinterpret_cast<float *>(a.out) + e);
                o[0] = make_float2(f[0], f[1]);
                crop_keep_stores_apart();
                o[1] = make_float2(f[2], f[3]);
            }
        }
    }
}

// the launch shape: workgroups over (row block, window, stream), w / 4 lanes a row, 64 threads where the whole window fits them
static inline void crop_grid(const CropLaunch &a, int n_streams, dim3 &grid, dim3 &block)
{
    const int lpr = a.w / 4;
    const int threads = a.h * lpr <= 64 ? 64 : kCropBlock, rows_wg = threads / lpr;
    grid = dim3((a.h + rows_wg - 1) / rows_wg, a.k, n_streams);
    block = dim3(threads);
}

}  // namespace oatgpu
