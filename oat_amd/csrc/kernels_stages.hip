// kernels_stages.hip -- the single-stage component kernels behind api_stages.hip: one Oat component on one frame a launch
// (`framefilt col`, `mask`, `bsub`, `thresh`, the front ends of `posidet hsv` / `thresh` / `diff`), the conversions between byte
// masks and bit planes, and the staging copy out of host memory.  None of them is on the fused hot path; the rules they share
// with the batched trackers' front kernels are in pixel_rules_inline.h, the lane mapping of the bit-plane writers in
// maskwords_inline.h.
#include "oatgpu_internal.h"
#include "hsv_inline.h"
#include "maskwords_inline.h"
#include "pixel_rules_inline.h"
#include <algorithm>

namespace oatgpu {

// One camera's frame out of page-locked HOST memory (a registered shared-memory segment: every load is a PCIe read) into
// its staging slot, by a kernel instead of a DMA copy (oatgpu_set_stage_copy): a launch costs the host ~5 us where a
// hipMemcpyAsync costs ~20 us of set-up per 6 MB frame.  A small grid -- the waves do nothing but wait for the link, and
// the per-pixel kernel wants the slots: 4 x 16 bytes in flight per lane, 128 workgroups = 2 MB in flight.
typedef unsigned nv4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_stage_copy(const nv4 *src, nv4 *dst, size_t n16, const uint8_t *src_tail, uint8_t *dst_tail, int tail)
{
    const size_t stride = (size_t)gridDim.x * 1024;
    for (size_t i = (size_t)blockIdx.x * 1024 + threadIdx.x; i < n16; i += stride) {
        nv4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) if (i + (size_t)u * 256 < n16) v[u] = __builtin_nontemporal_load(src + i + (size_t)u * 256);
#pragma unroll
        for (int u = 0; u < 4; ++u) if (i + (size_t)u * 256 < n16) __builtin_nontemporal_store(v[u], dst + i + (size_t)u * 256);
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < tail) dst_tail[threadIdx.x] = src_tail[threadIdx.x];
}
void launch_stage_copy(const void *src_dev_visible, void *dst, size_t bytes, hipStream_t st)
{
    const size_t n16 = bytes / 16;
    const int tail = (int)(bytes - n16 * 16);
    const unsigned blocks = (unsigned)std::min<size_t>(128, (n16 + 1023) / 1024 ? (n16 + 1023) / 1024 : 1);
    hipLaunchKernelGGL(k_stage_copy, dim3(blocks), dim3(256), 0, st, (const nv4 *)src_dev_visible, (nv4 *)dst, n16,
                       (const uint8_t *)src_dev_visible + n16 * 16, (uint8_t *)dst + n16 * 16, tail);
}

// framefilt col -C HSV: bgr2hsv_inline on every pixel, the arithmetic K1, the marker sets and the subtraction tracker use
__global__ __launch_bounds__(256) void k_bgr2hsv(const uint8_t *bgr, uint8_t *hsv, size_t npx)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += (size_t)gridDim.x * blockDim.x) {
        int h, s, v;
        bgr2hsv_inline(bgr[3 * i], bgr[3 * i + 1], bgr[3 * i + 2], h, s, v);
        hsv[3 * i] = (uint8_t)h; hsv[3 * i + 1] = (uint8_t)s; hsv[3 * i + 2] = (uint8_t)v;
    }
}

void launch_bgr2hsv(const uint8_t *bgr, uint8_t *hsv, size_t npx, hipStream_t st)
{
    hipLaunchKernelGGL(k_bgr2hsv, dim3(grid_stride_blocks(npx)), dim3(256), 0, st, bgr, hsv, npx);
}

// ---- the other entries of oat::color_conv_table (Color.h:45-51) behind ColorConvert::filter (ColorConvert.cpp:101-107) ----
// Four pixels a thread, every access a dword (4 px x 3 B = three dwords; 4 grey px = one); the last npx % 4 pixels
// are done byte-wise by the thread behind the last full group.

// COLOR_HSV2BGR on 8U, OpenCV 3.1.0: HSV2RGB_b over HSV2RGB_f(hrange 180) -- fp32, every operation rounded on its own
// (-ffp-contract=off), cvRound (nearest even) + saturation on the way out.  h <= 255 -> h * (6/180) < 8.5: the
// reference's "do h -= 6 while (h >= 6)" runs once at most and the sector is always one of 0..5.
__device__ __forceinline__ void hsv2bgr_px(unsigned hh, unsigned ss, unsigned vv, unsigned &b, unsigned &g, unsigned &r)
{
    float h = (float)hh;
    const float s = (float)ss * (1.f / 255.f), v = (float)vv * (1.f / 255.f);
    float fb, fg, fr;
    if (s == 0.f) fb = fg = fr = v;
    else {
        h *= 6.f / 180.f;
        if (h >= 6.f) h -= 6.f;
        const int sector = (int)floorf(h);
        h -= (float)sector;
        const float t0 = v, t1 = v * (1.f - s), t2 = v * (1.f - s * h), t3 = v * (1.f - s * (1.f - h));
        switch (sector) {                       // sector_data[][3] of HSV2RGB_f, (b, g, r)
        case 0:  fb = t1; fg = t3; fr = t0; break;
        case 1:  fb = t1; fg = t0; fr = t2; break;
        case 2:  fb = t3; fg = t0; fr = t1; break;
        case 3:  fb = t0; fg = t2; fr = t1; break;
        case 4:  fb = t0; fg = t1; fr = t3; break;
        default: fb = t2; fg = t1; fr = t0; break;
        }
    }
    b = (unsigned)min(max(__float2int_rn(fb * 255.f), 0), 255);
    g = (unsigned)min(max(__float2int_rn(fg * 255.f), 0), 255);
    r = (unsigned)min(max(__float2int_rn(fr * 255.f), 0), 255);
}

template <int kCode>   // 0: BGR -> GREY, 1: GREY -> BGR, 2: HSV -> BGR
__global__ __launch_bounds__(256) void k_cvt_color(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, size_t npx)
{
    const size_t groups = npx >> 2;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < groups) {
        if (kCode == 1) {
            const unsigned q = ((const unsigned *)in)[t];
            const unsigned p0 = q & 255u, p1 = (q >> 8) & 255u, p2 = (q >> 16) & 255u, p3 = q >> 24;
            unsigned *o = (unsigned *)out + 3 * t;
            o[0] = p0 * 0x010101u | p1 << 24;
            o[1] = p1 * 0x0101u | p2 * 0x01010000u;
            o[2] = p2 | p3 * 0x01010100u;
        } else {
            const unsigned *w = (const unsigned *)in + 3 * t;
            const unsigned w0 = w[0], w1 = w[1], w2 = w[2];
            // channel c of pixel k is byte 3k + c of the twelve
            const unsigned a0 = w0 & 255u, a1 = (w0 >> 8) & 255u, a2 = (w0 >> 16) & 255u;
            const unsigned b0 = w0 >> 24, b1 = w1 & 255u, b2 = (w1 >> 8) & 255u;
            const unsigned c0 = (w1 >> 16) & 255u, c1 = w1 >> 24, c2 = w2 & 255u;
            const unsigned d0 = (w2 >> 8) & 255u, d1 = (w2 >> 16) & 255u, d2 = w2 >> 24;
            if (kCode == 0) {
                ((unsigned *)out)[t] = grey_bgr(a0, a1, a2) | grey_bgr(b0, b1, b2) << 8 | grey_bgr(c0, c1, c2) << 16 |
                                       grey_bgr(d0, d1, d2) << 24;
            } else {
                unsigned pb[4], pg[4], pr[4];
                hsv2bgr_px(a0, a1, a2, pb[0], pg[0], pr[0]);
                hsv2bgr_px(b0, b1, b2, pb[1], pg[1], pr[1]);
                hsv2bgr_px(c0, c1, c2, pb[2], pg[2], pr[2]);
                hsv2bgr_px(d0, d1, d2, pb[3], pg[3], pr[3]);
                unsigned *o = (unsigned *)out + 3 * t;
                o[0] = pb[0] | pg[0] << 8 | pr[0] << 16 | pb[1] << 24;
                o[1] = pg[1] | pr[1] << 8 | pb[2] << 16 | pg[2] << 24;
                o[2] = pr[2] | pb[3] << 8 | pg[3] << 16 | pr[3] << 24;
            }
        }
    } else if (t == groups) {
        for (size_t i = groups << 2; i < npx; ++i) {
            if (kCode == 0) out[i] = (uint8_t)grey_bgr(in[3 * i], in[3 * i + 1], in[3 * i + 2]);
            else if (kCode == 1) out[3 * i] = out[3 * i + 1] = out[3 * i + 2] = in[i];
            else {
                unsigned b, g, r;
                hsv2bgr_px(in[3 * i], in[3 * i + 1], in[3 * i + 2], b, g, r);
                out[3 * i] = (uint8_t)b; out[3 * i + 1] = (uint8_t)g; out[3 * i + 2] = (uint8_t)r;
            }
        }
    }
}

void launch_cvt_color(int code, const uint8_t *in, uint8_t *out, size_t npx, hipStream_t st)
{
    const unsigned blocks = (unsigned)(((npx >> 2) + 1 + 255) / 256);
    if (code == 0) hipLaunchKernelGGL(k_cvt_color<0>, dim3(blocks), dim3(256), 0, st, in, out, npx);
    else if (code == 1) hipLaunchKernelGGL(k_cvt_color<1>, dim3(blocks), dim3(256), 0, st, in, out, npx);
    else hipLaunchKernelGGL(k_cvt_color<2>, dim3(blocks), dim3(256), 0, st, in, out, npx);
}

// one wave = one mask word (64 pixels of one row)
__global__ __launch_bounds__(256) void k_inrange_bits(Geom g, const uint8_t *frame, int channels, RangeParams rp, u64 *bits)
{
    if (WordLane::this_word() >= (g.Palloc >> 6)) return;
    const WordLane l(g);
    bool thr = false;
    if (l.inside(g)) {
        const size_t i = (size_t)l.y * g.W + l.x;
        if (channels == 3) thr = in_range3(frame[3 * i], frame[3 * i + 1], frame[3 * i + 2], rp);
        else { const int v = frame[i]; thr = v >= rp.lo[0] && v <= rp.hi[0]; }
    }
    store_word(thr, l.lane, bits, l.word);
}

void launch_inrange_bits(const Geom &g, const uint8_t *frame, int channels, const RangeParams &rp, u64 *bits, hipStream_t st)
{
    const int nwords = g.Palloc >> 6;
    hipLaunchKernelGGL(k_inrange_bits, dim3((nwords + 3) / 4), dim3(256), 0, st, g, frame, channels, rp, bits);
}

// framefilt bsub: bsub_elem on every byte (BackgroundSubtractor.cpp:87-100).  The state is stored on the first frame and
// whenever it learns; without LEARN the accumulator is not read.
template <bool LEARN>
__global__ __launch_bounds__(256) void k_bsub(const uint8_t *in, uint8_t *out, uint8_t *bg, float *bg_f, size_t n, float a, float b, int first)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float f = 0.f;
        int g = 0;
        if (!first) { if (LEARN) f = bg_f[i]; else g = bg[i]; }
        const int d = bsub_elem<LEARN>(in[i], first, g, f, a, b);
        if (first || LEARN) { bg_f[i] = f; bg[i] = (uint8_t)g; }
        out[i] = (uint8_t)d;
    }
}

void launch_bsub(const uint8_t *in, uint8_t *out, uint8_t *bg, float *bg_f, size_t n, float a, float b, int first, int learn, hipStream_t st)
{
    auto launch = [&](auto *k) { hipLaunchKernelGGL(k, dim3(grid_stride_blocks(n)), dim3(256), 0, st, in, out, bg, bg_f, n, a, b, first); };
    learn ? launch(k_bsub<true>) : launch(k_bsub<false>);
}

// framefilt mask: frame.setTo(0, roi_mask == 0) (FrameMasker.cpp:71-75) with the 1-bit ROI plane
__global__ __launch_bounds__(256) void k_apply_roi(Geom g, const uint8_t *in, uint8_t *out, int ch, const u64 *roi)
{
    const size_t npx = (size_t)g.H * g.W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += (size_t)gridDim.x * blockDim.x) {
        const int y = (int)(i / g.W), x = (int)(i - (size_t)y * g.W);
        const int p = y * g.Wp + x;
        const bool keep = (roi[p >> 6] >> (p & 63)) & 1ull;
        for (int c = 0; c < ch; ++c) out[i * ch + c] = keep ? in[i * ch + c] : 0;
    }
}
void launch_apply_roi(const Geom &g, const uint8_t *in, uint8_t *out, int channels, const u64 *roi, hipStream_t st)
{
    hipLaunchKernelGGL(k_apply_roi, dim3(grid_stride_blocks((size_t)g.H * g.W)), dim3(256), 0, st, g, in, out, channels, roi);
}

// framefilt thresh: grey_bgr (a byte: the same value in signed arithmetic), inRange, setTo(0)
__global__ __launch_bounds__(256) void k_thresh_filter(const uint8_t *in, uint8_t *out, size_t npx, int ch, int lo, int hi)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += (size_t)gridDim.x * blockDim.x) {
        if (ch == 3) {
            const int b = in[3 * i], g = in[3 * i + 1], r = in[3 * i + 2];
            const int y = (int)grey_bgr(b, g, r);
            const bool keep = y >= lo && y <= hi;
            out[3 * i] = keep ? b : 0; out[3 * i + 1] = keep ? g : 0; out[3 * i + 2] = keep ? r : 0;
        } else {
            const int y = in[i];
            out[i] = (y >= lo && y <= hi) ? y : 0;
        }
    }
}

void launch_thresh_filter(const uint8_t *in, uint8_t *out, size_t npx, int channels, int lo, int hi, hipStream_t st)
{
    hipLaunchKernelGGL(k_thresh_filter, dim3(grid_stride_blocks(npx)), dim3(256), 0, st, in, out, npx, channels, lo, hi);
}

// posidet diff: motion_bit of a GREY frame against the previous one (DifferenceDetector.cpp:156-161), one wave = one mask
// word; also refreshes the previous frame.
__global__ __launch_bounds__(256) void k_absdiff_bits(Geom g, const uint8_t *frame, uint8_t *last, int thr, int have_last, u64 *bits)
{
    if (WordLane::this_word() >= (g.Palloc >> 6)) return;
    const WordLane l(g);
    bool on = false;
    if (l.inside(g)) {
        const size_t i = (size_t)l.y * g.W + l.x;
        const int v = frame[i];
        on = motion_bit(v, have_last ? last[i] : 0, have_last, thr);
        last[i] = (uint8_t)v;
    }
    store_word(on, l.lane, bits, l.word);
}

void launch_absdiff_bits(const Geom &g, const uint8_t *frame, uint8_t *last, int thr, int have_last, u64 *bits, hipStream_t st)
{
    const int nwords = g.Palloc >> 6;
    hipLaunchKernelGGL(k_absdiff_bits, dim3((nwords + 3) / 4), dim3(256), 0, st, g, frame, last, thr, have_last, bits);
}

__global__ __launch_bounds__(256) void k_unpack_bits(Geom g, const u64 *bits, uint8_t *out)
{
    const size_t npx = (size_t)g.H * g.W;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += (size_t)gridDim.x * blockDim.x) {
        const int y = (int)(i / g.W), x = (int)(i - (size_t)y * g.W);
        const int p = y * g.Wp + x;
        out[i] = ((bits[p >> 6] >> (p & 63)) & 1ull) ? 255 : 0;
    }
}

void launch_pack_bits(const Geom &g, const uint8_t *in, u64 *bits, hipStream_t st)
{
    RangeParams rp;
    rp.lo[0] = 1; rp.hi[0] = 255; rp.lo[1] = rp.lo[2] = 0; rp.hi[1] = rp.hi[2] = 255;
    launch_inrange_bits(g, in, 1, rp, bits, st);     // nonzero == in [1,255]
}

void launch_unpack_bits(const Geom &g, const u64 *bits, uint8_t *out, hipStream_t st)
{
    hipLaunchKernelGGL(k_unpack_bits, dim3(grid_stride_blocks((size_t)g.H * g.W)), dim3(256), 0, st, g, bits, out);
}

}  // namespace oatgpu
