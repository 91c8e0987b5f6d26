// pixel_rules_inline.h -- the reference's per-pixel rules that more than one kernel applies, each written once: the single-stage
// component kernels (kernels_stages.hip) and the front kernels of the two batched trackers (kernels_diff.hip,
// kernels_bsubtrack.hip) must produce the same value for the same pixel, bit for bit.
#pragma once

#include "oatgpu_internal.h"

namespace oatgpu {

// COLOR_BGR2GRAY on 8U: RGB2Gray<uchar>'s table sums (ColorConvert.cpp:104, Threshold.cpp:67-81); at most 255 for bytes
__device__ __forceinline__ unsigned grey_bgr(unsigned b, unsigned g, unsigned r)
{
    return (1868u * b + 9617u * g + 4899u * r + (1u << 13)) >> 14;
}

// framefilt bsub, one channel of one pixel (BackgroundSubtractor.cpp:79-100): the state moves on, the saturated difference comes
// back.  First frame -> background; LEARN: cv::accumulateWeighted in fp32 (x*a + acc*b in separate roundings, a = (float)alpha,
// b = 1 - a: the units are built with -ffp-contract=off) and convertTo(CV_8U) (round half even, saturate); then x - bg, saturating.
template <bool LEARN> __device__ __forceinline__ int bsub_elem(int x, bool first, int &bg, float &acc, float a, float b)
{
    if (first) { acc = (float)x; bg = x; }
    if (LEARN) {
        acc = x * a + acc * b;
        bg = min(255, max(0, __float2int_rn(acc)));
    }
    return x > bg ? x - bg : 0;
}

// posidet diff, one GREY pixel (DifferenceDetector.cpp:156-171): cv::absdiff + cv::threshold(THRESH_BINARY) against the previous
// frame's pixel; on the first frame (threshold_frame_ = frame.clone()) the pixel itself.  The caller stores v as the new `last`.
__device__ __forceinline__ bool differs(int a, int b, int thr) { return (a > b ? a - b : b - a) > thr; }
__device__ __forceinline__ bool motion_bit(int v, int last, bool have, int thr) { return have ? differs(v, last, thr) : v != 0; }

}  // namespace oatgpu
