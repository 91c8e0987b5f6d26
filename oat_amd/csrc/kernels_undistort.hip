// kernels_undistort.hip -- `framefilt undistort` (src/framefilter/Undistorter.cpp:83-88: cv::undistort(temp, frame, K, D)).
//
// Two halves:
//   undistort_build_map   host code, run once per configuration: OpenCV 3.1's cv::undistort map, stripe by stripe
//                         (initUndistortRectifyMap with CV_16SC2 into map1 = (sx, sy) shorts and map2 = 1/32-px fractions).
//                         cv::undistort rebuilds the same map on every frame; here it is built once and kept on the device.
//   k_undistort           the per-frame remap (INTER_LINEAR, BORDER_CONSTANT 0) of 8-bit frames in OpenCV's fixed point:
//                         dst = (sum S * BilinearTab_i + 16384) >> 15 == (sum S * p + 512) >> 10 with p = w / 32.
// -ffp-contract=off (Makefile HIPFLAGS) is a parity requirement of the map builder: a contracted FMA moves u, v and flips
// 1/32-px cells.
#include "oatgpu_internal.h"
#include "undistort_inline.h"

#include <algorithm>
#include <climits>
#include <cmath>

namespace oatgpu {

// ------------------------------------------------------------------------------------------------ map (host, double) ---

// cvRound on x86-64 (SSE2 cvtsd2si): round half to even; NaN or a result outside int gives INT_MIN ("integer indefinite")
static inline int cv_round(double v)
{
    const double r = std::nearbyint(v);
    if (!(r >= -2147483648.0 && r <= 2147483647.0)) return INT_MIN;
    return (int)r;
}

int undistort_check_coeffs(int n_dist, const char **why)
{
    // Undistorter.cpp:61-62; OpenCV 3.1's initUndistortRectifyMap asserts on every count but 4, 5, 8, 12 (and 14 later)
    if (n_dist < 5 || n_dist > 8) { *why = "Distortion coefficients consist of 5 to 8 values."; return -1; }
    if (n_dist == 6 || n_dist == 7) {
        *why = "Distortion coefficients: 6 or 7 values pass the reference's check, but cv::undistort (OpenCV 3.1) accepts "
               "only 4, 5, 8 or 12 and the reference fails at its first frame; give 5 or 8.";
        return -1;
    }
    return 0;
}

// cv::invert(DECOMP_LU), its closed-form 3x3 path: det3, d = 1/d, the adjugate product by product; singular -> zeros
static void inv3_lu(const double m[9], double t[9])
{
#define M(i, j) m[(i) * 3 + (j)]
    double d = M(0, 0) * (M(1, 1) * M(2, 2) - M(1, 2) * M(2, 1)) -
               M(0, 1) * (M(1, 0) * M(2, 2) - M(1, 2) * M(2, 0)) +
               M(0, 2) * (M(1, 0) * M(2, 1) - M(1, 1) * M(2, 0));
    if (d == 0.0) { for (int i = 0; i < 9; ++i) t[i] = 0.0; return; }
    d = 1. / d;
    t[0] = (M(1, 1) * M(2, 2) - M(1, 2) * M(2, 1)) * d;
    t[1] = (M(0, 2) * M(2, 1) - M(0, 1) * M(2, 2)) * d;
    t[2] = (M(0, 1) * M(1, 2) - M(0, 2) * M(1, 1)) * d;
    t[3] = (M(1, 2) * M(2, 0) - M(1, 0) * M(2, 2)) * d;
    t[4] = (M(0, 0) * M(2, 2) - M(0, 2) * M(2, 0)) * d;
    t[5] = (M(0, 2) * M(1, 0) - M(0, 0) * M(1, 2)) * d;
    t[6] = (M(1, 0) * M(2, 1) - M(1, 1) * M(2, 0)) * d;
    t[7] = (M(0, 1) * M(2, 0) - M(0, 0) * M(2, 1)) * d;
    t[8] = (M(0, 0) * M(1, 1) - M(0, 1) * M(1, 0)) * d;
#undef M
}

void undistort_build_map(int rows, int cols, const double K[9], const double *dist, int n_dist, int16_t *map1, uint16_t *map2)
{
    // cv::undistort: stripes of min(max(1, 4096 / cols), rows) rows, Ar = K with Ar(1,2) = K(1,2) - y, no new camera matrix
    const int stripe0 = std::min(std::max(1, 4096 / std::max(cols, 1)), rows);
    const double k1 = dist[0], k2 = dist[1], p1 = dist[2], p2 = dist[3], k3 = dist[4];
    const double k4 = n_dist >= 8 ? dist[5] : 0., k5 = n_dist >= 8 ? dist[6] : 0., k6 = n_dist >= 8 ? dist[7] : 0.;
    const double u0 = K[2], v0 = K[5], fx = K[0], fy = K[4];     // initUndistortRectifyMap: from A, not from Ar
    double Ar[9];
    for (int i = 0; i < 9; ++i) Ar[i] = K[i];                    // Ar * I == Ar
    for (int y = 0; y < rows; y += stripe0) {
        const int stripe = std::min(stripe0, rows - y);
        Ar[5] = K[5] - y;
        double ir[9];
        inv3_lu(Ar, ir);
        for (int i = 0; i < stripe; ++i) {
            int16_t *m1 = map1 + (size_t)(y + i) * cols * 2;
            uint16_t *m2 = map2 + (size_t)(y + i) * cols;
            double _x = i * ir[1] + ir[2], _y = i * ir[4] + ir[5], _w = i * ir[7] + ir[8];
            // the column loop accumulates: _x0 + j * ir[0] differs in the last bits
            for (int j = 0; j < cols; j++, _x += ir[0], _y += ir[3], _w += ir[6]) {
                const double w = 1. / _w, x = _x * w, yy = _y * w;
                const double x2 = x * x, y2 = yy * yy;
                const double r2 = x2 + y2, _2xy = 2 * x * yy;
                const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
                const double u = fx * (x * kr + p1 * _2xy + p2 * (r2 + 2 * x2)) + u0;
                const double v = fy * (yy * kr + p1 * (r2 + 2 * y2) + p2 * _2xy) + v0;
                const int iu = cv_round(u * 32), iv = cv_round(v * 32);          // INTER_TAB_SIZE
                m1[j * 2] = (int16_t)(iu >> 5);                                   // (short): truncates, wraps
                m1[j * 2 + 1] = (int16_t)(iv >> 5);
                m2[j] = (uint16_t)((iv & 31) * 32 + (iu & 31));
            }
        }
    }
}

// --------------------------------------------------------------------------------------------------- remap (device) ---
//
// One lane, kPx consecutive output pixels of the raster (one 16-byte map1 load, one 8-byte map2 load, 4 / 12 bytes out).
// The per-stream map planes are padded to a multiple of kMapAlign entries (undistort_map_stride), so the vector map loads
// of a stream's last lane stay inside its padded plane and are aligned.  The per-pixel arithmetic -- remap_px, its unaligned
// corner loads, the inside / partly inside / outside rule (BORDER_CONSTANT, cval 0) -- is undistort_inline.h's, shared with the
// front kernels of the motion and the subtraction tracker.
constexpr int kPx = 4;
constexpr int kUndistortWG = 256;

__device__ __forceinline__ void st_u32(uint8_t *p, uint32_t v) { ((ua_u32 *)p)->v = v; }

// kPx output pixels of one frame from its stream's map planes, starting at raster position p0 (< H*W)
template <int CH>
__device__ __forceinline__ void remap_lane(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                           const uint32_t *__restrict__ map1, const uint16_t *__restrict__ map2, size_t p0,
                                           size_t npx, int H, int W)
{
    uint32_t m1v[kPx], m2v[kPx];
    load_map4(map1, map2, p0, m1v, m2v);
    uint32_t v[kPx][CH];
#pragma unroll
    for (int k = 0; k < kPx; ++k) remap_px<CH>(src, H, W, m1v[k], m2v[k], v[k]);
    uint8_t *d = dst + p0 * CH;
    if (p0 + kPx <= npx) {
        if constexpr (CH == 3) {
            // three dword stores, kept apart: merged into one dwordx3 they would be a wide store
            st_u32(d, v[0][0] | v[0][1] << 8 | v[0][2] << 16 | v[1][0] << 24);
            asm volatile("" ::: "memory");
            st_u32(d + 4, v[1][1] | v[1][2] << 8 | v[2][0] << 16 | v[2][1] << 24);
            asm volatile("" ::: "memory");
            st_u32(d + 8, v[2][2] | v[3][0] << 8 | v[3][1] << 16 | v[3][2] << 24);
        } else {
            st_u32(d, v[0][0] | v[1][0] << 8 | v[2][0] << 16 | v[3][0] << 24);
        }
    } else {                                     // the frame's last, partial group
        for (int k = 0; k < kPx; ++k)
            if (p0 + k < npx)
                for (int c = 0; c < CH; ++c) d[k * CH + c] = (uint8_t)v[k][c];
    }
}

// grid: x = lanes of kPx pixels over one frame, y = stream of the launch
template <int CH>
__global__ __launch_bounds__(kUndistortWG) void k_undistort(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                            const uint32_t *__restrict__ map1, const uint16_t *__restrict__ map2,
                                                            size_t map_stride, int H, int W)
{
    const size_t npx = (size_t)H * W;
    const size_t p0 = ((size_t)blockIdx.x * kUndistortWG + threadIdx.x) * kPx;
    if (p0 >= npx) return;
    const int s = blockIdx.y;
    remap_lane<CH>(in + (size_t)s * npx * CH, out + (size_t)s * npx * CH, map1 + (size_t)s * map_stride,
                   map2 + (size_t)s * map_stride, p0, npx, H, W);
}

// The fused tracker's form (oatgpu_set_track_undistort): grid x = lanes of kPx pixels over one frame, y = stream (its map),
// z = frame of the step, each frame with input and output planes of its own (stream-major sets of n_streams frames).
struct UndistortFrames { const uint8_t *in[2]; uint8_t *out[2]; };

template <int CH>
__global__ __launch_bounds__(kUndistortWG) void k_undistort_frames(UndistortFrames f, const uint32_t *__restrict__ map1,
                                                                   const uint16_t *__restrict__ map2, size_t map_stride, int H,
                                                                   int W)
{
    const size_t npx = (size_t)H * W;
    const size_t p0 = ((size_t)blockIdx.x * kUndistortWG + threadIdx.x) * kPx;
    if (p0 >= npx) return;
    const int s = blockIdx.y;
    const uint8_t *in = blockIdx.z ? f.in[1] : f.in[0];
    uint8_t *out = blockIdx.z ? f.out[1] : f.out[0];
    remap_lane<CH>(in + (size_t)s * npx * CH, out + (size_t)s * npx * CH, map1 + (size_t)s * map_stride,
                   map2 + (size_t)s * map_stride, p0, npx, H, W);
}

size_t undistort_map_stride(int H, int W) { return ((size_t)H * W + kMapAlign - 1) / kMapAlign * kMapAlign; }

void launch_undistort(const uint8_t *in, uint8_t *out, const uint32_t *map1, const uint16_t *map2, size_t map_stride, int H,
                      int W, int channels, int n_streams, hipStream_t st)
{
    const size_t npx = (size_t)H * W, lanes = (npx + kPx - 1) / kPx;
    const dim3 grid((unsigned)((lanes + kUndistortWG - 1) / kUndistortWG), (unsigned)n_streams);
    if (channels == 3)
        hipLaunchKernelGGL(k_undistort<3>, grid, dim3(kUndistortWG), 0, st, in, out, map1, map2, map_stride, H, W);
    else
        hipLaunchKernelGGL(k_undistort<1>, grid, dim3(kUndistortWG), 0, st, in, out, map1, map2, map_stride, H, W);
}

void launch_undistort_frames(const uint8_t *const *in, uint8_t *const *out, int n_frames, const uint32_t *map1,
                             const uint16_t *map2, size_t map_stride, int H, int W, int channels, int n_streams, hipStream_t st)
{
    const size_t npx = (size_t)H * W, lanes = (npx + kPx - 1) / kPx;
    UndistortFrames f{};
    for (int i = 0; i < 2; ++i) {
        f.in[i] = in[i < n_frames ? i : 0];
        f.out[i] = out[i < n_frames ? i : 0];
    }
    const dim3 grid((unsigned)((lanes + kUndistortWG - 1) / kUndistortWG), (unsigned)n_streams, (unsigned)n_frames);
    if (channels == 3)
        hipLaunchKernelGGL(k_undistort_frames<3>, grid, dim3(kUndistortWG), 0, st, f, map1, map2, map_stride, H, W);
    else
        hipLaunchKernelGGL(k_undistort_frames<1>, grid, dim3(kUndistortWG), 0, st, f, map1, map2, map_stride, H, W);
}

}  // namespace oatgpu
