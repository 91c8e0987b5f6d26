// posfilt_inline.h -- the arithmetic of `posifilt kalman` and `posifilt homography`, ONE definition for every user:
// k_kalman (kernels_kalman.hip, the foreground result), k_marker_filters (kernels_markers.hip, the combined record of a marker
// set) and the host epilogue of api_track.hip (the homography of a plain track call).
//
// Reference: oat::KalmanFilter2D::filter / initializeFilter / initializeStaticMatracies
// (src/positionfilter/KalmanFilter2D.cpp:95-210) over cv::KalmanFilter(4, 2, 0, CV_64F) (OpenCV 3.1
// modules/video/src/kalman.cpp, [OCV-mem]); oat::HomographyTransform2D::filter (HomographyTransform2D.cpp:62-107) over
// cv::perspectiveTransform.  All fp64, operation order identical to oracle/kalman.c and oracle/pipeline.c (every user is built
// with -ffp-contract=off).
#pragma once

#include <float.h>
#include <math.h>

#include "oatgpu_internal.h"

namespace oatgpu {

// d (n x m) = a (n x 4) * b [+ c]; b is (4 x m), or (m x 4) when transposed; k runs 0..3 in order
__host__ __device__ inline void mul4(const double *a, int n, const double *b, int m, bool b_transposed, const double *c, double *d)
{
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < m; ++j) {
            double s = 0.0;
            for (int q = 0; q < 4; ++q) s += a[i * 4 + q] * (b_transposed ? b[j * 4 + q] : b[q * m + j]);
            d[i * m + j] = c ? s + c[i * m + j] : s;
        }
}

struct Filter {     // registers copy of one stream's KalmanState
    double statePre[4], statePost[4], Ppre[16], Ppost[16], meas[2], reported[4];
    int found, missing, aliased;
};

__host__ __device__ inline void static_matrices(const KalmanLaunch &k, double *A, double *Q, double *R)
{
    const double dt = k.dt, sa = k.sig_accel;
    for (int i = 0; i < 16; ++i) { A[i] = 0.0; Q[i] = 0.0; }
    for (int i = 0; i < 4; ++i) A[i * 5] = 1.0;
    A[0 * 4 + 1] = dt;
    A[2 * 4 + 3] = dt;
    Q[0 * 4 + 0] = sa * sa * (dt * dt * dt * dt) / 4.0;
    Q[0 * 4 + 1] = sa * sa * (dt * dt * dt) / 2.0;
    Q[1 * 4 + 0] = sa * sa * (dt * dt * dt) / 2.0;
    Q[1 * 4 + 1] = sa * sa * (dt * dt);
    Q[2 * 4 + 2] = sa * sa * (dt * dt * dt * dt) / 4.0;
    Q[2 * 4 + 3] = sa * sa * (dt * dt * dt) / 2.0;
    Q[3 * 4 + 2] = sa * sa * (dt * dt * dt) / 2.0;
    Q[3 * 4 + 3] = sa * sa * (dt * dt);
    R[0] = R[3] = k.sig_noise * k.sig_noise;
    R[1] = R[2] = 0.0;
}

// KalmanFilter2D::filter, KalmanFilter2D.cpp:95-141
__host__ __device__ inline void filter_step(Filter &f, const KalmanLaunch &k, bool valid, double x, double y)
{
    const double H[8] = {1, 0, 0, 0, 0, 0, 1, 0};
    if (valid) {
        f.meas[0] = x; f.meas[1] = y;
        f.missing = 0;
        if (!f.found) {                                         // initializeFilter, :143-164
            for (int i = 0; i < 16; ++i) f.Ppre[i] = 0.0;
            for (int i = 0; i < 4; ++i) f.Ppre[i * 5] = 1000.0;
            f.statePre[0] = x; f.statePre[1] = 0.0; f.statePre[2] = y; f.statePre[3] = 0.0;
            for (int i = 0; i < 4; ++i) f.statePost[i] = f.statePre[i];
        }
        f.found = 1;
    } else {
        f.missing++;
    }
    if (f.missing >= k.threshold) f.found = 0;
    if (!f.found) return;

    double A[16], Q[16], R[4], t1[16], t2[8], t3[4], t4[8], t5[2], hx[2];
    static_matrices(k, A, Q, R);
    // cv::KalmanFilter::predict
    mul4(A, 4, f.statePost, 1, false, nullptr, f.statePre);
    mul4(A, 4, f.Ppost, 4, false, nullptr, t1);
    mul4(t1, 4, A, 4, true, Q, f.Ppre);
    for (int i = 0; i < 4; ++i) f.statePost[i] = f.statePre[i];
    for (int i = 0; i < 16; ++i) f.Ppost[i] = f.Ppre[i];
    f.aliased = 1;
    // cv::KalmanFilter::correct (2x2 system in closed form, see oracle/kalman.c)
    mul4(H, 2, f.Ppre, 4, false, nullptr, t2);
    mul4(t2, 2, H, 2, true, R, t3);
    const double det = t3[0] * t3[3] - t3[1] * t3[2];
    for (int j = 0; j < 4; ++j) {
        t4[j] = (t3[3] * t2[j] - t3[1] * t2[4 + j]) / det;
        t4[4 + j] = (t3[0] * t2[4 + j] - t3[2] * t2[j]) / det;
    }
    mul4(H, 2, f.statePre, 1, false, nullptr, hx);
    t5[0] = f.meas[0] - hx[0];
    t5[1] = f.meas[1] - hx[1];
    for (int i = 0; i < 4; ++i) {
        const double g0 = t4[i], g1 = t4[4 + i];
        f.statePost[i] = f.statePre[i] + (g0 * t5[0] + g1 * t5[1]);
        for (int j = 0; j < 4; ++j) f.Ppost[i * 4 + j] = f.Ppre[i * 4 + j] - (g0 * t2[j] + g1 * t2[4 + j]);
    }
}

// A stream's state between its launches: only touched with agent-scope atomics (coherent across XCDs without cache write-backs)
__device__ __forceinline__ double ld(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// cv::perspectiveTransform of one CV_64FC2 point (OpenCV 3.1.0 core/matmul.cpp perspectiveTransform_<double>:
// w = x m6 + y m7 + m8; |w| > FLT_EPSILON -> multiply by 1/w, else (0, 0)).  off: 0 takes the matrix with its offsets m2, m5
// zeroed, as HomographyTransform2D::filter does for a velocity and a heading (:79-101); the products and sums are the same
// ones in the same order, the addend alone is 0.0.
__host__ __device__ inline void perspective_point(const double *m, double &px, double &py, bool off = true)
{
    const double x = px, y = py;
    double w = x * m[6] + y * m[7] + m[8];
    if (fabs(w) > (double)FLT_EPSILON) {
        w = 1. / w;
        px = (x * m[0] + y * m[1] + (off ? m[2] : 0.0)) * w;
        py = (x * m[3] + y * m[4] + (off ? m[5] : 0.0)) * w;
    } else {
        px = py = 0;
    }
}

}  // namespace oatgpu
