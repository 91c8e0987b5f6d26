// posfilt_inline.h -- the arithmetic of `posifilt kalman` and `posifilt homography`, and posidet's centroid in front of them
// (centroid_of), ONE definition for every user: k_kalman (kernels_kalman.hip, the foreground result), k_marker_filters and
// k_tracker_filters (kernels_trackfilt.hip: the combined record of a marker set, the result record of the motion and the
// subtraction tracker), k_marker_combine (kernels_markers.hip, the centroid) and the host epilogue of api_track.hip (to_position;
// the homography of a plain track call).  The chain kalman -> homography -> region of the two filter kernels is chain_step below.
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

// posidet's centroid of a result record from its exact integer sums: contourMoments' epilogue (imgproc/moments.cpp: m00 = a00 *
// db1_2, m10 = a10 * db1_6, m01 = a01 * db1_6) and siftContours' centroid m10 / m00, m01 / m00 (DetectorFunc.cpp:54-62).  An
// invalid record gives false and the (0, 0) an invalid Position2D keeps.  ONE definition for the position the host hands out
// (to_position, api_track.hip; area: where m00 goes, the position's area) and for what k_kalman, k_marker_combine and
// k_tracker_filters take as their measurement: a position and its filtered record agree to the bit.
__host__ __device__ inline bool centroid_of(const ResultRec &r, double &x, double &y, double *area = nullptr)
{
    x = 0.0; y = 0.0;
    if (!r.valid) return false;
    const double a00 = (double)r.a00, a10 = (double)r.a10, a01 = (double)r.a01;
    const double db1_2 = a00 > 0 ? 0.5 : -0.5;
    const double db1_6 = a00 > 0 ? 0.16666666666666666666666666666667 : -0.16666666666666666666666666666667;
    const double m00 = a00 * db1_2;
    x = (a10 * db1_6) / m00;
    y = (a01 * db1_6) / m00;
    if (area) *area = m00;
    return true;
}

// A ranked blob's shape from its exact integer sums (oatgpu_shape, include/oatgpu.h "target shapes": the text there is the
// contract, this is its one implementation): contourMoments' epilogue for the order-2 moments (m20 = a20 * db1_12, m11 = a11 *
// db1_24, m02 = a02 * db1_12), completeMomentState's central moments (cx = m10 * inv_m00, mu20 = m20 - m10 * cx, ...), then the
// covariance's eigenvalues and the eigenvector of the larger one in closed form.  fp64, + - * / sqrt only, one rounding each.
struct ShapeDerived {
    double mu20, mu11, mu02, axis_x, axis_y, major, minor;
    int axis_valid;
};
__host__ __device__ inline void shape_of(long long a00_, long long a10_, long long a01_, long long a20_, long long a11_,
                                         long long a02_, ShapeDerived &o)
{
    const double a00 = (double)a00_, a10 = (double)a10_, a01 = (double)a01_;
    const double a20 = (double)a20_, a11 = (double)a11_, a02 = (double)a02_;
    const double db1_2 = a00 > 0 ? 0.5 : -0.5;
    const double db1_6 = a00 > 0 ? 0.16666666666666666666666666666667 : -0.16666666666666666666666666666667;
    const double db1_12 = a00 > 0 ? 0.083333333333333333333333333333333 : -0.083333333333333333333333333333333;
    const double db1_24 = a00 > 0 ? 0.041666666666666666666666666666667 : -0.041666666666666666666666666666667;
    const double m00 = a00 * db1_2, m10 = a10 * db1_6, m01 = a01 * db1_6;
    const double m20 = a20 * db1_12, m11 = a11 * db1_24, m02 = a02 * db1_12;
    const double inv = 1.0 / m00;
    const double cx = m10 * inv, cy = m01 * inv;
    o.mu20 = m20 - m10 * cx;
    o.mu11 = m11 - m10 * cy;
    o.mu02 = m02 - m01 * cy;
    const double a = o.mu20 * inv, b = o.mu11 * inv, c = o.mu02 * inv;
    const double h = (a - c) * 0.5;
    const double r = sqrt(h * h + b * b);
    const double l1 = (a + c) * 0.5 + r, l2 = (a + c) * 0.5 - r;
    o.major = 2.0 * sqrt(l1 > 0.0 ? l1 : 0.0);
    o.minor = 2.0 * sqrt(l2 > 0.0 ? l2 : 0.0);
    double vx, vy;
    if (h >= 0.0) { vx = h + r; vy = b; } else { vx = b; vy = r - h; }
    const double n = sqrt(vx * vx + vy * vy);
    o.axis_valid = n > 0.0 ? 1 : 0;
    o.axis_x = 0.0; o.axis_y = 0.0;
    if (o.axis_valid) {
        o.axis_x = vx / n; o.axis_y = vy / n;
        if (vx < 0.0 || (vx == 0.0 && vy < 0.0)) { o.axis_x = -o.axis_x; o.axis_y = -o.axis_y; }
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

// ---- the chain `posifilt kalman` -> `posifilt homography` -> `posifilt region` on one record: k_marker_filters, k_tracker_filters ----

// a stream's filter state between launches, as k_kalman reads and writes it (there in the kernel's own body: moving it into a
// function shared with this one changed that kernel's register allocation, which is held to the measured one)
__device__ inline void load_filter(Filter &f, const KalmanState *ks)
{
    for (int i = 0; i < 4; ++i) { f.statePre[i] = ld(&ks->statePre[i]); f.statePost[i] = ld(&ks->statePost[i]); f.reported[i] = ld(&ks->reported[i]); }
    for (int i = 0; i < 16; ++i) { f.Ppre[i] = ld(&ks->Ppre[i]); f.Ppost[i] = ld(&ks->Ppost[i]); }
    f.meas[0] = ld(&ks->meas[0]); f.meas[1] = ld(&ks->meas[1]);
    f.found = __hip_atomic_load(&ks->found, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    f.missing = __hip_atomic_load(&ks->missing, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    f.aliased = __hip_atomic_load(&ks->aliased, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline void store_filter(const Filter &f, KalmanState *ks)
{
    for (int i = 0; i < 4; ++i) { st(&ks->statePre[i], f.statePre[i]); st(&ks->statePost[i], f.statePost[i]); }
    for (int i = 0; i < 16; ++i) { st(&ks->Ppre[i], f.Ppre[i]); st(&ks->Ppost[i], f.Ppost[i]); }
    st(&ks->meas[0], f.meas[0]); st(&ks->meas[1], f.meas[1]);
    __hip_atomic_store(&ks->found, f.found, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&ks->missing, f.missing, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&ks->aliased, f.aliased, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// cv::pointPolygonTest(contour, pt, measureDist = false) >= 0 for an integer contour and an integer point: OpenCV 3.1's purely
// integer branch (modules/imgproc/src/geometry.cpp, [OCV-mem]) in 64-bit integers -- a crossing count over the edges
// (v0 = previous vertex, v), the boundary counted as inside, an empty contour never hit.  The vertices are read from memory.
__device__ inline bool point_in_region(const int (*__restrict__ v)[2], int n, long long px, long long py)
{
    if (n <= 0) return false;
    long long x0 = v[n - 1][0], y0 = v[n - 1][1];
    int crossings = 0;
    for (int i = 0; i < n; ++i) {
        const long long x = v[i][0], y = v[i][1];
        if ((y0 <= py && y <= py) || (y0 > py && y > py) || (x0 < px && x < px)) {
            if (py == y && (px == x || (py == y0 && ((x0 <= px && px <= x) || (x <= px && px <= x0))))) return true;
        } else {
            long long d = (py - y0) * (x - x0) - (px - x0) * (y - y0);
            if (d == 0) return true;
            if (y < y0) d = -d;
            crossings += d > 0;
        }
        x0 = x; y0 = y;
    }
    return (crossings & 1) != 0;
}

// the chain's Kalman parameters as filter_step takes them (the ticket of KalmanState is not used by the chain)
__device__ inline KalmanLaunch chain_kalman(const MarkerFilterParams *p, KalmanState *state)
{
    KalmanLaunch k;
    k.state = state; k.dt = p->dt; k.sig_accel = p->sig_accel; k.sig_noise = p->sig_noise; k.threshold = p->threshold; k.ticket = 0u;
    return k;
}

// One sample of one stream through the chain, written to *out as nine 64-bit words (MarkerFiltered's layout).
//   kalman      KalmanFilter2D::filter on (position_valid, x, y) -- x, y under position_valid == 0 is no measurement;
//               position_valid = velocity_valid = found, position / velocity = the reported state (k_kalman's); the heading
//               passes through
//   homography  HomographyTransform2D::filter (:63-106): the position where valid, velocity and heading where valid through the
//               matrix with its offsets zeroed; the heading then through cv::normalize of a one-element vector -- multiplied
//               by the reciprocal of its length (0 where the length is not above DBL_EPSILON), plus 0.0
//   region      RegionFilter2D::filter (:130-152) where position_valid: (cv::Point)position = cvRound per coordinate, the
//               regions in configured order, the first hit wins; a coordinate that is not finite or beyond int32 hits none
__device__ inline void chain_step(const MarkerFilterParams *__restrict__ p, const KalmanLaunch &k, Filter &f, int position_valid,
                                  const int heading_valid, double x, double y, double hx, double hy, MarkerFiltered *out)
{
    const int n_regions = p->n_regions;
    int velocity_valid = 0;
    double vx = 0.0, vy = 0.0;
    if (p->kalman != 0) {
        filter_step(f, k, position_valid != 0, x, y);
        const double *rep = f.aliased ? f.statePre : f.reported;
        x = rep[0]; vx = rep[1]; y = rep[2]; vy = rep[3];
        position_valid = velocity_valid = f.found;
    }
    if (p->homography != 0) {
        if (position_valid) perspective_point(p->h, x, y);
        if (velocity_valid) perspective_point(p->h, vx, vy, false);
        if (heading_valid) {
            perspective_point(p->h, hx, hy, false);
            const double len = sqrt(hx * hx + hy * hy);
            const double scale = len > DBL_EPSILON ? 1.0 / len : 0.0;
            hx = hx * scale + 0.0;
            hy = hy * scale + 0.0;
        }
    }
    int region = -1;
    if (n_regions > 0 && position_valid) {
        const double rx = rint(x), ry = rint(y);               // cvRound: to nearest, ties to even
        if (rx >= -2147483648.0 && rx <= 2147483647.0 && ry >= -2147483648.0 && ry <= 2147483647.0) {
            const long long px = (long long)rx, py = (long long)ry;
            for (int r = 0; r < n_regions && region < 0; ++r)
                if (point_in_region(p->verts + p->region[r][0], p->region[r][1], px, py)) region = r;
        }
    }
    // 64-bit stores, one field (or pair of flags) each (nothing wider than 64 bits)
    u64 *o = reinterpret_cast<u64 *>(out);
    auto put = [&](int i, u64 v) { __hip_atomic_store(o + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    put(0, (u64)(unsigned)position_valid | (u64)(unsigned)velocity_valid << 32);
    put(1, (u64)(unsigned)heading_valid | (u64)(unsigned)(region >= 0) << 32);
    put(2, (u64)(unsigned)region);
    put(3, (u64)__double_as_longlong(x));
    put(4, (u64)__double_as_longlong(y));
    put(5, (u64)__double_as_longlong(vx));
    put(6, (u64)__double_as_longlong(vy));
    put(7, (u64)__double_as_longlong(hx));
    put(8, (u64)__double_as_longlong(hy));
}

}  // namespace oatgpu
