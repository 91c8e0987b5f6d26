// kernels_kalman.hip -- `oat posifilt kalman` on the batch of positions the blob stage just produced.
//
// Reference: oat::KalmanFilter2D::filter / initializeFilter / initializeStaticMatracies
// (src/positionfilter/KalmanFilter2D.cpp:95-210) over cv::KalmanFilter(4, 2, 0, CV_64F)
// (OpenCV 3.1 modules/video/src/kalman.cpp, [OCV-mem]).  One lane per camera stream, all fp64,
// operation order identical to oracle/kalman.c (built with -ffp-contract=off like the rest).
// The reference's observable quirks are kept: 6.0-filled report before the first track, the
// every-sample timeout test (default --timeout 0 never tracks), correction with the stale
// measurement on samples without a detection, predicted (not corrected) state reported.
//
// Ordering: consecutive frames of a stream run their back halves on different HIP streams, so the
// filter update takes a per-stream ticket: the launch of frame n waits until the state's ticket
// equals n.  State and ticket are only touched with agent-scope atomics (coherent across XCDs
// without cache write-backs); the ticket is bumped after the state stores have drained.
#include "oatgpu_internal.h"
#include "posfilt_inline.h"     // Filter / filter_step / static_matrices / centroid_of: shared with the chain kernels

namespace oatgpu {

__global__ __launch_bounds__(64) void k_kalman(KalmanLaunch k, ResultRec *results, int n_streams)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_streams) return;
    KalmanState *ks = k.state + s;
    while (__hip_atomic_load(&ks->ticket, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != k.ticket)
        __builtin_amdgcn_s_sleep(4);

    Filter f;
    for (int i = 0; i < 4; ++i) { f.statePre[i] = ld(&ks->statePre[i]); f.statePost[i] = ld(&ks->statePost[i]); f.reported[i] = ld(&ks->reported[i]); }
    for (int i = 0; i < 16; ++i) { f.Ppre[i] = ld(&ks->Ppre[i]); f.Ppost[i] = ld(&ks->Ppost[i]); }
    f.meas[0] = ld(&ks->meas[0]); f.meas[1] = ld(&ks->meas[1]);
    f.found = __hip_atomic_load(&ks->found, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    f.missing = __hip_atomic_load(&ks->missing, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    f.aliased = __hip_atomic_load(&ks->aliased, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

    ResultRec &r = results[s];
    double x, y;
    const bool valid = centroid_of(r, x, y);       // posidet's centroid: the host epilogue's (posfilt_inline.h)
    filter_step(f, k, valid, x, y);

    const double *rep = f.aliased ? f.statePre : f.reported;
    r.kx = rep[0]; r.kvx = rep[1]; r.ky = rep[2]; r.kvy = rep[3];
    r.kal_valid = f.found;

    for (int i = 0; i < 4; ++i) { st(&ks->statePre[i], f.statePre[i]); st(&ks->statePost[i], f.statePost[i]); }
    for (int i = 0; i < 16; ++i) { st(&ks->Ppre[i], f.Ppre[i]); st(&ks->Ppost[i], f.Ppost[i]); }
    st(&ks->meas[0], f.meas[0]); st(&ks->meas[1], f.meas[1]);
    __hip_atomic_store(&ks->found, f.found, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&ks->missing, f.missing, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&ks->aliased, f.aliased, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_s_waitcnt(0);                    // state stores have reached memory ...
    __hip_atomic_store(&ks->ticket, k.ticket + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ... before the next frame may read them
}

__global__ void k_kalman_reset(KalmanState *state, int n_streams, unsigned ticket)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_streams) return;
    KalmanState &k = state[s];
    for (int i = 0; i < 4; ++i) { k.statePre[i] = 0.0; k.statePost[i] = 0.0; k.reported[i] = 6.0; }
    for (int i = 0; i < 16; ++i) { k.Ppre[i] = 0.0; k.Ppost[i] = 0.0; }
    k.meas[0] = k.meas[1] = 6.0;
    k.found = 0; k.missing = 0; k.aliased = 0;
    k.ticket = ticket;
}

void launch_kalman(const KalmanLaunch &k, ResultRec *results, int n_streams, hipStream_t st)
{
    hipLaunchKernelGGL(k_kalman, dim3((n_streams + 63) / 64), dim3(64), 0, st, k, results, n_streams);
}

void launch_kalman_reset(KalmanState *state, int n_streams, unsigned ticket, hipStream_t st)
{
    hipLaunchKernelGGL(k_kalman_reset, dim3((n_streams + 63) / 64), dim3(64), 0, st, state, n_streams, ticket);
}

}  // namespace oatgpu
