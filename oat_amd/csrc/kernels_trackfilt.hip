// kernels_trackfilt.hip -- the two kernels over the chain `posifilt kalman` -> `posifilt homography` -> `posifilt region`
// (chain_step, posfilt_inline.h: ONE definition): k_marker_filters behind the combined record of a marker set
// (oatgpu_set_marker_filters) and k_tracker_filters behind the motion and the subtraction tracker
// (oatgpu_set_tracker_filters).  One lane per camera stream, fp64; out: nine 64-bit words a stream
// (MarkerFiltered), 64-bit stores only.
#include "oatgpu_internal.h"
#include "posfilt_inline.h"

namespace oatgpu {

static_assert(sizeof(MarkerFiltered) == 72, "nine 64-bit words");

// The chain's input is the combined record: a partial-sum x, y under position_valid == 0 is no measurement.  The nf (1 or 2)
// frames of the step are taken IN ORDER in the lane's own loop: the Kalman recurrence of a paired step is not split over the grid
// as the combiner's frames are.
__global__ __launch_bounds__(64) void k_marker_filters(const MarkerFilterParams *__restrict__ p, KalmanState *state,
                                                       const MarkerCombined *in0, const MarkerCombined *in1, MarkerFiltered *out0,
                                                       MarkerFiltered *out1, int nf, int n_streams)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_streams) return;
    const bool kalman = p->kalman != 0;
    const KalmanLaunch k = chain_kalman(p, state);
    Filter f;
    if (kalman) load_filter(f, state + s);
#pragma unroll 1
    for (int t = 0; t < nf; ++t) {
        const MarkerCombined *in = (t ? in1 : in0) + s;
        chain_step(p, k, f, in->position_valid, in->heading_valid, in->x, in->y, in->hx, in->hy, (t ? out1 : out0) + s);
    }
    if (kalman) store_filter(f, state + s);
}

void launch_marker_filters(const MarkerFilterParams *params, KalmanState *state, const MarkerCombined *const *in,
                           MarkerFiltered *const *out, int n_streams, int nf, hipStream_t st)
{
    const int k = nf > 1 ? 1 : 0;
    hipLaunchKernelGGL(k_marker_filters, dim3((n_streams + 63) / 64), dim3(64), 0, st, params, state, in[0], in[k], out[0], out[k],
                       nf, n_streams);
}

// The chain's input is the tracker's own result record of one slot (BatchedTrackerState::rec: host-mapped, written by the blob
// kernels of the launch before on the same HIP stream).  A detector publishes no heading: heading_valid = 0, hx = hy = 0.
// Frame order: one launch a frame.  The launches of consecutive frames sit on different HIP streams inside the sequence calls
// (frame t's back half runs on B[t % 3]); the HOST orders them with an event per slot (api_trackfilt.hip) -- nothing waits on the
// device, so the state needs no ticket.
__global__ __launch_bounds__(64) void k_tracker_filters(const MarkerFilterParams *__restrict__ p, KalmanState *state,
                                                        const ResultRec *in, MarkerFiltered *out, int n_streams)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_streams) return;
    const bool kalman = p->kalman != 0;
    const KalmanLaunch k = chain_kalman(p, state);
    Filter f;
    if (kalman) load_filter(f, state + s);
    double x, y;
    const bool valid = centroid_of(in[s], x, y);    // posidet's centroid: the host epilogue's and k_kalman's
    chain_step(p, k, f, valid ? 1 : 0, 0, x, y, 0.0, 0.0, out + s);
    if (kalman) store_filter(f, state + s);
}

void launch_tracker_filters(const MarkerFilterParams *params, KalmanState *state, const ResultRec *in, MarkerFiltered *out,
                            int n_streams, hipStream_t st)
{
    hipLaunchKernelGGL(k_tracker_filters, dim3((n_streams + 63) / 64), dim3(64), 0, st, params, state, in, out, n_streams);
}

}  // namespace oatgpu
