// kernels_trackfilt.hip -- `posifilt kalman` -> `posifilt homography` -> `posifilt region` behind the motion and the subtraction
// tracker (oatgpu_set_tracker_filters).
//
// The input is the tracker's own result record of one slot (DiffTracker::rec / BsubTracker::rec: host-mapped, written by the blob
// kernels of the launch before on the same HIP stream); the chain -- chain_step, posfilt_inline.h -- is k_marker_filters' and has
// ONE definition.  A detector publishes no heading: heading_valid = 0, hx = hy = 0.
//
// Frame order: one launch a frame.  The launches of consecutive frames sit on different HIP streams inside the sequence calls
// (frame t's back half runs on B[t % 3]); the HOST orders them with an event per slot (api_trackfilt.hip) -- nothing waits on the
// device, so the state needs no ticket.
#include "oatgpu_internal.h"
#include "posfilt_inline.h"

namespace oatgpu {

// One lane per camera stream, fp64.  out: nine 64-bit words a stream (MarkerFiltered), 64-bit stores only.
__global__ __launch_bounds__(64) void k_tracker_filters(const MarkerFilterParams *__restrict__ p, KalmanState *state,
                                                        const ResultRec *in, MarkerFiltered *out, int n_streams)
{
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_streams) return;
    const bool kalman = p->kalman != 0;
    const KalmanLaunch k = chain_kalman(p, state);
    Filter f;
    if (kalman) load_filter(f, state + s);
    // posidet's centroid, exactly as k_kalman and the host epilogue (to_position) derive it from the integer sums; an invalid
    // Position2D keeps its initial (0, 0)
    const ResultRec &r = in[s];
    double x = 0.0, y = 0.0;
    const bool valid = r.valid != 0;
    if (valid) {
        const double a00 = (double)r.a00, a10 = (double)r.a10, a01 = (double)r.a01;
        const double db1_2 = a00 > 0 ? 0.5 : -0.5;
        const double db1_6 = a00 > 0 ? 0.16666666666666666666666666666667 : -0.16666666666666666666666666666667;
        const double m00 = a00 * db1_2;
        x = (a10 * db1_6) / m00;
        y = (a01 * db1_6) / m00;
    }
    chain_step(p, k, f, valid ? 1 : 0, 0, x, y, 0.0, 0.0, out + s);
    if (kalman) store_filter(f, state + s);
}

void launch_tracker_filters(const MarkerFilterParams *params, KalmanState *state, const ResultRec *in, MarkerFiltered *out,
                            int n_streams, hipStream_t st)
{
    static_assert(sizeof(MarkerFiltered) == 72, "nine 64-bit words");
    hipLaunchKernelGGL(k_tracker_filters, dim3((n_streams + 63) / 64), dim3(64), 0, st, params, state, in, out, n_streams);
}

}  // namespace oatgpu
