// kernels_debayer.hip -- Bayer RAW8 -> BGR: the frame server's pixel-format conversion of a colour camera
// (src/frameserver/PointGreyCam.cpp:48-50, :729) as a device stage, for every camera stream (grid y) and both frames of a
// two-frame step (grid z) in one launch.
//
// The arithmetic is OpenCV 3.1's bilinear Bayer2RGB_ in 32-bit integers (debayer_inline.h, shared with the front kernels that
// demosaic in registers).  Output (y, x) is the triple of (clamp(y, 1, H - 2), clamp(x, 1, W - 2)) with THAT pixel's site
// colours: first / last column and row repeat their neighbours.
//
// The pattern is run-time data: per stream two parity bits, the row and the column of the R sample of the 2 x 2 tile, one bit
// a stream in two 64-bit kernel arguments (so at most 64 streams a launch).
//
// Two lane mappings:
//   wide   (W % 4 == 0, raw and BGR planes 4-byte aligned): a lane owns 4 pixels x 2 rows at (2 ty, 4 tx), the lanes laid
//          over the (H + 1) / 2 x W / 4 blocks in raster order.  It reads the dwords at x0 - 4, x0, x0 + 4 of the FOUR raw rows
//          around its block (the neighbour columns are extra dword loads, served by the vector cache: the lanes left and
//          right load the same dwords as their centre) and writes 3 dwords (12 bytes) of each of its two BGR rows.
//   narrow (everything else): one pixel a lane, byte accesses.
// No LDS, no scratch; nothing wider than a dword is stored (DESIGN.md 3b does not arise).
#include "oatgpu_internal.h"
#include "debayer_inline.h"

namespace oatgpu {

namespace {

constexpr int kDebayerWG = 256;

struct DebayerArgs {
    const uint8_t *in[2];                // [n][H*W] stream-major, one plane set a frame of the step
    uint8_t *out[2];                     // [n][H*W*3]
    u64 r_row, r_col;                    // bit (stream - first_stream): parity of the row / the column of the R sample
    int H, W, first_stream;
};

// 12 bytes as three dword stores, kept apart: merged into one dwordx3 they would be a wide store
__device__ __forceinline__ void store4(uint8_t *d, const unsigned px[4])
{
    unsigned *q = (unsigned *)d;
    q[0] = px[0] | px[1] << 24;
    asm volatile("" ::: "memory");
    q[1] = px[1] >> 8 | px[2] << 16;
    asm volatile("" ::: "memory");
    q[2] = px[2] >> 16 | px[3] << 8;
}

// grid: x = lanes over the (H + 1) / 2 x W / 4 blocks of one frame, y = stream of the launch, z = frame of the step
__global__ __launch_bounds__(kDebayerWG) void k_debayer_wide(DebayerArgs a)
{
    const int H = a.H, W = a.W, bw = W >> 2;
    const unsigned id = blockIdx.x * (unsigned)kDebayerWG + threadIdx.x;
    const unsigned nblk = (unsigned)((H + 1) >> 1) * (unsigned)bw;
    if (id >= nblk) return;
    const int ty = (int)(id / (unsigned)bw), tx = (int)(id - (unsigned)ty * (unsigned)bw);
    const int y0 = ty * 2, x0 = tx * 4;
    const int s = a.first_stream + (int)blockIdx.y;
    const bool r_row = (a.r_row >> blockIdx.y) & 1ull, r_col = (a.r_col >> blockIdx.y) & 1ull;      // uniform
    const size_t npx = (size_t)H * W;
    const uint8_t *in = (blockIdx.z ? a.in[1] : a.in[0]) + (size_t)s * npx;
    uint8_t *out = (blockIdx.z ? a.out[1] : a.out[0]) + (size_t)s * npx * 3;

    // the rows whose triples the lane's two output rows take (the same row twice at the top and bottom edges)
    const int ya = min(max(y0, 1), H - 2), yb = min(max(y0 + 1, 1), H - 2);
    const int xl = x0 > 0 ? x0 - 4 : x0, xr = x0 + 4 < W ? x0 + 4 : x0;     // clamped: the values they give are not used
    u64 w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint8_t *row = in + (size_t)min(ya - 1 + k, H - 1) * W;
        w[k] = window(*(const unsigned *)(row + xl), *(const unsigned *)(row + x0), *(const unsigned *)(row + xr));
    }
    const bool col0_r = r_col == false;                  // x0 is even: column x0 holds R samples iff the R column parity is 0
    unsigned pa[4], pb[4];
    row4(w[0], w[1], w[2], ((ya & 1) != 0) == r_row, col0_r, pa);
    row4(w[1], w[2], w[3], (((ya + 1) & 1) != 0) == r_row, col0_r, pb);
    if (yb == ya) {
#pragma unroll
        for (int i = 0; i < 4; ++i) pb[i] = pa[i];
    }
    if (x0 == 0) { pa[0] = pa[1]; pb[0] = pb[1]; }       // first and last column: the neighbour's triple
    if (x0 + 4 == W) { pa[3] = pa[2]; pb[3] = pb[2]; }
    store4(out + ((size_t)y0 * W + x0) * 3, pa);
    if (y0 + 1 < H) store4(out + ((size_t)(y0 + 1) * W + x0) * 3, pb);
}

// grid: x = pixels of one frame, y = stream of the launch, z = frame of the step
__global__ __launch_bounds__(kDebayerWG) void k_debayer_narrow(DebayerArgs a)
{
    const int H = a.H, W = a.W;
    const size_t npx = (size_t)H * W;
    const size_t p = (size_t)blockIdx.x * kDebayerWG + threadIdx.x;
    if (p >= npx) return;
    const int y = (int)(p / (size_t)W), x = (int)(p - (size_t)y * W);
    const int s = a.first_stream + (int)blockIdx.y;
    const bool r_row = (a.r_row >> blockIdx.y) & 1ull, r_col = (a.r_col >> blockIdx.y) & 1ull;
    const uint8_t *in = (blockIdx.z ? a.in[1] : a.in[0]) + (size_t)s * npx;
    uint8_t *out = (blockIdx.z ? a.out[1] : a.out[0]) + (size_t)s * npx * 3;
    const unsigned v = debayer_px1(in, H, W, y, x, r_row, r_col);
    uint8_t *d = out + p * 3;
    d[0] = (uint8_t)v; d[1] = (uint8_t)(v >> 8); d[2] = (uint8_t)(v >> 16);
}

}  // namespace

bool debayer_is_wide(int W, const uint8_t *const *in, uint8_t *const *out, int n_frames)
{
    uintptr_t m = 0;
    for (int i = 0; i < n_frames; ++i) m |= (uintptr_t)in[i] | (uintptr_t)out[i];
    return W % 4 == 0 && (m & 3u) == 0;
}

// patterns[n_streams]: OATGPU_BAYER_* values 1..4 (checked by the caller); H, W >= 3
void launch_debayer_frames(const uint8_t *const *in, uint8_t *const *out, int n_frames, const int *patterns, int H, int W,
                           int n_streams, hipStream_t st)
{
    const bool wide = debayer_is_wide(W, in, out, n_frames);
    const size_t lanes = wide ? (size_t)((H + 1) / 2) * (size_t)(W / 4) : (size_t)H * W;
    const unsigned gx = (unsigned)((lanes + kDebayerWG - 1) / kDebayerWG);
    for (int s0 = 0; s0 < n_streams; s0 += 64) {         // the parity bits of a launch are two 64-bit kernel arguments
        const int n = n_streams - s0 < 64 ? n_streams - s0 : 64;
        DebayerArgs a{};
        for (int i = 0; i < 2; ++i) {
            a.in[i] = in[i < n_frames ? i : 0];
            a.out[i] = out[i < n_frames ? i : 0];
        }
        a.H = H; a.W = W; a.first_stream = s0;
        bayer_parity_bits(patterns + s0, n, a.r_row, a.r_col);
        const dim3 grid(gx, (unsigned)n, (unsigned)n_frames);
        if (wide) hipLaunchKernelGGL(k_debayer_wide, grid, dim3(kDebayerWG), 0, st, a);
        else hipLaunchKernelGGL(k_debayer_narrow, grid, dim3(kDebayerWG), 0, st, a);
    }
}

}  // namespace oatgpu
