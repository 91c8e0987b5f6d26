// kernels_measure.hip -- the kernels of api_measure.hip: what plain streaming reaches on this chip and what an empty launch costs
#include "oatgpu_internal.h"

namespace oatgpu {

// ---- achievable-bandwidth probes: the best plain streaming kernels found on this chip ----
// (tools/k1_lab.hip, profiles/r02_k1_lab.txt: one 16-byte element per thread on a FULL grid with the
// streaming cache policy copies at 6.6 TB/s; the usual 2048-block grid-stride loop reaches 5.0)
typedef unsigned nv4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_stream_read(const uint4 *src, size_t n, unsigned *sink)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const nv4 v = __builtin_nontemporal_load((const nv4 *)src + i);
    if ((v.x ^ v.y ^ v.z ^ v.w) == 0x9e3779b9u) *sink = v.x;      // keeps the load alive, practically never taken
}
__global__ __launch_bounds__(256) void k_stream_copy(const uint4 *src, uint4 *dst, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    __builtin_nontemporal_store(__builtin_nontemporal_load((const nv4 *)src + i), (nv4 *)dst + i);
}
void launch_stream_read(const void *src, size_t n16, unsigned *sink, hipStream_t st)
{
    hipLaunchKernelGGL(k_stream_read, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, st, (const uint4 *)src, n16, sink);
}
void launch_stream_copy(const void *src, void *dst, size_t n16, hipStream_t st)
{
    hipLaunchKernelGGL(k_stream_copy, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, st, (const uint4 *)src, (uint4 *)dst, n16);
}

__global__ void k_nop() {}
void launch_nop(hipStream_t st) { hipLaunchKernelGGL(k_nop, dim3(1), dim3(64), 0, st); }

}  // namespace oatgpu
