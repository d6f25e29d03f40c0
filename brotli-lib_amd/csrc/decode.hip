// brotli_amd: the product decode kernels' translation unit -- decode_streams_kernel and
// decode_parts_kernel (decode_core.inc) and their launchers.  The streaming sessions' kernel
// is decode_stream.hip's.
#define MIB_TU_VAR
#include "decode_core.inc"

// A launch with at most one stream (or part) per CU runs the build that gives each its CU's
// whole LDS; a larger one the four-per-CU build.
extern "C" hipError_t mib_decode_launch(mib::DecJob *d_jobs, int njobs, uint8_t *d_scratch, uint64_t per_block,
                                        uint64_t ring_bytes, int grid, int per_cu, hipStream_t stream) {
  if (per_cu <= 1)
    hipLaunchKernelGGL(mib::decode_streams_kernel<true>, dim3(grid), dim3(64), 0, stream, d_jobs, njobs, d_scratch, per_block,
                       ring_bytes);
  else
    hipLaunchKernelGGL(mib::decode_streams_kernel<false>, dim3(grid), dim3(64), 0, stream, d_jobs, njobs, d_scratch, per_block,
                       ring_bytes);
  return hipGetLastError();
}

extern "C" hipError_t mib_decode_parts_launch(mib::DecJob *d_jobs, int njobs, uint8_t *d_scratch, uint64_t per_block,
                                              unsigned *d_ticket, int grid, int per_cu, hipStream_t stream) {
  if (per_cu <= 1)
    hipLaunchKernelGGL(mib::decode_parts_kernel<true>, dim3(grid), dim3(64), 0, stream, d_jobs, njobs, d_scratch, per_block,
                       d_ticket);
  else
    hipLaunchKernelGGL(mib::decode_parts_kernel<false>, dim3(grid), dim3(64), 0, stream, d_jobs, njobs, d_scratch, per_block,
                       d_ticket);
  return hipGetLastError();
}

extern "C" hipError_t mib_decode_init_tables(const int16_t *host_lut) {
  return hipMemcpyToSymbol(HIP_SYMBOL(mib::kCmdLut), host_lut, sizeof(int16_t) * 704 * 4);
}

// First two bytes of each stream (window bits peek for scratch sizing) in one launch.
namespace mib {
__global__ void peek_heads_kernel(const uint8_t *in, const uint64_t *offsets, int k, uint8_t *heads) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < k; i += gridDim.x * blockDim.x) {
    uint64_t a = offsets[i], n = offsets[i + 1] - a;
    for (int q = 0; q < 16; q++) heads[16 * i + q] = (uint64_t)q < n ? in[a + q] : 0;
  }
}
}  // namespace mib

extern "C" hipError_t mib_decode_peek_heads(const uint8_t *d_in, const uint64_t *d_offsets, int k, uint8_t *d_heads,
                                            hipStream_t stream) {
  hipLaunchKernelGGL(mib::peek_heads_kernel, dim3((k + 255) / 256), dim3(256), 0, stream, d_in, d_offsets, k, d_heads);
  return hipGetLastError();
}

#ifdef MIB_PROF
extern "C" int mib_debug_read_hdr_prof(unsigned long long *out) {
  hipMemcpyFromSymbol(out, HIP_SYMBOL(mib::g_hdr_prof), sizeof(unsigned long long) * 16);
  unsigned long long z[16] = {0};
  hipMemcpyToSymbol(HIP_SYMBOL(mib::g_hdr_prof), z, sizeof(z));
  return 0;
}
extern "C" int mib_debug_read_part_prof(unsigned long long *out, int n) {
  if (n > mib::kPartProfMax) n = mib::kPartProfMax;
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(mib::g_part_prof), sizeof(unsigned long long) * 8 * n);
}
extern "C" int mib_debug_read_prof(unsigned long long *out) {
  hipMemcpyFromSymbol(out, HIP_SYMBOL(mib::g_prof), sizeof(unsigned long long) * 16);
  unsigned long long z[16] = {0};
  hipMemcpyToSymbol(HIP_SYMBOL(mib::g_prof), z, sizeof(z));
  return 0;
}
#endif

