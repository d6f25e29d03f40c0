// Shared by the kernels that copy byte ranges of any alignment in 16-byte vectors
// (decode_stream.hip's moves and copies, woff2_file.hip's sfnt assembly).
#ifndef MIB_LOAD16_H_
#define MIB_LOAD16_H_
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mib {

// 16 source bytes of any alignment: the two aligned vectors they lie in, shifted together.
// Only called for 16 bytes that all belong to the source, so the second vector (read when the
// address is not aligned) holds the last of them and lies in the same allocation.
__device__ __forceinline__ uint4 load16_any(const uint8_t *s) {
  const uint32_t sh = (uint32_t)((uintptr_t)s & 15);
  const uint4 *p = reinterpret_cast<const uint4 *>(s - sh);
  const uint4 lo = p[0];
  if (sh == 0) return lo;
  const uint4 hi = p[1];
  uint32_t w0, w1, w2, w3, w4;
  switch (sh >> 2) {
    case 0: w0 = lo.x; w1 = lo.y; w2 = lo.z; w3 = lo.w; w4 = hi.x; break;
    case 1: w0 = lo.y; w1 = lo.z; w2 = lo.w; w3 = hi.x; w4 = hi.y; break;
    case 2: w0 = lo.z; w1 = lo.w; w2 = hi.x; w3 = hi.y; w4 = hi.z; break;
    default: w0 = lo.w; w1 = hi.x; w2 = hi.y; w3 = hi.z; w4 = hi.w; break;
  }
  const uint32_t bs = (sh & 3) * 8;
  uint4 r;
  r.x = (uint32_t)((((uint64_t)w1 << 32) | w0) >> bs);
  r.y = (uint32_t)((((uint64_t)w2 << 32) | w1) >> bs);
  r.z = (uint32_t)((((uint64_t)w3 << 32) | w2) >> bs);
  r.w = (uint32_t)((((uint64_t)w4 << 32) | w3) >> bs);
  return r;
}

}  // namespace mib
#endif
