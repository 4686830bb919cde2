// Byte rows at any address, through LDS (image_io.hip, image_yuv.hip): the row segment sits in LDS at its global
// address mod 4, whole aligned dwords move as dwords, and the up to three bytes at either end move as bytes --
// nothing outside the segment is read or written.  One wave per call.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace mlic {

__device__ inline int addr_mod4(const void* p) { return (int)(reinterpret_cast<uintptr_t>(p) & 3); }

// global bytes p[0, n) -> LDS bytes r[sh, sh + n), sh = p mod 4 (r is dword-aligned): one wave
__device__ inline void stage_in(const uint8_t* __restrict__ p, int n, uint32_t* r, int lane) {
  const int sh = addr_mod4(p);
  uint8_t* r8 = reinterpret_cast<uint8_t*>(r);
  const int end = sh + n, nd = (end + 3) >> 2;
  for (int k = lane; k < nd; k += 64) {
    const int lo = 4 * k, hi = lo + 4;
    if (lo >= sh && hi <= end) {
      r[k] = *reinterpret_cast<const uint32_t*>(p + (lo - sh));
    } else {
      for (int i = max(lo, sh); i < min(hi, end); ++i) r8[i] = p[i - sh];
    }
  }
}

// LDS bytes r[sh, sh + n) -> global bytes p[0, n), sh = p mod 4: one wave
__device__ inline void stage_out(uint8_t* __restrict__ p, int n, const uint32_t* r, int lane) {
  const int sh = addr_mod4(p);
  const uint8_t* r8 = reinterpret_cast<const uint8_t*>(r);
  const int end = sh + n, nd = (end + 3) >> 2;
  for (int k = lane; k < nd; k += 64) {
    const int lo = 4 * k, hi = lo + 4;
    if (lo >= sh && hi <= end) {
      *reinterpret_cast<uint32_t*>(p + (lo - sh)) = r[k];
    } else {
      for (int i = max(lo, sh); i < min(hi, end); ++i) p[i - sh] = r8[i];
    }
  }
}

}  // namespace mlic
