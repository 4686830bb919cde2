// What the residual kernels' files (residual.hip, residual16.hip, residual_yuv.hip) share: the wave and block
// reductions, the front kernels' output set and modes, the RGB launches' strides and block count, and the host-side
// checks of the entries' output pointers.  Helpers only: the kernels stay in their files.  The flush of a thread's
// packed class counts and the low-bit plane's ballot pack and shuffle unpack are written out in each kernel: as
// inline functions they changed the register allocation of the kernels that call them.
#pragma once
#include <cstdint>
#include <string>

#include "kernels.h"
#include "residual.h"

namespace mlic {

constexpr int R_TW = 256;  // columns of a staged row segment, in every residual kernel
enum { F_CTX = 0, F_STATS = 1, F_FULL = 2 };  // front: without x; statistics only; everything

struct RStride {  // element strides of an RGB image batch
  int64_t img, row, col, ch;
};

struct FrontOut {  // what a front launch of the deep kinds writes
  uint8_t* ctx;
  unsigned int* ctx_count;
  unsigned long long* digest;
  int16_t* sym;
  unsigned long long* plane;
  unsigned int* hist;
  unsigned int* max_err;
  unsigned int* max_abs_q;
  unsigned long long* sum_abs_q;
};

__device__ inline unsigned long long wave_sum64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
__device__ inline unsigned int wave_max32(unsigned int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, (unsigned int)__shfl_down(v, off, 64));
  return v;
}

// the tail of a four-wave block's reduction: lane 0 of wave w has left its value in r[w]
__device__ inline unsigned long long sum4(const unsigned long long* r) { return r[0] + r[1] + r[2] + r[3]; }
__device__ inline unsigned int max4(const unsigned int* r) { return max(max(r[0], r[1]), max(r[2], r[3])); }

// ---- host side
inline bool aligned(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }

// the blocks of an RGB launch: column tiles of R_TW, row tiles of block_rows
inline unsigned r_blocks(int B, int H, int W, int block_rows, int* tx, int* ty, const char* what) {
  *tx = (W + R_TW - 1) / R_TW;
  *ty = (H + block_rows - 1) / block_rows;
  const int64_t blocks = (int64_t)B * *tx * *ty;
  if (blocks > 0x7fffffffLL) throw Error(std::string("mlic: ") + what + ": batch too large for one launch");
  return (unsigned)blocks;
}

// the checks of a front entry's outputs, in the entries' order; w: the entry's name
inline void check_front_out(const std::string& w, const void* ctx, const void* ctx_count, const void* digest) {
  MLIC_CHECK(ctx != nullptr, w + ": null ctx");
  MLIC_CHECK(ctx_count != nullptr, w + ": null ctx_count");
  MLIC_CHECK(digest != nullptr, w + ": null digest");
  MLIC_CHECK(aligned(ctx_count, 4) && aligned(digest, 8), w + ": ctx_count must be 4-byte and digest 8-byte aligned");
}

inline void check_front_x_needed(const std::string& w, const void* sym, const void* hist, const void* max_err,
                                 const void* max_abs_q, const void* sum_abs_q) {
  MLIC_CHECK(sym != nullptr && hist != nullptr && max_err != nullptr && max_abs_q != nullptr && sum_abs_q != nullptr,
             w + ": with x, sym, hist, max_err, max_abs_q and sum_abs_q are all needed");
}

inline void check_front_x_aligned(const std::string& w, const void* sym, const void* lo_plane, const void* hist,
                                  const void* max_err, const void* max_abs_q, const void* sum_abs_q) {
  MLIC_CHECK(aligned(sym, 2) && aligned(hist, 4) && aligned(max_err, 4) && aligned(max_abs_q, 4) &&
                 aligned(sum_abs_q, 8) && aligned(lo_plane, 8),
             w + ": sym must be 2-byte, hist, max_err and max_abs_q 4-byte, sum_abs_q and lo_plane 8-byte aligned");
}

inline void check_front_without_x(const std::string& w, const void* sym, const void* lo_plane, const void* hist,
                                  const void* max_err, const void* max_abs_q, const void* sum_abs_q) {
  MLIC_CHECK(sym == nullptr && lo_plane == nullptr && hist == nullptr && max_err == nullptr && max_abs_q == nullptr &&
                 sum_abs_q == nullptr,
             w + ": sym, lo_plane, hist, max_err, max_abs_q and sum_abs_q go with x");
}

// an apply entry's scores: sq_err and max_err are given exactly when ref is
inline void check_apply_scores(const std::string& w, bool has_ref, const void* sq_err, const void* max_err) {
  MLIC_CHECK(!has_ref || sq_err != nullptr, w + ": ref without sq_err");
  MLIC_CHECK(!has_ref || max_err != nullptr, w + ": ref without max_err");
  MLIC_CHECK(has_ref || (sq_err == nullptr && max_err == nullptr), w + ": sq_err and max_err go with ref");
}

inline void check_apply_scores_aligned(const std::string& w, const void* sq_err, const void* max_err) {
  MLIC_CHECK(aligned(sq_err, 8) && aligned(max_err, 4), w + ": sq_err must be 8-byte and max_err 4-byte aligned");
}

}  // namespace mlic
