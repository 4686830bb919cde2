// Residual coding of 9..16-bit samples (DESIGN.md section 5 "Residual coding", "Deep samples"): the integer
// definitions shared by the kernels (residual16.hip), the C entries (capi.cpp) and the file (container.cpp).  Host and
// device, no HIP call.  residual.h's classes, bins and digest are reused as they are.
//
// Samples are d-bit RGB, d in 9..16, LSB-aligned in uint16 words, in the canonical order i = (c H + y) W + x;
// maxv = 2^d - 1, and a word above maxv reads as maxv (as the 16-bit ingest reads it).  base is the inner file decoded
// alone at depth d, x the original, tau in 0..127, step = 2 tau + 1:
//     r = x - base;  q = sign(r) floor((|r| + tau) / step);  rec = clamp(base + q step, 0, maxv)
// so |x - rec| <= tau, rec = x at tau = 0 and |q| <= maxv.
// Split by the file's shift s in 0..d-7: hi = q >> s (arithmetic, floor), lo = q - (hi << s) in 0..2^s-1, and
// q = (hi << s) + lo.  hi goes through residual.h's bins and the 24-context tables, so a file's s must satisfy
// (max|q| + 2^s - 1) >> s <= 255, which keeps |hi| <= 255; s = d - 7 always does.  The symbol plane holds hi as int16,
// saturated: a shift that does not fit shows in max|q|, never as a wrapped symbol.
// Context: 8 c + residual_class(a >> (d - 8)), a = max - min of channel c of base over the clamped 3 x 3 neighbourhood.
// Low-bit plane: row r = c H + y, group g = x / 64, G = ceil(W / 64); 64-bit word (r G + g) s + j holds bit j of
// lo(r, x) at bit x mod 64; bits beyond column W are zero.
#ifndef MLIC_RESIDUAL16_H
#define MLIC_RESIDUAL16_H
#include "residual.h"

namespace mlic {

constexpr int RES16_MIN_DEPTH = 9, RES16_MAX_DEPTH = 16;
constexpr int RES16_MAX_HI = 255;

MLIC_RES_HD inline int residual16_max_shift(int depth) { return depth - 7; }

// n / step for 0 <= n < 2^17 and odd 1 <= step <= 255 without a division: magic = floor(2^32 / step) + 1 for
// step >= 2 (it fits 32 bits) and the high word of n magic; magic step = 2^32 + e with 1 <= e <= step, so the
// quotient is exact while n e < 2^32, and n e < 2^25 here.  step = 1 has magic 0 and returns n.
// (tools/container_residual_deep_check.cpp sweeps every (n, step) of the range against a true division.)
MLIC_RES_HD inline uint32_t residual16_magic(int step) {
  return step <= 1 ? 0u : (uint32_t)((1ull << 32) / (uint32_t)step) + 1u;
}
MLIC_RES_HD inline uint32_t residual16_div(uint32_t n, uint32_t magic) {
  return magic ? (uint32_t)(((uint64_t)n * magic) >> 32) : n;
}

MLIC_RES_HD inline int residual16_quant(int x, int base, int tau, uint32_t magic) {
  const int r = x - base, a = r < 0 ? -r : r;
  const int q = (int)residual16_div((uint32_t)(a + tau), magic);
  return r < 0 ? -q : q;
}

MLIC_RES_HD inline int residual16_rec(int base, int q, int tau, int maxv) {
  const int v = base + q * (2 * tau + 1);
  return v < 0 ? 0 : v > maxv ? maxv : v;
}

MLIC_RES_HD inline int residual16_hi(int q, int s) { return q >> s; }  // arithmetic: floor
MLIC_RES_HD inline int residual16_lo(int q, int s) { return q - (q >> s) * (1 << s); }
MLIC_RES_HD inline int residual16_join(int hi, int lo, int s) { return hi * (1 << s) + lo; }
MLIC_RES_HD inline int residual16_sat(int hi) { return hi < -32768 ? -32768 : hi > 32767 ? 32767 : hi; }

// whether shift s keeps every |hi| within 255 for an image whose largest |q| is max_abs_q
MLIC_RES_HD inline bool residual16_fits(uint32_t max_abs_q, int s) {
  return ((max_abs_q + (1u << s) - 1u) >> s) <= (uint32_t)RES16_MAX_HI;
}

MLIC_RES_HD inline int residual16_context(int c, int a, int depth) { return 8 * c + residual_class(a >> (depth - 8)); }

// The shift rule: the smallest s in 0..d-7 that fits and has sum|q| <= 8 N 2^s (N = 3 H W samples); d - 7 if none.
inline int residual16_shift(int depth, uint64_t N, uint32_t max_abs_q, uint64_t sum_abs_q) {
  for (int s = 0; s <= residual16_max_shift(depth); ++s) {
    // 8 N 2^s: N <= 3 2^32 and s <= 9, so the product is below 2^47
    if (residual16_fits(max_abs_q, s) && sum_abs_q <= ((8 * N) << s)) return s;
  }
  return residual16_max_shift(depth);
}

// 64-bit words of one image's low-bit plane
inline uint64_t residual16_plane_words(uint64_t H, uint64_t W, int s) { return 3 * H * ((W + 63) / 64) * (uint64_t)s; }

}  // namespace mlic
#endif
