// Residual coding (DESIGN.md section 5 "Residual coding"): the integer definitions shared by the kernels
// (residual.hip), the table builder (capi.cpp) and the file (container.cpp).  Host and device, no HIP call.
//
// Samples are 8-bit RGB in the canonical order i = (c H + y) W + x.  base is the byte image the inner file decodes
// to, x the original, tau in 0..127 the bound, step = 2 tau + 1:
//     r = x - base;  q = sign(r) floor((|r| + tau) / step);  rec = clamp(base + q step, 0, 255)
// so |x - rec| <= tau for every (x, base, tau), rec = x at tau = 0, and |q| <= 255.
// Context of a sample: 8 c + class, class from a = max - min of channel c of base over the 3 x 3 neighbourhood with
// coordinates clamped into the image: 0 for a < 2, else floor(log2 a) (a <= 255, so at most 7).
// Histogram: 128 bins per context, bin q + 63 for |q| <= 63, bin 127 (the escape) for everything else.
// Digest of base: sum over i of (base_i + 1) ((i + 1) K) mod 2^64, K = 0x9E3779B97F4A7C15: a sum of wrapping
// products, so independent of order, and K is odd, so a change of one byte changes the sum.
#ifndef MLIC_RESIDUAL_H
#define MLIC_RESIDUAL_H
#include <cstdint>

#if defined(__HIPCC__)
#define MLIC_RES_HD __host__ __device__
#else
#define MLIC_RES_HD
#endif

namespace mlic {

constexpr int RES_MAX_TAU = 127;
constexpr int RES_CTX = 24;          // 3 channels x 8 classes
constexpr int RES_BINS = 128;        // per context
constexpr int RES_MAX_M = 63;        // the largest |q| with a bin of its own
constexpr int RES_ESCAPE_BIN = 127;
constexpr int RES_CDF_STRIDE = 2 * RES_MAX_M + 3;  // entries of the widest table's CDF
constexpr uint8_t RES_ABSENT = 0xFF;               // the file's m byte of a context without a table
constexpr uint64_t RES_DIGEST_K = 0x9E3779B97F4A7C15ull;

MLIC_RES_HD inline int residual_class(int a) {  // a = max - min, 0..255
  int k = 0;
  while (a >= 2) {
    a >>= 1;
    ++k;
  }
  return k;
}

// n / step for 0 <= n < 512 and 1 <= step <= 255 without a division: magic = ceil(2^17 / step), (n magic) >> 17
// (n magic < 2^27; exact for these ranges: tools/container_residual_check.cpp sweeps all of them)
MLIC_RES_HD inline uint32_t residual_magic(int step) { return ((1u << 17) + (uint32_t)step - 1) / (uint32_t)step; }
MLIC_RES_HD inline int residual_div(int n, uint32_t magic) { return (int)(((uint32_t)n * magic) >> 17); }

MLIC_RES_HD inline int residual_quant(int x, int base, int tau) {
  const int r = x - base, a = r < 0 ? -r : r;
  const int q = (a + tau) / (2 * tau + 1);
  return r < 0 ? -q : q;
}

MLIC_RES_HD inline int residual_rec(int base, int q, int tau) {
  const int v = base + q * (2 * tau + 1);
  return v < 0 ? 0 : v > 255 ? 255 : v;
}

MLIC_RES_HD inline int residual_bin(int q) { return q >= -RES_MAX_M && q <= RES_MAX_M ? q + RES_MAX_M : RES_ESCAPE_BIN; }

// one sample's term of the digest, before the multiplication by K (which distributes over the sum)
MLIC_RES_HD inline uint64_t residual_digest_term(int base, uint64_t i) { return (uint64_t)(base + 1) * (i + 1); }

}  // namespace mlic
#endif
