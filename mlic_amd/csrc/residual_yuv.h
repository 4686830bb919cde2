// Residual coding of Y'CbCr frames (DESIGN.md section 5 "Residual coding", "Y'CbCr frames"): the integer definitions
// shared by the kernels (residual_yuv.hip), the C entries (capi.cpp) and the file (container.cpp).  Host and device,
// no HIP call.  residual.h's classes, bins, escape and digest and residual16.h's quantiser, split and shift rule are
// reused as they are.
//
// A frame is three planes: p = 0 is Y' of H x W, p = 1 (Cb) and p = 2 (Cr) are hc x wc with hc = ceil(H / sub_y) and
// wc = ceil(W / sub_x), (sub_x, sub_y) one of (1, 1), (2, 1), (2, 2).  Samples have d bits, d in 8..16, maxv = 2^d - 1:
// bytes at d = 8, uint16 words above, LSB-aligned (sample = min(word, maxv)) or MSB-aligned (sample = word >> (16 - d),
// and a written word carries zero low bits): the rules of the 16-bit I/O calls.  Lossless means lossless in the samples.
// Canonical order, plane-major, then row, then column: i = off_p + y w_p + x with off_0 = 0, off_1 = H W,
// off_2 = H W + hc wc; N = H W + 2 hc wc samples, N <= RES_SEG_MAX_N.
// base is the three planes the Y'CbCr egress writes from the inner file decoded alone; q and rec are residual16_quant
// and residual16_rec with maxv (residual.h's values at d = 8): rec clamps to [0, maxv], not to the legal range, so a
// limited-range frame with samples outside it comes back exactly.
// Context: 8 p + residual_class(a >> (d - 8)), a = max - min of base plane p over the 3 x 3 neighbourhood with the
// coordinates clamped into that plane.
// Shift s in 0..max_shift(d): 0 at d = 8 and d - 7 above; residual16_shift with this frame's N chooses it.
// Low-bit plane: rows in canonical order (H of luma, hc of Cb, hc of Cr), G_p = ceil(w_p / 64); the 64-bit word
// (rowbase_p + y G_p + g) s + j holds bit j of lo at bit x mod 64, bits beyond the plane's width are zero;
// s (H G_0 + 2 hc G_1) words a frame.
// Digest: the sum of residual_digest_term(base_i, i) over the canonical index, times K.
#ifndef MLIC_RESIDUAL_YUV_H
#define MLIC_RESIDUAL_YUV_H
#include "residual16.h"
#include "residual_seg.h"

namespace mlic {

constexpr int RESYUV_MIN_DEPTH = 8, RESYUV_MAX_DEPTH = 16;

MLIC_RES_HD inline int residual_yuv_max_shift(int depth) { return depth <= 8 ? 0 : residual16_max_shift(depth); }
MLIC_RES_HD inline bool residual_yuv_sub_ok(int sub_x, int sub_y) {
  return (sub_x == 1 && sub_y == 1) || (sub_x == 2 && (sub_y == 1 || sub_y == 2));
}

// the sizes of one frame: what every index above is made of
struct ResYuvGeom {
  int64_t h[3], w[3];     // rows and columns of plane p
  int64_t off[3];         // the canonical index of plane p's first sample
  int64_t G[3];           // 64-column groups of a row of plane p
  int64_t rowbase[3];     // groups before plane p's first row
  int64_t N, groups;      // samples; 64-column groups of all rows: the low-bit plane has groups * s words
};

MLIC_RES_HD inline ResYuvGeom residual_yuv_geom(int64_t H, int64_t W, int sub_x, int sub_y) {
  ResYuvGeom g;
  g.h[0] = H, g.w[0] = W;
  g.h[1] = g.h[2] = (H + sub_y - 1) / sub_y;
  g.w[1] = g.w[2] = (W + sub_x - 1) / sub_x;
  int64_t off = 0, rb = 0;
  for (int p = 0; p < 3; ++p) {
    g.off[p] = off, g.rowbase[p] = rb;
    g.G[p] = (g.w[p] + 63) / 64;
    off += g.h[p] * g.w[p];
    rb += g.h[p] * g.G[p];
  }
  g.N = off, g.groups = rb;
  return g;
}

MLIC_RES_HD inline int residual_yuv_context(int p, int a, int depth) { return 8 * p + residual_class(a >> (depth - 8)); }

// a sample of a word: shr = 16 - d for MSB-aligned words, 0 otherwise (and for bytes)
MLIC_RES_HD inline int residual_yuv_sample(int word, int shr, int maxv) {
  const int v = word >> shr;
  return v > maxv ? maxv : v;
}

inline int residual_yuv_shift(int depth, uint64_t N, uint32_t max_abs_q, uint64_t sum_abs_q) {
  return depth <= 8 ? 0 : residual16_shift(depth, N, max_abs_q, sum_abs_q);
}

inline uint64_t residual_yuv_plane_words(uint64_t H, uint64_t W, int sub_x, int sub_y, int s) {
  return (uint64_t)residual_yuv_geom((int64_t)H, (int64_t)W, sub_x, sub_y).groups * (uint64_t)s;
}

}  // namespace mlic
#endif
