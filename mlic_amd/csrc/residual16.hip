// Residual coding of 9..16-bit samples: the two passes over full-resolution uint16 words (residual16.h has the
// definitions; DESIGN.md section 5 "Residual coding", "Deep samples").  The structure is residual.hip's.
//
// residual_front_u16: base (and, for the encoder, the original x) -> the context plane, the per-context counts and the
// digest of base; with x also hi (the symbol plane), the low-bit plane, the histograms of hi, the largest |x - rec| and
// the statistics max|q| and sum|q|.  A statistics launch of the same kernel gives the last two alone: the shift is
// chosen from them, so they are needed before hi and lo can be formed.
// residual_apply_u16: base + hi + low-bit plane -> rec, optionally scored against a reference.
//
// Word images come through element strides {image, row, column, channel}.  Row segments go through LDS with
// image_stage.h's byte staging (words are 2-byte aligned, so a segment sits at its address mod 4, 0 or 2): HWC keeps
// its interleaved words, CHW three plane segments, any other stride set is gathered into the CHW form.  All forms
// give the same bits.
//
// front: 256 threads, one pixel column each, RF_GROUPS groups of RF_ROWS rows; per group RF_ROWS + 2 base rows and
// RF_ROWS rows of x are staged.  At two bytes a sample that is 15.6 + 12.5 KB of rows beside the 12 KB of histograms,
// 40 KB a block, so LDS allows four blocks (16 waves) a CU where the byte kernel has six.  A 256-column tile starts on
// a multiple of 64, so a wave is one 64-column group of the low-bit plane: bit j of lo is one ballot, lane j keeps
// word j, and lanes 0..s-1 store the group's s words of a row.  Lanes beyond the image take part with lo = 0, which
// is the plane's zero padding.
#include "image_stage.h"
#include "kernels.h"
#include "residual16.h"
#include "residual_dev.h"

namespace mlic {

namespace {

constexpr int R_SEG = (2 * (R_TW + 2) + 3 + 3) / 4;  // dwords of a (R_TW + 2)-word plane segment at any alignment
constexpr int R_ROW = 3 * R_SEG;                     // one staged row: three plane segments, or the HWC words
constexpr int RF_ROWS = 8, RF_GROUPS = 8;            // front: rows per group, groups per block
constexpr int RA_ROWS = 4, RA_REF_GROUPS = 16;       // apply: a row per wave; with ref a block walks 16 groups
enum { R_GENERAL = 0, R_HWC = 1, R_CHW = 2 };
static_assert(RF_ROWS * RF_GROUPS <= 255, "a thread's packed class counts are 8 bits each");
static_assert(6 * (R_TW + 2) + 3 <= 4 * R_ROW, "an HWC row fits the staged row");
static_assert(R_TW % 64 == 0, "a wave is one 64-column group of the low-bit plane");

int r_path(const int64_t* s) { return (s[2] == 3 && s[3] == 1) ? R_HWC : s[2] == 1 ? R_CHW : R_GENERAL; }

// n pixels from p (channel 0 of the segment's first pixel) into the staged row r: one wave
__device__ inline void seg_in(int path, const uint16_t* __restrict__ p, int64_t col, int64_t ch, int n, uint32_t* r,
                              int lane) {
  if (path == R_HWC) {
    stage_in(reinterpret_cast<const uint8_t*>(p), 6 * n, r, lane);
  } else if (path == R_CHW) {
    for (int c = 0; c < 3; ++c) stage_in(reinterpret_cast<const uint8_t*>(p + c * ch), 2 * n, r + c * R_SEG, lane);
  } else {
    uint16_t* r16 = reinterpret_cast<uint16_t*>(r);
    for (int c = 0; c < 3; ++c)
      for (int k = lane; k < n; k += 64) r16[c * R_SEG * 2 + k] = p[(int64_t)k * col + c * ch];
  }
}

// where channel c of pixel k sits in the staged row: byte index = seg_at(...) + (HWC ? 6 k : 2 k), always even
__device__ inline int seg_at(int path, const uint16_t* p, int64_t ch, int c) {
  if (path == R_HWC) return addr_mod4(p) + 2 * c;
  if (path == R_CHW) return c * R_SEG * 4 + addr_mod4(p + c * ch);
  return c * R_SEG * 4;
}

__device__ inline int word_at(const uint8_t* row, int byte) { return *reinterpret_cast<const uint16_t*>(row + byte); }

__device__ inline void seg_out(int path, uint16_t* __restrict__ p, int64_t ch, int n, const uint32_t* r, int lane) {
  if (path == R_HWC) {
    stage_out(reinterpret_cast<uint8_t*>(p), 6 * n, r, lane);
  } else {  // R_CHW: the general form writes straight to memory
    for (int c = 0; c < 3; ++c) stage_out(reinterpret_cast<uint8_t*>(p + c * ch), 2 * n, r + c * R_SEG, lane);
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void residual_front_u16_kernel(const uint16_t* __restrict__ base, RStride bs,
                                                                 int bpath, const uint16_t* __restrict__ xin,
                                                                 RStride xs, int xpath, int depth, int tau,
                                                                 uint32_t magic, int shift, int H, int W, FrontOut o,
                                                                 int tiles_x, int tiles_y) {
  constexpr bool HAS_X = MODE != F_CTX, CTX = MODE != F_STATS, FULL = MODE == F_FULL;
  __shared__ uint32_t SB[RF_ROWS + 2][R_ROW];
  __shared__ uint32_t SX[HAS_X ? RF_ROWS : 1][R_ROW];
  __shared__ unsigned int Hh[FULL ? RES_CTX * RES_BINS : 1];
  __shared__ unsigned int Cc[RES_CTX];
  __shared__ unsigned long long redD[4], redS[4];
  __shared__ unsigned int redM[4], redQ[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (FULL)
    for (int k = tid; k < RES_CTX * RES_BINS; k += 256) Hh[k] = 0;
  if (tid < RES_CTX) Cc[tid] = 0;
  const int64_t t = blockIdx.x;
  const int64_t ry = t / tiles_x;
  const int x0 = (int)(t - ry * tiles_x) * R_TW;  // < W: the tiles cover the image only
  const int64_t img = ry / tiles_y;
  const int yb = (int)(ry - img * tiles_y) * (RF_ROWS * RF_GROUPS);
  const int nx = min(R_TW, W - x0);
  const int xa = max(x0 - 1, 0), ns = min(x0 + nx + 1, W) - xa;  // the staged base columns [xa, xa + ns)
  const bool wave_on = 64 * wave < nx;  // the same for a whole wave: its 64-column group exists
  const bool active = tid < nx;
  const int x = x0 + tid;
  // this thread's three columns in the staged segment (clamped into the image, hence into the segment; a lane beyond
  // the image reads the last column and writes nothing)
  const int kl = min(max(x - 1, 0), W - 1) - xa, km = min(x, W - 1) - xa, kr = min(x + 1, W - 1) - xa;
  const int kx = min(tid, nx - 1);
  const int step = 2 * tau + 1, maxv = (1 << depth) - 1, cshift = depth - 8;
  const int bmul = bpath == R_HWC ? 6 : 2, xmul = xpath == R_HWC ? 6 : 2;
  const uint8_t* SB8 = reinterpret_cast<const uint8_t*>(&SB[0][0]);
  const uint8_t* SX8 = reinterpret_cast<const uint8_t*>(&SX[0][0]);
  const uint16_t* bimg = base + img * bs.img + (int64_t)xa * bs.col;
  const uint16_t* ximg = HAS_X ? xin + img * xs.img + (int64_t)x0 * xs.col : nullptr;
  const int64_t plane = (int64_t)H * W;
  const int64_t G = (W + 63) / 64, grp = x0 / 64 + wave;
  unsigned long long* lo_plane = FULL && shift ? o.plane + img * (3 * (int64_t)H * G * shift) : nullptr;

  unsigned long long cnt[3] = {0, 0, 0};  // 8 classes x 8 bits per channel
  unsigned long long dsum = 0, qsum = 0;
  unsigned int merr = 0, qmax = 0;
  int key[3] = {0, 0, 0};  // the run of equal histogram keys per channel
  unsigned int run[3] = {0, 0, 0};

  for (int g = 0; g < RF_GROUPS; ++g) {
    const int y0 = yb + g * RF_ROWS;
    if (y0 >= H) break;  // the same for the whole block
    const int rows = min(RF_ROWS, H - y0);
    __syncthreads();  // the last group's reads (the first time: the zeroing above) are done
    for (int r = wave; r < rows + 2; r += 4) {
      const int yc = min(max(y0 - 1 + r, 0), H - 1);
      seg_in(bpath, bimg + (int64_t)yc * bs.row, bs.col, bs.ch, ns, SB[r], lane);
    }
    if (HAS_X)
      for (int r = wave; r < rows; r += 4)
        seg_in(xpath, ximg + (int64_t)(y0 + r) * xs.row, xs.col, xs.ch, nx, SX[r], lane);
    __syncthreads();
    if (wave_on) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        int mn0 = 0, mx0 = 0, mn1 = 0, mx1 = 0, mid1 = 0;
        // staged row r of channel c: the sliding window's new row, and from r = 2 on the output of row r - 2
        for (int r = 0; r < rows + 2; ++r) {
          const int yc = min(max(y0 - 1 + r, 0), H - 1);
          const uint8_t* row = SB8 + r * (R_ROW * 4) + seg_at(bpath, bimg + (int64_t)yc * bs.row, bs.ch, c);
          const int vm = min(word_at(row, bmul * km), maxv);
          int mn2 = vm, mx2 = vm;
          if (CTX) {
            const int vl = min(word_at(row, bmul * kl), maxv), vr = min(word_at(row, bmul * kr), maxv);
            mn2 = min(vl, min(vm, vr)), mx2 = max(vl, max(vm, vr));
          }
          if (r >= 2) {
            const int y = y0 + r - 2;
            const int64_t i = c * plane + (int64_t)y * W + x;
            int cx = 0;
            if (CTX) {
              const int a = (max(mx0, max(mx1, mx2)) - min(mn0, min(mn1, mn2))) >> cshift;  // <= 255
              const int cls = a < 2 ? 0 : 31 - __clz(a);
              cx = 8 * c + cls;
              if (active) {
                o.ctx[img * 3 * plane + i] = (uint8_t)cx;
                cnt[c] += 1ull << (8 * cls);
                dsum += residual_digest_term(mid1, (uint64_t)i);
              }
            }
            if (HAS_X) {
              const uint8_t* xrow = SX8 + (r - 2) * (R_ROW * 4) + seg_at(xpath, ximg + (int64_t)y * xs.row, xs.ch, c);
              const int xv = min(word_at(xrow, xmul * kx), maxv);
              const int q = residual16_quant(xv, mid1, tau, magic);
              const unsigned int aq = (unsigned int)abs(q);
              int lo = 0;
              if (active) {
                qmax = max(qmax, aq);
                qsum += aq;
              }
              if (FULL) {
                const int hi = q >> shift;
                if (active) {
                  lo = q - hi * (1 << shift);
                  const int rec = min(max(mid1 + q * step, 0), maxv);
                  merr = max(merr, (unsigned int)abs(xv - rec));
                  o.sym[img * 3 * plane + i] = (int16_t)residual16_sat(hi);
                  const int k = cx * RES_BINS + residual_bin(hi);
                  if (k == key[c]) {
                    ++run[c];
                  } else {
                    if (run[c]) atomicAdd(&Hh[key[c]], run[c]);
                    key[c] = k;
                    run[c] = 1;
                  }
                }
                if (shift) {  // every lane of the wave is here: one ballot per bit of lo
                  unsigned long long mine = 0;
                  for (int j = 0; j < shift; ++j) {
                    const unsigned long long b = __ballot((lo >> j) & 1);
                    if (lane == j) mine = b;
                  }
                  if (lane < shift) lo_plane[(((int64_t)c * H + y) * G + grp) * shift + lane] = mine;
                }
              }
            }
          }
          mn0 = mn1, mx0 = mx1, mn1 = mn2, mx1 = mx2, mid1 = vm;
        }
      }
    }
  }
  if (FULL) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (run[c]) atomicAdd(&Hh[key[c]], run[c]);
  }
  if (CTX) {
    // counts: 8-bit fields -> two words of 16-bit fields (a wave's sum is at most 64 * 64 per field)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const unsigned long long even = wave_sum64(cnt[c] & 0x00ff00ff00ff00ffull);
      const unsigned long long odd = wave_sum64((cnt[c] >> 8) & 0x00ff00ff00ff00ffull);
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const unsigned int e = (unsigned int)(even >> (16 * k)) & 0xffffu, od = (unsigned int)(odd >> (16 * k)) & 0xffffu;
          if (e) atomicAdd(&Cc[8 * c + 2 * k], e);
          if (od) atomicAdd(&Cc[8 * c + 2 * k + 1], od);
        }
      }
    }
  }
  dsum = wave_sum64(dsum);
  qsum = wave_sum64(qsum);
  merr = wave_max32(merr);
  qmax = wave_max32(qmax);
  if (lane == 0) {
    redD[wave] = dsum;
    redS[wave] = qsum;
    redM[wave] = merr;
    redQ[wave] = qmax;
  }
  __syncthreads();
  if (tid == 0) {
    if (CTX) atomicAdd(o.digest + img, sum4(redD) * RES_DIGEST_K);
    if (HAS_X) {
      const unsigned int mq = max4(redQ);
      const unsigned long long sq = sum4(redS);
      if (mq) atomicMax(o.max_abs_q + img, mq);
      if (sq) atomicAdd(o.sum_abs_q + img, sq);
    }
    if (FULL) {
      const unsigned int m = max4(redM);
      if (m) atomicMax(o.max_err + img, m);
    }
  }
  if (CTX && tid < RES_CTX && Cc[tid]) atomicAdd(o.ctx_count + img * RES_CTX + tid, Cc[tid]);
  if (FULL)
    for (int k = tid; k < RES_CTX * RES_BINS; k += 256) {
      const unsigned int v = Hh[k];
      if (v) atomicAdd(o.hist + img * (RES_CTX * RES_BINS) + k, v);
    }
}

template <bool REF>
__global__ __launch_bounds__(256) void residual_apply_u16_kernel(
    const uint16_t* __restrict__ base, RStride bs, int bpath, const int16_t* __restrict__ sym,
    const unsigned long long* __restrict__ lo_plane, int depth, int tau, int shift, int H, int W,
    uint16_t* __restrict__ out, RStride os, int opath, const uint16_t* __restrict__ ref, RStride rs, int rpath,
    unsigned long long* __restrict__ sq_err, unsigned int* __restrict__ max_err, unsigned int* __restrict__ status,
    int tiles_x, int tiles_y) {
  __shared__ uint32_t SB[RA_ROWS][R_ROW];
  __shared__ uint32_t SO[RA_ROWS][R_ROW];
  __shared__ uint32_t SR[REF ? RA_ROWS : 1][R_ROW];
  __shared__ unsigned long long redS[RA_ROWS];
  __shared__ unsigned int redM[RA_ROWS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int NG = REF ? RA_REF_GROUPS : 1;
  const int64_t t = blockIdx.x;
  const int64_t ry = t / tiles_x;
  const int x0 = (int)(t - ry * tiles_x) * R_TW;
  const int64_t img = ry / tiles_y;
  const int yb = (int)(ry - img * tiles_y) * (NG * RA_ROWS) + wave;
  const int step = 2 * tau + 1, maxv = (1 << depth) - 1;
  const int bmul = bpath == R_HWC ? 6 : 2, omul = opath == R_HWC ? 6 : 2, rmul = rpath == R_HWC ? 6 : 2;
  const uint8_t* SB8 = reinterpret_cast<const uint8_t*>(SB[wave]);
  const uint8_t* SR8 = reinterpret_cast<const uint8_t*>(SR[REF ? wave : 0]);
  uint8_t* SO8 = reinterpret_cast<uint8_t*>(SO[wave]);
  const int64_t plane = (int64_t)H * W;
  const int64_t G = (W + 63) / 64, grp0 = x0 / 64;
  const unsigned long long* lo_img = shift ? lo_plane + img * (3 * (int64_t)H * G * shift) : nullptr;
  unsigned long long acc = 0;  // a squared difference takes 32 bits
  unsigned int merr = 0;
  bool bad = false;
  for (int g = 0; g < NG; ++g) {
    const int y = yb + g * RA_ROWS;
    const int nx = y < H ? min(R_TW, W - x0) : 0;
    const uint16_t* brow = base + img * bs.img + (int64_t)y * bs.row + (int64_t)x0 * bs.col;  // used when nx > 0
    uint16_t* orow = out + img * os.img + (int64_t)y * os.row + (int64_t)x0 * os.col;
    const uint16_t* rrow = REF ? ref + img * rs.img + (int64_t)y * rs.row + (int64_t)x0 * rs.col : nullptr;
    // the symbols and the low bits do not depend on the staging: loaded first, so their latency overlaps it
    int16_t qv[3][R_TW / 64];
    unsigned long long lw[3][R_TW / 64];  // lane k < shift: word k of the group's low bits
    if (nx > 0) {
      const int16_t* srow = sym + img * 3 * plane + (int64_t)y * W + x0;
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < R_TW / 64; ++j) {
          qv[c][j] = lane + 64 * j < nx ? srow[c * plane + lane + 64 * j] : (int16_t)0;
          lw[c][j] = lane < shift && 64 * j < nx ? lo_img[(((int64_t)c * H + y) * G + grp0 + j) * shift + lane] : 0ull;
        }
      seg_in(bpath, brow, bs.col, bs.ch, nx, SB[wave], lane);
      if (REF) seg_in(rpath, rrow, rs.col, rs.ch, nx, SR[wave], lane);
    }
    __syncthreads();
    if (nx > 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int bat = seg_at(bpath, brow, bs.ch, c);
        const int oat = opath == R_GENERAL ? 0 : seg_at(opath, orow, os.ch, c);
        const int rat = REF ? seg_at(rpath, rrow, rs.ch, c) : 0;
#pragma unroll
        for (int j = 0; j < R_TW / 64; ++j) {
          if (64 * j >= nx) break;  // the same for the whole wave
          const int px = lane + 64 * j;
          int lo = 0;
          for (int k = 0; k < shift; ++k) {  // every lane of the wave: lane k's word, this lane's bit
            const unsigned long long w = __shfl(lw[c][j], k, 64);
            lo |= (int)((w >> lane) & 1ull) << k;
          }
          if (px < nx) {
            const int b = min(word_at(SB8, bat + bmul * px), maxv);
            int hi = qv[c][j];
            if (hi < -RES16_MAX_HI || hi > RES16_MAX_HI) {  // no well-formed string holds it: refused, not applied
              bad = true;
              hi = 0;
              lo = 0;
            }
            const int q = hi * (1 << shift) + lo;
            const int rec = min(max(b + q * step, 0), maxv);
            if (opath == R_GENERAL) orow[(int64_t)px * os.col + c * os.ch] = (uint16_t)rec;
            else *reinterpret_cast<uint16_t*>(SO8 + oat + omul * px) = (uint16_t)rec;
            if (REF) {
              const int d = rec - min(word_at(SR8, rat + rmul * px), maxv);
              acc += (unsigned long long)((int64_t)d * d);
              merr = max(merr, (unsigned int)abs(d));
            }
          }
        }
      }
    }
    __syncthreads();
    if (opath != R_GENERAL && nx > 0) seg_out(opath, orow, os.ch, nx, SO[wave], lane);
    if (NG > 1) __syncthreads();  // the next group's words go into the same LDS
  }
  if (__any(bad) && lane == 0) atomicOr(status + img, 1u);
  if (REF) {
    const unsigned long long s = wave_sum64(acc);
    merr = wave_max32(merr);
    if (lane == 0) {
      redS[wave] = s;
      redM[wave] = merr;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned long long tot = sum4(redS);
      const unsigned int m = max4(redM);
      if (tot) atomicAdd(sq_err + img, tot);
      if (m) atomicMax(max_err + img, m);
    }
  }
}

void front_common(const char* what, const uint16_t* base, const int64_t* b, int B, int H, int W, int depth, int tau) {
  const std::string w(what);
  MLIC_CHECK(base != nullptr, w + ": null base");
  MLIC_CHECK(b != nullptr, w + ": null base strides");
  MLIC_CHECK(B >= 1, w + ": B must be positive");
  MLIC_CHECK(H >= 1 && W >= 1, w + ": H and W must be positive");
  MLIC_CHECK(depth >= RES16_MIN_DEPTH && depth <= RES16_MAX_DEPTH, w + ": depth must be in 9..16");
  MLIC_CHECK(tau >= 0 && tau <= RES_MAX_TAU, w + ": tau must be in 0..127");
  MLIC_CHECK(b[2] != 0 && b[3] != 0, w + ": zero column or channel stride (base)");
  MLIC_CHECK(aligned(base, 2), w + ": base must be 2-byte aligned");
}

}  // namespace

void image_residual_front_u16(const uint16_t* base, const int64_t* b, const uint16_t* x, const int64_t* xs, int B,
                              int H, int W, int depth, int tau, int shift, uint8_t* ctx, uint32_t* ctx_count,
                              uint64_t* digest, int16_t* sym, uint64_t* lo_plane, uint32_t* hist, uint32_t* max_err,
                              uint32_t* max_abs_q, uint64_t* sum_abs_q, hipStream_t st) {
  front_common("image_residual_front_u16", base, b, B, H, W, depth, tau);
  const std::string w("image_residual_front_u16");
  check_front_out(w, ctx, ctx_count, digest);
  if (x != nullptr) {
    MLIC_CHECK(xs != nullptr, "image_residual_front_u16: x needs strides");
    MLIC_CHECK(xs[2] != 0 && xs[3] != 0, "image_residual_front_u16: zero column or channel stride (x)");
    MLIC_CHECK(aligned(x, 2), "image_residual_front_u16: x must be 2-byte aligned");
    MLIC_CHECK(shift >= 0 && shift <= residual16_max_shift(depth),
               "image_residual_front_u16: shift must be in 0..depth - 7");
    check_front_x_needed(w, sym, hist, max_err, max_abs_q, sum_abs_q);
    MLIC_CHECK((lo_plane != nullptr) == (shift > 0), "image_residual_front_u16: lo_plane goes with a shift above 0");
    check_front_x_aligned(w, sym, lo_plane, hist, max_err, max_abs_q, sum_abs_q);
  } else {
    check_front_without_x(w, sym, lo_plane, hist, max_err, max_abs_q, sum_abs_q);
  }
  int tx, ty;
  const unsigned blocks = r_blocks(B, H, W, RF_ROWS * RF_GROUPS, &tx, &ty, "image_residual_front_u16");
  const RStride bs{b[0], b[1], b[2], b[3]};
  const RStride xr = x ? RStride{xs[0], xs[1], xs[2], xs[3]} : RStride{0, 0, 0, 0};
  const FrontOut o{ctx, ctx_count, reinterpret_cast<unsigned long long*>(digest), sym,
                   reinterpret_cast<unsigned long long*>(lo_plane), hist, max_err, max_abs_q,
                   reinterpret_cast<unsigned long long*>(sum_abs_q)};
  // the sums start from zero: zeroed here, on the stream
  HIP_OK(hipMemsetAsync(ctx_count, 0, sizeof(uint32_t) * RES_CTX * (size_t)B, st));
  HIP_OK(hipMemsetAsync(digest, 0, sizeof(uint64_t) * (size_t)B, st));
  const uint32_t magic = residual16_magic(2 * tau + 1);
  if (x) {
    HIP_OK(hipMemsetAsync(hist, 0, sizeof(uint32_t) * RES_CTX * RES_BINS * (size_t)B, st));
    HIP_OK(hipMemsetAsync(max_err, 0, sizeof(uint32_t) * (size_t)B, st));
    HIP_OK(hipMemsetAsync(max_abs_q, 0, sizeof(uint32_t) * (size_t)B, st));
    HIP_OK(hipMemsetAsync(sum_abs_q, 0, sizeof(uint64_t) * (size_t)B, st));
    hipLaunchKernelGGL(residual_front_u16_kernel<F_FULL>, dim3(blocks), dim3(256), 0, st, base, bs, r_path(b), x, xr,
                       r_path(xs), depth, tau, magic, shift, H, W, o, tx, ty);
  } else {
    hipLaunchKernelGGL(residual_front_u16_kernel<F_CTX>, dim3(blocks), dim3(256), 0, st, base, bs, r_path(b), x, xr,
                       R_GENERAL, depth, tau, magic, 0, H, W, o, tx, ty);
  }
  HIP_OK(hipGetLastError());
}

void image_residual_stats_u16(const uint16_t* base, const int64_t* b, const uint16_t* x, const int64_t* xs, int B,
                              int H, int W, int depth, int tau, uint32_t* max_abs_q, uint64_t* sum_abs_q,
                              hipStream_t st) {
  front_common("image_residual_stats_u16", base, b, B, H, W, depth, tau);
  MLIC_CHECK(x != nullptr && xs != nullptr, "image_residual_stats_u16: null x or x strides");
  MLIC_CHECK(xs[2] != 0 && xs[3] != 0, "image_residual_stats_u16: zero column or channel stride (x)");
  MLIC_CHECK(aligned(x, 2), "image_residual_stats_u16: x must be 2-byte aligned");
  MLIC_CHECK(max_abs_q != nullptr && sum_abs_q != nullptr, "image_residual_stats_u16: null max_abs_q or sum_abs_q");
  MLIC_CHECK(aligned(max_abs_q, 4) && aligned(sum_abs_q, 8),
             "image_residual_stats_u16: max_abs_q must be 4-byte and sum_abs_q 8-byte aligned");
  int tx, ty;
  const unsigned blocks = r_blocks(B, H, W, RF_ROWS * RF_GROUPS, &tx, &ty, "image_residual_stats_u16");
  const RStride bs{b[0], b[1], b[2], b[3]}, xr{xs[0], xs[1], xs[2], xs[3]};
  const FrontOut o{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, max_abs_q,
                   reinterpret_cast<unsigned long long*>(sum_abs_q)};
  HIP_OK(hipMemsetAsync(max_abs_q, 0, sizeof(uint32_t) * (size_t)B, st));
  HIP_OK(hipMemsetAsync(sum_abs_q, 0, sizeof(uint64_t) * (size_t)B, st));
  hipLaunchKernelGGL(residual_front_u16_kernel<F_STATS>, dim3(blocks), dim3(256), 0, st, base, bs, r_path(b), x, xr,
                     r_path(xs), depth, tau, residual16_magic(2 * tau + 1), 0, H, W, o, tx, ty);
  HIP_OK(hipGetLastError());
}

void image_residual_apply_u16(const uint16_t* base, const int64_t* b, const int16_t* sym, const uint64_t* lo_plane,
                              int B, int H, int W, int depth, int tau, int shift, uint16_t* out, const int64_t* o,
                              const uint16_t* ref, const int64_t* r, uint64_t* sq_err, uint32_t* max_err,
                              uint32_t* status, hipStream_t st) {
  front_common("image_residual_apply_u16", base, b, B, H, W, depth, tau);
  MLIC_CHECK(sym != nullptr, "image_residual_apply_u16: null sym");
  MLIC_CHECK(out != nullptr && o != nullptr, "image_residual_apply_u16: null out or out strides");
  MLIC_CHECK(status != nullptr, "image_residual_apply_u16: null status");
  MLIC_CHECK(shift >= 0 && shift <= residual16_max_shift(depth),
             "image_residual_apply_u16: shift must be in 0..depth - 7");
  MLIC_CHECK((lo_plane != nullptr) == (shift > 0), "image_residual_apply_u16: lo_plane goes with a shift above 0");
  MLIC_CHECK(o[2] != 0 && o[3] != 0, "image_residual_apply_u16: zero column or channel stride (out)");
  MLIC_CHECK(aligned(sym, 2) && aligned(out, 2) && aligned(lo_plane, 8) && aligned(status, 4),
             "image_residual_apply_u16: sym and out must be 2-byte, lo_plane 8-byte and status 4-byte aligned");
  check_apply_scores("image_residual_apply_u16", ref != nullptr, sq_err, max_err);
  MLIC_CHECK(ref == nullptr || (r != nullptr && r[2] != 0 && r[3] != 0),
             "image_residual_apply_u16: ref needs strides with nonzero column and channel stride");
  MLIC_CHECK(aligned(ref, 2) && aligned(sq_err, 8) && aligned(max_err, 4),
             "image_residual_apply_u16: ref must be 2-byte, sq_err 8-byte and max_err 4-byte aligned");
  int tx, ty;
  const unsigned blocks = r_blocks(B, H, W, (ref ? RA_REF_GROUPS : 1) * RA_ROWS, &tx, &ty, "image_residual_apply_u16");
  const RStride bs{b[0], b[1], b[2], b[3]}, os{o[0], o[1], o[2], o[3]};
  const RStride rr = ref ? RStride{r[0], r[1], r[2], r[3]} : RStride{0, 0, 0, 0};
  auto* sq64 = reinterpret_cast<unsigned long long*>(sq_err);
  auto* lo64 = reinterpret_cast<const unsigned long long*>(lo_plane);
  HIP_OK(hipMemsetAsync(status, 0, sizeof(uint32_t) * (size_t)B, st));
  if (ref) {
    HIP_OK(hipMemsetAsync(sq_err, 0, sizeof(uint64_t) * (size_t)B, st));
    HIP_OK(hipMemsetAsync(max_err, 0, sizeof(uint32_t) * (size_t)B, st));
    hipLaunchKernelGGL(residual_apply_u16_kernel<true>, dim3(blocks), dim3(256), 0, st, base, bs, r_path(b), sym, lo64,
                       depth, tau, shift, H, W, out, os, r_path(o), ref, rr, r_path(r), sq64, max_err, status, tx, ty);
  } else {
    hipLaunchKernelGGL(residual_apply_u16_kernel<false>, dim3(blocks), dim3(256), 0, st, base, bs, r_path(b), sym,
                       lo64, depth, tau, shift, H, W, out, os, r_path(o), ref, rr, R_GENERAL, sq64, max_err, status, tx,
                       ty);
  }
  HIP_OK(hipGetLastError());
}

}  // namespace mlic
