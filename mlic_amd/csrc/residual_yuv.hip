// Residual coding of Y'CbCr frames: the two passes over the planes of a frame (residual_yuv.h has the definitions;
// DESIGN.md section 5 "Residual coding", "Y'CbCr frames").  The structure is residual16.hip's with a plane as that
// kernel's image of one channel: the HWC / CHW forms go, the column stride comes.
//
// residual_front_planes: the base planes (and, for the encoder, the original planes x) -> the context plane, the
// per-context counts and the digest of base; with x also hi (the symbol plane), the low-bit plane, the histograms of
// hi, the largest |x - rec| and the statistics max|q| and sum|q|.  A statistics launch gives the last two alone.
// residual_apply_planes: base + hi + low-bit plane -> the three output planes, optionally scored against reference
// planes, per plane.
//
// One launch covers the three planes of all B frames: a frame has nb_0 + 2 nb_1 blocks (nb_p the blocks of plane p)
// and the block index maps to (frame, plane, tile) by two comparisons against them.
// Each plane comes as a pointer and element strides {image, row, column}.  Column stride 1 is a dense row, staged
// through LDS with image_stage.h (whole dwords).  Column stride 2 is the semi-planar case (NV12 / NV21 / P010,
// cr = cb + 1): the interleaved pair row between the segment's first and last sample is staged the same way and the
// plane's samples are picked out of LDS.  Any other stride is gathered.  On the way out a dense row is staged, any
// other stride is stored sample by sample (a staged pair row would write the other plane's samples).
//
// front: 256 threads, one column each, PF_GROUPS groups of PF_ROWS rows; per group PF_ROWS + 2 base rows and PF_ROWS
// rows of x are staged.  A 256-column tile starts on a multiple of 64, so a wave is one 64-column group of the
// low-bit plane: bit j of lo is one ballot, lane j keeps word j, and lanes 0..s-1 store the group's s words of a row.
// Lanes beyond the plane take part with lo = 0, which is the plane's zero padding.
#include "image_stage.h"
#include "kernels.h"
#include "residual_dev.h"
#include "residual_yuv.h"

namespace mlic {

namespace {

constexpr int P_TW = R_TW;                      // columns of a row segment
constexpr int PF_ROWS = 8, PF_GROUPS = 8;       // front: rows per group, groups per block
constexpr int PA_ROWS = 4, PA_REF_GROUPS = 16;  // apply: a row per wave; with ref a block walks 16 groups
enum { P_GENERAL = 0, P_DENSE = 1, P_PAIR = 2 };
static_assert(PF_ROWS * PF_GROUPS <= 255, "a thread's packed class counts are 8 bits each");
static_assert(P_TW % 64 == 0, "a wave is one 64-column group of the low-bit plane");

// dwords of a staged row: the pair row of P_TW + 2 samples (2 (P_TW + 2) - 1 words) at any alignment
template <typename WORD>
constexpr int seg_dwords() {
  return ((int)sizeof(WORD) * 2 * (P_TW + 2) + 3 + 3) / 4;
}

template <typename WORD>
struct PlaneSet {  // the three planes of a frame batch
  WORD* p[3];
  int64_t img[3], row[3], col[3];
  int path[3];
};

struct PGeom {  // the launch's sizes: plane 0 and planes 1, 2
  int H, W, hc, wc;
  int tx0, tx1;       // column tiles of a row
  unsigned nb0, nb1;  // blocks of a plane
};

template <typename T>
__device__ inline T sel(const T (&a)[3], int p) {  // p is the same for a block: two selects, no indexed access
  return p == 0 ? a[0] : p == 1 ? a[1] : a[2];
}

int p_path(int64_t col) { return col == 1 ? P_DENSE : col == 2 ? P_PAIR : P_GENERAL; }

// n samples from p (the segment's first sample) into the staged row r: one wave
template <typename WORD>
__device__ inline void seg_in(int path, const WORD* __restrict__ p, int64_t col, int n, uint32_t* r, int lane) {
  if (path == P_DENSE) {
    stage_in(reinterpret_cast<const uint8_t*>(p), (int)sizeof(WORD) * n, r, lane);
  } else if (path == P_PAIR) {  // the interleaved words from the first sample to the last, the other plane's between
    stage_in(reinterpret_cast<const uint8_t*>(p), (int)sizeof(WORD) * (2 * n - 1), r, lane);
  } else {
    WORD* rw = reinterpret_cast<WORD*>(r);
    for (int k = lane; k < n; k += 64) rw[k] = p[(int64_t)k * col];
  }
}

// where sample k sits in the staged row: byte seg_at(...) + seg_mul(...) k
template <typename WORD>
__device__ inline int seg_at(int path, const WORD* p) {
  return path == P_GENERAL ? 0 : addr_mod4(p);
}
template <typename WORD>
__device__ inline int seg_mul(int path) {
  return (int)sizeof(WORD) * (path == P_PAIR ? 2 : 1);
}

template <typename WORD>
__device__ inline int word_at(const uint8_t* row, int byte) {
  return *reinterpret_cast<const WORD*>(row + byte);
}

// what a block works on: frame, plane and the plane's sizes and places in the frame's canonical order
struct BlockAt {
  int64_t img;
  int p, Hp, Wp, x0, ty;
  int64_t off, N;            // canonical index of the plane's first sample; samples of a frame
  int64_t G, rowbase, groups;  // 64-column groups: of a row, before the plane's first row, of a frame
};

__device__ inline BlockAt block_at(const PGeom& g) {
  BlockAt a;
  const unsigned per = g.nb0 + 2 * g.nb1;
  a.img = blockIdx.x / per;
  unsigned r = blockIdx.x - (unsigned)a.img * per;
  a.p = (r >= g.nb0 ? 1 : 0) + (r >= g.nb0 + g.nb1 ? 1 : 0);
  r -= a.p == 0 ? 0u : a.p == 1 ? g.nb0 : g.nb0 + g.nb1;
  a.Hp = a.p ? g.hc : g.H;
  a.Wp = a.p ? g.wc : g.W;
  const int tx = a.p ? g.tx1 : g.tx0;
  a.ty = (int)(r / (unsigned)tx);
  a.x0 = (int)(r - (unsigned)a.ty * (unsigned)tx) * P_TW;  // < Wp: the tiles cover the plane only
  const int64_t n0 = (int64_t)g.H * g.W, n1 = (int64_t)g.hc * g.wc;
  const int64_t G0 = (g.W + 63) / 64, G1 = (g.wc + 63) / 64;
  a.N = n0 + 2 * n1;
  a.off = a.p == 0 ? 0 : a.p == 1 ? n0 : n0 + n1;
  a.G = a.p ? G1 : G0;
  a.rowbase = a.p == 0 ? 0 : a.p == 1 ? g.H * G0 : g.H * G0 + g.hc * G1;
  a.groups = g.H * G0 + 2 * g.hc * G1;
  return a;
}

template <typename WORD, int MODE>
__global__ __launch_bounds__(256) void residual_front_planes_kernel(PlaneSet<const WORD> base, PlaneSet<const WORD> xin,
                                                                    int depth, int shr, int tau, uint32_t magic,
                                                                    int shift, PGeom geom, FrontOut o) {
  constexpr bool HAS_X = MODE != F_CTX, CTX = MODE != F_STATS, FULL = MODE == F_FULL;
  constexpr int SEG = seg_dwords<WORD>();
  __shared__ uint32_t SB[PF_ROWS + 2][SEG];
  __shared__ uint32_t SX[HAS_X ? PF_ROWS : 1][SEG];
  __shared__ unsigned int Hh[FULL ? 8 * RES_BINS : 1];  // the plane's eight contexts
  __shared__ unsigned int Cc[8];
  __shared__ unsigned long long redD[4], redS[4];
  __shared__ unsigned int redM[4], redQ[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (FULL)
    for (int k = tid; k < 8 * RES_BINS; k += 256) Hh[k] = 0;
  if (tid < 8) Cc[tid] = 0;
  const BlockAt at = block_at(geom);
  const int p = at.p, H = at.Hp, W = at.Wp, x0 = at.x0;
  const int64_t img = at.img;
  const int yb = at.ty * (PF_ROWS * PF_GROUPS);
  const int nx = min(P_TW, W - x0);
  const int xa = max(x0 - 1, 0), ns = min(x0 + nx + 1, W) - xa;  // the staged base columns [xa, xa + ns)
  const bool wave_on = 64 * wave < nx;  // the same for a whole wave: its 64-column group exists
  const bool active = tid < nx;
  const int x = x0 + tid;
  // this thread's three columns in the staged segment (clamped into the plane, hence into the segment; a lane beyond
  // the plane reads the last column and writes nothing)
  const int kl = min(max(x - 1, 0), W - 1) - xa, km = min(x, W - 1) - xa, kr = min(x + 1, W - 1) - xa;
  const int kx = min(tid, nx - 1);
  const int step = 2 * tau + 1, maxv = (1 << depth) - 1, cshift = depth - 8;
  const int bpath = sel(base.path, p), xpath = HAS_X ? sel(xin.path, p) : P_GENERAL;
  const int64_t brow_s = sel(base.row, p), bcol = sel(base.col, p);
  const int64_t xrow_s = HAS_X ? sel(xin.row, p) : 0, xcol = HAS_X ? sel(xin.col, p) : 0;
  const int bmul = seg_mul<WORD>(bpath), xmul = seg_mul<WORD>(xpath);
  const uint8_t* SB8 = reinterpret_cast<const uint8_t*>(&SB[0][0]);
  const uint8_t* SX8 = reinterpret_cast<const uint8_t*>(&SX[0][0]);
  const WORD* bimg = sel(base.p, p) + img * sel(base.img, p) + (int64_t)xa * bcol;
  const WORD* ximg = HAS_X ? sel(xin.p, p) + img * sel(xin.img, p) + (int64_t)x0 * xcol : nullptr;
  const int64_t grp = x0 / 64 + wave;
  unsigned long long* lo_plane = FULL && shift ? o.plane + img * (at.groups * shift) : nullptr;

  unsigned long long cnt = 0;  // 8 classes x 8 bits
  unsigned long long dsum = 0, qsum = 0;
  unsigned int merr = 0, qmax = 0;
  int key = 0;  // the run of equal histogram keys
  unsigned int run = 0;

  for (int g = 0; g < PF_GROUPS; ++g) {
    const int y0 = yb + g * PF_ROWS;
    if (y0 >= H) break;  // the same for the whole block
    const int rows = min(PF_ROWS, H - y0);
    __syncthreads();  // the last group's reads (the first time: the zeroing above) are done
    for (int r = wave; r < rows + 2; r += 4) {
      const int yc = min(max(y0 - 1 + r, 0), H - 1);
      seg_in<WORD>(bpath, bimg + (int64_t)yc * brow_s, bcol, ns, SB[r], lane);
    }
    if (HAS_X)
      for (int r = wave; r < rows; r += 4) seg_in<WORD>(xpath, ximg + (int64_t)(y0 + r) * xrow_s, xcol, nx, SX[r], lane);
    __syncthreads();
    if (wave_on) {
      int mn0 = 0, mx0 = 0, mn1 = 0, mx1 = 0, mid1 = 0;
      // staged row r: the sliding window's new row, and from r = 2 on the output of row r - 2
      for (int r = 0; r < rows + 2; ++r) {
        const int yc = min(max(y0 - 1 + r, 0), H - 1);
        const uint8_t* row = SB8 + r * (SEG * 4) + seg_at<WORD>(bpath, bimg + (int64_t)yc * brow_s);
        const int vm = residual_yuv_sample(word_at<WORD>(row, bmul * km), shr, maxv);
        int mn2 = vm, mx2 = vm;
        if (CTX) {
          const int vl = residual_yuv_sample(word_at<WORD>(row, bmul * kl), shr, maxv);
          const int vr = residual_yuv_sample(word_at<WORD>(row, bmul * kr), shr, maxv);
          mn2 = min(vl, min(vm, vr)), mx2 = max(vl, max(vm, vr));
        }
        if (r >= 2) {
          const int y = y0 + r - 2;
          const int64_t i = at.off + (int64_t)y * W + x;
          int cls = 0;
          if (CTX) {
            const int a = (max(mx0, max(mx1, mx2)) - min(mn0, min(mn1, mn2))) >> cshift;  // <= 255
            cls = a < 2 ? 0 : 31 - __clz(a);
            if (active) {
              o.ctx[img * at.N + i] = (uint8_t)(8 * p + cls);
              cnt += 1ull << (8 * cls);
              dsum += residual_digest_term(mid1, (uint64_t)i);
            }
          }
          if (HAS_X) {
            const uint8_t* xrow = SX8 + (r - 2) * (SEG * 4) + seg_at<WORD>(xpath, ximg + (int64_t)y * xrow_s);
            const int xv = residual_yuv_sample(word_at<WORD>(xrow, xmul * kx), shr, maxv);
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
                o.sym[img * at.N + i] = (int16_t)residual16_sat(hi);
                const int k = cls * RES_BINS + residual_bin(hi);
                if (k == key) {
                  ++run;
                } else {
                  if (run) atomicAdd(&Hh[key], run);
                  key = k;
                  run = 1;
                }
              }
              if (shift) {  // every lane of the wave is here
                unsigned long long mine = 0;
                for (int j = 0; j < shift; ++j) {
                  const unsigned long long b = __ballot((lo >> j) & 1);
                  if (lane == j) mine = b;
                }
                if (lane < shift) lo_plane[(at.rowbase + (int64_t)y * at.G + grp) * shift + lane] = mine;
              }
            }
          }
        }
        mn0 = mn1, mx0 = mx1, mn1 = mn2, mx1 = mx2, mid1 = vm;
      }
    }
  }
  if (FULL && run) atomicAdd(&Hh[key], run);
  if (CTX) {
    // counts: 8-bit fields -> two words of 16-bit fields (a wave's sum is at most 64 * 64 per field)
    const unsigned long long even = wave_sum64(cnt & 0x00ff00ff00ff00ffull);
    const unsigned long long odd = wave_sum64((cnt >> 8) & 0x00ff00ff00ff00ffull);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned int e = (unsigned int)(even >> (16 * k)) & 0xffffu, od = (unsigned int)(odd >> (16 * k)) & 0xffffu;
        if (e) atomicAdd(&Cc[2 * k], e);
        if (od) atomicAdd(&Cc[2 * k + 1], od);
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
  if (CTX && tid < 8 && Cc[tid]) atomicAdd(o.ctx_count + img * RES_CTX + 8 * p + tid, Cc[tid]);
  if (FULL)
    for (int k = tid; k < 8 * RES_BINS; k += 256) {
      const unsigned int v = Hh[k];
      if (v) atomicAdd(o.hist + img * (RES_CTX * RES_BINS) + 8 * p * RES_BINS + k, v);
    }
}

template <typename WORD, bool REF>
__global__ __launch_bounds__(256) void residual_apply_planes_kernel(
    PlaneSet<const WORD> base, const int16_t* __restrict__ sym, const unsigned long long* __restrict__ lo_plane,
    int depth, int shr, int tau, int shift, PGeom geom, PlaneSet<WORD> out, PlaneSet<const WORD> ref,
    unsigned long long* __restrict__ sq_err, unsigned int* __restrict__ max_err, unsigned int* __restrict__ status) {
  constexpr int SEG = seg_dwords<WORD>();
  __shared__ uint32_t SB[PA_ROWS][SEG];
  __shared__ uint32_t SO[PA_ROWS][SEG];
  __shared__ uint32_t SR[REF ? PA_ROWS : 1][SEG];
  __shared__ unsigned long long redS[PA_ROWS];
  __shared__ unsigned int redM[PA_ROWS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int NG = REF ? PA_REF_GROUPS : 1;
  const BlockAt at = block_at(geom);
  const int p = at.p, H = at.Hp, W = at.Wp, x0 = at.x0;
  const int64_t img = at.img;
  const int yb = at.ty * (NG * PA_ROWS) + wave;
  const int step = 2 * tau + 1, maxv = (1 << depth) - 1;
  const int bpath = sel(base.path, p), opath = sel(out.path, p), rpath = REF ? sel(ref.path, p) : P_GENERAL;
  const int64_t bcol = sel(base.col, p), ocol = sel(out.col, p), rcol = REF ? sel(ref.col, p) : 0;
  const int bmul = seg_mul<WORD>(bpath), rmul = seg_mul<WORD>(rpath);
  const uint8_t* SB8 = reinterpret_cast<const uint8_t*>(SB[wave]);
  const uint8_t* SR8 = reinterpret_cast<const uint8_t*>(SR[REF ? wave : 0]);
  uint8_t* SO8 = reinterpret_cast<uint8_t*>(SO[wave]);
  const WORD* bimg = sel(base.p, p) + img * sel(base.img, p) + (int64_t)x0 * bcol;
  WORD* oimg = sel(out.p, p) + img * sel(out.img, p) + (int64_t)x0 * ocol;
  const WORD* rimg = REF ? sel(ref.p, p) + img * sel(ref.img, p) + (int64_t)x0 * rcol : nullptr;
  const int64_t brow_s = sel(base.row, p), orow_s = sel(out.row, p), rrow_s = REF ? sel(ref.row, p) : 0;
  const int64_t grp0 = x0 / 64;
  const unsigned long long* lo_img = shift ? lo_plane + img * (at.groups * shift) : nullptr;
  unsigned long long acc = 0;  // a squared difference takes 32 bits
  unsigned int merr = 0;
  bool bad = false;
  for (int g = 0; g < NG; ++g) {
    const int y = yb + g * PA_ROWS;
    const int nx = y < H ? min(P_TW, W - x0) : 0;
    const WORD* brow = bimg + (int64_t)y * brow_s;  // used when nx > 0
    WORD* orow = oimg + (int64_t)y * orow_s;
    const WORD* rrow = REF ? rimg + (int64_t)y * rrow_s : nullptr;
    // the symbols and the low bits do not depend on the staging: loaded first, so their latency overlaps it
    int16_t qv[P_TW / 64];
    unsigned long long lw[P_TW / 64];  // lane k < shift: word k of the group's low bits
    if (nx > 0) {
      const int16_t* srow = sym + img * at.N + at.off + (int64_t)y * W + x0;
#pragma unroll
      for (int j = 0; j < P_TW / 64; ++j) {
        qv[j] = lane + 64 * j < nx ? srow[lane + 64 * j] : (int16_t)0;
        lw[j] = lane < shift && 64 * j < nx ? lo_img[(at.rowbase + (int64_t)y * at.G + grp0 + j) * shift + lane] : 0ull;
      }
      seg_in<WORD>(bpath, brow, bcol, nx, SB[wave], lane);
      if (REF) seg_in<WORD>(rpath, rrow, rcol, nx, SR[wave], lane);
    }
    __syncthreads();
    if (nx > 0) {
      const int bat = seg_at<WORD>(bpath, brow);
      const int oat = opath == P_DENSE ? addr_mod4(orow) : 0;
      const int rat = REF ? seg_at<WORD>(rpath, rrow) : 0;
#pragma unroll
      for (int j = 0; j < P_TW / 64; ++j) {
        if (64 * j >= nx) break;  // the same for the whole wave
        const int px = lane + 64 * j;
        int lo = 0;
        for (int k = 0; k < shift; ++k) {  // every lane of the wave: lane k's word, this lane's bit
          const unsigned long long w = __shfl(lw[j], k, 64);
          lo |= (int)((w >> lane) & 1ull) << k;
        }
        if (px < nx) {
          const int b = residual_yuv_sample(word_at<WORD>(SB8, bat + bmul * px), shr, maxv);
          int hi = qv[j];
          if (hi < -RES16_MAX_HI || hi > RES16_MAX_HI) {  // no well-formed string holds it: refused, written as base
            bad = true;
            hi = 0;
            lo = 0;
          }
          const int q = hi * (1 << shift) + lo;
          const int rec = min(max(b + q * step, 0), maxv);
          const WORD wv = (WORD)(rec << shr);
          if (opath == P_DENSE) *reinterpret_cast<WORD*>(SO8 + oat + (int)sizeof(WORD) * px) = wv;
          else orow[(int64_t)px * ocol] = wv;
          if (REF) {
            const int d = rec - residual_yuv_sample(word_at<WORD>(SR8, rat + rmul * px), shr, maxv);
            acc += (unsigned long long)((int64_t)d * d);
            merr = max(merr, (unsigned int)abs(d));
          }
        }
      }
    }
    __syncthreads();
    if (opath == P_DENSE && nx > 0) stage_out(reinterpret_cast<uint8_t*>(orow), (int)sizeof(WORD) * nx, SO[wave], lane);
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
      if (tot) atomicAdd(sq_err + img * 3 + p, tot);
      if (m) atomicMax(max_err + img, m);
    }
  }
}

PGeom p_geom(const std::string& w, int B, int H, int W, const YuvDesc* d, int block_rows, unsigned* blocks) {
  const ResYuvGeom g = residual_yuv_geom(H, W, d->sub_x, d->sub_y);
  PGeom q;
  q.H = H, q.W = W, q.hc = (int)g.h[1], q.wc = (int)g.w[1];
  q.tx0 = (W + P_TW - 1) / P_TW, q.tx1 = (q.wc + P_TW - 1) / P_TW;
  const int64_t nb0 = (int64_t)q.tx0 * ((H + block_rows - 1) / block_rows);
  const int64_t nb1 = (int64_t)q.tx1 * ((q.hc + block_rows - 1) / block_rows);
  const int64_t all = (int64_t)B * (nb0 + 2 * nb1);
  MLIC_CHECK(all <= 0x7fffffffLL, w + ": batch too large for one launch");
  q.nb0 = (unsigned)nb0, q.nb1 = (unsigned)nb1;
  *blocks = (unsigned)all;
  return q;
}

void desc_check(const std::string& w, const YuvDesc* d, int depth) {
  MLIC_CHECK(d != nullptr, w + ": null mlic_yuv_desc");
  MLIC_CHECK((d->sub_x == 1 || d->sub_x == 2) && (d->sub_y == 1 || d->sub_y == 2), w + ": sub_x and sub_y must be 1 or 2");
  MLIC_CHECK(!(d->sub_x == 1 && d->sub_y == 2), w + ": sub_x 1 with sub_y 2 (4:4:0) is not supported");
  if (depth == 8) MLIC_CHECK(d->matrix == 0 || d->matrix == 1, w + ": matrix must be 0 (BT.601) or 1 (BT.709)");
  else MLIC_CHECK(d->matrix >= 0 && d->matrix <= 2,
                  w + ": matrix must be 0 (BT.601), 1 (BT.709) or 2 (BT.2020 non-constant-luminance)");
  MLIC_CHECK(d->full_range == 0 || d->full_range == 1, w + ": full_range must be 0 or 1");
  MLIC_CHECK(d->site_x == 0 || d->site_x == 1, w + ": site_x must be 0 (centre) or 1 (left)");
  MLIC_CHECK(d->reserved[0] == 0 && d->reserved[1] == 0 && d->reserved[2] == 0, w + ": reserved fields must be 0");
}

// what the three calls share; word_bytes 1: depth 8, no alignment; 2: depth 9..16, msb 0 / 1
void common_check(const std::string& w, int word_bytes, const void* const base[3], const int64_t* const bs[3],
                  const YuvDesc* d, int depth, int msb, int B, int H, int W, int tau) {
  static const char* const pn[3] = {"y", "cb", "cr"};
  for (int p = 0; p < 3; ++p) {
    MLIC_CHECK(base[p] != nullptr, w + ": null base plane (" + pn[p] + ")");
    MLIC_CHECK(bs[p] != nullptr, w + ": null base strides (" + pn[p] + ")");
  }
  MLIC_CHECK(B >= 1, w + ": B must be positive");
  MLIC_CHECK(H >= 1 && W >= 1, w + ": H and W must be positive");
  MLIC_CHECK(H <= (1 << 24) && W <= (1 << 24), w + ": frame side above 2^24");
  if (word_bytes == 1) {
    MLIC_CHECK(depth == 8, w + ": depth must be 8");
    MLIC_CHECK(msb == 0, w + ": msb must be 0");
  } else {
    MLIC_CHECK(depth >= RES16_MIN_DEPTH && depth <= RES16_MAX_DEPTH, w + ": depth must be in 9..16");
    MLIC_CHECK(msb == 0 || msb == 1, w + ": msb must be 0 or 1");
  }
  desc_check(w, d, depth);
  MLIC_CHECK(residual_yuv_geom(H, W, d->sub_x, d->sub_y).N <= RES_SEG_MAX_N, w + ": the frame has more than 2^29 samples");
  MLIC_CHECK(tau >= 0 && tau <= RES_MAX_TAU, w + ": tau must be in 0..127");
  for (int p = 0; p < 3; ++p) {
    MLIC_CHECK(bs[p][2] != 0, w + ": zero column stride (base " + pn[p] + ")");
    MLIC_CHECK(aligned(base[p], (uintptr_t)word_bytes), w + ": base planes must be 2-byte aligned");
  }
}

void planes_check(const std::string& w, int word_bytes, const char* name, const void* const pl[3],
                  const int64_t* const s[3]) {
  for (int p = 0; p < 3; ++p) {
    MLIC_CHECK(pl[p] != nullptr && s[p] != nullptr, w + ": " + name + " needs three planes with strides");
    MLIC_CHECK(s[p][2] != 0, w + ": zero column stride (" + name + ")");
    MLIC_CHECK(aligned(pl[p], (uintptr_t)word_bytes), w + ": " + name + " planes must be 2-byte aligned");
  }
}

void shift_check(const std::string& w, int depth, int shift, const void* lo_plane) {
  if (depth == 8) MLIC_CHECK(shift == 0, w + ": shift must be 0 at depth 8");
  else MLIC_CHECK(shift >= 0 && shift <= residual_yuv_max_shift(depth), w + ": shift must be in 0..depth - 7");
  if (depth == 8) MLIC_CHECK(lo_plane == nullptr, w + ": lo_plane must be null at depth 8");
  else MLIC_CHECK((lo_plane != nullptr) == (shift > 0), w + ": lo_plane goes with a shift above 0");
}

template <typename WORD, typename V>
PlaneSet<WORD> plane_set(V* const pl[3], const int64_t* const s[3]) {
  PlaneSet<WORD> q;
  for (int p = 0; p < 3; ++p) {
    q.p[p] = pl ? static_cast<WORD*>(pl[p]) : nullptr;
    q.img[p] = pl ? s[p][0] : 0, q.row[p] = pl ? s[p][1] : 0, q.col[p] = pl ? s[p][2] : 0;
    q.path[p] = pl ? p_path(s[p][2]) : P_GENERAL;
  }
  return q;
}

template <typename WORD>
void front_launch(int mode, const void* const base[3], const int64_t* const bs[3], const void* const x[3],
                  const int64_t* const xs[3], int depth, int msb, int tau, int shift, const PGeom& g, unsigned blocks,
                  const FrontOut& o, hipStream_t st) {
  const PlaneSet<const WORD> b = plane_set<const WORD>(base, bs), xp = plane_set<const WORD>(x, xs);
  const int shr = msb ? 16 - depth : 0;
  const uint32_t magic = residual16_magic(2 * tau + 1);
  if (mode == F_FULL)
    hipLaunchKernelGGL((residual_front_planes_kernel<WORD, F_FULL>), dim3(blocks), dim3(256), 0, st, b, xp, depth, shr,
                       tau, magic, shift, g, o);
  else if (mode == F_STATS)
    hipLaunchKernelGGL((residual_front_planes_kernel<WORD, F_STATS>), dim3(blocks), dim3(256), 0, st, b, xp, depth, shr,
                       tau, magic, 0, g, o);
  else
    hipLaunchKernelGGL((residual_front_planes_kernel<WORD, F_CTX>), dim3(blocks), dim3(256), 0, st, b, xp, depth, shr,
                       tau, magic, 0, g, o);
  HIP_OK(hipGetLastError());
}

}  // namespace

void image_residual_front_planes(const char* who, int word_bytes, const void* const base[3],
                                 const int64_t* const base_strides[3], const void* const x[3],
                                 const int64_t* const x_strides[3], const YuvDesc* desc, int depth, int msb, int B, int H,
                                 int W, int tau, int shift, uint8_t* ctx, uint32_t* ctx_count, uint64_t* digest,
                                 int16_t* sym, uint64_t* lo_plane, uint32_t* hist, uint32_t* max_err,
                                 uint32_t* max_abs_q, uint64_t* sum_abs_q, hipStream_t st) {
  const std::string w(who);
  common_check(w, word_bytes, base, base_strides, desc, depth, msb, B, H, W, tau);
  check_front_out(w, ctx, ctx_count, digest);
  const bool has_x = x[0] != nullptr || x[1] != nullptr || x[2] != nullptr;
  if (has_x) {
    planes_check(w, word_bytes, "x", x, x_strides);
    shift_check(w, depth, shift, lo_plane);
    check_front_x_needed(w, sym, hist, max_err, max_abs_q, sum_abs_q);
    check_front_x_aligned(w, sym, lo_plane, hist, max_err, max_abs_q, sum_abs_q);
  } else {
    check_front_without_x(w, sym, lo_plane, hist, max_err, max_abs_q, sum_abs_q);
  }
  unsigned blocks;
  const PGeom g = p_geom(w, B, H, W, desc, PF_ROWS * PF_GROUPS, &blocks);
  const FrontOut o{ctx, ctx_count, reinterpret_cast<unsigned long long*>(digest), sym,
                   reinterpret_cast<unsigned long long*>(lo_plane), hist, max_err, max_abs_q,
                   reinterpret_cast<unsigned long long*>(sum_abs_q)};
  // the sums start from zero: zeroed here, on the stream
  HIP_OK(hipMemsetAsync(ctx_count, 0, sizeof(uint32_t) * RES_CTX * (size_t)B, st));
  HIP_OK(hipMemsetAsync(digest, 0, sizeof(uint64_t) * (size_t)B, st));
  if (has_x) {
    HIP_OK(hipMemsetAsync(hist, 0, sizeof(uint32_t) * RES_CTX * RES_BINS * (size_t)B, st));
    HIP_OK(hipMemsetAsync(max_err, 0, sizeof(uint32_t) * (size_t)B, st));
    HIP_OK(hipMemsetAsync(max_abs_q, 0, sizeof(uint32_t) * (size_t)B, st));
    HIP_OK(hipMemsetAsync(sum_abs_q, 0, sizeof(uint64_t) * (size_t)B, st));
  }
  const int mode = has_x ? F_FULL : F_CTX;
  if (word_bytes == 1)
    front_launch<uint8_t>(mode, base, base_strides, has_x ? x : nullptr, x_strides, depth, msb, tau, shift, g, blocks, o, st);
  else
    front_launch<uint16_t>(mode, base, base_strides, has_x ? x : nullptr, x_strides, depth, msb, tau, shift, g, blocks, o, st);
}

void image_residual_stats_planes(const char* who, int word_bytes, const void* const base[3],
                                 const int64_t* const base_strides[3], const void* const x[3],
                                 const int64_t* const x_strides[3], const YuvDesc* desc, int depth, int msb, int B, int H,
                                 int W, int tau, uint32_t* max_abs_q, uint64_t* sum_abs_q, hipStream_t st) {
  const std::string w(who);
  common_check(w, word_bytes, base, base_strides, desc, depth, msb, B, H, W, tau);
  planes_check(w, word_bytes, "x", x, x_strides);
  MLIC_CHECK(max_abs_q != nullptr && sum_abs_q != nullptr, w + ": null max_abs_q or sum_abs_q");
  MLIC_CHECK(aligned(max_abs_q, 4) && aligned(sum_abs_q, 8), w + ": max_abs_q must be 4-byte and sum_abs_q 8-byte aligned");
  unsigned blocks;
  const PGeom g = p_geom(w, B, H, W, desc, PF_ROWS * PF_GROUPS, &blocks);
  const FrontOut o{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, max_abs_q,
                   reinterpret_cast<unsigned long long*>(sum_abs_q)};
  HIP_OK(hipMemsetAsync(max_abs_q, 0, sizeof(uint32_t) * (size_t)B, st));
  HIP_OK(hipMemsetAsync(sum_abs_q, 0, sizeof(uint64_t) * (size_t)B, st));
  if (word_bytes == 1)
    front_launch<uint8_t>(F_STATS, base, base_strides, x, x_strides, depth, msb, tau, 0, g, blocks, o, st);
  else
    front_launch<uint16_t>(F_STATS, base, base_strides, x, x_strides, depth, msb, tau, 0, g, blocks, o, st);
}

namespace {
template <typename WORD>
void apply_launch(const void* const base[3], const int64_t* const bs[3], const int16_t* sym, const uint64_t* lo_plane,
                  int depth, int msb, int tau, int shift, const PGeom& g, unsigned blocks, void* const out[3],
                  const int64_t* const os[3], const void* const ref[3], const int64_t* const rs[3], uint64_t* sq_err,
                  uint32_t* max_err, uint32_t* status, hipStream_t st) {
  const PlaneSet<const WORD> b = plane_set<const WORD>(base, bs), r = plane_set<const WORD>(ref, rs);
  const PlaneSet<WORD> o = plane_set<WORD>(out, os);
  const int shr = msb ? 16 - depth : 0;
  auto* sq64 = reinterpret_cast<unsigned long long*>(sq_err);
  auto* lo64 = reinterpret_cast<const unsigned long long*>(lo_plane);
  if (ref)
    hipLaunchKernelGGL((residual_apply_planes_kernel<WORD, true>), dim3(blocks), dim3(256), 0, st, b, sym, lo64, depth,
                       shr, tau, shift, g, o, r, sq64, max_err, status);
  else
    hipLaunchKernelGGL((residual_apply_planes_kernel<WORD, false>), dim3(blocks), dim3(256), 0, st, b, sym, lo64, depth,
                       shr, tau, shift, g, o, r, sq64, max_err, status);
  HIP_OK(hipGetLastError());
}
}  // namespace

void image_residual_apply_planes(const char* who, int word_bytes, const void* const base[3],
                                 const int64_t* const base_strides[3], const int16_t* sym, const uint64_t* lo_plane,
                                 const YuvDesc* desc, int depth, int msb, int B, int H, int W, int tau, int shift,
                                 void* const out[3], const int64_t* const out_strides[3], const void* const ref[3],
                                 const int64_t* const ref_strides[3], uint64_t* sq_err, uint32_t* max_err,
                                 uint32_t* status, hipStream_t st) {
  const std::string w(who);
  common_check(w, word_bytes, base, base_strides, desc, depth, msb, B, H, W, tau);
  MLIC_CHECK(sym != nullptr, w + ": null sym");
  MLIC_CHECK(status != nullptr, w + ": null status");
  shift_check(w, depth, shift, lo_plane);
  planes_check(w, word_bytes, "out", out, out_strides);
  MLIC_CHECK(aligned(sym, 2) && aligned(lo_plane, 8) && aligned(status, 4),
             w + ": sym must be 2-byte, lo_plane 8-byte and status 4-byte aligned");
  const bool has_ref = ref[0] != nullptr || ref[1] != nullptr || ref[2] != nullptr;
  if (has_ref) planes_check(w, word_bytes, "ref", ref, ref_strides);
  check_apply_scores(w, has_ref, sq_err, max_err);
  check_apply_scores_aligned(w, sq_err, max_err);
  unsigned blocks;
  const PGeom g = p_geom(w, B, H, W, desc, (has_ref ? PA_REF_GROUPS : 1) * PA_ROWS, &blocks);
  HIP_OK(hipMemsetAsync(status, 0, sizeof(uint32_t) * (size_t)B, st));
  if (has_ref) {
    HIP_OK(hipMemsetAsync(sq_err, 0, sizeof(uint64_t) * 3 * (size_t)B, st));
    HIP_OK(hipMemsetAsync(max_err, 0, sizeof(uint32_t) * (size_t)B, st));
  }
  if (word_bytes == 1)
    apply_launch<uint8_t>(base, base_strides, sym, lo_plane, depth, msb, tau, shift, g, blocks, out, out_strides,
                          has_ref ? ref : nullptr, ref_strides, sq_err, max_err, status, st);
  else
    apply_launch<uint16_t>(base, base_strides, sym, lo_plane, depth, msb, tau, shift, g, blocks, out, out_strides,
                           has_ref ? ref : nullptr, ref_strides, sq_err, max_err, status, st);
}

}  // namespace mlic
