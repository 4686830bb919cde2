// Residual coding's two passes over full-resolution bytes (residual.h has the definitions; DESIGN.md section 5
// "Residual coding").
//
// residual_front: base (and, for the encoder, the original x) -> the context plane, the per-context counts and the
// digest of base; with x also the quantised residual, the per-context histograms and the largest |x - rec|.
// residual_apply: base + symbols -> rec, optionally scored against a reference.
//
// Byte images come through element strides {image, row, column, channel}.  Row segments go through LDS as in
// image_io.hip (image_stage.h: whole aligned dwords as dwords, nothing outside the segment touched): HWC keeps its
// interleaved bytes, CHW three plane segments, and any other stride set is gathered into the CHW form with one byte
// load per sample.  All forms give the same bits.
//
// front: a block is 256 threads, one pixel column each, and walks RF_GROUPS groups of RF_ROWS rows.  Per group the
// RF_ROWS + 2 base rows (rows clamped into the image) and the RF_ROWS rows of x are staged once; a thread then runs
// down its column and keeps the row-wise min / max of the last three rows in registers, so a sample costs three LDS
// byte reads per staged row, not nine loads.  Histograms live in LDS (a thread adds a run of equal (context, bin)
// keys with one atomic), counts are packed per thread and reduced per wave, and a block flushes its nonzero bins,
// its counts, its digest sum and its maximum once, with global integer atomics -- every sum is of integers, so the
// order of the atomics changes nothing.
#include "image_stage.h"
#include "kernels.h"
#include "residual.h"
#include "residual_dev.h"

namespace mlic {

namespace {

constexpr int R_SEG = (R_TW + 2 + 3 + 3) / 4;  // dwords of a (R_TW + 2)-byte plane segment at any alignment
constexpr int R_ROW = 3 * R_SEG;               // one staged row: three plane segments, or 3 (R_TW + 2) + 3 HWC bytes
constexpr int RF_ROWS = 8, RF_GROUPS = 8;      // front: rows per group, groups per block
constexpr int RA_ROWS = 4, RA_REF_GROUPS = 16; // apply: a row per wave; with ref a block walks 16 groups (one atomic)
enum { R_GENERAL = 0, R_HWC = 1, R_CHW = 2 };
static_assert(RF_ROWS * RF_GROUPS <= 255, "a thread's packed class counts are 8 bits each");
static_assert(3 * (R_TW + 2) + 3 <= 4 * R_ROW, "an HWC row fits the staged row");

int r_path(const int64_t* s) { return (s[2] == 3 && s[3] == 1) ? R_HWC : s[2] == 1 ? R_CHW : R_GENERAL; }

// n pixels from p (channel 0 of the segment's first pixel) into the staged row r: one wave
__device__ inline void seg_in(int path, const uint8_t* __restrict__ p, int64_t col, int64_t ch, int n, uint32_t* r,
                              int lane) {
  if (path == R_HWC) {
    stage_in(p, 3 * n, r, lane);
  } else if (path == R_CHW) {
    for (int c = 0; c < 3; ++c) stage_in(p + c * ch, n, r + c * R_SEG, lane);
  } else {
    uint8_t* r8 = reinterpret_cast<uint8_t*>(r);
    for (int c = 0; c < 3; ++c)
      for (int k = lane; k < n; k += 64) r8[c * R_SEG * 4 + k] = p[(int64_t)k * col + c * ch];
  }
}

// where channel c of pixel k sits in the staged row: byte index = seg_at(...) + (HWC ? 3 k : k)
__device__ inline int seg_at(int path, const uint8_t* p, int64_t ch, int c) {
  if (path == R_HWC) return addr_mod4(p) + c;
  if (path == R_CHW) return c * R_SEG * 4 + addr_mod4(p + c * ch);
  return c * R_SEG * 4;
}

__device__ inline void seg_out(int path, uint8_t* __restrict__ p, int64_t ch, int n, const uint32_t* r, int lane) {
  if (path == R_HWC) {
    stage_out(p, 3 * n, r, lane);
  } else {  // R_CHW: the general form writes straight to memory
    for (int c = 0; c < 3; ++c) stage_out(p + c * ch, n, r + c * R_SEG, lane);
  }
}

template <bool HAS_X>
__global__ __launch_bounds__(256) void residual_front_kernel(
    const uint8_t* __restrict__ base, RStride bs, int bpath, const uint8_t* __restrict__ xin, RStride xs, int xpath,
    int tau, uint32_t magic, int H, int W, uint8_t* __restrict__ ctx, unsigned int* __restrict__ ctx_count,
    unsigned long long* __restrict__ digest, int16_t* __restrict__ sym, unsigned int* __restrict__ hist,
    unsigned int* __restrict__ max_err, int tiles_x, int tiles_y) {
  __shared__ uint32_t SB[RF_ROWS + 2][R_ROW];
  __shared__ uint32_t SX[HAS_X ? RF_ROWS : 1][R_ROW];
  __shared__ unsigned int Hh[HAS_X ? RES_CTX * RES_BINS : 1];
  __shared__ unsigned int Cc[RES_CTX];
  __shared__ unsigned long long redD[4];
  __shared__ unsigned int redM[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (HAS_X)
    for (int k = tid; k < RES_CTX * RES_BINS; k += 256) Hh[k] = 0;
  if (tid < RES_CTX) Cc[tid] = 0;
  const int64_t t = blockIdx.x;
  const int64_t ry = t / tiles_x;
  const int x0 = (int)(t - ry * tiles_x) * R_TW;  // < W: the tiles cover the image only
  const int64_t img = ry / tiles_y;
  const int yb = (int)(ry - img * tiles_y) * (RF_ROWS * RF_GROUPS);
  const int nx = min(R_TW, W - x0);
  const int xa = max(x0 - 1, 0), ns = min(x0 + nx + 1, W) - xa;  // the staged base columns [xa, xa + ns)
  const bool active = tid < nx;
  const int x = x0 + tid;
  // this thread's three columns in the staged segment (clamped into the image, hence into the segment)
  const int kl = max(x - 1, 0) - xa, km = min(x, W - 1) - xa, kr = min(x + 1, W - 1) - xa;
  const int step = 2 * tau + 1;
  const int bmul = bpath == R_HWC ? 3 : 1, xmul = xpath == R_HWC ? 3 : 1;
  const uint8_t* SB8 = reinterpret_cast<const uint8_t*>(&SB[0][0]);
  const uint8_t* SX8 = reinterpret_cast<const uint8_t*>(&SX[0][0]);
  const uint8_t* bimg = base + img * bs.img + (int64_t)xa * bs.col;
  const uint8_t* ximg = HAS_X ? xin + img * xs.img + (int64_t)x0 * xs.col : nullptr;
  const int64_t plane = (int64_t)H * W;

  unsigned long long cnt[3] = {0, 0, 0};  // 8 classes x 8 bits per channel
  unsigned long long dsum = 0;
  unsigned int merr = 0;
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
    if (active) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        int mn0 = 0, mx0 = 0, mn1 = 0, mx1 = 0, mid1 = 0;
        // staged row r of channel c: the sliding window's new row, and from r = 2 on the output of row r - 2
        auto step_row = [&](int r) {
          const int yc = min(max(y0 - 1 + r, 0), H - 1);
          const uint8_t* row = SB8 + r * (R_ROW * 4) + seg_at(bpath, bimg + (int64_t)yc * bs.row, bs.ch, c);
          const int vl = row[bmul * kl], vm = row[bmul * km], vr = row[bmul * kr];
          const int mn2 = min(vl, min(vm, vr)), mx2 = max(vl, max(vm, vr));
          if (r >= 2) {
            const int y = y0 + r - 2;
            const int a = max(mx0, max(mx1, mx2)) - min(mn0, min(mn1, mn2));
            const int cls = a < 2 ? 0 : 31 - __clz(a);
            const int cx = 8 * c + cls;
            const int64_t i = c * plane + (int64_t)y * W + x;
            ctx[img * 3 * plane + i] = (uint8_t)cx;
            cnt[c] += 1ull << (8 * cls);
            dsum += residual_digest_term(mid1, (uint64_t)i);
            if (HAS_X) {
              const uint8_t* xrow =
                  SX8 + (r - 2) * (R_ROW * 4) + seg_at(xpath, ximg + (int64_t)y * xs.row, xs.ch, c);
              const int xv = xrow[xmul * tid];
              const int d = xv - mid1, ad = d < 0 ? -d : d;
              const int qa = residual_div(ad + tau, magic);
              const int q = d < 0 ? -qa : qa;
              const int rec = min(max(mid1 + q * step, 0), 255);
              merr = max(merr, (unsigned int)abs(xv - rec));
              sym[img * 3 * plane + i] = (int16_t)q;
              const int k = cx * RES_BINS + residual_bin(q);
              if (k == key[c]) {
                ++run[c];
              } else {
                if (run[c]) atomicAdd(&Hh[key[c]], run[c]);
                key[c] = k;
                run[c] = 1;
              }
            }
          }
          mn0 = mn1, mx0 = mx1, mn1 = mn2, mx1 = mx2, mid1 = vm;
        };
        // rolled: a trial that unrolled this over a whole group (ten rows in flight) measured no faster without x
        // and slower with it, 0.95 against 0.83 ms at 32 x 1080 x 1920: its registers cost the fifth wave per SIMD
        for (int r = 0; r < rows + 2; ++r) step_row(r);
      }
    }
  }
  if (HAS_X) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (run[c]) atomicAdd(&Hh[key[c]], run[c]);
  }
  // counts: 8-bit fields -> two words of 16-bit fields (a wave's sum is at most 64 * 64 per field)
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const unsigned long long even = wave_sum64(cnt[c] & 0x00ff00ff00ff00ffull);
    const unsigned long long odd = wave_sum64((cnt[c] >> 8) & 0x00ff00ff00ff00ffull);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const unsigned int e = (unsigned int)(even >> (16 * k)) & 0xffffu, o = (unsigned int)(odd >> (16 * k)) & 0xffffu;
        if (e) atomicAdd(&Cc[8 * c + 2 * k], e);
        if (o) atomicAdd(&Cc[8 * c + 2 * k + 1], o);
      }
    }
  }
  dsum = wave_sum64(dsum);
  merr = wave_max32(merr);
  if (lane == 0) {
    redD[wave] = dsum;
    redM[wave] = merr;
  }
  __syncthreads();
  if (tid == 0) {
    atomicAdd(digest + img, sum4(redD) * RES_DIGEST_K);
    if (HAS_X) {
      const unsigned int m = max4(redM);
      if (m) atomicMax(max_err + img, m);
    }
  }
  if (tid < RES_CTX && Cc[tid]) atomicAdd(ctx_count + img * RES_CTX + tid, Cc[tid]);
  if (HAS_X)
    for (int k = tid; k < RES_CTX * RES_BINS; k += 256) {
      const unsigned int v = Hh[k];
      if (v) atomicAdd(hist + img * (RES_CTX * RES_BINS) + k, v);
    }
}

template <bool REF>
__global__ __launch_bounds__(256) void residual_apply_kernel(const uint8_t* __restrict__ base, RStride bs, int bpath,
                                                             const int16_t* __restrict__ sym, int tau, int H, int W,
                                                             uint8_t* __restrict__ out, RStride os, int opath,
                                                             const uint8_t* __restrict__ ref, RStride rs, int rpath,
                                                             unsigned long long* __restrict__ sq_err,
                                                             unsigned int* __restrict__ max_err, int tiles_x,
                                                             int tiles_y) {
  __shared__ uint32_t SB[RA_ROWS][R_ROW];
  __shared__ uint32_t SO[RA_ROWS][R_ROW];
  __shared__ uint32_t SR[REF ? RA_ROWS : 1][R_ROW];
  __shared__ unsigned long long redS[RA_ROWS];
  __shared__ unsigned int redM[RA_ROWS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int G = REF ? RA_REF_GROUPS : 1;
  const int64_t t = blockIdx.x;
  const int64_t ry = t / tiles_x;
  const int x0 = (int)(t - ry * tiles_x) * R_TW;
  const int64_t img = ry / tiles_y;
  const int yb = (int)(ry - img * tiles_y) * (G * RA_ROWS) + wave;
  const int step = 2 * tau + 1;
  const int bmul = bpath == R_HWC ? 3 : 1, omul = opath == R_HWC ? 3 : 1, rmul = rpath == R_HWC ? 3 : 1;
  const uint8_t* SB8 = reinterpret_cast<const uint8_t*>(SB[wave]);
  const uint8_t* SR8 = reinterpret_cast<const uint8_t*>(SR[REF ? wave : 0]);
  uint8_t* SO8 = reinterpret_cast<uint8_t*>(SO[wave]);
  const int64_t plane = (int64_t)H * W;
  unsigned int acc = 0, merr = 0;  // acc <= G * 4 * 3 * 255^2 per lane
  for (int g = 0; g < G; ++g) {
    const int y = yb + g * RA_ROWS;
    const int nx = y < H ? min(R_TW, W - x0) : 0;
    const uint8_t* brow = base + img * bs.img + (int64_t)y * bs.row + (int64_t)x0 * bs.col;  // used when nx > 0
    uint8_t* orow = out + img * os.img + (int64_t)y * os.row + (int64_t)x0 * os.col;
    const uint8_t* rrow = REF ? ref + img * rs.img + (int64_t)y * rs.row + (int64_t)x0 * rs.col : nullptr;
    // the symbols do not depend on the staging: loaded first, so their latency overlaps it
    int16_t qv[3][R_TW / 64];
    if (nx > 0) {
      const int16_t* srow = sym + img * 3 * plane + (int64_t)y * W + x0;
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < R_TW / 64; ++j) qv[c][j] = lane + 64 * j < nx ? srow[c * plane + lane + 64 * j] : (int16_t)0;
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
          const int px = lane + 64 * j;
          if (px >= nx) break;
          const int b = SB8[bat + bmul * px];
          const int q = qv[c][j];
          const int rec = min(max(b + q * step, 0), 255);
          if (opath == R_GENERAL) orow[(int64_t)px * os.col + c * os.ch] = (uint8_t)rec;
          else SO8[oat + omul * px] = (uint8_t)rec;
          if (REF) {
            const int d = rec - (int)SR8[rat + rmul * px];
            acc += (unsigned int)(d * d);
            merr = max(merr, (unsigned int)abs(d));
          }
        }
      }
    }
    __syncthreads();
    if (opath != R_GENERAL && nx > 0) seg_out(opath, orow, os.ch, nx, SO[wave], lane);
    if (G > 1) __syncthreads();  // the next group's bytes go into the same LDS
  }
  if (REF) {
    const unsigned long long s = wave_sum64((unsigned long long)acc);
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

}  // namespace

void image_residual_front_u8(const uint8_t* base, const int64_t* b, const uint8_t* x, const int64_t* xs, int B, int H,
                             int W, int tau, uint8_t* ctx, uint32_t* ctx_count, uint64_t* digest, int16_t* sym,
                             uint32_t* hist, uint32_t* max_err, hipStream_t st) {
  MLIC_CHECK(base != nullptr, "image_residual_front_u8: null base");
  MLIC_CHECK(b != nullptr, "image_residual_front_u8: null base strides");
  MLIC_CHECK(B >= 1, "image_residual_front_u8: B must be positive");
  MLIC_CHECK(H >= 1 && W >= 1, "image_residual_front_u8: H and W must be positive");
  MLIC_CHECK(tau >= 0 && tau <= RES_MAX_TAU, "image_residual_front_u8: tau must be in 0..127");
  MLIC_CHECK(b[2] != 0 && b[3] != 0, "image_residual_front_u8: zero column or channel stride (base)");
  check_front_out("image_residual_front_u8", ctx, ctx_count, digest);
  if (x != nullptr) {
    MLIC_CHECK(xs != nullptr, "image_residual_front_u8: x needs strides");
    MLIC_CHECK(xs[2] != 0 && xs[3] != 0, "image_residual_front_u8: zero column or channel stride (x)");
    MLIC_CHECK(sym != nullptr && hist != nullptr && max_err != nullptr,
               "image_residual_front_u8: with x, sym, hist and max_err are all needed");
    MLIC_CHECK(aligned(sym, 2) && aligned(hist, 4) && aligned(max_err, 4),
               "image_residual_front_u8: sym must be 2-byte, hist and max_err 4-byte aligned");
  } else {
    MLIC_CHECK(sym == nullptr && hist == nullptr && max_err == nullptr,
               "image_residual_front_u8: sym, hist and max_err go with x");
  }
  int tx, ty;
  const unsigned blocks = r_blocks(B, H, W, RF_ROWS * RF_GROUPS, &tx, &ty, "image_residual_front_u8");
  const RStride bs{b[0], b[1], b[2], b[3]};
  const RStride xr = x ? RStride{xs[0], xs[1], xs[2], xs[3]} : RStride{0, 0, 0, 0};
  auto* c64 = reinterpret_cast<unsigned long long*>(digest);
  // the sums start from zero: zeroed here, on the stream
  HIP_OK(hipMemsetAsync(ctx_count, 0, sizeof(uint32_t) * RES_CTX * (size_t)B, st));
  HIP_OK(hipMemsetAsync(digest, 0, sizeof(uint64_t) * (size_t)B, st));
  if (x) {
    HIP_OK(hipMemsetAsync(hist, 0, sizeof(uint32_t) * RES_CTX * RES_BINS * (size_t)B, st));
    HIP_OK(hipMemsetAsync(max_err, 0, sizeof(uint32_t) * (size_t)B, st));
    hipLaunchKernelGGL(residual_front_kernel<true>, dim3(blocks), dim3(256), 0, st, base, bs, r_path(b), x, xr,
                       r_path(xs), tau, residual_magic(2 * tau + 1), H, W, ctx, ctx_count, c64, sym, hist, max_err, tx,
                       ty);
  } else {
    hipLaunchKernelGGL(residual_front_kernel<false>, dim3(blocks), dim3(256), 0, st, base, bs, r_path(b), x, xr,
                       R_GENERAL, tau, residual_magic(2 * tau + 1), H, W, ctx, ctx_count, c64, sym, hist, max_err, tx,
                       ty);
  }
  HIP_OK(hipGetLastError());
}

void image_residual_apply_u8(const uint8_t* base, const int64_t* b, const int16_t* sym, int B, int H, int W, int tau,
                             uint8_t* out, const int64_t* o, const uint8_t* ref, const int64_t* r, uint64_t* sq_err,
                             uint32_t* max_err, hipStream_t st) {
  MLIC_CHECK(base != nullptr, "image_residual_apply_u8: null base");
  MLIC_CHECK(b != nullptr, "image_residual_apply_u8: null base strides");
  MLIC_CHECK(sym != nullptr, "image_residual_apply_u8: null sym");
  MLIC_CHECK(out != nullptr && o != nullptr, "image_residual_apply_u8: null out or out strides");
  MLIC_CHECK(B >= 1, "image_residual_apply_u8: B must be positive");
  MLIC_CHECK(H >= 1 && W >= 1, "image_residual_apply_u8: H and W must be positive");
  MLIC_CHECK(tau >= 0 && tau <= RES_MAX_TAU, "image_residual_apply_u8: tau must be in 0..127");
  MLIC_CHECK(b[2] != 0 && b[3] != 0, "image_residual_apply_u8: zero column or channel stride (base)");
  MLIC_CHECK(o[2] != 0 && o[3] != 0, "image_residual_apply_u8: zero column or channel stride (out)");
  MLIC_CHECK(aligned(sym, 2), "image_residual_apply_u8: sym must be 2-byte aligned");
  check_apply_scores("image_residual_apply_u8", ref != nullptr, sq_err, max_err);
  MLIC_CHECK(ref == nullptr || (r != nullptr && r[2] != 0 && r[3] != 0),
             "image_residual_apply_u8: ref needs strides with nonzero column and channel stride");
  check_apply_scores_aligned("image_residual_apply_u8", sq_err, max_err);
  int tx, ty;
  const unsigned blocks =
      r_blocks(B, H, W, (ref ? RA_REF_GROUPS : 1) * RA_ROWS, &tx, &ty, "image_residual_apply_u8");
  const RStride bs{b[0], b[1], b[2], b[3]}, os{o[0], o[1], o[2], o[3]};
  const RStride rr = ref ? RStride{r[0], r[1], r[2], r[3]} : RStride{0, 0, 0, 0};
  auto* sq64 = reinterpret_cast<unsigned long long*>(sq_err);
  if (ref) {
    HIP_OK(hipMemsetAsync(sq_err, 0, sizeof(uint64_t) * (size_t)B, st));
    HIP_OK(hipMemsetAsync(max_err, 0, sizeof(uint32_t) * (size_t)B, st));
    hipLaunchKernelGGL(residual_apply_kernel<true>, dim3(blocks), dim3(256), 0, st, base, bs, r_path(b), sym, tau, H,
                       W, out, os, r_path(o), ref, rr, r_path(r), sq64, max_err, tx, ty);
  } else {
    hipLaunchKernelGGL(residual_apply_kernel<false>, dim3(blocks), dim3(256), 0, st, base, bs, r_path(b), sym, tau, H,
                       W, out, os, r_path(o), ref, rr, R_GENERAL, sq64, max_err, tx, ty);
  }
  HIP_OK(hipGetLastError());
}

}  // namespace mlic
