// Rate and error maps (DESIGN.md §5 "Rate maps"): where the bits of the entropy model and the squared error of a
// decode lie in the image, and the heat-map picture of either.  All three are bandwidth-bound with a few
// operations per element; every result is a fixed sequence of rounded operations (or integers), so it does not
// depend on the batch, the position in it, the launch geometry or scheduling.
//
// rate_map, two launches.
//   terms: a thread owns one output element -- one pixel of one slice of y_map, or one pixel of z_map -- and adds
//   its channels' terms in ascending channel order from +0.0:  s = s + (-(double)log2f(lik)),
//   neglog2_partial_kernel's term.  Consecutive threads are consecutive pixels of a channel plane, so every load
//   of a wave is one contiguous piece of that plane; the channel loop is unrolled, the loads of a group go out
//   together and the additions keep their order.  The z pixels (few threads, N terms each) are the first blocks of
//   the grid, so they run beside the y blocks rather than after them.
//   finish: cell_bits, one thread per latent pixel:  v = z_map[i / 4][j / 4] / 16;  v = v + y_map[s][i][j] for
//   s = 0 .. S - 1.  slice_bits, one block per (image, plane): a wave owns a row; lane l adds the row's elements
//   l, l + 64, l + 128, ... in that order from +0.0, the 64 lane sums are folded in halves (lane l += lane
//   l + 32, then + 16, 8, 4, 2, 1), and one thread adds the row sums top to bottom from +0.0.  The 64 is part of
//   the definition (codec._slice_bits_cpu restates it), not of the launch.
// sq_err_blocks: a block owns one block row and 256 columns of it; a thread walks its column down the block's
//   rows, the columns of a block are folded by shuffles (a block is 8 .. 64 wide: inside a wave), one store per
//   block.  Integers only.
// heat: egress_u8_kernel's shape -- a wave owns one image row and 256 pixels of it, the two canonical byte layouts
//   go through LDS (image_stage.h), under-image included when it has the output's layout.  Per pixel, in doubles,
//   each operation rounded once:  q = clamp(floor((v - lo) / (hi - lo) * 255 + 0.5), 0, 255).
#include <cmath>

#include "image_stage.h"
#include "kernels.h"

namespace mlic {

namespace {

constexpr int MAP_TW = 256, MAP_ROWS = 4;   // heat tile: one row per wave, 4 pixels per lane
constexpr int MAP_SEG = MAP_TW / 4 + 1;     // dwords of a 256-byte segment at any alignment
constexpr int MAP_LDS = 3 * MAP_SEG;        // per wave: one 768-byte segment (HWC) or three of 256 (CHW)
enum { MAP_GENERAL = 0, MAP_HWC = 1, MAP_CHW = 2 };
enum { UNDER_NONE = 0, UNDER_BYTES = 1, UNDER_STAGED = 2 };

struct MapStride4 {
  int64_t img, row, col, ch;
};

__device__ inline double neglog2_terms(const float* __restrict__ p, int n, int64_t step) {
  double s = 0.0;  // +0.0: a term of lik == 1 is -0.0, and +0.0 + -0.0 = +0.0
#pragma unroll 8
  for (int c = 0; c < n; ++c) s += -(double)log2f(p[c * step]);
  return s;
}

__global__ __launch_bounds__(256) void rate_terms_kernel(const float* __restrict__ y_lik, int64_t y_bs,
                                                         const float* __restrict__ z_lik, int64_t z_bs, int cps, int S,
                                                         int hw, int N, int hwz, double* __restrict__ y_map,
                                                         double* __restrict__ z_map, unsigned z_blocks, int64_t ny,
                                                         int64_t nz) {
  if (blockIdx.x < z_blocks) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // over [B][hz * wz]
    if (i >= nz) return;
    const int64_t b = i / hwz;
    z_map[i] = neglog2_terms(z_lik + b * z_bs + (i - b * hwz), N, hwz);
  } else {
    const int64_t i = (int64_t)(blockIdx.x - z_blocks) * 256 + threadIdx.x;  // over [B][S][h * w]
    if (i >= ny) return;
    const int64_t bs = i / hw, b = bs / S;
    const int s = (int)(bs - b * S);
    y_map[i] = neglog2_terms(y_lik + b * y_bs + (int64_t)s * cps * hw + (i - bs * hw), cps, hw);
  }
}

__global__ __launch_bounds__(256) void rate_finish_kernel(const double* __restrict__ y_map,
                                                          const double* __restrict__ z_map, int S, int h, int w,
                                                          double* __restrict__ cell_bits, double* __restrict__ slice_bits,
                                                          unsigned sum_blocks, int64_t ncell) {
  __shared__ double rows[256];
  const int hz = h >> 2, wz = w >> 2;
  if (blockIdx.x < sum_blocks) {  // blockIdx.x = image * (S + 1) + plane; plane S is z_map
    const int64_t b = blockIdx.x / (unsigned)(S + 1);
    const int s = (int)(blockIdx.x - b * (S + 1));
    const int ph = s < S ? h : hz, pw = s < S ? w : wz;
    const double* pl = s < S ? y_map + (b * S + s) * (int64_t)h * w : z_map + b * (int64_t)hz * wz;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double total = 0.0;  // thread 0's
    for (int r0 = 0; r0 < ph; r0 += 256) {
      const int r1 = min(r0 + 256, ph);
      for (int r = r0 + wave; r < r1; r += 4) {  // the same rows for every lane of a wave
        double v = 0.0;
        for (int x = lane; x < pw; x += 64) v += pl[(int64_t)r * pw + x];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);  // lane 0: the fold in halves
        if (lane == 0) rows[r - r0] = v;
      }
      __syncthreads();
      if (threadIdx.x == 0)
        for (int k = 0; k < r1 - r0; ++k) total += rows[k];
      __syncthreads();
    }
    if (threadIdx.x == 0) slice_bits[blockIdx.x] = total;
  } else {
    const int64_t i = (int64_t)(blockIdx.x - sum_blocks) * 256 + threadIdx.x;  // over [B][h][w]
    if (i >= ncell) return;
    const int64_t hw = (int64_t)h * w;
    const int64_t b = i / hw, p = i - b * hw;
    const int y = (int)(p / w), x = (int)(p - (int64_t)y * w);
    double v = z_map[(b * hz + (y >> 2)) * wz + (x >> 2)] / 16.0;  // exact: a power of two
    for (int s = 0; s < S; ++s) v += y_map[(b * S + s) * hw + p];
    cell_bits[i] = v;
  }
}

__global__ __launch_bounds__(256) void sq_err_blocks_kernel(const uint8_t* __restrict__ a, MapStride4 as,
                                                            const uint8_t* __restrict__ b, MapStride4 bs, int H, int W,
                                                            int block, int nby, int nbx, int tiles_x,
                                                            uint32_t* __restrict__ out) {
  // blockIdx.x = (image, block row, column tile), column tile fastest
  const int64_t t = blockIdx.x;
  const int64_t r = t / tiles_x;
  const int x = (int)(t - r * tiles_x) * 256 + (int)threadIdx.x;
  const int64_t img = r / nby;
  const int by = (int)(r - img * nby);
  const int y0 = by * block, y1 = min(H, y0 + block);
  unsigned int acc = 0;  // a whole block: <= 64 * 64 * 3 * 255^2 < 2^30
  if (x < W) {
    const uint8_t* pa = a + img * as.img + (int64_t)x * as.col;
    const uint8_t* pb = b + img * bs.img + (int64_t)x * bs.col;
    for (int y = y0; y < y1; ++y) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int d = (int)pa[(int64_t)y * as.row + c * as.ch] - (int)pb[(int64_t)y * bs.row + c * bs.ch];
        acc += (unsigned int)(d * d);
      }
    }
  }
  // the columns of a block are `block` consecutive lanes that start at a multiple of `block`: inside one wave
  for (int off = block >> 1; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & (block - 1)) == 0 && x < W) out[(img * nby + by) * nbx + x / block] = acc;
}

struct HeatParams {
  double lo, hi;
  int shift, cmap, alpha, ph, pw;  // cell = 1 << shift
};

template <int PATH, int UNDER>
__global__ __launch_bounds__(256) void heat_u8_kernel(const double* __restrict__ plane, HeatParams q, int H, int W,
                                                      uint8_t* __restrict__ dst, MapStride4 ds,
                                                      const uint8_t* __restrict__ under, MapStride4 us, int tiles_x,
                                                      int tiles_y) {
  __shared__ uint32_t S[MAP_ROWS][MAP_LDS];
  __shared__ uint32_t U[UNDER == UNDER_STAGED ? MAP_ROWS : 1][MAP_LDS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // blockIdx.x = (image, row block, column tile), column tile fastest
  const int64_t t = blockIdx.x;
  const int64_t ry = t / tiles_x;
  const int x0 = (int)(t - ry * tiles_x) * MAP_TW;
  const int64_t img = ry / tiles_y;
  const int y = (int)(ry - img * tiles_y) * MAP_ROWS + wave;
  const int nx = y < H ? min(MAP_TW, W - x0) : 0;  // x0 < W: the tiles cover the image only
  uint8_t* row = dst + img * ds.img + (int64_t)y * ds.row + (int64_t)x0 * ds.col;
  const uint8_t* urow = UNDER != UNDER_NONE ? under + img * us.img + (int64_t)y * us.row + (int64_t)x0 * us.col : nullptr;
  uint8_t* S8 = reinterpret_cast<uint8_t*>(S[wave]);
  const uint8_t* U8 = reinterpret_cast<const uint8_t*>(U[UNDER == UNDER_STAGED ? wave : 0]);
  int sh[3] = {0, 0, 0}, ush[3] = {0, 0, 0};
  if (PATH == MAP_HWC) sh[0] = addr_mod4(row);
  if (PATH == MAP_CHW) {
#pragma unroll
    for (int c = 0; c < 3; ++c) sh[c] = addr_mod4(row + c * ds.ch);
  }
  if (UNDER == UNDER_STAGED) {  // the under-image has the output's layout
    if (PATH == MAP_HWC && nx > 0) {
      ush[0] = addr_mod4(urow);
      stage_in(urow, 3 * nx, U[wave], lane);
    }
    if (PATH == MAP_CHW && nx > 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        ush[c] = addr_mod4(urow + c * us.ch);
        stage_in(urow + c * us.ch, nx, U[wave] + c * MAP_SEG, lane);
      }
    }
    __syncthreads();
  }
  const double* prow = plane + (img * q.ph + (y >> q.shift)) * q.pw;  // read when nx > 0: y < H, inside the plane
  const double range = __dsub_rn(q.hi, q.lo);
#pragma unroll
  for (int j = 0; j < MAP_TW / 64; ++j) {
    const int px = lane + 64 * j;
    if (px >= nx) break;
    const double v = prow[(x0 + px) >> q.shift];
    const bool nan = v != v;
    int col[3] = {255, 0, 255};  // a NaN cell, unblended
    if (!nan) {
      double f = __dadd_rn(__dmul_rn(__ddiv_rn(__dsub_rn(v, q.lo), range), 255.0), 0.5);
      f = floor(f);
      const int k = f < 0.0 ? 0 : f > 255.0 ? 255 : (int)f;
      if (q.cmap == 0) {
        col[0] = col[1] = col[2] = k;
      } else {
        col[0] = min(255, 3 * k);
        col[1] = min(max(3 * k - 255, 0), 255);
        col[2] = min(max(3 * k - 510, 0), 255);
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      int o = col[c];
      if (UNDER != UNDER_NONE && !nan) {
        int u;
        if (UNDER == UNDER_STAGED && PATH == MAP_HWC) u = U8[ush[0] + 3 * px + c];
        else if (UNDER == UNDER_STAGED && PATH == MAP_CHW) u = U8[c * MAP_SEG * 4 + ush[c] + px];
        else u = urow[(int64_t)px * us.col + c * us.ch];
        o = (q.alpha * o + (256 - q.alpha) * u + 128) >> 8;
      }
      if (PATH == MAP_HWC) S8[sh[0] + 3 * px + c] = (uint8_t)o;
      else if (PATH == MAP_CHW) S8[c * MAP_SEG * 4 + sh[c] + px] = (uint8_t)o;
      else row[(int64_t)px * ds.col + c * ds.ch] = (uint8_t)o;
    }
  }
  if (PATH != MAP_GENERAL) {
    __syncthreads();
    if (PATH == MAP_HWC && nx > 0) stage_out(row, 3 * nx, S[wave], lane);
    if (PATH == MAP_CHW && nx > 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) stage_out(row + c * ds.ch, nx, S[wave] + c * MAP_SEG, lane);
    }
  }
}

int map_path(const int64_t* s) { return s[2] == 3 && s[3] == 1 ? MAP_HWC : s[2] == 1 ? MAP_CHW : MAP_GENERAL; }

// strides {image, row, column, channel} of a B x H x W x 3 byte image: the column and channel strides are not 0,
// and the offset of the last byte, (B - 1) |image| + (H - 1) |row| + (W - 1) |column| + 2 |channel|, fits int64
bool strides_ok(const int64_t* s, int B, int H, int W) {
  if (s[2] == 0 || s[3] == 0) return false;
  const int64_t n[4] = {B - 1, H - 1, W - 1, 2};
  int64_t sum = 0;
  for (int k = 0; k < 4; ++k) {
    if (s[k] == INT64_MIN) return false;
    int64_t term;
    if (__builtin_mul_overflow(s[k] < 0 ? -s[k] : s[k], n[k], &term) || __builtin_add_overflow(sum, term, &sum))
      return false;
  }
  return true;
}

template <int PATH>
void heat_launch(int under_mode, unsigned blocks, hipStream_t st, const double* plane, HeatParams q, int H, int W,
                 uint8_t* dst, MapStride4 ds, const uint8_t* under, MapStride4 us, int tx, int ty) {
  if (under_mode == UNDER_NONE)
    hipLaunchKernelGGL((heat_u8_kernel<PATH, UNDER_NONE>), dim3(blocks), dim3(256), 0, st, plane, q, H, W, dst, ds, under,
                       us, tx, ty);
  else if (under_mode == UNDER_BYTES)
    hipLaunchKernelGGL((heat_u8_kernel<PATH, UNDER_BYTES>), dim3(blocks), dim3(256), 0, st, plane, q, H, W, dst, ds, under,
                       us, tx, ty);
  else
    hipLaunchKernelGGL((heat_u8_kernel<PATH, UNDER_STAGED>), dim3(blocks), dim3(256), 0, st, plane, q, H, W, dst, ds,
                       under, us, tx, ty);
}

}  // namespace

void rate_map_check(const float* y_lik, int64_t y_bs, const float* z_lik, int64_t z_bs, int B, int M, int S, int h, int w,
                    int N, const double* y_map, const double* z_map, const double* cell_bits,
                    const double* slice_bits) {
  MLIC_CHECK(y_lik != nullptr && z_lik != nullptr, "rate_map: null likelihood tensor");
  MLIC_CHECK(y_map != nullptr || z_map != nullptr || cell_bits != nullptr || slice_bits != nullptr,
             "rate_map: at least one output expected");
  MLIC_CHECK(B >= 1 && M >= 1 && S >= 1 && N >= 1 && h >= 1 && w >= 1, "rate_map: B, M, S, N, h and w must be positive");
  MLIC_CHECK(M % S == 0, "rate_map: M must be a multiple of S (slices of equal width)");
  MLIC_CHECK(h % 4 == 0 && w % 4 == 0, "rate_map: h and w must be multiples of 4 (h = 4 hz, w = 4 wz)");
  MLIC_CHECK(B <= (1 << 20) && M <= (1 << 20) && N <= (1 << 20), "rate_map: B, M or N above 2^20");
  MLIC_CHECK((int64_t)h * w <= 0x7fffffffLL, "rate_map: latent grid above 2^31 pixels");
  MLIC_CHECK(y_bs >= (int64_t)M * h * w && z_bs >= (int64_t)N * (h / 4) * (w / 4),
             "rate_map: a batch stride is smaller than one image (dense NCHW per image expected)");
  MLIC_CHECK(y_bs <= INT64_MAX / B && z_bs <= INT64_MAX / B, "rate_map: batch stride overflows");
  MLIC_CHECK(reinterpret_cast<uintptr_t>(y_lik) % 4 == 0 && reinterpret_cast<uintptr_t>(z_lik) % 4 == 0,
             "rate_map: the likelihood tensors must be 4-byte aligned");
  MLIC_CHECK((reinterpret_cast<uintptr_t>(y_map) | reinterpret_cast<uintptr_t>(z_map) |
              reinterpret_cast<uintptr_t>(cell_bits) | reinterpret_cast<uintptr_t>(slice_bits)) % 8 == 0,
             "rate_map: the outputs must be 8-byte aligned");
  const int64_t ny = (int64_t)B * S * h * w, nz = (int64_t)B * (h / 4) * (w / 4);
  MLIC_CHECK((ny + 255) / 256 + (nz + 255) / 256 <= 0x7fffffffLL &&
                 (int64_t)B * (S + 1) + (ny / S + 255) / 256 <= 0x7fffffffLL,
             "rate_map: batch too large for one launch");
}

void rate_map(const float* y_lik, int64_t y_bs, const float* z_lik, int64_t z_bs, int B, int M, int S, int h, int w,
              int N, double* y_map, double* z_map, double* cell_bits, double* slice_bits, hipStream_t st) {
  rate_map_check(y_lik, y_bs, z_lik, z_bs, B, M, S, h, w, N, y_map, z_map, cell_bits, slice_bits);
  MLIC_CHECK(y_map != nullptr && z_map != nullptr, "rate_map: y_map and z_map (or scratch in their place) expected");
  const int hw = h * w, hwz = hw / 16;
  const int64_t ny = (int64_t)B * S * hw, nz = (int64_t)B * hwz;
  const unsigned zb = (unsigned)((nz + 255) / 256), yb = (unsigned)((ny + 255) / 256);
  hipLaunchKernelGGL(rate_terms_kernel, dim3(zb + yb), dim3(256), 0, st, y_lik, y_bs, z_lik, z_bs, M / S, S, hw, N, hwz,
                     y_map, z_map, zb, ny, nz);
  HIP_OK(hipGetLastError());
  if (cell_bits == nullptr && slice_bits == nullptr) return;
  const int64_t sb = slice_bits ? (int64_t)B * (S + 1) : 0;
  const int64_t ncell = cell_bits ? (int64_t)B * hw : 0;
  hipLaunchKernelGGL(rate_finish_kernel, dim3((unsigned)(sb + (ncell + 255) / 256)), dim3(256), 0, st, y_map, z_map, S, h,
                     w, cell_bits, slice_bits, (unsigned)sb, ncell);
  HIP_OK(hipGetLastError());
}

void sq_err_blocks_u8(const uint8_t* a, const int64_t* as, const uint8_t* b, const int64_t* bs, int B, int H, int W,
                      int block, uint32_t* out, hipStream_t st) {
  MLIC_CHECK(a != nullptr && as != nullptr && b != nullptr && bs != nullptr, "sq_err_blocks: null image or strides");
  MLIC_CHECK(out != nullptr && reinterpret_cast<uintptr_t>(out) % 4 == 0, "sq_err_blocks: out must be 4-byte aligned");
  MLIC_CHECK(B >= 1 && H >= 1 && W >= 1, "sq_err_blocks: B, H and W must be positive");
  MLIC_CHECK(H <= (1 << 24) && W <= (1 << 24), "sq_err_blocks: image side above 2^24");
  MLIC_CHECK(block == 8 || block == 16 || block == 32 || block == 64, "sq_err_blocks: block must be 8, 16, 32 or 64");
  MLIC_CHECK(strides_ok(as, B, H, W) && strides_ok(bs, B, H, W),
             "sq_err_blocks: zero column or channel stride, or strides that overflow");
  const int nby = (H + block - 1) / block, nbx = (W + block - 1) / block, tx = (W + 255) / 256;
  const int64_t blocks = (int64_t)B * nby * tx;
  MLIC_CHECK(blocks <= 0x7fffffffLL, "sq_err_blocks: batch too large for one launch");
  hipLaunchKernelGGL(sq_err_blocks_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a,
                     MapStride4{as[0], as[1], as[2], as[3]}, b, MapStride4{bs[0], bs[1], bs[2], bs[3]}, H, W, block, nby,
                     nbx, tx, out);
  HIP_OK(hipGetLastError());
}

void image_heat_u8(const double* plane, int B, int ph, int pw, int cell, double lo, double hi, int cmap, int H, int W,
                   uint8_t* dst, const int64_t* d, const uint8_t* under, const int64_t* u, int alpha, hipStream_t st) {
  MLIC_CHECK(plane != nullptr && dst != nullptr && d != nullptr, "heat_u8: null plane, image or strides");
  MLIC_CHECK(reinterpret_cast<uintptr_t>(plane) % 8 == 0, "heat_u8: the plane must be 8-byte aligned");
  MLIC_CHECK(B >= 1 && H >= 1 && W >= 1 && ph >= 1 && pw >= 1, "heat_u8: B, H, W, ph and pw must be positive");
  MLIC_CHECK(H <= (1 << 24) && W <= (1 << 24), "heat_u8: image side above 2^24");
  MLIC_CHECK(cell == 8 || cell == 16 || cell == 32 || cell == 64, "heat_u8: cell must be 8, 16, 32 or 64");
  MLIC_CHECK((int64_t)ph * cell >= H && (int64_t)pw * cell >= W, "heat_u8: the plane's cells do not cover H x W");
  MLIC_CHECK((int64_t)ph * pw <= 0x7fffffffLL, "heat_u8: plane above 2^31 cells");
  MLIC_CHECK(cmap == 0 || cmap == 1, "heat_u8: cmap must be 0 (gray) or 1 (hot)");
  MLIC_CHECK(std::isfinite(lo) && std::isfinite(hi) && hi > lo && std::isfinite(hi - lo),
             "heat_u8: finite lo < hi (and a finite hi - lo) expected");
  MLIC_CHECK(alpha >= 0 && alpha <= 256, "heat_u8: alpha must be in [0, 256]");
  MLIC_CHECK(under != nullptr || alpha == 256, "heat_u8: alpha below 256 needs an under-image");
  MLIC_CHECK(under == nullptr || u != nullptr, "heat_u8: the under-image needs strides");
  MLIC_CHECK(strides_ok(d, B, H, W), "heat_u8: zero column or channel stride, or strides that overflow (dst)");
  MLIC_CHECK(under == nullptr || strides_ok(u, B, H, W),
             "heat_u8: zero column or channel stride, or strides that overflow (under)");
  const int path = map_path(d);
  const int um = under == nullptr ? UNDER_NONE : (path != MAP_GENERAL && map_path(u) == path) ? UNDER_STAGED : UNDER_BYTES;
  const int tx = (W + MAP_TW - 1) / MAP_TW, ty = (H + MAP_ROWS - 1) / MAP_ROWS;
  const int64_t blocks = (int64_t)B * tx * ty;
  MLIC_CHECK(blocks <= 0x7fffffffLL, "heat_u8: batch too large for one launch");
  int shift = 3;
  while ((1 << shift) != cell) ++shift;
  const HeatParams q{lo, hi, shift, cmap, alpha, ph, pw};
  const MapStride4 ds{d[0], d[1], d[2], d[3]};
  const MapStride4 us = under ? MapStride4{u[0], u[1], u[2], u[3]} : MapStride4{0, 0, 0, 0};
  if (path == MAP_HWC) heat_launch<MAP_HWC>(um, (unsigned)blocks, st, plane, q, H, W, dst, ds, under, us, tx, ty);
  else if (path == MAP_CHW) heat_launch<MAP_CHW>(um, (unsigned)blocks, st, plane, q, H, W, dst, ds, under, us, tx, ty);
  else heat_launch<MAP_GENERAL>(um, (unsigned)blocks, st, plane, q, H, W, dst, ds, under, us, tx, ty);
  HIP_OK(hipGetLastError());
}

}  // namespace mlic
