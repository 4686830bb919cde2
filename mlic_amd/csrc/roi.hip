// Region-of-interest coding support (DESIGN.md §5 "ROI coding"): the level map of a mask, the gain plane of a
// level map, and the squared error of a decode split by the mask.  One launch each; integers only where a value
// is compared or stored, so every result is exact and does not depend on scheduling.
//
// roi_levels: a block owns one cell of the z grid (64 x 64 image pixels, clipped to H x W) of one image: its 256
// threads count the nonzero mask bytes of the cell (a thread walks a quarter row at a time, so a wave reads
// consecutive columns), the counts are summed in LDS, and one thread stores
//     level = lo + ceil((hi - lo) * count / area),     area = the cell's pixels inside the image (>= 1).
// gain_plane: nearest expansion of the level map to the latent grid (a cell is 4 x 4 latent pixels), the level
// looked up in a table that travels in the kernel arguments.
// sq_err_roi: as the egress kernel's sq_err, split by the mask: per block four 64-bit partial sums, one integer
// atomic each (order-independent: the sums are exact integers).
#include <algorithm>
#include <cmath>

#include "kernels.h"

namespace mlic {

namespace {

struct RoiStride3 {
  int64_t img, row, col;
};
struct RoiStride4 {
  int64_t img, row, col, ch;
};
struct RoiGains {
  float g[ROI_MAX_LEVELS];
};

__global__ __launch_bounds__(256) void roi_levels_kernel(const uint8_t* __restrict__ mask, RoiStride3 s, int H, int W,
                                                         int hz, int wz, int lo, int hi,
                                                         uint8_t* __restrict__ levels) {
  __shared__ unsigned int red[256];
  const int64_t cell = blockIdx.x;  // (image, cell row, cell column), column fastest
  const int cx = (int)(cell % wz), cy = (int)((cell / wz) % hz);
  const int64_t img = cell / ((int64_t)wz * hz);
  const int y0 = cy * 64, x0 = cx * 64;
  const int ny = min(64, H - y0), nx = min(64, W - x0);  // >= 1: hz, wz = ceil(H / 64), ceil(W / 64)
  const uint8_t* base = mask + img * s.img + (int64_t)y0 * s.row + (int64_t)x0 * s.col;
  unsigned int cnt = 0;
  // 4096 cell pixels over 256 threads: thread t takes pixel t + 256 k, i.e. column t % 64 of row t / 64 + 4 k
  const int x = threadIdx.x & 63;
  if (x < nx)
    for (int y = threadIdx.x >> 6; y < ny; y += 4) cnt += base[(int64_t)y * s.row + (int64_t)x * s.col] != 0 ? 1u : 0u;
  red[threadIdx.x] = cnt;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const unsigned int area = (unsigned int)(ny * nx);  // <= 4096; (hi - lo) * count <= 255 * 4096
    levels[cell] = (uint8_t)(lo + (int)(((unsigned int)(hi - lo) * red[0] + area - 1) / area));
  }
}

__global__ __launch_bounds__(256) void roi_gain_plane_kernel(const uint8_t* __restrict__ levels, int hz, int wz,
                                                             RoiGains t, int n_levels, float* __restrict__ g,
                                                             int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // over [B][4 hz][4 wz]
  if (i >= n) return;
  const int wy = 4 * wz, hy = 4 * hz;
  const int x = (int)(i % wy), y = (int)((i / wy) % hy);
  const int64_t b = i / ((int64_t)wy * hy);
  const int lv = levels[(b * hz + (y >> 2)) * wz + (x >> 2)];
  float v = t.g[0];  // a level the table does not hold (the caller's contract excludes it) reads the last entry
#pragma unroll
  for (int k = 1; k < ROI_MAX_LEVELS; ++k)
    if (k < n_levels && lv >= k) v = t.g[k];
  g[i] = v;
}

__global__ __launch_bounds__(256) void sq_err_roi_kernel(const uint8_t* __restrict__ a, RoiStride4 as,
                                                         const uint8_t* __restrict__ b, RoiStride4 bs,
                                                         const uint8_t* __restrict__ mask, RoiStride3 ms, int H, int W,
                                                         unsigned long long* __restrict__ out) {
  __shared__ unsigned long long red[4][256];
  const int64_t img = blockIdx.y;
  const int64_t n = (int64_t)H * W;
  unsigned long long acc[4] = {0, 0, 0, 0};  // sq_err inside, pixels inside, sq_err outside, pixels outside
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t y = i / W, x = i - y * W;
    const uint8_t* pa = a + img * as.img + y * as.row + x * as.col;
    const uint8_t* pb = b + img * bs.img + y * bs.row + x * bs.col;
    unsigned int sq = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int d = (int)pa[c * as.ch] - (int)pb[c * bs.ch];
      sq += (unsigned int)(d * d);
    }
    const int side = mask[img * ms.img + y * ms.row + x * ms.col] != 0 ? 0 : 2;
    acc[side] += sq;
    acc[side + 1] += 1;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) red[k][threadIdx.x] = acc[k];
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) {
#pragma unroll
      for (int j = 0; j < 4; ++j) red[j][threadIdx.x] += red[j][threadIdx.x + k];
    }
    __syncthreads();
  }
  if (threadIdx.x < 4 && red[threadIdx.x][0]) atomicAdd(out + img * 4 + threadIdx.x, red[threadIdx.x][0]);
}

}  // namespace

void roi_levels_u8(const uint8_t* mask, const int64_t* s, int B, int H, int W, int lo, int hi, uint8_t* levels,
                   hipStream_t st) {
  MLIC_CHECK(mask != nullptr && s != nullptr && levels != nullptr, "roi_levels: null argument");
  MLIC_CHECK(B >= 1 && H >= 1 && W >= 1, "roi_levels: B, H and W must be positive");
  MLIC_CHECK(H <= (1 << 24) && W <= (1 << 24), "roi_levels: image side above 2^24");
  MLIC_CHECK(lo <= hi, "roi_levels: lo is above hi");
  MLIC_CHECK(lo >= 0 && hi <= 255, "roi_levels: levels are bytes (0 <= lo, hi <= 255)");
  const int hz = (H + 63) / 64, wz = (W + 63) / 64;
  const int64_t blocks = (int64_t)B * hz * wz;
  MLIC_CHECK(blocks <= 0x7fffffffLL, "roi_levels: batch too large for one launch");
  hipLaunchKernelGGL(roi_levels_kernel, dim3((unsigned)blocks), dim3(256), 0, st, mask, RoiStride3{s[0], s[1], s[2]}, H,
                     W, hz, wz, lo, hi, levels);
  HIP_OK(hipGetLastError());
}

void roi_gain_plane(const uint8_t* levels, int B, int hz, int wz, const float* gains, int n_levels, float* g,
                    hipStream_t st) {
  MLIC_CHECK(levels != nullptr && gains != nullptr && g != nullptr, "roi_gain_plane: null argument");
  MLIC_CHECK(B >= 1 && hz >= 1 && wz >= 1, "roi_gain_plane: B, hz and wz must be positive");
  MLIC_CHECK(hz <= (1 << 18) && wz <= (1 << 18), "roi_gain_plane: grid side above 2^18");
  MLIC_CHECK(n_levels >= 1 && n_levels <= ROI_MAX_LEVELS, "roi_gain_plane: n_levels must be in [1, 16]");
  RoiGains t;
  for (int k = 0; k < ROI_MAX_LEVELS; ++k) {
    const float v = gains[k < n_levels ? k : n_levels - 1];
    MLIC_CHECK(std::isfinite(v) && v > 0.0f, "roi_gain_plane: a gain is not finite and positive");
    t.g[k] = v;
  }
  const int64_t n = (int64_t)B * 16 * hz * wz;
  MLIC_CHECK((n + 255) / 256 <= 0x7fffffffLL, "roi_gain_plane: batch too large for one launch");
  hipLaunchKernelGGL(roi_gain_plane_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, levels, hz, wz, t,
                     n_levels, g, n);
  HIP_OK(hipGetLastError());
}

void sq_err_roi_u8(const uint8_t* a, const int64_t* as, const uint8_t* b, const int64_t* bs, const uint8_t* mask,
                   const int64_t* ms, int B, int H, int W, uint64_t* out, hipStream_t st) {
  MLIC_CHECK(a != nullptr && as != nullptr && b != nullptr && bs != nullptr, "sq_err_roi: null image or strides");
  MLIC_CHECK(mask != nullptr && ms != nullptr, "sq_err_roi: null mask or strides");
  MLIC_CHECK(out != nullptr && reinterpret_cast<uintptr_t>(out) % 8 == 0, "sq_err_roi: out must be 8-byte aligned");
  MLIC_CHECK(B >= 1 && B <= 65535 && H >= 1 && W >= 1, "sq_err_roi: B in [1, 65535], H and W positive expected");
  MLIC_CHECK(H <= (1 << 24) && W <= (1 << 24), "sq_err_roi: image side above 2^24");
  HIP_OK(hipMemsetAsync(out, 0, sizeof(uint64_t) * 4 * (size_t)B, st));
  const int64_t n = (int64_t)H * W;
  const int nb = (int)std::min<int64_t>(1024, (n + 255) / 256);
  hipLaunchKernelGGL(sq_err_roi_kernel, dim3(nb, B), dim3(256), 0, st, a, RoiStride4{as[0], as[1], as[2], as[3]}, b,
                     RoiStride4{bs[0], bs[1], bs[2], bs[3]}, mask, RoiStride3{ms[0], ms[1], ms[2]}, H, W,
                     reinterpret_cast<unsigned long long*>(out));
  HIP_OK(hipGetLastError());
}

}  // namespace mlic
