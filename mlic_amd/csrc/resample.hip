// Scaled coding's two edge kernels (DESIGN.md section 5 "Scaled coding"): the uint8 ingest and egress of image_io.hip
// with a separable, antialiased polyphase resampler (resample_table.h) fused in, one launch each per batch.
//
// ingest: uint8 Hi x Wi x 3 images through element strides {image, row, column, channel}; v = byte / 255 (the true
// division of ingest_u8), resampled to h x w, clamped to [0, 1], written as fp32 [B][3][Hp][Wp] with +0 in the
// right / bottom padding; every destination element is written.
// egress: the h x w crop of fp32 planes (strides {image, channel, row}); v = fminf(fmaxf(x, 0), 1) (NaN -> 0),
// resampled to Ho x Wo, floor(clamp(., 0, 1) * 255), written through {image, row, column, channel} strides (only
// the image's own bytes); with a reference the exact per-image integer sum of squared byte differences.
//
// Arithmetic (the contract, bit for bit): per image and channel, horizontal first, nothing rounded to 8 bits in
// between: t[y][xo] = sum_j wx[xo][j] * v[y][sx[xo] + j], out[yo][xo] = sum_i wy[yo][i] * t[sy[yo] + i][xo], both
// fp32 with taps ascending, acc = +0; acc = acc + w * v with the product and the sum rounded once each (no FMA);
// taps j >= n are not part of the sum.  An identity axis (n = 1, weight 1) returns v itself.
//
// A block of four waves owns an R-row x 64-column output tile (R = 16, or 8 where the window of 16 rows would not
// fit 64 KiB of LDS) and walks the three channels.  Per channel the waves stream the input rows of the tile's
// window: a wave converts its row segment to fp32 into its own LDS row (the division happens once per input
// element, not once per tap), then every lane sums its column's horizontal taps -- the weights of the tile's 64
// columns sit in LDS, tap-major -- into the LDS intermediate [window rows][64].  After a barrier each lane sums its
// column's vertical taps in order (the row weights are wave-uniform).  The fp32 side moves 256-byte row pieces per
// wave instruction; the egress bytes of the canonical HWC / CHW layouts leave through LDS and stage_out
// (image_stage.h), any other stride set is written byte by byte; all forms give the same bits.
#include <map>
#include <memory>
#include <mutex>
#include <tuple>
#include <vector>

#include "image_stage.h"
#include "kernels.h"
#include "resample_table.h"

namespace mlic {

namespace {

constexpr int RS_TW = 64;                   // tile columns: one per lane
constexpr int RS_OB = 3 * (RS_TW / 4 + 1);  // dwords of a tile row's bytes: one 192-byte HWC segment or three CHW ones
constexpr size_t RS_LDS_MAX = 64 * 1024;
enum { RS_GENERAL = 0, RS_HWC = 1, RS_CHW = 2 };

struct RsStride3 {
  int64_t img, ch, row;
};
struct RsStride4 {
  int64_t img, row, col, ch;
};
// one axis' device table
struct RsAxis {
  const int32_t* start;
  const int32_t* count;
  const float* w;  // [Lo][taps]
  int taps, Li, Lo;
};
// what a launch needs beside the tables
struct RsGeom {
  int R, tiles_x, tiles_y;
  int t_rows;   // rows of the LDS intermediate: the widest row window of a tile
  int row_cap;  // floats of a wave's LDS row: the widest column window of a tile
};

struct RsTile {
  int64_t img;
  int y0, x0;
};
__device__ inline RsTile rs_tile(const RsGeom& g) {
  const int64_t t = blockIdx.x;
  const int64_t ry = t / g.tiles_x;
  RsTile o;
  o.x0 = (int)(t - ry * g.tiles_x) * RS_TW;
  o.img = ry / g.tiles_y;
  o.y0 = (int)(ry - o.img * g.tiles_y) * g.R;
  return o;
}

// the tile's window on the input and this lane's column
struct RsWin {
  int ya, nr, xa, nc;  // input rows [ya, ya + nr), columns [xa, xa + nc)
  int sxo, nxo;        // this lane's first tap within the window and its tap count (0 outside the image)
};
__device__ inline RsWin rs_window(const RsAxis& ax, const RsAxis& ay, const RsTile& t, int R, int lane) {
  const int ylast = min(t.y0 + R, ay.Lo) - 1, xlast = min(t.x0 + RS_TW, ax.Lo) - 1;
  RsWin q;
  q.ya = ay.start[t.y0];
  q.nr = ay.start[ylast] + ay.count[ylast] - q.ya;
  q.xa = ax.start[t.x0];
  q.nc = ax.start[xlast] + ax.count[xlast] - q.xa;
  const int xo = t.x0 + lane;
  const bool valid = xo < ax.Lo;
  q.sxo = valid ? ax.start[xo] - q.xa : 0;
  q.nxo = valid ? ax.count[xo] : 0;
  return q;
}

// the weights of the tile's 64 columns, tap-major: WX[j * 64 + lane]
__device__ inline void rs_stage_wx(const RsAxis& ax, int x0, float* WX, int lane, int wave) {
  const int xo = x0 + lane;
  for (int j = wave; j < ax.taps; j += 4) WX[j * RS_TW + lane] = xo < ax.Lo ? ax.w[(int64_t)xo * ax.taps + j] : 0.0f;
}

__device__ inline float rs_horizontal(const float* WX, const float* row, const RsWin& q, int taps, int lane) {
  float acc = 0.0f;
  for (int j = 0; j < taps; ++j)
    if (j < q.nxo) acc = __fadd_rn(acc, __fmul_rn(WX[j * RS_TW + lane], row[q.sxo + j]));
  return acc;
}

// output row yo of the tile's column `lane`: T holds the window's horizontally resampled rows
__device__ inline float rs_vertical(const RsAxis& ay, const float* T, int yo, int ya, int lane) {
  const int sy = ay.start[yo] - ya, ny = ay.count[yo];
  const float* wr = ay.w + (int64_t)yo * ay.taps;
  float acc = 0.0f;
  for (int i = 0; i < ny; ++i) acc = __fadd_rn(acc, __fmul_rn(wr[i], T[(sy + i) * RS_TW + lane]));
  return acc;
}

__global__ __launch_bounds__(256) void ingest_u8_scaled_kernel(const uint8_t* __restrict__ src, RsStride4 s, RsAxis ax,
                                                               RsAxis ay, float* __restrict__ dst, int Hp, int Wp,
                                                               RsGeom g) {
  extern __shared__ float rs_lds[];
  float* WX = rs_lds;
  float* T = WX + ax.taps * RS_TW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* ROW = T + g.t_rows * RS_TW + wave * g.row_cap;
  const RsTile t = rs_tile(g);
  const int h = ay.Lo, w = ax.Lo, rpw = g.R / 4;
  const int64_t plane = (int64_t)Hp * Wp;
  // the tiles cover Hp x Wp exactly (R divides 64): every element of the tile is the destination's
  float* out = dst + t.img * 3 * plane + (int64_t)(t.y0 + wave * rpw) * Wp + t.x0 + lane;
  if (t.y0 >= h || t.x0 >= w) {  // all padding
    for (int c = 0; c < 3; ++c)
      for (int k = 0; k < rpw; ++k) out[c * plane + (int64_t)k * Wp] = 0.0f;
    return;
  }
  const RsWin q = rs_window(ax, ay, t, g.R, lane);
  rs_stage_wx(ax, t.x0, WX, lane, wave);
  const uint8_t* win = src + t.img * s.img + (int64_t)q.ya * s.row + (int64_t)q.xa * s.col;
  for (int c = 0; c < 3; ++c) {
    for (int r0 = 0; r0 < q.nr; r0 += 4) {  // the same trip count for the whole block
      const int r = r0 + wave;
      if (r < q.nr) {
        const uint8_t* rp = win + (int64_t)r * s.row + c * s.ch;
        for (int k = lane; k < q.nc; k += 64) ROW[k] = (float)rp[(int64_t)k * s.col] / 255.0f;  // correctly rounded
      }
      __syncthreads();  // the wave's row (and, the first time, WX) is in LDS; the last channel's T has been read
      if (r < q.nr) T[r * RS_TW + lane] = rs_horizontal(WX, ROW, q, ax.taps, lane);
    }
    __syncthreads();
    for (int k = 0; k < rpw; ++k) {
      const int yo = t.y0 + wave * rpw + k;
      float o = 0.0f;
      if (yo < h && q.nxo > 0) o = fminf(fmaxf(rs_vertical(ay, T, yo, q.ya, lane), 0.0f), 1.0f);
      out[c * plane + (int64_t)k * Wp] = o;
    }
  }
}

template <int PATH, bool REF>
__global__ __launch_bounds__(256) void egress_u8_scaled_kernel(const float* __restrict__ src, RsStride3 ss, RsAxis ax,
                                                               RsAxis ay, uint8_t* __restrict__ dst, RsStride4 ds,
                                                               const uint8_t* __restrict__ ref, RsStride4 rs,
                                                               unsigned long long* __restrict__ sq_err, RsGeom g) {
  extern __shared__ float rs_lds[];
  __shared__ unsigned int red[4];
  float* WX = rs_lds;
  float* T = WX + ax.taps * RS_TW;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* ROW = T + g.t_rows * RS_TW + wave * g.row_cap;
  uint32_t* OB = reinterpret_cast<uint32_t*>(T + g.t_rows * RS_TW + 4 * g.row_cap);  // [R][RS_OB]
  const RsTile t = rs_tile(g);  // the tiles cover Ho x Wo only: y0 < Ho, x0 < Wo
  const int Ho = ay.Lo, Wo = ax.Lo, rpw = g.R / 4;
  const RsWin q = rs_window(ax, ay, t, g.R, lane);
  rs_stage_wx(ax, t.x0, WX, lane, wave);
  const float* win = src + t.img * ss.img + (int64_t)q.ya * ss.row + q.xa;
  uint8_t* tile = dst + t.img * ds.img + (int64_t)t.x0 * ds.col;  // + yo * ds.row: the row's first byte of the tile
  const int nx = min(RS_TW, Wo - t.x0);
  unsigned int sq = 0;  // <= 3 * rpw * 255^2 per lane
  for (int c = 0; c < 3; ++c) {
    for (int r0 = 0; r0 < q.nr; r0 += 4) {
      const int r = r0 + wave;
      if (r < q.nr) {
        const float* rp = win + c * ss.ch + (int64_t)r * ss.row;
        for (int k = lane; k < q.nc; k += 64) ROW[k] = fminf(fmaxf(rp[k], 0.0f), 1.0f);
      }
      __syncthreads();
      if (r < q.nr) T[r * RS_TW + lane] = rs_horizontal(WX, ROW, q, ax.taps, lane);
    }
    __syncthreads();
    for (int k = 0; k < rpw; ++k) {
      const int rl = wave * rpw + k, yo = t.y0 + rl;
      if (yo >= Ho || lane >= nx) continue;
      const float v = rs_vertical(ay, T, yo, q.ya, lane);
      const uint8_t u = (uint8_t)floorf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f);
      uint8_t* row = tile + (int64_t)yo * ds.row;
      uint8_t* ob = reinterpret_cast<uint8_t*>(OB + rl * RS_OB);
      if (PATH == RS_HWC) ob[addr_mod4(row) + 3 * lane + c] = u;
      else if (PATH == RS_CHW) ob[c * (RS_OB / 3) * 4 + addr_mod4(row + c * ds.ch) + lane] = u;
      else row[(int64_t)lane * ds.col + c * ds.ch] = u;
      if (REF) {
        const int d = (int)u - (int)ref[t.img * rs.img + (int64_t)yo * rs.row + (int64_t)(t.x0 + lane) * rs.col + c * rs.ch];
        sq += (unsigned int)(d * d);
      }
    }
  }
  if (PATH != RS_GENERAL) {
    __syncthreads();
    for (int k = 0; k < rpw; ++k) {
      const int rl = wave * rpw + k, yo = t.y0 + rl;
      if (yo >= Ho) break;
      uint8_t* row = tile + (int64_t)yo * ds.row;
      if (PATH == RS_HWC) stage_out(row, 3 * nx, OB + rl * RS_OB, lane);
      if (PATH == RS_CHW) {
        for (int c = 0; c < 3; ++c) stage_out(row + c * ds.ch, nx, OB + rl * RS_OB + c * (RS_OB / 3), lane);
      }
    }
  }
  if (REF) {
    // a wave's sum is at most 64 * 3 * 4 * 255^2 < 2^26
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sq += __shfl_down(sq, off, 64);
    if (lane == 0) red[wave] = sq;
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned long long sum =
          (unsigned long long)red[0] + (unsigned long long)red[1] + (unsigned long long)red[2] + (unsigned long long)red[3];
      if (sum) atomicAdd(sq_err + t.img, sum);
    }
  }
}

// ---- the tables on the device, built once per (device, filter, Li, Lo) and kept for the life of the library
struct RsTable {
  std::vector<int32_t> start, count;
  int taps = 0, Li = 0, Lo = 0;
  void* dev = nullptr;
  RsAxis axis() const {
    const int32_t* p = static_cast<const int32_t*>(dev);
    return RsAxis{p, p + Lo, reinterpret_cast<const float*>(p + 2 * (size_t)Lo), taps, Li, Lo};
  }
  // the widest input window of `tile` consecutive outputs starting at multiples of `tile`
  int window(int tile) const {
    int most = 0;
    for (int o = 0; o < Lo; o += tile) {
      const int last = std::min(o + tile, Lo) - 1;
      most = std::max(most, start[last] + count[last] - start[o]);
    }
    return most;
  }
};

const RsTable& rs_table(int filter, int Li, int Lo) {
  static std::mutex mu;
  static std::map<std::tuple<int, int, int, int>, std::unique_ptr<RsTable>> cache;
  int dev = 0;
  HIP_OK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  auto& slot = cache[std::make_tuple(dev, filter, Li, Lo)];
  if (slot) return *slot;
  auto t = std::make_unique<RsTable>();
  t->Li = Li;
  t->Lo = Lo;
  if (const char* err = resample_table(filter, Li, Lo, nullptr, nullptr, nullptr, 0, &t->taps))
    throw Error(std::string("mlic: ") + err);
  t->start.resize((size_t)Lo);
  t->count.resize((size_t)Lo);
  std::vector<float> w((size_t)Lo * t->taps);
  if (const char* err = resample_table(filter, Li, Lo, t->start.data(), t->count.data(), w.data(), t->taps, &t->taps))
    throw Error(std::string("mlic: ") + err);
  // one allocation: start[Lo] | count[Lo] | w[Lo][taps]; the copies return with the data on the device
  const size_t ints = sizeof(int32_t) * (size_t)Lo, bytes = 2 * ints + sizeof(float) * w.size();
  HIP_OK(hipMalloc(&t->dev, bytes));
  uint8_t* d = static_cast<uint8_t*>(t->dev);
  hipError_t e = hipMemcpy(d, t->start.data(), ints, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + ints, t->count.data(), ints, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + 2 * ints, w.data(), sizeof(float) * w.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(t->dev);
    HIP_OK(e);
  }
  slot = std::move(t);
  return *slot;
}

// rows per tile, LDS floats and grid of a launch; egress adds the tile's byte rows
RsGeom rs_geom(const RsTable& tx, const RsTable& ty, int B, int rows, int cols, bool egress, size_t* lds_bytes,
               unsigned* blocks, const char* who) {
  RsGeom g{};
  g.row_cap = tx.window(RS_TW);
  for (int R : {16, 8}) {
    g.R = R;
    g.t_rows = ty.window(R);
    *lds_bytes = sizeof(float) * ((size_t)tx.taps * RS_TW + (size_t)g.t_rows * RS_TW + 4 * (size_t)g.row_cap +
                                  (egress ? (size_t)R * RS_OB : 0));
    if (*lds_bytes <= RS_LDS_MAX) break;
  }
  // R = 8 at the widest tables: 49 * 64 + (7 * 8 + 49) * 64 + 4 * (63 * 8 + 49) + 8 * 51 floats = 50 KiB
  MLIC_CHECK(*lds_bytes <= RS_LDS_MAX, std::string(who) + ": the tile's window does not fit LDS (internal)");
  g.tiles_x = (cols + RS_TW - 1) / RS_TW;
  g.tiles_y = (rows + g.R - 1) / g.R;
  const int64_t n = (int64_t)B * g.tiles_x * g.tiles_y;
  MLIC_CHECK(n <= 0x7fffffffLL, std::string(who) + ": batch too large for one launch");
  *blocks = (unsigned)n;
  return g;
}

void rs_sizes_check(int filter, int Hi, int Wi, int Ho, int Wo, const char* who) {
  const char* err = resample_axis_check(filter, Hi, Ho);
  if (!err) err = resample_axis_check(filter, Wi, Wo);
  if (err) throw Error(std::string("mlic: ") + who + ": " + err);
}

int rs_path(const int64_t* s) {
  const bool hwc = s[2] == 3 && s[3] == 1, chw = s[2] == 1;
  const int forced = opt(OPT_IMAGE_IO_PATH);
  if (forced < 0) return hwc ? RS_HWC : chw ? RS_CHW : RS_GENERAL;
  MLIC_CHECK(forced != RS_HWC || hwc, "image_io_path 1 (HWC) needs column stride 3 and channel stride 1");
  MLIC_CHECK(forced != RS_CHW || chw, "image_io_path 2 (CHW) needs column stride 1");
  return forced;
}

template <int PATH>
void rs_egress_launch(unsigned blocks, size_t lds, hipStream_t st, const float* src, RsStride3 ss, RsAxis ax, RsAxis ay,
                      uint8_t* dst, RsStride4 ds, const uint8_t* ref, RsStride4 rs, uint64_t* sq, RsGeom g) {
  auto* sq64 = reinterpret_cast<unsigned long long*>(sq);
  if (ref)
    hipLaunchKernelGGL((egress_u8_scaled_kernel<PATH, true>), dim3(blocks), dim3(256), lds, st, src, ss, ax, ay, dst, ds,
                       ref, rs, sq64, g);
  else
    hipLaunchKernelGGL((egress_u8_scaled_kernel<PATH, false>), dim3(blocks), dim3(256), lds, st, src, ss, ax, ay, dst, ds,
                       ref, rs, sq64, g);
}

}  // namespace

void image_ingest_u8_scaled(const uint8_t* src, const int64_t* s, int B, int Hi, int Wi, int filter, int h, int w,
                            float* dst, int Hp, int Wp, hipStream_t st) {
  MLIC_CHECK(src != nullptr && s != nullptr && dst != nullptr, "image_ingest_u8_scaled: null argument");
  MLIC_CHECK(B >= 1, "image_ingest_u8_scaled: B must be positive");
  rs_sizes_check(filter, Hi, Wi, h, w, "image_ingest_u8_scaled");
  MLIC_CHECK(Hp >= h && Wp >= w && Hp % 64 == 0 && Wp % 64 == 0,
             "image_ingest_u8_scaled: Hp, Wp must be multiples of 64 that cover the coded size");
  MLIC_CHECK(s[2] != 0 && s[3] != 0, "image_ingest_u8_scaled: zero column or channel stride");
  MLIC_CHECK(reinterpret_cast<uintptr_t>(dst) % 4 == 0, "image_ingest_u8_scaled: dst must be 4-byte aligned");
  const RsTable& tx = rs_table(filter, Wi, w);
  const RsTable& ty = rs_table(filter, Hi, h);
  size_t lds = 0;
  unsigned blocks = 0;
  const RsGeom g = rs_geom(tx, ty, B, Hp, Wp, false, &lds, &blocks, "image_ingest_u8_scaled");
  const RsStride4 ss{s[0], s[1], s[2], s[3]};
  hipLaunchKernelGGL(ingest_u8_scaled_kernel, dim3(blocks), dim3(256), lds, st, src, ss, tx.axis(), ty.axis(), dst, Hp,
                     Wp, g);
  HIP_OK(hipGetLastError());
}

void image_egress_u8_scaled(const float* src, const int64_t* s, int B, int h, int w, int filter, int Ho, int Wo,
                            uint8_t* dst, const int64_t* d, const uint8_t* ref, const int64_t* r, uint64_t* sq_err,
                            hipStream_t st) {
  MLIC_CHECK(src != nullptr && s != nullptr && dst != nullptr && d != nullptr, "image_egress_u8_scaled: null argument");
  MLIC_CHECK(B >= 1, "image_egress_u8_scaled: B must be positive");
  rs_sizes_check(filter, h, w, Ho, Wo, "image_egress_u8_scaled");
  MLIC_CHECK(d[2] != 0 && d[3] != 0, "image_egress_u8_scaled: zero column or channel stride (dst)");
  MLIC_CHECK((ref != nullptr) == (sq_err != nullptr), "image_egress_u8_scaled: ref and sq_err go together");
  MLIC_CHECK(ref == nullptr || (r != nullptr && r[2] != 0 && r[3] != 0),
             "image_egress_u8_scaled: ref needs strides with nonzero column and channel stride");
  MLIC_CHECK(reinterpret_cast<uintptr_t>(src) % 4 == 0 && reinterpret_cast<uintptr_t>(sq_err) % 8 == 0,
             "image_egress_u8_scaled: src must be 4-byte and sq_err 8-byte aligned");
  const int path = rs_path(d);
  const RsTable& tx = rs_table(filter, w, Wo);
  const RsTable& ty = rs_table(filter, h, Ho);
  size_t lds = 0;
  unsigned blocks = 0;
  const RsGeom g = rs_geom(tx, ty, B, Ho, Wo, true, &lds, &blocks, "image_egress_u8_scaled");
  const RsStride3 ss{s[0], s[1], s[2]};
  const RsStride4 ds{d[0], d[1], d[2], d[3]};
  const RsStride4 rs = ref ? RsStride4{r[0], r[1], r[2], r[3]} : RsStride4{0, 0, 0, 0};
  if (sq_err) HIP_OK(hipMemsetAsync(sq_err, 0, sizeof(uint64_t) * (size_t)B, st));
  const RsAxis ax = tx.axis(), ay = ty.axis();
  if (path == RS_HWC) rs_egress_launch<RS_HWC>(blocks, lds, st, src, ss, ax, ay, dst, ds, ref, rs, sq_err, g);
  else if (path == RS_CHW) rs_egress_launch<RS_CHW>(blocks, lds, st, src, ss, ax, ay, dst, ds, ref, rs, sq_err, g);
  else rs_egress_launch<RS_GENERAL>(blocks, lds, st, src, ss, ax, ay, dst, ds, ref, rs, sq_err, g);
  HIP_OK(hipGetLastError());
}

}  // namespace mlic
