// uint8 image ingest / egress (utils/testing.py:338-424: ToTensor -> pad ... crop -> uint8), one launch each.
//
// ingest: uint8 H x W x 3 images, read through element strides {image, row, column, channel}, become the
// model's input: fp32 [B][3][Hp][Wp], v / 255 inside the image (a true IEEE division: torch's CPU
// `u8.float().div(255)` bit for bit; v * (1 / 255.f) differs for 126 of the 256 values) and +0 in the
// right / bottom padding.  Every destination element is written.
// egress: the H x W crop of fp32 planes (element strides {image, channel, row}) becomes uint8,
// floor(clamp(v, 0, 1) * 255) as sq_err_u8_kernel and metrics.hip have it (fmaxf drops a NaN: NaN -> 0), written
// through {image, row, column, channel} strides; nothing outside the crop's bytes is written.  With a
// reference image the per-image sum of squared uint8 differences is accumulated in integers (exact,
// order-independent: one 64-bit integer atomic per block).
// blur3_pad: the rate loop's 3x3 prefilter on the padded fp32 planes, with the gather that compacts the images
// still over budget (its own comment below).
// tile_blend: egress of a region of a tiled image from its overlapping tiles, feathered seams (its own comment).
//
// A block is four waves; a wave owns one image row of the tile and 256 pixels of it.  Byte rows start at
// any address (W * 3 is odd for odd W), so the two canonical layouts go through LDS: the row segment sits
// in LDS at its global address mod 4, whole aligned dwords move as dwords, and the up to three bytes at
// either end move as bytes -- nothing outside the segment is read or written.  The fp32 side is one
// 256-byte row piece per wave instruction.  Any other stride set takes the general kernels (byte accesses
// straight from / to global memory); all forms give the same bits.
#include "container.h"
#include "image_stage.h"
#include "kernels.h"

namespace mlic {

namespace {

constexpr int IO_TW = 256, IO_ROWS = 4;        // tile: one row per wave, 4 pixels per lane
constexpr int IO_SEG = IO_TW / 4 + 1;          // dwords of a 256-byte segment at any alignment
constexpr int IO_LDS = 3 * IO_SEG;             // per wave: one 768-byte segment (HWC) or three of 256 (CHW)
// With a reference image a block walks this many row groups and issues one atomic for all of them: 69 120
// blocks' atomics onto 32 addresses (32 x 1080 x 1920, one group per block) cost 0.40 ms of that launch's 0.65
constexpr int IO_REF_GROUPS = 16;
enum { IO_GENERAL = 0, IO_HWC = 1, IO_CHW = 2 };

struct IoStride3 {
  int64_t img, ch, row;
};
struct IoStride4 {
  int64_t img, row, col, ch;
};

// stage_in / stage_out / addr_mod4: image_stage.h

// blockIdx.x = (image, row block, column tile), column tile fastest; y = this wave's row in the block's first
// row group (a row block is `rows` rows)
struct IoTile {
  int64_t img;
  int y, x0;
};
__device__ inline IoTile io_tile(int tiles_x, int tiles_y, int rows = IO_ROWS) {
  const int64_t t = blockIdx.x;
  const int64_t ry = t / tiles_x;
  IoTile o;
  o.x0 = (int)(t - ry * tiles_x) * IO_TW;
  o.img = ry / tiles_y;
  o.y = (int)(ry - o.img * tiles_y) * rows + (int)(threadIdx.x >> 6);
  return o;
}

template <int PATH>
__global__ __launch_bounds__(256) void ingest_u8_kernel(const uint8_t* __restrict__ src, IoStride4 s, int H, int W,
                                                        float* __restrict__ dst, int Hp, int Wp, int tiles_x,
                                                        int tiles_y) {
  __shared__ uint32_t S[IO_ROWS][IO_LDS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const IoTile t = io_tile(tiles_x, tiles_y);
  // pixels of this wave's row segment that lie inside the image (the rest is padding)
  const int nx = t.y < H ? min(IO_TW, max(W - t.x0, 0)) : 0;
  const uint8_t* row = src + t.img * s.img + (int64_t)t.y * s.row + (int64_t)t.x0 * s.col;  // used when nx > 0
  int sh[3] = {0, 0, 0};
  if (PATH == IO_HWC && nx > 0) {
    sh[0] = addr_mod4(row);
    stage_in(row, 3 * nx, S[wave], lane);
  }
  if (PATH == IO_CHW && nx > 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      sh[c] = addr_mod4(row + c * s.ch);
      stage_in(row + c * s.ch, nx, S[wave] + c * IO_SEG, lane);
    }
  }
  if (PATH != IO_GENERAL) __syncthreads();
  const uint8_t* S8 = reinterpret_cast<const uint8_t*>(S[wave]);
  const int64_t plane = (int64_t)Hp * Wp;
  float* out = dst + t.img * 3 * plane + (int64_t)t.y * Wp + t.x0;
#pragma unroll
  for (int j = 0; j < IO_TW / 64; ++j) {
    const int px = lane + 64 * j;
    if (t.x0 + px >= Wp) break;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = 0.0f;
      if (px < nx) {
        uint8_t u;
        if (PATH == IO_HWC) u = S8[sh[0] + 3 * px + c];
        else if (PATH == IO_CHW) u = S8[c * IO_SEG * 4 + sh[c] + px];
        else u = row[(int64_t)px * s.col + c * s.ch];
        v = (float)u / 255.0f;  // correctly rounded (hipcc's default for fp32 division)
      }
      out[c * plane + px] = v;
    }
  }
}

template <int PATH, bool REF>
__global__ __launch_bounds__(256) void egress_u8_kernel(const float* __restrict__ src, IoStride3 ss, int H, int W,
                                                        uint8_t* __restrict__ dst, IoStride4 ds,
                                                        const uint8_t* __restrict__ ref, IoStride4 rs,
                                                        unsigned long long* __restrict__ sq_err, int tiles_x,
                                                        int tiles_y) {
  __shared__ uint32_t S[IO_ROWS][IO_LDS];
  __shared__ unsigned int red[IO_ROWS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int G = REF ? IO_REF_GROUPS : 1;  // row groups this block walks
  const IoTile t = io_tile(tiles_x, tiles_y, G * IO_ROWS);
  uint8_t* S8 = reinterpret_cast<uint8_t*>(S[wave]);
  unsigned int acc = 0;  // <= G * 4 * 3 * 255^2 per lane
  for (int g = 0; g < G; ++g) {
    const int y = t.y + g * IO_ROWS;
    const int nx = y < H ? min(IO_TW, W - t.x0) : 0;  // x0 < W: the tiles cover the crop only
    const float* in = src + t.img * ss.img + (int64_t)y * ss.row + t.x0;
    uint8_t* row = dst + t.img * ds.img + (int64_t)y * ds.row + (int64_t)t.x0 * ds.col;
    const uint8_t* rrow = REF ? ref + t.img * rs.img + (int64_t)y * rs.row + (int64_t)t.x0 * rs.col : nullptr;
    int sh[3] = {0, 0, 0};
    if (PATH == IO_HWC) sh[0] = addr_mod4(row);
    if (PATH == IO_CHW) {
#pragma unroll
      for (int c = 0; c < 3; ++c) sh[c] = addr_mod4(row + c * ds.ch);
    }
#pragma unroll
    for (int j = 0; j < IO_TW / 64; ++j) {
      const int px = lane + 64 * j;
      if (px >= nx) break;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v = in[c * ss.ch + px];
        const uint8_t u = (uint8_t)floorf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f);
        if (PATH == IO_HWC) S8[sh[0] + 3 * px + c] = u;
        else if (PATH == IO_CHW) S8[c * IO_SEG * 4 + sh[c] + px] = u;
        else row[(int64_t)px * ds.col + c * ds.ch] = u;
        if (REF) {
          const int d = (int)u - (int)rrow[(int64_t)px * rs.col + c * rs.ch];
          acc += (unsigned int)(d * d);
        }
      }
    }
    if (PATH != IO_GENERAL) {
      __syncthreads();
      if (PATH == IO_HWC && nx > 0) stage_out(row, 3 * nx, S[wave], lane);
      if (PATH == IO_CHW && nx > 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) stage_out(row + c * ds.ch, nx, S[wave] + c * IO_SEG, lane);
      }
      if (G > 1) __syncthreads();  // the next group's bytes go into the same LDS
    }
  }
  if (REF) {
    // a wave's sum is at most 64 * G * 4 * 3 * 255^2 < 2^30
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned long long s =
          (unsigned long long)red[0] + (unsigned long long)red[1] + (unsigned long long)red[2] + (unsigned long long)red[3];
      if (s) atomicAdd(sq_err + t.img, s);
    }
  }
}

// Tiled decode's egress (DESIGN.md section 5 "Tiled coding"): the h x w region at (y0, x0) of the full image as
// uint8, blended from the fp32 planes of the tiles that cover it.  tiles[ky * nx + kx] is tile (ky, kx)'s
// contiguous [3][pad64(extent_y)][pad64(extent_x)] planes or null (the host checked that no covering tile is
// null; a null is skipped all the same).  Per pixel and channel acc (double) = 0; acc += (double)(wy * wx) *
// (double)v over the covering tiles, tile row then tile column; wy * wx is a dyadic rational of at most 14 bits
// (exact in fp32), so each product is exact in double and the sums are rounded in that fixed order.  Then
// (float)acc goes through egress_u8_kernel's conversion, staging and squared-error sum.  egress_u8_kernel's
// structure: a wave owns one region row and 256 pixels of it.  Which tile rows and columns cover the piece is
// decided once per piece (scalar); a lane only tests whether its pixel lies inside the tile column at hand, and a
// piece that one tile covers outside every strip (most of them) skips the weights and the doubles altogether.
struct BlendGrid {
  int H, W, T, V, ny, nx;
};

template <int PATH, bool REF>
__global__ __launch_bounds__(256) void tile_blend_u8_kernel(const float* const* __restrict__ tiles, BlendGrid q,
                                                            int y0, int x0, int h, int w, uint8_t* __restrict__ dst,
                                                            IoStride4 ds, const uint8_t* __restrict__ ref,
                                                            IoStride4 rs, unsigned long long* __restrict__ sq_err,
                                                            int tiles_x, int tiles_y) {
  __shared__ uint32_t S[IO_ROWS][IO_LDS];
  __shared__ unsigned int red[IO_ROWS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int G = REF ? IO_REF_GROUPS : 1;
  const IoTile t = io_tile(tiles_x, tiles_y, G * IO_ROWS);  // one "image": t.img = 0
  uint8_t* S8 = reinterpret_cast<uint8_t*>(S[wave]);
  const int step = q.T - q.V, den = q.V ? 2 * q.V : 1;
  const float inv = 1.0f / (float)(den * den);  // a power of two
  unsigned int acc_sq = 0;
  for (int g = 0; g < G; ++g) {
    const int y = t.y + g * IO_ROWS;
    const int nx = y < h ? min(IO_TW, w - t.x0) : 0;
    uint8_t* row = dst + (int64_t)y * ds.row + (int64_t)t.x0 * ds.col;
    const uint8_t* rrow = REF ? ref + (int64_t)y * rs.row + (int64_t)t.x0 * rs.col : nullptr;
    float val[IO_TW / 64][3];  // (float)acc per pixel of this lane
#pragma unroll
    for (int j = 0; j < IO_TW / 64; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) val[j][c] = 0.0f;
    if (nx > 0) {
      const int Y = y0 + y, X0 = x0 + t.x0;  // Y < H, X0 + nx <= W: the host checked the region
      const int ky1 = min(Y / step, q.ny - 1);
      const int ky0 = (ky1 > 0 && Y - ky1 * step < q.V) ? ky1 - 1 : ky1;
      int kxa = min(X0 / step, q.nx - 1);
      if (kxa > 0 && X0 - kxa * step < q.V) --kxa;
      const int kxb = min((X0 + nx - 1) / step, q.nx - 1);
      if (ky0 == ky1 && kxa == kxb) {
        // One tile covers the whole piece and no pixel of it lies in a strip (the row is in no strip with tile
        // row ky1 - 1 and below the one with ky1 + 1; likewise the columns): every weight is 1 and acc = 0 + 1 * v
        // is v (a -0 becomes +0, which the clamp does too), so this is egress_u8_kernel's read
        const float* p = tiles[(int64_t)ky1 * q.nx + kxa];
        if (p != nullptr) {
          const int hp = (min(q.T, q.H - ky1 * step) + 63) & ~63, wp = (min(q.T, q.W - kxa * step) + 63) & ~63;
          const int64_t plane = (int64_t)hp * wp;
          const float* in = p + (int64_t)(Y - ky1 * step) * wp + (X0 - kxa * step);
#pragma unroll
          for (int j = 0; j < IO_TW / 64; ++j) {
            const int px = lane + 64 * j;
            if (px >= nx) break;
#pragma unroll
            for (int c = 0; c < 3; ++c) val[j][c] = in[c * plane + px];
          }
        }
      } else {
        double acc[IO_TW / 64][3];
#pragma unroll
        for (int j = 0; j < IO_TW / 64; ++j)
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[j][c] = 0.0;
        for (int ky = ky0; ky <= ky1; ++ky) {
          const int ly = Y - ky * step;  // 0 <= ly < extent of tile row ky
          const int hp = (min(q.T, q.H - ky * step) + 63) & ~63;
          const int numy = (int)tile_weight_num((uint32_t)ly, (uint32_t)ky, (uint32_t)q.ny, (uint32_t)q.T, (uint32_t)q.V);
          for (int kx = kxa; kx <= kxb; ++kx) {
            const float* p = tiles[(int64_t)ky * q.nx + kx];
            if (p == nullptr) continue;
            const int ext = min(q.T, q.W - kx * step), wp = (ext + 63) & ~63;
            const int64_t plane = (int64_t)hp * wp;
            const float* in = p + (int64_t)ly * wp;
            // every lane loads from a position clamped into the tile's row, so the twelve loads of a tile column
            // go out together; a pixel outside the tile keeps its sum (a select, not a product with 0)
            float v[IO_TW / 64][3];
            int lxs[IO_TW / 64];
#pragma unroll
            for (int j = 0; j < IO_TW / 64; ++j) {
              lxs[j] = X0 + lane + 64 * j - kx * step;
              const int at = min(max(lxs[j], 0), ext - 1);
#pragma unroll
              for (int c = 0; c < 3; ++c) v[j][c] = in[c * plane + at];
            }
#pragma unroll
            for (int j = 0; j < IO_TW / 64; ++j) {
              const int lx = lxs[j];
              const bool inside = lane + 64 * j < nx && lx >= 0 && lx < ext;
              const int numx = (int)tile_weight_num((uint32_t)min(max(lx, 0), ext - 1), (uint32_t)kx, (uint32_t)q.nx,
                                                    (uint32_t)q.T, (uint32_t)q.V);
              const double wgt = (double)((float)(numy * numx) * inv);
#pragma unroll
              for (int c = 0; c < 3; ++c) {
                const double sum = __dadd_rn(acc[j][c], __dmul_rn(wgt, (double)v[j][c]));
                acc[j][c] = inside ? sum : acc[j][c];
              }
            }
          }
        }
#pragma unroll
        for (int j = 0; j < IO_TW / 64; ++j)
#pragma unroll
          for (int c = 0; c < 3; ++c) val[j][c] = (float)acc[j][c];
      }
    }
    int sh[3] = {0, 0, 0};
    if (PATH == IO_HWC) sh[0] = addr_mod4(row);
    if (PATH == IO_CHW) {
#pragma unroll
      for (int c = 0; c < 3; ++c) sh[c] = addr_mod4(row + c * ds.ch);
    }
#pragma unroll
    for (int j = 0; j < IO_TW / 64; ++j) {
      const int px = lane + 64 * j;
      if (px >= nx) break;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const uint8_t u = (uint8_t)floorf(fminf(fmaxf(val[j][c], 0.0f), 1.0f) * 255.0f);
        if (PATH == IO_HWC) S8[sh[0] + 3 * px + c] = u;
        else if (PATH == IO_CHW) S8[c * IO_SEG * 4 + sh[c] + px] = u;
        else row[(int64_t)px * ds.col + c * ds.ch] = u;
        if (REF) {
          const int d = (int)u - (int)rrow[(int64_t)px * rs.col + c * rs.ch];
          acc_sq += (unsigned int)(d * d);
        }
      }
    }
    if (PATH != IO_GENERAL) {
      __syncthreads();
      if (PATH == IO_HWC && nx > 0) stage_out(row, 3 * nx, S[wave], lane);
      if (PATH == IO_CHW && nx > 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) stage_out(row + c * ds.ch, nx, S[wave] + c * IO_SEG, lane);
      }
      if (G > 1) __syncthreads();
    }
  }
  if (REF) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc_sq += __shfl_down(acc_sq, off, 64);
    if (lane == 0) red[wave] = acc_sq;
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned long long s =
          (unsigned long long)red[0] + (unsigned long long)red[1] + (unsigned long long)red[2] + (unsigned long long)red[3];
      if (s) atomicAdd(sq_err, s);
    }
  }
}

// The rate loop's prefilter (utils/testing.py:363-390: crop, 3x3 depthwise conv with padding 1, pad to 64
// again) on the padded fp32 planes, one read and one write of the plane.  A thread owns BL_RUN consecutive
// columns of BL_ROWS consecutive rows: 256 threads are whole row groups (Wp / BL_RUN is a multiple of 16), a
// block never leaves its plane (Hp * Wp / (BL_RUN * BL_ROWS) is a multiple of 256) and a wave's loads and
// stores are contiguous 16-byte pieces (one float4 per lane when both buffers are 16-byte aligned).  The
// BL_ROWS + 2 input rows are read once each and feed up to three output rows from registers; the columns left
// and right of a run come from the neighbouring lanes (a wave shuffle), and from memory only at the two ends of
// a wave.  A tap outside the H x W image is 0 whatever the padded buffer holds there, and every element is
// written (0 from column W / row H).  Per element: acc = 0; acc = acc + w[t] * v[t], t row-major (dy, then
// dx), each product and each sum rounded once.
constexpr int BL_RUN = 4, BL_ROWS = 4;

struct Blur9 {
  float w[9];
};

template <bool VEC>
__global__ __launch_bounds__(256) void blur3_pad_kernel(const float* __restrict__ src,
                                                        const int32_t* __restrict__ src_index, int H, int W, int Hp,
                                                        int Wp, Blur9 k, float* __restrict__ dst,
                                                        unsigned plane_blocks) {
  const unsigned pc = blockIdx.x / plane_blocks;  // output plane: image * 3 + channel
  const int q = (int)(blockIdx.x - pc * plane_blocks) * 256 + (int)threadIdx.x;  // run group within the plane
  const int rw = Wp / BL_RUN;
  const int yb = q / rw, x0 = (q - yb * rw) * BL_RUN, y0 = yb * BL_ROWS;
  const int lane = threadIdx.x & 63;
  const unsigned img = pc / 3, c = pc - 3 * img;
  const int64_t from = src_index ? (int64_t)src_index[img] : (int64_t)img;
  const int64_t plane = (int64_t)Hp * Wp;
  const float* sp = src + (from * 3 + c) * plane + x0;
  // rows start at multiples of 16 lanes, so lane - 1 (lane + 1) holds the run to the left (right) in the same
  // rows unless this run is the first (last) of its row or this lane the first (last) of its wave
  const bool left_lane = lane > 0 && x0 > 0, right_lane = lane < 63 && x0 + BL_RUN < Wp;
  float acc[BL_ROWS][BL_RUN];
#pragma unroll
  for (int r = 0; r < BL_ROWS; ++r)
#pragma unroll
    for (int e = 0; e < BL_RUN; ++e) acc[r][e] = 0.0f;
  // every lane takes every step (the shuffles need the whole wave); a lane outside the image holds zeros
#pragma unroll
  for (int j = 0; j < BL_ROWS + 2; ++j) {
    const int yy = y0 - 1 + j;
    const bool row = yy >= 0 && yy < H;
    const float* rp = sp + (int64_t)yy * Wp;  // dereferenced only inside the image
    float v[BL_RUN + 2];                      // columns x0 - 1 .. x0 + BL_RUN, 0 outside the image
#pragma unroll
    for (int e = 0; e < BL_RUN + 2; ++e) v[e] = 0.0f;
    if (row && x0 < W) {
      float m[BL_RUN];
      if (VEC) {
        const float4 f = *reinterpret_cast<const float4*>(rp);  // x0 + BL_RUN <= Wp: inside the row
        m[0] = f.x, m[1] = f.y, m[2] = f.z, m[3] = f.w;
      } else {
#pragma unroll
        for (int e = 0; e < BL_RUN; ++e) m[e] = rp[e];
      }
#pragma unroll
      for (int e = 0; e < BL_RUN; ++e) v[e + 1] = x0 + e < W ? m[e] : 0.0f;
    }
    const float lf = __shfl_up(v[BL_RUN], 1, 64), rt = __shfl_down(v[1], 1, 64);
    if (left_lane) v[0] = lf;
    else if (row && x0 > 0 && x0 < W) v[0] = rp[-1];
    if (right_lane) v[BL_RUN + 1] = rt;
    else if (row && x0 + BL_RUN < W) v[BL_RUN + 1] = rp[BL_RUN];
#pragma unroll
    for (int r = 0; r < BL_ROWS; ++r) {
      const int dy = j - r - 1;  // input row j is tap row dy of output row r
      if (dy < -1 || dy > 1) continue;
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const float w = k.w[(dy + 1) * 3 + dx];
#pragma unroll
        for (int e = 0; e < BL_RUN; ++e) acc[r][e] = __fadd_rn(acc[r][e], __fmul_rn(w, v[e + dx]));
      }
    }
  }
  float* dp = dst + (int64_t)pc * plane + (int64_t)y0 * Wp + x0;
#pragma unroll
  for (int r = 0; r < BL_ROWS; ++r) {
    float o[BL_RUN];
#pragma unroll
    for (int e = 0; e < BL_RUN; ++e) o[e] = y0 + r < H && x0 + e < W ? acc[r][e] : 0.0f;
    if (VEC) {
      *reinterpret_cast<float4*>(dp + (int64_t)r * Wp) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int e = 0; e < BL_RUN; ++e) dp[(int64_t)r * Wp + e] = o[e];
    }
  }
}

// the kernel form for a byte image with these strides; throws when a forced form does not fit
int io_path(const int64_t* s) {
  const bool hwc = s[2] == 3 && s[3] == 1, chw = s[2] == 1;
  const int forced = opt(OPT_IMAGE_IO_PATH);
  if (forced < 0) return hwc ? IO_HWC : chw ? IO_CHW : IO_GENERAL;
  MLIC_CHECK(forced != IO_HWC || hwc, "image_io_path 1 (HWC) needs column stride 3 and channel stride 1");
  MLIC_CHECK(forced != IO_CHW || chw, "image_io_path 2 (CHW) needs column stride 1");
  return forced;
}

unsigned io_blocks(int B, int rows, int cols, int* tiles_x, int* tiles_y, int block_rows = IO_ROWS) {
  *tiles_x = (cols + IO_TW - 1) / IO_TW;
  *tiles_y = (rows + block_rows - 1) / block_rows;
  const int64_t blocks = (int64_t)B * *tiles_x * *tiles_y;
  MLIC_CHECK(blocks <= 0x7fffffffLL, "image_io: batch too large for one launch");
  return (unsigned)blocks;
}

}  // namespace

void image_ingest_u8(const uint8_t* src, const int64_t* s, int B, int H, int W, float* dst, int Hp, int Wp,
                     hipStream_t st) {
  MLIC_CHECK(src != nullptr && s != nullptr && dst != nullptr, "image_ingest_u8: null argument");
  MLIC_CHECK(B >= 1 && H >= 1 && W >= 1, "image_ingest_u8: B, H and W must be positive");
  MLIC_CHECK(Hp >= H && Wp >= W && Hp % 64 == 0 && Wp % 64 == 0,
             "image_ingest_u8: Hp, Wp must be multiples of 64 that cover H, W");
  MLIC_CHECK(s[2] != 0 && s[3] != 0, "image_ingest_u8: zero column or channel stride");
  MLIC_CHECK(reinterpret_cast<uintptr_t>(dst) % 4 == 0, "image_ingest_u8: dst must be 4-byte aligned");
  const int path = io_path(s);
  int tx, ty;
  const unsigned blocks = io_blocks(B, Hp, Wp, &tx, &ty);
  const IoStride4 ss{s[0], s[1], s[2], s[3]};
  if (path == IO_HWC)
    hipLaunchKernelGGL(ingest_u8_kernel<IO_HWC>, dim3(blocks), dim3(256), 0, st, src, ss, H, W, dst, Hp, Wp, tx, ty);
  else if (path == IO_CHW)
    hipLaunchKernelGGL(ingest_u8_kernel<IO_CHW>, dim3(blocks), dim3(256), 0, st, src, ss, H, W, dst, Hp, Wp, tx, ty);
  else
    hipLaunchKernelGGL(ingest_u8_kernel<IO_GENERAL>, dim3(blocks), dim3(256), 0, st, src, ss, H, W, dst, Hp, Wp, tx, ty);
  HIP_OK(hipGetLastError());
}

template <int PATH>
static void egress_launch(unsigned blocks, hipStream_t st, const float* src, IoStride3 ss, int H, int W, uint8_t* dst,
                          IoStride4 ds, const uint8_t* ref, IoStride4 rs, uint64_t* sq, int tx, int ty) {
  auto* sq64 = reinterpret_cast<unsigned long long*>(sq);
  if (ref)
    hipLaunchKernelGGL((egress_u8_kernel<PATH, true>), dim3(blocks), dim3(256), 0, st, src, ss, H, W, dst, ds, ref, rs,
                       sq64, tx, ty);
  else
    hipLaunchKernelGGL((egress_u8_kernel<PATH, false>), dim3(blocks), dim3(256), 0, st, src, ss, H, W, dst, ds, ref, rs,
                       sq64, tx, ty);
}

void image_egress_u8(const float* src, const int64_t* s, int B, int H, int W, uint8_t* dst, const int64_t* d,
                     const uint8_t* ref, const int64_t* r, uint64_t* sq_err, hipStream_t st) {
  MLIC_CHECK(src != nullptr && s != nullptr && dst != nullptr && d != nullptr, "image_egress_u8: null argument");
  MLIC_CHECK(B >= 1 && H >= 1 && W >= 1, "image_egress_u8: B, H and W must be positive");
  MLIC_CHECK(d[2] != 0 && d[3] != 0, "image_egress_u8: zero column or channel stride (dst)");
  MLIC_CHECK((ref != nullptr) == (sq_err != nullptr), "image_egress_u8: ref and sq_err go together");
  MLIC_CHECK(ref == nullptr || (r != nullptr && r[2] != 0 && r[3] != 0),
             "image_egress_u8: ref needs strides with nonzero column and channel stride");
  MLIC_CHECK(reinterpret_cast<uintptr_t>(src) % 4 == 0 && reinterpret_cast<uintptr_t>(sq_err) % 8 == 0,
             "image_egress_u8: src must be 4-byte and sq_err 8-byte aligned");
  const int path = io_path(d);
  int tx, ty;
  const unsigned blocks = io_blocks(B, H, W, &tx, &ty, (ref ? IO_REF_GROUPS : 1) * IO_ROWS);
  const IoStride3 ss{s[0], s[1], s[2]};
  const IoStride4 ds{d[0], d[1], d[2], d[3]};
  const IoStride4 rs = ref ? IoStride4{r[0], r[1], r[2], r[3]} : IoStride4{0, 0, 0, 0};
  if (sq_err) HIP_OK(hipMemsetAsync(sq_err, 0, sizeof(uint64_t) * (size_t)B, st));
  if (path == IO_HWC) egress_launch<IO_HWC>(blocks, st, src, ss, H, W, dst, ds, ref, rs, sq_err, tx, ty);
  else if (path == IO_CHW) egress_launch<IO_CHW>(blocks, st, src, ss, H, W, dst, ds, ref, rs, sq_err, tx, ty);
  else egress_launch<IO_GENERAL>(blocks, st, src, ss, H, W, dst, ds, ref, rs, sq_err, tx, ty);
  HIP_OK(hipGetLastError());
}

template <int PATH>
static void blend_launch(unsigned blocks, hipStream_t st, const float* const* tiles, BlendGrid q, int y0, int x0, int h,
                         int w, uint8_t* dst, IoStride4 ds, const uint8_t* ref, IoStride4 rs, uint64_t* sq, int tx,
                         int ty) {
  auto* sq64 = reinterpret_cast<unsigned long long*>(sq);
  if (ref)
    hipLaunchKernelGGL((tile_blend_u8_kernel<PATH, true>), dim3(blocks), dim3(256), 0, st, tiles, q, y0, x0, h, w, dst,
                       ds, ref, rs, sq64, tx, ty);
  else
    hipLaunchKernelGGL((tile_blend_u8_kernel<PATH, false>), dim3(blocks), dim3(256), 0, st, tiles, q, y0, x0, h, w, dst,
                       ds, ref, rs, sq64, tx, ty);
}

void image_tile_blend_u8(const float* const* tiles_dev, const float* const* tiles_host, int H, int W, int T, int V,
                         int y0, int x0, int h, int w, uint8_t* dst, const int64_t* d, const uint8_t* ref,
                         const int64_t* r, uint64_t* sq_err, hipStream_t st) {
  MLIC_CHECK(tiles_dev != nullptr && tiles_host != nullptr && dst != nullptr && d != nullptr,
             "image_tile_blend_u8: null argument");
  MLIC_CHECK(H >= 1 && W >= 1 && H <= (1 << 24) && W <= (1 << 24), "image_tile_blend_u8: H, W in [1, 2^24] expected");
  MLIC_CHECK(T >= 0 && V >= 0, "image_tile_blend_u8: negative tile or overlap");
  if (const char* err = tile_params_check((uint32_t)T, (uint32_t)V))
    throw Error(std::string("mlic: image_tile_blend_u8: ") + err);
  MLIC_CHECK(h >= 1 && w >= 1 && y0 >= 0 && x0 >= 0 && y0 <= H - h && x0 <= W - w,
             "image_tile_blend_u8: the region must be non-empty and inside the image");
  MLIC_CHECK(d[1] != 0 && d[2] != 0, "image_tile_blend_u8: zero column or channel stride (dst)");
  MLIC_CHECK((ref != nullptr) == (sq_err != nullptr), "image_tile_blend_u8: ref and sq_err go together");
  MLIC_CHECK(ref == nullptr || (r != nullptr && r[1] != 0 && r[2] != 0),
             "image_tile_blend_u8: ref needs strides with nonzero column and channel stride");
  MLIC_CHECK(reinterpret_cast<uintptr_t>(tiles_dev) % 8 == 0 && reinterpret_cast<uintptr_t>(sq_err) % 8 == 0,
             "image_tile_blend_u8: the tile table and sq_err must be 8-byte aligned");
  const int ny = (int)tile_count((uint32_t)H, (uint32_t)T, (uint32_t)V);
  const int nx = (int)tile_count((uint32_t)W, (uint32_t)T, (uint32_t)V);
  // every tile that intersects the region must be there
  const int step = T - V;
  auto first = [&](int p, int n) {
    int k = std::min(p / step, n - 1);
    return (k > 0 && p - k * step < V) ? k - 1 : k;
  };
  const int ky0 = first(y0, ny), ky1 = std::min((y0 + h - 1) / step, ny - 1);
  const int kx0 = first(x0, nx), kx1 = std::min((x0 + w - 1) / step, nx - 1);
  for (int ky = ky0; ky <= ky1; ++ky)
    for (int kx = kx0; kx <= kx1; ++kx) {
      const float* p = tiles_host[(size_t)ky * nx + kx];
      MLIC_CHECK(p != nullptr, "image_tile_blend_u8: a tile that covers the region is null");
      MLIC_CHECK(reinterpret_cast<uintptr_t>(p) % 4 == 0, "image_tile_blend_u8: a tile is not 4-byte aligned");
    }
  const int64_t d4[4] = {0, d[0], d[1], d[2]};
  const int path = io_path(d4);
  int tx, ty;
  const unsigned blocks = io_blocks(1, h, w, &tx, &ty, (ref ? IO_REF_GROUPS : 1) * IO_ROWS);
  const BlendGrid q{H, W, T, V, ny, nx};
  const IoStride4 ds{0, d[0], d[1], d[2]};
  const IoStride4 rs = ref ? IoStride4{0, r[0], r[1], r[2]} : IoStride4{0, 0, 0, 0};
  if (sq_err) HIP_OK(hipMemsetAsync(sq_err, 0, sizeof(uint64_t), st));
  if (path == IO_HWC) blend_launch<IO_HWC>(blocks, st, tiles_dev, q, y0, x0, h, w, dst, ds, ref, rs, sq_err, tx, ty);
  else if (path == IO_CHW) blend_launch<IO_CHW>(blocks, st, tiles_dev, q, y0, x0, h, w, dst, ds, ref, rs, sq_err, tx, ty);
  else blend_launch<IO_GENERAL>(blocks, st, tiles_dev, q, y0, x0, h, w, dst, ds, ref, rs, sq_err, tx, ty);
  HIP_OK(hipGetLastError());
}

void image_blur3_pad(const float* src, const int32_t* src_index, int n, int H, int W, int Hp, int Wp, const float* w9,
                     float* dst, hipStream_t st) {
  MLIC_CHECK(n >= 1, "image_blur3_pad: n must be positive");
  MLIC_CHECK(H >= 1 && W >= 1, "image_blur3_pad: H and W must be positive");
  MLIC_CHECK(Hp >= H && Wp >= W && Hp % 64 == 0 && Wp % 64 == 0,
             "image_blur3_pad: Hp, Wp must be multiples of 64 that cover H, W");
  MLIC_CHECK(src != nullptr && dst != nullptr, "image_blur3_pad: null src or dst");
  MLIC_CHECK(reinterpret_cast<uintptr_t>(src) % 4 == 0 && reinterpret_cast<uintptr_t>(dst) % 4 == 0,
             "image_blur3_pad: src and dst must be 4-byte aligned");
  const uint64_t plane = (uint64_t)Hp * (uint64_t)Wp;
  MLIC_CHECK(plane <= (1ull << 31), "image_blur3_pad: padded plane above 2^31 elements");
  const uint64_t plane_blocks = plane / (BL_RUN * BL_ROWS * 256);  // exact: 64 * 64 divides the plane
  const uint64_t blocks = (uint64_t)n * 3 * plane_blocks;
  MLIC_CHECK(blocks <= 0x7fffffffull, "image_blur3_pad: batch too large for one launch");
  // the n images on either side, with the source batch's size unknown: the stencil cannot run in place
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), d0 = reinterpret_cast<uintptr_t>(dst);
  const uint64_t bytes = (uint64_t)n * 3 * plane * sizeof(float);
  MLIC_CHECK(!(d0 >= s0 && d0 - s0 < bytes) && !(s0 >= d0 && s0 - d0 < bytes),
             "image_blur3_pad: dst overlaps src (the filter cannot run in place)");
  Blur9 k = {{0x1.73b62cp-7f, 0x1.575320p-4f, 0x1.73b62cp-7f, 0x1.575320p-4f, 0x1.3d1b0ep-1f, 0x1.575320p-4f,
              0x1.73b62cp-7f, 0x1.575320p-4f, 0x1.73b62cp-7f}};  // sigma 0.5, normalised (utils/testing.py:264-284)
  if (w9)
    for (int t = 0; t < 9; ++t) k.w[t] = w9[t];
  const bool vec = s0 % 16 == 0 && d0 % 16 == 0;  // planes and rows are multiples of 16 bytes
  if (vec)
    hipLaunchKernelGGL(blur3_pad_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, src, src_index, H, W, Hp, Wp, k,
                       dst, (unsigned)plane_blocks);
  else
    hipLaunchKernelGGL(blur3_pad_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, src, src_index, H, W, Hp, Wp,
                       k, dst, (unsigned)plane_blocks);
  HIP_OK(hipGetLastError());
}

}  // namespace mlic
