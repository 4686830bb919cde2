// 9..16-bit samples in and out (DESIGN.md section 5 "High-bit-depth I/O"): the RGB ingest / egress of image_io.hip
// and the Y'CbCr ingest / egress of image_yuv.hip for uint16 words, one launch each.  The 8-bit kernels are left
// as they are; these are their structure with samples twice as wide.
//
// A sample of depth d (8..16) is a uint16 word in native byte order: LSB-aligned (msb = 0: the sample is
// min(word, maxv), maxv = 2^d - 1) or MSB-aligned (msb = 1, P010 / P016: the sample is word >> (16 - d), the low
// bits of an input word are ignored and those of an output word are zero).  Strides are in elements.
//   ingest_u16:    v = (float)sample / (float)maxv (a true IEEE division), +0 in the padding, every element written
//   egress_u16:    sample = floor(min(max(v, 0), 1) * maxv), NaN -> 0; with ref the exact per-image sum of squared
//                  sample differences, 64 bits wide from the lane upwards (65535^2 is just under 2^32)
//   ingest_yuv16 / egress_yuv16: the rules of image_yuv.hip with 128 -> half = 2^(d-1), 255 -> maxv and the
//                  constants folded from ys, cs, yo of depth d; BT.2020 non-constant-luminance is matrix 2
//
// A block is four waves; a wave owns a row and 256 pixels of it.  Sample rows with a fast form go through LDS at
// their global address mod 4 (0 or 2: pointers are 2-byte aligned), whole dwords as dwords and the one sample at
// either end as a sample; nothing outside the row segment is read or written.  The Y'CbCr ingest issues every
// staged row's loads before the first LDS store.  All forms give the same bits.
#include "image_stage.h"
#include "kernels.h"

namespace mlic {

namespace {

constexpr int TW = 256, ROWS = 4;          // tile: one row per wave
constexpr int SEG = TW / 2 + 1;            // dwords of 256 samples at either alignment
constexpr int CSEG = TW / 2 + 2;           // Y'CbCr ingest: up to 258 chroma samples at either alignment
constexpr int RGB_LDS = 3 * SEG;           // per wave: one segment of 768 samples (HWC) or three of 256 (CHW)
constexpr int YUV_IN_LDS = SEG + 4 * CSEG; // Y | Cb row 0, Cb row 1, Cr row 0, Cr row 1 (NV: uv row 0, uv row 1)
constexpr int YUV_OUT_LDS = 4 * SEG;       // Y row 0, Y row 1 | Cb, Cr (NV: uv, up to 513 samples)
constexpr int RGB_REF_GROUPS = 16, YUV_REF_GROUPS = 8;  // image_io.hip IO_REF_GROUPS, image_yuv.hip YUV_REF_GROUPS
enum { IO_GENERAL = 0, IO_HWC = 1, IO_CHW = 2 };
enum { YUV_GENERAL = 0, YUV_PLANAR = 1, YUV_NV = 2 };

struct Fmt16 {
  int maxv, shift, msb;  // shift = 16 - depth
};
__device__ inline int sample_of(uint32_t word, const Fmt16& f) {
  return f.msb ? (int)(word >> f.shift) : min((int)word, f.maxv);
}
__device__ inline uint16_t word_of(int sample, const Fmt16& f) {
  return (uint16_t)(f.msb ? sample << f.shift : sample);
}

struct IoStride3 {
  int64_t img, ch, row;
};
struct IoStride4 {
  int64_t img, row, col, ch;
};
struct Tile {
  int64_t img;
  int y, x0;
};
// blockIdx.x = (image, row block, column tile), column tile fastest; y = this wave's row in the block's first
// row group (a row block is `rows` rows)
__device__ inline Tile tile_of(int tiles_x, int tiles_y, int rows) {
  const int64_t t = blockIdx.x;
  const int64_t ry = t / tiles_x;
  Tile o;
  o.x0 = (int)(t - ry * tiles_x) * TW;
  o.img = ry / tiles_y;
  o.y = (int)(ry - o.img * tiles_y) * rows + (int)(threadIdx.x >> 6);
  return o;
}

__device__ inline const uint8_t* bytes(const uint16_t* p) { return reinterpret_cast<const uint8_t*>(p); }
__device__ inline uint8_t* bytes(uint16_t* p) { return reinterpret_cast<uint8_t*>(p); }
// the sample position within its dword: 0 or 1
__device__ inline int addr_half(const void* p) { return addr_mod4(p) >> 1; }

// ------------------------------------------------------------------------------------------------ RGB
template <int PATH>
__global__ __launch_bounds__(256) void ingest_u16_kernel(const uint16_t* __restrict__ src, IoStride4 s, Fmt16 f, int H,
                                                         int W, float* __restrict__ dst, int Hp, int Wp, int tiles_x,
                                                         int tiles_y) {
  __shared__ uint32_t S[ROWS][RGB_LDS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const Tile t = tile_of(tiles_x, tiles_y, ROWS);
  // pixels of this wave's row segment that lie inside the image (the rest is padding)
  const int nx = t.y < H ? min(TW, max(W - t.x0, 0)) : 0;
  const uint16_t* row = src + t.img * s.img + (int64_t)t.y * s.row + (int64_t)t.x0 * s.col;  // used when nx > 0
  int sh[3] = {0, 0, 0};  // in samples
  if (PATH == IO_HWC && nx > 0) {
    sh[0] = addr_half(row);
    stage_in(bytes(row), 6 * nx, S[wave], lane);
  }
  if (PATH == IO_CHW && nx > 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      sh[c] = addr_half(row + c * s.ch);
      stage_in(bytes(row + c * s.ch), 2 * nx, S[wave] + c * SEG, lane);
    }
  }
  if (PATH != IO_GENERAL) __syncthreads();
  const uint16_t* S16 = reinterpret_cast<const uint16_t*>(S[wave]);
  const float fmax = (float)f.maxv;
  const int64_t plane = (int64_t)Hp * Wp;
  float* out = dst + t.img * 3 * plane + (int64_t)t.y * Wp + t.x0;
#pragma unroll
  for (int j = 0; j < TW / 64; ++j) {
    const int px = lane + 64 * j;
    if (t.x0 + px >= Wp) break;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float v = 0.0f;
      if (px < nx) {
        uint16_t u;
        if (PATH == IO_HWC) u = S16[sh[0] + 3 * px + c];
        else if (PATH == IO_CHW) u = S16[c * SEG * 2 + sh[c] + px];
        else u = row[(int64_t)px * s.col + c * s.ch];
        v = (float)sample_of(u, f) / fmax;  // correctly rounded (hipcc's default for fp32 division)
      }
      out[c * plane + px] = v;
    }
  }
}

template <int PATH, bool REF>
__global__ __launch_bounds__(256) void egress_u16_kernel(const float* __restrict__ src, IoStride3 ss, int H, int W,
                                                         Fmt16 f, uint16_t* __restrict__ dst, IoStride4 ds,
                                                         const uint16_t* __restrict__ ref, IoStride4 rs,
                                                         unsigned long long* __restrict__ sq_err, int tiles_x,
                                                         int tiles_y) {
  __shared__ uint32_t S[ROWS][RGB_LDS];
  __shared__ unsigned long long red[ROWS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int G = REF ? RGB_REF_GROUPS : 1;  // row groups this block walks
  const Tile t = tile_of(tiles_x, tiles_y, G * ROWS);
  uint16_t* S16 = reinterpret_cast<uint16_t*>(S[wave]);
  const float fmax = (float)f.maxv;
  unsigned long long acc = 0;  // 64 bits from the lane upwards: one squared difference can be 65535^2
  for (int g = 0; g < G; ++g) {
    const int y = t.y + g * ROWS;
    const int nx = y < H ? min(TW, W - t.x0) : 0;  // x0 < W: the tiles cover the crop only
    const float* in = src + t.img * ss.img + (int64_t)y * ss.row + t.x0;
    uint16_t* row = dst + t.img * ds.img + (int64_t)y * ds.row + (int64_t)t.x0 * ds.col;
    const uint16_t* rrow = REF ? ref + t.img * rs.img + (int64_t)y * rs.row + (int64_t)t.x0 * rs.col : nullptr;
    int sh[3] = {0, 0, 0};
    if (PATH == IO_HWC) sh[0] = addr_half(row);
    if (PATH == IO_CHW) {
#pragma unroll
      for (int c = 0; c < 3; ++c) sh[c] = addr_half(row + c * ds.ch);
    }
#pragma unroll
    for (int j = 0; j < TW / 64; ++j) {
      const int px = lane + 64 * j;
      if (px >= nx) break;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v = in[c * ss.ch + px];
        const int u = (int)floorf(fminf(fmaxf(v, 0.0f), 1.0f) * fmax);
        const uint16_t w = word_of(u, f);
        if (PATH == IO_HWC) S16[sh[0] + 3 * px + c] = w;
        else if (PATH == IO_CHW) S16[c * SEG * 2 + sh[c] + px] = w;
        else row[(int64_t)px * ds.col + c * ds.ch] = w;
        if (REF) {
          const int d = u - sample_of(rrow[(int64_t)px * rs.col + c * rs.ch], f);
          const unsigned int a = (unsigned int)(d < 0 ? -d : d);
          acc += (unsigned long long)a * a;
        }
      }
    }
    if (PATH != IO_GENERAL) {
      __syncthreads();
      if (PATH == IO_HWC && nx > 0) stage_out(bytes(row), 6 * nx, S[wave], lane);
      if (PATH == IO_CHW && nx > 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) stage_out(bytes(row + c * ds.ch), 2 * nx, S[wave] + c * SEG, lane);
      }
      if (G > 1) __syncthreads();  // the next group's samples go into the same LDS
    }
  }
  if (REF) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned long long s = red[0] + red[1] + red[2] + red[3];  // < 2^48: no carry out of 64 bits
      if (s) atomicAdd(sq_err + t.img, s);
    }
  }
}

// ---------------------------------------------------------------------------------------------- Y'CbCr
struct PlaneStride {
  int64_t img, row, col;
};
struct Planes3 {
  uint16_t* p[3];  // Y, Cb, Cr
  PlaneStride s[3];
};
struct YuvGeom {
  int sub_x, sub_y, left;  // left: sub_x == 2 and chroma co-sited with the even luma column
  int uv_b, uv_r;          // NV form: Cb's and Cr's sample within the interleaved pair (the pair starts at p[1] - uv_b)
};
struct YuvIn {
  float yo, cy, crv, cgu, cgv, cbu, half;
};
struct YuvOut {
  float yo, yr, yg, yb, br, bg, bb, rr, rg, rb, half, maxv;
};

// image_yuv.hip's stage_load / stage_store for samples: the segment p[0, n) sits in LDS at samples [h, h + n),
// h = (p mod 4) / 2.  load: lane's whole dwords lane + 64 j that lie inside the segment, and one edge sample: lane 0
// takes the sample before the first whole dword (h == 1), lane 1 the one after the last (h + n odd).  Nothing
// outside the segment is read.  store: the same dwords and samples into LDS.
struct StageEdge {
  int pos;  // LDS sample position of this lane's edge sample, -1 = none
  uint32_t word;
};
template <int N>
__device__ inline void stage_load(const uint16_t* __restrict__ p, int n, int lane, uint32_t (&v)[N], StageEdge* e) {
  const int h = addr_half(p), end = h + n;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const int lo = 2 * (lane + 64 * j);
    v[j] = 0;
    if (lo >= h && lo + 2 <= end) v[j] = *reinterpret_cast<const uint32_t*>(p + (lo - h));
  }
  e->pos = -1;
  if (lane == 0 && h == 1 && n >= 1) e->pos = 1;
  if (lane == 1 && (end & 1) && n >= 1) e->pos = end - 1;  // even, so not the head sample
  e->word = 0;
  if (e->pos >= 0) e->word = p[e->pos - h];
}
template <int N>
__device__ inline void stage_store(uint32_t* r, int n, int h, int lane, const uint32_t (&v)[N], const StageEdge& e) {
  const int end = h + n;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const int lo = 2 * (lane + 64 * j);
    if (lo >= h && lo + 2 <= end) r[lane + 64 * j] = v[j];
  }
  if (e.pos >= 0) reinterpret_cast<uint16_t*>(r)[e.pos] = (uint16_t)e.word;
}

template <int FORM>
__global__ __launch_bounds__(256) void ingest_yuv16_kernel(Planes3 P, YuvGeom q, YuvIn k, Fmt16 f, int H, int W,
                                                           float* __restrict__ dst, int Hp, int Wp, int tiles_x,
                                                           int tiles_y, int vec) {
  __shared__ uint32_t S[ROWS][YUV_IN_LDS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const Tile t = tile_of(tiles_x, tiles_y, ROWS);
  const int y = t.y, x0 = t.x0;
  const int nx = y < H ? min(TW, max(W - x0, 0)) : 0;  // pixels of this row piece inside the image
  const int CW = (W + q.sub_x - 1) / q.sub_x, CH = (H + q.sub_y - 1) / q.sub_y;
  // the two chroma rows of this luma row and their weights (quarters)
  int r0 = y, r1 = y, wv0 = 4, wv1 = 0;
  if (q.sub_y == 2) {
    r0 = y >> 1;
    r1 = min(max(r0 + ((y & 1) ? 1 : -1), 0), CH - 1);
    wv0 = 3, wv1 = 1;
  }
  // chroma columns [lo, hi) that this row piece touches (used when nx > 0)
  const int c0 = x0 / q.sub_x;
  const int lo = q.sub_x == 2 ? max(c0 - 1, 0) : c0;
  const int hi = q.sub_x == 2 ? min(c0 + (nx + 1) / 2 + 1, CW) : c0 + nx;
  const uint16_t* yrow = P.p[0] + t.img * P.s[0].img + (int64_t)y * P.s[0].row + (int64_t)x0 * P.s[0].col;
  const uint16_t* crow[2][2];  // [plane][row]: the row's first sample
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    crow[p][0] = P.p[1 + p] + t.img * P.s[1 + p].img + (int64_t)r0 * P.s[1 + p].row;
    crow[p][1] = P.p[1 + p] + t.img * P.s[1 + p].img + (int64_t)r1 * P.s[1 + p].row;
  }
  const uint16_t* S16 = reinterpret_cast<const uint16_t*>(S[wave]);
  int shy = 0, shc[2][2] = {{0, 0}, {0, 0}};  // LDS sample offsets of sample `lo` (planar) / of pair `lo` (NV)
  if (FORM != YUV_GENERAL && nx > 0) {
    // every row's loads are issued before the first LDS store: one memory round trip a wave, not one per row
    const bool two = wv1 != 0;  // the second chroma row has a weight
    uint32_t vy[3];
    StageEdge ey;
    shy = addr_half(yrow);
    stage_load<3>(yrow, nx, lane, vy, &ey);
    if (FORM == YUV_PLANAR) {
      uint32_t vc[2][2][3];
      StageEdge ec[2][2];
      const uint16_t* g[2][2];
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          g[p][r] = crow[p][r] + lo;
          shc[p][r] = (SEG + (2 * p + r) * CSEG) * 2 + addr_half(g[p][r]);
          if (r == 0 || two) stage_load<3>(g[p][r], hi - lo, lane, vc[p][r], &ec[p][r]);
        }
      stage_store<3>(S[wave], nx, shy, lane, vy, ey);
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int r = 0; r < 2; ++r)
          if (r == 0 || two)
            stage_store<3>(S[wave] + SEG + (2 * p + r) * CSEG, hi - lo, addr_half(g[p][r]), lane, vc[p][r], ec[p][r]);
    } else {
      uint32_t vc[2][5];  // up to 2 * 256 samples and one more at either alignment: 257 dwords
      StageEdge ec[2];
      const uint16_t* g[2];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        g[r] = crow[0][r] - q.uv_b + 2 * (int64_t)lo;  // the pair of chroma sample lo
        const int at = (SEG + 2 * r * CSEG) * 2 + addr_half(g[r]);
        shc[0][r] = at + q.uv_b;
        shc[1][r] = at + q.uv_r;
        if (r == 0 || two) stage_load<5>(g[r], 2 * (hi - lo), lane, vc[r], &ec[r]);
      }
      stage_store<3>(S[wave], nx, shy, lane, vy, ey);
#pragma unroll
      for (int r = 0; r < 2; ++r)
        if (r == 0 || two)
          stage_store<5>(S[wave] + SEG + 2 * r * CSEG, 2 * (hi - lo), addr_half(g[r]), lane, vc[r], ec[r]);
    }
  }
  if (FORM != YUV_GENERAL) __syncthreads();
  // chroma sample i of plane p, row r
  auto C = [&](int p, int r, int i) -> int {
    if (FORM == YUV_PLANAR) return sample_of(S16[shc[p][r] + (i - lo)], f);
    if (FORM == YUV_NV) return sample_of(S16[shc[p][r] + 2 * (i - lo)], f);
    return sample_of(crow[p][r][(int64_t)i * P.s[1 + p].col], f);
  };
  // A lane owns four consecutive pixels: their chroma taps are four samples per chroma row and plane (the two
  // the pixels lie in and one neighbour on either side), and the fp32 side is one 16-byte store per channel.
  const int px = 4 * lane;
  if (x0 + px >= Wp) return;  // Wp is a multiple of 64: a lane's four pixels are all inside the row or all outside
  float o[3][4];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int e = 0; e < 4; ++e) o[c][e] = 0.0f;
  if (px < nx) {
    // h[p][r][e]: the horizontal taps of pixel e in chroma row r of plane p, in quarters.  Indices are clamped to
    // the samples this piece touches ([lo, hi - 1], inside the plane); a clamp that bites below the plane's own
    // edge belongs to a pixel outside the image, whose value is not kept
    int h[2][2][4];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        if (r == 1 && wv1 == 0) {
#pragma unroll
          for (int e = 0; e < 4; ++e) h[p][r][e] = 0;
          continue;
        }
        if (q.sub_x == 2) {
          const int ia = c0 + 2 * lane;
          const int cm = C(p, r, max(ia - 1, lo)), ca = C(p, r, min(ia, hi - 1)), cb = C(p, r, min(ia + 1, hi - 1)),
                    cn = C(p, r, min(ia + 2, hi - 1));
          if (q.left) {
            h[p][r][0] = 4 * ca, h[p][r][1] = 2 * ca + 2 * cb, h[p][r][2] = 4 * cb, h[p][r][3] = 2 * cb + 2 * cn;
          } else {
            h[p][r][0] = 3 * ca + cm, h[p][r][1] = 3 * ca + cb, h[p][r][2] = 3 * cb + ca, h[p][r][3] = 3 * cb + cn;
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) h[p][r][e] = 4 * C(p, r, min(x0 + px + e, hi - 1));
        }
      }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (px + e >= nx) break;
      const int Y = sample_of(FORM == YUV_GENERAL ? yrow[(int64_t)(px + e) * P.s[0].col] : S16[shy + px + e], f);
      // sixteenths, [0, 16 maxv] < 2^20: exact in fp32
      const int c16b = wv0 * h[0][0][e] + wv1 * h[0][1][e], c16r = wv0 * h[1][0][e] + wv1 * h[1][1][e];
      const float u = (float)c16b * 0.0625f - k.half, v = (float)c16r * 0.0625f - k.half;  // exact
      const float a = __fmul_rn(k.cy, (float)Y - k.yo);
      const float R = __fadd_rn(a, __fmul_rn(k.crv, v));
      const float G = __fsub_rn(__fsub_rn(a, __fmul_rn(k.cgu, u)), __fmul_rn(k.cgv, v));
      const float Bl = __fadd_rn(a, __fmul_rn(k.cbu, u));
      o[0][e] = fminf(fmaxf(R, 0.0f), 1.0f);
      o[1][e] = fminf(fmaxf(G, 0.0f), 1.0f);
      o[2][e] = fminf(fmaxf(Bl, 0.0f), 1.0f);
    }
  }
  const int64_t plane = (int64_t)Hp * Wp;
  float* out = dst + t.img * 3 * plane + (int64_t)y * Wp + x0 + px;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (vec) {  // dst is 16-byte aligned, and so is every group of four pixels (Wp and x0 + px are multiples of 4)
      *reinterpret_cast<float4*>(out + c * plane) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) out[c * plane + e] = o[c][e];
    }
  }
}

struct Chroma2 {
  float b, r;
};

__device__ inline void yuv_of_rgb(const YuvOut& k, float r, float g, float b, float* ty, Chroma2* c) {
  r = fminf(fmaxf(r, 0.0f), 1.0f);  // fmaxf drops a NaN: NaN -> 0
  g = fminf(fmaxf(g, 0.0f), 1.0f);
  b = fminf(fmaxf(b, 0.0f), 1.0f);
  *ty = __fadd_rn(__fadd_rn(k.yo, __fadd_rn(__fmul_rn(k.yr, r), __fmul_rn(k.yg, g))), __fmul_rn(k.yb, b));
  c->b = __fadd_rn(__fadd_rn(__fmul_rn(k.br, r), __fmul_rn(k.bg, g)), __fmul_rn(k.bb, b));
  c->r = __fadd_rn(__fadd_rn(__fmul_rn(k.rr, r), __fmul_rn(k.rg, g)), __fmul_rn(k.rb, b));
}

__device__ inline int yuv_sample(float t, float maxv) {
  return (int)floorf(fminf(fmaxf(__fadd_rn(t, 0.5f), 0.0f), maxv));
}

__device__ inline unsigned long long sq_diff(int a, int b) {
  const int d = a - b;
  const unsigned int m = (unsigned int)(d < 0 ? -d : d);
  return (unsigned long long)m * m;
}

template <int FORM, bool REF>
__global__ __launch_bounds__(256) void egress_yuv16_kernel(const float* __restrict__ src, IoStride3 ss, int H, int W,
                                                           YuvGeom q, YuvOut k, Fmt16 f, Planes3 D, Planes3 Rf,
                                                           unsigned long long* __restrict__ sq_err, int tiles_x,
                                                           int tiles_y) {
  __shared__ uint32_t S[ROWS][YUV_OUT_LDS];
  __shared__ unsigned long long red[ROWS][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int G = REF ? YUV_REF_GROUPS : 1;  // chroma row groups this block walks
  const Tile t = tile_of(tiles_x, tiles_y, G * ROWS);
  const int x0 = t.x0;
  const int CW = (W + q.sub_x - 1) / q.sub_x, CH = (H + q.sub_y - 1) / q.sub_y;
  uint16_t* S16 = reinterpret_cast<uint16_t*>(S[wave]);
  const int lx = x0 + 4 * lane;  // this lane's first luma column
  int xc[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) xc[e] = min(lx + e, W - 1);
  const int nc = q.sub_x == 2 ? 2 : 4;         // chroma samples per lane
  const int c0 = x0 / q.sub_x;                 // the piece's first chroma column
  const int cl = lx / q.sub_x;                 // this lane's first chroma column
  const int taps = (q.left ? 4 : q.sub_x) * q.sub_y;  // the filter's weights sum to this: 1, 2, 4 or 8
  const float scale = taps == 8 ? 0.125f : taps == 4 ? 0.25f : taps == 2 ? 0.5f : 1.0f;
  unsigned long long acc[3] = {0, 0, 0};       // 64 bits from the lane upwards
  for (int g = 0; g < G; ++g) {
    const int cy = t.y + g * ROWS;             // this wave's chroma row
    const int nx = cy < CH ? min(TW, W - x0) : 0;  // x0 < W: the tiles cover the crop only
    const int ncx = (nx + q.sub_x - 1) / q.sub_x;
    uint16_t* yrow[2] = {nullptr, nullptr};
    uint16_t* crow[2] = {nullptr, nullptr};
    int shy[2] = {0, 0}, shc[2] = {0, 0};
    if (nx > 0) {
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int yy = min(cy * q.sub_y + r, H - 1);
        yrow[r] = D.p[0] + t.img * D.s[0].img + (int64_t)yy * D.s[0].row + (int64_t)x0 * D.s[0].col;
        if (FORM != YUV_GENERAL) shy[r] = r * SEG * 2 + addr_half(yrow[r]);
      }
#pragma unroll
      for (int p = 0; p < 2; ++p)
        crow[p] = D.p[1 + p] + t.img * D.s[1 + p].img + (int64_t)cy * D.s[1 + p].row + (int64_t)c0 * D.s[1 + p].col;
      if (FORM == YUV_PLANAR) {
        shc[0] = 2 * SEG * 2 + addr_half(crow[0]);
        shc[1] = 3 * SEG * 2 + addr_half(crow[1]);
      }
      if (FORM == YUV_NV) {
        const int at = 2 * SEG * 2 + addr_half(crow[0] - q.uv_b);
        shc[0] = at + q.uv_b;
        shc[1] = at + q.uv_r;
      }
      // full-resolution chroma of this lane's four columns and of the column to their left, per luma row
      Chroma2 cf[2][5];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        if (r >= q.sub_y) break;
        const int yr = cy * q.sub_y + r;  // the block's row; past H it repeats row H - 1 and gives no Y samples
        const int yy = min(yr, H - 1);
        const float* in = src + t.img * ss.img + (int64_t)yy * ss.row;
        float ty[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
          yuv_of_rgb(k, in[xc[e]], in[ss.ch + xc[e]], in[2 * ss.ch + xc[e]], &ty[e], &cf[r][e + 1]);
        if (q.left) {
          // every lane takes the shuffles; lane - 1's last column is lx - 1 whenever this lane's columns are inside
          Chroma2 lf;
          lf.b = __shfl_up(cf[r][4].b, 1, 64);
          lf.r = __shfl_up(cf[r][4].r, 1, 64);
          if (lane == 0) {
            const int xl = max(x0 - 1, 0);
            float unused;
            yuv_of_rgb(k, in[xl], in[ss.ch + xl], in[2 * ss.ch + xl], &unused, &lf);
          }
          cf[r][0] = lf;
        }
        if (yr < H) {
          uint32_t rv[4] = {0, 0, 0, 0};  // the reference's four words: one 8-byte load where they are contiguous
          if (REF && lx < W) {
            const uint16_t* rp = Rf.p[0] + t.img * Rf.s[0].img + (int64_t)yr * Rf.s[0].row + (int64_t)lx * Rf.s[0].col;
            if (Rf.s[0].col == 1 && lx + 3 < W) {
              unsigned long long w8;
              __builtin_memcpy(&w8, rp, 8);
#pragma unroll
              for (int e = 0; e < 4; ++e) rv[e] = (uint32_t)((w8 >> (16 * e)) & 0xffffu);
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (lx + e < W) rv[e] = rp[(int64_t)e * Rf.s[0].col];
            }
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (lx + e >= W) break;
            const int u = yuv_sample(ty[e], k.maxv);
            if (FORM == YUV_GENERAL) yrow[r][(int64_t)(4 * lane + e) * D.s[0].col] = word_of(u, f);
            else S16[shy[r] + 4 * lane + e] = word_of(u, f);
            if (REF) acc[0] += sq_diff(u, sample_of(rv[e], f));
          }
        }
      }
      // the filtered chroma samples of this lane
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        if (m >= nc || cl + m >= CW) break;
        float sb = 0.0f, sr = 0.0f;
        if (q.sub_x == 1) {
          sb = cf[0][m + 1].b, sr = cf[0][m + 1].r;
        } else {
          bool first = true;
#pragma unroll
          for (int r = 0; r < 2; ++r) {
            if (r >= q.sub_y) break;
#pragma unroll
            for (int e = 0; e < 3; ++e) {  // columns 2 m - 1 (left siting only), 2 m, 2 m + 1
              if (e == 0 && !q.left) continue;
              if (m >= 2) continue;  // (keeps the index a constant of the unrolled loop)
              const Chroma2 c = cf[r][2 * (m & 1) + e];
              const float w = (q.left && e == 1) ? 2.0f : 1.0f;
              const float vb = __fmul_rn(w, c.b), vr = __fmul_rn(w, c.r);
              sb = first ? vb : __fadd_rn(sb, vb);
              sr = first ? vr : __fadd_rn(sr, vr);
              first = false;
            }
          }
        }
        const int ub = yuv_sample(__fadd_rn(__fmul_rn(sb, scale), k.half), k.maxv);
        const int ur = yuv_sample(__fadd_rn(__fmul_rn(sr, scale), k.half), k.maxv);
        const int ci = cl + m - c0;  // within the piece
        if (FORM == YUV_GENERAL) {
          crow[0][(int64_t)ci * D.s[1].col] = word_of(ub, f);
          crow[1][(int64_t)ci * D.s[2].col] = word_of(ur, f);
        } else {
          const int st = FORM == YUV_NV ? 2 : 1;
          S16[shc[0] + st * ci] = word_of(ub, f);
          S16[shc[1] + st * ci] = word_of(ur, f);
        }
        if (REF) {
          const uint16_t wb = Rf.p[1][t.img * Rf.s[1].img + (int64_t)cy * Rf.s[1].row + (int64_t)(cl + m) * Rf.s[1].col];
          const uint16_t wr = Rf.p[2][t.img * Rf.s[2].img + (int64_t)cy * Rf.s[2].row + (int64_t)(cl + m) * Rf.s[2].col];
          acc[1] += sq_diff(ub, sample_of(wb, f));
          acc[2] += sq_diff(ur, sample_of(wr, f));
        }
      }
    }
    if (FORM != YUV_GENERAL) {
      __syncthreads();
      if (nx > 0) {
#pragma unroll
        for (int r = 0; r < 2; ++r)
          if (r < q.sub_y && cy * q.sub_y + r < H) stage_out(bytes(yrow[r]), 2 * nx, S[wave] + r * SEG, lane);
        if (FORM == YUV_PLANAR) {
          stage_out(bytes(crow[0]), 2 * ncx, S[wave] + 2 * SEG, lane);
          stage_out(bytes(crow[1]), 2 * ncx, S[wave] + 3 * SEG, lane);
        } else {
          stage_out(bytes(crow[0] - q.uv_b), 4 * ncx, S[wave] + 2 * SEG, lane);
        }
      }
      if (G > 1) __syncthreads();  // the next group's samples go into the same LDS
    }
  }
  if (REF) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) acc[c] += __shfl_down(acc[c], off, 64);
      if (lane == 0) red[wave][c] = acc[c];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
      const int c = threadIdx.x;
      const unsigned long long s = red[0][c] + red[1][c] + red[2][c] + red[3][c];
      if (s) atomicAdd(sq_err + t.img * 3 + c, s);
    }
  }
}

// ------------------------------------------------------------------------------------------------ host
Fmt16 fmt16(int depth, int msb, const char* who) {
  const std::string w = std::string("mlic: ") + who + ": ";
  if (depth < 8 || depth > 16) throw Error(w + "depth must be in [8, 16]");
  if (msb != 0 && msb != 1) throw Error(w + "msb must be 0 (LSB-aligned samples) or 1 (MSB-aligned, P010 style)");
  return Fmt16{(1 << depth) - 1, 16 - depth, msb};
}

void aligned2(const void* p, const char* who, const char* what) {
  if (reinterpret_cast<uintptr_t>(p) % 2 != 0)
    throw Error(std::string("mlic: ") + who + ": " + what + " must be 2-byte aligned (uint16 samples)");
}

// the kernel form for a uint16 image with these strides; throws when a forced form does not fit
int io_path(const int64_t* s) {
  const bool hwc = s[2] == 3 && s[3] == 1, chw = s[2] == 1;
  const int forced = opt(OPT_IMAGE_IO_PATH);
  if (forced < 0) return hwc ? IO_HWC : chw ? IO_CHW : IO_GENERAL;
  MLIC_CHECK(forced != IO_HWC || hwc, "image_io_path 1 (HWC) needs column stride 3 and channel stride 1");
  MLIC_CHECK(forced != IO_CHW || chw, "image_io_path 2 (CHW) needs column stride 1");
  return forced;
}

unsigned blocks_of(int B, int rows, int cols, int block_rows, int* tiles_x, int* tiles_y) {
  *tiles_x = (cols + TW - 1) / TW;
  *tiles_y = (rows + block_rows - 1) / block_rows;
  const int64_t blocks = (int64_t)B * *tiles_x * *tiles_y;
  MLIC_CHECK(blocks <= 0x7fffffffLL, "image_io16: batch too large for one launch");
  return (unsigned)blocks;
}

template <int PATH>
void egress_launch(unsigned blocks, hipStream_t st, const float* src, IoStride3 ss, int H, int W, Fmt16 f, uint16_t* dst,
                   IoStride4 ds, const uint16_t* ref, IoStride4 rs, uint64_t* sq, int tx, int ty) {
  auto* sq64 = reinterpret_cast<unsigned long long*>(sq);
  if (ref)
    hipLaunchKernelGGL((egress_u16_kernel<PATH, true>), dim3(blocks), dim3(256), 0, st, src, ss, H, W, f, dst, ds, ref,
                       rs, sq64, tx, ty);
  else
    hipLaunchKernelGGL((egress_u16_kernel<PATH, false>), dim3(blocks), dim3(256), 0, st, src, ss, H, W, f, dst, ds, ref,
                       rs, sq64, tx, ty);
}

struct YuvSetup {
  YuvGeom q;
  YuvIn in;
  YuvOut out;
};

// the description's checks (each refusal its own message) and the constants of depth d, folded in double and
// rounded once: image_yuv.hip's yuv_setup with ys, cs, yo scaled by 2^(d-8) (limited range) or maxv (full range)
YuvSetup yuv_setup(const YuvDesc* d, int depth, const char* who) {
  const std::string w = std::string(who) + ": ";
  if (d == nullptr) throw Error("mlic: " + w + "null desc");
  if (!((d->sub_x == 1 || d->sub_x == 2) && (d->sub_y == 1 || d->sub_y == 2)))
    throw Error("mlic: " + w + "sub_x and sub_y must be 1 or 2");
  if (d->sub_x == 1 && d->sub_y == 2) throw Error("mlic: " + w + "sub_x 1 with sub_y 2 (4:4:0) is not supported");
  if (d->matrix < 0 || d->matrix > 2)
    throw Error("mlic: " + w + "matrix must be 0 (BT.601), 1 (BT.709) or 2 (BT.2020 non-constant-luminance)");
  if (d->full_range != 0 && d->full_range != 1) throw Error("mlic: " + w + "full_range must be 0 or 1");
  if (d->site_x != 0 && d->site_x != 1) throw Error("mlic: " + w + "site_x must be 0 (centre) or 1 (left)");
  if (d->reserved[0] != 0 || d->reserved[1] != 0 || d->reserved[2] != 0)
    throw Error("mlic: " + w + "reserved fields must be 0");
  const double Kr = d->matrix == 2 ? 0.2627 : d->matrix ? 0.2126 : 0.299;
  const double Kb = d->matrix == 2 ? 0.0593 : d->matrix ? 0.0722 : 0.114, Kg = 1.0 - Kr - Kb;
  const double maxv = (double)((1 << depth) - 1), sc = (double)(1 << (depth - 8)), half = (double)(1 << (depth - 1));
  const double ys = d->full_range ? maxv : 219.0 * sc, cs = d->full_range ? maxv : 224.0 * sc,
               yo = d->full_range ? 0.0 : 16.0 * sc;
  YuvSetup s;
  s.q = YuvGeom{d->sub_x, d->sub_y, (d->sub_x == 2 && d->site_x == 1) ? 1 : 0, 0, 1};
  s.in = YuvIn{(float)yo,
               (float)(1.0 / ys),
               (float)(2.0 * (1.0 - Kr) / cs),
               (float)(2.0 * Kb * (1.0 - Kb) / (Kg * cs)),
               (float)(2.0 * Kr * (1.0 - Kr) / (Kg * cs)),
               (float)(2.0 * (1.0 - Kb) / cs),
               (float)half};
  s.out = YuvOut{(float)yo,
                 (float)(ys * Kr),
                 (float)(ys * Kg),
                 (float)(ys * Kb),
                 (float)(-(cs * Kr) / (2.0 * (1.0 - Kb))),
                 (float)(-(cs * Kg) / (2.0 * (1.0 - Kb))),
                 (float)(cs / 2.0),
                 (float)(cs / 2.0),
                 (float)(-(cs * Kg) / (2.0 * (1.0 - Kr))),
                 (float)(-(cs * Kb) / (2.0 * (1.0 - Kr))),
                 (float)half,
                 (float)maxv};
  return s;
}

// the kernel form for these planes, as image_yuv.hip's yuv_form picks one; fills the NV sample positions
int yuv_form(const uint16_t* const* p, const int64_t* const* s, YuvGeom* q) {
  const bool y1 = s[0][2] == 1;
  const bool planar = y1 && s[1][2] == 1 && s[2][2] == 1;
  const bool pair = (p[2] == p[1] + 1 || p[1] == p[2] + 1);
  const bool nv = y1 && s[1][2] == 2 && s[2][2] == 2 && pair && s[1][0] == s[2][0] && s[1][1] == s[2][1];
  if (p[1] == p[2] + 1) q->uv_b = 1, q->uv_r = 0;
  const int forced = opt(OPT_IMAGE_IO_PATH);
  if (forced < 0) return planar ? YUV_PLANAR : nv ? YUV_NV : YUV_GENERAL;
  MLIC_CHECK(forced != 1, "image_io_path 1 (HWC) does not exist for Y'CbCr planes: 0 (general) or 2 (LDS) expected");
  if (forced == 0) return YUV_GENERAL;
  MLIC_CHECK(planar || nv, "image_io_path 2 needs unit column strides, or interleaved chroma with column stride 2");
  return planar ? YUV_PLANAR : YUV_NV;
}

Planes3 planes3(const uint16_t* const* p, const int64_t* const* s) {
  Planes3 P;
  for (int c = 0; c < 3; ++c) {
    P.p[c] = const_cast<uint16_t*>(p[c]);
    P.s[c] = PlaneStride{s[c][0], s[c][1], s[c][2]};
  }
  return P;
}

template <int FORM>
void egress_yuv_launch(unsigned blocks, hipStream_t st, const float* src, IoStride3 ss, int H, int W, YuvGeom q,
                       YuvOut k, Fmt16 f, Planes3 D, Planes3 Rf, bool ref, uint64_t* sq, int tx, int ty) {
  auto* sq64 = reinterpret_cast<unsigned long long*>(sq);
  if (ref)
    hipLaunchKernelGGL((egress_yuv16_kernel<FORM, true>), dim3(blocks), dim3(256), 0, st, src, ss, H, W, q, k, f, D, Rf,
                       sq64, tx, ty);
  else
    hipLaunchKernelGGL((egress_yuv16_kernel<FORM, false>), dim3(blocks), dim3(256), 0, st, src, ss, H, W, q, k, f, D, Rf,
                       sq64, tx, ty);
}

}  // namespace

void image_yuv16_check(const YuvDesc* desc, int depth, int msb, const void* y, const void* cb, const void* cr,
                       const char* who) {
  (void)fmt16(depth, msb, who);
  (void)yuv_setup(desc, depth, who);
  aligned2(y, who, "y");
  aligned2(cb, who, "cb");
  aligned2(cr, who, "cr");
}

void image_ingest_u16(const uint16_t* src, const int64_t* s, int depth, int msb, int B, int H, int W, float* dst, int Hp,
                      int Wp, hipStream_t st) {
  MLIC_CHECK(src != nullptr && s != nullptr && dst != nullptr, "image_ingest_u16: null argument");
  MLIC_CHECK(B >= 1 && H >= 1 && W >= 1, "image_ingest_u16: B, H and W must be positive");
  MLIC_CHECK(Hp >= H && Wp >= W && Hp % 64 == 0 && Wp % 64 == 0,
             "image_ingest_u16: Hp, Wp must be multiples of 64 that cover H, W");
  const Fmt16 f = fmt16(depth, msb, "image_ingest_u16");
  MLIC_CHECK(s[2] != 0 && s[3] != 0, "image_ingest_u16: zero column or channel stride");
  aligned2(src, "image_ingest_u16", "src");
  MLIC_CHECK(reinterpret_cast<uintptr_t>(dst) % 4 == 0, "image_ingest_u16: dst must be 4-byte aligned");
  const int path = io_path(s);
  int tx, ty;
  const unsigned blocks = blocks_of(B, Hp, Wp, ROWS, &tx, &ty);
  const IoStride4 ss{s[0], s[1], s[2], s[3]};
  if (path == IO_HWC)
    hipLaunchKernelGGL(ingest_u16_kernel<IO_HWC>, dim3(blocks), dim3(256), 0, st, src, ss, f, H, W, dst, Hp, Wp, tx, ty);
  else if (path == IO_CHW)
    hipLaunchKernelGGL(ingest_u16_kernel<IO_CHW>, dim3(blocks), dim3(256), 0, st, src, ss, f, H, W, dst, Hp, Wp, tx, ty);
  else
    hipLaunchKernelGGL(ingest_u16_kernel<IO_GENERAL>, dim3(blocks), dim3(256), 0, st, src, ss, f, H, W, dst, Hp, Wp, tx,
                       ty);
  HIP_OK(hipGetLastError());
}

void image_egress_u16(const float* src, const int64_t* s, int B, int H, int W, int depth, int msb, uint16_t* dst,
                      const int64_t* d, const uint16_t* ref, const int64_t* r, uint64_t* sq_err, hipStream_t st) {
  MLIC_CHECK(src != nullptr && s != nullptr && dst != nullptr && d != nullptr, "image_egress_u16: null argument");
  MLIC_CHECK(B >= 1 && H >= 1 && W >= 1, "image_egress_u16: B, H and W must be positive");
  const Fmt16 f = fmt16(depth, msb, "image_egress_u16");
  MLIC_CHECK(d[2] != 0 && d[3] != 0, "image_egress_u16: zero column or channel stride (dst)");
  MLIC_CHECK((ref != nullptr) == (sq_err != nullptr), "image_egress_u16: ref and sq_err go together");
  MLIC_CHECK(ref == nullptr || (r != nullptr && r[2] != 0 && r[3] != 0),
             "image_egress_u16: ref needs strides with nonzero column and channel stride");
  aligned2(dst, "image_egress_u16", "dst");
  aligned2(ref, "image_egress_u16", "ref");
  MLIC_CHECK(reinterpret_cast<uintptr_t>(src) % 4 == 0 && reinterpret_cast<uintptr_t>(sq_err) % 8 == 0,
             "image_egress_u16: src must be 4-byte and sq_err 8-byte aligned");
  const int path = io_path(d);
  int tx, ty;
  const unsigned blocks = blocks_of(B, H, W, (ref ? RGB_REF_GROUPS : 1) * ROWS, &tx, &ty);
  const IoStride3 ss{s[0], s[1], s[2]};
  const IoStride4 ds{d[0], d[1], d[2], d[3]};
  const IoStride4 rs = ref ? IoStride4{r[0], r[1], r[2], r[3]} : IoStride4{0, 0, 0, 0};
  if (sq_err) HIP_OK(hipMemsetAsync(sq_err, 0, sizeof(uint64_t) * (size_t)B, st));
  if (path == IO_HWC) egress_launch<IO_HWC>(blocks, st, src, ss, H, W, f, dst, ds, ref, rs, sq_err, tx, ty);
  else if (path == IO_CHW) egress_launch<IO_CHW>(blocks, st, src, ss, H, W, f, dst, ds, ref, rs, sq_err, tx, ty);
  else egress_launch<IO_GENERAL>(blocks, st, src, ss, H, W, f, dst, ds, ref, rs, sq_err, tx, ty);
  HIP_OK(hipGetLastError());
}

void image_ingest_yuv16(const uint16_t* y, const int64_t* ys, const uint16_t* cb, const int64_t* bs, const uint16_t* cr,
                        const int64_t* rs, const YuvDesc* desc, int depth, int msb, int B, int H, int W, float* dst,
                        int Hp, int Wp, hipStream_t st) {
  MLIC_CHECK(y != nullptr && cb != nullptr && cr != nullptr && dst != nullptr, "image_ingest_yuv16: null plane or dst");
  MLIC_CHECK(ys != nullptr && bs != nullptr && rs != nullptr, "image_ingest_yuv16: null strides");
  MLIC_CHECK(B >= 1 && H >= 1 && W >= 1, "image_ingest_yuv16: B, H and W must be positive");
  MLIC_CHECK(Hp >= H && Wp >= W && Hp % 64 == 0 && Wp % 64 == 0,
             "image_ingest_yuv16: Hp, Wp must be multiples of 64 that cover H, W");
  const Fmt16 f = fmt16(depth, msb, "image_ingest_yuv16");
  YuvSetup u = yuv_setup(desc, depth, "image_ingest_yuv16");
  MLIC_CHECK(ys[2] != 0 && bs[2] != 0 && rs[2] != 0, "image_ingest_yuv16: zero column stride");
  aligned2(y, "image_ingest_yuv16", "y");
  aligned2(cb, "image_ingest_yuv16", "cb");
  aligned2(cr, "image_ingest_yuv16", "cr");
  MLIC_CHECK(reinterpret_cast<uintptr_t>(dst) % 4 == 0, "image_ingest_yuv16: dst must be 4-byte aligned");
  const uint16_t* p[3] = {y, cb, cr};
  const int64_t* s[3] = {ys, bs, rs};
  const int form = yuv_form(p, s, &u.q);
  int tx, ty;
  const unsigned blocks = blocks_of(B, Hp, Wp, ROWS, &tx, &ty);
  const Planes3 P = planes3(p, s);
  const int vec = reinterpret_cast<uintptr_t>(dst) % 16 == 0;  // planes and rows are multiples of 16 bytes
  if (form == YUV_PLANAR)
    hipLaunchKernelGGL(ingest_yuv16_kernel<YUV_PLANAR>, dim3(blocks), dim3(256), 0, st, P, u.q, u.in, f, H, W, dst, Hp,
                       Wp, tx, ty, vec);
  else if (form == YUV_NV)
    hipLaunchKernelGGL(ingest_yuv16_kernel<YUV_NV>, dim3(blocks), dim3(256), 0, st, P, u.q, u.in, f, H, W, dst, Hp, Wp,
                       tx, ty, vec);
  else
    hipLaunchKernelGGL(ingest_yuv16_kernel<YUV_GENERAL>, dim3(blocks), dim3(256), 0, st, P, u.q, u.in, f, H, W, dst, Hp,
                       Wp, tx, ty, vec);
  HIP_OK(hipGetLastError());
}

void image_egress_yuv16(const float* src, const int64_t* ss, int B, int H, int W, const YuvDesc* desc, int depth, int msb,
                        uint16_t* y, const int64_t* ys, uint16_t* cb, const int64_t* bs, uint16_t* cr, const int64_t* rs,
                        const uint16_t* ref_y, const int64_t* rys, const uint16_t* ref_cb, const int64_t* rbs,
                        const uint16_t* ref_cr, const int64_t* rrs, uint64_t* sq_err, hipStream_t st) {
  MLIC_CHECK(src != nullptr && y != nullptr && cb != nullptr && cr != nullptr, "image_egress_yuv16: null src or plane");
  MLIC_CHECK(ss != nullptr && ys != nullptr && bs != nullptr && rs != nullptr, "image_egress_yuv16: null strides");
  MLIC_CHECK(B >= 1 && H >= 1 && W >= 1, "image_egress_yuv16: B, H and W must be positive");
  const Fmt16 f = fmt16(depth, msb, "image_egress_yuv16");
  YuvSetup u = yuv_setup(desc, depth, "image_egress_yuv16");
  MLIC_CHECK(ys[2] != 0 && bs[2] != 0 && rs[2] != 0, "image_egress_yuv16: zero column stride");
  const int nref = (ref_y != nullptr) + (ref_cb != nullptr) + (ref_cr != nullptr) + (sq_err != nullptr);
  MLIC_CHECK(nref == 0 || nref == 4, "image_egress_yuv16: the three ref planes and sq_err are all given or all NULL");
  MLIC_CHECK(nref == 0 || (rys != nullptr && rbs != nullptr && rrs != nullptr), "image_egress_yuv16: null ref strides");
  MLIC_CHECK(nref == 0 || (rys[2] != 0 && rbs[2] != 0 && rrs[2] != 0), "image_egress_yuv16: zero column stride (ref)");
  aligned2(y, "image_egress_yuv16", "y");
  aligned2(cb, "image_egress_yuv16", "cb");
  aligned2(cr, "image_egress_yuv16", "cr");
  aligned2(ref_y, "image_egress_yuv16", "ref_y");
  aligned2(ref_cb, "image_egress_yuv16", "ref_cb");
  aligned2(ref_cr, "image_egress_yuv16", "ref_cr");
  MLIC_CHECK(reinterpret_cast<uintptr_t>(src) % 4 == 0, "image_egress_yuv16: src must be 4-byte aligned");
  MLIC_CHECK(reinterpret_cast<uintptr_t>(sq_err) % 8 == 0, "image_egress_yuv16: sq_err must be 8-byte aligned");
  const uint16_t* p[3] = {y, cb, cr};
  const int64_t* s[3] = {ys, bs, rs};
  const int form = yuv_form(p, s, &u.q);
  const bool ref = nref == 4;
  const int CH = (H + u.q.sub_y - 1) / u.q.sub_y;
  int tx, ty;
  const unsigned blocks = blocks_of(B, CH, W, (ref ? YUV_REF_GROUPS : 1) * ROWS, &tx, &ty);
  const Planes3 D = planes3(p, s);
  Planes3 Rf = D;
  if (ref) {
    const uint16_t* rp[3] = {ref_y, ref_cb, ref_cr};
    const int64_t* rst[3] = {rys, rbs, rrs};
    Rf = planes3(rp, rst);
  }
  const IoStride3 s3{ss[0], ss[1], ss[2]};
  if (sq_err) HIP_OK(hipMemsetAsync(sq_err, 0, sizeof(uint64_t) * 3 * (size_t)B, st));
  if (form == YUV_PLANAR)
    egress_yuv_launch<YUV_PLANAR>(blocks, st, src, s3, H, W, u.q, u.out, f, D, Rf, ref, sq_err, tx, ty);
  else if (form == YUV_NV)
    egress_yuv_launch<YUV_NV>(blocks, st, src, s3, H, W, u.q, u.out, f, D, Rf, ref, sq_err, tx, ty);
  else
    egress_yuv_launch<YUV_GENERAL>(blocks, st, src, s3, H, W, u.q, u.out, f, D, Rf, ref, sq_err, tx, ty);
  HIP_OK(hipGetLastError());
}

}  // namespace mlic
