// 8-bit Y'CbCr frames in and out (DESIGN.md section 5 "YCbCr I/O"), one launch each.
//
// ingest: three byte planes (Y of H x W, Cb and Cr of ceil(W / sub_x) x ceil(H / sub_y)), each read through its own
// element strides {image, row, column}, become the model's input fp32 [B][3][Hp][Wp]: chroma is upsampled to the
// luma grid in integers (sixteenths: 3 : 1 between the two nearest samples of a subsampled axis, centre sited, or
// 4 : 0 / 2 : 2 across columns when the chroma sample is co-sited with the even luma column), then
//   a = cy (Y - yo);  R = a + crv v;  G = (a - cgu u) - cgv v;  B = a + cbu u;  clamp to [0, 1]
// in fp32 with every product and sum rounded once.  +0 in the right / bottom padding; every element is written.
// egress: the H x W crop of fp32 planes becomes the three byte planes: per pixel the clamped r, g, b give t_Y and
// the full-resolution chroma (t_Cb, t_Cr without the 128), chroma is filtered at luma resolution (the mean of the
// sub_x x sub_y block, or [1 2 1] / 4 across columns for left siting) with indices clamped into the image, 128 is
// added, and floor(clamp(t + 0.5, 0, 255)) is the byte.  With reference planes the per-plane sums of squared byte
// differences are accumulated in integers (three 64-bit atomics per block).
//
// A block is four waves.  Ingest: a wave owns one luma row and 256 pixels of it (image_io.hip's ingest_u8_kernel
// with two more byte rows per chroma plane), a lane four consecutive pixels: four chroma samples per row and plane
// feed them, and the fp32 side is one 16-byte store per lane and channel; the loads of all its byte rows are
// issued before the first LDS store (stage_load / stage_store below: a wave waits for memory once).  Egress: a wave owns one chroma row and
// 256 luma columns of it, a lane four luma columns of the sub_y luma rows (two sub_x x sub_y quads, or four 4:4:4
// pixels); the column to the left of a lane's first quad (left siting) comes from the neighbouring lane, and from
// memory only at a wave's first lane.
// Byte rows with unit column stride (planar), and interleaved chroma with column stride 2 (NV12 / NV21), go
// through LDS (image_stage.h); any other stride set takes byte accesses straight from / to global memory.  All
// forms give the same bits.
#include "image_stage.h"
#include "kernels.h"

namespace mlic {

namespace {

constexpr int YUV_TW = 256, YUV_ROWS = 4;
constexpr int YUV_SEG = YUV_TW / 4 + 1;    // dwords of a 256-byte segment at any alignment
constexpr int YUV_CSEG = YUV_TW / 4 + 2;   // ingest: up to 258 chroma bytes (a neighbour at either end) at any alignment
constexpr int YUV_IN_LDS = YUV_SEG + 4 * YUV_CSEG;  // Y | Cb row 0, Cb row 1, Cr row 0, Cr row 1 (NV: uv row 0, uv row 1)
constexpr int YUV_OUT_LDS = 4 * YUV_SEG;            // Y row 0, Y row 1 | Cb, Cr (NV: uv, up to 515 bytes)
// image_io.hip IO_REF_GROUPS, halved: a group here is eight pixels a lane, and 32 x 1080 x 1920 keeps 4 608 blocks
constexpr int YUV_REF_GROUPS = 8;
enum { YUV_GENERAL = 0, YUV_PLANAR = 1, YUV_NV = 2 };

struct PlaneStride {
  int64_t img, row, col;
};
struct Planes3 {
  uint8_t* p[3];  // Y, Cb, Cr
  PlaneStride s[3];
};
struct SrcStride3 {
  int64_t img, ch, row;
};
struct YuvGeom {
  int sub_x, sub_y, left;  // left: sub_x == 2 and chroma co-sited with the even luma column
  int uv_b, uv_r;          // NV form: Cb's and Cr's byte within the interleaved pair (the pair starts at p[1] - uv_b)
};
struct YuvIn {
  float yo, cy, crv, cgu, cgv, cbu;
};
struct YuvOut {
  float yo, yr, yg, yb, br, bg, bb, rr, rg, rb;
};

struct YuvTile {
  int64_t img;
  int y, x0;
};
// blockIdx.x = (image, row block, column tile), column tile fastest; y = this wave's row in the block's first group
__device__ inline YuvTile yuv_tile(int tiles_x, int tiles_y, int rows) {
  const int64_t t = blockIdx.x;
  const int64_t ry = t / tiles_x;
  YuvTile o;
  o.x0 = (int)(t - ry * tiles_x) * YUV_TW;
  o.img = ry / tiles_y;
  o.y = (int)(ry - o.img * tiles_y) * rows + (int)(threadIdx.x >> 6);
  return o;
}

// stage_in (image_stage.h) in two steps and without a loop, so that several rows' loads are in flight together.
// The segment p[0, n) sits in LDS at bytes [sh, sh + n), sh = p mod 4.  load: lane's whole dwords lane + 64 j of it
// (those that lie inside the segment) and one edge byte: lanes 0..2 take the up to three bytes before the first
// whole dword, lanes 3..5 the up to three after the last.  Nothing outside the segment is read.  store: the same
// dwords and bytes into LDS.
struct StageEdge {
  int pos;  // LDS byte position of this lane's edge byte, -1 = none
  uint32_t byte;
};
__device__ inline int stage_edge_pos(int sh, int end, int lane) {
  const int k0 = (sh + 3) >> 2, k1 = end >> 2;  // whole dwords [k0, k1)
  const int head_end = min(4 * k0, end), tail = max(4 * k1, 4 * k0);
  int pos = -1;
  if (lane < 3 && sh + lane < head_end) pos = sh + lane;
  if (lane >= 3 && lane < 6 && tail + (lane - 3) < end) pos = tail + (lane - 3);
  return pos;
}
template <int N>
__device__ inline void stage_load(const uint8_t* __restrict__ p, int n, int lane, uint32_t (&v)[N], StageEdge* e) {
  const int sh = addr_mod4(p), end = sh + n;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const int lo = 4 * (lane + 64 * j);
    v[j] = 0;
    if (lo >= sh && lo + 4 <= end) v[j] = *reinterpret_cast<const uint32_t*>(p + (lo - sh));
  }
  e->pos = stage_edge_pos(sh, end, lane);
  e->byte = 0;
  if (e->pos >= 0) e->byte = p[e->pos - sh];
}
template <int N>
__device__ inline void stage_store(uint32_t* r, int n, int sh, int lane, const uint32_t (&v)[N], const StageEdge& e) {
  const int end = sh + n;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const int lo = 4 * (lane + 64 * j);
    if (lo >= sh && lo + 4 <= end) r[lane + 64 * j] = v[j];
  }
  if (e.pos >= 0) reinterpret_cast<uint8_t*>(r)[e.pos] = (uint8_t)e.byte;
}

template <int FORM>
__global__ __launch_bounds__(256) void ingest_yuv8_kernel(Planes3 P, YuvGeom q, YuvIn k, int H, int W,
                                                          float* __restrict__ dst, int Hp, int Wp, int tiles_x,
                                                          int tiles_y, int vec) {
  __shared__ uint32_t S[YUV_ROWS][YUV_IN_LDS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const YuvTile t = yuv_tile(tiles_x, tiles_y, YUV_ROWS);
  const int y = t.y, x0 = t.x0;
  const int nx = y < H ? min(YUV_TW, max(W - x0, 0)) : 0;  // pixels of this row piece inside the image
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
  const uint8_t* yrow = P.p[0] + t.img * P.s[0].img + (int64_t)y * P.s[0].row + (int64_t)x0 * P.s[0].col;
  const uint8_t* crow[2][2];  // [plane][row]: the row's first sample
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    crow[p][0] = P.p[1 + p] + t.img * P.s[1 + p].img + (int64_t)r0 * P.s[1 + p].row;
    crow[p][1] = P.p[1 + p] + t.img * P.s[1 + p].img + (int64_t)r1 * P.s[1 + p].row;
  }
  uint8_t* S8 = reinterpret_cast<uint8_t*>(S[wave]);
  int shy = 0, shc[2][2] = {{0, 0}, {0, 0}};  // LDS byte offsets of sample `lo` (planar) / of pair `lo` (NV)
  if (FORM != YUV_GENERAL && nx > 0) {
    // every row's loads are issued before the first LDS store: one memory round trip a wave, not one per row
    const bool two = wv1 != 0;  // the second chroma row has a weight
    uint32_t vy[2];
    StageEdge ey;
    shy = addr_mod4(yrow);
    stage_load<2>(yrow, nx, lane, vy, &ey);
    if (FORM == YUV_PLANAR) {
      uint32_t vc[2][2][2];
      StageEdge ec[2][2];
      const uint8_t* g[2][2];
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          g[p][r] = crow[p][r] + lo;
          shc[p][r] = (YUV_SEG + (2 * p + r) * YUV_CSEG) * 4 + addr_mod4(g[p][r]);
          if (r == 0 || two) stage_load<2>(g[p][r], hi - lo, lane, vc[p][r], &ec[p][r]);
        }
      stage_store<2>(S[wave], nx, shy, lane, vy, ey);
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int r = 0; r < 2; ++r)
          if (r == 0 || two)
            stage_store<2>(S[wave] + YUV_SEG + (2 * p + r) * YUV_CSEG, hi - lo, addr_mod4(g[p][r]), lane, vc[p][r],
                           ec[p][r]);
    } else {
      uint32_t vc[2][3];
      StageEdge ec[2];
      const uint8_t* g[2];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        g[r] = crow[0][r] - q.uv_b + 2 * (int64_t)lo;  // the pair of chroma sample lo
        const int at = (YUV_SEG + 2 * r * YUV_CSEG) * 4 + addr_mod4(g[r]);
        shc[0][r] = at + q.uv_b;
        shc[1][r] = at + q.uv_r;
        if (r == 0 || two) stage_load<3>(g[r], 2 * (hi - lo), lane, vc[r], &ec[r]);
      }
      stage_store<2>(S[wave], nx, shy, lane, vy, ey);
#pragma unroll
      for (int r = 0; r < 2; ++r)
        if (r == 0 || two) stage_store<3>(S[wave] + YUV_SEG + 2 * r * YUV_CSEG, 2 * (hi - lo), addr_mod4(g[r]), lane, vc[r],
                                             ec[r]);
    }
  }
  if (FORM != YUV_GENERAL) __syncthreads();
  // chroma sample i of plane p, row r
  auto C = [&](int p, int r, int i) -> int {
    if (FORM == YUV_PLANAR) return S8[shc[p][r] + (i - lo)];
    if (FORM == YUV_NV) return S8[shc[p][r] + 2 * (i - lo)];
    return crow[p][r][(int64_t)i * P.s[1 + p].col];
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
          const int cm = C(p, r, max(ia - 1, lo)), ca = C(p, r, ia), cb = C(p, r, min(ia + 1, hi - 1)),
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
      const int Y = FORM == YUV_GENERAL ? (int)yrow[(int64_t)(px + e) * P.s[0].col] : (int)S8[shy + px + e];
      const int c16b = wv0 * h[0][0][e] + wv1 * h[0][1][e], c16r = wv0 * h[1][0][e] + wv1 * h[1][1][e];  // [0, 4080]
      const float u = (float)c16b * 0.0625f - 128.0f, v = (float)c16r * 0.0625f - 128.0f;  // exact
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

__device__ inline int yuv_byte(float t) { return (int)floorf(fminf(fmaxf(__fadd_rn(t, 0.5f), 0.0f), 255.0f)); }

template <int FORM, bool REF>
__global__ __launch_bounds__(256) void egress_yuv8_kernel(const float* __restrict__ src, SrcStride3 ss, int H, int W,
                                                          YuvGeom q, YuvOut k, Planes3 D, Planes3 Rf,
                                                          unsigned long long* __restrict__ sq_err, int tiles_x,
                                                          int tiles_y) {
  __shared__ uint32_t S[YUV_ROWS][YUV_OUT_LDS];
  __shared__ unsigned int red[YUV_ROWS][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int G = REF ? YUV_REF_GROUPS : 1;  // chroma row groups this block walks
  const YuvTile t = yuv_tile(tiles_x, tiles_y, G * YUV_ROWS);
  const int x0 = t.x0;
  const int CW = (W + q.sub_x - 1) / q.sub_x, CH = (H + q.sub_y - 1) / q.sub_y;
  uint8_t* S8 = reinterpret_cast<uint8_t*>(S[wave]);
  const int lx = x0 + 4 * lane;  // this lane's first luma column
  int xc[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) xc[e] = min(lx + e, W - 1);
  const int nc = q.sub_x == 2 ? 2 : 4;         // chroma samples per lane
  const int c0 = x0 / q.sub_x;                 // the piece's first chroma column
  const int cl = lx / q.sub_x;                 // this lane's first chroma column
  const int taps = (q.left ? 4 : q.sub_x) * q.sub_y;  // the filter's weights sum to this: 1, 2, 4 or 8
  const float scale = taps == 8 ? 0.125f : taps == 4 ? 0.25f : taps == 2 ? 0.5f : 1.0f;
  unsigned int acc[3] = {0, 0, 0};             // <= G * 8 * 255^2 per lane
  for (int g = 0; g < G; ++g) {
    const int cy = t.y + g * YUV_ROWS;         // this wave's chroma row
    const int nx = cy < CH ? min(YUV_TW, W - x0) : 0;  // x0 < W: the tiles cover the crop only
    const int ncx = (nx + q.sub_x - 1) / q.sub_x;
    uint8_t* yrow[2];
    uint8_t* crow[2];
    int shy[2] = {0, 0}, shc[2] = {0, 0};
    if (nx > 0) {
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int yy = min(cy * q.sub_y + r, H - 1);
        yrow[r] = D.p[0] + t.img * D.s[0].img + (int64_t)yy * D.s[0].row + (int64_t)x0 * D.s[0].col;
        if (FORM != YUV_GENERAL) shy[r] = r * YUV_SEG * 4 + addr_mod4(yrow[r]);
      }
#pragma unroll
      for (int p = 0; p < 2; ++p)
        crow[p] = D.p[1 + p] + t.img * D.s[1 + p].img + (int64_t)cy * D.s[1 + p].row + (int64_t)c0 * D.s[1 + p].col;
      if (FORM == YUV_PLANAR) {
        shc[0] = 2 * YUV_SEG * 4 + addr_mod4(crow[0]);
        shc[1] = 3 * YUV_SEG * 4 + addr_mod4(crow[1]);
      }
      if (FORM == YUV_NV) {
        const int at = 2 * YUV_SEG * 4 + addr_mod4(crow[0] - q.uv_b);
        shc[0] = at + q.uv_b;
        shc[1] = at + q.uv_r;
      }
      // full-resolution chroma of this lane's four columns and of the column to their left, per luma row
      Chroma2 cf[2][5];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        if (r >= q.sub_y) break;
        const int yr = cy * q.sub_y + r;  // the block's row; past H it repeats row H - 1 and gives no Y bytes
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
          int rv[4] = {0, 0, 0, 0};  // the reference's four bytes: one 4-byte load where they are contiguous
          if (REF && lx < W) {
            const uint8_t* rp = Rf.p[0] + t.img * Rf.s[0].img + (int64_t)yr * Rf.s[0].row + (int64_t)lx * Rf.s[0].col;
            if (Rf.s[0].col == 1 && lx + 3 < W) {
              uint32_t w4;
              __builtin_memcpy(&w4, rp, 4);
#pragma unroll
              for (int e = 0; e < 4; ++e) rv[e] = (int)((w4 >> (8 * e)) & 255u);
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e)
                if (lx + e < W) rv[e] = (int)rp[(int64_t)e * Rf.s[0].col];
            }
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            if (lx + e >= W) break;
            const int u = yuv_byte(ty[e]);
            if (FORM == YUV_GENERAL) yrow[r][(int64_t)(4 * lane + e) * D.s[0].col] = (uint8_t)u;
            else S8[shy[r] + 4 * lane + e] = (uint8_t)u;
            if (REF) {
              const int d = u - rv[e];
              acc[0] += (unsigned int)(d * d);
            }
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
        const int ub = yuv_byte(__fadd_rn(__fmul_rn(sb, scale), 128.0f));
        const int ur = yuv_byte(__fadd_rn(__fmul_rn(sr, scale), 128.0f));
        const int ci = cl + m - c0;  // within the piece
        if (FORM == YUV_GENERAL) {
          crow[0][(int64_t)ci * D.s[1].col] = (uint8_t)ub;
          crow[1][(int64_t)ci * D.s[2].col] = (uint8_t)ur;
        } else {
          const int st = FORM == YUV_NV ? 2 : 1;
          S8[shc[0] + st * ci] = (uint8_t)ub;
          S8[shc[1] + st * ci] = (uint8_t)ur;
        }
        if (REF) {
          const int db = ub - (int)Rf.p[1][t.img * Rf.s[1].img + (int64_t)cy * Rf.s[1].row +
                                           (int64_t)(cl + m) * Rf.s[1].col];
          const int dr = ur - (int)Rf.p[2][t.img * Rf.s[2].img + (int64_t)cy * Rf.s[2].row +
                                           (int64_t)(cl + m) * Rf.s[2].col];
          acc[1] += (unsigned int)(db * db);
          acc[2] += (unsigned int)(dr * dr);
        }
      }
    }
    if (FORM != YUV_GENERAL) {
      __syncthreads();
      if (nx > 0) {
#pragma unroll
        for (int r = 0; r < 2; ++r)
          if (r < q.sub_y && cy * q.sub_y + r < H) stage_out(yrow[r], nx, S[wave] + r * YUV_SEG, lane);
        if (FORM == YUV_PLANAR) {
          stage_out(crow[0], ncx, S[wave] + 2 * YUV_SEG, lane);
          stage_out(crow[1], ncx, S[wave] + 3 * YUV_SEG, lane);
        } else {
          stage_out(crow[0] - q.uv_b, 2 * ncx, S[wave] + 2 * YUV_SEG, lane);
        }
      }
      if (G > 1) __syncthreads();  // the next group's bytes go into the same LDS
    }
  }
  if (REF) {
    // a wave's sum is at most 64 * G * 8 * 255^2 < 2^30
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) acc[c] += __shfl_down(acc[c], off, 64);
      if (lane == 0) red[wave][c] = acc[c];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
      const int c = threadIdx.x;
      const unsigned long long s = (unsigned long long)red[0][c] + (unsigned long long)red[1][c] +
                                   (unsigned long long)red[2][c] + (unsigned long long)red[3][c];
      if (s) atomicAdd(sq_err + t.img * 3 + c, s);
    }
  }
}

struct YuvSetup {
  YuvGeom q;
  YuvIn in;
  YuvOut out;
};

// the description's checks (each refusal its own message) and the constants, folded in double and rounded once
YuvSetup yuv_setup(const YuvDesc* d, const char* who) {
  const std::string w = std::string(who) + ": ";
  if (d == nullptr) throw Error("mlic: " + w + "null desc");
  if (!((d->sub_x == 1 || d->sub_x == 2) && (d->sub_y == 1 || d->sub_y == 2)))
    throw Error("mlic: " + w + "sub_x and sub_y must be 1 or 2");
  if (d->sub_x == 1 && d->sub_y == 2) throw Error("mlic: " + w + "sub_x 1 with sub_y 2 (4:4:0) is not supported");
  if (d->matrix != 0 && d->matrix != 1) throw Error("mlic: " + w + "matrix must be 0 (BT.601) or 1 (BT.709)");
  if (d->full_range != 0 && d->full_range != 1) throw Error("mlic: " + w + "full_range must be 0 or 1");
  if (d->site_x != 0 && d->site_x != 1) throw Error("mlic: " + w + "site_x must be 0 (centre) or 1 (left)");
  if (d->reserved[0] != 0 || d->reserved[1] != 0 || d->reserved[2] != 0)
    throw Error("mlic: " + w + "reserved fields must be 0");
  const double Kr = d->matrix ? 0.2126 : 0.299, Kb = d->matrix ? 0.0722 : 0.114, Kg = 1.0 - Kr - Kb;
  const double ys = d->full_range ? 255.0 : 219.0, cs = d->full_range ? 255.0 : 224.0, yo = d->full_range ? 0.0 : 16.0;
  YuvSetup s;
  s.q = YuvGeom{d->sub_x, d->sub_y, (d->sub_x == 2 && d->site_x == 1) ? 1 : 0, 0, 1};
  s.in = YuvIn{(float)yo,
               (float)(1.0 / ys),
               (float)(2.0 * (1.0 - Kr) / cs),
               (float)(2.0 * Kb * (1.0 - Kb) / (Kg * cs)),
               (float)(2.0 * Kr * (1.0 - Kr) / (Kg * cs)),
               (float)(2.0 * (1.0 - Kb) / cs)};
  s.out = YuvOut{(float)yo,
                 (float)(ys * Kr),
                 (float)(ys * Kg),
                 (float)(ys * Kb),
                 (float)(-(cs * Kr) / (2.0 * (1.0 - Kb))),
                 (float)(-(cs * Kg) / (2.0 * (1.0 - Kb))),
                 (float)(cs / 2.0),
                 (float)(cs / 2.0),
                 (float)(-(cs * Kg) / (2.0 * (1.0 - Kr))),
                 (float)(-(cs * Kb) / (2.0 * (1.0 - Kr)))};
  return s;
}

// the kernel form for these planes, as io_path picks one for a byte image; fills the NV byte positions
int yuv_form(const uint8_t* const* p, const int64_t* const* s, YuvGeom* q) {
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

unsigned yuv_blocks(int B, int rows, int cols, int block_rows, int* tiles_x, int* tiles_y) {
  *tiles_x = (cols + YUV_TW - 1) / YUV_TW;
  *tiles_y = (rows + block_rows - 1) / block_rows;
  const int64_t blocks = (int64_t)B * *tiles_x * *tiles_y;
  MLIC_CHECK(blocks <= 0x7fffffffLL, "image_yuv: batch too large for one launch");
  return (unsigned)blocks;
}

Planes3 planes3(const uint8_t* const* p, const int64_t* const* s) {
  Planes3 P;
  for (int c = 0; c < 3; ++c) {
    P.p[c] = const_cast<uint8_t*>(p[c]);
    P.s[c] = PlaneStride{s[c][0], s[c][1], s[c][2]};
  }
  return P;
}

template <int FORM>
void egress_yuv_launch(unsigned blocks, hipStream_t st, const float* src, SrcStride3 ss, int H, int W, YuvGeom q,
                       YuvOut k, Planes3 D, Planes3 Rf, bool ref, uint64_t* sq, int tx, int ty) {
  auto* sq64 = reinterpret_cast<unsigned long long*>(sq);
  if (ref)
    hipLaunchKernelGGL((egress_yuv8_kernel<FORM, true>), dim3(blocks), dim3(256), 0, st, src, ss, H, W, q, k, D, Rf,
                       sq64, tx, ty);
  else
    hipLaunchKernelGGL((egress_yuv8_kernel<FORM, false>), dim3(blocks), dim3(256), 0, st, src, ss, H, W, q, k, D, Rf,
                       sq64, tx, ty);
}

}  // namespace

void image_ingest_yuv8(const uint8_t* y, const int64_t* ys, const uint8_t* cb, const int64_t* bs, const uint8_t* cr,
                       const int64_t* rs, const YuvDesc* desc, int B, int H, int W, float* dst, int Hp, int Wp,
                       hipStream_t st) {
  MLIC_CHECK(y != nullptr && cb != nullptr && cr != nullptr && dst != nullptr, "image_ingest_yuv8: null plane or dst");
  MLIC_CHECK(ys != nullptr && bs != nullptr && rs != nullptr, "image_ingest_yuv8: null strides");
  MLIC_CHECK(B >= 1 && H >= 1 && W >= 1, "image_ingest_yuv8: B, H and W must be positive");
  MLIC_CHECK(Hp >= H && Wp >= W && Hp % 64 == 0 && Wp % 64 == 0,
             "image_ingest_yuv8: Hp, Wp must be multiples of 64 that cover H, W");
  YuvSetup u = yuv_setup(desc, "image_ingest_yuv8");
  MLIC_CHECK(ys[2] != 0 && bs[2] != 0 && rs[2] != 0, "image_ingest_yuv8: zero column stride");
  MLIC_CHECK(reinterpret_cast<uintptr_t>(dst) % 4 == 0, "image_ingest_yuv8: dst must be 4-byte aligned");
  const uint8_t* p[3] = {y, cb, cr};
  const int64_t* s[3] = {ys, bs, rs};
  const int form = yuv_form(p, s, &u.q);
  int tx, ty;
  const unsigned blocks = yuv_blocks(B, Hp, Wp, YUV_ROWS, &tx, &ty);
  const Planes3 P = planes3(p, s);
  const int vec = reinterpret_cast<uintptr_t>(dst) % 16 == 0;  // planes and rows are multiples of 16 bytes
  if (form == YUV_PLANAR)
    hipLaunchKernelGGL(ingest_yuv8_kernel<YUV_PLANAR>, dim3(blocks), dim3(256), 0, st, P, u.q, u.in, H, W, dst, Hp, Wp,
                       tx, ty, vec);
  else if (form == YUV_NV)
    hipLaunchKernelGGL(ingest_yuv8_kernel<YUV_NV>, dim3(blocks), dim3(256), 0, st, P, u.q, u.in, H, W, dst, Hp, Wp, tx,
                       ty, vec);
  else
    hipLaunchKernelGGL(ingest_yuv8_kernel<YUV_GENERAL>, dim3(blocks), dim3(256), 0, st, P, u.q, u.in, H, W, dst, Hp,
                       Wp, tx, ty, vec);
  HIP_OK(hipGetLastError());
}

void image_egress_yuv8(const float* src, const int64_t* ss, int B, int H, int W, const YuvDesc* desc, uint8_t* y,
                       const int64_t* ys, uint8_t* cb, const int64_t* bs, uint8_t* cr, const int64_t* rs,
                       const uint8_t* ref_y, const int64_t* rys, const uint8_t* ref_cb, const int64_t* rbs,
                       const uint8_t* ref_cr, const int64_t* rrs, uint64_t* sq_err, hipStream_t st) {
  MLIC_CHECK(src != nullptr && y != nullptr && cb != nullptr && cr != nullptr, "image_egress_yuv8: null src or plane");
  MLIC_CHECK(ss != nullptr && ys != nullptr && bs != nullptr && rs != nullptr, "image_egress_yuv8: null strides");
  MLIC_CHECK(B >= 1 && H >= 1 && W >= 1, "image_egress_yuv8: B, H and W must be positive");
  YuvSetup u = yuv_setup(desc, "image_egress_yuv8");
  MLIC_CHECK(ys[2] != 0 && bs[2] != 0 && rs[2] != 0, "image_egress_yuv8: zero column stride");
  const int nref = (ref_y != nullptr) + (ref_cb != nullptr) + (ref_cr != nullptr) + (sq_err != nullptr);
  MLIC_CHECK(nref == 0 || nref == 4, "image_egress_yuv8: the three ref planes and sq_err are all given or all NULL");
  MLIC_CHECK(nref == 0 || (rys != nullptr && rbs != nullptr && rrs != nullptr), "image_egress_yuv8: null ref strides");
  MLIC_CHECK(nref == 0 || (rys[2] != 0 && rbs[2] != 0 && rrs[2] != 0), "image_egress_yuv8: zero column stride (ref)");
  MLIC_CHECK(reinterpret_cast<uintptr_t>(src) % 4 == 0, "image_egress_yuv8: src must be 4-byte aligned");
  MLIC_CHECK(reinterpret_cast<uintptr_t>(sq_err) % 8 == 0, "image_egress_yuv8: sq_err must be 8-byte aligned");
  const uint8_t* p[3] = {y, cb, cr};
  const int64_t* s[3] = {ys, bs, rs};
  const int form = yuv_form(p, s, &u.q);
  const bool ref = nref == 4;
  const int CH = (H + u.q.sub_y - 1) / u.q.sub_y;
  int tx, ty;
  const unsigned blocks = yuv_blocks(B, CH, W, (ref ? YUV_REF_GROUPS : 1) * YUV_ROWS, &tx, &ty);
  const Planes3 D = planes3(p, s);
  Planes3 Rf = D;
  if (ref) {
    const uint8_t* rp[3] = {ref_y, ref_cb, ref_cr};
    const int64_t* rst[3] = {rys, rbs, rrs};
    Rf = planes3(rp, rst);
  }
  const SrcStride3 s3{ss[0], ss[1], ss[2]};
  if (sq_err) HIP_OK(hipMemsetAsync(sq_err, 0, sizeof(uint64_t) * 3 * (size_t)B, st));
  if (form == YUV_PLANAR) egress_yuv_launch<YUV_PLANAR>(blocks, st, src, s3, H, W, u.q, u.out, D, Rf, ref, sq_err, tx, ty);
  else if (form == YUV_NV) egress_yuv_launch<YUV_NV>(blocks, st, src, s3, H, W, u.q, u.out, D, Rf, ref, sq_err, tx, ty);
  else egress_yuv_launch<YUV_GENERAL>(blocks, st, src, s3, H, W, u.q, u.out, D, Rf, ref, sq_err, tx, ty);
  HIP_OK(hipGetLastError());
}

}  // namespace mlic
