// MS-SSIM (utils/metrics.py:13-53 via pytorch_msssim's defaults, restated in DESIGN.md §3) of uint8-valued
// images: one fused launch per level and one small combine launch.
//
// A level launch tiles the h x w input plane in 64 x 64 tiles whose origin sits on the 2x2 pooling grid
// (origin -1 on an odd side: the pooling's leading zero pad).  A block stages its tile plus the 10-pixel
// right/bottom halo of both images in LDS (level 0 converts the caller's fp32 to uint8 values on load,
// exactly as sq_err_u8_kernel), and from that one staged copy
//   - writes the 2x2-pooled tile of both images for the next level (the pooled plane covers all of h x w),
//   - forms the five 11-tap Gaussian moments separably in registers for the map pixels whose window starts
//     in the tile (the map covers (h-10) x (w-10)), evaluates cs_map and ssim_map and reduces them to one
//     pair of double partial sums per block.
// No moment plane and no map goes to memory.  The combine kernel adds the partials in tile order, so the
// result is bit-reproducible and does not depend on the batch an image is scored in.
#include "kernels.h"

#include <cmath>

namespace mlic {

namespace {

constexpr int MS_TH = 64, MS_TW = 64;  // tile of window origins / pooled inputs (even: stays on the pooling grid)
constexpr int MS_HALO = 10, MS_WIN = 11;
constexpr int MS_SH = MS_TH + MS_HALO, MS_SW = MS_TW + MS_HALO;  // staged rows / columns
constexpr int MS_ROWS = MS_TH / 4;  // map rows per thread: 256 threads = 64 columns x 4 row groups
constexpr int MS_LEVELS = 5;

typedef float v2f __attribute__((ext_vector_type(2)));

struct MsWin {
  float g[MS_WIN];
};

struct MsStride {
  int64_t img, ch, row;
};

struct MsCombine {
  int64_t part_off[MS_LEVELS];  // doubles from the start of the partial sums
  int tiles[MS_LEVELS];
  double count[MS_LEVELS];  // map pixels per plane
  double weight[MS_LEVELS];
};

template <bool U8>
__global__ __launch_bounds__(256) void ms_ssim_level_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                            MsStride sa, MsStride sb, int C, int h, int w,
                                                            int tiles_x, int tiles_y, float* __restrict__ pa,
                                                            float* __restrict__ pb, double* __restrict__ part,
                                                            MsWin win) {
  __shared__ float2 S[MS_SH * MS_SW];  // {a, b} per pixel: one 8-byte LDS read serves both images
  __shared__ double red[8];
  const int tid = threadIdx.x;
  const int tiles = tiles_x * tiles_y;
  const int64_t plane = (int64_t)blockIdx.x / tiles;
  const int tile = (int)((int64_t)blockIdx.x - plane * tiles);
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int64_t img = plane / C, ch = plane - img * C;
  const int y0 = ty * MS_TH - (h & 1), x0 = tx * MS_TW - (w & 1);
  const float* ap = a + img * sa.img + ch * sa.ch;
  const float* bp = b + img * sb.img + ch * sb.ch;

  // stage: zeros outside the plane (the pooling's pad; no map pixel reads them)
  for (int i = tid; i < MS_SH * MS_SW; i += 256) {
    const int r = i / MS_SW, c = i - r * MS_SW;
    const int gy = y0 + r, gx = x0 + c;
    float va = 0.0f, vb = 0.0f;
    if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
      va = ap[(int64_t)gy * sa.row + gx];
      vb = bp[(int64_t)gy * sb.row + gx];
      if (U8) {
        va = floorf(fminf(fmaxf(va, 0.0f), 1.0f) * 255.0f);
        vb = floorf(fminf(fmaxf(vb, 0.0f), 1.0f) * 255.0f);
      }
    }
    S[i] = make_float2(va, vb);
  }
  __syncthreads();

  // avg_pool2d(2, 2, padding = side % 2, count_include_pad): window k = staged rows / columns {2k, 2k + 1}
  if (pa != nullptr) {
    const int ho = (h + 1) / 2, wo = (w + 1) / 2;
    float* pap = pa + plane * ((int64_t)ho * wo);
    float* pbp = pb + plane * ((int64_t)ho * wo);
    for (int i = tid; i < (MS_TH / 2) * (MS_TW / 2); i += 256) {
      const int ky = i / (MS_TW / 2), kx = i - ky * (MS_TW / 2);
      const int gky = ty * (MS_TH / 2) + ky, gkx = tx * (MS_TW / 2) + kx;
      if (gky < ho && gkx < wo) {
        const int o = 2 * ky * MS_SW + 2 * kx;
        const float2 p00 = S[o], p01 = S[o + 1], p10 = S[o + MS_SW], p11 = S[o + MS_SW + 1];
        pap[(int64_t)gky * wo + gkx] = ((p00.x + p01.x) + (p10.x + p11.x)) * 0.25f;
        pbp[(int64_t)gky * wo + gkx] = ((p00.y + p01.y) + (p10.y + p11.y)) * 0.25f;
      }
    }
  }

  // map pixels (y0 + ly0 + o, x0 + lx), o < MS_ROWS, of this thread; the window of map pixel (i, j) is
  // rows i .. i + 10, columns j .. j + 10
  const int lx = tid & 63, ly0 = (tid >> 6) * MS_ROWS;
  const v2f* S2 = reinterpret_cast<const v2f*>(S);
  const int gx = x0 + lx, gy0 = y0 + ly0;
  double cs_sum = 0.0, ss_sum = 0.0;
  if (gx >= 0 && gx < w - MS_HALO && gy0 < h - MS_HALO && gy0 + MS_ROWS > 0) {
    // moments of (x - sha), (y - shb), the values at the middle of the thread's windows: the variances
    // do not depend on the shift, and in a smooth region E[x'^2] - E[x']^2 no longer cancels ~2^14
    // against ~2^14 (at level 0 the subtraction is exact: integers)
    // (the row clamped into the plane: a zero of the padding would be no shift at all; the column is inside)
    const v2f sh = S2[min(ly0 + MS_ROWS / 2 + 5, h - 1 - y0) * MS_SW + lx + 5];
    const float sha = sh.x, shb = sh.y;
    const float C1 = (0.01f * 255.0f) * (0.01f * 255.0f), C2 = (0.03f * 255.0f) * (0.03f * 255.0f);
    // the two images' first and second moments as pairs {a, b}: packed fp32 instructions (v_pk_*_f32)
    v2f acc01[MS_ROWS], acc23[MS_ROWS];
    float acc4[MS_ROWS];
    // fully unrolled (every acc index is static); row r finishes map row r - 10, which is evaluated at
    // once, so at most 11 rows of accumulators are live
#pragma unroll
    for (int r = 0; r < MS_ROWS + MS_HALO; ++r) {
      const v2f* row = S2 + (ly0 + r) * MS_SW + lx;
      v2f h01 = {0.0f, 0.0f}, h23 = {0.0f, 0.0f};
      float h4 = 0.0f;
#pragma unroll
      for (int k = 0; k < MS_WIN; ++k) {
        const v2f x = row[k] - sh;
        const v2f gx = x * win.g[k];
        h01 += gx;
        h23 = __builtin_elementwise_fma(gx, x, h23);
        h4 = fmaf(gx.x, x.y, h4);
      }
#pragma unroll
      for (int o = 0; o < MS_ROWS; ++o) {
        const int k = r - o;
        if (k == 0) {  // first touch: no zero-initialised accumulator is live before its first row
          acc01[o] = h01 * win.g[0];
          acc23[o] = h23 * win.g[0];
          acc4[o] = h4 * win.g[0];
        } else if (k > 0 && k < MS_WIN) {
          const v2f gk = {win.g[k], win.g[k]};
          acc01[o] = __builtin_elementwise_fma(gk, h01, acc01[o]);
          acc23[o] = __builtin_elementwise_fma(gk, h23, acc23[o]);
          acc4[o] = fmaf(win.g[k], h4, acc4[o]);
        }
      }
      if (r >= MS_HALO) {
        const int o = r - MS_HALO, gy = gy0 + o;
        if (gy >= 0 && gy < h - MS_HALO) {
          const float ma = acc01[o].x, mb = acc01[o].y;
          const float va = acc23[o].x - ma * ma, vb = acc23[o].y - mb * mb, cab = acc4[o] - ma * mb;
          const float mu1 = sha + ma, mu2 = shb + mb;
          const float cs = (2.0f * cab + C2) / (va + vb + C2);
          const float lum = (2.0f * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1);
          cs_sum += (double)cs;
          ss_sum += (double)lum * (double)cs;
        }
      }
      // keep the scheduler from hoisting later rows' LDS reads over this one (register pressure)
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  // block sum in a fixed order: lanes by shuffle, then the four waves in turn
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    cs_sum += __shfl_down(cs_sum, off, 64);
    ss_sum += __shfl_down(ss_sum, off, 64);
  }
  if ((tid & 63) == 0) {
    red[(tid >> 6) * 2] = cs_sum;
    red[(tid >> 6) * 2 + 1] = ss_sum;
  }
  __syncthreads();
  if (tid == 0) {
    double* p = part + (int64_t)blockIdx.x * 2;
    p[0] = ((red[0] + red[2]) + red[4]) + red[6];
    p[1] = ((red[1] + red[3]) + red[5]) + red[7];
  }
}

// one block per image: term[l][c] = relu(mean of cs_map (levels 0-3) / ssim_map (level 4)), the partial
// sums added in tile order; out = mean over c of prod_l term[l][c] ^ weight[l]
__global__ void ms_ssim_combine_kernel(const double* __restrict__ part, MsCombine P, int C, double* __restrict__ tbuf,
                                       double* __restrict__ terms, double* __restrict__ out) {
  const int64_t img = blockIdx.x;
  for (int t = threadIdx.x; t < MS_LEVELS * C; t += blockDim.x) {
    const int l = t / C, c = t - l * C;
    const double* p = part + P.part_off[l] + (img * C + c) * (int64_t)P.tiles[l] * 2 + (l == MS_LEVELS - 1 ? 1 : 0);
    double s = 0.0;
    for (int k = 0; k < P.tiles[l]; ++k) s += p[2 * (int64_t)k];
    double v = s / P.count[l];
    v = v < 0.0 ? 0.0 : v;
    tbuf[img * MS_LEVELS * C + t] = v;
    if (terms != nullptr) terms[img * MS_LEVELS * C + t] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double acc = 0.0;
    for (int c = 0; c < C; ++c) {
      double prod = 1.0;
      for (int l = 0; l < MS_LEVELS; ++l) prod *= pow(tbuf[img * MS_LEVELS * C + l * C + c], P.weight[l]);
      acc += prod;
    }
    out[img] = acc / (double)C;
  }
}

// scratch layout: for levels 1..4 the pooled planes of a then b ([B*C][h_l][w_l] fp32), then the partial
// sums (per level [B*C][tiles_l][2] doubles), then the relu'd terms ([B][5][C] doubles); 256-byte aligned
struct MsPlan {
  int h[MS_LEVELS], w[MS_LEVELS], tx[MS_LEVELS], ty[MS_LEVELS];
  size_t plane_a[MS_LEVELS], plane_b[MS_LEVELS];  // byte offsets (levels 1..4)
  size_t part, terms, bytes;                      // byte offsets, total
  int64_t part_off[MS_LEVELS];                    // doubles from `part`
};

size_t align256(size_t v) { return (v + 255) / 256 * 256; }

MsPlan ms_plan(int B, int C, int H, int W) {
  MLIC_CHECK(B >= 1 && C >= 1, "ms_ssim: B and C must be positive");
  MLIC_CHECK(H > 160 && W > 160, "ms_ssim: the smaller image side must exceed 160 pixels (5 levels, 11-tap window)");
  MsPlan p{};
  const size_t planes = (size_t)B * (size_t)C;
  size_t off = 0;
  int64_t poff = 0;
  for (int l = 0; l < MS_LEVELS; ++l) {
    p.h[l] = l ? (p.h[l - 1] + 1) / 2 : H;
    p.w[l] = l ? (p.w[l - 1] + 1) / 2 : W;
    p.ty[l] = (p.h[l] + (p.h[l] & 1) + MS_TH - 1) / MS_TH;
    p.tx[l] = (p.w[l] + (p.w[l] & 1) + MS_TW - 1) / MS_TW;
    const int64_t blocks = (int64_t)planes * p.tx[l] * p.ty[l];
    MLIC_CHECK(blocks <= 0x7fffffffLL, "ms_ssim: batch too large for one launch per level");
    if (l) {
      const size_t one = align256(planes * (size_t)p.h[l] * (size_t)p.w[l] * sizeof(float));
      p.plane_a[l] = off;
      p.plane_b[l] = off + one;
      off += 2 * one;
    }
    p.part_off[l] = poff;
    poff += blocks * 2;
  }
  p.part = off;
  off += align256((size_t)poff * sizeof(double));
  p.terms = off;
  off += align256(planes * MS_LEVELS * sizeof(double));
  p.bytes = off;
  return p;
}

}  // namespace

size_t ms_ssim_scratch_bytes(int B, int C, int H, int W) { return ms_plan(B, C, H, W).bytes; }

void ms_ssim_u8(const float* a, const int64_t* a_strides, const float* b, const int64_t* b_strides, int B, int C,
                int H, int W, void* scratch, double* out, double* terms, hipStream_t st) {
  const MsPlan p = ms_plan(B, C, H, W);
  char* base = static_cast<char*>(scratch);
  double* part = reinterpret_cast<double*>(base + p.part);
  MsWin win;
  {
    double g[MS_WIN], s = 0.0;
    for (int k = 0; k < MS_WIN; ++k) s += g[k] = std::exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5));
    for (int k = 0; k < MS_WIN; ++k) win.g[k] = (float)(g[k] / s);
  }
  MsCombine cmb;
  const double weight[MS_LEVELS] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
  for (int l = 0; l < MS_LEVELS; ++l) {
    const int h = p.h[l], w = p.w[l];
    const unsigned blocks = (unsigned)((int64_t)B * C * p.tx[l] * p.ty[l]);
    const bool last = l == MS_LEVELS - 1;
    float* pa = last ? nullptr : reinterpret_cast<float*>(base + p.plane_a[l + 1]);
    float* pb = last ? nullptr : reinterpret_cast<float*>(base + p.plane_b[l + 1]);
    double* lp = part + p.part_off[l];
    if (l == 0) {
      const MsStride sa{a_strides[0], a_strides[1], a_strides[2]}, sb{b_strides[0], b_strides[1], b_strides[2]};
      hipLaunchKernelGGL(ms_ssim_level_kernel<true>, dim3(blocks), dim3(256), 0, st, a, b, sa, sb, C, h, w, p.tx[l],
                         p.ty[l], pa, pb, lp, win);
    } else {
      const MsStride s{(int64_t)C * h * w, (int64_t)h * w, (int64_t)w};
      hipLaunchKernelGGL(ms_ssim_level_kernel<false>, dim3(blocks), dim3(256), 0, st,
                         reinterpret_cast<const float*>(base + p.plane_a[l]),
                         reinterpret_cast<const float*>(base + p.plane_b[l]), s, s, C, h, w, p.tx[l], p.ty[l], pa, pb,
                         lp, win);
    }
    HIP_OK(hipGetLastError());
    cmb.part_off[l] = p.part_off[l];
    cmb.tiles[l] = p.tx[l] * p.ty[l];
    cmb.count[l] = (double)(h - MS_HALO) * (double)(w - MS_HALO);
    cmb.weight[l] = weight[l];
  }
  hipLaunchKernelGGL(ms_ssim_combine_kernel, dim3(B), dim3(64), 0, st, part, cmb, C,
                     reinterpret_cast<double*>(base + p.terms), terms, out);
  HIP_OK(hipGetLastError());
}

}  // namespace mlic
