// DISTS (DISTS_pytorch 0.1's DISTS() in eval mode, restated in DESIGN.md §3) of uint8-valued images, on the
// VGG16 trunk LPIPS uses (vgg_trunk.h): the same thirteen convs with "ReLU on read", L2 pooling in place of the
// max-pools, and a head of per-channel global statistics.
//
//   vgg_stem_kernel     (PRE_DISTS) uint8 convention, (v' - mean) / std and conv1_1 in exact fp32 on the VALU
//   dists_image_kernel  set 0: the moments of the three channels of v' itself, both operands read in place
//   conv_x4 (12 layers) the dense 3x3 convs through VggTrunk::run_conv
//   dists_tap_kernel    one launch per tap: reads a's and b's stored pre-activations once, ReLU in registers,
//                       per (pair, channel, block) the six double moments sum a, sum b, sum a^2, sum b^2,
//                       sum d, sum d^2 with d = a - b; for taps 1-4 also both images' L2-pooled planes
//                       sqrt(conv(x^2, hanning 3x3 / 16, stride 2, pad 1) + 1e-12) on the ceil grid
//   dists_stats_kernel  one wave per (pair, channel) over all six sets: block partials added in a fixed order ->
//                       means, variances, var(d) -> the channel's two weighted contributions
//   dists_reduce_kernel per pair: contributions -> the twelve terms [T1_0, T2_0, .., T1_5, T2_5] -> the value,
//                       in a fixed order (no atomics anywhere)
//
// The difference form: T1 = sum_c (alpha_c / w) (mu_a - mu_b)^2 / (mu_a^2 + mu_b^2 + c1) with mu_a - mu_b = mean(d),
// T2 = sum_c (beta_c / w) var(d) / (var_a + var_b + c2) with var(d) = mean(d^2) - mean(d)^2 = var_a + var_b - 2 cov:
// d is subtracted before anything is squared, so identical operands give d = 0 and every term exactly 0.
// All moments are raw double sums of fp32 values (DESIGN.md §3 bounds their cancellation against c2).
//
// Chunking as LPIPS: `nb` pairs at a time under the same scratch cap; every kernel is per image, so the result
// depends neither on the batch nor on the chunking.
#include "vgg_trunk.h"

namespace mlic {

namespace {

constexpr int DS_SETS = 6, DS_CH = 1475, DS_MOM = 6, DS_TERMS = 12;
constexpr int DS_SET_C[DS_SETS] = {3, 64, 128, 256, 512, 512};
constexpr int DS_SET_OFF[DS_SETS] = {0, 3, 67, 195, 451, 963};
constexpr int DS_STRIP = 8;  // pooled rows (16 plane rows) one thread walks; the row above a strip is read again
constexpr double DS_C1 = 1e-6, DS_C2 = 1e-6;

// block sum of the six moments in a fixed order: lanes by shuffle, then the four waves in wave order
__device__ __forceinline__ void ds_block_store(double (&m)[DS_MOM], double* __restrict__ dst) {
  __shared__ double sh[4][DS_MOM];
#pragma unroll
  for (int j = 0; j < DS_MOM; ++j) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m[j] += __shfl_down(m[j], o, 64);
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < DS_MOM; ++j) sh[wv][j] = m[j];
  }
  __syncthreads();
  const int j = threadIdx.x;
  if (j < DS_MOM) dst[j] = ((sh[0][j] + sh[1][j]) + sh[2][j]) + sh[3][j];
}

__device__ __forceinline__ void ds_count(double (&m)[DS_MOM], float fa, float fb) {
  const double a = (double)fa, b = (double)fb, d = a - b;
  m[0] += a;
  m[1] += b;
  m[2] += a * a;
  m[3] += b * b;
  m[4] += d;
  m[5] += d * d;
}

struct DsImage {
  const float *a, *b;
  LpStride sa, sb;
  int H, W, nblk;
  double* part;  // [n][3][nblk][6]
};

// set 0: grid (nblk, 3, n), a block owns 1024 consecutive pixels of one channel of one pair, a thread four of
// them 256 apart
__global__ __launch_bounds__(256) void dists_image_kernel(DsImage S) {
  const int c = blockIdx.y, i = blockIdx.z;
  const float* pa = S.a + (int64_t)i * S.sa.img + (int64_t)c * S.sa.ch;
  const float* pb = S.b + (int64_t)i * S.sb.img + (int64_t)c * S.sb.ch;
  const int HW = S.H * S.W;
  double m[DS_MOM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int idx = (blockIdx.x * 4 + j) * 256 + threadIdx.x;
    if (idx < HW) {
      const int y = idx / S.W, x = idx - y * S.W;
      const float ra = pa[(int64_t)y * S.sa.row + x], rb = pb[(int64_t)y * S.sb.row + x];
      const float ua = floorf(fminf(fmaxf(ra, 0.0f), 1.0f) * 255.0f);  // NaN -> 0, as sq_err_u8
      const float ub = floorf(fminf(fmaxf(rb, 0.0f), 1.0f) * 255.0f);
      ds_count(m, ua / 255.0f, ub / 255.0f);
    }
  }
  ds_block_store(m, S.part + (((int64_t)i * 3 + c) * S.nblk + blockIdx.x) * DS_MOM);
}

struct DsTap {
  const float* f;  // [2n][C][h][w] pre-activations: a's images, then b's
  float* pool;     // [2n][C][ph][pw] with ph = ceil(h/2), pw = ceil(w/2), or null (tap 5)
  double* part;    // [n][C][nblk][6]
  int n, C, h, w, ph, pw, nblk;
};

// three ReLU'd values of one plane row at columns x0 - 1, x0, x0 + 1 (x0 even); 0 outside the plane.  VEC (w
// even): x0 and x0 + 1 are one 8-byte load.  The left value is the lane below's right one wherever that lane
// holds the quad to the left; a wave's first lane (and the first of a row) loads it.
template <bool VEC>
__device__ __forceinline__ void ds_row(const float* __restrict__ p, int w, int y, bool rowok, int x0, bool live,
                                       bool left_by_shuffle, float (&v)[3]) {
  float c0 = 0.0f, c1 = 0.0f, l = 0.0f;
  const bool ok = live && rowok;
  if (ok) {
    const float* r = p + y * w + x0;
    if (VEC) {
      const float2 t = *reinterpret_cast<const float2*>(r);
      c0 = t.x;
      c1 = t.y;
    } else {
      c0 = r[0];
      if (x0 + 1 < w) c1 = r[1];
    }
    if (!left_by_shuffle && x0 > 0) l = r[-1];
  }
  const float up = __shfl_up(c1, 1, 64);
  if (left_by_shuffle) l = up;
  v[0] = l < 0.0f ? 0.0f : l;  // ReLU, NaN kept
  v[1] = c0 < 0.0f ? 0.0f : c0;
  v[2] = c1 < 0.0f ? 0.0f : c1;
}

// L2 pooling of one window from the squares of its three rows: hanning 3x3 / 16 = corners 1, edges 2, centre 4
// (powers of two, so only the adds round)
__device__ __forceinline__ float ds_l2pool(const float (&up)[3], const float (&mid)[3], const float (&dn)[3]) {
  const float corners = (up[0] + up[2]) + (dn[0] + dn[2]);
  const float edges = (up[1] + dn[1]) + (mid[0] + mid[2]);
  return sqrtf(((corners * 0.0625f + edges * 0.125f) + mid[1] * 0.25f) + 1e-12f);
}

// grid (nblk, C, n), 256 threads.  The ceil(h/2) x ceil(w/2) quads of a plane are cut into strips of DS_STRIP quad
// rows; thread q of the launch's x axis owns column q % pw of strip q / pw and walks it downwards, keeping the
// squares of the last row for the next pooling window.  A quad's up to four pixels are counted by its owner
// only (each pixel once); the window's row above and column to the left are read but not counted.  Every lane
// runs the same DS_STRIP iterations (rows past the plane read as 0 and add 0).
template <bool VEC>
__global__ __launch_bounds__(256) void dists_tap_kernel(DsTap T) {
  const int c = blockIdx.y, i = blockIdx.z;
  const int q = blockIdx.x * 256 + threadIdx.x;
  const int nstrip = (T.ph + DS_STRIP - 1) / DS_STRIP;
  const bool live = q < nstrip * T.pw;
  const int strip = live ? q / T.pw : 0, px = live ? q - strip * T.pw : 0;
  const int x0 = 2 * px, py0 = strip * DS_STRIP;
  const bool left_by_shuffle = live && px > 0 && (threadIdx.x & 63) > 0;
  const int64_t hw = (int64_t)T.h * T.w, phw = (int64_t)T.ph * T.pw;
  const float* fa = T.f + ((int64_t)i * T.C + c) * hw;
  const float* fb = T.f + ((int64_t)(T.n + i) * T.C + c) * hw;
  const bool pooled = T.pool != nullptr;
  float* oa = pooled ? T.pool + ((int64_t)i * T.C + c) * phw : nullptr;
  float* ob = pooled ? T.pool + ((int64_t)(T.n + i) * T.C + c) * phw : nullptr;
  float ua[3] = {0.0f, 0.0f, 0.0f}, ub[3] = {0.0f, 0.0f, 0.0f};  // squares of the row above the window's centre row
  if (pooled) {
    float t[3];
    ds_row<VEC>(fa, T.w, 2 * py0 - 1, py0 > 0, x0, live, left_by_shuffle, t);
#pragma unroll
    for (int e = 0; e < 3; ++e) ua[e] = t[e] * t[e];
    ds_row<VEC>(fb, T.w, 2 * py0 - 1, py0 > 0, x0, live, left_by_shuffle, t);
#pragma unroll
    for (int e = 0; e < 3; ++e) ub[e] = t[e] * t[e];
  }
  double m[DS_MOM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int r = 0; r < DS_STRIP; ++r) {
    const int py = py0 + r, y0 = 2 * py;
    float a0[3], a1[3], b0[3], b1[3];
    ds_row<VEC>(fa, T.w, y0, y0 < T.h, x0, live, left_by_shuffle, a0);
    ds_row<VEC>(fa, T.w, y0 + 1, y0 + 1 < T.h, x0, live, left_by_shuffle, a1);
    ds_row<VEC>(fb, T.w, y0, y0 < T.h, x0, live, left_by_shuffle, b0);
    ds_row<VEC>(fb, T.w, y0 + 1, y0 + 1 < T.h, x0, live, left_by_shuffle, b1);
    ds_count(m, a0[1], b0[1]);
    ds_count(m, a0[2], b0[2]);
    ds_count(m, a1[1], b1[1]);
    ds_count(m, a1[2], b1[2]);
    if (pooled) {
      float sa0[3], sa1[3], sb0[3], sb1[3];
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        sa0[e] = a0[e] * a0[e];
        sa1[e] = a1[e] * a1[e];
        sb0[e] = b0[e] * b0[e];
        sb1[e] = b1[e] * b1[e];
      }
      const float va = ds_l2pool(ua, sa0, sa1), vb = ds_l2pool(ub, sb0, sb1);  // the window's centre is (y0, x0)
      if (live && py < T.ph) {
        oa[py * T.pw + px] = va;
        ob[py * T.pw + px] = vb;
      }
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        ua[e] = sa1[e];
        ub[e] = sb1[e];
      }
    }
  }
  ds_block_store(m, T.part + (((int64_t)i * T.C + c) * T.nblk + blockIdx.x) * DS_MOM);
}

struct DsStats {
  const double* part[DS_SETS];  // [n][C_k][nblk_k][6]
  int nblk[DS_SETS];
  double count[DS_SETS];  // pixels of set k
  const double *aw, *bw;  // [1475] alpha / w, beta / w
  double* contrib;        // [n][1475][2]
};

// grid (ceil(1475 / 4), n), one wave per channel: lane t adds block partials t, t + 64, ... in order, the lanes
// are added by shuffle, lane 0 finishes the channel
__global__ __launch_bounds__(256) void dists_stats_kernel(DsStats S) {
  const int i = blockIdx.y, lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= DS_CH) return;
  int k = 0;
  while (k + 1 < DS_SETS && g >= DS_SET_OFF[k + 1]) ++k;
  const int c = g - DS_SET_OFF[k], nblk = S.nblk[k];
  const double* p = S.part[k] + ((int64_t)i * DS_SET_C[k] + c) * nblk * DS_MOM;
  double m[DS_MOM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int j = lane; j < nblk; j += 64) {
#pragma unroll
    for (int e = 0; e < DS_MOM; ++e) m[e] += p[(int64_t)j * DS_MOM + e];
  }
#pragma unroll
  for (int e = 0; e < DS_MOM; ++e) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m[e] += __shfl_down(m[e], o, 64);
  }
  if (lane == 0) {
    const double N = S.count[k];
    const double mua = m[0] / N, mub = m[1] / N, mud = m[4] / N;
    const double va = m[2] / N - mua * mua, vb = m[3] / N - mub * mub, vd = m[5] / N - mud * mud;
    double* o = S.contrib + ((int64_t)i * DS_CH + g) * 2;
    o[0] = S.aw[g] * ((mud * mud) / (mua * mua + mub * mub + DS_C1));
    o[1] = S.bw[g] * (vd / (va + vb + DS_C2));
  }
}

// one block of twelve waves per pair: wave j sums term j (set j / 2, T1 or T2) over its set's channels, lane t
// the channels t, t + 64, ... in order, lanes by shuffle; thread 0 adds the twelve terms in order
__global__ __launch_bounds__(64 * DS_TERMS) void dists_reduce_kernel(const double* __restrict__ contrib,
                                                                     double* __restrict__ out,
                                                                     double* __restrict__ terms) {
  __shared__ double t[DS_TERMS];
  const int i = blockIdx.x, lane = threadIdx.x & 63, j = threadIdx.x >> 6;
  const int k = j >> 1;
  const double* p = contrib + ((int64_t)i * DS_CH + DS_SET_OFF[k]) * 2 + (j & 1);
  double s = 0.0;
  for (int c = lane; c < DS_SET_C[k]; c += 64) s += p[2 * c];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if (lane == 0) t[j] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = 0.0;
    for (int e = 0; e < DS_TERMS; ++e) {
      total += t[e];
      if (terms != nullptr) terms[(int64_t)i * DS_TERMS + e] = t[e];
    }
    out[i] = total;
  }
}

// scratch of one chunk of nb pairs: X, Y (ping-pong activations, [2 nb][64][H][W] floats each: the largest
// layer), P (pooled planes on the ceil grid, [2 nb][64][ceil(H/2)][ceil(W/2)]: the largest level), the conv
// workspace, the block partials per set, the channel contributions
struct DsPlan {
  int nb;
  int h[LP_TAPS], w[LP_TAPS];  // the grid of tap k + 1 (set k + 1)
  int nblk[DS_SETS];
  size_t X, Y, P, ws, ws_bytes, part[DS_SETS], contrib, bytes;
};

int ds_tap_blocks(int h, int w) {
  const int ph = (h + 1) / 2, pw = (w + 1) / 2;
  return (int)((((int64_t)(ph + DS_STRIP - 1) / DS_STRIP) * pw + 255) / 256);
}

DsPlan ds_plan_for(int nb, int H, int W) {
  DsPlan p{};
  p.nb = nb;
  p.nblk[0] = (int)(((int64_t)H * W + 1023) / 1024);
  for (int k = 0; k < LP_TAPS; ++k) {
    p.h[k] = k ? (p.h[k - 1] + 1) / 2 : H;
    p.w[k] = k ? (p.w[k - 1] + 1) / 2 : W;
    p.nblk[k + 1] = ds_tap_blocks(p.h[k], p.w[k]);
  }
  const size_t act = align256((size_t)2 * nb * 64 * (size_t)H * (size_t)W * sizeof(float));
  size_t off = 0;
  p.X = off;
  off += act;
  p.Y = off;
  off += act;
  p.P = off;
  off += align256((size_t)2 * nb * 64 * (size_t)p.h[1] * (size_t)p.w[1] * sizeof(float));
  p.ws = off;
  p.ws_bytes = lp_conv_ws_bytes(nb, p.h, p.w);
  off += p.ws_bytes;
  for (int k = 0; k < DS_SETS; ++k) {
    p.part[k] = off;
    off += align256((size_t)nb * DS_SET_C[k] * p.nblk[k] * DS_MOM * sizeof(double));
  }
  p.contrib = off;
  off += align256((size_t)nb * DS_CH * 2 * sizeof(double));
  p.bytes = off;
  return p;
}

DsPlan ds_plan(int B, int H, int W) {
  MLIC_CHECK(B >= 1, "dists: B must be positive");
  MLIC_CHECK(H >= 16 && W >= 16, "dists: H and W must be at least 16");
  MLIC_CHECK((int64_t)H * W <= LP_MAX_PIXELS, "dists: more than 2^23 pixels per image");
  const size_t one = ds_plan_for(1, H, W).bytes;
  int nb = (int)std::min<size_t>((size_t)B, std::max<size_t>(1, LPIPS_SCRATCH_CAP / one));
  while (nb > 1 && ds_plan_for(nb, H, W).bytes > LPIPS_SCRATCH_CAP) --nb;
  return ds_plan_for(nb, H, W);
}

}  // namespace

class Dists {
 public:
  VggTrunk trunk{"dists"};
  double *aw = nullptr, *bw = nullptr;  // [1475] alpha / w, beta / w
  float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};

  void load(int n, const char* const* names, const float* const* ptrs, const int64_t* shapes, const int* ndims,
            hipStream_t st) {
    const float *al = nullptr, *be = nullptr, *mn = nullptr, *sd = nullptr;
    trunk.load_convs(
        n, names, ptrs, shapes, ndims,
        [&](int i, const std::string& k, const VggTrunk::ShapeIs& shape_is) {
          if (ends_with(k, ".filter")) return true;  // the package's L2-pooling buffers: the window is fixed here
          if (k == "alpha" || k == "beta") {
            MLIC_CHECK(shape_is({1, DS_CH, 1, 1}), "dists_create: tensor " + k + " must be [1,1475,1,1]");
            (k == "alpha" ? al : be) = ptrs[i];
            return true;
          }
          if (k == "mean" || k == "std") {
            MLIC_CHECK(shape_is({1, 3, 1, 1}), "dists_create: tensor " + k + " must be [1,3,1,1]");
            (k == "mean" ? mn : sd) = ptrs[i];
            return true;
          }
          return false;
        },
        st);
    MLIC_CHECK(al != nullptr, "dists_create: missing tensor alpha");
    MLIC_CHECK(be != nullptr, "dists_create: missing tensor beta");
    MLIC_CHECK((mn == nullptr) == (sd == nullptr), std::string("dists_create: missing tensor ") + (mn ? "std" : "mean"));
    std::vector<float> ha(DS_CH), hb(DS_CH);
    HIP_OK(hipMemcpyAsync(ha.data(), al, sizeof(float) * DS_CH, hipMemcpyDeviceToHost, st));
    HIP_OK(hipMemcpyAsync(hb.data(), be, sizeof(float) * DS_CH, hipMemcpyDeviceToHost, st));
    if (mn) {
      HIP_OK(hipMemcpyAsync(mean, mn, sizeof(mean), hipMemcpyDeviceToHost, st));
      HIP_OK(hipMemcpyAsync(stdv, sd, sizeof(stdv), hipMemcpyDeviceToHost, st));
    }
    HIP_OK(hipStreamSynchronize(st));  // the caller's tensors may go away
    double wa = 0.0, wb = 0.0;
    for (int c = 0; c < DS_CH; ++c) wa += (double)ha[c];
    for (int c = 0; c < DS_CH; ++c) wb += (double)hb[c];
    const double w = wa + wb;
    MLIC_CHECK(std::isfinite(w) && w != 0.0, "dists_create: the sum of tensors alpha and beta must be finite and nonzero");
    std::vector<double> da(DS_CH), db(DS_CH);
    for (int c = 0; c < DS_CH; ++c) {
      da[c] = (double)ha[c] / w;
      db[c] = (double)hb[c] / w;
    }
    aw = trunk.alloc<double>(DS_CH);
    bw = trunk.alloc<double>(DS_CH);
    HIP_OK(hipMemcpyAsync(aw, da.data(), sizeof(double) * DS_CH, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(bw, db.data(), sizeof(double) * DS_CH, hipMemcpyHostToDevice, st));
    HIP_OK(hipStreamSynchronize(st));
  }

  void run_chunk(const DsPlan& p, const float* a, const LpStride& sa, const float* b, const LpStride& sb, int n,
                 int H, int W, char* base, double* out, double* terms, int prec, hipStream_t st) {
    float* X = reinterpret_cast<float*>(base + p.X);
    float* Y = reinterpret_cast<float*>(base + p.Y);
    float* Pl = reinterpret_cast<float*>(base + p.P);
    void* ws = base + p.ws;
    const int B2 = 2 * n;
    DsStats R{};
    for (int k = 0; k < DS_SETS; ++k) {
      R.part[k] = reinterpret_cast<double*>(base + p.part[k]);
      R.nblk[k] = p.nblk[k];
      R.count[k] = k ? (double)p.h[k - 1] * (double)p.w[k - 1] : (double)H * (double)W;
    }
    R.aw = aw;
    R.bw = bw;
    R.contrib = reinterpret_cast<double*>(base + p.contrib);
    trunk.run_stem<PRE_DISTS>(a, sa, b, sb, n, H, W, mean, stdv, X, st);
    trunk.timed(VggTrunk::ST_TAP, st, [&] {
      DsImage S{a, b, sa, sb, H, W, p.nblk[0], reinterpret_cast<double*>(base + p.part[0])};
      hipLaunchKernelGGL(dists_image_kernel, dim3(p.nblk[0], 3, n), dim3(256), 0, st, S);
      HIP_OK(hipGetLastError());
    });
    float* cur = X;  // holds the pre-activation of the last conv run
    int l = 1;
    for (int k = 0; k < LP_TAPS; ++k) {
      const int h = p.h[k], w = p.w[k];
      bool from_pool = k > 0;  // the stage's first conv reads the L2-pooled (non-negative) planes
      for (; l <= LP_TAP_LAST[k]; ++l) {
        float* in = from_pool ? Pl : cur;
        float* o = from_pool ? X : (cur == X ? Y : X);
        trunk.timed(VggTrunk::ST_CONV, st, [&] { trunk.run_conv(l, in, o, B2, h, w, !from_pool, prec, ws, st); });
        cur = o;
        from_pool = false;
      }
      DsTap T{};
      T.f = cur;
      T.pool = k + 1 < LP_TAPS ? Pl : nullptr;
      T.part = reinterpret_cast<double*>(base + p.part[k + 1]);
      T.n = n;
      T.C = LP_TAP_C[k];
      T.h = h;
      T.w = w;
      T.ph = (h + 1) / 2;
      T.pw = (w + 1) / 2;
      T.nblk = p.nblk[k + 1];
      trunk.timed(VggTrunk::ST_TAP, st, [&] {
        const dim3 grid(T.nblk, T.C, n);
        if (w % 2 == 0) hipLaunchKernelGGL(dists_tap_kernel<true>, grid, dim3(256), 0, st, T);
        else hipLaunchKernelGGL(dists_tap_kernel<false>, grid, dim3(256), 0, st, T);
        HIP_OK(hipGetLastError());
        if (k + 1 == LP_TAPS) {
          hipLaunchKernelGGL(dists_stats_kernel, dim3((DS_CH + 3) / 4, n), dim3(256), 0, st, R);
          HIP_OK(hipGetLastError());
          hipLaunchKernelGGL(dists_reduce_kernel, dim3(n), dim3(64 * DS_TERMS), 0, st, R.contrib, out, terms);
          HIP_OK(hipGetLastError());
        }
      });
    }
  }

  void run(const float* a, const int64_t* as, const float* b, const int64_t* bs, int B, int H, int W, void* scratch,
           double* out, double* terms, hipStream_t st) {
    const DsPlan p = ds_plan(B, H, W);
    const LpStride sa{as[0], as[1], as[2]}, sb{bs[0], bs[1], bs[2]};
    trunk.run_guarded(st, [&](int prec) {
      for (int i0 = 0; i0 < B; i0 += p.nb)
        run_chunk(p, a + (int64_t)i0 * sa.img, sa, b + (int64_t)i0 * sb.img, sb, std::min(p.nb, B - i0), H, W,
                  static_cast<char*>(scratch), out + i0, terms ? terms + (int64_t)i0 * DS_TERMS : nullptr, prec, st);
    });
  }
};

Dists* dists_create(int n, const char* const* names, const float* const* ptrs, const int64_t* shapes,
                    const int* ndims, hipStream_t st) {
  Dists* h = new Dists();
  try {
    h->load(n, names, ptrs, shapes, ndims, st);
  } catch (...) {
    delete h;
    throw;
  }
  return h;
}

void dists_destroy(Dists* h) { delete h; }

void dists_set_precision(Dists* h, int precision) { h->trunk.set_precision(precision); }

size_t dists_scratch_bytes(int B, int H, int W) { return ds_plan(B, H, W).bytes; }

void dists_u8(Dists* h, const float* a, const int64_t* a_strides, const float* b, const int64_t* b_strides, int B,
              int H, int W, void* scratch, double* out, double* terms, hipStream_t st) {
  h->run(a, a_strides, b, b_strides, B, H, W, scratch, out, terms, st);
}

void dists_profile(Dists* h, bool on, double* ms3) { h->trunk.profile(on, ms3); }

int64_t dists_range_fallbacks(Dists* h, bool reset) { return h->trunk.range_fallbacks(reset); }

}  // namespace mlic
