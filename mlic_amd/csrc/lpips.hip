// LPIPS-VGG (lpips.LPIPS(net="vgg", version="0.1") in eval mode, restated in DESIGN.md §3) of uint8-valued
// images.  "ReLU on read": every conv stores its pre-activation and each consumer applies the ReLU as it
// loads, so the conv kernels run with a plain epilogue.
//
//   lpips_stem_kernel   uint8 convention, normalize, ScalingLayer and conv1_1 (3 -> 64) in exact fp32 on
//                       the VALU; reads both operands in place through their strides, writes 64 planes
//   conv_x4 (12 layers) the dense 3x3 convs through conv_select / conv_run, weights packed at create time;
//                       the producer's ReLU rides on the operand pack (EPI_RELU_IN)
//   lpips_tap_kernel    one launch per tap: ReLU in registers, the two channel norms, then
//                       sum_c w[c] (fa/(na + eps) - fb/(nb + eps))^2 in a second pass over C (subtract, then
//                       square: identical inputs give exactly 0), pixels reduced to one double per block; for
//                       taps 0-3 also the 2x2 floor max-pool of the ReLU'd planes, the next slice's input
//   lpips_reduce_kernel block partials -> per-image per-tap doubles in a fixed order (no atomics)
//
// The B pairs are processed in chunks of `nb` pairs (reference images, then distorted ones, as one conv batch of
// 2 nb) sized so the scratch stays under LPIPS_SCRATCH_CAP; every kernel is per image, so the result depends
// neither on the batch nor on the chunking.
#include "kernels.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace mlic {

namespace {

constexpr int LP_TAPS = 5, LP_CONVS = 13;
constexpr size_t LPIPS_SCRATCH_CAP = (size_t)4 << 30;  // chunked scratch stays below this while one pair fits
constexpr int64_t LP_MAX_PIXELS = (int64_t)1 << 23;    // per image (3840 x 2176 fits): the size the conv kernels are exercised at
constexpr int LP_FEAT[LP_CONVS] = {0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28};  // vgg16().features indices
constexpr int LP_CIN[LP_CONVS] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
constexpr int LP_COUT[LP_CONVS] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr int LP_TAP_C[LP_TAPS] = {64, 128, 256, 512, 512};
constexpr int LP_TAP_LAST[LP_TAPS] = {1, 3, 6, 9, 12};  // the conv whose ReLU'd output is tap k

struct LpStride {
  int64_t img, ch, row;
};

struct LpStem {
  const float *a, *b;
  LpStride sa, sb;
  int n, H, W;        // n pairs: images 0 .. n-1 of the output are a's, n .. 2n-1 are b's
  const float* w;     // [64][3][3][3]
  const float* bias;  // [64]
  float shift[3], scale[3];
  float* out;  // [2n][64][H][W] pre-activations
};

// one thread per 4 pixels of a row: the 3 x 3 x 6 scaled inputs in registers (0 outside the image: conv1_1
// pads the scaled image), then per output channel four fma chains in weight order; the weight index is
// uniform, so the 27 weights arrive as scalar loads and serve four pixels.  A lane's four outputs leave as one
// 16-byte store where the plane allows (VEC: W % 4 == 0), lane-consecutively either way.
template <bool VEC>
__global__ __launch_bounds__(256) void lpips_stem_kernel(LpStem S) {
  const int img = blockIdx.y;
  const int64_t HW = (int64_t)S.H * S.W;
  const int tw = (S.W + 3) / 4;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)S.H * tw) return;
  const int y = (int)(t / tw), x0 = 4 * (int)(t - (int64_t)y * tw);
  const bool first = img < S.n;
  const LpStride st = first ? S.sa : S.sb;
  const float* src = first ? S.a + (int64_t)img * st.img : S.b + (int64_t)(img - S.n) * st.img;
  float v[3][3][6];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const int yy = y + dy - 1, xx = x0 + j - 1;
        float s = 0.0f;
        if (yy >= 0 && yy < S.H && xx >= 0 && xx < S.W) {
          const float raw = src[(int64_t)c * st.ch + (int64_t)yy * st.row + xx];
          const float u = floorf(fminf(fmaxf(raw, 0.0f), 1.0f) * 255.0f);  // NaN -> 0, as sq_err_u8
          const float tt = 2.0f * (u / 255.0f) - 1.0f;
          s = (tt - S.shift[c]) / S.scale[c];
        }
        v[c][dy][j] = s;
      }
    }
  }
  float* o = S.out + (int64_t)img * 64 * HW + (int64_t)y * S.W + x0;
#pragma unroll 2
  for (int co = 0; co < 64; ++co) {
    const float bias = S.bias[co];
    float acc[4] = {bias, bias, bias, bias};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const float wk = S.w[co * 27 + c * 9 + dy * 3 + dx];
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[j] = fmaf(wk, v[c][dy][j + dx], acc[j]);
        }
      }
    }
    if (VEC) {
      *reinterpret_cast<float4*>(o + (int64_t)co * HW) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x0 + j < S.W) o[(int64_t)co * HW + j] = acc[j];
    }
  }
}

__global__ __launch_bounds__(256) void lpips_relu_kernel(float* __restrict__ x, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const float v = x[i];
    x[i] = v < 0.0f ? 0.0f : v;
  }
}

struct LpTap {
  const float* f;    // [2n][C][h][w] pre-activations: a's images, then b's
  const float* lin;  // [C]
  float* pool;       // [2n][C][h/2][w/2], or null (tap 4)
  double* part;      // [n][nblk]
  int n, C, h, w, nblk;
};

// grid (nblk, n), one wave per block; a lane owns one 2x2 quad of the h x w grid (lanes run along the quad
// row, so a wave reads 128 consecutive floats of each of two rows of every channel plane).  Pass 1: ReLU,
// sum of squares per pixel of both images, pooled maxima written.  Pass 2 (the planes come back from L2):
// the weighted squared difference of the normalised features.  The quad's pixels, the wave's lanes and
// later the blocks are added in a fixed order, in double.  VEC (w even): a quad row is one 8-byte load.
template <bool VEC>
__device__ __forceinline__ void lp_quad(const float* __restrict__ p, const int (&off)[4], const bool (&ok)[4],
                                        float (&v)[4]) {
  if (VEC) {
    const float2 z = make_float2(0.0f, 0.0f);
    const float2 r0 = ok[0] ? *reinterpret_cast<const float2*>(p + off[0]) : z;
    const float2 r1 = ok[2] ? *reinterpret_cast<const float2*>(p + off[2]) : z;
    v[0] = r0.x;
    v[1] = r0.y;
    v[2] = r1.x;
    v[3] = r1.y;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = ok[e] ? p[off[e]] : 0.0f;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = v[e] < 0.0f ? 0.0f : v[e];  // ReLU, NaN kept
}

template <bool VEC>
__global__ __launch_bounds__(64) void lpips_tap_kernel(LpTap T) {
  const int i = blockIdx.y;
  const int qw = (T.w + 1) / 2, qh = (T.h + 1) / 2;
  const int q = blockIdx.x * 64 + threadIdx.x;
  const bool live = q < qh * qw;
  const int qy = live ? q / qw : 0, qx = live ? q - qy * qw : 0;
  const int64_t hw = (int64_t)T.h * T.w;
  const float* fa = T.f + (int64_t)i * T.C * hw;
  const float* fb = T.f + (int64_t)(T.n + i) * T.C * hw;
  int off[4];
  bool ok[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int y = 2 * qy + (e >> 1), x = 2 * qx + (e & 1);
    ok[e] = live && y < T.h && x < T.w;
    off[e] = ok[e] ? y * T.w + x : 0;
  }
  const int ph = T.h / 2, pw = T.w / 2;
  const int64_t phw = (int64_t)ph * pw;
  const bool pooled = T.pool != nullptr && ok[3];  // the whole quad is inside: floor mode drops the rest
  float* pa = pooled ? T.pool + (int64_t)i * T.C * phw + (int64_t)qy * pw + qx : nullptr;
  float* pb = pooled ? T.pool + (int64_t)(T.n + i) * T.C * phw + (int64_t)qy * pw + qx : nullptr;
  double sa[4] = {0.0, 0.0, 0.0, 0.0}, sb[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int c = 0; c < T.C; ++c) {
    float va[4], vb[4];
    lp_quad<VEC>(fa + (int64_t)c * hw, off, ok, va);
    lp_quad<VEC>(fb + (int64_t)c * hw, off, ok, vb);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      sa[e] += (double)va[e] * (double)va[e];
      sb[e] += (double)vb[e] * (double)vb[e];
    }
    if (pooled) {
      pa[(int64_t)c * phw] = fmaxf(fmaxf(va[0], va[1]), fmaxf(va[2], va[3]));
      pb[(int64_t)c * phw] = fmaxf(fmaxf(vb[0], vb[1]), fmaxf(vb[2], vb[3]));
    }
  }
  float ia[4], ib[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    ia[e] = 1.0f / (sqrtf((float)sa[e]) + 1e-10f);
    ib[e] = 1.0f / (sqrtf((float)sb[e]) + 1e-10f);
  }
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int c = 0; c < T.C; ++c) {
    const double wc = (double)T.lin[c];
    float xa[4], xb[4];
    lp_quad<VEC>(fa + (int64_t)c * hw, off, ok, xa);
    lp_quad<VEC>(fb + (int64_t)c * hw, off, ok, xb);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float d = xa[e] * ia[e] - xb[e] * ib[e];
      acc[e] += wc * ((double)d * (double)d);
    }
  }
  double s = 0.0;
#pragma unroll
  for (int e = 0; e < 4; ++e) s += ok[e] ? acc[e] : 0.0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if (threadIdx.x == 0) T.part[(int64_t)i * T.nblk + blockIdx.x] = s;
}

struct LpReduce {
  const double* part[LP_TAPS];  // [n][nblk[k]]
  int nblk[LP_TAPS];
  double count[LP_TAPS];  // pixels of tap k
};

// one wave per image: lane t adds partials t, t + 64, ... in order, the lanes are added by shuffle, the
// five terms in tap order
__global__ __launch_bounds__(64) void lpips_reduce_kernel(LpReduce R, double* __restrict__ out,
                                                          double* __restrict__ terms) {
  const int i = blockIdx.x;
  double total = 0.0;
  for (int k = 0; k < LP_TAPS; ++k) {
    const double* p = R.part[k] + (int64_t)i * R.nblk[k];
    double s = 0.0;
    for (int j = threadIdx.x; j < R.nblk[k]; j += 64) s += p[j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    const double t = s / R.count[k];
    if (threadIdx.x == 0 && terms != nullptr) terms[(int64_t)i * LP_TAPS + k] = t;
    total += t;
  }
  if (threadIdx.x == 0) out[i] = total;
}

size_t align256(size_t v) { return (v + 255) / 256 * 256; }

ConvParams lp_conv_params(int l, int B2, int h, int w) {
  ConvParams P{};
  P.nseg = 1;
  P.seg[0] = {nullptr, LP_CIN[l], (int64_t)LP_CIN[l] * h * w};
  P.Cin = LP_CIN[l];
  P.H = P.Ho = h;
  P.W = P.Wo = w;
  P.Cout = LP_COUT[l];
  P.K = 3;
  P.stride = 1;
  P.pad = 1;
  P.out_cs = (int64_t)h * w;
  P.out_bs = (int64_t)LP_COUT[l] * h * w;
  P.B = B2;
  return P;
}

int lp_conv_tap(int l) {  // the tap (= pooling level) conv l runs at
  int k = 0;
  while (l > LP_TAP_LAST[k]) ++k;
  return k;
}

// scratch of one chunk of nb pairs: X, Y (ping-pong activations, [2 nb][64][H][W] floats each: the largest
// layer), P (pooled planes, [2 nb][64][H/2][W/2]), the conv workspace (x4's packed operand: the largest of
// the 12 layers), the block partials per tap
struct LpPlan {
  int nb;
  int h[LP_TAPS], w[LP_TAPS], nblk[LP_TAPS];
  size_t X, Y, P, ws, ws_bytes, part[LP_TAPS], bytes;
};

LpPlan lp_plan_for(int nb, int H, int W) {
  LpPlan p{};
  p.nb = nb;
  for (int k = 0; k < LP_TAPS; ++k) {
    p.h[k] = k ? p.h[k - 1] / 2 : H;
    p.w[k] = k ? p.w[k - 1] / 2 : W;
    p.nblk[k] = (((p.h[k] + 1) / 2) * ((p.w[k] + 1) / 2) + 63) / 64;
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
  for (int l = 1; l < LP_CONVS; ++l) {
    const int k = lp_conv_tap(l);
    ConvParams P = lp_conv_params(l, 2 * nb, p.h[k], p.w[k]);
    P.epi = EPI_RELU_IN;
    ConvWeights cw{};
    cw.cin_pad = LP_CIN[l];
    p.ws_bytes = std::max(p.ws_bytes, align256((size_t)conv_ws_bytes(CONV_X4, P, cw)));
  }
  off += p.ws_bytes;
  for (int k = 0; k < LP_TAPS; ++k) {
    p.part[k] = off;
    off += align256((size_t)nb * p.nblk[k] * sizeof(double));
  }
  p.bytes = off;
  return p;
}

LpPlan lp_plan(int B, int H, int W) {
  MLIC_CHECK(B >= 1, "lpips: B must be positive");
  MLIC_CHECK(H >= 16 && W >= 16, "lpips: H and W must be at least 16 (tap 4 needs one pixel)");
  MLIC_CHECK((int64_t)H * W <= LP_MAX_PIXELS, "lpips: more than 2^23 pixels per image");
  const size_t one = lp_plan_for(1, H, W).bytes;
  int nb = (int)std::min<size_t>((size_t)B, std::max<size_t>(1, LPIPS_SCRATCH_CAP / one));
  while (nb > 1 && lp_plan_for(nb, H, W).bytes > LPIPS_SCRATCH_CAP) --nb;
  return lp_plan_for(nb, H, W);
}

bool ends_with(const std::string& s, const char* suf) {
  const size_t n = std::strlen(suf);
  return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

}  // namespace

class Lpips {
 public:
  struct Layer {
    float* w = nullptr;  // layer 0: torch layout [64][27]; others: pack_conv [9][Cin][Cout]
    float* bias = nullptr;
    _Float16 *wh = nullptr, *wl = nullptr, *wx4 = nullptr;
    int wexp = 0;
  };
  Layer conv[LP_CONVS];
  float* lin[LP_TAPS] = {};
  float shift[3] = {-0.030f, -0.088f, -0.188f}, scale[3] = {0.458f, 0.448f, 0.450f};
  int* rflag = nullptr;
  int precision = 2;
  int64_t fallbacks = 0;
  std::vector<void*> owned;
  // stage timing (lpips_profile): event pairs around the stem, every dense conv (its ReLU pass and operand
  // pack included) and every tap launch (the reduce with the last), read back once the call has ended
  enum Stage { ST_STEM = 0, ST_CONV = 1, ST_TAP = 2, ST_COUNT = 3 };
  struct Span {
    int stage;
    hipEvent_t e0, e1;
  };
  bool profiling = false;
  double stage_ms[ST_COUNT] = {0.0, 0.0, 0.0};
  std::vector<Span> spans;

  ~Lpips() {
    drop_spans();
    for (void* p : owned) (void)hipFree(p);
  }

  void drop_spans() {
    for (Span& s : spans) {
      (void)hipEventDestroy(s.e0);
      (void)hipEventDestroy(s.e1);
    }
    spans.clear();
  }

  template <class F>
  void timed(int stage, hipStream_t st, F&& f) {
    if (!profiling) return f();
    Span s{stage, nullptr, nullptr};
    HIP_OK(hipEventCreate(&s.e0));
    HIP_OK(hipEventCreate(&s.e1));
    spans.push_back(s);
    HIP_OK(hipEventRecord(s.e0, st));
    f();
    HIP_OK(hipEventRecord(s.e1, st));
  }

  void collect(hipStream_t st) {
    if (spans.empty()) return;
    HIP_OK(hipStreamSynchronize(st));
    for (Span& s : spans) {
      float ms = 0.0f;
      HIP_OK(hipEventElapsedTime(&ms, s.e0, s.e1));
      stage_ms[s.stage] += ms;
    }
    drop_spans();
  }

  template <class T>
  T* alloc(size_t count) {
    void* p = nullptr;
    HIP_OK(hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T)));
    owned.push_back(p);
    return static_cast<T*>(p);
  }

  void load(int n, const char* const* names, const float* const* ptrs, const int64_t* shapes, const int* ndims,
            hipStream_t st) {
    MLIC_CHECK(n >= 0 && (n == 0 || (names && ptrs && shapes && ndims)), "lpips_create: null tensor table");
    const float* cw[LP_CONVS] = {};
    const float* cb[LP_CONVS] = {};
    const float* lw[LP_TAPS] = {};
    const float *sh = nullptr, *sc = nullptr;
    const int64_t* shp = shapes;
    for (int i = 0; i < n; shp += ndims[i], ++i) {
      MLIC_CHECK(names[i] != nullptr, "lpips_create: null tensor name");
      const std::string k = names[i];
      MLIC_CHECK(ptrs[i] != nullptr, "lpips_create: null pointer for tensor " + k);
      auto shape_is = [&](std::initializer_list<int64_t> want) {
        if ((size_t)ndims[i] != want.size()) return false;
        int j = 0;
        for (int64_t d : want)
          if (shp[j++] != d) return false;
        return true;
      };
      if (k.compare(0, 5, "lins.") == 0) continue;  // the package's duplicate of lin{k}
      if (k == "scaling_layer.shift" || k == "scaling_layer.scale") {
        MLIC_CHECK(shape_is({1, 3, 1, 1}), "lpips_create: tensor " + k + " must be [1,3,1,1]");
        (k == "scaling_layer.shift" ? sh : sc) = ptrs[i];
        continue;
      }
      if (k.size() == 19 && k.compare(0, 3, "lin") == 0 && ends_with(k, ".model.1.weight") && k[3] >= '0' &&
          k[3] < '0' + LP_TAPS) {
        const int t = k[3] - '0';
        MLIC_CHECK(shape_is({1, LP_TAP_C[t], 1, 1}),
                   "lpips_create: tensor " + k + " must be [1," + std::to_string(LP_TAP_C[t]) + ",1,1]");
        lw[t] = ptrs[i];
        continue;
      }
      // a conv tensor: "<anything.>IDX.weight|bias", IDX its vgg16().features index
      const bool isw = ends_with(k, ".weight"), isb = ends_with(k, ".bias");
      MLIC_CHECK(isw || isb, "lpips_create: unexpected tensor " + k);
      const std::string stem = k.substr(0, k.size() - (isw ? 7 : 5));
      const size_t dot = stem.rfind('.');
      const std::string idx = dot == std::string::npos ? stem : stem.substr(dot + 1);
      MLIC_CHECK(!idx.empty() && idx.size() <= 2 && idx.find_first_not_of("0123456789") == std::string::npos,
                 "lpips_create: unexpected tensor " + k);
      int l = -1;
      for (int j = 0; j < LP_CONVS; ++j)
        if (LP_FEAT[j] == std::stoi(idx)) l = j;
      MLIC_CHECK(l >= 0, "lpips_create: extra conv tensor " + k + " (no VGG16 conv at that features index)");
      if (isw) {
        MLIC_CHECK(shape_is({LP_COUT[l], LP_CIN[l], 3, 3}), "lpips_create: tensor " + k + " must be [" +
                                                                 std::to_string(LP_COUT[l]) + "," +
                                                                 std::to_string(LP_CIN[l]) + ",3,3]");
        MLIC_CHECK(cw[l] == nullptr, "lpips_create: extra conv tensor " + k + " (given twice)");
        cw[l] = ptrs[i];
      } else {
        MLIC_CHECK(shape_is({LP_COUT[l]}), "lpips_create: tensor " + k + " must be [" + std::to_string(LP_COUT[l]) + "]");
        MLIC_CHECK(cb[l] == nullptr, "lpips_create: extra conv tensor " + k + " (given twice)");
        cb[l] = ptrs[i];
      }
    }
    for (int l = 0; l < LP_CONVS; ++l) {
      MLIC_CHECK(cw[l] != nullptr, "lpips_create: missing tensor " + std::to_string(LP_FEAT[l]) + ".weight");
      MLIC_CHECK(cb[l] != nullptr, "lpips_create: missing tensor " + std::to_string(LP_FEAT[l]) + ".bias");
    }
    for (int t = 0; t < LP_TAPS; ++t)
      MLIC_CHECK(lw[t] != nullptr, "lpips_create: missing tensor lin" + std::to_string(t) + ".model.1.weight");
    MLIC_CHECK((sh == nullptr) == (sc == nullptr), "lpips_create: missing tensor scaling_layer.shift or .scale");

    for (int l = 0; l < LP_CONVS; ++l) {
      Layer& L = conv[l];
      const int Cin = LP_CIN[l], Cout = LP_COUT[l];
      const int64_t nw = (int64_t)Cout * Cin * 9;
      L.w = alloc<float>(nw);
      L.bias = alloc<float>(Cout);
      HIP_OK(hipMemcpyAsync(L.bias, cb[l], sizeof(float) * Cout, hipMemcpyDeviceToDevice, st));
      if (l == 0) {
        HIP_OK(hipMemcpyAsync(L.w, cw[l], sizeof(float) * nw, hipMemcpyDeviceToDevice, st));
        continue;
      }
      const int64_t nh = (int64_t)Cout * 9 * Cin;  // Cin is a multiple of 32: cin_pad = Cin
      L.wh = alloc<_Float16>(nh);
      L.wl = alloc<_Float16>(nh);
      L.wx4 = alloc<_Float16>(x4_weight_halves(Cout, 9, Cin));
      pack_conv(cw[l], L.w, Cout, Cin, 9, st);
      L.wexp = split_weights(cw[l], L.wh, L.wl, Cout, Cin, 9, Cin, true, st);
      x4_pack_weights(L.wh, L.wl, Cout, 9, Cin, L.wx4, st);
    }
    for (int t = 0; t < LP_TAPS; ++t) {
      lin[t] = alloc<float>(LP_TAP_C[t]);
      HIP_OK(hipMemcpyAsync(lin[t], lw[t], sizeof(float) * LP_TAP_C[t], hipMemcpyDeviceToDevice, st));
    }
    if (sh) {
      HIP_OK(hipMemcpyAsync(shift, sh, sizeof(shift), hipMemcpyDeviceToHost, st));
      HIP_OK(hipMemcpyAsync(scale, sc, sizeof(scale), hipMemcpyDeviceToHost, st));
    }
    rflag = alloc<int>(1);
    HIP_OK(hipMemsetAsync(rflag, 0, sizeof(int), st));
    HIP_OK(hipStreamSynchronize(st));  // the caller's tensors may go away
  }

  // conv l on [B2][Cin][h][w] at `in` (a stored pre-activation when relu_in) -> pre-activations at `out`
  void run_conv(int l, float* in, float* out, int B2, int h, int w, bool relu_in, int prec, void* ws,
                hipStream_t st) {
    const Layer& L = conv[l];
    ConvParams P = lp_conv_params(l, B2, h, w);
    P.seg[0].p = in;
    P.wpk = L.w;
    P.bias = L.bias;
    P.out = out;
    P.rflag = rflag;
    P.epi = relu_in && prec != 0 ? EPI_RELU_IN : EPI_NONE;
    ConvWeights cw{L.w, L.wh, L.wl, LP_CIN[l], L.wx4, L.wexp};
    const int impl = conv_select(P, cw, prec);
    MLIC_CHECK(impl == (prec == 0 ? CONV_F32 : CONV_X4),
               "lpips: the dense convs run on conv_x4 (or the fp32 MFMA conv at precision 0); the kernel "
               "options select another family");
    if (relu_in && prec == 0) {  // the fp32 family does not know EPI_RELU_IN
      const int64_t n = (int64_t)B2 * LP_CIN[l] * h * w;
      hipLaunchKernelGGL(lpips_relu_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, in, n);
      HIP_OK(hipGetLastError());
    }
    conv_run(impl, P, cw, st, ws);
  }

  void run_chunk(const LpPlan& p, const float* a, const LpStride& sa, const float* b, const LpStride& sb, int n,
                 int H, int W, char* base, double* out, double* terms, int prec, hipStream_t st) {
    float* X = reinterpret_cast<float*>(base + p.X);
    float* Y = reinterpret_cast<float*>(base + p.Y);
    float* Pl = reinterpret_cast<float*>(base + p.P);
    void* ws = base + p.ws;
    const int B2 = 2 * n;
    {
      LpStem S{};
      S.a = a;
      S.b = b;
      S.sa = sa;
      S.sb = sb;
      S.n = n;
      S.H = H;
      S.W = W;
      S.w = conv[0].w;
      S.bias = conv[0].bias;
      for (int c = 0; c < 3; ++c) {
        S.shift[c] = shift[c];
        S.scale[c] = scale[c];
      }
      S.out = X;
      const int64_t nt = (int64_t)H * ((W + 3) / 4);
      const dim3 grid((unsigned)((nt + 255) / 256), B2);
      timed(ST_STEM, st, [&] {
        if (W % 4 == 0) hipLaunchKernelGGL(lpips_stem_kernel<true>, grid, dim3(256), 0, st, S);
        else hipLaunchKernelGGL(lpips_stem_kernel<false>, grid, dim3(256), 0, st, S);
        HIP_OK(hipGetLastError());
      });
    }
    LpReduce R{};
    float* cur = X;  // holds the pre-activation of the last conv run
    int l = 1;
    for (int k = 0; k < LP_TAPS; ++k) {
      const int h = p.h[k], w = p.w[k];
      bool from_pool = k > 0;  // the slice's first conv reads the pooled (already ReLU'd) planes
      for (; l <= LP_TAP_LAST[k]; ++l) {
        float* in = from_pool ? Pl : cur;
        float* o = from_pool ? X : (cur == X ? Y : X);
        timed(ST_CONV, st, [&] { run_conv(l, in, o, B2, h, w, !from_pool, prec, ws, st); });
        cur = o;
        from_pool = false;
      }
      LpTap T{};
      T.f = cur;
      T.lin = lin[k];
      T.pool = k + 1 < LP_TAPS ? Pl : nullptr;
      T.part = reinterpret_cast<double*>(base + p.part[k]);
      T.n = n;
      T.C = LP_TAP_C[k];
      T.h = h;
      T.w = w;
      T.nblk = p.nblk[k];
      R.part[k] = T.part;
      R.nblk[k] = T.nblk;
      R.count[k] = (double)h * (double)w;
      timed(ST_TAP, st, [&] {
        if (w % 2 == 0) hipLaunchKernelGGL(lpips_tap_kernel<true>, dim3(T.nblk, n), dim3(64), 0, st, T);
        else hipLaunchKernelGGL(lpips_tap_kernel<false>, dim3(T.nblk, n), dim3(64), 0, st, T);
        HIP_OK(hipGetLastError());
        if (k + 1 == LP_TAPS) {
          hipLaunchKernelGGL(lpips_reduce_kernel, dim3(n), dim3(64), 0, st, R, out, terms);
          HIP_OK(hipGetLastError());
        }
      });
    }
  }

  void run(const float* a, const int64_t* as, const float* b, const int64_t* bs, int B, int H, int W, void* scratch,
           double* out, double* terms, hipStream_t st) {
    const LpPlan p = lp_plan(B, H, W);
    const LpStride sa{as[0], as[1], as[2]}, sb{bs[0], bs[1], bs[2]};
    auto pass = [&](int prec) {
      for (int i0 = 0; i0 < B; i0 += p.nb)
        run_chunk(p, a + (int64_t)i0 * sa.img, sa, b + (int64_t)i0 * sb.img, sb, std::min(p.nb, B - i0), H, W,
                  static_cast<char*>(scratch), out + i0, terms ? terms + (int64_t)i0 * LP_TAPS : nullptr, prec, st);
    };
    if (precision == 0) {
      pass(0);
      collect(st);
      return;
    }
    HIP_OK(hipMemsetAsync(rflag, 0, sizeof(int), st));
    pass(precision);
    int hit = 0;
    HIP_OK(hipMemcpyAsync(&hit, rflag, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    if (hit) {  // an operand left fp16's range: the whole call again with the fp32 MFMA convs
      ++fallbacks;
      HIP_OK(hipMemsetAsync(rflag, 0, sizeof(int), st));
      pass(0);
    }
    collect(st);
  }
};

Lpips* lpips_create(int n, const char* const* names, const float* const* ptrs, const int64_t* shapes,
                    const int* ndims, hipStream_t st) {
  Lpips* h = new Lpips();
  try {
    h->load(n, names, ptrs, shapes, ndims, st);
  } catch (...) {
    delete h;
    throw;
  }
  return h;
}

void lpips_destroy(Lpips* h) { delete h; }

void lpips_set_precision(Lpips* h, int precision) {
  MLIC_CHECK(precision == 0 || precision == 2, "lpips: precision must be 2 (split-fp16) or 0 (fp32 MFMA)");
  h->precision = precision;
}

size_t lpips_scratch_bytes(int B, int H, int W) { return lp_plan(B, H, W).bytes; }

void lpips_u8(Lpips* h, const float* a, const int64_t* a_strides, const float* b, const int64_t* b_strides, int B,
              int H, int W, void* scratch, double* out, double* terms, hipStream_t st) {
  h->run(a, a_strides, b, b_strides, B, H, W, scratch, out, terms, st);
}

void lpips_profile(Lpips* h, bool on, double* ms3) {
  for (int i = 0; i < Lpips::ST_COUNT; ++i) {
    if (ms3) ms3[i] = h->stage_ms[i];
    h->stage_ms[i] = 0.0;
  }
  h->profiling = on;
}

int64_t lpips_range_fallbacks(Lpips* h, bool reset) {
  const int64_t v = h->fallbacks;
  if (reset) h->fallbacks = 0;
  return v;
}

}  // namespace mlic
