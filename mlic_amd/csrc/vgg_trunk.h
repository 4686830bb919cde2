// The VGG16 trunk LPIPS (lpips.hip) and DISTS (dists.hip) share: the thirteen 3x3 convs of vgg16().features up to
// conv5_3, "ReLU on read" (every conv stores its pre-activation and each consumer applies the ReLU as it loads).
//
//   vgg_stem_kernel   uint8 convention, the metric's input affine and conv1_1 (3 -> 64) in exact fp32 on the
//                     VALU; reads both operands in place through their strides, writes 64 planes
//   VggTrunk          the conv tensors of a weight table (matched by their features index), weights packed at
//                     create time, run_conv (conv_x4, or the fp32 MFMA conv at precision 0), the fp16 range flag
//                     with the whole-call fp32 re-run, the stage timers
//
// Included by the two metric translation units only; everything here has internal linkage.
#pragma once
#include "kernels.h"

#include <cmath>
#include <cstring>
#include <functional>
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

// the input affine in front of conv1_1: LPIPS scores t = 2 v' - 1 through its ScalingLayer, DISTS v' itself
enum { PRE_LPIPS = 0, PRE_DISTS = 1 };

// one thread per 4 pixels of a row: the 3 x 3 x 6 scaled inputs in registers (0 outside the image: conv1_1
// pads the scaled image), then per output channel four fma chains in weight order; the weight index is
// uniform, so the 27 weights arrive as scalar loads and serve four pixels.  A lane's four outputs leave as one
// 16-byte store where the plane allows (VEC: W % 4 == 0), lane-consecutively either way.
template <bool VEC, int PRE>
__global__ __launch_bounds__(256) void vgg_stem_kernel(LpStem S) {
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
          const float tt = PRE == PRE_LPIPS ? 2.0f * (u / 255.0f) - 1.0f : u / 255.0f;
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

__global__ __launch_bounds__(256) void vgg_relu_kernel(float* __restrict__ x, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const float v = x[i];
    x[i] = v < 0.0f ? 0.0f : v;
  }
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

// the x4 workspace the twelve dense convs need on the grids h[k] x w[k] (the packed operand of the largest layer)
size_t lp_conv_ws_bytes(int nb, const int* h, const int* w) {
  size_t bytes = 0;
  for (int l = 1; l < LP_CONVS; ++l) {
    const int k = lp_conv_tap(l);
    ConvParams P = lp_conv_params(l, 2 * nb, h[k], w[k]);
    P.epi = EPI_RELU_IN;
    ConvWeights cw{};
    cw.cin_pad = LP_CIN[l];
    bytes = std::max(bytes, align256((size_t)conv_ws_bytes(CONV_X4, P, cw)));
  }
  return bytes;
}

bool ends_with(const std::string& s, const char* suf) {
  const size_t n = std::strlen(suf);
  return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
}

class VggTrunk {
 public:
  struct Layer {
    float* w = nullptr;  // layer 0: torch layout [64][27]; others: pack_conv [9][Cin][Cout]
    float* bias = nullptr;
    _Float16 *wh = nullptr, *wl = nullptr, *wx4 = nullptr;
    int wexp = 0;
  };
  const std::string who;  // "lpips" or "dists": the prefix of every message
  Layer conv[LP_CONVS];
  int* rflag = nullptr;
  int precision = 2;
  int64_t fallbacks = 0;
  std::vector<void*> owned;
  // stage timing (*_profile): event pairs around the stem, every dense conv (its ReLU pass and operand pack
  // included) and every tap launch (the reduce with the last), read back once the call has ended
  enum Stage { ST_STEM = 0, ST_CONV = 1, ST_TAP = 2, ST_COUNT = 3 };
  struct Span {
    int stage;
    hipEvent_t e0, e1;
  };
  bool profiling = false;
  double stage_ms[ST_COUNT] = {0.0, 0.0, 0.0};
  std::vector<Span> spans;

  explicit VggTrunk(const char* name) : who(name) {}
  VggTrunk(const VggTrunk&) = delete;
  VggTrunk& operator=(const VggTrunk&) = delete;

  ~VggTrunk() {
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

  void profile(bool on, double* ms3) {
    for (int i = 0; i < ST_COUNT; ++i) {
      if (ms3) ms3[i] = stage_ms[i];
      stage_ms[i] = 0.0;
    }
    profiling = on;
  }

  void set_precision(int p) {
    MLIC_CHECK(p == 0 || p == 2, who + ": precision must be 2 (split-fp16) or 0 (fp32 MFMA)");
    precision = p;
  }

  int64_t range_fallbacks(bool reset) {
    const int64_t v = fallbacks;
    if (reset) fallbacks = 0;
    return v;
  }

  template <class T>
  T* alloc(size_t count) {
    void* p = nullptr;
    HIP_OK(hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T)));
    owned.push_back(p);
    return static_cast<T*>(p);
  }

  // One pass over the tensor table.  head(i, name, shape_is) claims the metric's own tensors (true = taken, or it
  // throws); every other tensor must be a conv tensor "<anything.>IDX.weight|bias", IDX its vgg16().features
  // index.  All thirteen convs must be there; they are packed and the range flag is made.  The caller waits for
  // the stream before its tensors go away.
  using ShapeIs = std::function<bool(std::initializer_list<int64_t>)>;
  void load_convs(int n, const char* const* names, const float* const* ptrs, const int64_t* shapes, const int* ndims,
                  const std::function<bool(int, const std::string&, const ShapeIs&)>& head, hipStream_t st) {
    const std::string pre = who + "_create: ";
    MLIC_CHECK(n >= 0 && (n == 0 || (names && ptrs && shapes && ndims)), pre + "null tensor table");
    const float* cw[LP_CONVS] = {};
    const float* cb[LP_CONVS] = {};
    const int64_t* shp = shapes;
    for (int i = 0; i < n; shp += ndims[i], ++i) {
      MLIC_CHECK(names[i] != nullptr, pre + "null tensor name");
      const std::string k = names[i];
      MLIC_CHECK(ptrs[i] != nullptr, pre + "null pointer for tensor " + k);
      const ShapeIs shape_is = [&](std::initializer_list<int64_t> want) {
        if ((size_t)ndims[i] != want.size()) return false;
        int j = 0;
        for (int64_t d : want)
          if (shp[j++] != d) return false;
        return true;
      };
      if (head(i, k, shape_is)) continue;
      const bool isw = ends_with(k, ".weight"), isb = ends_with(k, ".bias");
      MLIC_CHECK(isw || isb, pre + "unexpected tensor " + k);
      const std::string stem = k.substr(0, k.size() - (isw ? 7 : 5));
      const size_t dot = stem.rfind('.');
      const std::string idx = dot == std::string::npos ? stem : stem.substr(dot + 1);
      MLIC_CHECK(!idx.empty() && idx.size() <= 2 && idx.find_first_not_of("0123456789") == std::string::npos,
                 pre + "unexpected tensor " + k);
      int l = -1;
      for (int j = 0; j < LP_CONVS; ++j)
        if (LP_FEAT[j] == std::stoi(idx)) l = j;
      MLIC_CHECK(l >= 0, pre + "extra conv tensor " + k + " (no VGG16 conv at that features index)");
      if (isw) {
        MLIC_CHECK(shape_is({LP_COUT[l], LP_CIN[l], 3, 3}), pre + "tensor " + k + " must be [" +
                                                                 std::to_string(LP_COUT[l]) + "," +
                                                                 std::to_string(LP_CIN[l]) + ",3,3]");
        MLIC_CHECK(cw[l] == nullptr, pre + "extra conv tensor " + k + " (given twice)");
        cw[l] = ptrs[i];
      } else {
        MLIC_CHECK(shape_is({LP_COUT[l]}), pre + "tensor " + k + " must be [" + std::to_string(LP_COUT[l]) + "]");
        MLIC_CHECK(cb[l] == nullptr, pre + "extra conv tensor " + k + " (given twice)");
        cb[l] = ptrs[i];
      }
    }
    for (int l = 0; l < LP_CONVS; ++l) {
      MLIC_CHECK(cw[l] != nullptr, pre + "missing tensor " + std::to_string(LP_FEAT[l]) + ".weight");
      MLIC_CHECK(cb[l] != nullptr, pre + "missing tensor " + std::to_string(LP_FEAT[l]) + ".bias");
    }
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
    rflag = alloc<int>(1);
    HIP_OK(hipMemsetAsync(rflag, 0, sizeof(int), st));
  }

  // conv1_1 with the metric's input affine on n pairs -> [2n][64][H][W] pre-activations at `out`
  template <int PRE>
  void run_stem(const float* a, const LpStride& sa, const float* b, const LpStride& sb, int n, int H, int W,
                const float* shift, const float* scale, float* out, hipStream_t st) {
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
    S.out = out;
    const int64_t nt = (int64_t)H * ((W + 3) / 4);
    const dim3 grid((unsigned)((nt + 255) / 256), 2 * n);
    timed(ST_STEM, st, [&] {
      if (W % 4 == 0) hipLaunchKernelGGL((vgg_stem_kernel<true, PRE>), grid, dim3(256), 0, st, S);
      else hipLaunchKernelGGL((vgg_stem_kernel<false, PRE>), grid, dim3(256), 0, st, S);
      HIP_OK(hipGetLastError());
    });
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
               who + ": the dense convs run on conv_x4 (or the fp32 MFMA conv at precision 0); the kernel "
                     "options select another family");
    if (relu_in && prec == 0) {  // the fp32 family does not know EPI_RELU_IN
      const int64_t n = (int64_t)B2 * LP_CIN[l] * h * w;
      hipLaunchKernelGGL(vgg_relu_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, in, n);
      HIP_OK(hipGetLastError());
    }
    conv_run(impl, P, cw, st, ws);
  }

  // pass(prec) runs the whole call; at precision 2 the range flag is read once and, when an operand left fp16's
  // range, the whole call runs again with the fp32 MFMA convs and is counted
  template <class F>
  void run_guarded(hipStream_t st, F&& pass) {
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
    if (hit) {
      ++fallbacks;
      HIP_OK(hipMemsetAsync(rflag, 0, sizeof(int), st));
      pass(0);
    }
    collect(st);
  }
};

}  // namespace

}  // namespace mlic
