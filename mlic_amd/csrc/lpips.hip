// LPIPS-VGG (lpips.LPIPS(net="vgg", version="0.1") in eval mode, restated in DESIGN.md §3) of uint8-valued
// images.  "ReLU on read": every conv stores its pre-activation and each consumer applies the ReLU as it
// loads, so the conv kernels run with a plain epilogue.
//
//   vgg_stem_kernel     (vgg_trunk.h, PRE_LPIPS) uint8 convention, normalize, ScalingLayer and conv1_1
//                       (3 -> 64) in exact fp32 on the VALU; reads both operands in place through their
//                       strides, writes 64 planes
//   conv_x4 (12 layers) the dense 3x3 convs through VggTrunk::run_conv, weights packed at create time;
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
#include "vgg_trunk.h"

namespace mlic {

namespace {

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
  p.ws_bytes = lp_conv_ws_bytes(nb, p.h, p.w);
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

}  // namespace

class Lpips {
 public:
  VggTrunk trunk{"lpips"};
  float* lin[LP_TAPS] = {};
  float shift[3] = {-0.030f, -0.088f, -0.188f}, scale[3] = {0.458f, 0.448f, 0.450f};

  void load(int n, const char* const* names, const float* const* ptrs, const int64_t* shapes, const int* ndims,
            hipStream_t st) {
    const float* lw[LP_TAPS] = {};
    const float *sh = nullptr, *sc = nullptr;
    trunk.load_convs(
        n, names, ptrs, shapes, ndims,
        [&](int i, const std::string& k, const VggTrunk::ShapeIs& shape_is) {
          if (k.compare(0, 5, "lins.") == 0) return true;  // the package's duplicate of lin{k}
          if (k == "scaling_layer.shift" || k == "scaling_layer.scale") {
            MLIC_CHECK(shape_is({1, 3, 1, 1}), "lpips_create: tensor " + k + " must be [1,3,1,1]");
            (k == "scaling_layer.shift" ? sh : sc) = ptrs[i];
            return true;
          }
          if (k.size() == 19 && k.compare(0, 3, "lin") == 0 && ends_with(k, ".model.1.weight") && k[3] >= '0' &&
              k[3] < '0' + LP_TAPS) {
            const int t = k[3] - '0';
            MLIC_CHECK(shape_is({1, LP_TAP_C[t], 1, 1}),
                       "lpips_create: tensor " + k + " must be [1," + std::to_string(LP_TAP_C[t]) + ",1,1]");
            lw[t] = ptrs[i];
            return true;
          }
          return false;
        },
        st);
    for (int t = 0; t < LP_TAPS; ++t)
      MLIC_CHECK(lw[t] != nullptr, "lpips_create: missing tensor lin" + std::to_string(t) + ".model.1.weight");
    MLIC_CHECK((sh == nullptr) == (sc == nullptr), "lpips_create: missing tensor scaling_layer.shift or .scale");
    for (int t = 0; t < LP_TAPS; ++t) {
      lin[t] = trunk.alloc<float>(LP_TAP_C[t]);
      HIP_OK(hipMemcpyAsync(lin[t], lw[t], sizeof(float) * LP_TAP_C[t], hipMemcpyDeviceToDevice, st));
    }
    if (sh) {
      HIP_OK(hipMemcpyAsync(shift, sh, sizeof(shift), hipMemcpyDeviceToHost, st));
      HIP_OK(hipMemcpyAsync(scale, sc, sizeof(scale), hipMemcpyDeviceToHost, st));
    }
    HIP_OK(hipStreamSynchronize(st));  // the caller's tensors may go away
  }

  void run_chunk(const LpPlan& p, const float* a, const LpStride& sa, const float* b, const LpStride& sb, int n,
                 int H, int W, char* base, double* out, double* terms, int prec, hipStream_t st) {
    float* X = reinterpret_cast<float*>(base + p.X);
    float* Y = reinterpret_cast<float*>(base + p.Y);
    float* Pl = reinterpret_cast<float*>(base + p.P);
    void* ws = base + p.ws;
    const int B2 = 2 * n;
    trunk.run_stem<PRE_LPIPS>(a, sa, b, sb, n, H, W, shift, scale, X, st);
    LpReduce R{};
    float* cur = X;  // holds the pre-activation of the last conv run
    int l = 1;
    for (int k = 0; k < LP_TAPS; ++k) {
      const int h = p.h[k], w = p.w[k];
      bool from_pool = k > 0;  // the slice's first conv reads the pooled (already ReLU'd) planes
      for (; l <= LP_TAP_LAST[k]; ++l) {
        float* in = from_pool ? Pl : cur;
        float* o = from_pool ? X : (cur == X ? Y : X);
        trunk.timed(VggTrunk::ST_CONV, st, [&] { trunk.run_conv(l, in, o, B2, h, w, !from_pool, prec, ws, st); });
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
      trunk.timed(VggTrunk::ST_TAP, st, [&] {
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
    // an operand left fp16's range: the whole call again with the fp32 MFMA convs
    trunk.run_guarded(st, [&](int prec) {
      for (int i0 = 0; i0 < B; i0 += p.nb)
        run_chunk(p, a + (int64_t)i0 * sa.img, sa, b + (int64_t)i0 * sb.img, sb, std::min(p.nb, B - i0), H, W,
                  static_cast<char*>(scratch), out + i0, terms ? terms + (int64_t)i0 * LP_TAPS : nullptr, prec, st);
    });
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

void lpips_set_precision(Lpips* h, int precision) { h->trunk.set_precision(precision); }

size_t lpips_scratch_bytes(int B, int H, int W) { return lp_plan(B, H, W).bytes; }

void lpips_u8(Lpips* h, const float* a, const int64_t* a_strides, const float* b, const int64_t* b_strides, int B,
              int H, int W, void* scratch, double* out, double* terms, hipStream_t st) {
  h->run(a, a_strides, b, b_strides, B, H, W, scratch, out, terms, st);
}

void lpips_profile(Lpips* h, bool on, double* ms3) { h->trunk.profile(on, ms3); }

int64_t lpips_range_fallbacks(Lpips* h, bool reset) { return h->trunk.range_fallbacks(reset); }

}  // namespace mlic
