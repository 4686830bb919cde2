// C ABI of libmlic_hip.so (include/mlic_hip.h): status codes, thread-local error text.
#include "../../include/mlic_hip.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "container.h"
#include "model.h"
#include "options.h"
#include "resample_table.h"
#include "residual.h"
#include "residual16.h"
#include "residual_seg.h"
#include "residual_yuv.h"

using namespace mlic;

struct mlic_model {
  Model* impl;
  // mlic_encode_image_u8 / mlic_decode_image_u8: the padded fp32 image [3][Hp][Wp] between the uint8 kernels and
  // the model (grows on demand), and the header fields of the last encode
  float* stage = nullptr;
  size_t stage_bytes = 0;
  // mlic_encode_image_u8_budget: the other half of the filter's ping-pong (grows likewise)
  float* stage2 = nullptr;
  size_t stage2_bytes = 0;
  int enc_H = 0, enc_W = 0, enc_level = -1;  // enc_H == 0: nothing encoded yet
  int enc_passes = 0;                        // filter passes of the last encode
  // mlic_encode_image_u8_scaled: the display size and filter of the last encode when it was a scaled one (enc_H,
  // enc_W are then the coded size); sc_H == 0: it was not
  int sc_H = 0, sc_W = 0, sc_filter = 0;
};

struct mlic_lpips {
  Lpips* impl = nullptr;
};

struct mlic_dists {
  Dists* impl = nullptr;
};

static thread_local std::string g_err;

template <class F>
static int guard(F&& f) {
  try {
    OptionScope scope;  // the whole entry runs under one snapshot of the kernel options
    f();
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
  } catch (...) {
    g_err = "mlic: unknown error";
  }
  return 1;
}

// Every entry point that takes a handle goes through here: a null handle is an error, not a crash.
static Model& impl(mlic_model* m) {
  MLIC_CHECK(m != nullptr && m->impl != nullptr, "null mlic_model handle");
  return *m->impl;
}

static CdfTables make_tables(const int32_t* cdf, const int32_t* len, const int32_t* off, int n, int stride) {
  CdfTables t;
  t.n = n;
  t.stride = stride;
  t.cdf.assign(cdf, cdf + (size_t)n * stride);
  t.length.assign(len, len + n);
  t.offset.assign(off, off + n);
  for (int i = 0; i < n; ++i)
    MLIC_CHECK(t.length[i] >= 3 && t.length[i] <= stride, "cdf length out of range");
  t.prepare();
  return t;
}

extern "C" {

const char* mlic_last_error(void) { return g_err.c_str(); }
const char* mlic_version(void) { return "mlic_hip 0.1 gfx950"; }

int mlic_create(const char* model_name, int n, const char* const* names, const float* const* ptrs,
                const int64_t* shapes, const int* ndims, void* stream, mlic_model** out) {
  return guard([&] {
    MLIC_CHECK(out != nullptr, "null out");
    auto* m = new mlic_model();
    m->impl = nullptr;
    try {
      m->impl = new Model(model_name, n, names, ptrs, shapes, ndims, (hipStream_t)stream);
      if (opt_str(OPT_LANES)) m->impl->set_lanes(opt(OPT_LANES));
      if (opt_str(OPT_PRECISION)) m->impl->set_precision(opt(OPT_PRECISION));
      if (opt_str(OPT_SYNTH_FP16)) m->impl->set_synthesis_precision(opt(OPT_SYNTH_FP16));
      if (opt_str(OPT_POISON)) m->impl->set_poison(opt(OPT_POISON) != 0);
    } catch (...) {
      delete m;
      throw;
    }
    *out = m;
  });
}

int mlic_destroy(mlic_model* m) {
  return guard([&] {
    if (!m) return;
    delete m->impl;
    if (m->stage) (void)hipFree(m->stage);
    if (m->stage2) (void)hipFree(m->stage2);
    delete m;
  });
}

int mlic_forward(mlic_model* m, void* stream, const float* x, int B, int H, int W, float* x_hat, float* y_lik,
                 float* z_lik, float vbr_scale) {
  return guard([&] {
    MLIC_CHECK(m && x && B > 0, "bad arguments");
    const std::vector<float> sc(B, vbr_scale);
    impl(m).forward(x, B, H, W, x_hat, y_lik, z_lik, sc.data(), (hipStream_t)stream);
  });
}

int mlic_forward_v(mlic_model* m, void* stream, const float* x, int B, int H, int W, float* x_hat, float* y_lik,
                   float* z_lik, const float* vbr_scales) {
  return guard([&] {
    MLIC_CHECK(m && x && B > 0, "bad arguments");
    impl(m).forward(x, B, H, W, x_hat, y_lik, z_lik, vbr_scales, (hipStream_t)stream);
  });
}

int mlic_set_entropy_tables(mlic_model* m, const int32_t* gc_cdf, const int32_t* gc_len, const int32_t* gc_off,
                            int gc_n, int gc_stride, const int32_t* eb_cdf, const int32_t* eb_len,
                            const int32_t* eb_off, int eb_n, int eb_stride) {
  return guard([&] {
    MLIC_CHECK(m, "null model");
    impl(m).set_tables(make_tables(gc_cdf, gc_len, gc_off, gc_n, gc_stride),
                        make_tables(eb_cdf, eb_len, eb_off, eb_n, eb_stride));
  });
}

int mlic_compress(mlic_model* m, void* stream, const float* x, int B, int H, int W, float vbr_scale) {
  return guard([&] {
    MLIC_CHECK(m && x && B > 0, "bad arguments");
    const std::vector<float> sc(B, vbr_scale);
    impl(m).compress(x, B, H, W, sc.data(), (hipStream_t)stream);
  });
}

int mlic_compress_v(mlic_model* m, void* stream, const float* x, int B, int H, int W, const float* vbr_scales) {
  return guard([&] {
    MLIC_CHECK(m && x && B > 0, "bad arguments");
    impl(m).compress(x, B, H, W, vbr_scales, (hipStream_t)stream);
  });
}

int mlic_encoded_size(mlic_model* m, int b, size_t* y_len, size_t* z_len) {
  return guard([&] {
    const EncodedImage& e = impl(m).encoded(b);
    *y_len = e.y.size();
    *z_len = e.z.size();
  });
}

int mlic_encoded_copy(mlic_model* m, int b, uint8_t* y, uint8_t* z) {
  return guard([&] {
    const EncodedImage& e = impl(m).encoded(b);
    std::memcpy(y, e.y.data(), e.y.size());
    std::memcpy(z, e.z.data(), e.z.size());
  });
}

int mlic_encoded_streams(mlic_model* m, int b, int64_t* n_y, int64_t* n_z, int32_t* y_sym, int32_t* y_idx,
                         int32_t* z_sym) {
  return guard([&] {
    const EncodedImage& e = impl(m).encoded(b);
    *n_y = e.y_in.size();
    *n_z = (int64_t)e.z_sym.size();
    e.y_in.gather(y_sym, y_idx);
    if (z_sym) std::memcpy(z_sym, e.z_sym.data(), e.z_sym.size() * 4);
  });
}

int mlic_encoded_bits(mlic_model* m, int b, double* y_bits, double* z_bits) {
  return guard([&] {
    const EncodedImage& e = impl(m).encoded(b);
    if (y_bits) *y_bits = e.y_bits;
    if (z_bits) *z_bits = e.z_bits;
  });
}


int mlic_decompress_v(mlic_model* m, void* stream, const uint8_t* const* y, const size_t* y_len,
                      const uint8_t* const* z, const size_t* z_len, int B, int hz, int wz, float* x_hat,
                      const float* vbr_scales) {
  return guard([&] {
    MLIC_CHECK(m && y && z && x_hat && B > 0 && hz > 0 && wz > 0, "bad arguments");
    impl(m).decompress(y, y_len, z, z_len, B, hz, wz, x_hat, vbr_scales, (hipStream_t)stream);
  });
}

int mlic_batch_stream(mlic_model* m, int first, int count, uint8_t* out, size_t cap, size_t* len) {
  return guard([&] {
    MLIC_CHECK(m && len, "bad arguments");
    const std::string s = impl(m).batch_stream(first, count);
    *len = s.size();
    if (out) {
      MLIC_CHECK(cap >= s.size(), "batch_stream: buffer too small");
      std::memcpy(out, s.data(), s.size());
    }
  });
}

int mlic_decompress_batch_stream(mlic_model* m, void* stream, const uint8_t* y, size_t y_len, const uint8_t* const* z,
                                 const size_t* z_len, int B, int hz, int wz, float* x_hat, const float* vbr_scales) {
  return guard([&] {
    MLIC_CHECK(m && y && z && x_hat && B > 0 && hz > 0 && wz > 0, "bad arguments");
    const uint8_t* ys[1] = {y};
    const size_t yl[1] = {y_len};
    impl(m).decompress(ys, yl, z, z_len, B, hz, wz, x_hat, vbr_scales, (hipStream_t)stream, true);
  });
}

int mlic_layer_streams(mlic_model* m, int b, const uint8_t** ptrs, size_t* lens, int cap, int* n) {
  return guard([&] {
    MLIC_CHECK(m && n, "bad arguments");
    const std::vector<std::string>& l = impl(m).layer_streams(b);
    *n = (int)l.size();
    if (ptrs || lens) {
      MLIC_CHECK(ptrs && lens && cap >= (int)l.size(), "layer_streams: ptrs and lens of at least S entries");
      for (size_t k = 0; k < l.size(); ++k) {
        ptrs[k] = reinterpret_cast<const uint8_t*>(l[k].data());
        lens[k] = l[k].size();
      }
    }
  });
}

int mlic_decompress_prefix(mlic_model* m, void* stream, const uint8_t* const* y, const size_t* y_len,
                           int strings_per_image, const uint8_t* const* z, const size_t* z_len, int B, int hz, int wz,
                           int slices, int fill, const float* vbr_scales, float* x_hat) {
  return guard([&] {
    MLIC_CHECK(m && y && y_len && z && z_len && x_hat && B > 0 && hz > 0 && wz > 0, "bad arguments");
    Model& mod = impl(m);
    const int S = mod.cfg().S;
    if (slices < 0 || slices > S)
      throw Error("mlic: decompress_prefix: slices must be in [0, " + std::to_string(S) + "], got " +
                  std::to_string(slices));
    if (fill != 0 && fill != 1) throw Error("mlic: decompress_prefix: fill must be 0 (mean) or 1 (zero)");
    if (strings_per_image < 1) throw Error("mlic: decompress_prefix: strings_per_image must be at least 1");
    if (strings_per_image > 1 && strings_per_image < slices)
      throw Error("mlic: decompress_prefix: " + std::to_string(strings_per_image) + " layer strings per image, " +
                  std::to_string(slices) + " slices asked for");
    const int used = strings_per_image == 1 ? (slices > 0 ? 1 : 0) : slices;
    for (int b = 0; b < B; ++b) {
      for (int k = 0; k < used; ++k)
        if (y[(size_t)b * strings_per_image + k] == nullptr)
          throw Error("mlic: decompress_prefix: a null y string among those that are read");
      if (z[b] == nullptr) throw Error("mlic: decompress_prefix: a null z string");
    }
    Prefix p;
    p.slices = slices;
    p.fill = fill;
    p.strings = strings_per_image;
    mod.decompress(y, y_len, z, z_len, B, hz, wz, x_hat, vbr_scales, (hipStream_t)stream, false, nullptr, p);
  });
}

int mlic_decompress(mlic_model* m, void* stream, const uint8_t* const* y, const size_t* y_len,
                    const uint8_t* const* z, const size_t* z_len, int B, int hz, int wz, float* x_hat,
                    float vbr_scale) {
  const std::vector<float> sc(B > 0 ? B : 0, vbr_scale);
  return mlic_decompress_v(m, stream, y, y_len, z, z_len, B, hz, wz, x_hat, sc.data());
}

// ROI coding: what the three _g entries refuse before any GPU call
static Model& roi_model(mlic_model* m, const float* gain_plane, const char* who) {
  Model& mod = impl(m);
  if (!mod.cfg().vbr) throw Error(std::string("mlic: ") + who + ": a gain plane needs a *_VBR model, got " + mod.cfg().name);
  if (gain_plane == nullptr) throw Error(std::string("mlic: ") + who + ": null gain plane");
  return mod;
}

int mlic_forward_g(mlic_model* m, void* stream, const float* x, int B, int H, int W, float* x_hat, float* y_lik,
                   float* z_lik, const float* gain_plane) {
  return guard([&] {
    Model& mod = roi_model(m, gain_plane, "forward_g");
    MLIC_CHECK(x && B > 0, "bad arguments");
    mod.forward(x, B, H, W, x_hat, y_lik, z_lik, nullptr, (hipStream_t)stream, gain_plane);
  });
}

int mlic_compress_g(mlic_model* m, void* stream, const float* x, int B, int H, int W, const float* gain_plane) {
  return guard([&] {
    Model& mod = roi_model(m, gain_plane, "compress_g");
    MLIC_CHECK(x && B > 0, "bad arguments");
    mod.compress(x, B, H, W, nullptr, (hipStream_t)stream, gain_plane);
  });
}

int mlic_decompress_g(mlic_model* m, void* stream, const uint8_t* const* y, const size_t* y_len,
                      const uint8_t* const* z, const size_t* z_len, int B, int hz, int wz, float* x_hat,
                      const float* gain_plane) {
  return guard([&] {
    Model& mod = roi_model(m, gain_plane, "decompress_g");
    MLIC_CHECK(y && y_len && z && z_len && x_hat && B > 0 && hz > 0 && wz > 0, "bad arguments");
    for (int b = 0; b < B; ++b)
      if (y[b] == nullptr)
        throw Error("mlic: decompress_g: one y string per image expected (the batch-stream layout is not supported "
                    "with a gain plane)");
    mod.decompress(y, y_len, z, z_len, B, hz, wz, x_hat, nullptr, (hipStream_t)stream, false, gain_plane);
  });
}

int mlic_image_roi_levels_u8(void* stream, const uint8_t* mask, const int64_t* mask_strides, int B, int H, int W, int lo,
                             int hi, uint8_t* levels) {
  return guard([&] { roi_levels_u8(mask, mask_strides, B, H, W, lo, hi, levels, (hipStream_t)stream); });
}

int mlic_roi_gain_plane(void* stream, const uint8_t* levels, int B, int hz, int wz, const float* gains_host,
                        int n_levels, float* g) {
  return guard([&] { roi_gain_plane(levels, B, hz, wz, gains_host, n_levels, g, (hipStream_t)stream); });
}

int mlic_image_sq_err_roi_u8(void* stream, const uint8_t* a, const int64_t* a_strides, const uint8_t* b,
                             const int64_t* b_strides, const uint8_t* mask, const int64_t* mask_strides, int B, int H,
                             int W, uint64_t* out) {
  return guard([&] {
    sq_err_roi_u8(a, a_strides, b, b_strides, mask, mask_strides, B, H, W, out, (hipStream_t)stream);
  });
}

int mlic_rate_map_run(void* stream, const float* y_lik, int64_t y_bs, const float* z_lik, int64_t z_bs, int B, int M,
                      int S, int h, int w, int N, double* y_map, double* z_map, double* cell_bits, double* slice_bits) {
  return guard([&] {
    rate_map_check(y_lik, y_bs, z_lik, z_bs, B, M, S, h, w, N, y_map, z_map, cell_bits, slice_bits);
    // cell_bits and slice_bits are computed from the two maps: a map the caller leaves out goes into scratch
    const size_t ny = y_map ? 0 : (size_t)B * S * h * w, nz = z_map ? 0 : (size_t)B * (h / 4) * (w / 4);
    if (ny + nz == 0) {
      rate_map(y_lik, y_bs, z_lik, z_bs, B, M, S, h, w, N, y_map, z_map, cell_bits, slice_bits, (hipStream_t)stream);
      return;
    }
    double* scratch = nullptr;
    HIP_OK(hipMalloc(&scratch, sizeof(double) * (ny + nz)));
    try {
      rate_map(y_lik, y_bs, z_lik, z_bs, B, M, S, h, w, N, y_map ? y_map : scratch, z_map ? z_map : scratch + ny,
               cell_bits, slice_bits, (hipStream_t)stream);
      HIP_OK(hipStreamSynchronize((hipStream_t)stream));
    } catch (...) {
      (void)hipFree(scratch);
      throw;
    }
    HIP_OK(hipFree(scratch));
  });
}

int mlic_image_sq_err_blocks_u8(void* stream, const uint8_t* a, const int64_t* a_strides, const uint8_t* b,
                                const int64_t* b_strides, int B, int H, int W, int block, uint32_t* out) {
  return guard([&] { sq_err_blocks_u8(a, a_strides, b, b_strides, B, H, W, block, out, (hipStream_t)stream); });
}

int mlic_image_heat_u8(void* stream, const double* plane, int B, int ph, int pw, int cell, double lo, double hi,
                       int cmap, int H, int W, uint8_t* dst, const int64_t* dst_strides, const uint8_t* under,
                       const int64_t* under_strides, int alpha) {
  return guard([&] {
    image_heat_u8(plane, B, ph, pw, cell, lo, hi, cmap, H, W, dst, dst_strides, under, under_strides, alpha,
                  (hipStream_t)stream);
  });
}

int mlic_run_module(mlic_model* m, void* stream, const char* which, int idx, const float* in0, const float* in1,
                    int B, int Cin, int H, int W, float* out) {
  return guard([&] { impl(m).run_module(which, idx, in0, in1, B, Cin, H, W, out, (hipStream_t)stream); });
}

int mlic_workspace_bytes(mlic_model* m, size_t* arena, size_t* weights) {
  return guard([&] {
    *arena = impl(m).arena_bytes();
    *weights = impl(m).weight_bytes();
  });
}

int mlic_set_precision(mlic_model* m, int precision) {
  return guard([&] {
    MLIC_CHECK(precision >= PREC_F32 && precision <= PREC_F16X3_V2, "precision must be 0 (f32), 1 or 2 (f16x3)");
    impl(m).set_precision(precision);
  });
}

int mlic_ab_families(int* built) {
  return guard([&] {
    MLIC_CHECK(built, "null out");
    *built = ab_families_built() ? 1 : 0;
  });
}

int mlic_set_kernel_option(const char* name, int value) {
  return guard([&] {
    MLIC_CHECK(name, "null option name");
    opt_set(name, value);
  });
}

int mlic_get_kernel_option(const char* name, int* value) {
  return guard([&] {
    MLIC_CHECK(name && value, "null option name or value");
    *value = opt_get(name);
  });
}

int mlic_set_poison(mlic_model* m, int on) {
  return guard([&] { impl(m).set_poison(on != 0); });
}

int mlic_range_fallbacks(mlic_model* m, int64_t* forward_full, int64_t* forward_gs, int64_t* decompress_gs,
                         int reset) {
  return guard([&] {
    Model::Fallbacks& f = impl(m).fallbacks();
    if (forward_full) *forward_full = f.forward_full.load();
    if (forward_gs) *forward_gs = f.forward_gs.load();
    if (decompress_gs) *decompress_gs = f.decompress_gs.load();
    if (reset) {
      f.forward_full = 0;
      f.forward_gs = 0;
      f.decompress_gs = 0;
    }
  });
}

int mlic_set_synthesis_precision(mlic_model* m, int mode) {
  return guard([&] {
    MLIC_CHECK(mode == 0 || mode == 1, "synthesis precision must be 0 (fp32-faithful) or 1 (fp16 operands)");
    impl(m).set_synthesis_precision(mode);
  });
}

int mlic_set_lanes(mlic_model* m, int lanes) {
  return guard([&] { impl(m).set_lanes(lanes); });
}

int mlic_set_priority_base(mlic_model* m, int base) {
  return guard([&] {
    MLIC_CHECK(base >= 0, "priority base must be >= 0");
    impl(m).set_priority_base(base);
  });
}

int mlic_set_profiling(mlic_model* m, int on) {
  return guard([&] { impl(m).set_profiling(on != 0); });
}

int mlic_profile_read(mlic_model* m, int cat, int64_t* launches, double* ms, double* flops, double* bytes) {
  return guard([&] {
    MLIC_CHECK(cat >= 0 && cat < PCAT_COUNT, "profile category");
    ProfStat s = impl(m).profile_read(cat);
    *launches = s.launches;
    *ms = s.ms;
    *flops = s.flops;
    *bytes = s.bytes;
  });
}

int mlic_profile_layers(mlic_model* m, char* buf, size_t cap, size_t* written) {
  return guard([&] {
    std::string s = impl(m).profile_layers();
    *written = s.size();
    if (buf && cap) {
      const size_t n = std::min(cap - 1, s.size());
      std::memcpy(buf, s.data(), n);
      buf[n] = 0;
    }
  });
}

// conv micro-benchmark: random operands of one layer shape, `iters` launches timed with events.
// impl: 0 = conv_mfma (fp32), 1 = conv_f16x3.  Returns ms per launch and TFLOP/s (algorithmic).
int mlic_bench_conv(int impl, int B, int Cin, int Cout, int H, int W, int K, int stride, int epi, int iters,
                    double* ms_per, double* tflops) {
  return guard([&] {
    const int pad = K / 2;
    const int Ho = (H + 2 * pad - K) / stride + 1, Wo = (W + 2 * pad - K) / stride + 1;
    const int64_t nx = (int64_t)B * Cin * H * W, ny = (int64_t)B * Cout * Ho * Wo, nw = (int64_t)Cout * Cin * K * K;
    const int cin_pad = (Cin + 31) / 32 * 32;
    const int64_t nh = (int64_t)Cout * K * K * cin_pad;
    float *x, *y, *w, *wp, *bias;
    _Float16 *wh, *wl;
    HIP_OK(hipMalloc(&x, nx * 4));
    HIP_OK(hipMalloc(&y, ny * 4));
    HIP_OK(hipMalloc(&w, nw * 4));
    HIP_OK(hipMalloc(&wp, nw * 4));
    HIP_OK(hipMalloc(&bias, Cout * 4));
    HIP_OK(hipMalloc(&wh, nh * 2));
    HIP_OK(hipMalloc(&wl, nh * 2));
    {
      std::vector<float> hx(std::max(nx, nw));
      uint32_t st = 12345;
      for (auto& v : hx) { st = st * 1664525u + 1013904223u; v = ((st >> 9) * (1.0f / 8388608.0f)) - 0.5f; }
      HIP_OK(hipMemcpy(x, hx.data(), nx * 4, hipMemcpyHostToDevice));
      HIP_OK(hipMemcpy(w, hx.data(), nw * 4, hipMemcpyHostToDevice));
      HIP_OK(hipMemset(bias, 0, Cout * 4));
    }
    pack_conv(w, wp, Cout, Cin, K * K, nullptr);
    const int wexp = split_weights(w, wh, wl, Cout, Cin, K * K, cin_pad, true, nullptr);
    ConvParams P{};
    P.nseg = 1;
    P.seg[0] = {x, Cin, (int64_t)Cin * H * W};
    P.Cin = Cin; P.H = H; P.W = W; P.Cout = Cout; P.Ho = Ho; P.Wo = Wo; P.K = K; P.stride = stride; P.pad = pad;
    P.wpk = wp; P.bias = bias; P.out = y; P.B = B;
    P.out_bs = (int64_t)Cout * Ho * Wo;
    P.out_cs = (int64_t)Ho * Wo;
    P.epi = epi;
    MLIC_CHECK(!(epi & (EPI_GDN | EPI_IGDN | EPI_SHUFFLE)) || !(epi & EPI_RES), "bench: unsupported epilogue");
    if (epi & (EPI_GDN | EPI_IGDN)) {  // the conv input doubles as the GDN operand (Cin == Cout)
      MLIC_CHECK(Cin == Cout && stride == 1, "bench: GDN needs Cin == Cout");
      P.aux = x;
      P.aux_bs = (int64_t)Cin * H * W;
    }
    if (epi & EPI_RES) {  // in place, as the LRP head's residual into y_hat
      P.res = y;
      P.res_bs = P.out_bs;
    }
    _Float16 *wx = nullptr, *wxh = nullptr;
    if (conv_x4_ok(P, cin_pad)) {
      HIP_OK(hipMalloc((void**)&wx, x4_weight_halves(Cout, K * K, cin_pad) * 2));
      x4_pack_weights(wh, wl, Cout, K * K, cin_pad, wx, nullptr);
      if (impl == CONV_X4H) {
        HIP_OK(hipMalloc((void**)&wxh, x4_weight_halves(Cout, K * K, cin_pad, true) * 2));
        x4_pack_weights(wh, wl, Cout, K * K, cin_pad, wxh, nullptr, true);
      }
    }
    ConvWeights cw{wp, wh, wl, cin_pad, wx, wexp};
    cw.wx4h = wxh;
    const int which = impl < 0 ? conv_select(P, cw, 2) : impl;  // < 0: what the model runs (precision 2)
    if (which == CONV_X4H) MLIC_CHECK(conv_x4_ok(P, cin_pad), "x4: unsupported shape");
    if (which == CONV_PW) MLIC_CHECK(pw_resident_ok(P, cin_pad), "pw_resident: unsupported shape");
    if (which == CONV_X4) MLIC_CHECK(conv_x4_ok(P, cin_pad), "x4: unsupported shape");
    void* ws = nullptr;
    const int64_t wsb = conv_ws_bytes(which, P, cw);
    if (wsb > 0) HIP_OK(hipMalloc(&ws, wsb));
    auto launch = [&] { conv_run(which, P, cw, nullptr, ws); };
    launch();
    HIP_OK(hipDeviceSynchronize());
    hipEvent_t a, b;
    HIP_OK(hipEventCreate(&a));
    HIP_OK(hipEventCreate(&b));
    HIP_OK(hipEventRecord(a, nullptr));
    for (int i = 0; i < iters; ++i) launch();
    HIP_OK(hipEventRecord(b, nullptr));
    HIP_OK(hipEventSynchronize(b));
    float ms = 0;
    HIP_OK(hipEventElapsedTime(&ms, a, b));
    *ms_per = ms / iters;
    *tflops = 2.0 * (double)B * Cout * Ho * Wo * Cin * K * K / (*ms_per * 1e-3) / 1e12;
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    for (void* p : {(void*)x, (void*)y, (void*)w, (void*)wp, (void*)bias, (void*)wh, (void*)wl, (void*)wx, (void*)wxh, ws})
      if (p) (void)hipFree(p);
  });
}

int mlic_host_stats(mlic_model* m, double* enc_ms, double* dec_ms, double* wait_ms, int reset) {
  return guard([&] {
    HostStats& h = impl(m).host_stats();
    *enc_ms = h.enc_ns.load() * 1e-6;
    *dec_ms = h.dec_ns.load() * 1e-6;
    *wait_ms = h.wait_ns.load() * 1e-6;
    if (reset) {
      h.enc_ns = 0;
      h.dec_ns = 0;
      h.wait_ns = 0;
    }
  });
}

int mlic_profile_categories(int* n) {
  return guard([&] { *n = PCAT_COUNT; });
}

int mlic_profile_category_name(int cat, char* buf, size_t cap) {
  return guard([&] {
    MLIC_CHECK(cat >= 0 && cat < PCAT_COUNT, "profile category");
    const std::string nm = prof_cat_name(cat);
    MLIC_CHECK(cap > nm.size(), "buffer too small");
    std::memcpy(buf, nm.c_str(), nm.size() + 1);
  });
}

int mlic_conv_choice(int B, int Cin, int Cout, int H, int W, int K, int stride, int epi, int* impl) {
  return guard([&] {
    MLIC_CHECK(impl && B > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0 && (K == 1 || K == 3 || K == 5) && stride > 0,
               "conv_choice: bad arguments");
    const int pad = K / 2;
    ConvParams P{};
    P.nseg = 1;
    P.seg[0] = {nullptr, Cin, (int64_t)Cin * H * W};
    P.Cin = Cin; P.H = H; P.W = W; P.Cout = Cout; P.K = K; P.stride = stride; P.pad = pad;
    P.Ho = (H + 2 * pad - K) / stride + 1;
    P.Wo = (W + 2 * pad - K) / stride + 1;
    P.B = B;
    P.epi = epi;
    const int cin_pad = (Cin + 31) / 32 * 32;
    // weight pointers only signal presence, by the model's own allocation rule (model.cpp: split
    // fp16 copies for Cin >= 16, x4 images of those for K in {1, 3, 5} and Cout >= 64)
    static const _Float16 tag = 0;
    const bool split = Cin >= 16;
    const bool x4 = split && Cout >= 64;
    const ConvWeights cw{nullptr, split ? &tag : nullptr, split ? &tag : nullptr, cin_pad, x4 ? &tag : nullptr, 0};
    *impl = conv_select(P, cw, 2);
  });
}

int mlic_conv_run(void* stream, int impl, const float* x, const float* w, const float* bias, float* y, int B, int Cin,
                  int Cout, int H, int W, int K, int stride, int epi, const float* aux, const float* res) {
  return guard([&] {
    hipStream_t st = (hipStream_t)stream;
    const int pad = K / 2;
    const int Ho = (H + 2 * pad - K) / stride + 1, Wo = (W + 2 * pad - K) / stride + 1;
    const int cin_pad = (Cin + 31) / 32 * 32;
    const int64_t nw = (int64_t)Cout * Cin * K * K, nh = (int64_t)Cout * K * K * cin_pad;
    float* wp = nullptr;
    _Float16 *wh = nullptr, *wl = nullptr;
    HIP_OK(hipMallocAsync((void**)&wp, nw * 4, st));
    HIP_OK(hipMallocAsync((void**)&wh, nh * 2, st));
    HIP_OK(hipMallocAsync((void**)&wl, nh * 2, st));
    pack_conv(w, wp, Cout, Cin, K * K, st);
    const int wexp = split_weights(w, wh, wl, Cout, Cin, K * K, cin_pad, true, st);
    ConvParams P{};
    P.nseg = 1;
    P.seg[0] = {x, Cin, (int64_t)Cin * H * W};
    P.Cin = Cin; P.H = H; P.W = W; P.Cout = Cout; P.Ho = Ho; P.Wo = Wo; P.K = K; P.stride = stride; P.pad = pad;
    P.wpk = wp; P.bias = bias; P.out = y; P.B = B; P.epi = epi;
    const bool shuffle = (epi & EPI_SHUFFLE) != 0;
    MLIC_CHECK(!shuffle || Cout % 4 == 0, "shuffle needs Cout % 4 == 0");
    P.out_cs = shuffle ? (int64_t)4 * Ho * Wo : (int64_t)Ho * Wo;
    P.out_bs = (int64_t)Cout * Ho * Wo;
    MLIC_CHECK(!(epi & (EPI_GDN | EPI_IGDN)) || aux, "GDN epilogue needs aux");
    MLIC_CHECK(!(epi & EPI_RES) || res, "residual epilogue needs res");
    P.aux = aux; P.aux_bs = (int64_t)Cout * Ho * Wo;
    P.res = res; P.res_bs = P.out_bs;
    _Float16 *wx = nullptr, *wxh = nullptr;
    if (conv_x4_ok(P, cin_pad)) {
      HIP_OK(hipMallocAsync((void**)&wx, x4_weight_halves(Cout, K * K, cin_pad) * 2, st));
      x4_pack_weights(wh, wl, Cout, K * K, cin_pad, wx, st);
      if (impl == CONV_X4H) {
        HIP_OK(hipMallocAsync((void**)&wxh, x4_weight_halves(Cout, K * K, cin_pad, true) * 2, st));
        x4_pack_weights(wh, wl, Cout, K * K, cin_pad, wxh, st, true);
      }
    }
    ConvWeights cw{wp, wh, wl, cin_pad, wx, wexp};
    cw.wx4h = wxh;
    const int which = impl < 0 ? conv_select(P, cw, 2) : impl;
    if (which == CONV_X4H) MLIC_CHECK(conv_x4_ok(P, cin_pad), "x4: unsupported shape");
    if (which == CONV_PW) MLIC_CHECK(pw_resident_ok(P, cin_pad), "pw_resident: unsupported shape");
    if (which == CONV_NARROW) MLIC_CHECK(conv_narrow_ok(P), "narrow: unsupported shape");
    if (which == CONV_SMALLCIN) MLIC_CHECK(conv_smallcin_ok(P), "smallcin: unsupported shape");
    if (which == CONV_HALO) MLIC_CHECK(conv_halo_ok(P, cin_pad), "halo: unsupported shape");
    if (which == CONV_X4) MLIC_CHECK(conv_x4_ok(P, cin_pad), "x4: unsupported shape");
    void* ws = nullptr;
    const int64_t wsb = conv_ws_bytes(which, P, cw);
    if (wsb > 0) HIP_OK(hipMallocAsync(&ws, wsb, st));
    conv_run(which, P, cw, st, ws);
    if (ws) HIP_OK(hipFreeAsync(ws, st));
    if (wx) HIP_OK(hipFreeAsync(wx, st));
    if (wxh) HIP_OK(hipFreeAsync(wxh, st));
    HIP_OK(hipFreeAsync(wp, st));
    HIP_OK(hipFreeAsync(wh, st));
    HIP_OK(hipFreeAsync(wl, st));
    HIP_OK(hipStreamSynchronize(st));
  });
}

int mlic_dw_run(void* stream, const float* x, const float* w, const float* bias, float* y, int B, int C, int H, int W,
                int stride, int gelu) {
  return guard([&] {
    DwParams P{};
    P.nseg = 1;
    P.seg[0] = {x, C, (int64_t)C * H * W};
    P.C = C; P.H = H; P.W = W; P.stride = stride;
    P.Ho = (H - 1) / stride + 1;
    P.Wo = (W - 1) / stride + 1;
    P.w = w; P.bias = bias; P.out = y; P.out_bs = (int64_t)C * P.Ho * P.Wo; P.gelu = gelu; P.B = B;
    dw3x3(P, (hipStream_t)stream);
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  });
}

int mlic_dwpw_run(void* stream, const float* x, const float* dww, const float* dwb, const float* w, const float* bias,
                  float* y, int B, int C, int Cout, int H, int W, int epi, const float* res) {
  return guard([&] {
    hipStream_t st = (hipStream_t)stream;
    const int cin_pad = (C + 31) / 32 * 32;
    const int64_t nh = (int64_t)Cout * cin_pad;
    _Float16 *wh = nullptr, *wl = nullptr;
    HIP_OK(hipMallocAsync((void**)&wh, nh * 2, st));
    HIP_OK(hipMallocAsync((void**)&wl, nh * 2, st));
    const int wexp = split_weights(w, wh, wl, Cout, C, 1, cin_pad, true, st);
    ConvParams P{};
    P.nseg = 1;
    P.seg[0] = {x, C, (int64_t)C * H * W};
    P.Cin = C; P.H = H; P.W = W; P.Cout = Cout; P.Ho = H; P.Wo = W; P.K = 1; P.stride = 1; P.pad = 0;
    P.wexp = wexp; P.bias = bias; P.out = y; P.B = B; P.epi = epi;
    P.out_cs = (int64_t)H * W;
    P.out_bs = (int64_t)Cout * H * W;
    MLIC_CHECK(!(epi & EPI_RES) || res, "residual epilogue needs res");
    P.res = res; P.res_bs = P.out_bs;
    MLIC_CHECK(dwpw_ok(P, cin_pad), "dwpw: unsupported shape");
    dwpw_forward(P, wh, wl, cin_pad, dww, dwb, st);
    HIP_OK(hipFreeAsync(wh, st));
    HIP_OK(hipFreeAsync(wl, st));
    HIP_OK(hipStreamSynchronize(st));
  });
}

int mlic_local_attn_run(void* stream, int impl, const float* qkv, const float* rel_table, const int32_t* rel_index,
                        float* out, int C, int H, int W, int B, float scale) {
  return guard([&] {
    LocalAttnParams A{};
    A.qkv = qkv;
    A.qkv_bs = (int64_t)3 * C * H * W;
    A.out = out;
    A.out_bs = (int64_t)25 * C * H * W;
    A.rel_table = rel_table;
    A.rel_index = rel_index;
    A.scale = scale;
    A.C = C; A.H = H; A.W = W; A.B = B;
    if (impl == 0) local_attn_valu(A, (hipStream_t)stream);
    else local_attn_mfma(A, (hipStream_t)stream);
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  });
}

int mlic_local_attn_packed_run(void* stream, const float* qkv, const float* rel_table, const int32_t* rel_index,
                               uint16_t* out, int H, int W, int B, float scale) {
  return guard([&] {
    LocalAttnParams A{};
    A.qkv = qkv;
    A.qkv_bs = (int64_t)3 * 32 * H * W;
    A.rel_table = rel_table;
    A.rel_index = rel_index;
    A.scale = scale;
    A.C = 32; A.H = H; A.W = W; A.B = B;
    local_attn_packed(A, reinterpret_cast<_Float16*>(out), (H * W + 31) / 32 * 32, (hipStream_t)stream);
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  });
}

int mlic_local_attn_packed_half_run(void* stream, const float* qkv, const float* rel_table, const int32_t* rel_index,
                                    uint16_t* out, int H, int W, int B, float scale, int ckbd) {
  return guard([&] {
    MLIC_CHECK(ckbd == 1 || ckbd == 2, "ckbd: 1 (anchors) or 2 (non-anchors)");
    LocalAttnParams A{};
    A.qkv = qkv;
    A.qkv_bs = (int64_t)3 * 32 * H * W;
    A.rel_table = rel_table;
    A.rel_index = rel_index;
    A.scale = scale;
    A.C = 32; A.H = H; A.W = W; A.B = B;
    A.ckbd = ckbd;
    local_attn_packed(A, reinterpret_cast<_Float16*>(out), (H * W / 2 + 31) / 32 * 32, (hipStream_t)stream);
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  });
}

// one image's pixel count as the kernels index it (int, with a launch block of headroom), and the
// launch grids' y / z extents
static void check_grid(int B, int H, int W, int rows) {
  MLIC_CHECK(B >= 1 && B <= 65535, "B must be in 1..65535");
  MLIC_CHECK(H >= 1 && W >= 1 && (int64_t)H * W <= (int64_t)1 << 30, "H, W must be >= 1 and H * W <= 2^30");
  MLIC_CHECK(rows >= 1 && (int64_t)rows * B <= 65535, "too many (image, head) rows for one launch");
}

int mlic_linatt_splits(int HW, int* nsplit) {
  return guard([&] {
    MLIC_CHECK(nsplit != nullptr, "null nsplit");
    MLIC_CHECK(HW >= 1, "HW must be >= 1");
    *nsplit = ctx_splits(HW);
  });
}

int mlic_linear_attention_run(void* stream, const float* k, const float* v, const float* q, float* out, float* ctx_out,
                              int B, int heads, int hd, int H, int W, int nsplit, int kmask, int qmask) {
  return guard([&] {
    MLIC_CHECK(k && v && q && out, "null tensor");
    MLIC_CHECK(hd == 16 || hd == 32, "hd must be 16 or 32");
    MLIC_CHECK(heads >= 1, "heads must be >= 1");
    check_grid(B, H, W, heads);
    MLIC_CHECK(nsplit <= 64, "nsplit must be <= 64 (<= 0: the model's choice)");
    MLIC_CHECK((kmask == 0 || kmask == 1) && (qmask == 0 || qmask == 1), "kmask, qmask must be 0 or 1");
    hipStream_t st = (hipStream_t)stream;
    const int HW = H * W;
    const int ns = nsplit <= 0 ? ctx_splits(HW) : nsplit;
    const int64_t bs = (int64_t)heads * hd * HW, nctx = (int64_t)B * heads * hd * hd;
    float *part = nullptr, *ctx = nullptr;
    HIP_OK(hipMallocAsync((void**)&part, linear_attention_part_floats(heads, hd, B, ns) * 4, st));
    HIP_OK(hipMallocAsync((void**)&ctx, nctx * 4, st));
    linear_attention(k, bs, v, bs, q, bs, out, bs, part, ctx, heads, hd, H, W, B, ns, kmask, qmask, st);
    if (ctx_out) HIP_OK(hipMemcpyAsync(ctx_out, ctx, nctx * 4, hipMemcpyDeviceToDevice, st));
    HIP_OK(hipFreeAsync(part, st));
    HIP_OK(hipFreeAsync(ctx, st));
    HIP_OK(hipStreamSynchronize(st));
  });
}

int mlic_linatt_pack_run(void* stream, const float* q, const float* ctx, uint16_t* out_halves, int B, int heads, int hd,
                         int H, int W, int K, int qmask) {
  return guard([&] {
    MLIC_CHECK(q && ctx && out_halves, "null tensor");
    MLIC_CHECK(hd == 16 || hd == 32, "hd must be 16 or 32");
    MLIC_CHECK(heads >= 1 && (heads * (int64_t)hd) % 32 == 0, "heads * hd must be a multiple of 32");
    MLIC_CHECK(K == 3 || K == 5, "K must be 3 or 5");
    check_grid(B, H, W, heads * hd / 32);
    check_grid(B, H + K - 1, W + K - 1, 1);  // the padded image's lines
    MLIC_CHECK(qmask == 0 || qmask == 1, "qmask must be 0 or 1");
    ConvParams P{};
    P.nseg = 1;
    P.seg[0] = {nullptr, heads * hd, (int64_t)heads * hd * H * W};  // geometry only: the pack reads q
    P.Cin = heads * hd; P.H = H; P.W = W; P.Cout = P.Cin; P.Ho = H; P.Wo = W; P.K = K; P.stride = 1; P.pad = K / 2;
    P.B = B;
    P.rflag = nullptr;
    linatt_pack(q, P.seg[0].bs, ctx, heads, hd, qmask, P, reinterpret_cast<_Float16*>(out_halves), (hipStream_t)stream);
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  });
}

int mlic_ln_channels_run(void* stream, const float* x, const float* gamma, const float* beta, float* y, int B, int C,
                         int HW) {
  return guard([&] {
    MLIC_CHECK(x && gamma && beta && y, "null tensor");
    MLIC_CHECK(C == 32 || C == 64 || C == 128, "C must be 32, 64 or 128");
    check_grid(B, 1, HW, 1);
    ln_channels(x, (int64_t)C * HW, y, (int64_t)C * HW, gamma, beta, C, HW, B, (hipStream_t)stream);
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  });
}

int mlic_taps_gather_run(void* stream, const float* part, const float* bias, float* out, int B, int H, int W) {
  return guard([&] {
    MLIC_CHECK(part && out, "null tensor");
    check_grid(B, H, W, 1);
    MLIC_CHECK((H + 3) / 4 <= 65535, "H too large for one launch");
    taps_gather(part, (int64_t)108 * H * W, bias, out, (int64_t)12 * H * W, H, W, B, (hipStream_t)stream);
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  });
}

// ---- the entropy front alone: quantisation, scale indexes, dequantisation, the bottleneck, the masks ----
// the geometry the three slice-loop kernels share: one image's C * H * W elements as they index them, the
// squeezed streams' W / 2, and every batch stride at least the tensor it strides
static QuantParams quant_params(const mlic_quant_desc* d) {
  MLIC_CHECK(d != nullptr, "null descriptor");
  MLIC_CHECK(d->params && d->table, "null tensor");
  check_grid(d->B, d->H, d->W, 1);
  MLIC_CHECK(d->C >= 1 && (int64_t)d->C * d->H * d->W <= (int64_t)1 << 30, "C must be >= 1 and C * H * W <= 2^30");
  MLIC_CHECK(d->W % 2 == 0, "W must be even");
  MLIC_CHECK(d->phase == 0 || d->phase == 1, "phase must be 0 (anchor) or 1 (non-anchor)");
  MLIC_CHECK(d->ntable >= 2 && d->ntable <= 256, "ntable must be in 2..256");
  MLIC_CHECK(d->vbr == 0 || d->vbr == 1, "vbr must be 0 or 1");
  MLIC_CHECK(d->vbr || (!d->scp && !d->rsp), "gain planes need vbr");
  const int64_t n = (int64_t)d->C * d->H * d->W;
  MLIC_CHECK(d->params_bs >= 2 * n, "params_bs smaller than [2C][H][W]");
  QuantParams Q{};
  Q.y = d->y; Q.y_bs = d->y_bs;
  Q.params = d->params; Q.params_bs = d->params_bs;
  Q.params_a = d->params_a; Q.params_a_bs = d->params_a_bs;
  Q.yh = d->yh; Q.yh_bs = d->yh_bs;
  Q.lik = d->lik; Q.lik_bs = d->lik_bs;
  Q.sym = d->sym; Q.idx = d->idx;
  Q.sym16 = d->sym16; Q.idx8 = d->idx8; Q.ovf = d->ovf;
  Q.nlim = d->nlim;
  Q.table = d->table; Q.ntable = d->ntable;
  Q.phase = d->phase; Q.vbr = d->vbr;
  Q.sc = d->sc; Q.rs = d->rs;
  Q.C = d->C; Q.H = d->H; Q.W = d->W; Q.B = d->B;
  Q.scp = d->scp; Q.rsp = d->rsp;
  return Q;
}

int mlic_quant_phase_run(void* stream, const mlic_quant_desc* d) {
  return guard([&] {
    const QuantParams Q = quant_params(d);
    const int64_t n = (int64_t)Q.C * Q.H * Q.W;
    MLIC_CHECK(Q.y && Q.yh, "null tensor");
    MLIC_CHECK(Q.y_bs >= n, "y_bs smaller than [C][H][W]");
    MLIC_CHECK(Q.yh_bs >= n, "yh_bs smaller than [C][H][W]");
    MLIC_CHECK(!Q.lik || Q.params_a, "lik needs params_a");
    MLIC_CHECK(!Q.lik || Q.lik_bs >= n, "lik_bs smaller than [C][H][W]");
    MLIC_CHECK(!Q.params_a || Q.params_a_bs >= 2 * n, "params_a_bs smaller than [2C][H][W]");
    MLIC_CHECK(!Q.sym16 || (Q.idx8 && Q.ovf), "sym16 needs idx8 and ovf");
    MLIC_CHECK(Q.sym16 || (!Q.idx8 && !Q.ovf), "idx8 and ovf need sym16");
    MLIC_CHECK(!Q.idx || Q.sym || Q.sym16, "idx needs sym or sym16");
    MLIC_CHECK((Q.scp != nullptr) == (Q.rsp != nullptr), "scp and rsp: both or neither");
    MLIC_CHECK(!Q.vbr || Q.scp || (Q.sc && Q.rs), "vbr needs sc and rs, or gain planes");
    MLIC_CHECK(Q.nlim >= 1 && Q.nlim <= 32767, "nlim must be in 1..32767");
    quant_phase(Q, (hipStream_t)stream);
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  });
}

int mlic_phase_indexes_run(void* stream, const mlic_quant_desc* d) {
  return guard([&] {
    const QuantParams Q = quant_params(d);
    MLIC_CHECK(Q.idx8 || Q.idx, "null output: idx8 or idx");
    MLIC_CHECK(!Q.vbr || Q.scp || Q.sc, "vbr needs sc, or the gain plane scp");
    phase_indexes(Q, (hipStream_t)stream);
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  });
}

int mlic_phase_dequant_run(void* stream, const mlic_quant_desc* d) {
  return guard([&] {
    const QuantParams Q = quant_params(d);
    const int64_t n = (int64_t)Q.C * Q.H * Q.W;
    MLIC_CHECK(Q.yh, "null tensor");
    MLIC_CHECK(Q.yh_bs >= n, "yh_bs smaller than [C][H][W]");
    MLIC_CHECK(Q.sym16 || Q.sym, "null input: sym16 or sym");
    MLIC_CHECK(!Q.vbr || Q.rsp || Q.rs, "vbr needs rs, or the reciprocal plane rsp");
    phase_dequant(Q, (hipStream_t)stream);
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  });
}

int mlic_phase_fill_run(void* stream, const mlic_quant_desc* d) {
  return guard([&] {
    const QuantParams Q = quant_params(d);
    const int64_t n = (int64_t)Q.C * Q.H * Q.W;
    MLIC_CHECK(Q.yh, "null tensor");
    MLIC_CHECK(Q.yh_bs >= n, "yh_bs smaller than [C][H][W]");
    phase_fill(Q, (hipStream_t)stream);
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  });
}

int mlic_recip_plane_run(void* stream, const float* g, float* r, int64_t n) {
  return guard([&] {
    MLIC_CHECK(g && r, "null tensor");
    MLIC_CHECK(n >= 1 && n <= (int64_t)1 << 31, "n must be in 1..2^31");
    recip_plane(g, r, n, (hipStream_t)stream);
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  });
}

// B * C * H * W elements in one 1-D launch
static void check_eb_grid(int B, int C, int H, int W) {
  check_grid(B, H, W, 1);
  MLIC_CHECK(C >= 1 && (int64_t)B * C * H * W <= (int64_t)1 << 31, "C must be >= 1 and B * C * H * W <= 2^31");
}

int mlic_eb_forward_run(void* stream, const float* z, float* z_hat, float* lik, int32_t* sym, const float* quantiles,
                        const float* m0, const float* m1, const float* m2, const float* m3, const float* m4,
                        const float* b0, const float* b1, const float* b2, const float* b3, const float* b4,
                        const float* f0, const float* f1, const float* f2, const float* f3, int B, int C, int H,
                        int W) {
  return guard([&] {
    MLIC_CHECK(z && quantiles, "null tensor");
    MLIC_CHECK(m0 && m1 && m2 && m3 && m4 && b0 && b1 && b2 && b3 && b4 && f0 && f1 && f2 && f3, "null parameter");
    MLIC_CHECK(z_hat || lik || sym, "null outputs: at least one of z_hat, lik, sym");
    check_eb_grid(B, C, H, W);
    EbParams P{};
    P.z = z; P.z_hat = z_hat; P.lik = lik; P.sym = sym;
    P.quantiles = quantiles;
    P.m0 = m0; P.m1 = m1; P.m2 = m2; P.m3 = m3; P.m4 = m4;
    P.b0 = b0; P.b1 = b1; P.b2 = b2; P.b3 = b3; P.b4 = b4;
    P.f0 = f0; P.f1 = f1; P.f2 = f2; P.f3 = f3;
    P.C = C; P.H = H; P.W = W; P.B = B;
    eb_forward(P, (hipStream_t)stream);
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  });
}

int mlic_eb_dequant_run(void* stream, const int32_t* sym, const float* quantiles, float* z_hat, int B, int C, int H,
                        int W) {
  return guard([&] {
    MLIC_CHECK(sym && quantiles && z_hat, "null tensor");
    check_eb_grid(B, C, H, W);
    eb_dequant(sym, quantiles, z_hat, C, H * W, B, (hipStream_t)stream);
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  });
}

int mlic_ckbd_mask_run(void* stream, const float* x, int64_t x_bs, float* y, int64_t y_bs, int B, int C, int H, int W,
                       int keep_anchor) {
  return guard([&] {
    MLIC_CHECK(x && y, "null tensor");
    check_grid(B, H, W, 1);
    MLIC_CHECK(C >= 1 && (int64_t)C * H * W <= (int64_t)1 << 30, "C must be >= 1 and C * H * W <= 2^30");
    MLIC_CHECK(keep_anchor == 0 || keep_anchor == 1, "keep_anchor must be 0 or 1");
    MLIC_CHECK(x_bs >= (int64_t)C * H * W, "x_bs smaller than [C][H][W]");
    MLIC_CHECK(y_bs >= (int64_t)C * H * W, "y_bs smaller than [C][H][W]");
    ckbd_mask(x, x_bs, y, y_bs, C, H, W, B, keep_anchor, (hipStream_t)stream);
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  });
}

int mlic_local_attn_mask(void* stream, float* out, int H, int W) {
  return guard([&] { local_mask(out, H, W, (hipStream_t)stream); });
}

int mlic_image_sq_err_u8(void* stream, const float* a, const float* b, int B, int64_t n_per, double* out) {
  return guard([&] { sq_err_u8(a, n_per, b, n_per, out, n_per, B, (hipStream_t)stream); });
}

int mlic_ms_ssim_scratch_bytes(int B, int C, int H, int W, size_t* bytes) {
  return guard([&] {
    MLIC_CHECK(bytes != nullptr, "ms_ssim_scratch_bytes: null bytes");
    *bytes = ms_ssim_scratch_bytes(B, C, H, W);
  });
}

int mlic_image_ms_ssim_u8(void* stream, const float* a, const int64_t* a_strides, const float* b,
                          const int64_t* b_strides, int B, int C, int H, int W, void* scratch,
                          size_t scratch_bytes, double* out, double* terms) {
  return guard([&] {
    const size_t need = ms_ssim_scratch_bytes(B, C, H, W);  // checks B, C, H, W
    MLIC_CHECK(a && b && a_strides && b_strides && out, "ms_ssim: null argument");
    MLIC_CHECK(scratch != nullptr && scratch_bytes >= need, "ms_ssim: scratch too small (mlic_ms_ssim_scratch_bytes)");
    MLIC_CHECK(reinterpret_cast<uintptr_t>(scratch) % 8 == 0, "ms_ssim: scratch must be 8-byte aligned");
    ms_ssim_u8(a, a_strides, b, b_strides, B, C, H, W, scratch, out, terms, (hipStream_t)stream);
  });
}

int mlic_lpips_create(int n, const char* const* names, const float* const* ptrs, const int64_t* shapes,
                      const int* ndims, void* stream, mlic_lpips** out) {
  return guard([&] {
    MLIC_CHECK(out != nullptr, "lpips_create: null out");
    *out = nullptr;
    auto* h = new mlic_lpips();
    try {
      h->impl = lpips_create(n, names, ptrs, shapes, ndims, (hipStream_t)stream);
    } catch (...) {
      delete h;
      throw;
    }
    *out = h;
  });
}

int mlic_lpips_destroy(mlic_lpips* h) {
  return guard([&] {
    if (!h) return;
    lpips_destroy(h->impl);
    delete h;
  });
}

int mlic_lpips_set_precision(mlic_lpips* h, int precision) {
  return guard([&] {
    MLIC_CHECK(h != nullptr && h->impl != nullptr, "null mlic_lpips handle");
    lpips_set_precision(h->impl, precision);
  });
}

int mlic_lpips_scratch_bytes(int B, int H, int W, size_t* bytes) {
  return guard([&] {
    MLIC_CHECK(bytes != nullptr, "lpips_scratch_bytes: null bytes");
    *bytes = lpips_scratch_bytes(B, H, W);
  });
}

int mlic_image_lpips_u8(mlic_lpips* h, void* stream, const float* a, const int64_t* a_strides, const float* b,
                        const int64_t* b_strides, int B, int H, int W, void* scratch, size_t scratch_bytes,
                        double* out, double* terms) {
  return guard([&] {
    MLIC_CHECK(h != nullptr && h->impl != nullptr, "null mlic_lpips handle");
    const size_t need = lpips_scratch_bytes(B, H, W);  // checks B, H, W
    MLIC_CHECK(a && b && a_strides && b_strides, "lpips: null image or strides");
    MLIC_CHECK(scratch != nullptr && scratch_bytes >= need, "lpips: scratch too small (mlic_lpips_scratch_bytes)");
    MLIC_CHECK(reinterpret_cast<uintptr_t>(scratch) % 256 == 0, "lpips: scratch must be 256-byte aligned");
    MLIC_CHECK(out != nullptr, "lpips: null out");
    lpips_u8(h->impl, a, a_strides, b, b_strides, B, H, W, scratch, out, terms, (hipStream_t)stream);
  });
}

int mlic_lpips_profile(mlic_lpips* h, int on, double* ms3) {
  return guard([&] {
    MLIC_CHECK(h != nullptr && h->impl != nullptr, "null mlic_lpips handle");
    lpips_profile(h->impl, on != 0, ms3);
  });
}

int mlic_lpips_range_fallbacks(mlic_lpips* h, int64_t* count, int reset) {
  return guard([&] {
    MLIC_CHECK(h != nullptr && h->impl != nullptr, "null mlic_lpips handle");
    const int64_t v = lpips_range_fallbacks(h->impl, reset != 0);
    if (count) *count = v;
  });
}

int mlic_dists_create(int n, const char* const* names, const float* const* ptrs, const int64_t* shapes,
                      const int* ndims, void* stream, mlic_dists** out) {
  return guard([&] {
    MLIC_CHECK(out != nullptr, "dists_create: null out");
    *out = nullptr;
    auto* h = new mlic_dists();
    try {
      h->impl = dists_create(n, names, ptrs, shapes, ndims, (hipStream_t)stream);
    } catch (...) {
      delete h;
      throw;
    }
    *out = h;
  });
}

int mlic_dists_destroy(mlic_dists* h) {
  return guard([&] {
    if (!h) return;
    dists_destroy(h->impl);
    delete h;
  });
}

int mlic_dists_set_precision(mlic_dists* h, int precision) {
  return guard([&] {
    MLIC_CHECK(h != nullptr && h->impl != nullptr, "null mlic_dists handle");
    dists_set_precision(h->impl, precision);
  });
}

int mlic_dists_scratch_bytes(int B, int H, int W, size_t* bytes) {
  return guard([&] {
    MLIC_CHECK(bytes != nullptr, "dists_scratch_bytes: null bytes");
    *bytes = dists_scratch_bytes(B, H, W);
  });
}

int mlic_image_dists_u8(mlic_dists* h, void* stream, const float* a, const int64_t* a_strides, const float* b,
                        const int64_t* b_strides, int B, int H, int W, void* scratch, size_t scratch_bytes,
                        double* out, double* terms) {
  return guard([&] {
    MLIC_CHECK(h != nullptr && h->impl != nullptr, "null mlic_dists handle");
    const size_t need = dists_scratch_bytes(B, H, W);  // checks B, H, W
    MLIC_CHECK(a && b && a_strides && b_strides, "dists: null image or strides");
    // the images are read in place with int64 element offsets: rows must not overlap and the column stride is 1
    MLIC_CHECK(a_strides[2] >= W && b_strides[2] >= W && a_strides[1] >= 0 && b_strides[1] >= 0 &&
                   a_strides[0] >= 0 && b_strides[0] >= 0,
               "dists: bad strides (row stride below W, or a negative stride)");
    MLIC_CHECK(scratch != nullptr && scratch_bytes >= need, "dists: scratch too small (mlic_dists_scratch_bytes)");
    MLIC_CHECK(reinterpret_cast<uintptr_t>(scratch) % 256 == 0, "dists: scratch must be 256-byte aligned");
    MLIC_CHECK(out != nullptr, "dists: null out");
    dists_u8(h->impl, a, a_strides, b, b_strides, B, H, W, scratch, out, terms, (hipStream_t)stream);
  });
}

int mlic_dists_profile(mlic_dists* h, int on, double* ms3) {
  return guard([&] {
    MLIC_CHECK(h != nullptr && h->impl != nullptr, "null mlic_dists handle");
    dists_profile(h->impl, on != 0, ms3);
  });
}

int mlic_dists_range_fallbacks(mlic_dists* h, int64_t* count, int reset) {
  return guard([&] {
    MLIC_CHECK(h != nullptr && h->impl != nullptr, "null mlic_dists handle");
    const int64_t v = dists_range_fallbacks(h->impl, reset != 0);
    if (count) *count = v;
  });
}

int mlic_image_ingest_u8(void* stream, const uint8_t* src, const int64_t* src_strides, int B, int H, int W, float* dst,
                         int Hp, int Wp) {
  return guard([&] { image_ingest_u8(src, src_strides, B, H, W, dst, Hp, Wp, (hipStream_t)stream); });
}

int mlic_image_blur3_pad(void* stream, const float* src, const int32_t* src_index, int n, int H, int W, int Hp, int Wp,
                         const float* w9, float* dst) {
  return guard([&] { image_blur3_pad(src, src_index, n, H, W, Hp, Wp, w9, dst, (hipStream_t)stream); });
}

int mlic_image_egress_u8(void* stream, const float* src, const int64_t* src_strides, int B, int H, int W, uint8_t* dst,
                         const int64_t* dst_strides, const uint8_t* ref, const int64_t* ref_strides, uint64_t* sq_err) {
  return guard([&] {
    image_egress_u8(src, src_strides, B, H, W, dst, dst_strides, ref, ref_strides, sq_err, (hipStream_t)stream);
  });
}

static void container_ok(const char* err) {
  if (err) throw Error(std::string("mlic: ") + err);
}

int mlic_container_bytes(size_t y_len, size_t z_len, int vbr, size_t* bytes) {
  return guard([&] {
    MLIC_CHECK(bytes != nullptr, "container_bytes: null bytes");
    *bytes = container_bytes(y_len, z_len, vbr != 0);
  });
}

int mlic_container_write(uint32_t H, uint32_t W, int level, uint32_t hz, uint32_t wz, const uint8_t* y, size_t y_len,
                         const uint8_t* z, size_t z_len, uint8_t* out, size_t cap, size_t* len) {
  return guard([&] { container_ok(container_write(H, W, level, hz, wz, y, y_len, z, z_len, out, cap, len)); });
}

static void to_abi(const ContainerInfo& c, mlic_container_info* o) {
  o->H = c.H;
  o->W = c.W;
  o->hz = c.hz;
  o->wz = c.wz;
  o->level = c.level;
  o->reserved = 0;
  o->y_off = c.y_off;
  o->y_len = c.y_len;
  o->z_off = c.z_off;
  o->z_len = c.z_len;
}

int mlic_container_parse(const uint8_t* data, size_t n, int vbr, int n_levels, uint64_t max_pixels,
                         mlic_container_info* info) {
  return guard([&] {
    MLIC_CHECK(info != nullptr, "container_parse: null info");
    MLIC_CHECK(!vbr || n_levels >= 1, "container_parse: a VBR file needs n_levels >= 1");
    ContainerInfo c;
    container_ok(container_parse(data, n, vbr != 0, (uint32_t)std::max(n_levels, 0), max_pixels, &c));
    to_abi(c, info);
  });
}

int mlic_container_layered_bytes(size_t z_len, const size_t* layer_lens, int S, int vbr, size_t* bytes) {
  return guard([&] {
    MLIC_CHECK(bytes != nullptr && layer_lens != nullptr, "container_layered_bytes: null argument");
    MLIC_CHECK(S >= 1 && S <= (int)LAYERED_MAX_S, "container_layered_bytes: S must be in 1..32");
    *bytes = container_layered_bytes(z_len, layer_lens, (uint32_t)S, vbr != 0);
    MLIC_CHECK(*bytes != 0, "container_layered_bytes: the file does not fit size_t");
  });
}

int mlic_container_write_layered(uint32_t H, uint32_t W, int level, uint32_t hz, uint32_t wz, const uint8_t* z,
                                 size_t z_len, const uint8_t* const* layers, const size_t* layer_lens, int S,
                                 uint8_t* out, size_t cap, size_t* len) {
  return guard([&] {
    MLIC_CHECK(S >= 1 && S <= (int)LAYERED_MAX_S, "container_write_layered: S must be in 1..32");
    container_ok(container_write_layered(H, W, level, hz, wz, z, z_len, layers, layer_lens, (uint32_t)S, out, cap, len));
  });
}

int mlic_container_parse_layered(const uint8_t* data, size_t n, int n_levels, uint64_t max_pixels, int allow_truncated,
                                 mlic_container_layered_info* info) {
  return guard([&] {
    MLIC_CHECK(info != nullptr, "container_parse_layered: null info");
    LayeredInfo c;
    container_ok(container_parse_layered(data, n, (uint32_t)std::max(n_levels, 0), max_pixels, allow_truncated != 0, &c));
    info->H = c.H;
    info->W = c.W;
    info->hz = c.hz;
    info->wz = c.wz;
    info->level = c.level;
    info->S = c.S;
    info->layers_present = c.layers_present;
    info->z_off = c.z_off;
    info->z_len = c.z_len;
    for (uint32_t k = 0; k < LAYERED_MAX_S; ++k) {
      info->layer_off[k] = k < c.layers_present ? c.layer_off[k] : 0;
      info->layer_len[k] = k < c.layers_present ? c.layer_len[k] : 0;
    }
  });
}

int mlic_container_write_roi(uint32_t H, uint32_t W, int level, uint32_t hz, uint32_t wz, const uint8_t* y,
                             size_t y_len, const uint8_t* z, size_t z_len, const uint8_t* levels, uint8_t* out,
                             size_t cap, size_t* len) {
  return guard(
      [&] { container_ok(container_write_roi(H, W, level, hz, wz, y, y_len, z, z_len, levels, out, cap, len)); });
}

int mlic_container_parse_roi(const uint8_t* data, size_t n, int n_levels, uint64_t max_pixels,
                             mlic_container_roi_info* info, uint8_t* levels, size_t levels_cap) {
  return guard([&] {
    MLIC_CHECK(info != nullptr, "container_parse_roi: null info");
    ContainerInfo c;
    size_t off = 0, len = 0;
    container_ok(container_parse_roi(data, n, (uint32_t)std::max(n_levels, 0), max_pixels, &c, &off, &len));
    to_abi(c, &info->file);
    info->map_off = off;
    info->map_len = len;
    if (levels != nullptr && len != 0) {
      const uint64_t cells = (uint64_t)c.hz * c.wz;
      MLIC_CHECK(cells <= levels_cap, "container_parse_roi: levels buffer too small (h_z * w_z bytes)");
      container_roi_unpack(data + off, cells, levels);
    }
  });
}

int mlic_tile_grid(uint32_t H, uint32_t W, uint32_t T, uint32_t V, uint32_t* ny, uint32_t* nx, uint32_t* rects,
                   size_t rects_cap) {
  return guard([&] {
    MLIC_CHECK(ny != nullptr && nx != nullptr, "tile_grid: null ny or nx");
    container_ok(tile_params_check(T, V));
    MLIC_CHECK(H >= 1 && W >= 1, "tile_grid: H and W must be positive");
    const uint32_t gy = tile_count(H, T, V), gx = tile_count(W, T, V);
    *ny = gy;
    *nx = gx;
    if (rects == nullptr) return;
    MLIC_CHECK((uint64_t)gy * gx <= rects_cap, "tile_grid: rects buffer too small (ny * nx entries of 4)");
    for (uint32_t ky = 0; ky < gy; ++ky)
      for (uint32_t kx = 0; kx < gx; ++kx) {
        uint32_t* r = rects + 4 * ((size_t)ky * gx + kx);
        r[0] = tile_start(ky, T, V);
        r[1] = tile_start(kx, T, V);
        r[2] = tile_extent(H, ky, T, V);
        r[3] = tile_extent(W, kx, T, V);
      }
  });
}

int mlic_image_tile_blend_u8(void* stream, const float* const* tiles_dev, const float* const* tiles_host, int H, int W,
                             int T, int V, int y0, int x0, int h, int w, uint8_t* dst, const int64_t* dst_strides,
                             const uint8_t* ref, const int64_t* ref_strides, uint64_t* sq_err) {
  return guard([&] {
    image_tile_blend_u8(tiles_dev, tiles_host, H, W, T, V, y0, x0, h, w, dst, dst_strides, ref, ref_strides, sq_err,
                        (hipStream_t)stream);
  });
}

int mlic_container_write_tiled(uint32_t H, uint32_t W, uint32_t T, uint32_t V, int vbr, const uint8_t* payload,
                               const uint64_t* lens, size_t n_tiles, uint8_t* out, size_t cap, size_t* len) {
  return guard([&] { container_ok(container_write_tiled(H, W, T, V, vbr != 0, payload, lens, n_tiles, out, cap, len)); });
}

static TiledInfo from_abi(const mlic_container_tiled_info& o) {
  TiledInfo t{};
  t.H = o.H, t.W = o.W, t.T = o.T, t.V = o.V, t.ny = o.ny, t.nx = o.nx;
  t.vbr = o.vbr != 0;
  t.table_off = (size_t)o.table_off, t.payload_off = (size_t)o.payload_off, t.payload_len = (size_t)o.payload_len;
  return t;
}

int mlic_container_parse_tiled(const uint8_t* data, size_t n, uint64_t max_pixels, mlic_container_tiled_info* info) {
  return guard([&] {
    MLIC_CHECK(info != nullptr, "container_parse_tiled: null info");
    TiledInfo t;
    container_ok(container_parse_tiled(data, n, max_pixels, &t));
    *info = mlic_container_tiled_info{t.H, t.W, t.T, t.V, t.ny, t.nx, t.vbr ? 1 : 0, 0,
                                      t.table_off, t.payload_off, t.payload_len};
  });
}

int mlic_container_tiled_tile(const uint8_t* data, size_t n, const mlic_container_tiled_info* info, uint64_t k,
                              uint64_t* off, uint64_t* len) {
  return guard([&] {
    MLIC_CHECK(info != nullptr && off != nullptr && len != nullptr, "container_tiled_tile: null argument");
    const TiledInfo t = from_abi(*info);
    size_t o = 0, l = 0;
    container_ok(container_tiled_tile(data, n, &t, k, &o, &l));
    *off = o;
    *len = l;
  });
}

// the handle's staging image: at least `bytes`, grown by reallocation (hipFree waits for the device)
static float* grow(float*& buf, size_t& have, size_t bytes) {
  if (have < bytes) {
    if (buf) HIP_OK(hipFree(buf));
    buf = nullptr;
    have = 0;
    HIP_OK(hipMalloc((void**)&buf, bytes));
    have = bytes;
  }
  return buf;
}
static float* stage(mlic_model* m, size_t bytes) { return grow(m->stage, m->stage_bytes, bytes); }
static float* stage2(mlic_model* m, size_t bytes) { return grow(m->stage2, m->stage2_bytes, bytes); }

// the file of the handle's last one-image encode
static void write_encoded(mlic_model* m, Model& mod, uint8_t* out, size_t cap, size_t* len) {
  const EncodedImage& e = mod.encoded(0);
  container_ok(container_write((uint32_t)m->enc_H, (uint32_t)m->enc_W, m->enc_level, (uint32_t)((m->enc_H + 63) / 64),
                               (uint32_t)((m->enc_W + 63) / 64), reinterpret_cast<const uint8_t*>(e.y.data()),
                               e.y.size(), reinterpret_cast<const uint8_t*>(e.z.data()), e.z.size(), out, cap, len));
}

int mlic_encode_image_u8(mlic_model* m, void* stream, const uint8_t* rgb_dev, const int64_t* strides, int H, int W,
                         float vbr_scale, int level, uint8_t* out, size_t cap, size_t* len) {
  return guard([&] {
    Model& mod = impl(m);
    MLIC_CHECK(len != nullptr, "encode_image_u8: null len");
    if (rgb_dev != nullptr) {
      MLIC_CHECK(strides != nullptr && H >= 1 && W >= 1, "encode_image_u8: strides, H >= 1 and W >= 1 expected");
      MLIC_CHECK(H <= (1 << 24) && W <= (1 << 24), "encode_image_u8: image side above 2^24");
      const int Hp = (H + 63) / 64 * 64, Wp = (W + 63) / 64 * 64;
      const int64_t s4[4] = {0, strides[0], strides[1], strides[2]};
      m->enc_H = m->sc_H = 0;
      float* x = stage(m, sizeof(float) * 3 * (size_t)Hp * (size_t)Wp);
      image_ingest_u8(rgb_dev, s4, 1, H, W, x, Hp, Wp, (hipStream_t)stream);
      const float sc[1] = {vbr_scale};
      mod.compress(x, 1, Hp, Wp, sc, (hipStream_t)stream);
      m->enc_H = H;
      m->enc_W = W;
      m->enc_level = level < 0 ? -1 : level;
      m->enc_passes = 0;
    }
    MLIC_CHECK(m->enc_H > 0, "encode_image_u8: rgb_dev is NULL and the handle has no encoded image");
    write_encoded(m, mod, out, cap, len);
  });
}

int mlic_encode_image_u8_budget(mlic_model* m, void* stream, const uint8_t* rgb_dev, const int64_t* strides, int H,
                                int W, float vbr_scale, int level, double max_bpp, int max_passes, uint8_t* out,
                                size_t cap, size_t* len, int* passes) {
  return guard([&] {
    Model& mod = impl(m);
    MLIC_CHECK(len != nullptr, "encode_image_u8_budget: null len");
    if (rgb_dev != nullptr) {
      MLIC_CHECK(strides != nullptr && H >= 1 && W >= 1, "encode_image_u8_budget: strides, H >= 1 and W >= 1 expected");
      MLIC_CHECK(H <= (1 << 24) && W <= (1 << 24), "encode_image_u8_budget: image side above 2^24");
      MLIC_CHECK(max_bpp > 0 && std::isfinite(max_bpp), "encode_image_u8_budget: max_bpp must be positive and finite");
      MLIC_CHECK(max_passes >= 0, "encode_image_u8_budget: max_passes must not be negative");
      const int Hp = (H + 63) / 64 * 64, Wp = (W + 63) / 64 * 64;
      const size_t bytes = sizeof(float) * 3 * (size_t)Hp * (size_t)Wp;
      const int64_t s4[4] = {0, strides[0], strides[1], strides[2]};
      const float sc[1] = {vbr_scale};
      m->enc_H = m->sc_H = 0;
      float* x = stage(m, bytes);
      image_ingest_u8(rgb_dev, s4, 1, H, W, x, Hp, Wp, (hipStream_t)stream);
      int k = 0;
      for (;;) {
        mod.compress(x, 1, Hp, Wp, sc, (hipStream_t)stream);  // returns with the strings complete
        const EncodedImage& e = mod.encoded(0);
        const double bpp = 8.0 * (double)container_bytes(e.y.size(), e.z.size(), level >= 0) / ((double)H * (double)W);
        if (!(bpp > max_bpp) || k >= max_passes) break;
        float* y = x == m->stage ? stage2(m, bytes) : m->stage;
        image_blur3_pad(x, nullptr, 1, H, W, Hp, Wp, nullptr, y, (hipStream_t)stream);
        x = y;
        ++k;
      }
      m->enc_H = H;
      m->enc_W = W;
      m->enc_level = level < 0 ? -1 : level;
      m->enc_passes = k;
    }
    MLIC_CHECK(m->enc_H > 0, "encode_image_u8_budget: rgb_dev is NULL and the handle has no encoded image");
    if (passes) *passes = m->enc_passes;
    write_encoded(m, mod, out, cap, len);
  });
}

int mlic_decode_image_u8(mlic_model* m, void* stream, const uint8_t* file, size_t n, int n_levels, uint64_t max_pixels,
                         const float* vbr_gains, uint8_t* rgb_dev, const int64_t* strides, size_t cap_bytes, int* H,
                         int* W, int* level) {
  return guard([&] {
    MLIC_CHECK(file != nullptr || n == 0, "decode_image_u8: null file");
    const bool vbr = n_levels > 0;
    ContainerInfo c;
    // 2^24 pixels a side at most (the int sizes of this ABI), whatever max_pixels allows
    container_ok(container_parse(file, n, vbr, (uint32_t)std::max(n_levels, 0), max_pixels, &c));
    MLIC_CHECK(c.H <= (1u << 24) && c.W <= (1u << 24), "decode_image_u8: image side above 2^24");
    if (H) *H = (int)c.H;
    if (W) *W = (int)c.W;
    if (level) *level = c.level;
    if (rgb_dev == nullptr) return;
    Model& mod = impl(m);
    MLIC_CHECK(strides != nullptr && strides[0] >= 0 && strides[1] > 0 && strides[2] > 0,
               "decode_image_u8: strides {row, column, channel} must be non-negative, column and channel nonzero");
    const uint64_t extent = 1 + (uint64_t)(c.H - 1) * (uint64_t)strides[0] + (uint64_t)(c.W - 1) * (uint64_t)strides[1] +
                            2 * (uint64_t)strides[2];
    MLIC_CHECK(extent <= cap_bytes, "decode_image_u8: the file's image does not fit cap_bytes");
    const int Hp = (int)c.hz * 64, Wp = (int)c.wz * 64;
    float* x = stage(m, sizeof(float) * 3 * (size_t)Hp * (size_t)Wp);
    const uint8_t* ys[1] = {file + c.y_off};
    const uint8_t* zs[1] = {file + c.z_off};
    const size_t yl[1] = {c.y_len}, zl[1] = {c.z_len};
    const float sc[1] = {vbr && vbr_gains ? vbr_gains[c.level] : 1.0f};
    mod.decompress(ys, yl, zs, zl, 1, (int)c.hz, (int)c.wz, x, sc, (hipStream_t)stream);
    const int64_t s3[3] = {0, (int64_t)Hp * Wp, Wp};
    const int64_t d4[4] = {0, strides[0], strides[1], strides[2]};
    image_egress_u8(x, s3, 1, (int)c.H, (int)c.W, rgb_dev, d4, nullptr, nullptr, nullptr, (hipStream_t)stream);
  });
}

// ---- scaled coding (DESIGN.md section 5 "Scaled coding")
int mlic_resample_table(int filter, int Li, int Lo, int32_t* start, int32_t* count, float* weights, int stride,
                        int* taps) {
  return guard([&] { container_ok(resample_table(filter, Li, Lo, start, count, weights, stride, taps)); });
}

int mlic_image_ingest_u8_scaled(void* stream, const uint8_t* src, const int64_t* src_strides, int B, int Hi, int Wi,
                                int filter, int h, int w, float* dst, int Hp, int Wp) {
  return guard(
      [&] { image_ingest_u8_scaled(src, src_strides, B, Hi, Wi, filter, h, w, dst, Hp, Wp, (hipStream_t)stream); });
}

int mlic_image_egress_u8_scaled(void* stream, const float* src, const int64_t* src_strides, int B, int h, int w,
                                int filter, int Ho, int Wo, uint8_t* dst, const int64_t* dst_strides, const uint8_t* ref,
                                const int64_t* ref_strides, uint64_t* sq_err) {
  return guard([&] {
    image_egress_u8_scaled(src, src_strides, B, h, w, filter, Ho, Wo, dst, dst_strides, ref, ref_strides, sq_err,
                           (hipStream_t)stream);
  });
}

int mlic_container_write_scaled(uint32_t H, uint32_t W, int vbr, int filter, const uint8_t* inner, size_t inner_len,
                                uint8_t* out, size_t cap, size_t* len) {
  return guard([&] {
    MLIC_CHECK(filter >= 0, "container_write_scaled: negative filter");
    container_ok(container_write_scaled(H, W, vbr != 0, (uint32_t)filter, inner, inner_len, out, cap, len));
  });
}

int mlic_container_parse_scaled(const uint8_t* data, size_t n, int n_levels, uint64_t max_pixels,
                                mlic_container_scaled_info* info) {
  return guard([&] {
    MLIC_CHECK(info != nullptr, "container_parse_scaled: null info");
    ScaledInfo s;
    container_ok(container_parse_scaled(data, n, (uint32_t)std::max(n_levels, 0), max_pixels, &s));
    info->H = s.H;
    info->W = s.W;
    info->filter = (int32_t)s.filter;
    info->vbr = s.vbr ? 1 : 0;
    info->inner_off = s.inner_off;
    info->inner_len = s.inner_len;
    to_abi(s.inner, &info->inner);
  });
}

// ---- residual coding (DESIGN.md section 5 "Residual coding")
int mlic_image_residual_front_u8(void* stream, const uint8_t* base, const int64_t* base_strides, const uint8_t* x,
                                 const int64_t* x_strides, int B, int H, int W, int tau, uint8_t* ctx,
                                 uint32_t* ctx_count, uint64_t* digest, int16_t* sym, uint32_t* hist, uint32_t* max_err) {
  return guard([&] {
    image_residual_front_u8(base, base_strides, x, x_strides, B, H, W, tau, ctx, ctx_count, digest, sym, hist, max_err,
                            (hipStream_t)stream);
  });
}

int mlic_image_residual_apply_u8(void* stream, const uint8_t* base, const int64_t* base_strides, const int16_t* sym,
                                 int B, int H, int W, int tau, uint8_t* out, const int64_t* out_strides,
                                 const uint8_t* ref, const int64_t* ref_strides, uint64_t* sq_err, uint32_t* max_err) {
  return guard([&] {
    image_residual_apply_u8(base, base_strides, sym, B, H, W, tau, out, out_strides, ref, ref_strides, sq_err, max_err,
                            (hipStream_t)stream);
  });
}

int mlic_residual_tables(const uint32_t* hist, uint8_t* m, uint16_t* freq, int32_t* cdf, int32_t* cdf_len,
                         int32_t* offset) {
  return guard([&] {
    MLIC_CHECK(hist != nullptr, "residual_tables: null hist");
    MLIC_CHECK(m != nullptr, "residual_tables: null m");
    MLIC_CHECK((cdf != nullptr) == (cdf_len != nullptr) && (cdf != nullptr) == (offset != nullptr),
               "residual_tables: cdf, cdf_len and offset go together");
    for (int k = 0; k < RES_CTX; ++k) {
      const uint32_t* h = hist + (size_t)k * RES_BINS;
      uint64_t total = 0;
      int mk = 0;
      for (int j = 0; j < RES_BINS; ++j) {
        total += h[j];
        if (j != RES_ESCAPE_BIN && h[j]) mk = std::max(mk, std::abs(j - RES_MAX_M));
      }
      if (cdf) {
        std::fill(cdf + (size_t)k * RES_CDF_STRIDE, cdf + (size_t)(k + 1) * RES_CDF_STRIDE, 0);
        cdf_len[k] = 0;
        offset[k] = 0;
      }
      if (freq) std::fill(freq + (size_t)k * RES_BINS, freq + (size_t)(k + 1) * RES_BINS, (uint16_t)0);
      if (total == 0) {
        m[k] = RES_ABSENT;
        continue;
      }
      m[k] = (uint8_t)mk;
      std::vector<float> pmf((size_t)2 * mk + 2);
      for (int j = -mk; j <= mk; ++j) pmf[(size_t)(j + mk)] = (float)h[j + RES_MAX_M] / (float)total;
      pmf[(size_t)2 * mk + 1] = (float)h[RES_ESCAPE_BIN] / (float)total;
      const auto c = pmf_to_quantized_cdf(pmf.data(), (int)pmf.size(), 16);
      MLIC_CHECK(c.size() == pmf.size() + 1 && c.front() == 0 && c.back() == 65536, "residual_tables: bad CDF");
      for (size_t j = 0; j + 1 < c.size(); ++j) {
        MLIC_CHECK(c[j + 1] > c[j], "residual_tables: a zero frequency");
        if (freq) freq[(size_t)k * RES_BINS + j] = (uint16_t)(c[j + 1] - c[j]);
      }
      if (cdf) {
        for (size_t j = 0; j < c.size(); ++j) cdf[(size_t)k * RES_CDF_STRIDE + j] = (int32_t)c[j];
        cdf_len[k] = (int32_t)c.size();
        offset[k] = -mk;
      }
    }
  });
}

int mlic_container_write_residual(uint32_t H, uint32_t W, int vbr, int tau, uint64_t digest, const uint8_t* m,
                                  const uint16_t* freq, const uint8_t* inner, size_t inner_len, const uint8_t* res,
                                  size_t res_len, uint8_t* out, size_t cap, size_t* len) {
  return guard([&] {
    MLIC_CHECK(tau >= 0, "container_write_residual: negative tau");
    container_ok(container_write_residual(H, W, vbr != 0, (uint32_t)tau, digest, m, freq, inner, inner_len, res, res_len,
                                          out, cap, len));
  });
}

int mlic_container_parse_residual(const uint8_t* data, size_t n, int n_levels, uint64_t max_pixels,
                                  mlic_container_residual_info* info) {
  return guard([&] {
    MLIC_CHECK(info != nullptr, "container_parse_residual: null info");
    ResidualInfo s;
    container_ok(container_parse_residual(data, n, (uint32_t)std::max(n_levels, 0), max_pixels, &s));
    info->H = s.H;
    info->W = s.W;
    info->tau = (int32_t)s.tau;
    info->vbr = s.vbr ? 1 : 0;
    info->digest = s.digest;
    for (uint32_t k = 0; k < RESIDUAL_CTX; ++k) {
      info->m[k] = s.m[k];
      info->freq_off[k] = s.freq_off[k];
    }
    info->inner_off = s.inner_off;
    info->inner_len = s.inner_len;
    info->res_off = s.res_off;
    info->res_len = s.res_len;
    to_abi(s.inner, &info->inner);
  });
}

// ---- segmented residual strings (residual_seg.h; DESIGN.md section 5 "Residual coding", "Segments")
namespace {
struct SegScratch {  // the device entries' scratch: tables | seg_off | seg_bytes | total | status
  size_t tabs, off, bytes, total, status, size;
  SegScratch(int B, int64_t n_seg) {
    auto up = [](size_t v) { return (v + 15) / 16 * 16; };
    tabs = 0;
    off = up((size_t)B * std::max(sizeof(ResSegEncTable), sizeof(ResSegDecTable)));
    bytes = up(off + sizeof(uint32_t) * (size_t)B * n_seg);
    total = up(bytes + sizeof(uint32_t) * (size_t)B * n_seg);
    status = up(total + sizeof(uint64_t) * (size_t)B);
    size = up(status + sizeof(uint32_t) * (size_t)B);
  }
};

void seg_status_throw(const char* what, const std::vector<uint32_t>& st) {
  for (size_t b = 0; b < st.size(); ++b)
    if (st[b] != RES_SEG_CLEAN)
      throw Error(std::string("mlic: ") + what + ": image " + std::to_string(b) + ", segment " +
                  std::to_string(st[b] >> 4) + ": " + residual_seg_reason(st[b] & 15u));
}

bool aligned_to(const void* p, uintptr_t a) { return reinterpret_cast<uintptr_t>(p) % a == 0; }
}  // namespace

int mlic_residual_segments_scratch_bytes(int B, int64_t n_seg, size_t* bytes) {
  return guard([&] {
    MLIC_CHECK(bytes != nullptr, "residual_segments_scratch_bytes: null bytes");
    MLIC_CHECK(B >= 1 && n_seg >= 1 && n_seg <= RES_SEG_MAX_N / RES_SEG_MIN,
               "residual_segments_scratch_bytes: B >= 1 and 1 <= n_seg <= 2^21 expected");
    *bytes = SegScratch(B, n_seg).size;
  });
}

namespace {
// the four entries below, for a string of N samples; `check` is residual_seg_check or residual_seg_check_n
void seg_encode_dev(const std::string& w, const std::function<void()>& check, void* stream, const int16_t* sym, const uint8_t* ctx, int B,
                    int64_t N, const uint8_t* m, const uint16_t* freq, int seg_len, int64_t n_seg, uint8_t* out,
                    size_t cap, uint32_t* seg_bytes, uint64_t* len, void* scratch, size_t scratch_bytes,
                    uint32_t* status) {
  const char* what = w.c_str();
  MLIC_CHECK(sym != nullptr, w + ": null sym");
  MLIC_CHECK(ctx != nullptr, w + ": null ctx");
  MLIC_CHECK(out != nullptr, w + ": null out");
  MLIC_CHECK(seg_bytes != nullptr, w + ": null seg_bytes");
  MLIC_CHECK(len != nullptr, w + ": null len");
  MLIC_CHECK(scratch != nullptr, w + ": null scratch");
  check();
  residual_seg_tables_check(what, m, freq, B);
  MLIC_CHECK(cap % 4 == 0, w + ": the capacity must be a multiple of 4");
  MLIC_CHECK(cap >= (size_t)RES_SEG_MIN_BYTES * (size_t)n_seg,
             w + ": the capacity is too small (below 8 bytes a segment)");
  MLIC_CHECK(cap <= 0xffffffffu, w + ": the capacity must fit 32 bits");
  const SegScratch sc(B, n_seg);
  MLIC_CHECK(scratch_bytes >= sc.size, w + ": scratch too small");
  MLIC_CHECK(aligned_to(sym, 2) && aligned_to(out, 4) && aligned_to(seg_bytes, 4) && aligned_to(scratch, 16),
             w + ": sym must be 2-byte, out and seg_bytes 4-byte, scratch 16-byte aligned");
  std::vector<ResSegEncTable> tabs((size_t)B);
  for (int b = 0; b < B; ++b)
    residual_seg_enc_table(m + (size_t)b * RES_CTX, freq + (size_t)b * RES_CTX * RES_BINS, &tabs[(size_t)b]);
  auto st = (hipStream_t)stream;
  auto* base = static_cast<uint8_t*>(scratch);
  auto* d_tabs = reinterpret_cast<ResSegEncTable*>(base + sc.tabs);
  auto* d_status = reinterpret_cast<uint32_t*>(base + sc.status);
  auto* d_total = reinterpret_cast<uint64_t*>(base + sc.total);
  HIP_OK(hipMemcpyAsync(d_tabs, tabs.data(), sizeof(ResSegEncTable) * (size_t)B, hipMemcpyHostToDevice, st));
  residual_encode_segments(sym, ctx, B, N, seg_len, n_seg, d_tabs, out, cap, reinterpret_cast<uint32_t*>(base + sc.off),
                           seg_bytes, d_total, d_status, st);
  std::vector<uint32_t> hs((size_t)B);
  HIP_OK(hipMemcpyAsync(hs.data(), d_status, sizeof(uint32_t) * (size_t)B, hipMemcpyDeviceToHost, st));
  HIP_OK(hipMemcpyAsync(len, d_total, sizeof(uint64_t) * (size_t)B, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if (status) std::copy(hs.begin(), hs.end(), status);
  seg_status_throw(what, hs);
}

void seg_decode_dev(const std::string& w, const std::function<void()>& check, void* stream, const uint8_t* data, size_t data_stride,
                    const uint64_t* data_len, const uint32_t* seg_bytes, const uint8_t* ctx, int B, int64_t N,
                    const uint8_t* m, const uint16_t* freq, int seg_len, int64_t n_seg, int16_t* sym, void* scratch,
                    size_t scratch_bytes, uint32_t* status) {
  const char* what = w.c_str();
  MLIC_CHECK(data != nullptr, w + ": null data");
  MLIC_CHECK(ctx != nullptr, w + ": null ctx");
  MLIC_CHECK(sym != nullptr, w + ": null sym");
  MLIC_CHECK(scratch != nullptr, w + ": null scratch");
  check();
  residual_seg_tables_check(what, m, freq, B);
  MLIC_CHECK(data_stride % 4 == 0, w + ": the data stride must be a multiple of 4");
  residual_seg_lengths_check(what, seg_bytes, data_len, data_stride, B, N, seg_len, n_seg);
  const SegScratch sc(B, n_seg);
  MLIC_CHECK(scratch_bytes >= sc.size, w + ": scratch too small");
  MLIC_CHECK(aligned_to(sym, 2) && aligned_to(data, 4) && aligned_to(scratch, 16),
             w + ": sym must be 2-byte, data 4-byte, scratch 16-byte aligned");
  std::vector<ResSegDecTable> tabs((size_t)B);
  std::vector<uint32_t> offs((size_t)B * n_seg);
  for (int b = 0; b < B; ++b) {
    residual_seg_dec_table(m + (size_t)b * RES_CTX, freq + (size_t)b * RES_CTX * RES_BINS, &tabs[(size_t)b]);
    uint32_t o = 0;
    for (int64_t k = 0; k < n_seg; ++k) {
      offs[(size_t)b * n_seg + k] = o;
      o += seg_bytes[(size_t)b * n_seg + k];
    }
  }
  auto st = (hipStream_t)stream;
  auto* base = static_cast<uint8_t*>(scratch);
  auto* d_tabs = reinterpret_cast<ResSegDecTable*>(base + sc.tabs);
  auto* d_off = reinterpret_cast<uint32_t*>(base + sc.off);
  auto* d_bytes = reinterpret_cast<uint32_t*>(base + sc.bytes);
  auto* d_status = reinterpret_cast<uint32_t*>(base + sc.status);
  HIP_OK(hipMemcpyAsync(d_tabs, tabs.data(), sizeof(ResSegDecTable) * (size_t)B, hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_off, offs.data(), sizeof(uint32_t) * offs.size(), hipMemcpyHostToDevice, st));
  HIP_OK(hipMemcpyAsync(d_bytes, seg_bytes, sizeof(uint32_t) * offs.size(), hipMemcpyHostToDevice, st));
  residual_decode_segments(data, data_stride, d_off, d_bytes, ctx, B, N, seg_len, n_seg, d_tabs, sym, d_status, st);
  std::vector<uint32_t> hs((size_t)B);
  HIP_OK(hipMemcpyAsync(hs.data(), d_status, sizeof(uint32_t) * (size_t)B, hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if (status) std::copy(hs.begin(), hs.end(), status);
  seg_status_throw(what, hs);
}

void seg_encode_host(const std::string& w, const std::function<void()>& check, const int16_t* sym, const uint8_t* ctx, int B, int64_t N,
                     const uint8_t* m, const uint16_t* freq, int seg_len, int64_t n_seg, uint8_t* out, size_t cap,
                     uint32_t* seg_bytes, uint64_t* len) {
  MLIC_CHECK(sym != nullptr, w + ": null sym");
  MLIC_CHECK(ctx != nullptr, w + ": null ctx");
  MLIC_CHECK(seg_bytes != nullptr, w + ": null seg_bytes");
  MLIC_CHECK(len != nullptr, w + ": null len");
  check();
  residual_seg_tables_check(w.c_str(), m, freq, B);
  if (out != nullptr) {
    MLIC_CHECK(cap % 4 == 0, w + ": the capacity must be a multiple of 4");
    MLIC_CHECK(cap >= (size_t)RES_SEG_MIN_BYTES * (size_t)n_seg,
               w + ": the capacity is too small (below 8 bytes a segment)");
  }
  residual_seg_encode_host_n(w.c_str(), sym, ctx, B, N, m, freq, seg_len, n_seg, out, cap, seg_bytes, len);
}

void seg_decode_host(const std::string& w, const std::function<void()>& check, const uint8_t* data, size_t data_stride,
                     const uint64_t* data_len, const uint32_t* seg_bytes, const uint8_t* ctx, int B, int64_t N,
                     const uint8_t* m, const uint16_t* freq, int seg_len, int64_t n_seg, int16_t* sym) {
  MLIC_CHECK(data != nullptr, w + ": null data");
  MLIC_CHECK(ctx != nullptr, w + ": null ctx");
  MLIC_CHECK(sym != nullptr, w + ": null sym");
  check();
  residual_seg_tables_check(w.c_str(), m, freq, B);
  MLIC_CHECK(data_stride % 4 == 0, w + ": the data stride must be a multiple of 4");
  residual_seg_lengths_check(w.c_str(), seg_bytes, data_len, data_stride, B, N, seg_len, n_seg);
  residual_seg_decode_host_n(w.c_str(), data, data_stride, data_len, seg_bytes, ctx, B, N, m, freq, seg_len, n_seg, sym);
}
}  // namespace

int mlic_residual_encode_segments(void* stream, const int16_t* sym, const uint8_t* ctx, int B, int H, int W,
                                  const uint8_t* m, const uint16_t* freq, int seg_len, int64_t n_seg, uint8_t* out,
                                  size_t cap, uint32_t* seg_bytes, uint64_t* len, void* scratch, size_t scratch_bytes,
                                  uint32_t* status) {
  return guard([&] {
    seg_encode_dev("residual_encode_segments", [&] { residual_seg_check("residual_encode_segments", B, H, W, seg_len, n_seg); },
                   stream, sym, ctx, B, 3 * (int64_t)H * W, m, freq, seg_len, n_seg, out, cap, seg_bytes, len, scratch,
                   scratch_bytes, status);
  });
}

int mlic_residual_decode_segments(void* stream, const uint8_t* data, size_t data_stride, const uint64_t* data_len,
                                  const uint32_t* seg_bytes, const uint8_t* ctx, int B, int H, int W, const uint8_t* m,
                                  const uint16_t* freq, int seg_len, int64_t n_seg, int16_t* sym, void* scratch,
                                  size_t scratch_bytes, uint32_t* status) {
  return guard([&] {
    seg_decode_dev("residual_decode_segments", [&] { residual_seg_check("residual_decode_segments", B, H, W, seg_len, n_seg); },
                   stream, data, data_stride, data_len, seg_bytes, ctx, B, 3 * (int64_t)H * W, m, freq, seg_len, n_seg,
                   sym, scratch, scratch_bytes, status);
  });
}

int mlic_residual_encode_segments_host(const int16_t* sym, const uint8_t* ctx, int B, int H, int W, const uint8_t* m,
                                       const uint16_t* freq, int seg_len, int64_t n_seg, uint8_t* out, size_t cap,
                                       uint32_t* seg_bytes, uint64_t* len) {
  return guard([&] {
    seg_encode_host("residual_encode_segments_host",
                    [&] { residual_seg_check("residual_encode_segments_host", B, H, W, seg_len, n_seg); }, sym, ctx, B,
                    3 * (int64_t)H * W, m, freq, seg_len, n_seg, out, cap, seg_bytes, len);
  });
}

int mlic_residual_decode_segments_host(const uint8_t* data, size_t data_stride, const uint64_t* data_len,
                                       const uint32_t* seg_bytes, const uint8_t* ctx, int B, int H, int W,
                                       const uint8_t* m, const uint16_t* freq, int seg_len, int64_t n_seg,
                                       int16_t* sym) {
  return guard([&] {
    seg_decode_host("residual_decode_segments_host",
                    [&] { residual_seg_check("residual_decode_segments_host", B, H, W, seg_len, n_seg); }, data,
                    data_stride, data_len, seg_bytes, ctx, B, 3 * (int64_t)H * W, m, freq, seg_len, n_seg, sym);
  });
}

// the same four for a string of N samples (a Y'CbCr frame's N = H W + 2 hc wc: residual_yuv.h)
int mlic_residual_segments_scratch_bytes_n(int B, int64_t N, int seg_len, size_t* bytes) {
  return guard([&] {
    MLIC_CHECK(bytes != nullptr, "residual_segments_scratch_bytes_n: null bytes");
    MLIC_CHECK(seg_len >= RES_SEG_MIN && seg_len <= RES_SEG_MAX,
               "residual_segments_scratch_bytes_n: the segment length is outside 256..65536");
    residual_seg_check_n("residual_segments_scratch_bytes_n", B, N, seg_len, residual_n_seg(N, seg_len));
    *bytes = SegScratch(B, residual_n_seg(N, seg_len)).size;
  });
}

int mlic_residual_encode_segments_n(void* stream, const int16_t* sym, const uint8_t* ctx, int B, int64_t N,
                                    const uint8_t* m, const uint16_t* freq, int seg_len, int64_t n_seg, uint8_t* out,
                                    size_t cap, uint32_t* seg_bytes, uint64_t* len, void* scratch,
                                    size_t scratch_bytes, uint32_t* status) {
  return guard([&] {
    seg_encode_dev("residual_encode_segments_n", [&] { residual_seg_check_n("residual_encode_segments_n", B, N, seg_len, n_seg); },
                   stream, sym, ctx, B, N, m, freq, seg_len, n_seg, out, cap, seg_bytes, len, scratch, scratch_bytes,
                   status);
  });
}

int mlic_residual_decode_segments_n(void* stream, const uint8_t* data, size_t data_stride, const uint64_t* data_len,
                                    const uint32_t* seg_bytes, const uint8_t* ctx, int B, int64_t N, const uint8_t* m,
                                    const uint16_t* freq, int seg_len, int64_t n_seg, int16_t* sym, void* scratch,
                                    size_t scratch_bytes, uint32_t* status) {
  return guard([&] {
    seg_decode_dev("residual_decode_segments_n", [&] { residual_seg_check_n("residual_decode_segments_n", B, N, seg_len, n_seg); },
                   stream, data, data_stride, data_len, seg_bytes, ctx, B, N, m, freq, seg_len, n_seg, sym, scratch,
                   scratch_bytes, status);
  });
}

int mlic_residual_encode_segments_host_n(const int16_t* sym, const uint8_t* ctx, int B, int64_t N, const uint8_t* m,
                                         const uint16_t* freq, int seg_len, int64_t n_seg, uint8_t* out, size_t cap,
                                         uint32_t* seg_bytes, uint64_t* len) {
  return guard([&] {
    seg_encode_host("residual_encode_segments_host_n",
                    [&] { residual_seg_check_n("residual_encode_segments_host_n", B, N, seg_len, n_seg); }, sym, ctx, B,
                    N, m, freq, seg_len, n_seg, out, cap, seg_bytes, len);
  });
}

int mlic_residual_decode_segments_host_n(const uint8_t* data, size_t data_stride, const uint64_t* data_len,
                                         const uint32_t* seg_bytes, const uint8_t* ctx, int B, int64_t N,
                                         const uint8_t* m, const uint16_t* freq, int seg_len, int64_t n_seg,
                                         int16_t* sym) {
  return guard([&] {
    seg_decode_host("residual_decode_segments_host_n",
                    [&] { residual_seg_check_n("residual_decode_segments_host_n", B, N, seg_len, n_seg); }, data,
                    data_stride, data_len, seg_bytes, ctx, B, N, m, freq, seg_len, n_seg, sym);
  });
}

int mlic_container_write_residual_seg(uint32_t H, uint32_t W, int vbr, int tau, uint64_t digest, const uint8_t* m,
                                      const uint16_t* freq, uint32_t seg_len, uint32_t n_seg, const uint32_t* seg_bytes,
                                      const uint8_t* inner, size_t inner_len, const uint8_t* segs, size_t segs_len,
                                      uint8_t* out, size_t cap, size_t* len) {
  return guard([&] {
    MLIC_CHECK(tau >= 0, "container_write_residual_seg: negative tau");
    container_ok(container_write_residual_seg(H, W, vbr != 0, (uint32_t)tau, digest, m, freq, seg_len, n_seg, seg_bytes,
                                              inner, inner_len, segs, segs_len, out, cap, len));
  });
}

extern "C++" {  // a template cannot have C linkage
// the fields every segmented residual file has, into its ABI struct (the "MLR2", "MLR3" or "MLR4" one)
template <typename Abi>
static void seg_to_abi(const ResidualSegInfo& s, Abi* info) {
  info->H = s.H;
  info->W = s.W;
  info->tau = (int32_t)s.tau;
  info->vbr = s.vbr ? 1 : 0;
  info->digest = s.digest;
  for (uint32_t k = 0; k < RESIDUAL_CTX; ++k) {
    info->m[k] = s.m[k];
    info->freq_off[k] = s.freq_off[k];
  }
  info->seg_len = s.seg_len;
  info->n_seg = s.n_seg;
  info->inner_off = s.inner_off;
  info->inner_len = s.inner_len;
  info->res_off = s.res_off;
  info->res_len = s.res_len;
  info->index_off = s.index_off;
  info->data_off = s.data_off;
  info->data_len = s.data_len;
  to_abi(s.inner, &info->inner);
}
}  // extern "C++"

int mlic_container_parse_residual_seg(const uint8_t* data, size_t n, int n_levels, uint64_t max_pixels,
                                      mlic_container_residual_seg_info* info) {
  return guard([&] {
    MLIC_CHECK(info != nullptr, "container_parse_residual_seg: null info");
    ResidualSegInfo s;
    container_ok(container_parse_residual_seg(data, n, (uint32_t)std::max(n_levels, 0), max_pixels, &s));
    seg_to_abi(s, info);
  });
}

// ---- residual coding of 9..16-bit samples (residual16.h; DESIGN.md section 5 "Residual coding", "Deep samples")
int mlic_image_residual_front_u16(void* stream, const uint16_t* base, const int64_t* base_strides, const uint16_t* x,
                                  const int64_t* x_strides, int B, int H, int W, int depth, int tau, int shift,
                                  uint8_t* ctx, uint32_t* ctx_count, uint64_t* digest, int16_t* sym, uint64_t* lo_plane,
                                  uint32_t* hist, uint32_t* max_err, uint32_t* max_abs_q, uint64_t* sum_abs_q) {
  return guard([&] {
    image_residual_front_u16(base, base_strides, x, x_strides, B, H, W, depth, tau, shift, ctx, ctx_count, digest, sym,
                             lo_plane, hist, max_err, max_abs_q, sum_abs_q, (hipStream_t)stream);
  });
}

int mlic_image_residual_stats_u16(void* stream, const uint16_t* base, const int64_t* base_strides, const uint16_t* x,
                                  const int64_t* x_strides, int B, int H, int W, int depth, int tau,
                                  uint32_t* max_abs_q, uint64_t* sum_abs_q) {
  return guard([&] {
    image_residual_stats_u16(base, base_strides, x, x_strides, B, H, W, depth, tau, max_abs_q, sum_abs_q,
                             (hipStream_t)stream);
  });
}

int mlic_image_residual_apply_u16(void* stream, const uint16_t* base, const int64_t* base_strides, const int16_t* sym,
                                  const uint64_t* lo_plane, int B, int H, int W, int depth, int tau, int shift,
                                  uint16_t* out, const int64_t* out_strides, const uint16_t* ref,
                                  const int64_t* ref_strides, uint64_t* sq_err, uint32_t* max_err, uint32_t* status) {
  return guard([&] {
    image_residual_apply_u16(base, base_strides, sym, lo_plane, B, H, W, depth, tau, shift, out, out_strides, ref,
                             ref_strides, sq_err, max_err, status, (hipStream_t)stream);
  });
}

int mlic_residual_shift(int depth, uint64_t N, uint32_t max_abs_q, uint64_t sum_abs_q, int* shift) {
  return guard([&] {
    MLIC_CHECK(shift != nullptr, "residual_shift: null shift");
    MLIC_CHECK(depth >= RES16_MIN_DEPTH && depth <= RES16_MAX_DEPTH, "residual_shift: depth must be in 9..16");
    MLIC_CHECK(N >= 1 && N <= 3 * (1ull << 32), "residual_shift: N must be in 1..3 * 2^32");
    MLIC_CHECK(max_abs_q < (1u << depth), "residual_shift: max_abs_q must be below 2^depth");
    MLIC_CHECK(sum_abs_q <= (uint64_t)max_abs_q * N, "residual_shift: sum_abs_q above N max_abs_q");
    *shift = residual16_shift(depth, N, max_abs_q, sum_abs_q);
  });
}

int mlic_container_write_residual_deep(uint32_t H, uint32_t W, int vbr, int tau, int depth, int shift, uint64_t digest,
                                       const uint8_t* m, const uint16_t* freq, uint32_t seg_len, uint32_t n_seg,
                                       const uint32_t* seg_bytes, const uint8_t* inner, size_t inner_len,
                                       const uint8_t* segs, size_t segs_len, const uint8_t* lo, size_t lo_len,
                                       uint8_t* out, size_t cap, size_t* len) {
  return guard([&] {
    MLIC_CHECK(tau >= 0, "container_write_residual_deep: negative tau");
    MLIC_CHECK(depth >= 0 && shift >= 0, "container_write_residual_deep: negative depth or shift");
    container_ok(container_write_residual_deep(H, W, vbr != 0, (uint32_t)tau, (uint32_t)depth, (uint32_t)shift, digest,
                                               m, freq, seg_len, n_seg, seg_bytes, inner, inner_len, segs, segs_len, lo,
                                               lo_len, out, cap, len));
  });
}

int mlic_container_parse_residual_deep(const uint8_t* data, size_t n, int n_levels, uint64_t max_pixels,
                                       mlic_container_residual_deep_info* info) {
  return guard([&] {
    MLIC_CHECK(info != nullptr, "container_parse_residual_deep: null info");
    ResidualDeepInfo d;
    container_ok(container_parse_residual_deep(data, n, (uint32_t)std::max(n_levels, 0), max_pixels, &d));
    seg_to_abi(d.seg, info);
    info->depth = (int32_t)d.depth;
    info->shift = (int32_t)d.shift;
    info->lo_off = d.lo_off;
    info->lo_len = d.lo_len;
  });
}

int mlic_encode_image_u8_scaled(mlic_model* m, void* stream, const uint8_t* rgb_dev, const int64_t* strides, int H,
                                int W, int coded_H, int coded_W, int filter, float vbr_scale, int level, uint8_t* out,
                                size_t cap, size_t* len) {
  return guard([&] {
    Model& mod = impl(m);
    MLIC_CHECK(len != nullptr, "encode_image_u8_scaled: null len");
    if (rgb_dev != nullptr) {
      MLIC_CHECK(strides != nullptr && H >= 1 && W >= 1, "encode_image_u8_scaled: strides, H >= 1 and W >= 1 expected");
      MLIC_CHECK(coded_H >= 1 && coded_W >= 1, "encode_image_u8_scaled: the coded size must be positive");
      const char* err = resample_axis_check(filter, H, coded_H);
      if (!err) err = resample_axis_check(filter, W, coded_W);
      if (err) throw Error(std::string("mlic: encode_image_u8_scaled: ") + err);
      const int Hp = (coded_H + 63) / 64 * 64, Wp = (coded_W + 63) / 64 * 64;
      const int64_t s4[4] = {0, strides[0], strides[1], strides[2]};
      m->enc_H = m->sc_H = 0;
      float* x = stage(m, sizeof(float) * 3 * (size_t)Hp * (size_t)Wp);
      image_ingest_u8_scaled(rgb_dev, s4, 1, H, W, filter, coded_H, coded_W, x, Hp, Wp, (hipStream_t)stream);
      const float sc[1] = {vbr_scale};
      mod.compress(x, 1, Hp, Wp, sc, (hipStream_t)stream);
      m->enc_H = coded_H;
      m->enc_W = coded_W;
      m->enc_level = level < 0 ? -1 : level;
      m->enc_passes = 0;
      m->sc_H = H;
      m->sc_W = W;
      m->sc_filter = filter;
    }
    MLIC_CHECK(m->enc_H > 0 && m->sc_H > 0,
               "encode_image_u8_scaled: rgb_dev is NULL and the handle's last encode was not a scaled one");
    size_t inner = 0;
    write_encoded(m, mod, nullptr, 0, &inner);
    *len = SCALED_HEADER + inner;
    if (out == nullptr) return;
    MLIC_CHECK(cap >= *len, "encode_image_u8_scaled: buffer too small");
    std::vector<uint8_t> file(inner);
    write_encoded(m, mod, file.data(), file.size(), &inner);
    container_ok(container_write_scaled((uint32_t)m->sc_H, (uint32_t)m->sc_W, m->enc_level >= 0,
                                        (uint32_t)m->sc_filter, file.data(), file.size(), out, cap, len));
  });
}

int mlic_decode_image_u8_sized(mlic_model* m, void* stream, const uint8_t* file, size_t n, int n_levels,
                               uint64_t max_pixels, const float* vbr_gains, int out_H, int out_W, int filter,
                               uint8_t* rgb_dev, const int64_t* strides, size_t cap_bytes, int* H, int* W, int* level,
                               int* coded_H, int* coded_W) {
  return guard([&] {
    MLIC_CHECK(file != nullptr || n == 0, "decode_image_u8_sized: null file");
    MLIC_CHECK((out_H == 0) == (out_W == 0) && out_H >= 0 && out_W >= 0,
               "decode_image_u8_sized: out_H, out_W must both be positive or both be 0 (the file's display size)");
    MLIC_CHECK(filter >= -1 && filter < RESAMPLE_FILTERS,
               "decode_image_u8_sized: filter must be -1 (the file's; lanczos3 for a plain file), 0, 1 or 2");
    const bool vbr = n_levels > 0;
    ContainerInfo c;
    uint32_t dH, dW;
    int flt = filter < 0 ? RESAMPLE_LANCZOS3 : filter;
    const uint8_t* inner = file;
    if (is_scaled_file(file, n)) {
      ScaledInfo s;
      container_ok(container_parse_scaled(file, n, (uint32_t)std::max(n_levels, 0), max_pixels, &s));
      MLIC_CHECK(s.vbr == vbr, "decode_image_u8_sized: the file's VBR flag does not match n_levels");
      c = s.inner;
      inner = file + s.inner_off;
      dH = s.H, dW = s.W;
      if (filter < 0) flt = (int)s.filter;
    } else {
      container_ok(container_parse(file, n, vbr, (uint32_t)std::max(n_levels, 0), max_pixels, &c));
      dH = c.H, dW = c.W;
    }
    MLIC_CHECK(c.H <= (1u << 24) && c.W <= (1u << 24) && dH <= (1u << 24) && dW <= (1u << 24),
               "decode_image_u8_sized: image side above 2^24");
    const int oH = out_H ? out_H : (int)dH, oW = out_W ? out_W : (int)dW;
    if (H) *H = oH;
    if (W) *W = oW;
    if (level) *level = c.level;
    if (coded_H) *coded_H = (int)c.H;
    if (coded_W) *coded_W = (int)c.W;
    const char* err = resample_axis_check(flt, (int)c.H, oH);
    if (!err) err = resample_axis_check(flt, (int)c.W, oW);
    if (err) throw Error(std::string("mlic: decode_image_u8_sized: ") + err);
    if (rgb_dev == nullptr) return;
    Model& mod = impl(m);
    MLIC_CHECK(strides != nullptr && strides[0] >= 0 && strides[1] > 0 && strides[2] > 0,
               "decode_image_u8_sized: strides {row, column, channel} must be non-negative, column and channel nonzero");
    const uint64_t extent = 1 + (uint64_t)(oH - 1) * (uint64_t)strides[0] + (uint64_t)(oW - 1) * (uint64_t)strides[1] +
                            2 * (uint64_t)strides[2];
    MLIC_CHECK(extent <= cap_bytes, "decode_image_u8_sized: the output image does not fit cap_bytes");
    const int Hp = (int)c.hz * 64, Wp = (int)c.wz * 64;
    float* x = stage(m, sizeof(float) * 3 * (size_t)Hp * (size_t)Wp);
    const uint8_t* ys[1] = {inner + c.y_off};
    const uint8_t* zs[1] = {inner + c.z_off};
    const size_t yl[1] = {c.y_len}, zl[1] = {c.z_len};
    const float sc[1] = {vbr && vbr_gains ? vbr_gains[c.level] : 1.0f};
    mod.decompress(ys, yl, zs, zl, 1, (int)c.hz, (int)c.wz, x, sc, (hipStream_t)stream);
    const int64_t s3[3] = {0, (int64_t)Hp * Wp, Wp};
    const int64_t d4[4] = {0, strides[0], strides[1], strides[2]};
    image_egress_u8_scaled(x, s3, 1, (int)c.H, (int)c.W, flt, oH, oW, rgb_dev, d4, nullptr, nullptr, nullptr,
                           (hipStream_t)stream);
  });
}

static YuvDesc yuv_desc(const mlic_yuv_desc* d) {
  MLIC_CHECK(d != nullptr, "null mlic_yuv_desc");
  return YuvDesc{d->sub_x, d->sub_y, d->matrix, d->full_range, d->site_x, {d->reserved[0], d->reserved[1], d->reserved[2]}};
}

int mlic_image_ingest_yuv8(void* stream, const uint8_t* y, const int64_t* y_strides, const uint8_t* cb,
                           const int64_t* cb_strides, const uint8_t* cr, const int64_t* cr_strides,
                           const mlic_yuv_desc* desc, int B, int H, int W, float* dst, int Hp, int Wp) {
  return guard([&] {
    const YuvDesc d = yuv_desc(desc);
    image_ingest_yuv8(y, y_strides, cb, cb_strides, cr, cr_strides, &d, B, H, W, dst, Hp, Wp, (hipStream_t)stream);
  });
}

int mlic_image_egress_yuv8(void* stream, const float* src, const int64_t* src_strides, int B, int H, int W,
                           const mlic_yuv_desc* desc, uint8_t* y, const int64_t* y_strides, uint8_t* cb,
                           const int64_t* cb_strides, uint8_t* cr, const int64_t* cr_strides, const uint8_t* ref_y,
                           const int64_t* ref_y_strides, const uint8_t* ref_cb, const int64_t* ref_cb_strides,
                           const uint8_t* ref_cr, const int64_t* ref_cr_strides, uint64_t* sq_err) {
  return guard([&] {
    const YuvDesc d = yuv_desc(desc);
    image_egress_yuv8(src, src_strides, B, H, W, &d, y, y_strides, cb, cb_strides, cr, cr_strides, ref_y, ref_y_strides,
                      ref_cb, ref_cb_strides, ref_cr, ref_cr_strides, sq_err, (hipStream_t)stream);
  });
}

int mlic_encode_image_yuv8(mlic_model* m, void* stream, const uint8_t* y_dev, const int64_t* y_strides,
                           const uint8_t* cb_dev, const int64_t* cb_strides, const uint8_t* cr_dev,
                           const int64_t* cr_strides, const mlic_yuv_desc* desc, int H, int W, float vbr_scale,
                           int level, uint8_t* out, size_t cap, size_t* len) {
  return guard([&] {
    Model& mod = impl(m);
    MLIC_CHECK(len != nullptr, "encode_image_yuv8: null len");
    if (y_dev != nullptr) {
      MLIC_CHECK(cb_dev != nullptr && cr_dev != nullptr, "encode_image_yuv8: null chroma plane");
      MLIC_CHECK(y_strides != nullptr && cb_strides != nullptr && cr_strides != nullptr && H >= 1 && W >= 1,
                 "encode_image_yuv8: strides, H >= 1 and W >= 1 expected");
      MLIC_CHECK(H <= (1 << 24) && W <= (1 << 24), "encode_image_yuv8: image side above 2^24");
      const YuvDesc d = yuv_desc(desc);
      const int Hp = (H + 63) / 64 * 64, Wp = (W + 63) / 64 * 64;
      const int64_t ys[3] = {0, y_strides[0], y_strides[1]}, bs[3] = {0, cb_strides[0], cb_strides[1]},
                    rs[3] = {0, cr_strides[0], cr_strides[1]};
      m->enc_H = m->sc_H = 0;
      float* x = stage(m, sizeof(float) * 3 * (size_t)Hp * (size_t)Wp);
      image_ingest_yuv8(y_dev, ys, cb_dev, bs, cr_dev, rs, &d, 1, H, W, x, Hp, Wp, (hipStream_t)stream);
      const float sc[1] = {vbr_scale};
      mod.compress(x, 1, Hp, Wp, sc, (hipStream_t)stream);
      m->enc_H = H;
      m->enc_W = W;
      m->enc_level = level < 0 ? -1 : level;
      m->enc_passes = 0;
    }
    MLIC_CHECK(m->enc_H > 0, "encode_image_yuv8: y_dev is NULL and the handle has no encoded image");
    write_encoded(m, mod, out, cap, len);
  });
}

int mlic_decode_image_yuv8(mlic_model* m, void* stream, const uint8_t* file, size_t n, int n_levels,
                           uint64_t max_pixels, const float* vbr_gains, const mlic_yuv_desc* desc, uint8_t* y_dev,
                           const int64_t* y_strides, size_t y_cap, uint8_t* cb_dev, const int64_t* cb_strides,
                           size_t cb_cap, uint8_t* cr_dev, const int64_t* cr_strides, size_t cr_cap, int* H, int* W,
                           int* level) {
  return guard([&] {
    MLIC_CHECK(file != nullptr || n == 0, "decode_image_yuv8: null file");
    const bool vbr = n_levels > 0;
    ContainerInfo c;
    container_ok(container_parse(file, n, vbr, (uint32_t)std::max(n_levels, 0), max_pixels, &c));
    MLIC_CHECK(c.H <= (1u << 24) && c.W <= (1u << 24), "decode_image_yuv8: image side above 2^24");
    if (H) *H = (int)c.H;
    if (W) *W = (int)c.W;
    if (level) *level = c.level;
    if (y_dev == nullptr) return;
    Model& mod = impl(m);
    MLIC_CHECK(cb_dev != nullptr && cr_dev != nullptr, "decode_image_yuv8: null chroma plane");
    const YuvDesc d = yuv_desc(desc);
    MLIC_CHECK((d.sub_x == 1 || d.sub_x == 2) && (d.sub_y == 1 || d.sub_y == 2),
               "decode_image_yuv8: sub_x and sub_y must be 1 or 2");
    const int64_t* st[3] = {y_strides, cb_strides, cr_strides};
    const size_t caps[3] = {y_cap, cb_cap, cr_cap};
    for (int p = 0; p < 3; ++p) {
      MLIC_CHECK(st[p] != nullptr && st[p][0] >= 0 && st[p][1] > 0,
                 "decode_image_yuv8: strides {row, column} must be non-negative, column nonzero");
      const uint64_t ph = p ? (c.H + d.sub_y - 1) / d.sub_y : c.H, pw = p ? (c.W + d.sub_x - 1) / d.sub_x : c.W;
      const uint64_t extent = 1 + (ph - 1) * (uint64_t)st[p][0] + (pw - 1) * (uint64_t)st[p][1];
      MLIC_CHECK(extent <= caps[p], "decode_image_yuv8: the file's plane does not fit its cap_bytes");
    }
    const int Hp = (int)c.hz * 64, Wp = (int)c.wz * 64;
    float* x = stage(m, sizeof(float) * 3 * (size_t)Hp * (size_t)Wp);
    const uint8_t* ys[1] = {file + c.y_off};
    const uint8_t* zs[1] = {file + c.z_off};
    const size_t yl[1] = {c.y_len}, zl[1] = {c.z_len};
    const float sc[1] = {vbr && vbr_gains ? vbr_gains[c.level] : 1.0f};
    mod.decompress(ys, yl, zs, zl, 1, (int)c.hz, (int)c.wz, x, sc, (hipStream_t)stream);
    const int64_t s3[3] = {0, (int64_t)Hp * Wp, Wp};
    const int64_t y3[3] = {0, y_strides[0], y_strides[1]}, b3[3] = {0, cb_strides[0], cb_strides[1]},
                  r3[3] = {0, cr_strides[0], cr_strides[1]};
    image_egress_yuv8(x, s3, 1, (int)c.H, (int)c.W, &d, y_dev, y3, cb_dev, b3, cr_dev, r3, nullptr, nullptr, nullptr,
                      nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream);
  });
}

int mlic_image_ingest_u16(void* stream, const uint16_t* src, const int64_t* src_strides, int depth, int msb, int B,
                          int H, int W, float* dst, int Hp, int Wp) {
  return guard([&] { image_ingest_u16(src, src_strides, depth, msb, B, H, W, dst, Hp, Wp, (hipStream_t)stream); });
}

int mlic_image_egress_u16(void* stream, const float* src, const int64_t* src_strides, int B, int H, int W, int depth,
                          int msb, uint16_t* dst, const int64_t* dst_strides, const uint16_t* ref,
                          const int64_t* ref_strides, uint64_t* sq_err) {
  return guard([&] {
    image_egress_u16(src, src_strides, B, H, W, depth, msb, dst, dst_strides, ref, ref_strides, sq_err,
                     (hipStream_t)stream);
  });
}

int mlic_image_ingest_yuv16(void* stream, const uint16_t* y, const int64_t* y_strides, const uint16_t* cb,
                            const int64_t* cb_strides, const uint16_t* cr, const int64_t* cr_strides,
                            const mlic_yuv_desc* desc, int depth, int msb, int B, int H, int W, float* dst, int Hp,
                            int Wp) {
  return guard([&] {
    const YuvDesc d = yuv_desc(desc);
    image_ingest_yuv16(y, y_strides, cb, cb_strides, cr, cr_strides, &d, depth, msb, B, H, W, dst, Hp, Wp,
                       (hipStream_t)stream);
  });
}

int mlic_image_egress_yuv16(void* stream, const float* src, const int64_t* src_strides, int B, int H, int W,
                            const mlic_yuv_desc* desc, int depth, int msb, uint16_t* y, const int64_t* y_strides,
                            uint16_t* cb, const int64_t* cb_strides, uint16_t* cr, const int64_t* cr_strides,
                            const uint16_t* ref_y, const int64_t* ref_y_strides, const uint16_t* ref_cb,
                            const int64_t* ref_cb_strides, const uint16_t* ref_cr, const int64_t* ref_cr_strides,
                            uint64_t* sq_err) {
  return guard([&] {
    const YuvDesc d = yuv_desc(desc);
    image_egress_yuv16(src, src_strides, B, H, W, &d, depth, msb, y, y_strides, cb, cb_strides, cr, cr_strides, ref_y,
                       ref_y_strides, ref_cb, ref_cb_strides, ref_cr, ref_cr_strides, sq_err, (hipStream_t)stream);
  });
}

int mlic_encode_image_yuv16(mlic_model* m, void* stream, const uint16_t* y_dev, const int64_t* y_strides,
                            const uint16_t* cb_dev, const int64_t* cb_strides, const uint16_t* cr_dev,
                            const int64_t* cr_strides, const mlic_yuv_desc* desc, int depth, int msb, int H, int W,
                            float vbr_scale, int level, uint8_t* out, size_t cap, size_t* len) {
  return guard([&] {
    // every argument is checked before the handle is touched: a refused call keeps the handle's last encoded image
    // and makes no device call
    MLIC_CHECK(len != nullptr, "encode_image_yuv16: null len");
    YuvDesc d{};
    if (y_dev != nullptr) {
      MLIC_CHECK(cb_dev != nullptr && cr_dev != nullptr, "encode_image_yuv16: null chroma plane");
      MLIC_CHECK(y_strides != nullptr && cb_strides != nullptr && cr_strides != nullptr && H >= 1 && W >= 1,
                 "encode_image_yuv16: strides, H >= 1 and W >= 1 expected");
      MLIC_CHECK(H <= (1 << 24) && W <= (1 << 24), "encode_image_yuv16: image side above 2^24");
      MLIC_CHECK(y_strides[1] != 0 && cb_strides[1] != 0 && cr_strides[1] != 0,
                 "encode_image_yuv16: zero column stride");
      d = yuv_desc(desc);
      image_yuv16_check(&d, depth, msb, y_dev, cb_dev, cr_dev, "encode_image_yuv16");
    }
    Model& mod = impl(m);
    if (y_dev != nullptr) {
      const int Hp = (H + 63) / 64 * 64, Wp = (W + 63) / 64 * 64;
      const int64_t ys[3] = {0, y_strides[0], y_strides[1]}, bs[3] = {0, cb_strides[0], cb_strides[1]},
                    rs[3] = {0, cr_strides[0], cr_strides[1]};
      m->enc_H = m->sc_H = 0;
      float* x = stage(m, sizeof(float) * 3 * (size_t)Hp * (size_t)Wp);
      image_ingest_yuv16(y_dev, ys, cb_dev, bs, cr_dev, rs, &d, depth, msb, 1, H, W, x, Hp, Wp, (hipStream_t)stream);
      const float sc[1] = {vbr_scale};
      mod.compress(x, 1, Hp, Wp, sc, (hipStream_t)stream);
      m->enc_H = H;
      m->enc_W = W;
      m->enc_level = level < 0 ? -1 : level;
      m->enc_passes = 0;
    }
    MLIC_CHECK(m->enc_H > 0, "encode_image_yuv16: y_dev is NULL and the handle has no encoded image");
    write_encoded(m, mod, out, cap, len);
  });
}

int mlic_decode_image_yuv16(mlic_model* m, void* stream, const uint8_t* file, size_t n, int n_levels,
                            uint64_t max_pixels, const float* vbr_gains, const mlic_yuv_desc* desc, int depth, int msb,
                            uint16_t* y_dev, const int64_t* y_strides, size_t y_cap, uint16_t* cb_dev,
                            const int64_t* cb_strides, size_t cb_cap, uint16_t* cr_dev, const int64_t* cr_strides,
                            size_t cr_cap, int* H, int* W, int* level) {
  return guard([&] {
    MLIC_CHECK(file != nullptr || n == 0, "decode_image_yuv16: null file");
    const bool vbr = n_levels > 0;
    ContainerInfo c;
    container_ok(container_parse(file, n, vbr, (uint32_t)std::max(n_levels, 0), max_pixels, &c));
    MLIC_CHECK(c.H <= (1u << 24) && c.W <= (1u << 24), "decode_image_yuv16: image side above 2^24");
    if (H) *H = (int)c.H;
    if (W) *W = (int)c.W;
    if (level) *level = c.level;
    if (y_dev == nullptr) return;
    // every argument is checked before the handle is touched: a refused call makes no device call
    MLIC_CHECK(cb_dev != nullptr && cr_dev != nullptr, "decode_image_yuv16: null chroma plane");
    const YuvDesc d = yuv_desc(desc);
    image_yuv16_check(&d, depth, msb, y_dev, cb_dev, cr_dev, "decode_image_yuv16");
    const int64_t* st[3] = {y_strides, cb_strides, cr_strides};
    const size_t caps[3] = {y_cap, cb_cap, cr_cap};
    for (int p = 0; p < 3; ++p) {
      MLIC_CHECK(st[p] != nullptr && st[p][0] >= 0 && st[p][1] > 0,
                 "decode_image_yuv16: strides {row, column} must be non-negative, column nonzero");
      const uint64_t ph = p ? (c.H + d.sub_y - 1) / d.sub_y : c.H, pw = p ? (c.W + d.sub_x - 1) / d.sub_x : c.W;
      const uint64_t extent = 1 + (ph - 1) * (uint64_t)st[p][0] + (pw - 1) * (uint64_t)st[p][1];  // elements
      MLIC_CHECK(extent <= caps[p] / sizeof(uint16_t), "decode_image_yuv16: the file's plane does not fit its cap_bytes");
    }
    Model& mod = impl(m);
    const int Hp = (int)c.hz * 64, Wp = (int)c.wz * 64;
    float* x = stage(m, sizeof(float) * 3 * (size_t)Hp * (size_t)Wp);
    const uint8_t* ys[1] = {file + c.y_off};
    const uint8_t* zs[1] = {file + c.z_off};
    const size_t yl[1] = {c.y_len}, zl[1] = {c.z_len};
    const float sc[1] = {vbr && vbr_gains ? vbr_gains[c.level] : 1.0f};
    mod.decompress(ys, yl, zs, zl, 1, (int)c.hz, (int)c.wz, x, sc, (hipStream_t)stream);
    const int64_t s3[3] = {0, (int64_t)Hp * Wp, Wp};
    const int64_t y3[3] = {0, y_strides[0], y_strides[1]}, b3[3] = {0, cb_strides[0], cb_strides[1]},
                  r3[3] = {0, cr_strides[0], cr_strides[1]};
    image_egress_yuv16(x, s3, 1, (int)c.H, (int)c.W, &d, depth, msb, y_dev, y3, cb_dev, b3, cr_dev, r3, nullptr, nullptr,
                       nullptr, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream);
  });
}

// ---- residual coding of Y'CbCr frames (residual_yuv.h; DESIGN.md section 5 "Residual coding", "Y'CbCr frames")
namespace {
struct Planes3 {  // three plane pointers and their strides, as the kernels' host entries take them
  const void* p[3];
  const int64_t* s[3];
};
struct DescArg {  // the descriptor, or null for the entries' own refusal
  YuvDesc d;
  const YuvDesc* ptr;
  explicit DescArg(const mlic_yuv_desc* desc) : d{}, ptr(nullptr) {
    if (desc) {
      d = yuv_desc(desc);
      ptr = &d;
    }
  }
};
}  // namespace

#define MLIC_RES_YUV_ENTRIES(SFX, WORD, BYTES, DEPTH_PARAMS, DEPTH, MSB)                                              \
  int mlic_image_residual_front_##SFX(                                                                                \
      void* stream, const WORD* base_y, const int64_t* base_y_strides, const WORD* base_cb,                           \
      const int64_t* base_cb_strides, const WORD* base_cr, const int64_t* base_cr_strides, const WORD* x_y,           \
      const int64_t* x_y_strides, const WORD* x_cb, const int64_t* x_cb_strides, const WORD* x_cr,                    \
      const int64_t* x_cr_strides, const mlic_yuv_desc* desc, DEPTH_PARAMS int B, int H, int W, int tau, int shift,   \
      uint8_t* ctx, uint32_t* ctx_count, uint64_t* digest, int16_t* sym, uint64_t* lo_plane, uint32_t* hist,          \
      uint32_t* max_err, uint32_t* max_abs_q, uint64_t* sum_abs_q) {                                                  \
    return guard([&] {                                                                                                \
      const Planes3 b{{base_y, base_cb, base_cr}, {base_y_strides, base_cb_strides, base_cr_strides}};               \
      const Planes3 x{{x_y, x_cb, x_cr}, {x_y_strides, x_cb_strides, x_cr_strides}};                                 \
      const DescArg d(desc);                                                                                          \
      image_residual_front_planes("image_residual_front_" #SFX, BYTES, b.p, b.s, x.p, x.s, d.ptr, DEPTH, MSB, B, H,  \
                                  W, tau, shift, ctx, ctx_count, digest, sym, lo_plane, hist, max_err, max_abs_q,     \
                                  sum_abs_q, (hipStream_t)stream);                                                    \
    });                                                                                                               \
  }                                                                                                                   \
  int mlic_image_residual_stats_##SFX(                                                                                \
      void* stream, const WORD* base_y, const int64_t* base_y_strides, const WORD* base_cb,                           \
      const int64_t* base_cb_strides, const WORD* base_cr, const int64_t* base_cr_strides, const WORD* x_y,           \
      const int64_t* x_y_strides, const WORD* x_cb, const int64_t* x_cb_strides, const WORD* x_cr,                    \
      const int64_t* x_cr_strides, const mlic_yuv_desc* desc, DEPTH_PARAMS int B, int H, int W, int tau,              \
      uint32_t* max_abs_q, uint64_t* sum_abs_q) {                                                                     \
    return guard([&] {                                                                                                \
      const Planes3 b{{base_y, base_cb, base_cr}, {base_y_strides, base_cb_strides, base_cr_strides}};               \
      const Planes3 x{{x_y, x_cb, x_cr}, {x_y_strides, x_cb_strides, x_cr_strides}};                                 \
      const DescArg d(desc);                                                                                          \
      image_residual_stats_planes("image_residual_stats_" #SFX, BYTES, b.p, b.s, x.p, x.s, d.ptr, DEPTH, MSB, B, H,  \
                                  W, tau, max_abs_q, sum_abs_q, (hipStream_t)stream);                                 \
    });                                                                                                               \
  }                                                                                                                   \
  int mlic_image_residual_apply_##SFX(                                                                                \
      void* stream, const WORD* base_y, const int64_t* base_y_strides, const WORD* base_cb,                           \
      const int64_t* base_cb_strides, const WORD* base_cr, const int64_t* base_cr_strides, const int16_t* sym,        \
      const uint64_t* lo_plane, const mlic_yuv_desc* desc, DEPTH_PARAMS int B, int H, int W, int tau, int shift,      \
      WORD* out_y, const int64_t* out_y_strides, WORD* out_cb, const int64_t* out_cb_strides, WORD* out_cr,           \
      const int64_t* out_cr_strides, const WORD* ref_y, const int64_t* ref_y_strides, const WORD* ref_cb,             \
      const int64_t* ref_cb_strides, const WORD* ref_cr, const int64_t* ref_cr_strides, uint64_t* sq_err,             \
      uint32_t* max_err, uint32_t* status) {                                                                          \
    return guard([&] {                                                                                                \
      const Planes3 b{{base_y, base_cb, base_cr}, {base_y_strides, base_cb_strides, base_cr_strides}};               \
      const Planes3 r{{ref_y, ref_cb, ref_cr}, {ref_y_strides, ref_cb_strides, ref_cr_strides}};                     \
      void* const o[3] = {out_y, out_cb, out_cr};                                                                     \
      const int64_t* const os[3] = {out_y_strides, out_cb_strides, out_cr_strides};                                   \
      const DescArg d(desc);                                                                                          \
      image_residual_apply_planes("image_residual_apply_" #SFX, BYTES, b.p, b.s, sym, lo_plane, d.ptr, DEPTH, MSB,   \
                                  B, H, W, tau, shift, o, os, r.p, r.s, sq_err, max_err, status,                      \
                                  (hipStream_t)stream);                                                               \
    });                                                                                                               \
  }
#define MLIC_NO_PARAMS
#define MLIC_DEPTH_PARAMS int depth, int msb,
MLIC_RES_YUV_ENTRIES(yuv8, uint8_t, 1, MLIC_NO_PARAMS, 8, 0)
MLIC_RES_YUV_ENTRIES(yuv16, uint16_t, 2, MLIC_DEPTH_PARAMS, depth, msb)
#undef MLIC_RES_YUV_ENTRIES
#undef MLIC_NO_PARAMS
#undef MLIC_DEPTH_PARAMS

namespace {
void res_yuv_size_check(const std::string& w, int H, int W, int sub_x, int sub_y) {
  MLIC_CHECK(H >= 1 && W >= 1, w + ": H and W must be positive");
  MLIC_CHECK(H <= (1 << 24) && W <= (1 << 24), w + ": frame side above 2^24");
  MLIC_CHECK(residual_yuv_sub_ok(sub_x, sub_y), w + ": sub_x, sub_y must be one of {1, 1}, {2, 1}, {2, 2}");
  MLIC_CHECK(residual_yuv_geom(H, W, sub_x, sub_y).N <= RES_SEG_MAX_N, w + ": the frame has more than 2^29 samples");
}
}  // namespace

int mlic_residual_yuv_samples(int H, int W, int sub_x, int sub_y, uint64_t* N) {
  return guard([&] {
    MLIC_CHECK(N != nullptr, "residual_yuv_samples: null N");
    res_yuv_size_check("residual_yuv_samples", H, W, sub_x, sub_y);
    *N = (uint64_t)residual_yuv_geom(H, W, sub_x, sub_y).N;
  });
}

int mlic_residual_yuv_plane_words(int H, int W, int sub_x, int sub_y, int shift, uint64_t* words) {
  return guard([&] {
    MLIC_CHECK(words != nullptr, "residual_yuv_plane_words: null words");
    res_yuv_size_check("residual_yuv_plane_words", H, W, sub_x, sub_y);
    MLIC_CHECK(shift >= 0 && shift <= residual16_max_shift(RES16_MAX_DEPTH), "residual_yuv_plane_words: shift must be in 0..9");
    *words = residual_yuv_plane_words((uint64_t)H, (uint64_t)W, sub_x, sub_y, shift);
  });
}

int mlic_container_write_residual_yuv(uint32_t H, uint32_t W, int vbr, int tau, int depth, int shift, int sub_x,
                                      int sub_y, int matrix, int full_range, int site_x, uint64_t digest,
                                      const uint8_t* m, const uint16_t* freq, uint32_t seg_len, uint32_t n_seg,
                                      const uint32_t* seg_bytes, const uint8_t* inner, size_t inner_len,
                                      const uint8_t* segs, size_t segs_len, const uint8_t* lo, size_t lo_len,
                                      uint8_t* out, size_t cap, size_t* len) {
  return guard([&] {
    MLIC_CHECK(tau >= 0, "container_write_residual_yuv: negative tau");
    MLIC_CHECK(depth >= 0 && shift >= 0, "container_write_residual_yuv: negative depth or shift");
    MLIC_CHECK(sub_x >= 0 && sub_y >= 0 && matrix >= 0, "container_write_residual_yuv: negative sub_x, sub_y or matrix");
    MLIC_CHECK(full_range == 0 || full_range == 1, "container_write_residual_yuv: full_range must be 0 or 1");
    MLIC_CHECK(site_x == 0 || site_x == 1, "container_write_residual_yuv: site_x must be 0 (centre) or 1 (left)");
    container_ok(container_write_residual_yuv(H, W, vbr != 0, (uint32_t)tau, (uint32_t)depth, (uint32_t)shift,
                                              (uint32_t)sub_x, (uint32_t)sub_y, (uint32_t)matrix,
                                              (uint32_t)(full_range | (site_x << 1)), digest, m, freq, seg_len, n_seg,
                                              seg_bytes, inner, inner_len, segs, segs_len, lo, lo_len, out, cap, len));
  });
}

int mlic_container_parse_residual_yuv(const uint8_t* data, size_t n, int n_levels, uint64_t max_pixels,
                                      mlic_container_residual_yuv_info* info) {
  return guard([&] {
    MLIC_CHECK(info != nullptr, "container_parse_residual_yuv: null info");
    ResidualYuvInfo y;
    container_ok(container_parse_residual_yuv(data, n, (uint32_t)std::max(n_levels, 0), max_pixels, &y));
    seg_to_abi(y.deep.seg, info);
    info->depth = (int32_t)y.deep.depth;
    info->shift = (int32_t)y.deep.shift;
    info->lo_off = y.deep.lo_off;
    info->lo_len = y.deep.lo_len;
    info->sub_x = (int32_t)y.sub_x;
    info->sub_y = (int32_t)y.sub_y;
    info->matrix = (int32_t)y.matrix;
    info->full_range = y.full_range ? 1 : 0;
    info->site_x = y.site_left ? 1 : 0;
  });
}

int mlic_neglog2_sum(void* stream, const float* lik, int B, int64_t n_per, double* out) {
  return guard([&] {
    double* part = nullptr;
    HIP_OK(hipMalloc(&part, sizeof(double) * neglog2_partial_doubles(B)));
    try {
      neglog2_sum(lik, n_per, B, out, part, (hipStream_t)stream);
      HIP_OK(hipStreamSynchronize((hipStream_t)stream));
    } catch (...) {
      (void)hipFree(part);
      throw;
    }
    HIP_OK(hipFree(part));
  });
}

int mlic_gaussian_likelihood(void* stream, const float* y, const float* scales, const float* means, int64_t n,
                             float vbr_scale, float* lik) {
  return guard([&] {
    MLIC_CHECK(n >= 0 && (n == 0 || (y && scales && means && lik)), "gaussian_likelihood arguments");
    gauss_likelihood(y, scales, means, n, vbr_scale, lik, (hipStream_t)stream);
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  });
}

int mlic_scale_indexes(void* stream, const float* scales, int64_t n, const float* table, int ntable, int32_t* out) {
  return guard([&] {
    MLIC_CHECK(ntable >= 2 && ntable <= 1024, "scale table size");
    MLIC_CHECK(n >= 0 && (n == 0 || (scales && table && out)), "scale_indexes arguments");
    scale_indexes(scales, n, table, ntable, out, (hipStream_t)stream);
    HIP_OK(hipStreamSynchronize((hipStream_t)stream));
  });
}

int mlic_pmf_to_quantized_cdf(const float* pmf, int n, int precision, int32_t* cdf_out) {
  return guard([&] {
    auto c = pmf_to_quantized_cdf(pmf, n, precision);
    for (size_t i = 0; i < c.size(); ++i) cdf_out[i] = (int32_t)c[i];
  });
}

int mlic_rans_encode(const int32_t* symbols, const int32_t* indexes, int64_t n, const int32_t* cdf,
                     const int32_t* cdf_len, const int32_t* offset, int n_tables, int stride, uint8_t* out,
                     size_t cap, size_t* written) {
  return guard([&] {
    CdfTables t = make_tables(cdf, cdf_len, offset, n_tables, stride);
    std::string s = rans_encode(symbols, indexes, n, t);
    *written = s.size();
    MLIC_CHECK(s.size() <= cap, "output buffer too small");
    std::memcpy(out, s.data(), s.size());
  });
}

int mlic_rans_decode(const uint8_t* data, size_t nbytes, const int32_t* indexes, int64_t n, const int32_t* cdf,
                     const int32_t* cdf_len, const int32_t* offset, int n_tables, int stride, int32_t* out) {
  return guard([&] {
    CdfTables t = make_tables(cdf, cdf_len, offset, n_tables, stride);
    RansDecoderState d;
    d.set_stream(data, nbytes);
    d.decode(indexes, n, t, out);
  });
}

int mlic_rans_decode_narrow(const uint8_t* data, size_t nbytes, const uint8_t* indexes, int64_t n, int nparts,
                            const int32_t* cdf, const int32_t* cdf_len, const int32_t* offset, int n_tables,
                            int stride, int32_t* out, int* widened) {
  return guard([&] {
    MLIC_CHECK(nparts >= 1 && n % nparts == 0 && widened, "rans_decode_narrow: n / nparts");
    CdfTables t = make_tables(cdf, cdf_len, offset, n_tables, stride);
    RansDecoderState d;
    d.set_stream(data, nbytes);
    const int64_t np = n / nparts;
    std::vector<int16_t> s16(np);
    *widened = 0;
    for (int k = 0; k < nparts; ++k) {
      if (rans_decode_piece(d, indexes + k * np, np, t, s16.data(), out + k * np, opt(OPT_NARROW_LIMIT)))
        for (int64_t i = 0; i < np; ++i) out[k * np + i] = s16[i];
      else
        ++*widened;
    }
  });
}

}  // extern "C"
