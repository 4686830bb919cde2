// Host-side launchers of the MLIC++ HIP kernels (see conv_mfma.hip, kernels.hip).
#pragma once
#include "common.h"
#include "options.h"

#include <algorithm>

namespace mlic {

// implicit-GEMM conv on MFMA (conv_mfma.hip)
// tile instantiation chosen for P: 0 = <64,64>, 1 = <64,128>, 2 = <128,64>, 3 = <128,128>
int conv_variant(const ConvParams& P);
void conv_forward(const ConvParams& P, hipStream_t st);

// split-fp16 ("f16x3") MFMA conv (conv_f16x3.hip): same contract, weights pre-split to
// hi/lo fp16 [Cout][K*K][cin_pad] (cin_pad = Cin rounded up to 32)
int conv_f16x3_variant(const ConvParams& P);
void conv_f16x3_forward(const ConvParams& P, const _Float16* wh, const _Float16* wl, int cin_pad, hipStream_t st);
int conv_x3v2_variant(const ConvParams& P);
void conv_x3v2_forward(const ConvParams& P, const _Float16* wh, const _Float16* wl, int cin_pad, hipStream_t st);
// prescale: split w * 2^e with the layer's max |w| * 2^e in [2^14, 2^15); returns e (0 without
// prescale).  Synchronises st.
int split_weights(const float* w, _Float16* wh, _Float16* wl, int Cout, int Cin, int KK, int cin_pad, bool prescale,
                  hipStream_t st);

// specialised convs (conv_pw.hip)
bool pw_resident_ok(const ConvParams& P, int cin_pad);
void pw_resident_forward(const ConvParams& P, const _Float16* wh, const _Float16* wl, int cin_pad, hipStream_t st);
bool conv_narrow_ok(const ConvParams& P);
void conv_narrow_forward(const ConvParams& P, hipStream_t st);
// A/B-only families (ab/*.hip, make AB=1): v1 tiles, halo tiles, VALU local attention; the product
// build links ab/ab_stubs.cpp instead (they throw; conv_halo_ok is false)
bool ab_families_built();
bool conv_halo_ok(const ConvParams& P, int cin_pad);
void conv_halo_forward(const ConvParams& P, const _Float16* wh, const _Float16* wl, int cin_pad, hipStream_t st);
// g_s's N -> 12 3x3 output conv as 1x1 per-tap partials [B][108][H][W] + this gather (conv_pw.hip):
// out [B][3][2H][2W] = PixelShuffle(2)(bias + sum over taps of the shifted partials)
void taps_gather(const float* part, int64_t part_bs, const float* bias, float* out, int64_t out_bs, int H, int W,
                 int B, hipStream_t st);
bool conv_smallcin_ok(const ConvParams& P);
void conv_smallcin_forward(const ConvParams& P, hipStream_t st);

// fused depthwise 3x3 (stride 1, pad 1) + pointwise 1x1 (conv_dwpw.hip): P describes the pointwise
// conv with the DEPTHWISE input as its input; dww [Cin][9], dwb [Cin]; needs W even (dwpw_ok)
bool dwpw_ok(const ConvParams& P, int cin_pad);
// the model's choice on top of dwpw_ok: grids where the fused kernel measured faster (per image only)
bool dwpw_grid_ok(const ConvParams& P);
// producer / consumer forms for Cin = Cout in {96, 128, 160, 192}, bias / GELU (+ residual): dwpw_forward
// takes the chosen one where it applies: mlic_set_kernel_option("dwpw2"): -1 = $MLIC_DWPW2 (default 2),
// 0 = dwpw_kernel, 1 = the row-pipelined LDS form (ab/conv_dwpw2.hip: A/B-only family, make AB=1), 2 = the
// register-row form (conv_dwpw3.hip)
bool dwpw2_ok(const ConvParams& P, int cin_pad);
// the A/B-only row-pipelined LDS form (ab/conv_dwpw2.hip; the product build's stub reports false / throws)
bool dwpw2_lds_ok(const ConvParams& P, int cin_pad);
void dwpw2_lds_forward(const ConvParams& P, const _Float16* wh, const _Float16* wl, int cin_pad, const float* dww,
                       const float* dwb, hipStream_t st);
bool dwpw3_shape_ok(const ConvParams& P, int cin_pad);
// the same kernel's pointwise-only form for the full-resolution 1x1 convs (pw_resident MODE 0 - 3, Cin = Cout
// in {96, 128, 160, 192}): pw_resident_forward takes it where pw3_ok; mlic_set_kernel_option("pw3"):
// -1 = $MLIC_PW3 (default 1), 0 off, 1 from 256 K px per image, 2 every grid
bool pw3_ok(const ConvParams& P, int cin_pad);
void pw3_forward(const ConvParams& P, const _Float16* wh, const _Float16* wl, int cin_pad, hipStream_t st);
void dwpw3_forward(const ConvParams& P, const _Float16* wh, const _Float16* wl, int cin_pad, const float* dww,
                   const float* dwb, hipStream_t st);
void dwpw2_forward(const ConvParams& P, const _Float16* wh, const _Float16* wl, int cin_pad, const float* dww,
                   const float* dwb, hipStream_t st);
void dwpw_forward(const ConvParams& P, const _Float16* wh, const _Float16* wl, int cin_pad, const float* dww,
                  const float* dwb, hipStream_t st);

// LDS-DMA split-fp16 conv (conv_x4.hip): activations packed per call into a zero-bordered split
// layout (x4_pack_act, workspace of x4_act_halves halves), weights packed once (x4_pack_weights)
int x4_bm(int Cout);
// hi = the reduced-precision form (single fp16 term, 64-channel chunks; g_s only)
int x4_nchunk(int cin_pad, bool hi);
int64_t x4_weight_halves(int Cout, int KK, int cin_pad, bool hi = false);
void x4_pack_weights(const _Float16* wh, const _Float16* wl, int Cout, int KK, int cin_pad, _Float16* dst,
                     hipStream_t st, bool hi = false);
int64_t x4_act_halves(const ConvParams& P, int cin_pad, bool hi = false);
bool conv_x4_ok(const ConvParams& P, int cin_pad);
void x4_pack_act(const ConvParams& P, int cin_pad, _Float16* dst, hipStream_t st, bool hi = false);
// 1x1 layers: x4 builds its B rows from the fp32 input itself (no packed copy; act = nullptr)
bool x4_direct_ok(const ConvParams& P, bool hi);
// part: the split-K partial planes (x4_part_bytes bytes; nullptr = no split)
int x4_splitk(const ConvParams& P, int cin_pad, bool hi = false);
int64_t x4_part_bytes(const ConvParams& P, int cin_pad, bool hi = false);
void conv_x4_forward(const ConvParams& P, const _Float16* act, const _Float16* wx, int cin_pad, hipStream_t st,
                     float* part = nullptr, bool hi = false);

// kernel-family selection (conv_dispatch.cpp)
enum ConvImpl : int {
  CONV_F32 = 0, CONV_X3 = 1, CONV_X3V2 = 2, CONV_PW = 3, CONV_NARROW = 4, CONV_SMALLCIN = 5, CONV_HALO = 6,
  CONV_X4 = 7,
  CONV_X4H = 8  // x4 in the reduced-precision form (fp16 operands, fp32 accumulation): g_s on request only
};
struct ConvWeights {
  const float* wpk;  // fp32 packed [K*K][Cin][Cout] (in ConvParams too)
  const _Float16* wh;
  const _Float16* wl;
  int cin_pad;
  const _Float16* wx4 = nullptr;  // x4_pack_weights image (null: CONV_X4 not available)
  int wexp = 0;                   // wh/wl hold w * 2^wexp (split_weights)
  const _Float16* wx4h = nullptr; // the reduced-precision image (x4_pack_weights hi; null: no CONV_X4H)
};
int conv_select(const ConvParams& P, const ConvWeights& w, int precision);
// device workspace conv_run needs for impl (bytes; 0 = none)
int64_t conv_ws_bytes(int impl, const ConvParams& P, const ConvWeights& w);
void conv_run(int impl, const ConvParams& P, const ConvWeights& w, hipStream_t st, void* ws = nullptr);

// live-profiling categories (one per kernel family / tile instantiation)
enum ProfCat : int {
  PCAT_CONV_F32 = 0,     // 0..3  conv_mfma_kernel tiles (conv_variant)
  PCAT_CONV_X3 = 4,      // 4..7  conv_f16x3_kernel tiles (conv_f16x3_variant)
  PCAT_CONV_X3V2 = 8,    // 8..10 conv_x3v2_kernel tiles <64,128>, <128,256>, <128,128>
  PCAT_CONV_X3V2_WIDE = 11,  // conv_x3v2_kernel<256,256> (8 waves)
  PCAT_CONV_PW = 12,
  PCAT_CONV_NARROW = 13,
  PCAT_CONV_SMALLCIN = 14,
  PCAT_CONV_HALO = 15,
  PCAT_DW = 16,
  PCAT_LOCAL = 17,
  PCAT_LINATT = 18,
  PCAT_ELEM = 19,
  PCAT_CONV_X4 = 20,
  PCAT_CHAIN = 21,
  PCAT_DWPW = 22,
  PCAT_COUNT = 23
};
int conv_prof_cat(int impl, const ConvParams& P);
const char* prof_cat_name(int cat);

struct DwParams {
  Seg seg[MAXSEG];
  int nseg;
  int C, H, W, Ho, Wo, stride;
  const float* w;     // [C][9]
  const float* bias;  // [C]
  float* out;
  int64_t out_bs;
  int gelu;
  int B;
  // checkerboard half (dw_half_ok): 0 = every pixel; 1 = the anchor pixels only ((y + x) odd), 2 = the
  // non-anchor pixels only, written squeezed: planes of H x W / 2, pixel (y, x) at y * W / 2 + x / 2
  // (LocalAttnParams::ckbd's layout); each value is the whole-grid form's, bit for bit
  int ckbd;
};
void dw3x3(const DwParams& P, hipStream_t st);
// shapes the half form serves (stride 1, W a multiple of 4 up to 256, 16-byte batch strides); base pointers
// must be 16-byte aligned (checked at the launch, so the answer is the same in an arena's planning pass)
bool dw_half_ok(const DwParams& P);

void ln_channels(const float* x, int64_t x_bs, float* y, int64_t y_bs, const float* g, const float* b, int C,
                 int HW, int B, hipStream_t st);

struct LocalAttnParams {
  const float* qkv;
  int64_t qkv_bs;
  float* out;  // [C*25][HW]
  int64_t out_bs;
  const float* rel_table;  // [81][2]
  const int* rel_index;    // [625] int32
  float scale;
  int C, H, W, B;
  // local_attn_packed only: 0 = every query pixel; 1 / 2 = the anchor / non-anchor pixels only, written
  // at their squeezed position y * W / 2 + x / 2 (W even)
  int ckbd;
};
void local_attn(const LocalAttnParams& P, hipStream_t st);       // MFMA (attn_local.hip) unless MLIC_LOCAL_ATTN_VALU=1
void local_attn_mfma(const LocalAttnParams& P, hipStream_t st);
void local_attn_valu(const LocalAttnParams& P, hipStream_t st);
// dim 32 only: output in conv_x4's packed split layout [B][25 query cells][npos][64 halves]
// (channel head*16 + d), the B operand of the fusion conv with its K permuted to cell*32 + channel
void local_attn_packed(const LocalAttnParams& P, _Float16* out, int npos, hipStream_t st);

// context.py:180-187 / 235-239 in three launches (no materialised softmax); kmask: anchor-only keys,
// qmask: non-anchor-only queries; part: linear_attention_part_floats() floats
// the model's split policy (also mlic_linatt_splits): splits of at least 256 keys, at most 64 of them, none
// empty -- ctx_partial's loop bounds are ceil(HW / nsplit) keys per split
inline int ctx_splits(int HW) { return std::max(1, std::min(64, HW / 256)); }
int64_t linear_attention_part_floats(int heads, int hd, int B, int nsplit);
void linear_attention(const float* K, int64_t k_bs, const float* V, int64_t v_bs, const float* Q, int64_t q_bs,
                      float* out, int64_t o_bs, float* part, float* ctx, int heads, int hd, int H, int W, int B,
                      int nsplit, int kmask, int qmask, hipStream_t st);
// the fused form: ctx = softmax_L(K) . V^T (partials + the fixed-order combine), then linatt_pack
// (conv_x4.hip) computes ctx^T . softmax_c(Q) straight into the packed operand of the conv that
// consumes the attention (P: that conv's params; dst: x4_act_halves(P, P.Cin) halves)
void linear_attention_ctx(const float* K, int64_t k_bs, const float* V, int64_t v_bs, float* part, float* ctx,
                          int heads, int hd, int H, int W, int B, int nsplit, int kmask, hipStream_t st);
void linatt_pack(const float* Q, int64_t q_bs, const float* ctx, int heads, int hd, int qmask, const ConvParams& P,
                 _Float16* dst, hipStream_t st);
void ckbd_mask(const float* x, int64_t x_bs, float* y, int64_t y_bs, int C, int H, int W, int B, int keep_anchor,
               hipStream_t st);

struct QuantParams {
  const float* y;  // latent slice [C][HW] (encoder side)
  int64_t y_bs;
  const float* params;  // EP output of this phase [2C][HW]
  int64_t params_bs;
  const float* params_a;  // anchor-phase EP output (likelihood merge), phase 1 only
  int64_t params_a_bs;
  float* yh;  // y_hat slice [C][HW]
  int64_t yh_bs;
  float* lik;  // likelihood slice or null
  int64_t lik_bs;
  int32_t* sym;  // squeezed symbols or null
  int32_t* idx;  // squeezed indexes or null
  // the narrow coder streams that cross PCIe (a scale index is < 64; a symbol almost always fits 16
  // bits): encoder: written beside sym, a symbol beyond int16 saturates sym16 and sets *ovf (the host
  // then takes the int32 sym); decoder: phase_indexes writes idx8, phase_dequant reads sym16 when set
  int16_t* sym16;
  uint8_t* idx8;
  int* ovf;
  int nlim;  // the narrow range [-nlim - 1, nlim]: 32767 (int16); smaller only under the test knob below
  const float* table;
  int ntable;
  int phase;  // 0 anchor, 1 non-anchor
  int vbr;
  const float* sc;  // [B] per-image VBR gain (mlicpp_vbr.py:137, Gain[s] or inputscale), when vbr
  const float* rs;  // [B] 1 / sc, computed once on the host in fp32 (the reference's 1 / scale)
  int C, H, W, B;
  // ROI coding: the gain per latent pixel, [B][H][W], and its reciprocal plane (recip_plane); both or neither.
  // When set (with vbr) the three kernels read sc / rs at their own pixel instead of at [b].
  const float* scp;
  const float* rsp;
};
// r[i] = 1.0f / g[i], correctly rounded (the host's fp32 1 / scale bit for bit)
void recip_plane(const float* g, float* r, int64_t n, hipStream_t st);
void quant_phase(const QuantParams& P, hipStream_t st);
void phase_indexes(const QuantParams& P, hipStream_t st);
void phase_dequant(const QuantParams& P, hipStream_t st);
// progressive decode: phase_dequant on all-zero symbols (yh = 0.0f + m at the phase's pixels; the anchor phase
// zeroes the others) that reads neither sym, sym16, idx8 nor the gains
void phase_fill(const QuantParams& P, hipStream_t st);

struct EbParams {
  const float* z;
  float* z_hat;
  float* lik;
  int32_t* sym;
  const float* quantiles;  // [C][1][3]
  const float *m0, *m1, *m2, *m3, *m4;
  const float *b0, *b1, *b2, *b3, *b4;
  const float *f0, *f1, *f2, *f3;
  int C, H, W, B;
};
void eb_forward(const EbParams& P, hipStream_t st);
void eb_dequant(const int32_t* sym, const float* quantiles, float* z_hat, int C, int HW, int B, hipStream_t st);

void pack_conv(const float* w, float* out, int Cout, int Cin, int KK, hipStream_t st);
// many device-to-device float copies in one launch (the weight load's per-parameter copies: one kernel
// instead of a blit per tensor); `descs` is a device array of n {dst, src, count}
struct CopyDesc {
  float* dst;
  const float* src;
  int64_t n;
};
void copy_many(const CopyDesc* descs, int n, hipStream_t st);
void gdn_prep(const float* beta, const float* gamma, const float* bb, const float* bped, const float* gb,
              const float* gped, float* beta_eff, float* gamma_pk, float* gamma_eff, int C, hipStream_t st);
void local_mask(float* out, int H, int W, hipStream_t st);
void sq_err_u8(const float* a, int64_t a_bs, const float* b, int64_t b_bs, double* out, int64_t n_per, int B,
               hipStream_t st);
// per-image sum of -log2(lik) (fixed order); part = neglog2_partial_doubles(B) doubles of scratch
int64_t neglog2_partial_doubles(int B);
void neglog2_sum(const float* lik, int64_t n_per, int B, double* out, double* part, hipStream_t st);
// per-image MS-SSIM of uint8-valued images (metrics.hip): a, b [B][C][H][W] fp32 in [0,1] with element
// strides {image, channel, row}; scratch = ms_ssim_scratch_bytes() bytes; out B doubles; terms (optional)
// [B][5][C] doubles.  ms_ssim_scratch_bytes is host logic only and throws on B < 1, C < 1, min(H, W) <= 160.
size_t ms_ssim_scratch_bytes(int B, int C, int H, int W);
void ms_ssim_u8(const float* a, const int64_t* a_strides, const float* b, const int64_t* b_strides, int B, int C,
                int H, int W, void* scratch, double* out, double* terms, hipStream_t st);
// LPIPS-VGG of uint8-valued images (lpips.hip; the definition in DESIGN.md §3).  The handle owns the packed
// weights (13 convs, 5 lin layers, the scaling layer), the fp16 range flag and its fallback counter; it serves
// one call at a time.  a, b [B][3][H][W] fp32 with element strides {image, channel, row}; out B doubles, terms
// (optional) [B][5] doubles.  lpips_scratch_bytes is host logic only and throws on B < 1, H or W < 16.  At
// precision 2 lpips_u8 waits for the stream once (it reads the range flag) and, when an operand of a dense conv
// left fp16's range, runs the whole call again with the fp32 MFMA convs and counts it.
class Lpips;
Lpips* lpips_create(int n, const char* const* names, const float* const* ptrs, const int64_t* shapes,
                    const int* ndims, hipStream_t st);
void lpips_destroy(Lpips* h);
void lpips_set_precision(Lpips* h, int precision);
size_t lpips_scratch_bytes(int B, int H, int W);
void lpips_u8(Lpips* h, const float* a, const int64_t* a_strides, const float* b, const int64_t* b_strides, int B,
              int H, int W, void* scratch, double* out, double* terms, hipStream_t st);
int64_t lpips_range_fallbacks(Lpips* h, bool reset);
// stage timing with device events: ms3 (optional) = {stem, dense convs, taps + reduce} summed over the calls since
// the last read, then cleared; `on` switches it for the calls that follow (a timed call waits for its stream)
void lpips_profile(Lpips* h, bool on, double* ms3);
// DISTS of uint8-valued images (dists.hip; the definition in DESIGN.md §3) on the same trunk (vgg_trunk.h), with
// LPIPS's handle rules, chunking, range guard and stage timing.  The table holds the 13 convs, "alpha" and
// "beta" [1][1475][1][1], optionally "mean" and "std" [1][3][1][1]; "*.filter" buffers are ignored.  out B
// doubles, terms (optional) [B][12] doubles [T1_0, T2_0, .., T1_5, T2_5].
class Dists;
Dists* dists_create(int n, const char* const* names, const float* const* ptrs, const int64_t* shapes,
                    const int* ndims, hipStream_t st);
void dists_destroy(Dists* h);
void dists_set_precision(Dists* h, int precision);
size_t dists_scratch_bytes(int B, int H, int W);
void dists_u8(Dists* h, const float* a, const int64_t* a_strides, const float* b, const int64_t* b_strides, int B,
              int H, int W, void* scratch, double* out, double* terms, hipStream_t st);
int64_t dists_range_fallbacks(Dists* h, bool reset);
void dists_profile(Dists* h, bool on, double* ms3);
// uint8 image I/O (image_io.hip).  Both check their arguments before any HIP call and throw.
// ingest: B images of H x W x 3 bytes read through element strides {image, row, column, channel} -> dst fp32
// [B][3][Hp][Wp] contiguous (Hp, Wp multiples of 64), v / 255 inside the image and +0 in the padding.
void image_ingest_u8(const uint8_t* src, const int64_t* src_strides, int B, int H, int W, float* dst, int Hp, int Wp,
                     hipStream_t st);
// egress: the H x W crop of src fp32 (element strides {image, channel, row}, column stride 1) as
// floor(clamp(v, 0, 1) * 255) (NaN -> 0) through dst's {image, row, column, channel} strides; with ref (its own
// strides), sq_err[b] = the exact sum of squared uint8 differences of image b
void image_egress_u8(const float* src, const int64_t* src_strides, int B, int H, int W, uint8_t* dst,
                     const int64_t* dst_strides, const uint8_t* ref, const int64_t* ref_strides, uint64_t* sq_err,
                     hipStream_t st);
// the rate loop's prefilter: dst image i [3][Hp][Wp] = the 3x3 filter (w9: 9 host floats, row-major; null = the
// reference's sigma 0.5 Gaussian) of src image src_index[i] (device indices; null = i), taps outside the H x W
// image 0, +0 in the padding, every element written; acc = acc + w[t] * v[t] in tap order, no FMA.  dst must not
// overlap the n images at src, nor any image src_index names.  Checks its arguments before any HIP call.
void image_blur3_pad(const float* src, const int32_t* src_index, int n, int H, int W, int Hp, int Wp, const float* w9,
                     float* dst, hipStream_t st);
// Scaled coding's edge kernels (resample.hip; DESIGN.md section 5 "Scaled coding"): image_ingest_u8 / image_egress_u8
// with the separable polyphase resampler of resample_table.h fused in (filter 0 lanczos3, 1 bicubic, 2 triangle).
// ingest: Hi x Wi bytes -> the h x w coded image, clamped to [0, 1], in fp32 [B][3][Hp][Wp] with +0 padding.
// egress: the h x w crop of src, clamped, -> Ho x Wo bytes, with the exact squared error against ref.  Strides as
// in the plain calls; every ratio output / input must lie in [1/8, 8].  The tables are device arrays built on
// first use of a (filter, input length, output length) triple (a blocking copy) and kept.  Both check their
// arguments before any HIP call and throw.
void image_ingest_u8_scaled(const uint8_t* src, const int64_t* src_strides, int B, int Hi, int Wi, int filter, int h,
                            int w, float* dst, int Hp, int Wp, hipStream_t st);
void image_egress_u8_scaled(const float* src, const int64_t* src_strides, int B, int h, int w, int filter, int Ho,
                            int Wo, uint8_t* dst, const int64_t* dst_strides, const uint8_t* ref,
                            const int64_t* ref_strides, uint64_t* sq_err, hipStream_t st);
// Residual coding's passes (residual.hip; residual.h has the definitions; DESIGN.md section 5 "Residual coding").
// Byte images through {image, row, column, channel} strides; ctx u8 and sym int16 are dense [B][3][H][W].
// front: ctx, ctx_count [B][24] and digest [B] always; with x also sym, hist [B][24][128] and max_err [B] (all three
// null without x).  apply: out = clamp(base + sym (2 tau + 1), 0, 255); with ref, sq_err [B] and max_err [B]
// against it.  Both zero the sums they accumulate into on the stream, check their arguments before any HIP call
// and throw.
void image_residual_front_u8(const uint8_t* base, const int64_t* base_strides, const uint8_t* x,
                             const int64_t* x_strides, int B, int H, int W, int tau, uint8_t* ctx, uint32_t* ctx_count,
                             uint64_t* digest, int16_t* sym, uint32_t* hist, uint32_t* max_err, hipStream_t st);
void image_residual_apply_u8(const uint8_t* base, const int64_t* base_strides, const int16_t* sym, int B, int H, int W,
                             int tau, uint8_t* out, const int64_t* out_strides, const uint8_t* ref,
                             const int64_t* ref_strides, uint64_t* sq_err, uint32_t* max_err, hipStream_t st);
// The same two passes on 9..16-bit samples in uint16 words (residual16.hip; residual16.h has the definitions; DESIGN.md
// section 5 "Residual coding", "Deep samples").  front without x: ctx, ctx_count, digest.  With x also sym (hi = q >>
// shift, int16), lo_plane (u64 [B][3 H ceil(W / 64) shift], null at shift 0), hist of hi, max_err, and the statistics
// max_abs_q u32 [B] and sum_abs_q u64 [B].  stats: a launch of the front kernel that gives the statistics alone (the
// shift is chosen from them).  apply: out = rec of (base, (sym << shift) + lo); status u32 [B] is nonzero for an image
// that holds a sym outside +-255.  All zero what they accumulate into on the stream, check their arguments before
// any HIP call and throw.
void image_residual_front_u16(const uint16_t* base, const int64_t* base_strides, const uint16_t* x,
                              const int64_t* x_strides, int B, int H, int W, int depth, int tau, int shift,
                              uint8_t* ctx, uint32_t* ctx_count, uint64_t* digest, int16_t* sym, uint64_t* lo_plane,
                              uint32_t* hist, uint32_t* max_err, uint32_t* max_abs_q, uint64_t* sum_abs_q,
                              hipStream_t st);
void image_residual_stats_u16(const uint16_t* base, const int64_t* base_strides, const uint16_t* x,
                              const int64_t* x_strides, int B, int H, int W, int depth, int tau, uint32_t* max_abs_q,
                              uint64_t* sum_abs_q, hipStream_t st);
void image_residual_apply_u16(const uint16_t* base, const int64_t* base_strides, const int16_t* sym,
                              const uint64_t* lo_plane, int B, int H, int W, int depth, int tau, int shift,
                              uint16_t* out, const int64_t* out_strides, const uint16_t* ref,
                              const int64_t* ref_strides, uint64_t* sq_err, uint32_t* max_err, uint32_t* status,
                              hipStream_t st);
// The device rANS coder of the segmented residual strings (residual_coder.hip; residual_seg.h has the definitions).
// sym int16 and ctx u8 are dense [B][N]; tabs, seg_off, seg_bytes [B][n_seg], total [B] and status [B] are device
// memory.  encode: a counting pass, a scan and a writing pass on `st`; image b's bytes go to out + b cap, each store
// checked.  decode: seg_off and seg_bytes come from the caller; q goes to sym.  Both reset status to RES_SEG_CLEAN on
// the stream; the caller has checked the arguments (residual_seg_check and its kin).
struct ResSegEncTable;
struct ResSegDecTable;
void residual_encode_segments(const int16_t* sym, const uint8_t* ctx, int B, int64_t N, int L, int64_t n_seg,
                              const ResSegEncTable* tabs, uint8_t* out, size_t cap, uint32_t* seg_off,
                              uint32_t* seg_bytes, uint64_t* total, uint32_t* status, hipStream_t st);
void residual_decode_segments(const uint8_t* data, size_t stride, const uint32_t* seg_off, const uint32_t* seg_bytes,
                              const uint8_t* ctx, int B, int64_t N, int L, int64_t n_seg, const ResSegDecTable* tabs,
                              int16_t* sym, uint32_t* status, hipStream_t st);
// 8-bit Y'CbCr frame I/O (image_yuv.hip; DESIGN.md section 5 "YCbCr I/O").  The fields of mlic_yuv_desc.
struct YuvDesc {
  int32_t sub_x, sub_y, matrix, full_range, site_x, reserved[3];
};
// ingest: three byte planes, each through its own element strides {image, row, column} (Y: H x W; Cb, Cr:
// ceil(H / sub_y) x ceil(W / sub_x)) -> dst fp32 [B][3][Hp][Wp]: integer chroma upsampling to sixteenths, the
// fp32 matrix with every operation rounded once, clamp to [0, 1]; +0 in the padding, every element written.
// Checks its arguments before any HIP call and throws.
void image_ingest_yuv8(const uint8_t* y, const int64_t* y_strides, const uint8_t* cb, const int64_t* cb_strides,
                       const uint8_t* cr, const int64_t* cr_strides, const YuvDesc* desc, int B, int H, int W, float* dst,
                       int Hp, int Wp, hipStream_t st);
// egress: the H x W crop of src fp32 (element strides {image, channel, row}, column stride 1) -> the three byte
// planes (chroma filtered at luma resolution before rounding); with the three ref planes, sq_err [B][3] = the
// exact per-plane sums of squared byte differences.  Only the planes' bytes are written.
void image_egress_yuv8(const float* src, const int64_t* src_strides, int B, int H, int W, const YuvDesc* desc,
                       uint8_t* y, const int64_t* y_strides, uint8_t* cb, const int64_t* cb_strides, uint8_t* cr,
                       const int64_t* cr_strides, const uint8_t* ref_y, const int64_t* ref_y_strides,
                       const uint8_t* ref_cb, const int64_t* ref_cb_strides, const uint8_t* ref_cr,
                       const int64_t* ref_cr_strides, uint64_t* sq_err, hipStream_t st);
// 9..16-bit sample I/O (image_io16.hip; DESIGN.md section 5 "High-bit-depth I/O"): the four calls above for uint16
// words of depth d in [8, 16], LSB-aligned (msb 0: the sample is min(word, 2^d - 1)) or MSB-aligned (msb 1: the
// sample is word >> (16 - d); output words have zero low bits).  Strides in elements, pointers 2-byte aligned.
// The Y'CbCr calls take matrix 2 (BT.2020 non-constant-luminance) as well.  They check their arguments before any
// HIP call and throw.
void image_ingest_u16(const uint16_t* src, const int64_t* src_strides, int depth, int msb, int B, int H, int W,
                      float* dst, int Hp, int Wp, hipStream_t st);
void image_egress_u16(const float* src, const int64_t* src_strides, int B, int H, int W, int depth, int msb,
                      uint16_t* dst, const int64_t* dst_strides, const uint16_t* ref, const int64_t* ref_strides,
                      uint64_t* sq_err, hipStream_t st);
void image_ingest_yuv16(const uint16_t* y, const int64_t* y_strides, const uint16_t* cb, const int64_t* cb_strides,
                        const uint16_t* cr, const int64_t* cr_strides, const YuvDesc* desc, int depth, int msb, int B,
                        int H, int W, float* dst, int Hp, int Wp, hipStream_t st);
void image_egress_yuv16(const float* src, const int64_t* src_strides, int B, int H, int W, const YuvDesc* desc,
                        int depth, int msb, uint16_t* y, const int64_t* y_strides, uint16_t* cb,
                        const int64_t* cb_strides, uint16_t* cr, const int64_t* cr_strides, const uint16_t* ref_y,
                        const int64_t* ref_y_strides, const uint16_t* ref_cb, const int64_t* ref_cb_strides,
                        const uint16_t* ref_cr, const int64_t* ref_cr_strides, uint64_t* sq_err, hipStream_t st);
// host logic only: the refusals of the two calls above that do not need the shapes (depth, msb, the descriptor with
// matrix in {0, 1, 2}, 2-byte alignment of the three plane pointers), each thrown with `who` in front, for callers
// that must refuse before they touch a device
void image_yuv16_check(const YuvDesc* desc, int depth, int msb, const void* y, const void* cb, const void* cr,
                       const char* who);
// Residual coding's two passes over the planes of Y'CbCr frames (residual_yuv.hip; residual_yuv.h has the definitions;
// DESIGN.md section 5 "Residual coding", "Y'CbCr frames").  word_bytes 1: byte planes, depth 8, msb 0, shift 0 and a
// null lo_plane; word_bytes 2: uint16 planes, depth 9..16, msb 0 / 1, shift 0..depth - 7.  Planes come as {y, cb, cr}
// pointers with element strides {image, row, column}; of desc only sub_x / sub_y are used, the rest is validated as
// the egress validates it.  ctx u8 and sym int16 are dense [B][N] in the canonical order, N = H W + 2 hc wc.
// front: ctx, ctx_count [B][24] and digest [B] always; with the three x planes (all null without) also sym, lo_plane
// (u64 [B][shift (H G_0 + 2 hc G_1)], null at shift 0), hist [B][24][128], max_err, max_abs_q [B] and sum_abs_q [B].
// stats: the last two alone.  apply: the three out planes = rec of (base, (sym << shift) + lo); with the three ref
// planes sq_err u64 [B][3] (per plane) and max_err u32 [B]; status u32 [B] is nonzero for a frame that holds a sym
// outside +-255 (such a sample is written as base).  All zero what they accumulate into on the stream, check their
// arguments before any HIP call and throw with `who` in front.
void image_residual_front_planes(const char* who, int word_bytes, const void* const base[3],
                                 const int64_t* const base_strides[3], const void* const x[3],
                                 const int64_t* const x_strides[3], const YuvDesc* desc, int depth, int msb, int B, int H,
                                 int W, int tau, int shift, uint8_t* ctx, uint32_t* ctx_count, uint64_t* digest,
                                 int16_t* sym, uint64_t* lo_plane, uint32_t* hist, uint32_t* max_err,
                                 uint32_t* max_abs_q, uint64_t* sum_abs_q, hipStream_t st);
void image_residual_stats_planes(const char* who, int word_bytes, const void* const base[3],
                                 const int64_t* const base_strides[3], const void* const x[3],
                                 const int64_t* const x_strides[3], const YuvDesc* desc, int depth, int msb, int B, int H,
                                 int W, int tau, uint32_t* max_abs_q, uint64_t* sum_abs_q, hipStream_t st);
void image_residual_apply_planes(const char* who, int word_bytes, const void* const base[3],
                                 const int64_t* const base_strides[3], const int16_t* sym, const uint64_t* lo_plane,
                                 const YuvDesc* desc, int depth, int msb, int B, int H, int W, int tau, int shift,
                                 void* const out[3], const int64_t* const out_strides[3], const void* const ref[3],
                                 const int64_t* const ref_strides[3], uint64_t* sq_err, uint32_t* max_err,
                                 uint32_t* status, hipStream_t st);
// tiled decode's egress: the h x w region at (y0, x0) of the H x W image, blended from the tiles of the grid
// (container.h: tile T, overlap V) with feathered seams, as uint8 through dst's {row, column, channel} strides.
// tiles_dev: the device table, tile index (row-major) -> that tile's contiguous fp32 [3][pad64(ey)][pad64(ex)]
// planes or null; tiles_host: the same table on the host, from which a region whose covering tile is null is
// refused.  Per value acc (double) = sum over the covering tiles, tile row then column, of (double)(wy * wx) *
// (double)v; (float)acc then goes through egress's conversion.  With ref ({row, column, channel} strides of the
// region's crop of the original), *sq_err = the exact sum of squared uint8 differences.
void image_tile_blend_u8(const float* const* tiles_dev, const float* const* tiles_host, int H, int W, int T, int V,
                         int y0, int x0, int h, int w, uint8_t* dst, const int64_t* dst_strides, const uint8_t* ref,
                         const int64_t* ref_strides, uint64_t* sq_err, hipStream_t st);
// ROI coding (roi.hip).  All three check their arguments before any HIP call and throw.
// levels [B][hz][wz] (hz, wz = ceil(H / 64), ceil(W / 64)) of a uint8 mask read through element strides {image,
// row, column}: level = lo + ceil((hi - lo) * count / area) per 64 x 64 cell clipped to the image, in integers
constexpr int ROI_MAX_LEVELS = 16;  // a level is four bits in the file
void roi_levels_u8(const uint8_t* mask, const int64_t* mask_strides, int B, int H, int W, int lo, int hi,
                   uint8_t* levels, hipStream_t st);
// g [B][4 hz][4 wz] = gains[levels[b][i >> 2][j >> 2]] (gains: n_levels <= 16 host floats, finite and positive)
void roi_gain_plane(const uint8_t* levels, int B, int hz, int wz, const float* gains, int n_levels, float* g,
                    hipStream_t st);
// out [B][4] = {sq_err inside, pixels inside, sq_err outside, pixels outside} of two uint8 images ({image, row,
// column, channel} strides each) split by a uint8 mask ({image, row, column}); exact integer sums
void sq_err_roi_u8(const uint8_t* a, const int64_t* a_strides, const uint8_t* b, const int64_t* b_strides,
                   const uint8_t* mask, const int64_t* mask_strides, int B, int H, int W, uint64_t* out,
                   hipStream_t st);
// Rate and error maps (ratemap.hip; DESIGN.md §5 "Rate maps").  All check their arguments before any HIP call
// and throw.
// y_lik [B][M][h][w], z_lik [B][N][h/4][w/4] (dense per image, batch strides y_bs / z_bs in floats) ->
// y_map [B][S][h][w] (per latent pixel the slice's M / S channel terms -(double)log2f(lik), ascending, from +0.0),
// z_map [B][h/4][w/4] (the N terms likewise), cell_bits [B][h][w] = ((z_map[i/4][j/4] / 16 + y_map[0]) + ...) +
// y_map[S-1], slice_bits [B][S+1] (the sum of each y_map[s] and of z_map in ratemap.hip's fixed order).  y_map and
// z_map are required here (the C entry puts scratch in a missing one's place); cell_bits / slice_bits may be null.
// rate_map_check alone: the refusals, with every output optional but one.
void rate_map_check(const float* y_lik, int64_t y_bs, const float* z_lik, int64_t z_bs, int B, int M, int S, int h, int w,
                    int N, const double* y_map, const double* z_map, const double* cell_bits, const double* slice_bits);
void rate_map(const float* y_lik, int64_t y_bs, const float* z_lik, int64_t z_bs, int B, int M, int S, int h, int w,
              int N, double* y_map, double* z_map, double* cell_bits, double* slice_bits, hipStream_t st);
// out [B][ceil(H / block)][ceil(W / block)] = the sum of squared byte differences of two uint8 images ({image, row,
// column, channel} strides each) over each block x block square clipped to H x W, three channels; block in
// {8, 16, 32, 64}; integers, every element written
void sq_err_blocks_u8(const uint8_t* a, const int64_t* a_strides, const uint8_t* b, const int64_t* b_strides, int B,
                      int H, int W, int block, uint32_t* out, hipStream_t st);
// plane [B][ph][pw] (doubles) drawn at H x W as uint8 RGB through dst's {image, row, column, channel} strides: pixel
// (y, x) shows cell (y / cell, x / cell), q = clamp(floor((v - lo) / (hi - lo) * 255 + 0.5), 0, 255) in separately
// rounded double operations, cmap 0 = gray (q, q, q), 1 = hot (min(255, 3q), clamp(3q - 255), clamp(3q - 510)),
// blended over `under` (optional, its own strides) as (alpha * colour + (256 - alpha) * under + 128) >> 8; a NaN
// cell is (255, 0, 255) unblended.  One launch.
void image_heat_u8(const double* plane, int B, int ph, int pw, int cell, double lo, double hi, int cmap, int H, int W,
                   uint8_t* dst, const int64_t* dst_strides, const uint8_t* under, const int64_t* under_strides,
                   int alpha, hipStream_t st);
// mlic_set_kernel_option("image_io_path"): -1 = by layout (default), 0 = the general-stride kernels, 1 = the
// interleaved (HWC) form, 2 = the planar (CHW) form; a forced form the layout does not fit is an error
// GaussianConditional likelihood (vbr_scale != 1: of y*sc, s*sc, m*sc) and build_indexes, element-wise
void gauss_likelihood(const float* y, const float* s, const float* m, int64_t n, float vbr_scale, float* lik,
                      hipStream_t st);
void scale_indexes(const float* s, int64_t n, const float* table, int ntable, int32_t* idx, hipStream_t st);

// fused 1x1 chain (chain.hip): layer widths cout[0..nl-1] in {320,256,128,64|128} (EntropyParameters)
// or {128,64} (LocalContext MLP), GELU between layers; weights pre-packed by chain_pack per layer,
// concatenated
struct ChainParams {
  Seg seg[MAXSEG];
  int nseg, cin0;  // layer-0 input: channel concat, cin0 % 32 == 0
  int HW, B;       // pixels per image (HW % 4 == 0)
  const float* bias[4];
  int wexp[4];       // each layer's split weights are w * 2^wexp (split_weights)
  const _Float16* wimg;
  float* out;      // [B][cout[nl-1]][HW] (batch stride out_bs)
  int64_t out_bs;
  const float* res;  // optional residual added to the output (same layout, batch stride res_bs)
  int64_t res_bs;
  int* rflag;        // fp16 range guard (common.h range_check)
  const float* aux;  // optional [B][C1][HW] added to layer 0's pre-activation (hoisted part of layer 0)
  int64_t aux_bs;
  // checkerboard half: 0 = every pixel; 1 = the anchor pixels only ((y + x) odd), 2 = the non-anchor
  // pixels only (W even): the other half of every output plane is not written.  EntropyParameters'
  // outputs are read at their own phase's pixels only (ckbd_anchor / ckbd_nonanchor masks,
  // mlicpp.py:226-228, 239-241; quant_phase / phase_indexes / phase_dequant read `mine` pixels)
  int ckbd, W;
  int sq_in;  // with ckbd: the inputs and the residual are squeezed planes of HW / 2 pixels (pixel q at q)
};
bool chain_supported(int nl, const int* cout);
int64_t chain_layer_halves(int Cout, int Cin);
void chain_pack(const _Float16* wh, const _Float16* wl, int Cout, int Cin, int cin_pad, int permute, _Float16* dst,
                hipStream_t st);
void chain_forward(const ChainParams& P, int nl, const int* cout, hipStream_t st);
// mlic_set_kernel_option("chain_nj"): 16-pixel column blocks per wave (-1 = $MLIC_CHAIN_NJ or 1; 2 = the
// rounds 2-5 four-wave form); the same bits either way

}  // namespace mlic
