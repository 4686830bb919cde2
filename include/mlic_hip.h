/* mlic_hip — MI355X-native (gfx950) MLIC++ encode/decode: C ABI.
 *
 * Drop-in boundary for the reference's CompressionModel API (MLIC++/models/mlicpp.py):
 *   mlic_create / mlic_destroy ........ MLICPlusPlus.__init__ + load_state_dict (mlicpp.py:14-77, 461-468);
 *                                       weights are the reference state_dict tensors, by name
 *   mlic_forward ...................... MLICPlusPlus.forward (mlicpp.py:79-185); VBR: mlicpp_vbr.py:137-519
 *   mlic_set_entropy_tables ........... GaussianConditional/EntropyBottleneck CDF buffers after update()
 *                                       (mlicpp.py:470-475; compressai _quantized_cdf/_cdf_length/_offset)
 *   mlic_compress / mlic_encoded_* .... MLICPlusPlus.compress (mlicpp.py:199-290) incl. the rANS coder
 *   mlic_decompress ................... MLICPlusPlus.decompress (mlicpp.py:292-378)
 *   mlic_pmf_to_quantized_cdf ......... compressai._CXX.pmf_to_quantized_cdf (used by update())
 *   mlic_rans_encode / mlic_rans_decode  compressai.ans.RansEncoder.encode_with_indexes /
 *                                       RansDecoder.decode_with_indexes (byte-compatible)
 *
 * Conventions: every function returns 0 on success, nonzero on error (message via mlic_last_error(),
 * thread-local); no C++ exception crosses the ABI.  Tensors are caller-owned device buffers, NCHW
 * fp32, contiguous.  `stream` is a hipStream_t (NULL = default stream); calls on one handle are
 * serialised on that stream.  The library owns its packed weights and a per-handle workspace.
 */
#ifndef MLIC_HIP_H
#define MLIC_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mlic_model mlic_model;

const char* mlic_last_error(void);
const char* mlic_version(void);

/* names/ptrs: n float32 device tensors (state_dict entries, plus "__scale_table" [64]);
 * shapes: n*4 int64 (unused dims 1), ndims: n */
int mlic_create(const char* model_name, int n, const char* const* names, const float* const* ptrs,
                const int64_t* shapes, const int* ndims, void* stream, mlic_model** out);
int mlic_destroy(mlic_model* m);

/* x [B,3,H,W] (H, W multiples of 64) -> x_hat [B,3,H,W], y_lik [B,M,H/16,W/16], z_lik [B,N,H/64,W/64];
 * outputs may be NULL.  vbr_scale = Gain[s] for *_VBR models (ignored otherwise, pass 1). */
int mlic_forward(mlic_model* m, void* stream, const float* x, int B, int H, int W, float* x_hat, float* y_lik,
                 float* z_lik, float vbr_scale);
/* *_v: one VBR gain per image (host array of B floats; NULL = 1), so one batch mixes levels
 * (BASELINE config 5); equal to B calls with the scalar form, bit for bit */
int mlic_forward_v(mlic_model* m, void* stream, const float* x, int B, int H, int W, float* x_hat, float* y_lik,
                   float* z_lik, const float* vbr_scales);

int mlic_set_entropy_tables(mlic_model* m, const int32_t* gc_cdf, const int32_t* gc_len, const int32_t* gc_off,
                            int gc_n, int gc_stride, const int32_t* eb_cdf, const int32_t* eb_len,
                            const int32_t* eb_off, int eb_n, int eb_stride);

/* compress/decompress split a batch over `lanes` host threads, each with its own HIP stream and
 * workspace, so the host rANS coding of one lane overlaps the kernels of another (default 4, or
 * $MLIC_LANES).  Results are identical for any lane count. */
int mlic_set_lanes(mlic_model* m, int lanes);
/* the lanes' HIP stream priorities are staggered (lane 0 highest, $MLIC_LANE_PRIORITY=0 disables); `base`
 * offsets this model's lanes (lane i at greatest + base + i, clamped to the device's range), so request
 * streams served by separate models drift apart as well.  Applies to lanes created afterwards (a model
 * creates its lanes on first use).  Scheduling only: results do not depend on it. */
int mlic_set_priority_base(mlic_model* m, int base);
int mlic_compress(mlic_model* m, void* stream, const float* x, int B, int H, int W, float vbr_scale);
int mlic_compress_v(mlic_model* m, void* stream, const float* x, int B, int H, int W, const float* vbr_scales);
int mlic_encoded_size(mlic_model* m, int b, size_t* y_len, size_t* z_len);
int mlic_encoded_copy(mlic_model* m, int b, uint8_t* y, uint8_t* z);
/* the coder inputs of image b from the last compress(): y symbols/indexes (all phases, coder order)
 * and z symbols; pass NULL buffers to query the counts */
int mlic_encoded_streams(mlic_model* m, int b, int64_t* n_y, int64_t* n_z, int32_t* y_sym, int32_t* y_idx,
                         int32_t* z_sym);
/* sum of -log2 of image b's y / z likelihoods in the last compress(): bpp_lik = (y + z) / (H * W) of the
 * unpadded image (loss/rd_loss.py:42-45) */
int mlic_encoded_bits(mlic_model* m, int b, double* y_bits, double* z_bits);
/* the reference's batched layout (models/mlicpp.py:215, 279-281: one y stream for a B > 1 batch,
 * phase-major and image-minor; strings = [[y], [z_0 .. z_B-1]]): images [first, first + count) of the
 * last compress coded into one stream (out = NULL queries the length; the coding runs on every call) */
int mlic_batch_stream(mlic_model* m, int first, int count, uint8_t* out, size_t cap, size_t* len);
/* decode such a stream (mlicpp.py:306-307 decodes strings[0][0] for the whole batch): one lane, the
 * images of each phase in order */
int mlic_decompress_batch_stream(mlic_model* m, void* stream, const uint8_t* y, size_t y_len, const uint8_t* const* z,
                                 const size_t* z_len, int B, int hz, int wz, float* x_hat, const float* vbr_scales);
/* y[b], z[b]: host byte strings of image b; hz, wz = latent z grid (shape returned by compress) */
int mlic_decompress(mlic_model* m, void* stream, const uint8_t* const* y, const size_t* y_len,
                    const uint8_t* const* z, const size_t* z_len, int B, int hz, int wz, float* x_hat,
                    float vbr_scale);
int mlic_decompress_v(mlic_model* m, void* stream, const uint8_t* const* y, const size_t* y_len,
                      const uint8_t* const* z, const size_t* z_len, int B, int hz, int wz, float* x_hat,
                      const float* vbr_scales);

/* ---- Progressive coding (DESIGN.md §5 "Progressive coding") ----
 * The entropy model is causal over the S channel slices, so the first K slices of any file decode exactly and the
 * rest can be filled with what the decoder knows without bits.
 * mlic_layer_streams: image b of the last compress as S rANS strings, one per slice (string k = the coder inputs
 * of phases 2 k and 2 k + 1, the lists the single string codes).  ptrs / lens: cap entries each, or NULL to query
 * *n = S; the pointers stay valid until the model's next compress.  Refused after mlic_compress_g.
 * mlic_decompress_prefix: y holds B * strings_per_image strings, image-major.  strings_per_image = 1: today's
 * single string (the decoder reads forward, so a prefix of its phases needs nothing new in the file);
 * >= slices: one string per slice, of which the first `slices` are read.  slices in [0, S] are entropy-decoded.
 * fill 0 (mean): the remaining slices run through the slice loop as if all their symbols were 0 (y_hat = 0.0f +
 * mean, LRP as in a decode), with no index kernel, copy, host decode or synchronisation; fill 1 (zero): the loop
 * stops after slice `slices` - 1 and the remaining channels of y_hat are cleared.  slices = S with fill 0 issues
 * exactly the launches of mlic_decompress_v.  Refused before any GPU call, each with its own message: slices
 * outside [0, S]; fill not 0 or 1; strings_per_image < 1, or > 1 and below slices; a null string among those
 * that are read. */
int mlic_layer_streams(mlic_model* m, int b, const uint8_t** ptrs, size_t* lens, int cap, int* n);
int mlic_decompress_prefix(mlic_model* m, void* stream, const uint8_t* const* y, const size_t* y_len,
                           int strings_per_image, const uint8_t* const* z, const size_t* z_len, int B, int hz, int wz,
                           int slices, int fill, const float* vbr_scales, float* x_hat);

/* ---- ROI coding on *_VBR models (DESIGN.md §5 "ROI coding") ----
 * The VBR gain is a quantisation step: y_hat = round((y - mu) * g) / g + mu, the table index from sigma * g, the
 * likelihood at (y, sigma, mu) * g.  The _g forms of forward / compress / decompress take it per latent pixel:
 * gain_plane = device fp32 [B][H/16][W/16] (decompress: [B][4 hz][4 wz]) in place of vbr_scales, produced on
 * `stream`.  The library derives the reciprocal plane itself (one small kernel per call, the correctly rounded
 * fp32 1 / g), so a constant plane gives exactly the bits and bytes of the scalar call with that gain.  z, the
 * hyperprior, the contexts, LRP and g_s do not see the plane.  Every value must be finite and positive: that
 * is the caller's contract and is not checked on the device (mlic_roi_gain_plane keeps it).  Encoder and
 * decoder must use bit-identical planes.  Per-image strings only: mlic_batch_stream refuses the images of a
 * mlic_compress_g, and mlic_decompress_g wants one y string per image.  Refused before any GPU call, each with
 * its own message: a model that is not *_VBR; a null plane; a missing y string. */
int mlic_forward_g(mlic_model* m, void* stream, const float* x, int B, int H, int W, float* x_hat, float* y_lik,
                   float* z_lik, const float* gain_plane);
int mlic_compress_g(mlic_model* m, void* stream, const float* x, int B, int H, int W, const float* gain_plane);
int mlic_decompress_g(mlic_model* m, void* stream, const uint8_t* const* y, const size_t* y_len,
                      const uint8_t* const* z, const size_t* z_len, int B, int hz, int wz, float* x_hat,
                      const float* gain_plane);
/* mask -> level map.  mask: uint8 on the device, nonzero = inside the ROI, read in place through element strides
 * {image, row, column}; levels: uint8 [B][hz][wz] (device) on the z grid, hz = ceil(H / 64), wz = ceil(W / 64),
 * one cell per 64 x 64 pixel block clipped to H x W.  In integers:
 *     level = lo + ceil((hi - lo) * count / area)
 * with count the cell's nonzero mask pixels and area its pixels inside the image (>= 1): lo where the cell holds
 * no ROI pixel, hi where it is all ROI, and any ROI pixel lifts the cell above lo.  One launch, deterministic,
 * asynchronous on `stream`.  Refused before any GPU call: null arguments; B, H or W < 1; lo > hi; lo < 0 or
 * hi > 255. */
int mlic_image_roi_levels_u8(void* stream, const uint8_t* mask, const int64_t* mask_strides, int B, int H, int W, int lo,
                             int hi, uint8_t* levels);
/* level map -> gain plane, nearest expansion: g[b][i][j] = gains_host[levels[b][i >> 2][j >> 2]] over the latent
 * grid [B][4 hz][4 wz] (device fp32).  gains_host: n_levels <= 16 host floats (|Gain| of the model), each finite
 * and positive; a level >= n_levels (excluded by mlic_container_parse_roi) reads the last entry.  Encoder and
 * decoder both build their plane with this one kernel from the same bytes.  Asynchronous on `stream`. */
int mlic_roi_gain_plane(void* stream, const uint8_t* levels, int B, int hz, int wz, const float* gains_host,
                        int n_levels, float* g);
/* Squared error inside and outside the ROI: a, b uint8 images (device) with {image, row, column, channel}
 * strides, mask as above; out: [B][4] uint64 (device) = {squared error inside, pixels inside, squared error
 * outside, pixels outside}, the squared error summed over the three channels.  Exact integer sums (integer
 * atomics: independent of scheduling), so PSNR_roi = 10 log10(255^2 * 3 * pixels / sq_err) comes with it;
 * inside + outside is mlic_image_egress_u8's sq_err.  Asynchronous on `stream`. */
int mlic_image_sq_err_roi_u8(void* stream, const uint8_t* a, const int64_t* a_strides, const uint8_t* b,
                             const int64_t* b_strides, const uint8_t* mask, const int64_t* mask_strides, int B, int H,
                             int W, uint64_t* out);

/* Rate maps: where the entropy model's bits lie.  y_lik: fp32 [B][M][h][w] and z_lik: fp32 [B][N][h/4][w/4] on the
 * device (mlic_forward's likelihood tensors), each image dense, y_bs / z_bs the batch strides in floats.  Outputs
 * (device doubles; each may be NULL, at least one is given):
 *   y_map [B][S][h][w]   per latent pixel, the sum over the slice's M / S channels, ascending, from +0.0, of
 *                        -(double)log2f(lik) -- the per-element term of mlic_neglog2_sum and mlic_encoded_bits
 *   z_map [B][h/4][w/4]  the same sum over the N channels of z
 *   cell_bits [B][h][w]  ((z_map[i/4][j/4] / 16 + y_map[0][i][j]) + y_map[1][i][j]) + ... + y_map[S-1][i][j]
 *   slice_bits [B][S+1]  the total of y_map[0 .. S-1] and, last, of z_map.  Per row, lane l of 64 adds elements l,
 *                        l + 64, ... from +0.0, the 64 sums are folded in halves (l += l + 32, 16, 8, 4, 2, 1);
 *                        the row sums are added top to bottom from +0.0.
 * A likelihood of 1 adds +0.0 (no -0.0 reaches an output), a NaN likelihood gives a NaN cell, every element is
 * written, and the bits do not depend on B, the image's place in the batch or the strides.  Two launches on
 * `stream`.  With y_map and z_map both given the call is asynchronous; a missing one that cell_bits / slice_bits
 * need is computed into scratch the call allocates, and the call then waits for the stream before it frees it.
 * Refused before any GPU call: null likelihoods or no output; B, M, S, N, h or w < 1; M % S; h % 4 or w % 4; a
 * batch stride below one image; B, M or N above 2^20. */
int mlic_rate_map_run(void* stream, const float* y_lik, int64_t y_bs, const float* z_lik, int64_t z_bs, int B, int M,
                      int S, int h, int w, int N, double* y_map, double* z_map, double* cell_bits, double* slice_bits);
/* Error map: out [B][ceil(H / block)][ceil(W / block)] uint32 (device) = the sum of squared byte differences of the
 * uint8 images a and b ({image, row, column, channel} strides each, read in place) over each block x block square
 * clipped to H x W, three channels (<= 64 * 64 * 3 * 255^2).  Integers; the grid's sum is mlic_image_egress_u8's
 * sq_err.  One launch, asynchronous.  Refused: null arguments; B, H or W < 1; a block other than 8, 16, 32, 64; a
 * zero column or channel stride; strides whose last byte offset overflows int64. */
int mlic_image_sq_err_blocks_u8(void* stream, const uint8_t* a, const int64_t* a_strides, const uint8_t* b,
                                const int64_t* b_strides, int B, int H, int W, int block, uint32_t* out);
/* Heat map: plane [B][ph][pw] (device doubles; ph * cell >= H, pw * cell >= W) drawn at H x W as uint8 RGB through
 * dst's {image, row, column, channel} strides.  Pixel (y, x) shows cell (y / cell, x / cell); cell in {8, 16, 32,
 * 64} (16: cell_bits / y_map, 64: z_map, block: an error map converted to double).
 *     q = clamp(floor((v - lo) / (hi - lo) * 255 + 0.5), 0, 255)      each operation a rounded double operation
 * (+-inf clamp), cmap 0 = gray: (q, q, q); 1 = hot: (min(255, 3q), clamp(3q - 255, 0, 255), clamp(3q - 510, 0, 255)).
 * With `under` (uint8, its own strides; NULL: none) out = (alpha * colour + (256 - alpha) * under + 128) >> 8,
 * alpha in [0, 256]; a NaN cell is (255, 0, 255), unblended.  One launch, asynchronous; only the image's bytes are
 * written.  Refused: null plane / dst / strides; sizes < 1; a bad cell, cmap or alpha; a plane that does not cover
 * the image; lo or hi not finite, or hi <= lo; alpha < 256 without `under`; zero or overflowing strides. */
int mlic_image_heat_u8(void* stream, const double* plane, int B, int ph, int pw, int cell, double lo, double hi,
                       int cmap, int H, int W, uint8_t* dst, const int64_t* dst_strides, const uint8_t* under,
                       const int64_t* under_strides, int alpha);

/* module-level entry points (tests / profiling): which = local|chan|inter|intra|epa|epn|lrpa|lrpn|g_a|h_a|h_s|g_s|rbu|rbws */
int mlic_run_module(mlic_model* m, void* stream, const char* which, int idx, const float* in0, const float* in1,
                    int B, int Cin, int H, int W, float* out);
int mlic_workspace_bytes(mlic_model* m, size_t* arena, size_t* weights);

/* dense-conv arithmetic: 2 = split-fp16 MFMA "f16x3" v2 tiles + specialised kernels (default; error
 * below fp32 summation-order noise), 1 = f16x3 v1 tiles, 0 = fp32 MFMA.  Also $MLIC_PRECISION. */
int mlic_set_precision(mlic_model* m, int precision);
/* g_s only (synthesis.py:56-73): 0 = the model precision above (default), 1 = its dense
 * subpel convs on fp16 operands with fp32 accumulation (one MFMA term instead of three).  Changes
 * x_hat only (forward / decompress); bitstreams and likelihoods are unaffected.  Gate: |dPSNR| <= 0.01 dB.
 * Also $MLIC_SYNTH_FP16=1. */
int mlic_set_synthesis_precision(mlic_model* m, int mode);
/* test switch: fill every workspace block with NaN (0xFF bytes) when it is handed out, so a kernel
 * reading memory its producer never wrote fails visibly (also $MLIC_POISON=1).  Off by default. */
int mlic_set_poison(mlic_model* m, int on);
/* process-wide kernel A/B switches (tests, micro-benchmarks).  One table holds every switch, its
 * environment fallback and its rule (csrc/options.cpp).  Every entry point of this ABI takes one
 * snapshot of all of them when it is entered and reads nothing else until it returns -- its sizing pass
 * and its real pass, every lane thread it starts and every model pass of a budget encode see the same
 * values -- so a set from any thread is safe at any time and takes effect at the next call, never inside
 * one.  The environment is read once per process, at the library's first use.  A value of -1 (and for
 * "chain_nj" 0 too) returns an option to its environment variable or default; an unknown name, or an
 * "image_io_path" outside [-1, 2], is an error and changes nothing.  "x4_halo" = the conv_x4 kernel's
 * halo-staged B operand for K x K stride-1 convs (1 on, 0 off, -1 default = $MLIC_X4_HALO or on for 5 x 5
 * and 3 x 3; $MLIC_X4_HALO=5: 5 x 5 only) -- the same bits while the K loop is unsplit;
 * "linatt_fused" = the linear attention's output written straight into the
 * reprojection conv's packed operand ($MLIC_LINATT_FUSED); "dw_strip" = the register-strip depthwise
 * 3x3 for stride-1 planes up to 64 columns ($MLIC_DW_STRIP); "x4_splitk" = split-K for few-tile
 * 3x3 / 5x5 convs (default off, $MLIC_X4_SPLITK=1); "dwpw2" = the form of the fused depthwise +
 * pointwise for Cin = Cout in {96, 128, 160, 192} (-1 default = $MLIC_DWPW2 or 2: the register-row
 * dwpw3_kernel; 1 the row-pipelined LDS form, A/B-only library since round 6; 0 the round-4 dwpw_kernel) --
 * every form gives the same bits; "pw3" = the full-resolution 1x1 convs with Cin = Cout (GDN / IGDN at
 * 544 x 960) on that kernel's pointwise form (-1 default = $MLIC_PW3 or 1: from 256 K px per image; 2: every
 * grid; 0 = pw_resident, the same bits); "narrow_limit" = L: coder symbols outside [-L - 1, L] cross PCIe
 * as int32 (the encoder's overflow copy, the decoder's int32 re-decode) -- a test knob for those fallback
 * paths, bitstreams unchanged (L <= 0: the int16 range, the default); "chain_nj" = 16-pixel column blocks
 * per wave of the fused 1x1 chain (-1 default = $MLIC_CHAIN_NJ or 1; 2 = four waves of 32 pixels, the same
 * bits); "ep_half" = the slice loop's EntropyParameters chains (and its LocalContext, read by the non-anchor
 * EntropyParameters only) over their own phase's checkerboard half
 * (-1 default = $MLIC_EP_HALF or on; 0 = the whole grid: the same bits at every pixel that is read);
 * "image_io_path" = the form of the uint8 ingest / egress kernels (-1 default = by the byte image's strides;
 * 0 = the general-stride form, 1 = the interleaved HWC form, 2 = the planar CHW form; a forced form that the
 * strides do not fit is refused) -- every form gives the same bits.  Three switches for work whose result
 * nobody reads (the first two off by default: they did not move the benchmark beyond its spread): "lrp_half" = the LRP head (last
 * depthwise + point conv with 0.5 tanh, checkerboard mask and the residual into y_hat) on its phase's
 * checkerboard half only (-1 default = $MLIC_LRP_HALF or 0 = the whole grid; the same bits, except that under
 * 1 a residual of -0.0 at a masked pixel stays -0.0 instead of becoming +0.0); "intra_half" = the intra context
 * reads its masked inputs through the resident 1x1's input mask instead of two masked copies and, where its
 * consumer runs on the non-anchor half ("ep_half"), runs its last depthwise + 1x1 on that half (-1 default =
 * $MLIC_INTRA_HALF or 0 = the copies and the whole grid; 2 = as 1, and mlic_run_module("intra") takes the half
 * tail too: only its non-anchor pixels are then defined); "gdn_skip" = g_a's first 1x1 stride-2 skip conv
 * (3 -> N) computed inside the GDN launch that adds it, where "pw3" serves that launch (-1 default =
 * $MLIC_GDN_SKIP or on; 0 = its own launch; the same bits); "x4_epi" = the conv_x4 kernel's lean epilogue for
 * blocks whose whole tile is stored (-1 default = $MLIC_X4_EPI or 1 = for the tile classes that measured
 * faster with it: 3 x 3 convs, 1 x 1 convs on 128- / 256-row tiles; 2 = every tile class; 0 = the generic
 * epilogue for every block; the same bits) */
int mlic_set_kernel_option(const char* name, int value);
/* the effective value of a mlic_set_kernel_option name as the next call would see it, after the
 * option's own rule: what was set, else the environment, else the default ("x4_halo": 0 off, 1 = the
 * default forms, 2 = forced on, 5 = 5 x 5 only; "chain_nj": 1 or 2; "narrow_limit": 1 .. 32767; the on / off
 * switches: 0 or 1) */
int mlic_get_kernel_option(const char* name, int* value);
/* 1 when this library holds the A/B-only kernel families (v1 split-fp16 tiles = precision 1, the halo
 * tiles = conv impl 6, the VALU local attention = local-attention impl 0; `make AB=1`), else 0: the
 * product build fails those requests loudly */
int mlic_ab_families(int* built);
/* fp16 range-guard fallbacks taken since the last reset (each changes the arithmetic of one call):
 * forward re-run whole in exact fp32 (the entropy model left fp16's range; compress refuses such an
 * input), forward's g_s alone, decompress's g_s alone (the same policy on both sides, so
 * decompress(compress(x)) == forward(x) bit for bit whenever compress succeeds) */
int mlic_range_fallbacks(mlic_model* m, int64_t* forward_full, int64_t* forward_gs, int64_t* decompress_gs,
                         int reset);
/* live kernel timing (HIP events on the executor stream), one category per kernel family / tile
 * instantiation: mlic_profile_categories gives the count, mlic_profile_category_name the kernel
 * name of each.  read() sums and clears. */
int mlic_set_profiling(mlic_model* m, int on);
int mlic_profile_read(mlic_model* m, int cat, int64_t* launches, double* ms, double* flops, double* bytes);
/* tab-separated per-layer table (layer, category, launches, ms, GFLOP, TFLOP/s) of the recorded
 * conv events, sorted by time; call before mlic_profile_read (which clears) */
int mlic_profile_layers(mlic_model* m, char* buf, size_t cap, size_t* written);

int mlic_profile_categories(int* n);
/* host time summed over threads since the last reset: rANS encode, rANS decode, waits on the GPU */
int mlic_host_stats(mlic_model* m, double* enc_ms, double* dec_ms, double* wait_ms, int reset);
int mlic_profile_category_name(int cat, char* buf, size_t cap);

/* kernel-level entry points (bit-exact tests, micro-benchmarks) */
/* one conv layer with a given kernel family: impl -1 = the model's choice (precision 2), 0 fp32 MFMA,
 * 1 f16x3, 2 f16x3 v2, 3 resident-weight 1x1, 4 narrow 3x3, 5 small-Cin 1x1, 6 halo-tiled 3x3,
 * 7 x4 (split-fp16, both operands staged by LDS-DMA; K in 1, 3, 5, stride 1), 8 x4 with fp16 operands
 * (single term, fp32 accumulation: the reduced-precision synthesis form).  w is torch layout
 * [Cout][Cin][K][K]; pad = K/2; epi = Epi flags of common.h (aux for GDN, res for residual).
 * Synchronous on `stream`. */
int mlic_conv_run(void* stream, int impl, const float* x, const float* w, const float* bias, float* y, int B, int Cin,
                  int Cout, int H, int W, int K, int stride, int epi, const float* aux, const float* res);
/* the kernel family the model runs a conv layer of this shape with (precision 2; no GPU needed:
 * host logic only) -> *impl.  Depends on the layer and one image's grid, never on B: the decoder must
 * reproduce the encoder's entropy parameters bit for bit whatever batch either side uses. */
int mlic_conv_choice(int B, int Cin, int Cout, int H, int W, int K, int stride, int epi, int* impl);
/* depthwise 3x3 (pad 1, stride 1|2, optional GELU); w [C][9]; synchronous on `stream` */
int mlic_dw_run(void* stream, const float* x, const float* w, const float* bias, float* y, int B, int C, int H, int W,
                int stride, int gelu);
/* fused depthwise 3x3 (stride 1, pad 1; dww [C][9], dwb [C]) + pointwise 1x1 (w [Cout][C]) with
 * epi in {0, GELU} | RES (res: [B][Cout][H][W]); C, Cout in {128, 192}; synchronous on `stream` */
int mlic_dwpw_run(void* stream, const float* x, const float* dww, const float* dwb, const float* w, const float* bias,
                  float* y, int B, int C, int Cout, int H, int W, int epi, const float* res);
/* impl as mlic_conv_run (CONV_* ids), < 0 = the model's choice; epi = Epi flags (RES in place,
   GDN/IGDN with the input as operand) */
int mlic_bench_conv(int impl, int B, int Cin, int Cout, int H, int W, int K, int stride, int epi, int iters,
                    double* ms_per, double* tflops);
int mlic_local_attn_mask(void* stream, float* out, int H, int W); /* [H*W, 25, 25] of {0, -100} */
/* LocalContext window attention: qkv [B][3C][H*W] -> out [B][25C][H*W]; impl 0 = VALU, 1 = MFMA */
int mlic_local_attn_run(void* stream, int impl, const float* qkv, const float* rel_table, const int32_t* rel_index,
                        float* out, int C, int H, int W, int B, float scale);
/* LocalContext attention (dim 32) in conv_x4's packed split layout: out = uint16 (fp16 bits)
   [B][25][npos][64], npos = ceil(H*W / 32) * 32; channel k = head*16 + d, hi at k, lo at 32 + k */
int mlic_local_attn_packed_run(void* stream, const float* qkv, const float* rel_table, const int32_t* rel_index,
                               uint16_t* out, int H, int W, int B, float scale);
/* the same for one checkerboard phase's query pixels only (ckbd 1: anchors, (y + x) odd; 2: non-anchors;
   W even), written at the squeezed position y * W / 2 + x / 2: npos = ceil(H*W/2 / 32) * 32 (round 6: the
   slice loop's LocalContext, whose only consumer reads the non-anchor pixels) */
int mlic_local_attn_packed_half_run(void* stream, const float* qkv, const float* rel_table, const int32_t* rel_index,
                                    uint16_t* out, int H, int W, int B, float scale, int ckbd);
/* the number of key splits the model runs the linear attention of an H*W = HW latent with (host logic
 * only, no GPU touched): 1 <= *nsplit <= 64, every split of ceil(HW / *nsplit) keys non-empty */
int mlic_linatt_splits(int HW, int* nsplit);
/* linear attention (context.py:180-187 / 235-239), the model's three launches: k, v, q -> out, all fp32
 * [B][heads*hd][H*W], hd 16 or 32; ctx_out: optional [B][heads][hd][hd], ctx = softmax_L(K) . V^T per head;
 * nsplit <= 0: the model's choice (mlic_linatt_splits), else 1..64 key splits; kmask 1: only the anchor pixels
 * ((y + x) odd) are keys; qmask 1: only the non-anchor pixels have queries (out is 0 at anchors).  The entry
 * owns its workspace; synchronous on `stream` */
int mlic_linear_attention_run(void* stream, const float* k, const float* v, const float* q, float* out, float* ctx_out,
                              int B, int heads, int hd, int H, int W, int nsplit, int kmask, int qmask);
/* the fused form's second half: ctx^T . softmax_c(q) written in conv_x4's packed split layout for a stride-1
 * K x K conv (K 3 or 5, pad K/2) over [B][heads*hd][H][W] (heads*hd a multiple of 32): out_halves = uint16
 * (fp16 bits) [B][heads*hd/32][(H+K-1)*(W+K-1)][64], one line per position of the zero-padded image, hi of the
 * chunk's 32 channels at 0..31 and lo at 32..63; no range flag; synchronous on `stream` */
int mlic_linatt_pack_run(void* stream, const float* q, const float* ctx, uint16_t* out_halves, int B, int heads, int hd,
                         int H, int W, int K, int qmask);
/* nn.LayerNorm(C) over the channel axis of x [B][C][HW] (eps 1e-5; gamma, beta [C]), C in {32, 64, 128};
 * synchronous on `stream` */
int mlic_ln_channels_run(void* stream, const float* x, const float* gamma, const float* beta, float* y, int B, int C,
                         int HW);
/* the tail of g_s: part [B][108][H][W] (row tap*12 + c: the per-tap partial products of the N -> 12 3x3 conv)
 * -> out [B][3][2H][2W] = PixelShuffle(2)(bias + the nine shifted partials summed in tap order); bias [12] or
 * NULL; synchronous on `stream` */
int mlic_taps_gather_run(void* stream, const float* part, const float* bias, float* out, int B, int H, int W);

/* ---- the entropy front's kernels alone (no model handle).  Every argument is checked before any GPU call;
 * each entry is synchronous on `stream`. ----
 *
 * The slice loop's quantisation of one checkerboard phase of one latent slice, all device pointers.  Anchor
 * pixels are those with (h + w) odd; phase 0 codes the anchors, phase 1 the others.  Element strides between
 * images (`*_bs`) are the caller's: the model passes slices of wider tensors.  The squeezed streams (sym, idx,
 * sym16, idx8) are contiguous [B][C][H][W/2], an element of the phase at ((c * H + h) * (W / 2) + (w >> 1)).
 *   params    [2C][H][W] per image: scales at [0, C), means at [C, 2C), the phase's entropy parameters
 *   params_a  the anchor phase's, read for `lik` only: the likelihood takes (s, m) from params_a at anchor
 *             pixels and from params elsewhere
 *   vbr 0     q = rint(y - m), yh = q + m, index from s
 *   vbr 1     q = rint((y - m) * g), yh = q * r + m, index from s * g, likelihood at (y, s, m) * g; the gain g
 *             and its reciprocal r per image (sc, rs: [B]) or per latent pixel (scp, rsp: [B][H][W], which
 *             take precedence)
 *   index     (ntable - 1) - #{t in table[:-1] : max(s', 0.11) <= t}
 *   sym16     q saturated to [-nlim - 1, nlim]; *ovf is set to 1 if some symbol did not fit and is not
 *             written otherwise
 * mlic_quant_phase_run writes yh (phase 0: +0 at the other parity; phase 1: the anchor pixels are left as
 * they are), lik at every pixel when given, and whichever of sym, idx, sym16 + idx8 + ovf are given.  It
 * refuses: a null y, params, yh or table; W odd; phase outside {0, 1}; lik without params_a; sym16 without
 * idx8 and ovf (or those without sym16); idx without sym or sym16; one gain plane without the other; planes
 * without vbr; vbr with neither sc and rs nor planes; nlim outside 1..32767; ntable outside 2..256; B outside
 * 1..65535, H or W < 1, H * W or C * H * W above 2^30; a batch stride smaller than the tensor it strides.
 * mlic_phase_indexes_run (decoder) reads params, table, phase, vbr, sc or scp and the geometry and writes idx8
 * when given, else idx.  mlic_phase_dequant_run (decoder) reads sym16 when given, else sym, and params, phase,
 * vbr, rs or rsp, and writes yh as mlic_quant_phase_run does. */
typedef struct mlic_quant_desc {
  const float* y;
  int64_t y_bs;
  const float* params;
  int64_t params_bs;
  const float* params_a;
  int64_t params_a_bs;
  float* yh;
  int64_t yh_bs;
  float* lik;
  int64_t lik_bs;
  int32_t* sym;
  int32_t* idx;
  int16_t* sym16;
  uint8_t* idx8;
  int32_t* ovf;
  int32_t nlim;
  int32_t ntable;
  const float* table;
  int32_t phase;
  int32_t vbr;
  const float* sc;
  const float* rs;
  const float* scp;
  const float* rsp;
  int32_t B, C, H, W;
} mlic_quant_desc;
int mlic_quant_phase_run(void* stream, const mlic_quant_desc* d);
int mlic_phase_indexes_run(void* stream, const mlic_quant_desc* d);
int mlic_phase_dequant_run(void* stream, const mlic_quant_desc* d);
/* progressive decode, a slice that is not entropy-decoded: mlic_phase_dequant_run on all-zero symbols without the
 * symbols.  yh = 0.0f + m at the phase's pixels (phase 0: +0 at the other parity; phase 1: the anchor pixels are
 * left as they are); for every finite rs > 0 that is mlic_phase_dequant_run's result bit for bit (m = -0 gives +0
 * in both).  Reads params, phase and the geometry only: sym, sym16, idx8 and the gains may be null. */
int mlic_phase_fill_run(void* stream, const mlic_quant_desc* d);
/* r[i] = 1 / g[i], the correctly rounded fp32 quotient, i < n (the reciprocal of a gain plane); 1 <= n <= 2^31 */
int mlic_recip_plane_run(void* stream, const float* g, float* r, int64_t n);
/* EntropyBottleneck (eval) on z [B][C][H][W]: r = rint(z - med[c]), z_hat = r + med[c], sym = (int32) r, lik =
 * max(sigmoid(logits(z_hat + 0.5)) - sigmoid(logits(z_hat - 0.5)), 1e-9) with the factorised cumulative's
 * parameters quantiles [C][1][3] (med = [:, 0, 1]), _matrix0..4 (m0 [C][3][1], m1..m3 [C][3][3], m4 [C][1][3]),
 * _bias0..4 (b0..b3 [C][3][1], b4 [C][1][1]), _factor0..3 ([C][3][1]).  z_hat, lik and sym are each optional,
 * at least one must be given; B * C * H * W <= 2^31 */
int mlic_eb_forward_run(void* stream, const float* z, float* z_hat, float* lik, int32_t* sym, const float* quantiles,
                        const float* m0, const float* m1, const float* m2, const float* m3, const float* m4,
                        const float* b0, const float* b1, const float* b2, const float* b3, const float* b4,
                        const float* f0, const float* f1, const float* f2, const float* f3, int B, int C, int H,
                        int W);
/* the decoder's z_hat = (float) sym + med[c] on [B][C][H][W] */
int mlic_eb_dequant_run(void* stream, const int32_t* sym, const float* quantiles, float* z_hat, int B, int C, int H,
                        int W);
/* y = x at the anchor pixels ((h + w) odd) when keep_anchor is 1, at the others when 0, and +0 elsewhere; x, y
 * [C][H][W] per image with element strides x_bs, y_bs between images (each >= C * H * W) */
int mlic_ckbd_mask_run(void* stream, const float* x, int64_t x_bs, float* y, int64_t y_bs, int B, int C, int H, int W,
                       int keep_anchor);
int mlic_image_sq_err_u8(void* stream, const float* a, const float* b, int B, int64_t n_per, double* out);
/* bytes of device scratch mlic_image_ms_ssim_u8 needs (pooled planes + partial sums); host logic only,
 * no GPU touched; nonzero rc with a message when C < 1, B < 1 or min(H, W) <= 160 */
int mlic_ms_ssim_scratch_bytes(int B, int C, int H, int W, size_t* bytes);
/* per-image MS-SSIM (pytorch_msssim defaults, data_range 255: DESIGN.md §3) of two [B][C][H][W] fp32 images
 * in [0,1], made uint8-valued as mlic_image_sq_err_u8 does; element strides {image, channel, row} per
 * operand (column stride 1), so a crop of a padded x_hat is scored in place; out: B doubles (device);
 * terms: optional B*5*C doubles (device), the relu'd per-level per-channel cs / ssim means, level-major
 * within an image; asynchronous on `stream`.  Arguments are checked before any GPU call; nothing outside
 * scratch[0, bytes), out and terms is written.  Bit-reproducible, and independent of B. */
int mlic_image_ms_ssim_u8(void* stream, const float* a, const int64_t* a_strides, const float* b,
                          const int64_t* b_strides, int B, int C, int H, int W, void* scratch,
                          size_t scratch_bytes, double* out, double* terms);

/* ---- LPIPS-VGG: lpips.LPIPS(net="vgg", version="0.1")(a/255, b/255, normalize=True) in eval mode, restated in
 * DESIGN.md §3, of two [B][3][H][W] fp32 images in [0,1] made uint8-valued as mlic_image_sq_err_u8 does ----
 *
 * create: the weights as device fp32 tensors in the table form of mlic_create.  13 conv weights [Cout][Cin][3][3]
 * and 13 biases, matched by the vgg16().features index that ends their name ("net.slice1.0.weight" and
 * "0.weight" are the same tensor; indices 0 2 5 7 10 12 14 17 19 21 24 26 28); five "lin{k}.model.1.weight"
 * [1][C][1][1] ("lins.*" duplicates are ignored); optionally "scaling_layer.shift" and "scaling_layer.scale"
 * [1][3][1][1] (default: the package's constants).  A missing tensor, an extra conv tensor or any other
 * unexpected name, and a mis-shaped tensor are refused, each with a message naming the tensor.  The weights are
 * packed once; the caller's tensors are not referenced after the call returns.  A handle serves one call at a
 * time. */
typedef struct mlic_lpips mlic_lpips;
int mlic_lpips_create(int n, const char* const* names, const float* const* ptrs, const int64_t* shapes,
                      const int* ndims, void* stream, mlic_lpips** out);
int mlic_lpips_destroy(mlic_lpips* h);
/* the dense convs' kernel family: 2 = split-fp16 conv_x4 (default), 0 = the fp32 MFMA conv */
int mlic_lpips_set_precision(mlic_lpips* h, int precision);
/* bytes of device scratch mlic_image_lpips_u8 needs; host logic only, no GPU touched; nonzero rc with a message
 * when B < 1, H or W < 16, or H * W > 2^23.  The B pairs are processed in chunks sized so that the scratch stays
 * under 4 GiB (one 1920x1088 pair needs about 3.5 GiB; a single pair above 4 GiB is its own chunk), so the
 * need grows with B only up to that cap.  It depends on the kernel options in force (x4_splitk). */
int mlic_lpips_scratch_bytes(int B, int H, int W, size_t* bytes);
/* per-pair LPIPS; element strides {image, channel, row} per operand (column stride 1), so a crop of a padded
 * x_hat is scored in place; out: B doubles (device); terms: optional B*5 doubles (device), the five taps'
 * terms whose sum (in tap order) is the value.  Checked before any GPU call, each with its own message: null
 * handle; B < 1; H or W < 16; null images; scratch too small or not 256-byte aligned; null out.  Nothing outside
 * scratch[0, bytes), out and terms is written, and no scratch element is read that this call did not write.
 * Identical operands give exactly 0.  Bit-reproducible, and independent of B and of the chunking.
 * fp16 range guard: at precision 2 the call waits for `stream` once to read the guard's flag; when an operand of
 * a dense conv left fp16's range (|v| >= 65520) the WHOLE call runs again with the fp32 MFMA convs and is
 * counted, so in such a call the images that did not overflow also carry the fp32 family's bits (which may
 * differ from their split-fp16 result within the accuracy gate).  At precision 0 the call is asynchronous. */
int mlic_image_lpips_u8(mlic_lpips* h, void* stream, const float* a, const int64_t* a_strides, const float* b,
                        const int64_t* b_strides, int B, int H, int W, void* scratch, size_t scratch_bytes,
                        double* out, double* terms);
/* stage timing (tools/lpips_bench.py): ms3 (optional, 3 doubles) = device-event milliseconds of {the stem, the
 * twelve dense convs with their operand packs, the tap launches with the reduce} summed over the calls since the
 * last read, then cleared; `on` switches the timing for the calls that follow (a timed call waits for `stream`) */
int mlic_lpips_profile(mlic_lpips* h, int on, double* ms3);
/* calls that were re-run in fp32 by the range guard since the last reset */
int mlic_lpips_range_fallbacks(mlic_lpips* h, int64_t* count, int reset);

/* ---- DISTS: DISTS_pytorch 0.1's DISTS()(a/255, b/255) in eval mode, restated in DESIGN.md §3, of two
 * [B][3][H][W] fp32 images in [0,1] made uint8-valued as mlic_image_sq_err_u8 does.  The same VGG16 trunk as
 * LPIPS with L2 pooling (3x3 Hanning, stride 2, ceil grids) and a head of per-channel means, variances and
 * covariances over six feature sets (the image and five taps, 1475 channels) ----
 *
 * create: the table form of mlic_lpips_create.  The 13 conv weights and biases by their trailing features index
 * ("stage2.5.weight" and "5.weight" are the same tensor); "alpha" and "beta" [1][1475][1][1]; optionally "mean"
 * and "std" [1][3][1][1] (default 0.485 0.456 0.406 / 0.229 0.224 0.225); names ending in ".filter" (the
 * package's pooling buffers) are ignored.  Missing, extra and mis-shaped tensors are refused by name, and so is
 * a sum(alpha) + sum(beta) that is zero or not finite.  A handle serves one call at a time. */
typedef struct mlic_dists mlic_dists;
int mlic_dists_create(int n, const char* const* names, const float* const* ptrs, const int64_t* shapes,
                      const int* ndims, void* stream, mlic_dists** out);
int mlic_dists_destroy(mlic_dists* h);
/* the dense convs' kernel family: 2 = split-fp16 conv_x4 (default), 0 = the fp32 MFMA conv */
int mlic_dists_set_precision(mlic_dists* h, int precision);
/* bytes of device scratch mlic_image_dists_u8 needs; host logic only, no GPU touched; nonzero rc with a message
 * when B < 1, H or W < 16, or H * W > 2^23.  Chunked under the same 4 GiB cap as LPIPS. */
int mlic_dists_scratch_bytes(int B, int H, int W, size_t* bytes);
/* per-pair DISTS; element strides {image, channel, row} per operand (column stride 1); out: B doubles (device);
 * terms: optional B*12 doubles (device) [T1_0, T2_0, .., T1_5, T2_5], the structure and texture terms of the six
 * sets, whose sum in that order is the value.  Checked before any GPU call, each with its own message: null
 * handle; B < 1; H or W < 16; null images or strides; a row stride below W or a negative stride; scratch too
 * small or not 256-byte aligned; null out.  Nothing outside scratch[0, bytes), out and terms is written, and no
 * scratch element is read that this call did not write.  Identical operands give exactly 0 (value and terms).
 * Bit-reproducible, and independent of B, of the chunking and of the strides.  The fp16 range guard and its
 * whole-call fp32 re-run are those of mlic_image_lpips_u8. */
int mlic_image_dists_u8(mlic_dists* h, void* stream, const float* a, const int64_t* a_strides, const float* b,
                        const int64_t* b_strides, int B, int H, int W, void* scratch, size_t scratch_bytes,
                        double* out, double* terms);
/* stage timing (tools/dists_bench.py), as mlic_lpips_profile: {the stem, the dense convs, the set-0, tap, stats
 * and reduce launches} */
int mlic_dists_profile(mlic_dists* h, int on, double* ms3);
/* calls that were re-run in fp32 by the range guard since the last reset */
int mlic_dists_range_fallbacks(mlic_dists* h, int64_t* count, int reset);

/* ---- uint8 images in, file bytes out, uint8 images back (utils/testing.py:338-424, submit/decode.py) ----
 *
 * ingest: B images of H x W x 3 bytes (device), read in place through element strides {image, row, column,
 * channel} (interleaved HWC = {H*W*3, W*3, 3, 1}, planar CHW = {3*H*W, W, 1, H*W}; a crop view, a row-padded
 * buffer or RGBA = {.., .., 4, 1} work as well; no alignment is assumed) -> dst: contiguous fp32
 * [B][3][Hp][Wp], Hp >= H and Wp >= W multiples of 64.  Every element of dst is written: v / 255 (true IEEE
 * division, torch's CPU `u8.float().div(255)` bit for bit) inside the image, +0.0 in the right / bottom padding.
 * Asynchronous on `stream`; arguments are checked before any GPU call. */
int mlic_image_ingest_u8(void* stream, const uint8_t* src, const int64_t* src_strides, int B, int H, int W, float* dst,
                         int Hp, int Wp);
/* egress: the H x W crop of fp32 src (element strides {image, channel, row}, column stride 1: a padded x_hat
 * is cropped in place, the convention of mlic_image_ms_ssim_u8) -> uint8 floor(clamp(v, 0, 1) * 255) (the
 * expression of mlic_image_sq_err_u8; NaN -> 0) written through dst_strides {image, row, column, channel}.
 * Only the crop's bytes are written.  ref (optional, device, its own {image, row, column, channel} strides,
 * the same H x W) together with sq_err (B uint64, device): sq_err[b] = the exact sum over image b of the squared
 * uint8 differences, accumulated in integers (deterministic), so PSNR = 10 log10(255^2 * 3 H W / sq_err) comes
 * with the decode.  ref and sq_err are both given or both NULL.  Asynchronous on `stream`; arguments are checked
 * before any GPU call. */
int mlic_image_egress_u8(void* stream, const float* src, const int64_t* src_strides, int B, int H, int W, uint8_t* dst,
                         const int64_t* dst_strides, const uint8_t* ref, const int64_t* ref_strides, uint64_t* sq_err);
/* The rate loop's prefilter (utils/testing.py:363-390: crop, 3x3 depthwise conv with padding 1, pad to 64 again)
 * in one launch, with the gather that compacts the images still over budget.  src: contiguous fp32
 * [Bsrc][3][Hp][Wp] as mlic_image_ingest_u8 writes it; dst: contiguous fp32 [n][3][Hp][Wp]; src_index: n image
 * indices into src on the device (each in [0, Bsrc): the kernel cannot check them; duplicates allowed), NULL =
 * the identity.  Output image i is the filter of input image src_index[i]: inside the H x W image
 * dst = sum_t w[t] * v[t] over the 3x3 neighbourhood with v = 0 outside the H x W image (not outside the padded
 * buffer), +0.0 in the right / bottom padding; every element of dst is written.  fp32, taps row-major (dy = -1..1,
 * then dx = -1..1), acc = 0; acc = acc + w[t] * v[t] with every product and sum rounded once (no FMA): what a
 * torch CPU loop `acc = acc + w[t] * view_t` computes, bit for bit.  w9: 9 host floats, NULL = the reference's
 * sigma 0.5 Gaussian (corner 0x1.73b62cp-7, edge 0x1.575320p-4, centre 0x1.3d1b0ep-1).
 * Refused before any GPU call, each with its own message: n < 1; H < 1 or W < 1; Hp / Wp not multiples of 64
 * that cover H / W; NULL src or dst; dst overlapping src (the stencil cannot run in place).  Bsrc is not known
 * here, so the overlap test covers the n images starting at src and at dst; with src_index the caller keeps dst
 * disjoint from every image it names.  Asynchronous on `stream`. */
int mlic_image_blur3_pad(void* stream, const float* src, const int32_t* src_index, int n, int H, int W, int Hp, int Wp,
                         const float* w9, float* dst);

/* The bitstream file of one image (utils/utils.py:28-83), big-endian:
 *     H, W [, level]  |  h_z, w_z, n_strings = 2  |  y length, y bytes  |  z length, z bytes
 * The format has no magic number: whether the level word is there is the caller's knowledge (a *_VBR model).
 * Host only, no GPU touched. */
typedef struct mlic_container_info {
  uint32_t H, W;       /* the unpadded image */
  uint32_t hz, wz;     /* ceil(H / 64), ceil(W / 64): the shape mlic_decompress takes */
  int32_t level;       /* -1 when the file has no level word */
  int32_t reserved;
  uint64_t y_off, y_len; /* the y string is data[y_off, y_off + y_len) */
  uint64_t z_off, z_len;
} mlic_container_info;
int mlic_container_bytes(size_t y_len, size_t z_len, int vbr, size_t* bytes);
/* level < 0: no level word.  *len = the file's size; out == NULL only queries it. */
int mlic_container_write(uint32_t H, uint32_t W, int level, uint32_t hz, uint32_t wz, const uint8_t* y, size_t y_len,
                         const uint8_t* z, size_t z_len, uint8_t* out, size_t cap, size_t* len);
/* Validating parser: never reads outside data[0, n) and makes no copies (info holds offsets into data).
 * Refused, each with its own message: input truncated anywhere; n_strings != 2; a length running past the
 * end; bytes left over after the z string; H == 0 or W == 0; h_z != ceil(H / 64) or w_z != ceil(W / 64);
 * (64 h_z) * (64 w_z) > max_pixels; with vbr, level >= n_levels. */
int mlic_container_parse(const uint8_t* data, size_t n, int vbr, int n_levels, uint64_t max_pixels,
                         mlic_container_info* info);

/* The ROI file: the file of mlic_container_write with the level word always present (ROI files are VBR files;
 * it holds the map's upper level) and n_strings = 3.  The third string is the level map on the z grid: one
 * version byte 0, then h_z * w_z levels of 4 bits each, row-major, high nibble first; 1 + ceil(h_z * w_z / 2)
 * bytes, after a length word of 4: 260 B more per file at 1920 x 1080 (17 x 30 cells), 53 B at 768 x 512.
 * write: levels = h_z * w_z host bytes, one per cell, each <= 15; the *len / out / cap protocol of
 * mlic_container_write.
 * parse: accepts 2 strings (map_len = 0: a plain VBR file) or 3; levels (optional, levels_cap >= h_z * w_z
 * bytes) receives the unpacked map.  Refused, each with its own message: everything mlic_container_parse
 * refuses; n_levels > 16; n_strings not 2 or 3; a map length that is not 1 + ceil(h_z * w_z / 2); a nonzero
 * version byte; a level >= n_levels; a nonzero padding nibble.  Never reads outside data[0, n).
 * mlic_container_parse itself keeps refusing n_strings = 3. */
typedef struct mlic_container_roi_info {
  mlic_container_info file;
  uint64_t map_off, map_len; /* the packed map is data[map_off, map_off + map_len); map_len 0 = no map */
} mlic_container_roi_info;
int mlic_container_write_roi(uint32_t H, uint32_t W, int level, uint32_t hz, uint32_t wz, const uint8_t* y,
                             size_t y_len, const uint8_t* z, size_t z_len, const uint8_t* levels, uint8_t* out,
                             size_t cap, size_t* len);
int mlic_container_parse_roi(const uint8_t* data, size_t n, int n_levels, uint64_t max_pixels,
                             mlic_container_roi_info* info, uint8_t* levels, size_t levels_cap);

/* Tiled coding (DESIGN.md section 5 "Tiled coding"): a large image is coded as independent tiles, each a plain
 * per-image file, held by a tiled file with an index; a decoder touches only the tiles a region needs.
 * The grid, per axis of length L, tile T (a multiple of 64, 128 <= T <= 65472), overlap V (0, 16, 32 or 64,
 * V <= T / 2), S = T - V: n = 1 if L <= T else ceil((L - V) / S); tile k starts at k S, extent min(T, L - k S).
 * Tiles are numbered row-major.  In the V-wide strip shared by tiles k and k + 1, at position j, the later tile
 * weighs (2 j + 1) / (2 V) and the earlier one 1 minus that; the 2-D weight is the product of the axis weights.
 * mlic_tile_grid: *ny, *nx; rects (optional, rects_cap >= ny * nx entries of 4) receives {y0, x0, h, w} per tile. */
int mlic_tile_grid(uint32_t H, uint32_t W, uint32_t T, uint32_t V, uint32_t* ny, uint32_t* nx, uint32_t* rects,
                   size_t rects_cap);
/* The blend egress, one launch: the h x w region at (y0, x0) of the H x W image as uint8 through dst_strides
 * {row, column, channel} (dst = the region's first byte; only the region's bytes are written).  tiles_dev: device
 * table of ny * nx pointers, tile index -> that tile's contiguous fp32 [3][pad64(h_t)][pad64(w_t)] x_hat planes
 * (device) or NULL; tiles_host: the same table in host memory, from which a region whose covering tile is NULL
 * is refused before any GPU call.  Per pixel and channel: acc (double) = sum over the covering tiles, tile row
 * then tile column, of (double)(wy * wx) * (double)x_hat (each product exact, the sums rounded in that order);
 * u = floor(clamp((float)acc, 0, 1) * 255), NaN -> 0.  Where one tile covers a pixel this is
 * mlic_image_egress_u8 of that tile.  ref (optional: the region's crop of the original, device, its own {row,
 * column, channel} strides) with sq_err (one device uint64): the exact sum of squared uint8 differences.
 * Asynchronous on `stream`. */
int mlic_image_tile_blend_u8(void* stream, const float* const* tiles_dev, const float* const* tiles_host, int H, int W,
                             int T, int V, int y0, int x0, int h, int w, uint8_t* dst, const int64_t* dst_strides,
                             const uint8_t* ref, const int64_t* ref_strides, uint64_t* sq_err);
/* The tiled file, big-endian:
 *     "MLT1" | u8 version 0 | u8 flags (bit 0: the tiles carry a VBR level word) | u32 H, W | u16 T, V
 *     u32 ny, nx | (ny nx + 1) x u64 offsets into the payload | payload: the tiles' files, row-major
 * Each tile's file is exactly the file mlic_container_write makes for that tile's crop.  write: payload = the
 * n_tiles files concatenated, lens = their lengths; the *len / out / cap protocol of mlic_container_write.
 * parse: validating, never reads outside data[0, n), no copies.  Refused, each with its own message: a truncated
 * header; bad magic, version or flags; T or V outside the rules; H or W zero; H * W > max_pixels (the whole
 * image's bound); ny or nx off the grid formula; an offset table that cannot fit in n (checked before it is
 * walked); a first offset that is not 0, offsets not strictly increasing, a last offset that is not the payload's
 * length.  mlic_container_tiled_tile: tile k's file is data[*off, *off + *len); it then goes through
 * mlic_container_parse, and its H, W must be the tile's extent.  mlic_container_parse keeps refusing a tiled
 * file (the magic read as H is about 1.3e9).  There is no single-call encode or decode of a tiled file here:
 * the tiles go through mlic_compress / mlic_decompress as batches (mlic_amd/codec.py does). */
typedef struct mlic_container_tiled_info {
  uint32_t H, W, T, V, ny, nx;
  int32_t vbr; /* flags bit 0 */
  int32_t reserved;
  uint64_t table_off, payload_off, payload_len;
} mlic_container_tiled_info;
int mlic_container_write_tiled(uint32_t H, uint32_t W, uint32_t T, uint32_t V, int vbr, const uint8_t* payload,
                               const uint64_t* lens, size_t n_tiles, uint8_t* out, size_t cap, size_t* len);
int mlic_container_parse_tiled(const uint8_t* data, size_t n, uint64_t max_pixels, mlic_container_tiled_info* info);
int mlic_container_tiled_tile(const uint8_t* data, size_t n, const mlic_container_tiled_info* info, uint64_t k,
                              uint64_t* off, uint64_t* len);

/* One image, pixels to file bytes: ingest into a staging buffer the handle owns (it grows on demand and is
 * freed by mlic_destroy), mlic_compress with B = 1, the container.  rgb_dev: H x W x 3 bytes on the device
 * with strides {row, column, channel}; level >= 0 is written into the header (vbr_scale is that level's gain),
 * -1 writes none.  *len = the file's size.  out == NULL: the image is encoded and only the size reported;
 * rgb_dev == NULL: nothing is encoded, the file of the handle's last encode is written again (so: one call
 * with out == NULL, allocate, one call with rgb_dev == NULL).  Returns with the file complete.
 * These two B = 1 conveniences run on one lane: they do not overlap one image's entropy coding with another's
 * kernels as a batched mlic_compress / mlic_decompress does.  Batch users compose mlic_image_ingest_u8,
 * mlic_compress, mlic_container_write themselves (mlic_amd/codec.py does). */
int mlic_encode_image_u8(mlic_model* m, void* stream, const uint8_t* rgb_dev, const int64_t* strides, int H, int W,
                         float vbr_scale, int level, uint8_t* out, size_t cap, size_t* len);
/* mlic_encode_image_u8 under a rate budget (utils/testing.py:363-390): encode; while the whole file, header
 * included, is above max_bpp bits per pixel of the H x W image and fewer than max_passes filter passes were
 * made, filter the float image with mlic_image_blur3_pad (default weights) and encode again.  The float image
 * is filtered again on the next pass, never re-quantised; it ping-pongs between the staging buffer and a second
 * one the handle owns likewise.  *passes = filter passes made (0: the first file fit); the file may still be
 * above the budget when *passes == max_passes.  max_bpp must be positive and finite, max_passes >= 0.  The
 * out == NULL / rgb_dev == NULL protocol is that of mlic_encode_image_u8 (*passes is reported on both calls).
 * The level of a *_VBR model is the caller's choice (mlic_amd/codec.py picks it from the budget). */
int mlic_encode_image_u8_budget(mlic_model* m, void* stream, const uint8_t* rgb_dev, const int64_t* strides, int H,
                                int W, float vbr_scale, int level, double max_bpp, int max_passes, uint8_t* out,
                                size_t cap, size_t* len, int* passes);
/* File bytes to pixels: mlic_container_parse (n_levels > 0 says the file has a level word; max_pixels bounds
 * the padded size before anything is allocated), mlic_decompress into the staging buffer, egress of the crop to
 * rgb_dev through strides {row, column, channel} (non-negative).  cap_bytes = bytes addressable from rgb_dev:
 * a file whose H x W needs more is refused before any GPU call.  vbr_gains: n_levels floats, the gain of each
 * level (NULL = 1).  H, W, level (-1 = none) are reported; rgb_dev == NULL only parses and reports them (m may
 * be NULL then).  Asynchronous on `stream` once the entropy decoding is done. */
int mlic_decode_image_u8(mlic_model* m, void* stream, const uint8_t* file, size_t n, int n_levels, uint64_t max_pixels,
                         const float* vbr_gains, uint8_t* rgb_dev, const int64_t* strides, size_t cap_bytes, int* H,
                         int* W, int* level);

/* ---- Scaled coding: code at reduced resolution, decode at a chosen size (DESIGN.md section 5 "Scaled coding") ----
 *
 * One separable, antialiased polyphase resampler (the rule of PIL's resize and of torch's
 * interpolate(antialias=True)), fused into the ingest and egress kernels.  filter: 0 lanczos3, 1 bicubic (Keys
 * a = -0.5), 2 triangle.  Per axis, input length Li, output length Lo, 1/8 <= Lo / Li <= 8, both <= 2^24:
 * s = Li / Lo, fs = max(s, 1), support = radius * fs; output o has centre c = (o + 0.5) s, first tap
 * x0 = max(0, int(c - support + 0.5)), n = min(Li, int(c + support + 0.5)) - x0 taps and weights
 * k((j + x0 - c + 0.5) / fs) / sum, computed in double and rounded once to fp32.  Lo == Li is the identity table.
 * No table has more than 49 taps.
 * mlic_resample_table: *taps = the largest n.  start, count (Lo entries) and weights (Lo rows of `stride` floats,
 * zero from column n) are filled when all three are given and stride >= *taps; all three NULL is the size query.
 * Host only. */
int mlic_resample_table(int filter, int Li, int Lo, int32_t* start, int32_t* count, float* weights, int stride,
                        int* taps);
/* mlic_image_ingest_u8 with the resampler: Hi x Wi x 3 bytes (strides {image, row, column, channel}) -> v / 255,
 * resampled to h x w (horizontal pass first, nothing rounded in between; per pass acc = +0, acc = acc + w * v over
 * the taps in ascending order, product and sum rounded once each), clamped to [0, 1], written as fp32
 * [B][3][Hp][Wp] with +0 in the padding; every element of dst is written.  One launch.  The first call with a new
 * (filter, Li, Lo) builds that table on the device (a blocking copy); it is kept for later calls. */
int mlic_image_ingest_u8_scaled(void* stream, const uint8_t* src, const int64_t* src_strides, int B, int Hi, int Wi,
                                int filter, int h, int w, float* dst, int Hp, int Wp);
/* mlic_image_egress_u8 with the resampler: the h x w crop of src (strides {image, channel, row}), clamped to
 * [0, 1] (NaN -> 0), resampled to Ho x Wo by the same arithmetic, floor(clamp(v, 0, 1) * 255), written through
 * dst_strides; only the image's bytes are written.  ref / sq_err as in mlic_image_egress_u8, ref being Ho x Wo.
 * With Ho x Wo == h x w the bytes are those of mlic_image_egress_u8. */
int mlic_image_egress_u8_scaled(void* stream, const float* src, const int64_t* src_strides, int B, int h, int w,
                                int filter, int Ho, int Wo, uint8_t* dst, const int64_t* dst_strides, const uint8_t* ref,
                                const int64_t* ref_strides, uint64_t* sq_err);
/* The scaled file, big-endian:
 *     "MLS1" | u8 version 0 | u8 flags (bit 0: the inner file has a VBR level word) | u8 filter | u8 reserved 0
 *     u32 H, W (display size) | the inner file, to the end
 * The inner file is exactly the file mlic_container_write makes for the coded image.  write: the *len / out / cap
 * protocol of mlic_container_write; the inner file is copied, not parsed.  parse: validating, never reads outside
 * data[0, n).  Refused, each with its own message: a truncated header; bad magic, version, flags, filter or
 * reserved byte; H or W zero; H * W > max_pixels; whatever mlic_container_parse refuses in the inner file (the
 * flags say whether it has a level word; n_levels bounds it); a coded size whose ratio to the display size leaves
 * [1/8, 8] on either axis.  info->inner's offsets are relative to the inner file, data + inner_off.
 * mlic_container_parse keeps refusing a scaled file (the magic read as H is about 1.3e9). */
typedef struct mlic_container_scaled_info {
  uint32_t H, W; /* display size */
  int32_t filter;
  int32_t vbr; /* flags bit 0 */
  uint64_t inner_off, inner_len;
  mlic_container_info inner;
} mlic_container_scaled_info;
int mlic_container_write_scaled(uint32_t H, uint32_t W, int vbr, int filter, const uint8_t* inner, size_t inner_len,
                                uint8_t* out, size_t cap, size_t* len);
int mlic_container_parse_scaled(const uint8_t* data, size_t n, int n_levels, uint64_t max_pixels,
                                mlic_container_scaled_info* info);
/* The layered file (progressive coding), big-endian:
 *     "MLL1" | u8 version 0 | u8 flags (bit 0: a VBR level word follows the size) | u8 S | u8 reserved 0
 *     u32 H, W | (flag bit 0) u32 level | u32 h_z, w_z | u32 z_len, z bytes | S x ( u32 len, bytes )
 * Layer k is mlic_layer_streams' string k.  bytes / write: level < 0 = no level word; the *len / out / cap protocol
 * of mlic_container_write.  parse: validating, never reads outside data[0, n).  Refused, each with its own message:
 * bad magic, version, flags or reserved byte; S == 0 or S > 32; what mlic_container_parse refuses about sizes,
 * grids and levels; a cut inside the header or inside z; a length running past the end; bytes left over after the
 * last layer.  allow_truncated != 0: a file cut at any byte after the complete z string is accepted,
 * layers_present counts the whole layer strings, and a partial trailing length word or string is ignored; without
 * it layers_present < S is refused.  That S is the model's is the caller's check.
 * mlic_container_parse keeps refusing a layered file (the magic read as H is about 1.3e9). */
typedef struct mlic_container_layered_info {
  uint32_t H, W, hz, wz;
  int32_t level; /* -1: none */
  uint32_t S, layers_present;
  uint64_t z_off, z_len;
  uint64_t layer_off[32], layer_len[32]; /* [0, layers_present) */
} mlic_container_layered_info;
int mlic_container_layered_bytes(size_t z_len, const size_t* layer_lens, int S, int vbr, size_t* bytes);
int mlic_container_write_layered(uint32_t H, uint32_t W, int level, uint32_t hz, uint32_t wz, const uint8_t* z,
                                 size_t z_len, const uint8_t* const* layers, const size_t* layer_lens, int S,
                                 uint8_t* out, size_t cap, size_t* len);
int mlic_container_parse_layered(const uint8_t* data, size_t n, int n_levels, uint64_t max_pixels, int allow_truncated,
                                 mlic_container_layered_info* info);
/* ---- Residual coding: near-lossless and lossless files (DESIGN.md section 5 "Residual coding") ----
 *
 * Integer definitions (csrc/residual.h).  Samples are 8-bit RGB in the canonical order i = (c H + y) W + x.  base is
 * the byte image the inner file decodes to, tau in 0..127, step = 2 tau + 1:
 *     r = x - base;  q = sign(r) floor((|r| + tau) / step);  rec = clamp(base + q step, 0, 255)
 * so |x - rec| <= tau, rec = x at tau = 0, |q| <= 255.  Context = 8 c + class; a = max - min of channel c of base
 * over the 3 x 3 neighbourhood (coordinates clamped into the image); class 0 for a < 2, else floor(log2 a).
 * Histogram bin q + 63 for |q| <= 63, bin 127 (the escape) otherwise.  Digest of base: the sum over i of
 * (base_i + 1) ((i + 1) 0x9E3779B97F4A7C15) mod 2^64.
 *
 * mlic_image_residual_front_u8: base, and optionally x, through element strides {image, row, column, channel}.
 * Always written: ctx u8 [B][3][H][W] (dense, canonical order), ctx_count u32 [B][24], digest u64 [B].  With x also
 * sym int16 [B][3][H][W], hist u32 [B][24][128] and max_err u32 [B], the largest |x - rec| of each image.  The call
 * zeroes ctx_count, digest, hist and max_err itself, on the stream.  One launch, asynchronous on `stream`.
 * Refused before any HIP call, each with its own message: null base; null base strides; B < 1; H or W < 1; tau
 * outside 0..127; a zero column or channel stride of base; null ctx; null ctx_count; null digest; ctx_count not
 * 4-byte or digest not 8-byte aligned; x without strides; a zero column or channel stride of x; x without all of
 * sym, hist and max_err; sym not 2-byte or hist / max_err not 4-byte aligned; sym, hist or max_err without x; a
 * batch too large for one launch. */
int mlic_image_residual_front_u8(void* stream, const uint8_t* base, const int64_t* base_strides, const uint8_t* x,
                                 const int64_t* x_strides, int B, int H, int W, int tau, uint8_t* ctx,
                                 uint32_t* ctx_count, uint64_t* digest, int16_t* sym, uint32_t* hist, uint32_t* max_err);
/* mlic_image_residual_apply_u8: out = rec of (base, sym), written through out_strides; only the image's bytes are
 * written.  With ref (its own strides): sq_err u64 [B], the exact sum of squared differences out - ref, and max_err
 * u32 [B], the largest |out - ref|; the call zeroes both on the stream.  One launch, asynchronous on `stream`.
 * Refused before any HIP call, each with its own message: null base; null base strides; null sym; null out or out
 * strides; B < 1; H or W < 1; tau outside 0..127; a zero column or channel stride of base, of out; sym not 2-byte
 * aligned; ref without sq_err; ref without max_err; sq_err or max_err without ref; ref without strides or with a
 * zero column or channel stride; sq_err not 8-byte or max_err not 4-byte aligned; a batch too large. */
int mlic_image_residual_apply_u8(void* stream, const uint8_t* base, const int64_t* base_strides, const int16_t* sym,
                                 int B, int H, int W, int tau, uint8_t* out, const int64_t* out_strides,
                                 const uint8_t* ref, const int64_t* ref_strides, uint64_t* sq_err, uint32_t* max_err);
/* One image's tables from its histograms hist[24][128].  Per context with a nonzero count: m = the largest |q| <= 63
 * seen (0 if none); the symbols -m..m and, last, the escape go through mlic_pmf_to_quantized_cdf at precision 16 on
 * (float)count / (float)total, which keeps every frequency >= 1.  m[24]: 0..63, or 0xFF for a context with count 0.
 * freq (optional) [24][128]: the 2 m + 2 frequencies of each table, zero behind them.  cdf [24][129], cdf_len [24]
 * (2 m + 3; 0 = absent) and offset [24] (-m) (optional, all three or none) are mlic_rans_encode's tables with
 * stride 129; the escape of that coder carries |q| > m.  Host only. */
int mlic_residual_tables(const uint32_t* hist, uint8_t* m, uint16_t* freq, int32_t* cdf, int32_t* cdf_len,
                         int32_t* offset);
/* The residual file, big-endian:
 *     "MLR1" | u8 version 0 | u8 flags (bit 0: the inner file has a VBR level word) | u8 tau | u8 n_ctx = 24
 *     u32 H, W | u64 digest
 *     24 x ( u8 m (0..63, or 0xFF = absent) | unless absent: (2 m + 2) x u16 frequencies, each >= 1, sum 65536 )
 *     u32 inner_len, inner file (exactly mlic_container_write's file for the image) | u32 res_len, residual bytes
 * write: the *len / out / cap protocol of mlic_container_write; m is 24 bytes and freq mlic_residual_tables' rows.
 * parse: validating, never reads outside data[0, n).  Refused, each with its own message: a truncated header, table
 * or string; bad magic, version, flags or n_ctx; tau > 127; H or W zero; H * W > max_pixels; an m in 64..254; a
 * zero frequency; a wrong sum; inner_len or res_len past the end; an empty inner file; trailing bytes; whatever
 * mlic_container_parse refuses in the inner file; an inner H x W different from the outer.  info->inner's offsets
 * are relative to the inner file.  mlic_container_parse and the ROI, tiled, scaled and layered parsers keep
 * refusing a residual file. */
typedef struct mlic_container_residual_info {
  uint32_t H, W;
  int32_t tau;
  int32_t vbr; /* flags bit 0 */
  uint64_t digest;
  uint8_t m[24];
  uint64_t freq_off[24]; /* table k's frequencies: data + freq_off[k], 2 m[k] + 2 big-endian u16 */
  uint64_t inner_off, inner_len, res_off, res_len;
  mlic_container_info inner;
} mlic_container_residual_info;
int mlic_container_write_residual(uint32_t H, uint32_t W, int vbr, int tau, uint64_t digest, const uint8_t* m,
                                  const uint16_t* freq, const uint8_t* inner, size_t inner_len, const uint8_t* res,
                                  size_t res_len, uint8_t* out, size_t cap, size_t* len);
int mlic_container_parse_residual(const uint8_t* data, size_t n, int n_levels, uint64_t max_pixels,
                                  mlic_container_residual_info* info);
/* ---- Segmented residual strings: the residual layer's device entropy coder ("Segments") ----
 *
 * The N = 3 H W samples of an image, in the canonical order, are cut into n_seg = ceil(N / seg_len) segments of
 * seg_len samples (256..65536; the last may be shorter).  A segment's bytes are exactly mlic_rans_encode of its
 * symbols and contexts under the image's tables, so segments code and decode independently, and a decoder that has
 * decoded a whole segment has consumed exactly its words and holds the state 2^31 again: both decoders check that.
 * A segment of n samples is at most 4 (n + 4) bytes (csrc/residual_seg.h derives n + 2 words).
 * Common arguments: sym int16 [B][N] and ctx u8 [B][N], dense; m u8 [B][24] and freq u16 [B][24][128], host memory,
 * the file's form of the tables (mlic_residual_tables); seg_bytes u32 [B][n_seg]; image b's bytes start at
 * out + b cap (data + b data_stride); len / data_len u64 [B], host memory.
 * Every entry refuses, before it does anything else (the device entries: before any HIP call), each with its own
 * message: null pointers; B < 1; H or W < 1; more than 2^29 samples; seg_len outside 256..65536; n_seg that is not
 * ceil(N / seg_len); an m in 64..254, a zero frequency or a wrong sum.  encode also: a cap that is not a multiple of
 * 4 or is below 8 n_seg.  decode also: a segment length that is not a multiple of 4, is below 8 or is above the
 * bound; lengths that do not sum to data_len[b]; data_len[b] above data_stride; a data_stride that is not a
 * multiple of 4.
 *
 * Device entries (sym, ctx, out / data and seg_bytes of encode in device memory; scratch: device memory of
 * mlic_residual_segments_scratch_bytes, 16-byte aligned).  They upload the tables, run on `stream`, wait for it and
 * return an error that names the image, the first bad segment and the reason when a kernel refused something.
 * encode: a counting pass, a scan of the lengths and a writing pass, no host round trip between them; an image
 * whose bytes exceed cap is refused ("the bytes do not fit the capacity") with nothing written past cap.
 * decode: seg_bytes is host memory (the file's lengths); the offsets are summed on the host and uploaded.  The
 * kernel never reads outside a segment's bytes and refuses a bypass length above 3, a symbol index above max_value,
 * a q outside +-255, a final state that is not 2^31 and a word count that is not the segment's.
 * status (optional, host, u32 [B]): 0xFFFFFFFF for a clean image, else (segment << 4) | reason. */
int mlic_residual_segments_scratch_bytes(int B, int64_t n_seg, size_t* bytes);
int mlic_residual_encode_segments(void* stream, const int16_t* sym, const uint8_t* ctx, int B, int H, int W,
                                  const uint8_t* m, const uint16_t* freq, int seg_len, int64_t n_seg, uint8_t* out,
                                  size_t cap, uint32_t* seg_bytes, uint64_t* len, void* scratch, size_t scratch_bytes,
                                  uint32_t* status);
int mlic_residual_decode_segments(void* stream, const uint8_t* data, size_t data_stride, const uint64_t* data_len,
                                  const uint32_t* seg_bytes, const uint8_t* ctx, int B, int H, int W, const uint8_t* m,
                                  const uint16_t* freq, int seg_len, int64_t n_seg, int16_t* sym, void* scratch,
                                  size_t scratch_bytes, uint32_t* status);
/* The same contract on host memory: a loop over segments on the host rANS coder; oracle, CPU path and fallback.
 * encode: out == NULL asks for len and seg_bytes only; an image whose bytes exceed cap is an error. */
int mlic_residual_encode_segments_host(const int16_t* sym, const uint8_t* ctx, int B, int H, int W, const uint8_t* m,
                                       const uint16_t* freq, int seg_len, int64_t n_seg, uint8_t* out, size_t cap,
                                       uint32_t* seg_bytes, uint64_t* len);
int mlic_residual_decode_segments_host(const uint8_t* data, size_t data_stride, const uint64_t* data_len,
                                       const uint32_t* seg_bytes, const uint8_t* ctx, int B, int H, int W,
                                       const uint8_t* m, const uint16_t* freq, int seg_len, int64_t n_seg,
                                       int16_t* sym);
/* The same five for a string of N samples that is not an RGB image's 3 H W (a Y'CbCr frame's N = H W + 2 hc wc:
 * mlic_residual_yuv_samples): int64_t N stands in place of int H, int W; scratch_bytes_n takes N and seg_len and
 * works out n_seg.  Refused, each with its own message: N < 1; N above 2^29; n_seg that is not ceil(N / seg_len);
 * everything else as the entries above.  At N = 3 H W they give the entries' above results byte for byte. */
int mlic_residual_segments_scratch_bytes_n(int B, int64_t N, int seg_len, size_t* bytes);
int mlic_residual_encode_segments_n(void* stream, const int16_t* sym, const uint8_t* ctx, int B, int64_t N,
                                    const uint8_t* m, const uint16_t* freq, int seg_len, int64_t n_seg, uint8_t* out,
                                    size_t cap, uint32_t* seg_bytes, uint64_t* len, void* scratch,
                                    size_t scratch_bytes, uint32_t* status);
int mlic_residual_decode_segments_n(void* stream, const uint8_t* data, size_t data_stride, const uint64_t* data_len,
                                    const uint32_t* seg_bytes, const uint8_t* ctx, int B, int64_t N, const uint8_t* m,
                                    const uint16_t* freq, int seg_len, int64_t n_seg, int16_t* sym, void* scratch,
                                    size_t scratch_bytes, uint32_t* status);
int mlic_residual_encode_segments_host_n(const int16_t* sym, const uint8_t* ctx, int B, int64_t N, const uint8_t* m,
                                         const uint16_t* freq, int seg_len, int64_t n_seg, uint8_t* out, size_t cap,
                                         uint32_t* seg_bytes, uint64_t* len);
int mlic_residual_decode_segments_host_n(const uint8_t* data, size_t data_stride, const uint64_t* data_len,
                                         const uint32_t* seg_bytes, const uint8_t* ctx, int B, int64_t N,
                                         const uint8_t* m, const uint16_t* freq, int seg_len, int64_t n_seg,
                                         int16_t* sym);
/* The segmented residual file, big-endian:
 *     "MLR2" | u8 version 0 | u8 flags (bit 0: VBR level word inside) | u8 tau | u8 n_ctx = 24 | u32 H, W | u64 digest
 *     the 24 tables, exactly as in "MLR1"
 *     u32 seg_len | u32 n_seg | u32 inner_len, inner file
 *     u32 res_len = 4 n_seg + the sum of the lengths | n_seg x u32 segment byte lengths | the segments
 * write: the *len / out / cap protocol of mlic_container_write; seg_bytes: n_seg host lengths, segs their bytes.
 * parse: validating, never reads outside data[0, n).  Refused, each with its own message: everything
 * mlic_container_parse_residual refuses; seg_len outside 256..65536; n_seg that is not ceil(3 H W / seg_len); a
 * segment length that is not a multiple of 4, is below 8 or is above the capacity bound of its samples; res_len
 * that is not 4 n_seg + the sum of the lengths; truncation anywhere; trailing bytes.  Every other parser refuses an
 * "MLR2" file, and this one refuses every other file. */
typedef struct mlic_container_residual_seg_info {
  uint32_t H, W;
  int32_t tau;
  int32_t vbr;
  uint64_t digest;
  uint8_t m[24];
  uint64_t freq_off[24];
  uint32_t seg_len, n_seg;
  uint64_t inner_off, inner_len, res_off, res_len;
  uint64_t index_off;          /* n_seg big-endian u32 lengths */
  uint64_t data_off, data_len; /* the concatenated segments */
  mlic_container_info inner;
} mlic_container_residual_seg_info;
int mlic_container_write_residual_seg(uint32_t H, uint32_t W, int vbr, int tau, uint64_t digest, const uint8_t* m,
                                      const uint16_t* freq, uint32_t seg_len, uint32_t n_seg, const uint32_t* seg_bytes,
                                      const uint8_t* inner, size_t inner_len, const uint8_t* segs, size_t segs_len,
                                      uint8_t* out, size_t cap, size_t* len);
int mlic_container_parse_residual_seg(const uint8_t* data, size_t n, int n_levels, uint64_t max_pixels,
                                      mlic_container_residual_seg_info* info);
/* ---- Residual coding of 9..16-bit samples (DESIGN.md section 5 "Residual coding", "Deep samples") ----
 *
 * Integer definitions (csrc/residual16.h).  Samples are d-bit RGB, d in 9..16, LSB-aligned in uint16 words, in the
 * canonical order; maxv = 2^d - 1 and a word above maxv reads as maxv.  base is the inner file decoded alone at depth
 * d (mlic_image_egress_u16, msb = 0), tau in 0..127, step = 2 tau + 1:
 *     r = x - base;  q = sign(r) floor((|r| + tau) / step);  rec = clamp(base + q step, 0, maxv)
 * so |x - rec| <= tau, rec = x at tau = 0, |q| <= maxv.  Split by the shift s in 0..d-7: hi = q >> s (arithmetic),
 * lo = q - (hi << s) in 0..2^s-1, q = (hi << s) + lo.  hi is the symbol of the 8-bit layer: its histogram bins, the
 * tables (mlic_residual_tables) and both segment coders (mlic_residual_encode_segments / _decode_segments) are reused
 * unchanged, which needs |hi| <= 255, i.e. (max|q| + 2^s - 1) >> s <= 255; s = d - 7 always fits.  Context = 8 c +
 * class(a >> (d - 8)), a = max - min of channel c of base over the clamped 3 x 3 neighbourhood.  Digest: the 8-bit
 * formula on the words of base.
 * Low-bit plane: row r = c H + y, group g = x / 64, G = ceil(W / 64); 64-bit word (r G + g) s + j holds bit j of
 * lo(r, x) at bit x mod 64, bits beyond column W zero; 3 H G s words an image, none at s = 0.
 *
 * mlic_image_residual_front_u16: base, and optionally x, through element strides {image, row, column, channel}.
 * Always written: ctx u8 [B][3][H][W], ctx_count u32 [B][24], digest u64 [B].  With x also sym int16 [B][3][H][W] (hi,
 * saturated to int16: a shift that does not fit shows in max_abs_q), lo_plane u64 [B][3 H G shift] (NULL exactly when
 * shift is 0), hist u32 [B][24][128] of hi, max_err u32 [B] (the largest |x - rec|), max_abs_q u32 [B] and sum_abs_q
 * u64 [B].  Without x, shift is ignored.  The call zeroes what it accumulates into, on the stream.  One launch.
 * mlic_image_residual_stats_u16: max_abs_q and sum_abs_q alone, by a statistics launch of the same kernel: the shift
 * is chosen from them (mlic_residual_shift), so they are needed before the front pass.
 * mlic_image_residual_apply_u16: out = rec of (base, (sym << shift) + lo), written through out_strides; with ref also
 * sq_err u64 [B] and max_err u32 [B].  status u32 [B] (required): nonzero for an image that holds a sym outside
 * +-255; such a sample is written as base and the caller must refuse the image.
 * Refused before any HIP call, each with its own message: what the 8-bit entries refuse; a depth outside 9..16; a
 * shift outside 0..depth - 7; a lo_plane that does not go with the shift; pointers that are not aligned to their
 * element (words 2 bytes, lo_plane and sum_abs_q 8); a null status. */
int mlic_image_residual_front_u16(void* stream, const uint16_t* base, const int64_t* base_strides, const uint16_t* x,
                                  const int64_t* x_strides, int B, int H, int W, int depth, int tau, int shift,
                                  uint8_t* ctx, uint32_t* ctx_count, uint64_t* digest, int16_t* sym, uint64_t* lo_plane,
                                  uint32_t* hist, uint32_t* max_err, uint32_t* max_abs_q, uint64_t* sum_abs_q);
int mlic_image_residual_stats_u16(void* stream, const uint16_t* base, const int64_t* base_strides, const uint16_t* x,
                                  const int64_t* x_strides, int B, int H, int W, int depth, int tau,
                                  uint32_t* max_abs_q, uint64_t* sum_abs_q);
int mlic_image_residual_apply_u16(void* stream, const uint16_t* base, const int64_t* base_strides, const int16_t* sym,
                                  const uint64_t* lo_plane, int B, int H, int W, int depth, int tau, int shift,
                                  uint16_t* out, const int64_t* out_strides, const uint16_t* ref,
                                  const int64_t* ref_strides, uint64_t* sq_err, uint32_t* max_err, uint32_t* status);
/* The shift rule, host only: the smallest s in 0..depth-7 with (max_abs_q + 2^s - 1) >> s <= 255 and sum_abs_q <=
 * 8 N 2^s (N = 3 H W), or depth - 7 if there is none.  The shift travels in the file; a decoder never evaluates this. */
int mlic_residual_shift(int depth, uint64_t N, uint32_t max_abs_q, uint64_t sum_abs_q, int* shift);
/* The deep residual file, big-endian (the plane's 64-bit words little-endian):
 *     "MLR3" | the "MLR2" header and tables | u8 depth (9..16) | u8 shift (0..depth - 7)
 *     u32 seg_len | u32 n_seg | u32 inner_len, inner file | u32 res_len | the index | the segments
 *     u32 lo_len = 8 * 3 H ceil(W / 64) shift | the low-bit plane
 * Always segmented.  parse refuses, each with its own message: everything mlic_container_parse_residual_seg refuses; a
 * depth or shift out of range; a wrong lo_len; truncation inside the plane; trailing bytes.  Every other parser
 * refuses an "MLR3" file. */
typedef struct mlic_container_residual_deep_info {
  uint32_t H, W;
  int32_t tau;
  int32_t vbr;
  uint64_t digest;
  uint8_t m[24];
  uint64_t freq_off[24];
  uint32_t seg_len, n_seg;
  uint64_t inner_off, inner_len, res_off, res_len;
  uint64_t index_off;
  uint64_t data_off, data_len;
  int32_t depth, shift;
  uint64_t lo_off, lo_len; /* the low-bit plane */
  mlic_container_info inner;
} mlic_container_residual_deep_info;
int mlic_container_write_residual_deep(uint32_t H, uint32_t W, int vbr, int tau, int depth, int shift, uint64_t digest,
                                       const uint8_t* m, const uint16_t* freq, uint32_t seg_len, uint32_t n_seg,
                                       const uint32_t* seg_bytes, const uint8_t* inner, size_t inner_len,
                                       const uint8_t* segs, size_t segs_len, const uint8_t* lo, size_t lo_len,
                                       uint8_t* out, size_t cap, size_t* len);
int mlic_container_parse_residual_deep(const uint8_t* data, size_t n, int n_levels, uint64_t max_pixels,
                                       mlic_container_residual_deep_info* info);
/* mlic_encode_image_u8 at reduced (or raised) resolution: the H x W image is resampled to coded_H x coded_W on
 * the way in, coded as mlic_encode_image_u8 codes an image of that size, and wrapped in the scaled file with H, W
 * as the display size.  The out == NULL / rgb_dev == NULL protocol is that of mlic_encode_image_u8. */
int mlic_encode_image_u8_scaled(mlic_model* m, void* stream, const uint8_t* rgb_dev, const int64_t* strides, int H,
                                int W, int coded_H, int coded_W, int filter, float vbr_scale, int level, uint8_t* out,
                                size_t cap, size_t* len);
/* mlic_decode_image_u8 at a chosen output size, for a plain, VBR or scaled file (told apart by the magic).
 * out_H x out_W: the size of the image written to rgb_dev; 0 x 0 = the file's display size (a plain file's own
 * H x W).  filter: the resampler from the coded to the output size; -1 = the file's filter (lanczos3 for a plain
 * file).  *H, *W report the output size, *coded_H, *coded_W the size the model decodes; rgb_dev == NULL only
 * parses, checks and reports.  Everything else as mlic_decode_image_u8. */
int mlic_decode_image_u8_sized(mlic_model* m, void* stream, const uint8_t* file, size_t n, int n_levels,
                               uint64_t max_pixels, const float* vbr_gains, int out_H, int out_W, int filter,
                               uint8_t* rgb_dev, const int64_t* strides, size_t cap_bytes, int* H, int* W, int* level,
                               int* coded_H, int* coded_W);

/* ---- 8-bit Y'CbCr frames in and out (DESIGN.md section 5 "YCbCr I/O") ----
 *
 * A frame is three byte planes on the device, each a pointer plus element strides {image, row, column}: Y is
 * H x W, Cb and Cr are ceil(H / sub_y) x ceil(W / sub_x) (odd H and W are legal).  The planes are independent, so
 * one description covers I420 / YV12 (swap the chroma pointers), I422, I444, NV12 (cb = uv, cr = uv + 1, column
 * stride 2) / NV21, row-padded pitches and crops of larger frames.  Matrix, range and siting are the caller's
 * knowledge, as the VBR level word's presence is: they are not written into the file.  Alpha and 4:4:0 are out of scope
 * and refused where reachable; bit depths above 8 and BT.2020 go through the *_yuv16 calls below, and these
 * 8-bit calls keep refusing matrix 2. */
typedef struct mlic_yuv_desc {
  int32_t sub_x, sub_y;  /* 1 or 2.  4:4:4 = {1,1}, 4:2:2 = {2,1}, 4:2:0 = {2,2}; {1,2} is refused */
  int32_t matrix;        /* 0 = BT.601 (Kr .299, Kb .114), 1 = BT.709 (Kr .2126, Kb .0722) */
  int32_t full_range;    /* 1: Y, C in 0..255 (JPEG);  0: Y = 16 + 219 Y', C = 128 + 224 C' */
  int32_t site_x;        /* horizontal chroma siting when sub_x == 2: 0 = centre (JPEG / MPEG-1),
                            1 = left, co-sited with the even luma column (MPEG-2, H.264 / HEVC default).
                            Vertical siting is always centre.  Ignored when sub_x == 1 */
  int32_t reserved[3];   /* must be 0 */
} mlic_yuv_desc;
/* ingest, one launch: dst = contiguous fp32 [B][3][Hp][Wp] (Hp >= H, Wp >= W multiples of 64), every element
 * written, +0.0 in the right / bottom padding; nothing outside the planes' extents is read.  Per luma pixel (x, y)
 * chroma is upsampled in integers, as sixteenths c16 in [0, 4080].  Across columns (sub_x == 2, i = x >> 1,
 * indices clamped to the plane): centre siting 3 C[i] + C[i -+ 1] (- for even x, + for odd x); left siting 4 C[i]
 * at even x, 2 C[i] + 2 C[i + 1] at odd x.  Down rows (sub_y == 2) the centre rule, 3 : 1.  An unsubsampled axis
 * contributes the factor 4.  u = c16 / 16 - 128 (exact in fp32), v likewise from Cr, then in fp32 with every
 * product and sum rounded once (no FMA):
 *     a = cy (Y - yo);  R = a + crv v;  G = (a - cgu u) - cgv v;  B = a + cbu u;  out = min(max(., 0), 1)
 *     yo = 0 | 16, ys = 255 | 219, cs = 255 | 224 (full | limited), Kg = 1 - Kr - Kb,
 *     cy = 1 / ys, crv = 2 (1 - Kr) / cs, cbu = 2 (1 - Kb) / cs, cgu = 2 Kb (1 - Kb) / (Kg cs), cgv = 2 Kr (1 - Kr) / (Kg cs),
 * each constant computed in double and rounded to fp32 once.  There is no intermediate 8-bit RGB.
 * Refused before any GPU call, each with its own message: a null plane, dst, strides or desc; B, H or W < 1;
 * Hp / Wp not multiples of 64 that cover H / W; sub_x / sub_y outside {1, 2} or {1, 2} together; matrix,
 * full_range or site_x out of range; nonzero reserved; a zero column stride; dst not 4-byte aligned.
 * Asynchronous on `stream`. */
int mlic_image_ingest_yuv8(void* stream, const uint8_t* y, const int64_t* y_strides, const uint8_t* cb,
                           const int64_t* cb_strides, const uint8_t* cr, const int64_t* cr_strides,
                           const mlic_yuv_desc* desc, int B, int H, int W, float* dst, int Hp, int Wp);
/* egress, one launch: the H x W crop of fp32 src (element strides {image, channel, row}, column stride 1: a padded
 * x_hat is read in place) -> the three byte planes.  Per pixel r, g, b = min(max(v, 0), 1) (a NaN becomes 0);
 *     t_Y  = (yo + ((ys Kr) r + (ys Kg) g)) + (ys Kb) b
 *     t_Cb = ((-cs Kr / (2 (1 - Kb))) r + (-cs Kg / (2 (1 - Kb))) g) + (cs / 2) b
 *     t_Cr = ((cs / 2) r + (-cs Kg / (2 (1 - Kr))) g) + (-cs Kb / (2 (1 - Kr))) b
 * with the constants folded in double and rounded once and every operation rounded once.  Chroma is filtered at
 * luma resolution before rounding: centre siting the mean of the sub_x x sub_y block; left siting [1 2 1] / 4
 * across columns 2 i - 1, 2 i, 2 i + 1 and the mean down the sub_y rows; indices clamped into the image; the sum
 * runs row-major from the first term (sums rounded; the products by 1, 2 and the final power of two are exact);
 * then 128 is added.  Bytes: floor(min(max(t + 0.5, 0), 255)).  Only the planes' bytes inside their extents are
 * written.  ref_y / ref_cb / ref_cr (device, their own strides) with sq_err ([B][3] uint64, device): sq_err[b][p] =
 * the exact sum over plane p of image b of the squared byte differences (integer atomics: deterministic); all four
 * given or all NULL.  Refusals as for the ingest, plus: ref_* / sq_err not all-or-none; src not 4-byte or sq_err
 * not 8-byte aligned.  Asynchronous on `stream`. */
int mlic_image_egress_yuv8(void* stream, const float* src, const int64_t* src_strides, int B, int H, int W,
                           const mlic_yuv_desc* desc, uint8_t* y, const int64_t* y_strides, uint8_t* cb,
                           const int64_t* cb_strides, uint8_t* cr, const int64_t* cr_strides, const uint8_t* ref_y,
                           const int64_t* ref_y_strides, const uint8_t* ref_cb, const int64_t* ref_cb_strides,
                           const uint8_t* ref_cr, const int64_t* ref_cr_strides, uint64_t* sq_err);
/* mlic_encode_image_u8 / mlic_decode_image_u8 with the Y'CbCr ingest / egress (the same staging buffer and the
 * same out == NULL / source == NULL two-call protocol; the file is a plain per-image file).  Planes: device
 * pointers with strides {row, column}.  encode: y_dev == NULL writes the handle's last file again.  decode:
 * y_dev == NULL only parses and reports H, W, level (m and desc may be NULL then); *_cap = bytes addressable from
 * each plane pointer, and a file whose planes need more is refused before any GPU call.  There is no budget
 * variant. */
int mlic_encode_image_yuv8(mlic_model* m, void* stream, const uint8_t* y_dev, const int64_t* y_strides,
                           const uint8_t* cb_dev, const int64_t* cb_strides, const uint8_t* cr_dev,
                           const int64_t* cr_strides, const mlic_yuv_desc* desc, int H, int W, float vbr_scale,
                           int level, uint8_t* out, size_t cap, size_t* len);
int mlic_decode_image_yuv8(mlic_model* m, void* stream, const uint8_t* file, size_t n, int n_levels,
                           uint64_t max_pixels, const float* vbr_gains, const mlic_yuv_desc* desc, uint8_t* y_dev,
                           const int64_t* y_strides, size_t y_cap, uint8_t* cb_dev, const int64_t* cb_strides,
                           size_t cb_cap, uint8_t* cr_dev, const int64_t* cr_strides, size_t cr_cap, int* H, int* W,
                           int* level);

/* ---- 9..16-bit samples in and out (DESIGN.md section 5 "High-bit-depth I/O") ----
 *
 * The four image calls above for samples deeper than a byte.  The model takes fp32 in [0, 1] and returns fp32, the
 * bitstream and the file do not change and do not know the depth: these are front doors only.
 * Sample format, shared by every call below: samples are uint16_t words in native byte order; depth d in [8, 16],
 * maxv = 2^d - 1, half = 2^(d-1), s = 2^(d-8).  msb = 0: LSB-aligned (y4m p10, I010, PPM), the sample is
 * min(word, maxv).  msb = 1: MSB-aligned (P010 / P016), the sample is word >> (16 - d), the low bits of an input
 * word are ignored; an output word is sample << (16 - d), its low bits zero.  Strides are in ELEMENTS (uint16), in
 * the orders of the 8-bit calls: RGB images {image, row, column, channel}, planes {image, row, column}.  Sample
 * pointers must be 2-byte aligned.  Refused before any GPU call, each with its own message: everything the 8-bit
 * counterpart refuses; depth outside [8, 16]; msb not 0 or 1; a misaligned sample pointer; (Y'CbCr) matrix outside
 * {0, 1, 2}.  Fast forms (rows through LDS) exist for unit column stride, interleaved HWC, and interleaved chroma
 * with column stride 2 (P010); any other stride set takes the general form; the kernel option image_io_path forces
 * one as for the 8-bit kernels; all forms give the same bits.
 *
 * mlic_image_ingest_u16: dst fp32 [B][3][Hp][Wp]; inside the image v = (float)sample / (float)maxv, a true IEEE
 * division (torch's CPU t.to(float32).div(maxv) bit for bit); +0.0 in the padding; every element written.
 * mlic_image_egress_u16: sample = floor(min(max(v, 0), 1) * maxv), NaN -> 0: mlic_image_egress_u8's expression with
 * 255 replaced by maxv (equal to it at d = 8; egress(ingest(v)) == v for every sample value at every depth).
 * Only the crop's words are written.  ref + sq_err ([B] uint64): the exact per-image sum of squared sample
 * differences, the reference read by the same msb rule, accumulated in 64 bits throughout.
 * There is no one-image encode / decode call for 16-bit RGB: compose mlic_image_ingest_u16, mlic_compress and
 * mlic_container_write (mlic_amd/codec.py does). */
int mlic_image_ingest_u16(void* stream, const uint16_t* src, const int64_t* src_strides, int depth, int msb, int B,
                          int H, int W, float* dst, int Hp, int Wp);
int mlic_image_egress_u16(void* stream, const float* src, const int64_t* src_strides, int B, int H, int W, int depth,
                          int msb, uint16_t* dst, const int64_t* dst_strides, const uint16_t* ref,
                          const int64_t* ref_strides, uint64_t* sq_err);
/* mlic_image_ingest_yuv8's rules verbatim at depth d: integer chroma upsampling to sixteenths c16 in [0, 16 maxv]
 * (below 2^20: exact in fp32) with the same siting rules, u = c16 / 16 - half (exact), then
 *     a = cy (Y - yo);  R = a + crv v;  G = (a - cgu u) - cgv v;  B = a + cbu u;  out = min(max(., 0), 1)
 *     yo = 0 | 16 s, ys = maxv | 219 s, cs = maxv | 224 s (full | limited)
 * with cy, crv, cbu, cgu, cgv as for mlic_image_ingest_yuv8 from this ys, cs.  desc->matrix may also be 2 = BT.2020
 * non-constant-luminance (Kr .2627, Kb .0593); the 8-bit calls keep refusing it.  mlic_yuv_desc is unchanged and its
 * reserved words must be 0: depth and alignment are arguments.  At d = 8 the bits are those of the 8-bit calls. */
int mlic_image_ingest_yuv16(void* stream, const uint16_t* y, const int64_t* y_strides, const uint16_t* cb,
                            const int64_t* cb_strides, const uint16_t* cr, const int64_t* cr_strides,
                            const mlic_yuv_desc* desc, int depth, int msb, int B, int H, int W, float* dst, int Hp,
                            int Wp);
/* mlic_image_egress_yuv8's rules at depth d: the same t_Y / t_Cb / t_Cr expressions with the constants folded from
 * ys, cs, yo of depth d, the same chroma filter, siting, clamping and summation order, half added in place of 128;
 * word = floor(min(max(t + 0.5, 0), maxv)) (shifted up for msb = 1).  Optional three reference planes with sq_err
 * ([B][3] uint64): exact, accumulated in 64 bits. */
int mlic_image_egress_yuv16(void* stream, const float* src, const int64_t* src_strides, int B, int H, int W,
                            const mlic_yuv_desc* desc, int depth, int msb, uint16_t* y, const int64_t* y_strides,
                            uint16_t* cb, const int64_t* cb_strides, uint16_t* cr, const int64_t* cr_strides,
                            const uint16_t* ref_y, const int64_t* ref_y_strides, const uint16_t* ref_cb,
                            const int64_t* ref_cb_strides, const uint16_t* ref_cr, const int64_t* ref_cr_strides,
                            uint64_t* sq_err);
/* mlic_encode_image_yuv8 / mlic_decode_image_yuv8 for uint16 planes (a hardware decoder's P010 surface: cb = uv,
 * cr = uv + 1, column stride 2, depth 10, msb 1): the same staging buffer, the same two-call protocol, a plain
 * per-image file.  Strides {row, column} in elements; *_cap stay in BYTES addressable from each plane pointer.
 * Every argument (depth, msb, plane alignment, the whole descriptor, strides, capacities) is checked before the
 * handle is looked at: a refused call makes no device call and leaves the handle's last encoded image as it was.
 * There is no budget variant. */
int mlic_encode_image_yuv16(mlic_model* m, void* stream, const uint16_t* y_dev, const int64_t* y_strides,
                            const uint16_t* cb_dev, const int64_t* cb_strides, const uint16_t* cr_dev,
                            const int64_t* cr_strides, const mlic_yuv_desc* desc, int depth, int msb, int H, int W,
                            float vbr_scale, int level, uint8_t* out, size_t cap, size_t* len);
int mlic_decode_image_yuv16(mlic_model* m, void* stream, const uint8_t* file, size_t n, int n_levels,
                            uint64_t max_pixels, const float* vbr_gains, const mlic_yuv_desc* desc, int depth, int msb,
                            uint16_t* y_dev, const int64_t* y_strides, size_t y_cap, uint16_t* cb_dev,
                            const int64_t* cb_strides, size_t cb_cap, uint16_t* cr_dev, const int64_t* cr_strides,
                            size_t cr_cap, int* H, int* W, int* level);
/* ---- Residual coding of Y'CbCr frames (DESIGN.md section 5 "Residual coding", "Y'CbCr frames") ----
 *
 * Integer definitions (csrc/residual_yuv.h).  A frame is three planes, p = 0 Y' of H x W, p = 1 Cb and p = 2 Cr of
 * hc x wc = ceil(H / sub_y) x ceil(W / sub_x); samples of depth d in 8..16, maxv = 2^d - 1: bytes at d = 8, uint16
 * words above, LSB-aligned (sample = min(word, maxv)) or MSB-aligned (sample = word >> (16 - d); written words carry
 * zero low bits).  Canonical order: i = off_p + y w_p + x, off = {0, H W, H W + hc wc}, N = H W + 2 hc wc <= 2^29.
 * base is the three planes mlic_image_egress_yuv8 / _yuv16 writes from the inner file decoded alone; q, rec, hi, lo
 * and the shift rule are those of the deep layer with maxv (rec clamps to [0, maxv], not to the legal range), the
 * shift is 0 at depth 8 and in 0..d-7 above.  Context = 8 p + class(a >> (d - 8)), a = max - min of base plane p over
 * the 3 x 3 neighbourhood clamped into that plane; bins, escape, tables and digest (over the canonical index) are the
 * 8-bit layer's.  Low-bit plane: rows in canonical order, G_p = ceil(w_p / 64); the 64-bit word
 * (rowbase_p + y G_p + g) s + j holds bit j of lo at bit x mod 64, zero beyond the plane's width;
 * s (H G_0 + 2 hc G_1) words a frame.
 *
 * Planes come as three pointers with element strides {image, row, column} (column stride 2: the semi-planar forms).
 * Of desc only sub_x / sub_y are used; the rest is validated as the egress validates it.
 * front: always ctx u8 [B][N], ctx_count u32 [B][24], digest u64 [B]; with the three x planes (all NULL without x)
 * also sym int16 [B][N] (hi, saturated), lo_plane u64, hist u32 [B][24][128], max_err, max_abs_q u32 [B] and
 * sum_abs_q u64 [B].  stats: max_abs_q and sum_abs_q alone.  apply: the three out planes through their own strides;
 * with the three ref planes also sq_err u64 [B][3] (per plane) and max_err u32 [B]; status u32 [B] (required) is
 * nonzero for a frame that holds a sym outside +-255, and such a sample is written as base.  One launch each, over
 * the three planes of all B frames; they zero what they accumulate into on the stream.
 * Refused before any HIP call, each with its own message: a null base plane or strides; B < 1; H or W < 1 or above
 * 2^24; more than 2^29 samples; what the egress refuses of desc; tau outside 0..127; a zero column stride; x, out
 * or ref given as fewer than three planes; null outputs that the call needs, outputs that go with x (ref) without
 * it; pointers not aligned to their element.  _yuv8: uint8 planes, depth 8, the shift must be 0 and lo_plane NULL.
 * _yuv16: uint16 planes, 2-byte aligned, depth 9..16, msb 0 / 1, shift 0..depth - 7, lo_plane NULL exactly when the
 * shift is 0. */
int mlic_image_residual_front_yuv8(void* stream, const uint8_t* base_y, const int64_t* base_y_strides,
                                   const uint8_t* base_cb, const int64_t* base_cb_strides, const uint8_t* base_cr,
                                   const int64_t* base_cr_strides, const uint8_t* x_y, const int64_t* x_y_strides,
                                   const uint8_t* x_cb, const int64_t* x_cb_strides, const uint8_t* x_cr,
                                   const int64_t* x_cr_strides, const mlic_yuv_desc* desc, int B, int H, int W, int tau,
                                   int shift, uint8_t* ctx, uint32_t* ctx_count, uint64_t* digest, int16_t* sym,
                                   uint64_t* lo_plane, uint32_t* hist, uint32_t* max_err, uint32_t* max_abs_q,
                                   uint64_t* sum_abs_q);
int mlic_image_residual_stats_yuv8(void* stream, const uint8_t* base_y, const int64_t* base_y_strides,
                                   const uint8_t* base_cb, const int64_t* base_cb_strides, const uint8_t* base_cr,
                                   const int64_t* base_cr_strides, const uint8_t* x_y, const int64_t* x_y_strides,
                                   const uint8_t* x_cb, const int64_t* x_cb_strides, const uint8_t* x_cr,
                                   const int64_t* x_cr_strides, const mlic_yuv_desc* desc, int B, int H, int W, int tau,
                                   uint32_t* max_abs_q, uint64_t* sum_abs_q);
int mlic_image_residual_apply_yuv8(void* stream, const uint8_t* base_y, const int64_t* base_y_strides,
                                   const uint8_t* base_cb, const int64_t* base_cb_strides, const uint8_t* base_cr,
                                   const int64_t* base_cr_strides, const int16_t* sym, const uint64_t* lo_plane,
                                   const mlic_yuv_desc* desc, int B, int H, int W, int tau, int shift, uint8_t* out_y,
                                   const int64_t* out_y_strides, uint8_t* out_cb, const int64_t* out_cb_strides,
                                   uint8_t* out_cr, const int64_t* out_cr_strides, const uint8_t* ref_y,
                                   const int64_t* ref_y_strides, const uint8_t* ref_cb, const int64_t* ref_cb_strides,
                                   const uint8_t* ref_cr, const int64_t* ref_cr_strides, uint64_t* sq_err,
                                   uint32_t* max_err, uint32_t* status);
int mlic_image_residual_front_yuv16(void* stream, const uint16_t* base_y, const int64_t* base_y_strides,
                                    const uint16_t* base_cb, const int64_t* base_cb_strides, const uint16_t* base_cr,
                                    const int64_t* base_cr_strides, const uint16_t* x_y, const int64_t* x_y_strides,
                                    const uint16_t* x_cb, const int64_t* x_cb_strides, const uint16_t* x_cr,
                                    const int64_t* x_cr_strides, const mlic_yuv_desc* desc, int depth, int msb, int B,
                                    int H, int W, int tau, int shift, uint8_t* ctx, uint32_t* ctx_count,
                                    uint64_t* digest, int16_t* sym, uint64_t* lo_plane, uint32_t* hist,
                                    uint32_t* max_err, uint32_t* max_abs_q, uint64_t* sum_abs_q);
int mlic_image_residual_stats_yuv16(void* stream, const uint16_t* base_y, const int64_t* base_y_strides,
                                    const uint16_t* base_cb, const int64_t* base_cb_strides, const uint16_t* base_cr,
                                    const int64_t* base_cr_strides, const uint16_t* x_y, const int64_t* x_y_strides,
                                    const uint16_t* x_cb, const int64_t* x_cb_strides, const uint16_t* x_cr,
                                    const int64_t* x_cr_strides, const mlic_yuv_desc* desc, int depth, int msb, int B,
                                    int H, int W, int tau, uint32_t* max_abs_q, uint64_t* sum_abs_q);
int mlic_image_residual_apply_yuv16(void* stream, const uint16_t* base_y, const int64_t* base_y_strides,
                                    const uint16_t* base_cb, const int64_t* base_cb_strides, const uint16_t* base_cr,
                                    const int64_t* base_cr_strides, const int16_t* sym, const uint64_t* lo_plane,
                                    const mlic_yuv_desc* desc, int depth, int msb, int B, int H, int W, int tau,
                                    int shift, uint16_t* out_y, const int64_t* out_y_strides, uint16_t* out_cb,
                                    const int64_t* out_cb_strides, uint16_t* out_cr, const int64_t* out_cr_strides,
                                    const uint16_t* ref_y, const int64_t* ref_y_strides, const uint16_t* ref_cb,
                                    const int64_t* ref_cb_strides, const uint16_t* ref_cr,
                                    const int64_t* ref_cr_strides, uint64_t* sq_err, uint32_t* max_err,
                                    uint32_t* status);
/* Host only.  *N = H W + 2 hc wc; *words = shift (H G_0 + 2 hc G_1), the 64-bit words of one frame's low-bit plane.
 * Refused: a null result; H or W < 1 or above 2^24; a sub pair that is not {1,1}, {2,1} or {2,2}; more than 2^29
 * samples; a shift outside 0..9.  The shift rule is mlic_residual_shift with the frame's N (depth 9..16; at depth 8
 * the shift is 0). */
int mlic_residual_yuv_samples(int H, int W, int sub_x, int sub_y, uint64_t* N);
int mlic_residual_yuv_plane_words(int H, int W, int sub_x, int sub_y, int shift, uint64_t* words);
/* The Y'CbCr residual file, big-endian (the plane's 64-bit words little-endian); H, W are the luma size:
 *     "MLR4" | the "MLR2" header and tables
 *     u8 depth (8..16) | u8 shift | u8 sub_x | u8 sub_y | u8 matrix | u8 flags (bit 0 full_range, bit 1 site_x left)
 *     u32 seg_len | u32 n_seg | u32 inner_len, inner file | u32 res_len | the index | the segments
 *     u32 lo_len = 8 shift (H G_0 + 2 hc G_1) | the low-bit plane
 * Always segmented; the inner file is byte for byte what the Y'CbCr encode writes without a residual.  parse refuses,
 * each with its own message: everything mlic_container_parse_residual_seg refuses, with n_seg against ceil(N /
 * seg_len) for this frame's N; a depth outside 8..16; a shift outside 0..depth - 7, a nonzero shift at depth 8; a sub
 * pair that is not {1,1}, {2,1} or {2,2}; a matrix outside 0..2, matrix 2 (BT.2020) at depth 8; reserved flag bits; a
 * wrong lo_len; truncation anywhere; trailing bytes.  Every other parser refuses an "MLR4" file.  There is no
 * single-call encode or decode of this file. */
typedef struct mlic_container_residual_yuv_info {
  uint32_t H, W;
  int32_t tau;
  int32_t vbr;
  uint64_t digest;
  uint8_t m[24];
  uint64_t freq_off[24];
  uint32_t seg_len, n_seg;
  uint64_t inner_off, inner_len, res_off, res_len;
  uint64_t index_off;
  uint64_t data_off, data_len;
  int32_t depth, shift;
  uint64_t lo_off, lo_len; /* the low-bit plane */
  int32_t sub_x, sub_y, matrix, full_range, site_x; /* site_x: 1 = left */
  mlic_container_info inner;
} mlic_container_residual_yuv_info;
int mlic_container_write_residual_yuv(uint32_t H, uint32_t W, int vbr, int tau, int depth, int shift, int sub_x,
                                      int sub_y, int matrix, int full_range, int site_x, uint64_t digest,
                                      const uint8_t* m, const uint16_t* freq, uint32_t seg_len, uint32_t n_seg,
                                      const uint32_t* seg_bytes, const uint8_t* inner, size_t inner_len,
                                      const uint8_t* segs, size_t segs_len, const uint8_t* lo, size_t lo_len,
                                      uint8_t* out, size_t cap, size_t* len);
int mlic_container_parse_residual_yuv(const uint8_t* data, size_t n, int n_levels, uint64_t max_pixels,
                                      mlic_container_residual_yuv_info* info);
/* per-image sum of -log2(lik) over n_per elements (fixed reduction order); synchronous */
int mlic_neglog2_sum(void* stream, const float* lik, int B, int64_t n_per, double* out);
/* GaussianConditional likelihood (compressai, eval; mlicpp.py:132,168) element-wise: lik = max(Phi((0.5-|v|)/s')
 * - Phi((-0.5-|v|)/s'), 1e-9), v = round(y - m), s' = max(s, 0.11); vbr_scale != 1 evaluates it at (y, s, m) *
 * vbr_scale (mlicpp_vbr.py:292).  The kernel's device function is the one the slice loop runs. */
int mlic_gaussian_likelihood(void* stream, const float* y, const float* scales, const float* means, int64_t n,
                             float vbr_scale, float* lik);
/* build_indexes (utils/ckbd.py:128-129): idx = (ntable-1) - #{t in table[:-1] : max(s, 0.11) <= t} */
int mlic_scale_indexes(void* stream, const float* scales, int64_t n, const float* table, int ntable, int32_t* out);

/* host entropy coder (compressai-compatible) */
int mlic_pmf_to_quantized_cdf(const float* pmf, int n, int precision, int32_t* cdf_out /* n + 1 */);
int mlic_rans_encode(const int32_t* symbols, const int32_t* indexes, int64_t n, const int32_t* cdf,
                     const int32_t* cdf_len, const int32_t* offset, int n_tables, int stride, uint8_t* out,
                     size_t cap, size_t* written);
int mlic_rans_decode(const uint8_t* data, size_t nbytes, const int32_t* indexes, int64_t n, const int32_t* cdf,
                     const int32_t* cdf_len, const int32_t* offset, int n_tables, int stride, int32_t* out);
/* The decompress path's narrow decode, on the host alone (tests): the stream is decoded in `nparts`
 * consecutive pieces of n / nparts symbols (the 20 phases of one image) with uint8 table indexes, each
 * piece first into int16 and, when a value falls outside the narrow range (int16, or
 * mlic_set_kernel_option("narrow_limit", L)), reset to the piece's start and decoded again into int32 --
 * exactly PhaseDecoder::run's per-image step.  out: all n symbols as int32; *widened: pieces that
 * took the int32 fallback. */
int mlic_rans_decode_narrow(const uint8_t* data, size_t nbytes, const uint8_t* indexes, int64_t n, int nparts,
                            const int32_t* cdf, const int32_t* cdf_len, const int32_t* offset, int n_tables,
                            int stride, int32_t* out, int* widened);

#ifdef __cplusplus
}
#endif
#endif
