// The per-image bitstream file (the layout documented at the top of mlic_amd/bitstream.py; utils/utils.py:28-83):
//     >II   H, W of the unpadded image            (VBR: >III H, W, level)
//     >III  h_z, w_z, n_strings (= 2)
//     2 x ( >I length, bytes )                    y stream, then z stream
// A writer that is byte-identical to bitstream.write_stream and a parser that validates every field before
// anything is sized from it.  Host only, plain C++17, no HIP: g++ alone compiles this file.
//
// The format has no magic number: whether a level word is present is the caller's knowledge (the model kind).
// Both functions return nullptr on success and a static message on refusal; they allocate nothing, copy
// nothing but the payload the writer is asked to write, and never read outside [data, data + n).
#ifndef MLIC_CONTAINER_H
#define MLIC_CONTAINER_H
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define MLIC_HOST_DEVICE __host__ __device__
#else
#define MLIC_HOST_DEVICE
#endif

namespace mlic {

struct ContainerInfo {
  uint32_t H, W;        // unpadded image
  uint32_t hz, wz;      // z grid: ceil(H / 64), ceil(W / 64)
  int32_t level;        // VBR level, -1 when the file has none
  size_t y_off, y_len;  // the y string: data[y_off, y_off + y_len)
  size_t z_off, z_len;
};

// header + two length words + the payloads (bitstream.file_bytes)
size_t container_bytes(size_t y_len, size_t z_len, bool vbr);

// level < 0: no level word.  *len = the file's size, also when out is null (a query) or cap is too small
// (refused).  y / z may be null when their length is 0.
const char* container_write(uint32_t H, uint32_t W, int32_t level, uint32_t hz, uint32_t wz, const uint8_t* y,
                            size_t y_len, const uint8_t* z, size_t z_len, uint8_t* out, size_t cap, size_t* len);

// Refused: input truncated anywhere, H == 0 or W == 0, (vbr) level >= n_levels, hz != ceil(H / 64) or
// wz != ceil(W / 64), (64 hz) (64 wz) > max_pixels, n_strings != 2, a length running past the end, bytes left
// over after the z string.  On success *info holds offsets and lengths into data (no copies).
const char* container_parse(const uint8_t* data, size_t n, bool vbr, uint32_t n_levels, uint64_t max_pixels,
                            ContainerInfo* info);

// The ROI file: the VBR file above with n_strings = 3.  The third string is the level map on the z grid:
//     one version byte 0, then h_z * w_z levels of 4 bits each, row-major, high nibble first
// (1 + ceil(h_z * w_z / 2) bytes; the low nibble of the last byte is 0 when the cell count is odd).  The level
// word is always present (ROI files are VBR files) and holds the map's upper level.
size_t container_roi_map_bytes(uint32_t hz, uint32_t wz);

// levels: h_z * w_z bytes, one level per cell, each <= 15.  The *len / out / cap protocol of container_write.
const char* container_write_roi(uint32_t H, uint32_t W, int32_t level, uint32_t hz, uint32_t wz, const uint8_t* y,
                                size_t y_len, const uint8_t* z, size_t z_len, const uint8_t* levels, uint8_t* out,
                                size_t cap, size_t* len);

// Accepts 2 strings (*map_len = 0: a plain VBR file) or 3.  Refused beyond what container_parse refuses:
// n_levels > 16, n_strings not 2 or 3, a map length that is not 1 + ceil(h_z * w_z / 2), a nonzero version byte,
// a level >= n_levels, a nonzero padding nibble.  The map is data[*map_off, *map_off + *map_len), still packed.
const char* container_parse_roi(const uint8_t* data, size_t n, uint32_t n_levels, uint64_t max_pixels,
                                ContainerInfo* info, size_t* map_off, size_t* map_len);

// the packed map (version byte included) of a parsed file -> one byte per cell
void container_roi_unpack(const uint8_t* map, uint64_t cells, uint8_t* levels);

// ---- Tiled coding (DESIGN.md section 5 "Tiled coding").  The grid, per axis of length L with tile T and overlap V,
// S = T - V: n = 1 if L <= T else ceil((L - V) / S); tile k starts at k * S and has extent min(T, L - k * S).
// T: a multiple of 64, 128 <= T <= 65472 (16 bits in the file); V in {0, 16, 32, 64}, V <= T / 2.
const char* tile_params_check(uint32_t T, uint32_t V);  // nullptr when T, V follow the rules
uint32_t tile_count(uint32_t L, uint32_t T, uint32_t V);
inline uint32_t tile_start(uint32_t k, uint32_t T, uint32_t V) { return k * (T - V); }
inline uint32_t tile_extent(uint32_t L, uint32_t k, uint32_t T, uint32_t V) {
  const uint32_t left = L - k * (T - V);
  return left < T ? left : T;
}
// Numerator of tile k's feather weight at its local position l, over den = max(2 V, 1): in the strip shared with
// tile k - 1 (l < V) the later tile's weight is (2 l + 1) / (2 V), in the strip shared with tile k + 1 (l >= S) it
// is 1 minus that tile's weight, elsewhere 1.  n: tiles on the axis.
MLIC_HOST_DEVICE inline uint32_t tile_weight_num(uint32_t l, uint32_t k, uint32_t n, uint32_t T, uint32_t V) {
  const uint32_t S = T - V, den = V ? 2 * V : 1;
  if (k > 0 && l < V) return 2 * l + 1;
  if (k + 1 < n && l >= S) return den - (2 * (l - S) + 1);
  return den;
}

// The tiled file.  All integers big-endian:
//     4 bytes "MLT1" | >B version 0 | >B flags (bit 0: the tiles carry a VBR level word) | >II H, W | >HH T, V
//     >II ny, nx (must equal the grid formula) | (ny nx + 1) x >Q offsets into the payload (offsets[0] = 0,
//     strictly increasing, the last = the payload's length) | payload: the tiles' files, row-major
constexpr size_t TILED_HEADER = 26;
struct TiledInfo {
  uint32_t H, W, T, V, ny, nx;
  bool vbr;
  size_t table_off, payload_off, payload_len;
};
// lens: n_tiles lengths (each > 0) of the tiles' files, concatenated row-major at payload.  The *len / out / cap
// protocol of container_write (payload may be null for a size query).
const char* container_write_tiled(uint32_t H, uint32_t W, uint32_t T, uint32_t V, bool vbr, const uint8_t* payload,
                                  const uint64_t* lens, size_t n_tiles, uint8_t* out, size_t cap, size_t* len);
// Refused, each with its own message: a truncated header, bad magic, version or flags, T or V outside the rules,
// H or W zero, H * W > max_pixels, ny or nx off the formula, an offset table that cannot fit in n (checked before
// it is walked), offsets[0] != 0, offsets not strictly increasing, a last offset that is not the payload's length.
const char* container_parse_tiled(const uint8_t* data, size_t n, uint64_t max_pixels, TiledInfo* info);
// tile k's file: data[*off, *off + *len), from a parsed file's table
const char* container_tiled_tile(const uint8_t* data, size_t n, const TiledInfo* info, uint64_t k, size_t* off,
                                 size_t* len);

// ---- Scaled coding (DESIGN.md section 5 "Scaled coding").  The scaled file, all integers big-endian:
//     4 bytes "MLS1" | >B version 0 | >B flags (bit 0: the inner file has a VBR level word)
//     >B filter (0 lanczos3, 1 bicubic, 2 triangle) | >B reserved 0 | >II H, W (display size) | the inner file
// The inner file is the plain or VBR file above of the coded size, unchanged, to the end.  As H, "MLS1" exceeds
// every max_pixels, so container_parse refuses a scaled file as it refuses a tiled one.
constexpr size_t SCALED_HEADER = 16;
struct ScaledInfo {
  uint32_t H, W;  // display size
  uint32_t filter;
  bool vbr;
  size_t inner_off, inner_len;  // the inner file: data[inner_off, inner_off + inner_len)
  ContainerInfo inner;          // its parse, offsets relative to the inner file
};
inline bool is_scaled_file(const uint8_t* data, size_t n) {
  return n >= 4 && data[0] == 'M' && data[1] == 'L' && data[2] == 'S' && data[3] == '1';
}
// nullptr when display / coded lie in [1/8, 8] (one axis)
const char* scaled_ratio_check(uint64_t display, uint64_t coded);
// inner: the coded image's file (container_write's), inner_len bytes.  The *len / out / cap protocol of
// container_write (inner may be null for a size query).  The inner file is not parsed here.
const char* container_write_scaled(uint32_t H, uint32_t W, bool vbr, uint32_t filter, const uint8_t* inner,
                                   size_t inner_len, uint8_t* out, size_t cap, size_t* len);
// Refused, each with its own message: a truncated header, bad magic, version, flags, filter or reserved byte, H or W
// zero, H * W > max_pixels, whatever container_parse (vbr from the flags, n_levels, max_pixels) refuses in the inner
// file, a coded size whose ratio to the display size leaves [1/8, 8] on either axis.
const char* container_parse_scaled(const uint8_t* data, size_t n, uint32_t n_levels, uint64_t max_pixels,
                                   ScaledInfo* info);

// ---- Progressive coding (DESIGN.md section 5 "Progressive coding").  The layered file, all integers big-endian:
//     4 bytes "MLL1" | >B version 0 | >B flags (bit 0: a VBR level word follows the size) | >B S | >B reserved 0
//     >II H, W | (flag bit 0) >I level | >II h_z, w_z | >I z_len, z bytes | S x ( >I len, bytes )
// Layer k is the rANS string of channel slice k alone (phases 2 k and 2 k + 1), so a file cut after any layer
// still decodes: z first, then the layers in the order the decoder needs them.  As H, "MLL1" exceeds every
// max_pixels, so container_parse refuses a layered file as it refuses a tiled or a scaled one.
constexpr uint32_t LAYERED_MAX_S = 32;
struct LayeredInfo {
  uint32_t H, W;    // unpadded image
  uint32_t hz, wz;  // z grid
  int32_t level;    // VBR level, -1 when the file has none
  uint32_t S;       // layers the whole file has
  uint32_t layers_present;  // whole layer strings in these n bytes (== S unless the file is truncated)
  size_t z_off, z_len;
  size_t layer_off[LAYERED_MAX_S], layer_len[LAYERED_MAX_S];  // [0, layers_present)
};
inline bool is_layered_file(const uint8_t* data, size_t n) {
  return n >= 4 && data[0] == 'M' && data[1] == 'L' && data[2] == 'L' && data[3] == '1';
}
// header + z + S length words + the layers; 0 when S is outside 1..32 or the sum does not fit size_t
size_t container_layered_bytes(size_t z_len, const size_t* layer_lens, uint32_t S, bool vbr);
// level < 0: no level word.  layers: S pointers (one may be null when its length is 0).  The *len / out / cap
// protocol of container_write (layers and z may be null for a size query).
const char* container_write_layered(uint32_t H, uint32_t W, int32_t level, uint32_t hz, uint32_t wz, const uint8_t* z,
                                    size_t z_len, const uint8_t* const* layers, const size_t* layer_lens, uint32_t S,
                                    uint8_t* out, size_t cap, size_t* len);
// Refused, each with its own message: bad magic, version, flags or reserved byte, S == 0 or S > 32, what
// container_parse refuses about sizes, grids and levels, a cut inside the header or inside z, a length running
// past the end, bytes left over after the last layer.  allow_truncated: a file cut at any byte after the
// complete z string is accepted; layers_present counts the whole layer strings and a partial trailing length
// word or string is ignored.  Without it layers_present < S is refused.
const char* container_parse_layered(const uint8_t* data, size_t n, uint32_t n_levels, uint64_t max_pixels,
                                    bool allow_truncated, LayeredInfo* info);

// ---- Residual coding (DESIGN.md section 5 "Residual coding"; residual.h has the definitions).  The residual file,
// all integers big-endian:
//     4 bytes "MLR1" | >B version 0 | >B flags (bit 0: the inner file has a VBR level word) | >B tau | >B n_ctx = 24
//     >II H, W | >Q digest of the base image
//     24 x ( >B m (0..63, or 0xFF = no table) | unless absent: (2 m + 2) x >H frequencies, each >= 1, sum 65536 )
//     >I inner_len, the inner file | >I res_len, the residual string
// The inner file is the plain or VBR file above, unchanged.  Table k codes the symbols -m..m and, last, the escape.
// As H, "MLR1" exceeds every max_pixels, so container_parse refuses a residual file as it refuses a scaled one.
constexpr size_t RESIDUAL_HEADER = 24;  // up to the tables
constexpr uint32_t RESIDUAL_CTX = 24;
constexpr uint32_t RESIDUAL_MAX_M = 63;
constexpr uint8_t RESIDUAL_ABSENT = 0xFF;
struct ResidualInfo {
  uint32_t H, W;
  uint32_t tau;
  bool vbr;
  uint64_t digest;
  uint8_t m[RESIDUAL_CTX];           // 0..63, or RESIDUAL_ABSENT
  size_t freq_off[RESIDUAL_CTX];     // table k's 2 m + 2 big-endian u16 frequencies start at data[freq_off[k]]
  size_t inner_off, inner_len;       // the inner file: data[inner_off, inner_off + inner_len)
  size_t res_off, res_len;           // the residual string
  ContainerInfo inner;               // the inner file's parse, offsets relative to the inner file
};
inline bool is_residual_file(const uint8_t* data, size_t n) {
  return n >= 4 && data[0] == 'M' && data[1] == 'L' && data[2] == 'R' && data[3] == '1';
}
// m: 24 bytes; freq: 24 rows of 128 frequencies, the first 2 m[k] + 2 of row k are written (65536 cannot occur:
// every frequency is >= 1 and there are at least two).  Refused: a null len, H or W zero, tau > 127, an m in
// 64..254, a zero frequency, a row that does not sum to 65536, an empty inner file, a string longer than a 32-bit
// length.  The *len / out / cap protocol of container_write (m, freq, inner and res may be null for a size query
// only when out is null; the size query still needs m).
const char* container_write_residual(uint32_t H, uint32_t W, bool vbr, uint32_t tau, uint64_t digest, const uint8_t* m,
                                     const uint16_t* freq, const uint8_t* inner, size_t inner_len, const uint8_t* res,
                                     size_t res_len, uint8_t* out, size_t cap, size_t* len);
// Refused, each with its own message: a truncated header, table or string; bad magic, version, flags or n_ctx;
// tau > 127; H or W zero; H * W > max_pixels; an m in 64..254; a zero frequency; frequencies that do not sum to
// 65536; inner_len or res_len running past the end; an empty inner file; bytes left over; whatever container_parse
// (vbr from the flags, n_levels, max_pixels) refuses in the inner file; an inner H x W that is not the outer one.
const char* container_parse_residual(const uint8_t* data, size_t n, uint32_t n_levels, uint64_t max_pixels,
                                     ResidualInfo* info);

// ---- The segmented residual file (DESIGN.md section 5 "Residual coding", "Segments"; residual_seg.h has the
// definitions): the residual string cut into independently coded segments of seg_len samples of the canonical order,
// so that a GPU codes and decodes them in parallel.  All integers big-endian:
//     4 bytes "MLR2" | >B version 0 | >B flags (bit 0: VBR level word inside) | >B tau | >B n_ctx = 24
//     >II H, W | >Q digest | the 24 tables, exactly as in "MLR1"
//     >I seg_len (256..65536) | >I n_seg = ceil(3 H W / seg_len) | >I inner_len, the inner file
//     >I res_len = 4 n_seg + the sum of the lengths | n_seg x >I segment byte lengths | the segments, concatenated
// A segment's bytes are rans_encode of its samples: a multiple of 4, at least 8 (the flush), and at most
// 4 (samples + RESIDUAL_SEG_SLACK) (residual_seg.h derives n + 2 words).  As H, "MLR2" exceeds every max_pixels.
constexpr uint32_t RESIDUAL_SEG_MIN = 256, RESIDUAL_SEG_MAX = 65536, RESIDUAL_SEG_SLACK = 4;
struct ResidualSegInfo {
  uint32_t H, W;
  uint32_t tau;
  bool vbr;
  uint64_t digest;
  uint8_t m[RESIDUAL_CTX];
  size_t freq_off[RESIDUAL_CTX];
  uint32_t seg_len, n_seg;
  size_t inner_off, inner_len;
  size_t res_off, res_len;    // the index and the segments
  size_t index_off;           // n_seg big-endian u32 lengths (= res_off)
  size_t data_off, data_len;  // the concatenated segments
  ContainerInfo inner;
};
inline bool is_residual_seg_file(const uint8_t* data, size_t n) {
  return n >= 4 && data[0] == 'M' && data[1] == 'L' && data[2] == 'R' && data[3] == '2';
}
// m, freq, inner as container_write_residual; seg_bytes: n_seg lengths; segs: their concatenation.  Refused, each with
// its own message: what container_write_residual refuses; seg_len outside 256..65536; n_seg not ceil(3 H W / seg_len);
// a segment length that is not a multiple of 4, is below 8 or is above the capacity bound; lengths that do not sum to
// segs_len.  The *len / out / cap protocol of container_write.
const char* container_write_residual_seg(uint32_t H, uint32_t W, bool vbr, uint32_t tau, uint64_t digest,
                                         const uint8_t* m, const uint16_t* freq, uint32_t seg_len, uint32_t n_seg,
                                         const uint32_t* seg_bytes, const uint8_t* inner, size_t inner_len,
                                         const uint8_t* segs, size_t segs_len, uint8_t* out, size_t cap, size_t* len);
// Refused, each with its own message: everything container_parse_residual refuses (with "MLR2" as the magic);
// truncation before seg_len / n_seg; seg_len outside 256..65536; n_seg not ceil(3 H W / seg_len); a segment length
// that is not a multiple of 4, is below 8 or is above the capacity bound of its samples; res_len below its index or
// not 4 n_seg + the sum of the lengths; bytes left over.
const char* container_parse_residual_seg(const uint8_t* data, size_t n, uint32_t n_levels, uint64_t max_pixels,
                                         ResidualSegInfo* info);

// ---- The deep residual file (DESIGN.md section 5 "Residual coding", "Deep samples"; residual16.h has the
// definitions): the segmented file for 9..16-bit samples.  The segments code hi = q >> shift; the low `shift` bits of
// every q are stored raw in the low-bit plane.  All integers big-endian, the plane's 64-bit words little-endian (as
// the rANS words are):
//     4 bytes "MLR3" | the rest of the "MLR2" header | the 24 tables | >B depth (9..16) | >B shift (0..depth - 7)
//     >I seg_len | >I n_seg | >I inner_len, the inner file | >I res_len | the index | the segments
//     >I lo_len = 8 * 3 H ceil(W / 64) shift | the low-bit plane
// There is no serial form.  As H, "MLR3" exceeds every max_pixels.
struct ResidualDeepInfo {
  ResidualSegInfo seg;  // everything the "MLR2" file has
  uint32_t depth, shift;
  size_t lo_off, lo_len;  // the low-bit plane
};
inline bool is_residual_deep_file(const uint8_t* data, size_t n) {
  return n >= 4 && data[0] == 'M' && data[1] == 'L' && data[2] == 'R' && data[3] == '3';
}
// As container_write_residual_seg, with depth, shift and the plane.  Refused besides, each with its own message: a
// depth outside 9..16; a shift outside 0..depth - 7; a lo_len that is not 8 * 3 H ceil(W / 64) shift.
const char* container_write_residual_deep(uint32_t H, uint32_t W, bool vbr, uint32_t tau, uint32_t depth,
                                          uint32_t shift, uint64_t digest, const uint8_t* m, const uint16_t* freq,
                                          uint32_t seg_len, uint32_t n_seg, const uint32_t* seg_bytes,
                                          const uint8_t* inner, size_t inner_len, const uint8_t* segs, size_t segs_len,
                                          const uint8_t* lo, size_t lo_len, uint8_t* out, size_t cap, size_t* len);
// Refused, each with its own message: everything container_parse_residual_seg refuses (with "MLR3" as the magic);
// truncation before depth and shift; a depth or shift out of range; truncation before lo_len; a wrong lo_len;
// truncation inside the plane; bytes left over.
const char* container_parse_residual_deep(const uint8_t* data, size_t n, uint32_t n_levels, uint64_t max_pixels,
                                          ResidualDeepInfo* info);

// ---- The Y'CbCr residual file (DESIGN.md section 5 "Residual coding", "Y'CbCr frames"; residual_yuv.h has the
// definitions): the deep file for the three planes of a frame.  H, W are the luma size, hc = ceil(H / sub_y),
// wc = ceil(W / sub_x), N = H W + 2 hc wc samples, G_0 = ceil(W / 64), G_1 = ceil(wc / 64).  Always segmented.
//     4 bytes "MLR4" | the rest of the "MLR2" header | the 24 tables
//     >B depth (8..16) | >B shift (0 at depth 8, else 0..depth - 7) | >B sub_x | >B sub_y | >B matrix (0..2)
//     >B flags (bit 0 full_range, bit 1 site_x left; the rest 0)
//     >I seg_len | >I n_seg = ceil(N / seg_len) | >I inner_len, the inner file | >I res_len | the index | the segments
//     >I lo_len = 8 shift (H G_0 + 2 hc G_1) | the low-bit plane (64-bit words little-endian)
// The inner file is what the Y'CbCr encode writes without a residual.  As H, "MLR4" exceeds every max_pixels.
struct ResidualYuvInfo {
  ResidualDeepInfo deep;  // everything the "MLR3" file has
  uint32_t sub_x, sub_y, matrix;
  bool full_range, site_left;
};
inline bool is_residual_yuv_file(const uint8_t* data, size_t n) {
  return n >= 4 && data[0] == 'M' && data[1] == 'L' && data[2] == 'R' && data[3] == '4';
}
// As container_write_residual_deep with the frame's fields; flags as in the file.  Refused besides, each with its own
// message: a depth outside 8..16; a nonzero shift at depth 8, a shift outside 0..depth - 7 above; a sub pair that is
// not {1, 1}, {2, 1} or {2, 2}; a matrix outside 0..2, matrix 2 at depth 8; reserved flag bits; n_seg not
// ceil(N / seg_len); a lo_len that is not 8 shift (H G_0 + 2 hc G_1).
const char* container_write_residual_yuv(uint32_t H, uint32_t W, bool vbr, uint32_t tau, uint32_t depth, uint32_t shift,
                                         uint32_t sub_x, uint32_t sub_y, uint32_t matrix, uint32_t flags,
                                         uint64_t digest, const uint8_t* m, const uint16_t* freq, uint32_t seg_len,
                                         uint32_t n_seg, const uint32_t* seg_bytes, const uint8_t* inner,
                                         size_t inner_len, const uint8_t* segs, size_t segs_len, const uint8_t* lo,
                                         size_t lo_len, uint8_t* out, size_t cap, size_t* len);
// Refused, each with its own message: everything container_parse_residual_seg refuses (with "MLR4" as the magic and
// n_seg against this frame's N); truncation before depth, shift and the frame's fields; what the writer refuses of
// them; truncation before lo_len; a wrong lo_len; truncation inside the plane; bytes left over.
const char* container_parse_residual_yuv(const uint8_t* data, size_t n, uint32_t n_levels, uint64_t max_pixels,
                                         ResidualYuvInfo* info);

}  // namespace mlic
#endif
