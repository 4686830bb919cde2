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

}  // namespace mlic
#endif
