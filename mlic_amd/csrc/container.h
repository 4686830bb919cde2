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

}  // namespace mlic
#endif
