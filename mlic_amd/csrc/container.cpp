// Bitstream file writer and validating parser (container.h).  Host only: no HIP, no allocation.
#include "container.h"

#include <cstring>

namespace mlic {

namespace {

void put32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24);
  p[1] = (uint8_t)(v >> 16);
  p[2] = (uint8_t)(v >> 8);
  p[3] = (uint8_t)v;
}

// bounds-checked big-endian reader over [data, data + n)
struct Reader {
  const uint8_t* data;
  size_t n, pos;
  bool u32(uint32_t* v) {
    if (n - pos < 4) return false;
    const uint8_t* p = data + pos;
    *v = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
    pos += 4;
    return true;
  }
};

}  // namespace

size_t container_bytes(size_t y_len, size_t z_len, bool vbr) { return (vbr ? 12 : 8) + 12 + (4 + y_len) + (4 + z_len); }

const char* container_write(uint32_t H, uint32_t W, int32_t level, uint32_t hz, uint32_t wz, const uint8_t* y,
                            size_t y_len, const uint8_t* z, size_t z_len, uint8_t* out, size_t cap, size_t* len) {
  if (len == nullptr) return "container_write: null len";
  if (y_len > 0xffffffffu || z_len > 0xffffffffu) return "container_write: a string longer than a 32-bit length";
  const bool vbr = level >= 0;
  const size_t total = container_bytes(y_len, z_len, vbr);
  *len = total;
  if (out == nullptr) return nullptr;
  if (cap < total) return "container_write: buffer too small";
  if ((y_len && y == nullptr) || (z_len && z == nullptr)) return "container_write: null string";
  uint8_t* p = out;
  put32(p, H);
  put32(p + 4, W);
  p += 8;
  if (vbr) {
    put32(p, (uint32_t)level);
    p += 4;
  }
  put32(p, hz);
  put32(p + 4, wz);
  put32(p + 8, 2);
  p += 12;
  put32(p, (uint32_t)y_len);
  p += 4;
  if (y_len) std::memcpy(p, y, y_len);
  p += y_len;
  put32(p, (uint32_t)z_len);
  p += 4;
  if (z_len) std::memcpy(p, z, z_len);
  return nullptr;
}

const char* container_parse(const uint8_t* data, size_t n, bool vbr, uint32_t n_levels, uint64_t max_pixels,
                            ContainerInfo* info) {
  if (info == nullptr) return "container_parse: null info";
  if (data == nullptr && n != 0) return "container_parse: null data";
  Reader r{data, n, 0};
  ContainerInfo c{};
  uint32_t level = 0, nstr = 0;
  if (!r.u32(&c.H) || !r.u32(&c.W)) return "container_parse: truncated header (H, W)";
  if (vbr && !r.u32(&level)) return "container_parse: truncated header (level)";
  if (!r.u32(&c.hz) || !r.u32(&c.wz) || !r.u32(&nstr)) return "container_parse: truncated header (h_z, w_z, n_strings)";
  if (c.H == 0 || c.W == 0) return "container_parse: H or W is zero";
  if (vbr && level >= n_levels) return "container_parse: level is not below n_levels";
  c.level = vbr ? (int32_t)level : -1;
  if ((uint64_t)c.hz != ((uint64_t)c.H + 63) / 64 || (uint64_t)c.wz != ((uint64_t)c.W + 63) / 64)
    return "container_parse: h_z, w_z are not ceil(H / 64), ceil(W / 64)";
  // Hp, Wp <= 2^32 each (their product may not fit 64 bits): Hp * Wp > max  <=>  Hp > max / Wp
  if ((uint64_t)c.hz * 64 > max_pixels / ((uint64_t)c.wz * 64)) return "container_parse: padded image exceeds max_pixels";
  if (nstr != 2) return "container_parse: n_strings is not 2";
  uint32_t ln = 0;
  if (!r.u32(&ln)) return "container_parse: truncated before the y length";
  if (ln > r.n - r.pos) return "container_parse: the y length runs past the end";
  c.y_off = r.pos;
  c.y_len = ln;
  r.pos += ln;
  if (!r.u32(&ln)) return "container_parse: truncated before the z length";
  if (ln > r.n - r.pos) return "container_parse: the z length runs past the end";
  c.z_off = r.pos;
  c.z_len = ln;
  r.pos += ln;
  if (r.pos != r.n) return "container_parse: bytes left over after the z string";
  *info = c;
  return nullptr;
}

}  // namespace mlic
