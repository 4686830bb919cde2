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

namespace {

// the shared parser: roi = the ROI form (a level word always, 2 or 3 strings)
const char* parse_file(const uint8_t* data, size_t n, bool vbr, uint32_t n_levels, uint64_t max_pixels, bool roi,
                       ContainerInfo* info, size_t* map_off, size_t* map_len) {
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
  if (!roi && nstr != 2) return "container_parse: n_strings is not 2";
  if (roi && nstr != 2 && nstr != 3) return "container_parse_roi: n_strings is not 2 or 3";
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
  size_t moff = 0, mlen = 0;
  if (nstr == 3) {
    if (!r.u32(&ln)) return "container_parse_roi: truncated before the map length";
    // 64 hz * 64 wz <= max_pixels < 2^64, so the cell count fits 64 bits
    const uint64_t cells = (uint64_t)c.hz * c.wz;
    if ((uint64_t)ln != 1 + (cells + 1) / 2) return "container_parse_roi: the map length is not 1 + ceil(h_z * w_z / 2)";
    if (ln > r.n - r.pos) return "container_parse_roi: the map length runs past the end";
    moff = r.pos;
    mlen = ln;
    r.pos += ln;
    if (r.pos != r.n) return "container_parse_roi: bytes left over after the level map";
    if (data[moff] != 0) return "container_parse_roi: the map's version byte is not 0";
    for (uint64_t k = 0; k < cells; ++k) {
      const uint8_t byte = data[moff + 1 + (size_t)(k >> 1)];
      const uint32_t lv = (k & 1) ? (byte & 15u) : (byte >> 4);
      if (lv >= n_levels) return "container_parse_roi: a level of the map is not below n_levels";
    }
    if ((cells & 1) && (data[moff + mlen - 1] & 15u) != 0)
      return "container_parse_roi: the map's padding nibble is not 0";
  } else if (r.pos != r.n) {
    return "container_parse: bytes left over after the z string";
  }
  *info = c;
  if (map_off) *map_off = moff;
  if (map_len) *map_len = mlen;
  return nullptr;
}

}  // namespace

const char* container_parse(const uint8_t* data, size_t n, bool vbr, uint32_t n_levels, uint64_t max_pixels,
                            ContainerInfo* info) {
  if (info == nullptr) return "container_parse: null info";
  return parse_file(data, n, vbr, n_levels, max_pixels, false, info, nullptr, nullptr);
}

size_t container_roi_map_bytes(uint32_t hz, uint32_t wz) { return 1 + (size_t)(((uint64_t)hz * wz + 1) / 2); }

const char* container_write_roi(uint32_t H, uint32_t W, int32_t level, uint32_t hz, uint32_t wz, const uint8_t* y,
                                size_t y_len, const uint8_t* z, size_t z_len, const uint8_t* levels, uint8_t* out,
                                size_t cap, size_t* len) {
  if (len == nullptr) return "container_write_roi: null len";
  if (level < 0) return "container_write_roi: an ROI file is a VBR file (level >= 0 expected)";
  if (hz == 0 || wz == 0) return "container_write_roi: h_z or w_z is zero";
  const uint64_t cells = (uint64_t)hz * wz;
  if (cells > 0x7fffffffu) return "container_write_roi: a map longer than a 32-bit length";
  const size_t map_len = container_roi_map_bytes(hz, wz);
  size_t head = 0;
  const char* err = container_write(H, W, level, hz, wz, y, y_len, z, z_len, nullptr, 0, &head);
  if (err) return err;
  *len = head + 4 + map_len;
  if (out == nullptr) return nullptr;
  if (cap < *len) return "container_write_roi: buffer too small";
  if (levels == nullptr) return "container_write_roi: null level map";
  for (uint64_t k = 0; k < cells; ++k)
    if (levels[k] > 15) return "container_write_roi: a level does not fit four bits";
  err = container_write(H, W, level, hz, wz, y, y_len, z, z_len, out, cap, &head);
  if (err) return err;
  put32(out + 12 + 8, 3);  // n_strings, after H, W, level, h_z, w_z
  uint8_t* p = out + head;
  put32(p, (uint32_t)map_len);
  p += 4;
  *p++ = 0;  // version
  for (uint64_t k = 0; k < cells; k += 2)
    *p++ = (uint8_t)((levels[k] << 4) | (k + 1 < cells ? levels[k + 1] : 0));
  return nullptr;
}

const char* container_parse_roi(const uint8_t* data, size_t n, uint32_t n_levels, uint64_t max_pixels,
                                ContainerInfo* info, size_t* map_off, size_t* map_len) {
  if (info == nullptr || map_off == nullptr || map_len == nullptr) return "container_parse_roi: null info";
  if (n_levels < 1) return "container_parse_roi: n_levels >= 1 expected";
  if (n_levels > 16) return "container_parse_roi: n_levels is above 16 (a level is four bits)";
  return parse_file(data, n, true, n_levels, max_pixels, true, info, map_off, map_len);
}

void container_roi_unpack(const uint8_t* map, uint64_t cells, uint8_t* levels) {
  for (uint64_t k = 0; k < cells; ++k) {
    const uint8_t byte = map[1 + (size_t)(k >> 1)];
    levels[k] = (k & 1) ? (uint8_t)(byte & 15u) : (uint8_t)(byte >> 4);
  }
}

}  // namespace mlic
