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

// ------------------------------------------------------------------------------------------ tiled
const char* tile_params_check(uint32_t T, uint32_t V) {
  if (T % 64 != 0 || T < 128) return "tile grid: the tile must be a multiple of 64 and at least 128";
  if (T > 65472) return "tile grid: the tile does not fit 16 bits (at most 65472)";
  if (V != 0 && V != 16 && V != 32 && V != 64) return "tile grid: the overlap must be 0, 16, 32 or 64";
  if (V > T / 2) return "tile grid: the overlap is above half the tile";
  return nullptr;
}

uint32_t tile_count(uint32_t L, uint32_t T, uint32_t V) {
  if (L <= T) return 1;
  const uint64_t S = T - V;
  return (uint32_t)(((uint64_t)L - V + S - 1) / S);
}

namespace {

void put64(uint8_t* p, uint64_t v) {
  put32(p, (uint32_t)(v >> 32));
  put32(p + 4, (uint32_t)v);
}

uint64_t get64(const uint8_t* p) {
  uint64_t v = 0;
  for (int i = 0; i < 8; ++i) v = (v << 8) | p[i];
  return v;
}

}  // namespace

const char* container_write_tiled(uint32_t H, uint32_t W, uint32_t T, uint32_t V, bool vbr, const uint8_t* payload,
                                  const uint64_t* lens, size_t n_tiles, uint8_t* out, size_t cap, size_t* len) {
  if (len == nullptr) return "container_write_tiled: null len";
  if (const char* err = tile_params_check(T, V)) return err;
  if (H == 0 || W == 0) return "container_write_tiled: H or W is zero";
  const uint32_t ny = tile_count(H, T, V), nx = tile_count(W, T, V);
  if ((uint64_t)ny * nx != (uint64_t)n_tiles) return "container_write_tiled: n_tiles is not ny * nx of the grid";
  if (lens == nullptr) return "container_write_tiled: null lens";
  uint64_t total = 0;  // n_tiles <= 2^26 (the grid of 32-bit sides), each length <= 2^36: no overflow
  for (size_t k = 0; k < n_tiles; ++k) {
    if (lens[k] == 0) return "container_write_tiled: an empty tile file";
    if (lens[k] > ((uint64_t)1 << 36)) return "container_write_tiled: a tile file above 2^36 bytes";
    total += lens[k];
  }
  const uint64_t head = TILED_HEADER + 8 * ((uint64_t)n_tiles + 1);
  if (head + total > (uint64_t)SIZE_MAX) return "container_write_tiled: the file does not fit size_t";
  *len = (size_t)(head + total);
  if (out == nullptr) return nullptr;
  if (cap < *len) return "container_write_tiled: buffer too small";
  if (payload == nullptr) return "container_write_tiled: null payload";
  uint8_t* p = out;
  std::memcpy(p, "MLT1", 4);
  p[4] = 0;
  p[5] = vbr ? 1 : 0;
  put32(p + 6, H);
  put32(p + 10, W);
  p[14] = (uint8_t)(T >> 8);
  p[15] = (uint8_t)T;
  p[16] = (uint8_t)(V >> 8);
  p[17] = (uint8_t)V;
  put32(p + 18, ny);
  put32(p + 22, nx);
  p += TILED_HEADER;
  uint64_t at = 0;
  put64(p, 0);
  p += 8;
  for (size_t k = 0; k < n_tiles; ++k, p += 8) put64(p, at += lens[k]);
  std::memcpy(p, payload, (size_t)total);
  return nullptr;
}

const char* container_parse_tiled(const uint8_t* data, size_t n, uint64_t max_pixels, TiledInfo* info) {
  if (info == nullptr) return "container_parse_tiled: null info";
  if (data == nullptr && n != 0) return "container_parse_tiled: null data";
  if (n < TILED_HEADER) return "container_parse_tiled: truncated header";
  if (std::memcmp(data, "MLT1", 4) != 0) return "container_parse_tiled: bad magic (not a tiled file)";
  if (data[4] != 0) return "container_parse_tiled: unknown version";
  if (data[5] & ~1u) return "container_parse_tiled: unknown flags";
  Reader r{data, n, 6};
  TiledInfo t{};
  t.vbr = (data[5] & 1u) != 0;
  r.u32(&t.H);  // n >= TILED_HEADER: the header's reads succeed
  r.u32(&t.W);
  t.T = ((uint32_t)data[14] << 8) | data[15];
  t.V = ((uint32_t)data[16] << 8) | data[17];
  r.pos = 18;
  r.u32(&t.ny);
  r.u32(&t.nx);
  if (const char* err = tile_params_check(t.T, t.V)) return err;
  if (t.H == 0 || t.W == 0) return "container_parse_tiled: H or W is zero";
  if ((uint64_t)t.H > max_pixels / (uint64_t)t.W) return "container_parse_tiled: image exceeds max_pixels";
  if (t.ny != tile_count(t.H, t.T, t.V) || t.nx != tile_count(t.W, t.T, t.V))
    return "container_parse_tiled: ny, nx are not the grid of H, W, T, V";
  // ny, nx < 2^32 / 64 each: the product fits 64 bits; the table must fit before anything walks it
  const uint64_t tiles = (uint64_t)t.ny * t.nx;
  if (tiles + 1 > (uint64_t)(n - TILED_HEADER) / 8) return "container_parse_tiled: the offset table does not fit the file";
  t.table_off = TILED_HEADER;
  t.payload_off = TILED_HEADER + 8 * (size_t)(tiles + 1);
  t.payload_len = n - t.payload_off;
  const uint8_t* tab = data + t.table_off;
  if (get64(tab) != 0) return "container_parse_tiled: the first offset is not 0";
  uint64_t prev = 0;
  for (uint64_t k = 1; k <= tiles; ++k) {
    const uint64_t o = get64(tab + 8 * k);
    if (o <= prev) return "container_parse_tiled: the offsets are not strictly increasing";
    prev = o;
  }
  if (prev != (uint64_t)t.payload_len) return "container_parse_tiled: the last offset is not the payload's length";
  *info = t;
  return nullptr;
}

const char* container_tiled_tile(const uint8_t* data, size_t n, const TiledInfo* info, uint64_t k, size_t* off,
                                 size_t* len) {
  if (data == nullptr || info == nullptr || off == nullptr || len == nullptr) return "container_tiled_tile: null argument";
  const uint64_t tiles = (uint64_t)info->ny * info->nx;
  if (k >= tiles) return "container_tiled_tile: tile index outside the grid";
  // info must be what container_parse_tiled made of these n bytes: the table inside them, the payload after it
  bool own = n >= TILED_HEADER && tiles + 1 <= (uint64_t)(n - TILED_HEADER) / 8;
  own = own && info->table_off == TILED_HEADER && info->payload_off == TILED_HEADER + 8 * (tiles + 1);
  own = own && info->payload_off <= n && info->payload_len == n - info->payload_off;
  uint64_t a = 0, b = 0;
  if (own) {
    a = get64(data + info->table_off + 8 * k);
    b = get64(data + info->table_off + 8 * (k + 1));
    own = a < b && b <= info->payload_len;
  }
  if (!own) return "container_tiled_tile: info is not the parse of this file";
  *off = info->payload_off + (size_t)a;
  *len = (size_t)(b - a);
  return nullptr;
}

// ----------------------------------------------------------------------------------------- scaled
const char* scaled_ratio_check(uint64_t display, uint64_t coded) {
  if (display == 0 || coded == 0) return "scaled file: a size is zero";
  if (coded > 8 * display || display > 8 * coded)
    return "scaled file: the ratio of coded to display size leaves [1/8, 8]";
  return nullptr;
}

const char* container_write_scaled(uint32_t H, uint32_t W, bool vbr, uint32_t filter, const uint8_t* inner,
                                   size_t inner_len, uint8_t* out, size_t cap, size_t* len) {
  if (len == nullptr) return "container_write_scaled: null len";
  if (H == 0 || W == 0) return "container_write_scaled: H or W is zero";
  if (filter > 2) return "container_write_scaled: unknown filter (0 lanczos3, 1 bicubic, 2 triangle)";
  if (inner_len == 0) return "container_write_scaled: an empty inner file";
  if (inner_len > SIZE_MAX - SCALED_HEADER) return "container_write_scaled: the file does not fit size_t";
  *len = SCALED_HEADER + inner_len;
  if (out == nullptr) return nullptr;
  if (cap < *len) return "container_write_scaled: buffer too small";
  if (inner == nullptr) return "container_write_scaled: null inner file";
  std::memcpy(out, "MLS1", 4);
  out[4] = 0;
  out[5] = vbr ? 1 : 0;
  out[6] = (uint8_t)filter;
  out[7] = 0;
  put32(out + 8, H);
  put32(out + 12, W);
  std::memcpy(out + SCALED_HEADER, inner, inner_len);
  return nullptr;
}

const char* container_parse_scaled(const uint8_t* data, size_t n, uint32_t n_levels, uint64_t max_pixels,
                                   ScaledInfo* info) {
  if (info == nullptr) return "container_parse_scaled: null info";
  if (data == nullptr && n != 0) return "container_parse_scaled: null data";
  if (n < SCALED_HEADER) return "container_parse_scaled: truncated header";
  if (std::memcmp(data, "MLS1", 4) != 0) return "container_parse_scaled: bad magic (not a scaled file)";
  if (data[4] != 0) return "container_parse_scaled: unknown version";
  if (data[5] & ~1u) return "container_parse_scaled: unknown flags";
  if (data[6] > 2) return "container_parse_scaled: unknown filter";
  if (data[7] != 0) return "container_parse_scaled: the reserved byte is not 0";
  Reader r{data, n, 8};
  ScaledInfo s{};
  s.vbr = (data[5] & 1u) != 0;
  s.filter = data[6];
  r.u32(&s.H);  // n >= SCALED_HEADER: the header's reads succeed
  r.u32(&s.W);
  if (s.H == 0 || s.W == 0) return "container_parse_scaled: H or W is zero";
  if ((uint64_t)s.H > max_pixels / (uint64_t)s.W) return "container_parse_scaled: image exceeds max_pixels";
  s.inner_off = SCALED_HEADER;
  s.inner_len = n - SCALED_HEADER;
  if (const char* err = container_parse(data + s.inner_off, s.inner_len, s.vbr, n_levels, max_pixels, &s.inner)) return err;
  if (scaled_ratio_check(s.H, s.inner.H) || scaled_ratio_check(s.W, s.inner.W))
    return "container_parse_scaled: the ratio of coded to display size leaves [1/8, 8]";
  *info = s;
  return nullptr;
}

// ---------------------------------------------------------------------------------------- layered
namespace {
constexpr size_t LAYERED_FIXED = 16;  // magic, version, flags, S, reserved, H, W
}

size_t container_layered_bytes(size_t z_len, const size_t* layer_lens, uint32_t S, bool vbr) {
  if (S == 0 || S > LAYERED_MAX_S || layer_lens == nullptr) return 0;
  size_t total = LAYERED_FIXED + (vbr ? 4 : 0) + 8 + 4 + 4 * (size_t)S;
  if (z_len > SIZE_MAX - total) return 0;
  total += z_len;
  for (uint32_t k = 0; k < S; ++k) {
    if (layer_lens[k] > SIZE_MAX - total) return 0;
    total += layer_lens[k];
  }
  return total;
}

const char* container_write_layered(uint32_t H, uint32_t W, int32_t level, uint32_t hz, uint32_t wz, const uint8_t* z,
                                    size_t z_len, const uint8_t* const* layers, const size_t* layer_lens, uint32_t S,
                                    uint8_t* out, size_t cap, size_t* len) {
  if (len == nullptr) return "container_write_layered: null len";
  if (S == 0 || S > LAYERED_MAX_S) return "container_write_layered: S must be in 1..32";
  if (layer_lens == nullptr) return "container_write_layered: null layer lengths";
  if (z_len > 0xffffffffu) return "container_write_layered: a string longer than a 32-bit length";
  for (uint32_t k = 0; k < S; ++k)
    if (layer_lens[k] > 0xffffffffu) return "container_write_layered: a string longer than a 32-bit length";
  const bool vbr = level >= 0;
  const size_t total = container_layered_bytes(z_len, layer_lens, S, vbr);
  if (total == 0) return "container_write_layered: the file does not fit size_t";
  *len = total;
  if (out == nullptr) return nullptr;
  if (cap < total) return "container_write_layered: buffer too small";
  if (z_len && z == nullptr) return "container_write_layered: null string";
  if (layers == nullptr) return "container_write_layered: null layers";
  for (uint32_t k = 0; k < S; ++k)
    if (layer_lens[k] && layers[k] == nullptr) return "container_write_layered: null string";
  uint8_t* p = out;
  std::memcpy(p, "MLL1", 4);
  p[4] = 0;
  p[5] = vbr ? 1 : 0;
  p[6] = (uint8_t)S;
  p[7] = 0;
  put32(p + 8, H);
  put32(p + 12, W);
  p += LAYERED_FIXED;
  if (vbr) {
    put32(p, (uint32_t)level);
    p += 4;
  }
  put32(p, hz);
  put32(p + 4, wz);
  put32(p + 8, (uint32_t)z_len);
  p += 12;
  if (z_len) std::memcpy(p, z, z_len);
  p += z_len;
  for (uint32_t k = 0; k < S; ++k) {
    put32(p, (uint32_t)layer_lens[k]);
    p += 4;
    if (layer_lens[k]) std::memcpy(p, layers[k], layer_lens[k]);
    p += layer_lens[k];
  }
  return nullptr;
}

const char* container_parse_layered(const uint8_t* data, size_t n, uint32_t n_levels, uint64_t max_pixels,
                                    bool allow_truncated, LayeredInfo* info) {
  if (info == nullptr) return "container_parse_layered: null info";
  if (data == nullptr && n != 0) return "container_parse_layered: null data";
  if (n < LAYERED_FIXED) return "container_parse_layered: truncated header";
  if (std::memcmp(data, "MLL1", 4) != 0) return "container_parse_layered: bad magic (not a layered file)";
  if (data[4] != 0) return "container_parse_layered: unknown version";
  if (data[5] & ~1u) return "container_parse_layered: unknown flags";
  if (data[6] == 0 || data[6] > LAYERED_MAX_S) return "container_parse_layered: S is not in 1..32";
  if (data[7] != 0) return "container_parse_layered: the reserved byte is not 0";
  const bool vbr = (data[5] & 1u) != 0;
  Reader r{data, n, 8};
  LayeredInfo c{};
  c.S = data[6];
  uint32_t level = 0, ln = 0;
  r.u32(&c.H);  // n >= LAYERED_FIXED: these two reads succeed
  r.u32(&c.W);
  if (vbr && !r.u32(&level)) return "container_parse_layered: truncated header (level)";
  if (!r.u32(&c.hz) || !r.u32(&c.wz)) return "container_parse_layered: truncated header (h_z, w_z)";
  if (c.H == 0 || c.W == 0) return "container_parse_layered: H or W is zero";
  if (vbr && level >= n_levels) return "container_parse_layered: level is not below n_levels";
  c.level = vbr ? (int32_t)level : -1;
  if ((uint64_t)c.hz != ((uint64_t)c.H + 63) / 64 || (uint64_t)c.wz != ((uint64_t)c.W + 63) / 64)
    return "container_parse_layered: h_z, w_z are not ceil(H / 64), ceil(W / 64)";
  if ((uint64_t)c.hz * 64 > max_pixels / ((uint64_t)c.wz * 64))
    return "container_parse_layered: padded image exceeds max_pixels";
  if (!r.u32(&ln)) return "container_parse_layered: truncated before the z length";
  if (ln > r.n - r.pos) return "container_parse_layered: the z length runs past the end";
  c.z_off = r.pos;
  c.z_len = ln;
  r.pos += ln;
  for (uint32_t k = 0; k < c.S; ++k) {
    const bool word = r.u32(&ln);
    if (!word || ln > r.n - r.pos) {
      if (allow_truncated) break;  // a partial trailing length word or string is ignored
      return word ? "container_parse_layered: a layer length runs past the end"
                  : "container_parse_layered: truncated before a layer length";
    }
    c.layer_off[k] = r.pos;
    c.layer_len[k] = ln;
    r.pos += ln;
    c.layers_present = k + 1;
  }
  if (c.layers_present == c.S && r.pos != r.n) return "container_parse_layered: bytes left over after the last layer";
  *info = c;
  return nullptr;
}

// --------------------------------------------------------------------------------------- residual
const char* container_write_residual(uint32_t H, uint32_t W, bool vbr, uint32_t tau, uint64_t digest, const uint8_t* m,
                                     const uint16_t* freq, const uint8_t* inner, size_t inner_len, const uint8_t* res,
                                     size_t res_len, uint8_t* out, size_t cap, size_t* len) {
  if (len == nullptr) return "container_write_residual: null len";
  if (H == 0 || W == 0) return "container_write_residual: H or W is zero";
  if (tau > 127) return "container_write_residual: tau above 127";
  if (m == nullptr) return "container_write_residual: null m";
  if (inner_len == 0) return "container_write_residual: an empty inner file";
  if (inner_len > 0xffffffffu || res_len > 0xffffffffu)
    return "container_write_residual: a string longer than a 32-bit length";
  size_t total = RESIDUAL_HEADER + 8;
  for (uint32_t k = 0; k < RESIDUAL_CTX; ++k) {
    if (m[k] != RESIDUAL_ABSENT && m[k] > RESIDUAL_MAX_M) return "container_write_residual: an m outside 0..63";
    total += 1 + (m[k] == RESIDUAL_ABSENT ? 0 : 2 * (2 * (size_t)m[k] + 2));
  }
  if (inner_len > SIZE_MAX - total || res_len > SIZE_MAX - total - inner_len)
    return "container_write_residual: the file does not fit size_t";
  total += inner_len + res_len;
  *len = total;
  if (out == nullptr) return nullptr;
  if (cap < total) return "container_write_residual: buffer too small";
  if (freq == nullptr) return "container_write_residual: null frequencies";
  if (inner == nullptr || (res_len && res == nullptr)) return "container_write_residual: null string";
  for (uint32_t k = 0; k < RESIDUAL_CTX; ++k) {
    if (m[k] == RESIDUAL_ABSENT) continue;
    uint32_t sum = 0;
    for (uint32_t j = 0; j < 2 * (uint32_t)m[k] + 2; ++j) {
      if (freq[k * 128 + j] == 0) return "container_write_residual: a zero frequency";
      sum += freq[k * 128 + j];
    }
    if (sum != 65536) return "container_write_residual: frequencies do not sum to 65536";
  }
  std::memcpy(out, "MLR1", 4);
  out[4] = 0;
  out[5] = vbr ? 1 : 0;
  out[6] = (uint8_t)tau;
  out[7] = (uint8_t)RESIDUAL_CTX;
  put32(out + 8, H);
  put32(out + 12, W);
  put32(out + 16, (uint32_t)(digest >> 32));
  put32(out + 20, (uint32_t)digest);
  uint8_t* p = out + RESIDUAL_HEADER;
  for (uint32_t k = 0; k < RESIDUAL_CTX; ++k) {
    *p++ = m[k];
    if (m[k] == RESIDUAL_ABSENT) continue;
    for (uint32_t j = 0; j < 2 * (uint32_t)m[k] + 2; ++j) {
      *p++ = (uint8_t)(freq[k * 128 + j] >> 8);
      *p++ = (uint8_t)freq[k * 128 + j];
    }
  }
  put32(p, (uint32_t)inner_len);
  std::memcpy(p + 4, inner, inner_len);
  p += 4 + inner_len;
  put32(p, (uint32_t)res_len);
  if (res_len) std::memcpy(p + 4, res, res_len);
  return nullptr;
}

const char* container_parse_residual(const uint8_t* data, size_t n, uint32_t n_levels, uint64_t max_pixels,
                                     ResidualInfo* info) {
  if (info == nullptr) return "container_parse_residual: null info";
  if (data == nullptr && n != 0) return "container_parse_residual: null data";
  if (n < RESIDUAL_HEADER) return "container_parse_residual: truncated header";
  if (std::memcmp(data, "MLR1", 4) != 0) return "container_parse_residual: bad magic (not a residual file)";
  if (data[4] != 0) return "container_parse_residual: unknown version";
  if (data[5] & ~1u) return "container_parse_residual: unknown flags";
  if (data[6] > 127) return "container_parse_residual: tau above 127";
  if (data[7] != RESIDUAL_CTX) return "container_parse_residual: n_ctx is not 24";
  Reader r{data, n, 8};
  ResidualInfo s{};
  s.vbr = (data[5] & 1u) != 0;
  s.tau = data[6];
  uint32_t hi = 0, lo = 0;
  r.u32(&s.H);  // n >= RESIDUAL_HEADER: the header's reads succeed
  r.u32(&s.W);
  r.u32(&hi);
  r.u32(&lo);
  s.digest = ((uint64_t)hi << 32) | lo;
  if (s.H == 0 || s.W == 0) return "container_parse_residual: H or W is zero";
  if ((uint64_t)s.H > max_pixels / (uint64_t)s.W) return "container_parse_residual: image exceeds max_pixels";
  for (uint32_t k = 0; k < RESIDUAL_CTX; ++k) {
    if (r.n - r.pos < 1) return "container_parse_residual: truncated before a table's m";
    const uint8_t m = data[r.pos++];
    s.m[k] = m;
    s.freq_off[k] = r.pos;
    if (m == RESIDUAL_ABSENT) continue;
    if (m > RESIDUAL_MAX_M) return "container_parse_residual: an m outside 0..63";
    const size_t cnt = 2 * (size_t)m + 2;
    if (r.n - r.pos < 2 * cnt) return "container_parse_residual: truncated inside a table";
    uint32_t sum = 0;
    for (size_t j = 0; j < cnt; ++j) {
      const uint32_t f = ((uint32_t)data[r.pos + 2 * j] << 8) | data[r.pos + 2 * j + 1];
      if (f == 0) return "container_parse_residual: a zero frequency";
      sum += f;
    }
    if (sum != 65536) return "container_parse_residual: a table's frequencies do not sum to 65536";
    r.pos += 2 * cnt;
  }
  uint32_t ln = 0;
  if (!r.u32(&ln)) return "container_parse_residual: truncated before the inner length";
  if (ln > r.n - r.pos) return "container_parse_residual: the inner length runs past the end";
  if (ln == 0) return "container_parse_residual: an empty inner file";
  s.inner_off = r.pos;
  s.inner_len = ln;
  r.pos += ln;
  if (!r.u32(&ln)) return "container_parse_residual: truncated before the residual length";
  if (ln > r.n - r.pos) return "container_parse_residual: the residual length runs past the end";
  s.res_off = r.pos;
  s.res_len = ln;
  r.pos += ln;
  if (r.pos != r.n) return "container_parse_residual: bytes left over after the residual string";
  if (const char* err = container_parse(data + s.inner_off, s.inner_len, s.vbr, n_levels, max_pixels, &s.inner)) return err;
  if (s.inner.H != s.H || s.inner.W != s.W) return "container_parse_residual: the inner file's H x W is not the outer one";
  *info = s;
  return nullptr;
}

// ------------------------------------------------------------------------------ residual, segmented
namespace {
enum { K_SEG = 0, K_DEEP = 1, K_YUV = 2 };  // "MLR2", "MLR3", "MLR4"
struct YuvFields {                          // what the "MLR4" file says of its frame beyond depth and shift
  uint32_t sub_x, sub_y, matrix, flags;
};
// samples of the canonical order: 3 H W of an RGB image, H W + 2 hc wc of a Y'CbCr frame
uint64_t residual_samples(int kind, uint32_t H, uint32_t W, const YuvFields& y) {
  if (kind != K_YUV) return 3 * (uint64_t)H * W;
  const uint64_t hc = ((uint64_t)H + y.sub_y - 1) / y.sub_y, wc = ((uint64_t)W + y.sub_x - 1) / y.sub_x;
  return (uint64_t)H * W + 2 * hc * wc;
}
uint64_t residual_seg_count(uint64_t N, uint32_t seg_len) { return (N + seg_len - 1) / seg_len; }
uint64_t residual_seg_bound(uint64_t N, uint32_t seg_len, uint64_t k) {  // bytes segment k may take
  const uint64_t left = N - k * seg_len;
  return 4 * ((left < seg_len ? left : seg_len) + RESIDUAL_SEG_SLACK);
}
// the low-bit plane of the "MLR3" and the "MLR4" file
uint64_t residual_lo_bytes(int kind, uint32_t H, uint32_t W, const YuvFields& y, uint32_t shift) {
  if (kind != K_YUV) return 8 * 3 * (uint64_t)H * (((uint64_t)W + 63) / 64) * shift;
  const uint64_t hc = ((uint64_t)H + y.sub_y - 1) / y.sub_y, wc = ((uint64_t)W + y.sub_x - 1) / y.sub_x;
  return 8 * (uint64_t)shift * ((uint64_t)H * (((uint64_t)W + 63) / 64) + 2 * hc * ((wc + 63) / 64));
}
const char* residual_magic_of(int kind) { return kind == K_YUV ? "MLR4" : kind == K_DEEP ? "MLR3" : "MLR2"; }
}  // namespace

namespace {
// depth, shift and the frame's fields of the "MLR4" file: the same refusals on both sides
const char* residual_yuv_fields_check(bool write, uint32_t depth, uint32_t shift, const YuvFields& y) {
#define YUV_MSG(text) (write ? "container_write_residual_yuv: " text : "container_parse_residual_yuv: " text)
  if (depth < 8 || depth > 16) return YUV_MSG("depth outside 8..16");
  if (depth == 8 && shift != 0) return YUV_MSG("shift must be 0 at depth 8");
  if (depth > 8 && shift > depth - 7) return YUV_MSG("shift outside 0..depth - 7");
  if (!((y.sub_x == 1 && y.sub_y == 1) || (y.sub_x == 2 && (y.sub_y == 1 || y.sub_y == 2))))
    return YUV_MSG("sub_x, sub_y is not one of {1, 1}, {2, 1}, {2, 2}");
  if (y.matrix > 2) return YUV_MSG("matrix outside 0..2");
  if (y.matrix == 2 && depth == 8) return YUV_MSG("matrix 2 (BT.2020) at depth 8");
  if (y.flags & ~3u) return YUV_MSG("reserved flag bits are set");
  return nullptr;
#undef YUV_MSG
}

// The "MLR2", the "MLR3" and the "MLR4" file differ by the magic, by depth and shift (and the frame's fields) behind
// the tables, by the number of samples and by the low-bit plane behind the segments: one writer and one parser serve
// all three, and each refusal carries the name of its entry.
#define SEG_MSG(text)                                                                                              \
  (kind == K_YUV ? "container_write_residual_yuv: " text                                                           \
                 : kind == K_DEEP ? "container_write_residual_deep: " text : "container_write_residual_seg: " text)
const char* write_residual_seg(int kind, const YuvFields& yf, uint32_t depth, uint32_t shift, const uint8_t* lo,
                               size_t lo_len, uint32_t H,
                               uint32_t W, bool vbr, uint32_t tau, uint64_t digest, const uint8_t* m,
                               const uint16_t* freq, uint32_t seg_len, uint32_t n_seg, const uint32_t* seg_bytes,
                               const uint8_t* inner, size_t inner_len, const uint8_t* segs, size_t segs_len,
                               uint8_t* out, size_t cap, size_t* len) {
  if (len == nullptr) return SEG_MSG("null len");
  if (H == 0 || W == 0) return SEG_MSG("H or W is zero");
  if (tau > 127) return SEG_MSG("tau above 127");
  if (m == nullptr) return SEG_MSG("null m");
  if (seg_len < RESIDUAL_SEG_MIN || seg_len > RESIDUAL_SEG_MAX)
    return SEG_MSG("seg_len outside 256..65536");
  const bool deep = kind != K_SEG;
  if (kind == K_YUV) {
    if (const char* err = residual_yuv_fields_check(true, depth, shift, yf)) return err;
  }
  const uint64_t N = residual_samples(kind, H, W, yf);
  if ((uint64_t)n_seg != residual_seg_count(N, seg_len))
    return kind == K_YUV ? SEG_MSG("n_seg is not ceil(N / seg_len)") : SEG_MSG("n_seg is not ceil(3 H W / seg_len)");
  if (kind == K_DEEP) {
    if (depth < 9 || depth > 16) return SEG_MSG("depth outside 9..16");
    if (shift > depth - 7) return SEG_MSG("shift outside 0..depth - 7");
  }
  if (deep) {
    if ((uint64_t)lo_len != residual_lo_bytes(kind, H, W, yf, shift))
      return kind == K_YUV ? SEG_MSG("lo_len is not 8 * shift * (H G_0 + 2 hc G_1)")
                           : SEG_MSG("lo_len is not 8 * 3 H ceil(W / 64) shift");
    if (lo_len > 0xffffffffu) return SEG_MSG("a string longer than a 32-bit length");
  }
  if (inner_len == 0) return SEG_MSG("an empty inner file");
  if (inner_len > 0xffffffffu || segs_len > 0xffffffffu - 4 * (uint64_t)n_seg)
    return SEG_MSG("a string longer than a 32-bit length");
  size_t total = RESIDUAL_HEADER + 16 + (deep ? 6 : 0) + (kind == K_YUV ? 4 : 0);
  for (uint32_t k = 0; k < RESIDUAL_CTX; ++k) {
    if (m[k] != RESIDUAL_ABSENT && m[k] > RESIDUAL_MAX_M) return SEG_MSG("an m outside 0..63");
    total += 1 + (m[k] == RESIDUAL_ABSENT ? 0 : 2 * (2 * (size_t)m[k] + 2));
  }
  const size_t res_len = 4 * (size_t)n_seg + segs_len;
  if (inner_len > SIZE_MAX - total || res_len > SIZE_MAX - total - inner_len)
    return SEG_MSG("the file does not fit size_t");
  total += inner_len + res_len;
  if (deep) {
    if (lo_len > SIZE_MAX - total) return SEG_MSG("the file does not fit size_t");
    total += lo_len;
  }
  *len = total;
  if (out == nullptr) return nullptr;
  if (cap < total) return SEG_MSG("buffer too small");
  if (freq == nullptr) return SEG_MSG("null frequencies");
  if (inner == nullptr || seg_bytes == nullptr || segs == nullptr || (lo_len && lo == nullptr))
    return SEG_MSG("null string");
  for (uint32_t k = 0; k < RESIDUAL_CTX; ++k) {
    if (m[k] == RESIDUAL_ABSENT) continue;
    uint32_t sum = 0;
    for (uint32_t j = 0; j < 2 * (uint32_t)m[k] + 2; ++j) {
      if (freq[k * 128 + j] == 0) return SEG_MSG("a zero frequency");
      sum += freq[k * 128 + j];
    }
    if (sum != 65536) return SEG_MSG("frequencies do not sum to 65536");
  }
  uint64_t sum = 0;
  for (uint32_t k = 0; k < n_seg; ++k) {
    if (seg_bytes[k] % 4) return SEG_MSG("a segment length that is not a multiple of 4");
    if (seg_bytes[k] < 8) return SEG_MSG("a segment length below 8");
    if (seg_bytes[k] > residual_seg_bound(N, seg_len, k))
      return SEG_MSG("a segment length above the capacity bound");
    sum += seg_bytes[k];
  }
  if (sum != segs_len) return SEG_MSG("the segment lengths do not sum to the data length");
  std::memcpy(out, residual_magic_of(kind), 4);
  out[4] = 0;
  out[5] = vbr ? 1 : 0;
  out[6] = (uint8_t)tau;
  out[7] = (uint8_t)RESIDUAL_CTX;
  put32(out + 8, H);
  put32(out + 12, W);
  put32(out + 16, (uint32_t)(digest >> 32));
  put32(out + 20, (uint32_t)digest);
  uint8_t* p = out + RESIDUAL_HEADER;
  for (uint32_t k = 0; k < RESIDUAL_CTX; ++k) {
    *p++ = m[k];
    if (m[k] == RESIDUAL_ABSENT) continue;
    for (uint32_t j = 0; j < 2 * (uint32_t)m[k] + 2; ++j) {
      *p++ = (uint8_t)(freq[k * 128 + j] >> 8);
      *p++ = (uint8_t)freq[k * 128 + j];
    }
  }
  if (deep) {
    *p++ = (uint8_t)depth;
    *p++ = (uint8_t)shift;
  }
  if (kind == K_YUV) {
    *p++ = (uint8_t)yf.sub_x;
    *p++ = (uint8_t)yf.sub_y;
    *p++ = (uint8_t)yf.matrix;
    *p++ = (uint8_t)yf.flags;
  }
  put32(p, seg_len);
  put32(p + 4, n_seg);
  put32(p + 8, (uint32_t)inner_len);
  std::memcpy(p + 12, inner, inner_len);
  p += 12 + inner_len;
  put32(p, (uint32_t)res_len);
  p += 4;
  for (uint32_t k = 0; k < n_seg; ++k, p += 4) put32(p, seg_bytes[k]);
  std::memcpy(p, segs, segs_len);
  if (deep) {
    p += segs_len;
    put32(p, (uint32_t)lo_len);
    if (lo_len) std::memcpy(p + 4, lo, lo_len);
  }
  return nullptr;
}
#undef SEG_MSG
}  // namespace

const char* container_write_residual_seg(uint32_t H, uint32_t W, bool vbr, uint32_t tau, uint64_t digest,
                                         const uint8_t* m, const uint16_t* freq, uint32_t seg_len, uint32_t n_seg,
                                         const uint32_t* seg_bytes, const uint8_t* inner, size_t inner_len,
                                         const uint8_t* segs, size_t segs_len, uint8_t* out, size_t cap, size_t* len) {
  return write_residual_seg(K_SEG, YuvFields{}, 0, 0, nullptr, 0, H, W, vbr, tau, digest, m, freq, seg_len, n_seg, seg_bytes, inner,
                            inner_len, segs, segs_len, out, cap, len);
}

const char* container_write_residual_deep(uint32_t H, uint32_t W, bool vbr, uint32_t tau, uint32_t depth,
                                          uint32_t shift, uint64_t digest, const uint8_t* m, const uint16_t* freq,
                                          uint32_t seg_len, uint32_t n_seg, const uint32_t* seg_bytes,
                                          const uint8_t* inner, size_t inner_len, const uint8_t* segs, size_t segs_len,
                                          const uint8_t* lo, size_t lo_len, uint8_t* out, size_t cap, size_t* len) {
  return write_residual_seg(K_DEEP, YuvFields{}, depth, shift, lo, lo_len, H, W, vbr, tau, digest, m, freq, seg_len,
                            n_seg, seg_bytes, inner, inner_len, segs, segs_len, out, cap, len);
}

const char* container_write_residual_yuv(uint32_t H, uint32_t W, bool vbr, uint32_t tau, uint32_t depth, uint32_t shift,
                                         uint32_t sub_x, uint32_t sub_y, uint32_t matrix, uint32_t flags,
                                         uint64_t digest, const uint8_t* m, const uint16_t* freq, uint32_t seg_len,
                                         uint32_t n_seg, const uint32_t* seg_bytes, const uint8_t* inner,
                                         size_t inner_len, const uint8_t* segs, size_t segs_len, const uint8_t* lo,
                                         size_t lo_len, uint8_t* out, size_t cap, size_t* len) {
  return write_residual_seg(K_YUV, YuvFields{sub_x, sub_y, matrix, flags}, depth, shift, lo, lo_len, H, W, vbr, tau,
                            digest, m, freq, seg_len, n_seg, seg_bytes, inner, inner_len, segs, segs_len, out, cap, len);
}

namespace {
#define SEG_MSG(text)                                                                                              \
  (kind == K_YUV ? "container_parse_residual_yuv: " text                                                           \
                 : kind == K_DEEP ? "container_parse_residual_deep: " text : "container_parse_residual_seg: " text)
const char* parse_residual_seg(int kind, const uint8_t* data, size_t n, uint32_t n_levels, uint64_t max_pixels,
                               ResidualSegInfo* info, ResidualDeepInfo* more, YuvFields* frame) {
  const bool deep = kind != K_SEG;
  if (info == nullptr) return SEG_MSG("null info");
  if (data == nullptr && n != 0) return SEG_MSG("null data");
  if (n < RESIDUAL_HEADER) return SEG_MSG("truncated header");
  if (std::memcmp(data, residual_magic_of(kind), 4) != 0)
    return kind == K_YUV    ? "container_parse_residual_yuv: bad magic (not a Y'CbCr residual file)"
           : kind == K_DEEP ? "container_parse_residual_deep: bad magic (not a deep residual file)"
                            : SEG_MSG("bad magic (not a segmented residual file)");
  if (data[4] != 0) return SEG_MSG("unknown version");
  if (data[5] & ~1u) return SEG_MSG("unknown flags");
  if (data[6] > 127) return SEG_MSG("tau above 127");
  if (data[7] != RESIDUAL_CTX) return SEG_MSG("n_ctx is not 24");
  Reader r{data, n, 8};
  ResidualSegInfo s{};
  s.vbr = (data[5] & 1u) != 0;
  s.tau = data[6];
  uint32_t hi = 0, lo = 0;
  r.u32(&s.H);  // n >= RESIDUAL_HEADER: the header's reads succeed
  r.u32(&s.W);
  r.u32(&hi);
  r.u32(&lo);
  s.digest = ((uint64_t)hi << 32) | lo;
  if (s.H == 0 || s.W == 0) return SEG_MSG("H or W is zero");
  if ((uint64_t)s.H > max_pixels / (uint64_t)s.W) return SEG_MSG("image exceeds max_pixels");
  for (uint32_t k = 0; k < RESIDUAL_CTX; ++k) {
    if (r.n - r.pos < 1) return SEG_MSG("truncated before a table's m");
    const uint8_t m = data[r.pos++];
    s.m[k] = m;
    s.freq_off[k] = r.pos;
    if (m == RESIDUAL_ABSENT) continue;
    if (m > RESIDUAL_MAX_M) return SEG_MSG("an m outside 0..63");
    const size_t cnt = 2 * (size_t)m + 2;
    if (r.n - r.pos < 2 * cnt) return SEG_MSG("truncated inside a table");
    uint32_t sum = 0;
    for (size_t j = 0; j < cnt; ++j) {
      const uint32_t f = ((uint32_t)data[r.pos + 2 * j] << 8) | data[r.pos + 2 * j + 1];
      if (f == 0) return SEG_MSG("a zero frequency");
      sum += f;
    }
    if (sum != 65536) return SEG_MSG("a table's frequencies do not sum to 65536");
    r.pos += 2 * cnt;
  }
  uint32_t depth = 0, shift = 0;
  YuvFields yf{};
  if (kind == K_DEEP) {
    if (r.n - r.pos < 2) return SEG_MSG("truncated before depth, shift");
    depth = data[r.pos++];
    shift = data[r.pos++];
    if (depth < 9 || depth > 16) return SEG_MSG("depth outside 9..16");
    if (shift > depth - 7) return SEG_MSG("shift outside 0..depth - 7");
  }
  if (kind == K_YUV) {
    if (r.n - r.pos < 6) return SEG_MSG("truncated before depth, shift and the frame's fields");
    depth = data[r.pos++];
    shift = data[r.pos++];
    yf.sub_x = data[r.pos++];
    yf.sub_y = data[r.pos++];
    yf.matrix = data[r.pos++];
    yf.flags = data[r.pos++];
    if (const char* err = residual_yuv_fields_check(false, depth, shift, yf)) return err;
  }
  const uint64_t N = residual_samples(kind, s.H, s.W, yf);
  if (!r.u32(&s.seg_len) || !r.u32(&s.n_seg)) return SEG_MSG("truncated before seg_len, n_seg");
  if (s.seg_len < RESIDUAL_SEG_MIN || s.seg_len > RESIDUAL_SEG_MAX)
    return SEG_MSG("seg_len outside 256..65536");
  if ((uint64_t)s.n_seg != residual_seg_count(N, s.seg_len))
    return kind == K_YUV ? SEG_MSG("n_seg is not ceil(N / seg_len)") : SEG_MSG("n_seg is not ceil(3 H W / seg_len)");
  uint32_t ln = 0;
  if (!r.u32(&ln)) return SEG_MSG("truncated before the inner length");
  if (ln > r.n - r.pos) return SEG_MSG("the inner length runs past the end");
  if (ln == 0) return SEG_MSG("an empty inner file");
  s.inner_off = r.pos;
  s.inner_len = ln;
  r.pos += ln;
  if (!r.u32(&ln)) return SEG_MSG("truncated before the residual length");
  if (ln > r.n - r.pos) return SEG_MSG("the residual length runs past the end");
  s.res_off = r.pos;
  s.res_len = ln;
  if ((uint64_t)ln < 4 * (uint64_t)s.n_seg) return SEG_MSG("the residual length is below its index");
  s.index_off = r.pos;
  uint64_t sum = 4 * (uint64_t)s.n_seg;
  for (uint32_t k = 0; k < s.n_seg; ++k) {
    uint32_t v = 0;
    r.u32(&v);  // inside the residual length, which is inside the file
    if (v % 4) return SEG_MSG("a segment length that is not a multiple of 4");
    if (v < 8) return SEG_MSG("a segment length below 8");
    if (v > residual_seg_bound(N, s.seg_len, k))
      return SEG_MSG("a segment length above the capacity bound");
    sum += v;
  }
  if (sum != ln) return SEG_MSG("the residual length is not 4 n_seg + the segment lengths");
  s.data_off = r.pos;
  s.data_len = ln - 4 * (size_t)s.n_seg;
  r.pos += s.data_len;
  if (deep) {
    uint32_t lo_len = 0;
    if (!r.u32(&lo_len)) return SEG_MSG("truncated before the low-bit plane's length");
    if ((uint64_t)lo_len != residual_lo_bytes(kind, s.H, s.W, yf, shift))
      return kind == K_YUV ? SEG_MSG("lo_len is not 8 * shift * (H G_0 + 2 hc G_1)")
                           : SEG_MSG("lo_len is not 8 * 3 H ceil(W / 64) shift");
    if (lo_len > r.n - r.pos) return SEG_MSG("truncated inside the low-bit plane");
    more->depth = depth;
    more->shift = shift;
    more->lo_off = r.pos;
    more->lo_len = lo_len;
    if (frame) *frame = yf;
    r.pos += lo_len;
    if (r.pos != r.n) return SEG_MSG("bytes left over after the low-bit plane");
  }
  if (r.pos != r.n) return SEG_MSG("bytes left over after the segments");
  if (const char* err = container_parse(data + s.inner_off, s.inner_len, s.vbr, n_levels, max_pixels, &s.inner)) return err;
  if (s.inner.H != s.H || s.inner.W != s.W)
    return SEG_MSG("the inner file's H x W is not the outer one");
  *info = s;
  return nullptr;
}
#undef SEG_MSG
}  // namespace

const char* container_parse_residual_seg(const uint8_t* data, size_t n, uint32_t n_levels, uint64_t max_pixels,
                                         ResidualSegInfo* info) {
  return parse_residual_seg(K_SEG, data, n, n_levels, max_pixels, info, nullptr, nullptr);
}

const char* container_parse_residual_deep(const uint8_t* data, size_t n, uint32_t n_levels, uint64_t max_pixels,
                                          ResidualDeepInfo* info) {
  if (info == nullptr) return "container_parse_residual_deep: null info";
  ResidualDeepInfo d{};
  if (const char* err = parse_residual_seg(K_DEEP, data, n, n_levels, max_pixels, &d.seg, &d, nullptr)) return err;
  *info = d;
  return nullptr;
}

const char* container_parse_residual_yuv(const uint8_t* data, size_t n, uint32_t n_levels, uint64_t max_pixels,
                                         ResidualYuvInfo* info) {
  if (info == nullptr) return "container_parse_residual_yuv: null info";
  ResidualYuvInfo y{};
  YuvFields f{};
  if (const char* err = parse_residual_seg(K_YUV, data, n, n_levels, max_pixels, &y.deep.seg, &y.deep, &f)) return err;
  y.sub_x = f.sub_x, y.sub_y = f.sub_y, y.matrix = f.matrix;
  y.full_range = (f.flags & 1u) != 0;
  y.site_left = (f.flags & 2u) != 0;
  *info = y;
  return nullptr;
}

void container_roi_unpack(const uint8_t* map, uint64_t cells, uint8_t* levels) {
  for (uint64_t k = 0; k < cells; ++k) {
    const uint8_t byte = map[1 + (size_t)(k >> 1)];
    levels[k] = (k & 1) ? (uint8_t)(byte & 15u) : (uint8_t)(byte >> 4);
  }
}

}  // namespace mlic
