// Host sanitizer check of the tiled container (mlic_amd/csrc/container.cpp: tile_count, container_write_tiled /
// container_parse_tiled / container_tiled_tile): the grid's properties, write, parse, every tile through the
// per-image parser, each listed refusal by its message, the truncation sweep and a seeded mutation sweep, every
// input in a heap block of exactly its size so that AddressSanitizer sees any read outside [data, data + n).
// Build and run from the repository root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       -Imlic_amd/csrc \
//       tools/container_tiled_check.cpp mlic_amd/csrc/container.cpp -o /tmp/container_tiled_check && /tmp/container_tiled_check
//
// Exit status 0 and a final "container_tiled_check ok" line mean: the grid covers every axis length tried with
// one or two tiles per position and weights that sum to the denominator, each file round-trips (header fields,
// every tile's bytes, every tile's H x W equal to the grid's extent), container_parse refuses it, every truncation
// is refused, each listed refusal gives its own message, 4000 single-byte and 4000 four-byte overwrites per file
// were each either refused with a message or parsed to an in-bounds, strictly increasing table, and the
// sanitizers reported nothing.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "container.h"

using namespace mlic;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {  // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

static long refused = 0, accepted = 0;
static const uint32_t NLEV = 6;
static const uint64_t MAXPIX = (uint64_t)1 << 32;

static bool grid_ok() {
  const uint32_t Ts[] = {128, 192, 256}, Vs[] = {0, 16, 32, 64};
  for (uint32_t T : Ts)
    for (uint32_t V : Vs) {
      if (tile_params_check(T, V) != nullptr) {
        std::printf("legal T = %u, V = %u refused\n", T, V);
        return false;
      }
      const uint32_t den = V ? 2 * V : 1;
      for (uint32_t L = 1; L <= 700; ++L) {
        const uint32_t n = tile_count(L, T, V);
        if (n > 1 && tile_extent(L, n - 1, T, V) <= V) return std::printf("last extent <= V at L = %u\n", L), false;
        if (tile_start(n - 1, T, V) + tile_extent(L, n - 1, T, V) != L) return std::printf("no cover at L = %u\n", L), false;
        for (uint32_t p = 0; p < L; ++p) {
          uint32_t cover = 0, sum = 0;
          for (uint32_t k = 0; k < n; ++k) {
            const uint32_t s = tile_start(k, T, V), e = tile_extent(L, k, T, V);
            if (p >= s && p < s + e) {
              ++cover;
              sum += tile_weight_num(p - s, k, n, T, V);
            }
          }
          if (cover < 1 || cover > 2 || sum != den) {
            std::printf("L = %u, T = %u, V = %u, position %u: %u tiles, weight %u / %u\n", L, T, V, p, cover, sum, den);
            return false;
          }
        }
      }
    }
  const uint32_t bad[][2] = {{0, 0}, {64, 0}, {100, 0}, {130, 0}, {65536, 0}, {128, 8}, {128, 48}, {128, 128}, {192, 128}};
  for (auto& b : bad)
    if (tile_params_check(b[0], b[1]) == nullptr) return std::printf("T = %u, V = %u accepted\n", b[0], b[1]), false;
  if (tile_params_check(128, 64) != nullptr || tile_params_check(65472, 64) != nullptr) return false;
  return true;
}

// parse a copy that owns exactly n bytes; *err_out = the refusal (or null); false on a contract violation
static bool probe(const std::vector<uint8_t>& file, size_t n, const char** err_out = nullptr, uint64_t max_pixels = MAXPIX) {
  std::unique_ptr<uint8_t[]> buf(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(buf.get(), file.data(), n);
  TiledInfo t;
  std::memset(&t, 0xee, sizeof t);
  const char* err = container_parse_tiled(n ? buf.get() : nullptr, n, max_pixels, &t);
  if (err_out) *err_out = err;
  if (err) {
    ++refused;
    if (!*err) {
      std::printf("refusal without a message\n");
      return false;
    }
    return true;
  }
  ++accepted;
  const uint64_t tiles = (uint64_t)t.ny * t.nx;
  bool ok = tile_params_check(t.T, t.V) == nullptr && t.H > 0 && t.W > 0 && (uint64_t)t.H * t.W <= max_pixels &&
            t.ny == tile_count(t.H, t.T, t.V) && t.nx == tile_count(t.W, t.T, t.V) && t.table_off == TILED_HEADER &&
            t.payload_off == TILED_HEADER + 8 * (tiles + 1) && t.payload_off <= n && t.payload_len == n - t.payload_off;
  size_t end = ok ? t.payload_off : 0;
  for (uint64_t k = 0; ok && k < tiles; ++k) {
    size_t off = 0, len = 0;
    ok = container_tiled_tile(buf.get(), n, &t, k, &off, &len) == nullptr && off == end && len > 0 && len <= n - off;
    if (ok) {
      // a tile's file through the per-image parser: refused or in bounds of the tile
      std::unique_ptr<uint8_t[]> tb(new uint8_t[len]);
      std::memcpy(tb.get(), buf.get() + off, len);
      ContainerInfo c;
      if (container_parse(tb.get(), len, t.vbr, NLEV, (uint64_t)1 << 28, &c) == nullptr)
        ok = c.y_off <= len && c.y_len <= len - c.y_off && c.z_off <= len && c.z_len <= len - c.z_off;
    }
    end = off + len;
  }
  ok = ok && end == n;
  size_t off = 0, len = 0;
  ok = ok && container_tiled_tile(buf.get(), n, &t, tiles, &off, &len) != nullptr;
  if (!ok) std::printf("accepted a file with out-of-contract fields\n");
  return ok;
}

static bool expect(const std::vector<uint8_t>& file, const char* word, uint64_t max_pixels = MAXPIX) {
  const char* err = nullptr;
  if (!probe(file, file.size(), &err, max_pixels)) return false;
  if (err == nullptr || std::strstr(err, word) == nullptr) {
    std::printf("expected a refusal naming \"%s\", got %s\n", word, err ? err : "acceptance");
    return false;
  }
  return true;
}

static void put32at(std::vector<uint8_t>& m, size_t at, uint32_t v) {
  m[at] = (uint8_t)(v >> 24), m[at + 1] = (uint8_t)(v >> 16), m[at + 2] = (uint8_t)(v >> 8), m[at + 3] = (uint8_t)v;
}

static bool sweep(uint32_t H, uint32_t W, uint32_t T, uint32_t V, int level) {
  const bool vbr = level >= 0;
  const uint32_t ny = tile_count(H, T, V), nx = tile_count(W, T, V);
  const size_t tiles = (size_t)ny * nx;
  std::vector<std::vector<uint8_t>> files(tiles);
  std::vector<uint8_t> payload;
  std::vector<uint64_t> lens(tiles);
  for (uint32_t ky = 0; ky < ny; ++ky)
    for (uint32_t kx = 0; kx < nx; ++kx) {
      const uint32_t h = tile_extent(H, ky, T, V), w = tile_extent(W, kx, T, V);
      std::vector<uint8_t> y(rnd() % 40), z(rnd() % 9);
      for (auto& v : y) v = (uint8_t)rnd();
      for (auto& v : z) v = (uint8_t)rnd();
      size_t len = 0;
      container_write(h, w, level, (h + 63) / 64, (w + 63) / 64, y.data(), y.size(), z.data(), z.size(), nullptr, 0, &len);
      auto& f = files[(size_t)ky * nx + kx];
      f.resize(len);
      if (container_write(h, w, level, (h + 63) / 64, (w + 63) / 64, y.data(), y.size(), z.data(), z.size(), f.data(), len,
                          &len)) {
        std::printf("tile write failed\n");
        return false;
      }
      lens[(size_t)ky * nx + kx] = len;
      payload.insert(payload.end(), f.begin(), f.end());
    }
  size_t len = 0;
  if (container_write_tiled(H, W, T, V, vbr, nullptr, lens.data(), tiles, nullptr, 0, &len) ||
      len != TILED_HEADER + 8 * (tiles + 1) + payload.size()) {
    std::printf("size query failed\n");
    return false;
  }
  std::vector<uint8_t> file(len);
  if (container_write_tiled(H, W, T, V, vbr, payload.data(), lens.data(), tiles, file.data(), len - 1, &len) == nullptr ||
      container_write_tiled(H, W, T, V, vbr, payload.data(), lens.data(), tiles + 1, file.data(), len, &len) == nullptr ||
      container_write_tiled(H, W, T + 1, V, vbr, payload.data(), lens.data(), tiles, file.data(), len, &len) == nullptr ||
      container_write_tiled(0, W, T, V, vbr, payload.data(), lens.data(), tiles, file.data(), len, &len) == nullptr) {
    std::printf("a short buffer, a wrong tile count, a bad tile size or H = 0 was not refused by the writer\n");
    return false;
  }
  {
    std::vector<uint64_t> l0 = lens;
    l0[tiles - 1] = 0;
    if (container_write_tiled(H, W, T, V, vbr, payload.data(), l0.data(), tiles, file.data(), len, &len) == nullptr) {
      std::printf("an empty tile was not refused by the writer\n");
      return false;
    }
  }
  if (container_write_tiled(H, W, T, V, vbr, payload.data(), lens.data(), tiles, file.data(), file.size(), &len)) {
    std::printf("write failed\n");
    return false;
  }
  // round trip: header, every tile's bytes, every tile's own header against the grid
  TiledInfo t;
  if (container_parse_tiled(file.data(), len, MAXPIX, &t) != nullptr || t.H != H || t.W != W || t.T != T || t.V != V ||
      t.ny != ny || t.nx != nx || t.vbr != vbr) {
    std::printf("round trip failed\n");
    return false;
  }
  for (size_t k = 0; k < tiles; ++k) {
    size_t off = 0, l = 0;
    ContainerInfo c;
    if (container_tiled_tile(file.data(), len, &t, k, &off, &l) != nullptr || l != files[k].size() ||
        std::memcmp(file.data() + off, files[k].data(), l) != 0 ||
        container_parse(file.data() + off, l, vbr, NLEV, (uint64_t)1 << 28, &c) != nullptr ||
        c.H != tile_extent(H, (uint32_t)(k / nx), T, V) || c.W != tile_extent(W, (uint32_t)(k % nx), T, V)) {
      std::printf("tile %zu did not round-trip\n", k);
      return false;
    }
  }
  // the per-image parsers keep refusing a tiled file
  ContainerInfo c;
  size_t mo = 0, ml = 0;
  if (container_parse(file.data(), len, false, 0, (uint64_t)1 << 28, &c) == nullptr ||
      container_parse(file.data(), len, true, NLEV, (uint64_t)1 << 28, &c) == nullptr ||
      container_parse_roi(file.data(), len, NLEV, (uint64_t)1 << 28, &c, &mo, &ml) == nullptr) {
    std::printf("a per-image parser accepted a tiled file\n");
    return false;
  }
  // the listed refusals, each by its message
  const size_t tab = TILED_HEADER, last = tab + 8 * tiles;
  std::vector<uint8_t> m = file;
  m[0] = 'X';
  if (!expect(m, "magic")) return false;
  m = file, m[4] = 1;
  if (!expect(m, "version")) return false;
  m = file, m[5] |= 2;
  if (!expect(m, "flags")) return false;
  m = file, m[15] = (uint8_t)(m[15] + 1);
  if (!expect(m, "multiple of 64")) return false;
  m = file, m[14] = 0, m[15] = 64;
  if (!expect(m, "at least 128")) return false;
  m = file, m[17] = 8;
  if (!expect(m, "0, 16, 32 or 64")) return false;
  m = file, put32at(m, 6, 0);
  if (!expect(m, "H or W is zero")) return false;
  m = file, put32at(m, 10, 0);
  if (!expect(m, "H or W is zero")) return false;
  if (!expect(file, "max_pixels", (uint64_t)H * W - 1)) return false;
  m = file, put32at(m, 18, ny + 1);
  if (!expect(m, "grid")) return false;
  m = file, put32at(m, 22, nx + 1);
  if (!expect(m, "grid")) return false;
  // a huge image whose table cannot fit: checked before the table is walked
  m = file, put32at(m, 6, 0xffffff00u), put32at(m, 10, 1), put32at(m, 18, tile_count(0xffffff00u, T, V)), put32at(m, 22, 1);
  if (!expect(m, "offset table does not fit")) return false;
  m = file, m[tab + 7] = 1;
  if (!expect(m, "first offset")) return false;
  if (tiles > 1) {
    m = file;
    std::memcpy(&m[tab + 8 * 2], &m[tab + 8], 8);  // offsets[2] = offsets[1]
    if (!expect(m, "strictly increasing")) return false;
  }
  m = file, m[last + 7] ^= 1;  // a tile's file is at least 20 bytes: the offset stays above the one before it
  if (!expect(m, "last offset")) return false;
  m = file, m.push_back(0);
  if (!expect(m, "last offset")) return false;
  {
    std::vector<uint8_t> head(file.begin(), file.begin() + TILED_HEADER - 1);
    if (!expect(head, "truncated header")) return false;
  }
  // truncation at every offset is refused
  for (size_t n = 0; n < len; ++n) {
    const char* err = nullptr;
    if (!probe(file, n, &err)) return false;
    if (err == nullptr) {
      std::printf("a file truncated to %zu of %zu bytes was accepted\n", n, len);
      return false;
    }
  }
  const size_t head = TILED_HEADER + 8 * (tiles + 1) + 32 < len ? TILED_HEADER + 8 * (tiles + 1) + 32 : len;
  for (int i = 0; i < 4000; ++i) {
    m = file;
    m[rnd() % ((i & 3) ? head : len)] = (uint8_t)rnd();  // mostly the header and the table
    if (!probe(m, len)) return false;
  }
  for (int i = 0; i < 4000; ++i) {
    m = file;
    const size_t at = rnd() % (((i & 3) ? head : len) - 3);
    put32at(m, at, (i & 1) ? rnd() : rnd() % 4096);
    if (!probe(m, len)) return false;
  }
  return true;
}

int main() {
  const bool ok = grid_ok() && sweep(200, 330, 128, 32, -1) && sweep(100, 90, 128, 0, 3) && sweep(128, 224, 128, 32, 5) &&
                  sweep(1, 1, 128, 64, -1) && sweep(700, 650, 192, 64, 0) && sweep(1080, 1920, 512, 16, -1);
  std::printf("refused %ld, accepted %ld\n", refused, accepted);
  if (!ok || refused == 0 || accepted == 0) {
    std::printf("container_tiled_check FAILED\n");
    return 1;
  }
  std::printf("container_tiled_check ok\n");
  return 0;
}
