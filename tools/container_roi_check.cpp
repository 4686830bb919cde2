// Host sanitizer check of the ROI container (mlic_amd/csrc/container.cpp: container_write_roi / container_parse_roi):
// write, parse, unpack, the truncation sweep and a seeded mutation sweep, every input in a heap block of exactly
// its size so that AddressSanitizer sees any read outside [data, data + n).  Build and run from the repository
// root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Imlic_amd/csrc \
//       tools/container_roi_check.cpp mlic_amd/csrc/container.cpp -o /tmp/container_roi_check && /tmp/container_roi_check
//
// Exit status 0 and a final "container_roi_check ok" line mean: each file round-trips (fields, strings, every
// level of the map), container_parse refuses it for its n_strings, every truncation is refused, each listed
// refusal gives its own message, 4000 single-byte and 4000 four-byte overwrites per file were each either refused
// with a message or parsed to in-bounds offsets and in-range levels, and the sanitizers reported nothing.
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
static const uint64_t MAXPIX = (uint64_t)1 << 28;

// parse a copy that owns exactly n bytes; *err_out = the refusal (or null); false on a contract violation
static bool probe(const std::vector<uint8_t>& file, size_t n, const char** err_out = nullptr, uint32_t n_levels = NLEV) {
  std::unique_ptr<uint8_t[]> buf(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(buf.get(), file.data(), n);
  ContainerInfo c;
  std::memset(&c, 0xee, sizeof c);
  size_t off = 0, len = 0;
  const char* err = container_parse_roi(n ? buf.get() : nullptr, n, n_levels, MAXPIX, &c, &off, &len);
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
  bool ok = c.y_off <= n && c.y_len <= n - c.y_off && c.z_off <= n && c.z_len <= n - c.z_off &&
            c.y_off + c.y_len + 4 == c.z_off && c.H > 0 && c.W > 0 && c.hz == (c.H + 63) / 64 &&
            c.wz == (c.W + 63) / 64 && (uint64_t)c.hz * c.wz * 4096 <= MAXPIX && c.level >= 0 &&
            c.level < (int32_t)n_levels;
  if (len == 0) {
    ok = ok && c.z_off + c.z_len == n;
  } else {
    const uint64_t cells = (uint64_t)c.hz * c.wz;
    ok = ok && off == c.z_off + c.z_len + 4 && off + len == n && len == container_roi_map_bytes(c.hz, c.wz);
    if (ok) {
      std::vector<uint8_t> lv(cells);
      container_roi_unpack(buf.get() + off, cells, lv.data());
      for (uint8_t v : lv) ok = ok && v < n_levels;
    }
  }
  if (!ok) std::printf("accepted a file with out-of-contract fields\n");
  return ok;
}

static bool expect(const std::vector<uint8_t>& file, const char* word, uint32_t n_levels = NLEV) {
  const char* err = nullptr;
  if (!probe(file, file.size(), &err, n_levels)) return false;
  if (err == nullptr || std::strstr(err, word) == nullptr) {
    std::printf("expected a refusal naming \"%s\", got %s\n", word, err ? err : "acceptance");
    return false;
  }
  return true;
}

static bool sweep(uint32_t H, uint32_t W, int level, size_t y_len, size_t z_len) {
  const uint32_t hz = (H + 63) / 64, wz = (W + 63) / 64;
  const size_t cells = (size_t)hz * wz;
  std::vector<uint8_t> y(y_len), z(z_len), lv(cells);
  for (auto& v : y) v = (uint8_t)rnd();
  for (auto& v : z) v = (uint8_t)rnd();
  for (auto& v : lv) v = (uint8_t)(rnd() % (uint32_t)(level + 1));
  size_t len = 0, plain = 0;
  if (container_write(H, W, level, hz, wz, y.data(), y_len, z.data(), z_len, nullptr, 0, &plain) ||
      container_write_roi(H, W, level, hz, wz, y.data(), y_len, z.data(), z_len, nullptr, nullptr, 0, &len) ||
      len != plain + 4 + 1 + (cells + 1) / 2) {
    std::printf("size query failed\n");
    return false;
  }
  std::vector<uint8_t> file(len);
  if (container_write_roi(H, W, level, hz, wz, y.data(), y_len, z.data(), z_len, lv.data(), file.data(), len, &len)) {
    std::printf("write failed\n");
    return false;
  }
  if (container_write_roi(H, W, level, hz, wz, y.data(), y_len, z.data(), z_len, lv.data(), file.data(), len - 1, &len) ==
      nullptr) {
    std::printf("a short buffer was not refused\n");
    return false;
  }
  std::vector<uint8_t> big = lv;
  big[cells - 1] = 16;
  if (container_write_roi(H, W, level, hz, wz, y.data(), y_len, z.data(), z_len, big.data(), file.data(), len, &len) ==
          nullptr ||
      container_write_roi(H, W, -1, hz, wz, y.data(), y_len, z.data(), z_len, lv.data(), file.data(), len, &len) ==
          nullptr) {
    std::printf("a level above 15 or a file without a level word was not refused\n");
    return false;
  }
  if (container_write_roi(H, W, level, hz, wz, y.data(), y_len, z.data(), z_len, lv.data(), file.data(), len, &len)) {
    std::printf("write failed\n");
    return false;
  }
  // round trip
  ContainerInfo c;
  size_t off = 0, mlen = 0;
  std::vector<uint8_t> back(cells, 0xee);
  if (container_parse_roi(file.data(), len, NLEV, MAXPIX, &c, &off, &mlen) != nullptr || c.H != H || c.W != W ||
      c.level != level || c.y_len != y_len || c.z_len != z_len || mlen != 1 + (cells + 1) / 2 ||
      (y_len && std::memcmp(file.data() + c.y_off, y.data(), y_len) != 0) ||
      (z_len && std::memcmp(file.data() + c.z_off, z.data(), z_len) != 0)) {
    std::printf("round trip failed\n");
    return false;
  }
  container_roi_unpack(file.data() + off, cells, back.data());
  if (back != lv) {
    std::printf("the map did not round-trip\n");
    return false;
  }
  // the plain parser keeps refusing three strings
  const char* perr = container_parse(file.data(), len, true, NLEV, MAXPIX, &c);
  if (perr == nullptr || std::strstr(perr, "n_strings") == nullptr) {
    std::printf("container_parse did not refuse n_strings = 3\n");
    return false;
  }
  // the two-string file of the same strings parses with an empty map
  std::vector<uint8_t> two(plain);
  size_t l2 = 0;
  container_write(H, W, level, hz, wz, y.data(), y_len, z.data(), z_len, two.data(), plain, &l2);
  if (container_parse_roi(two.data(), plain, NLEV, MAXPIX, &c, &off, &mlen) != nullptr || mlen != 0) {
    std::printf("a two-string file did not parse with an empty map\n");
    return false;
  }
  // the listed refusals, each by its message
  std::vector<uint8_t> m = file;
  const size_t map_at = len - (1 + (cells + 1) / 2);
  m[map_at] = 1;
  if (!expect(m, "version byte")) return false;
  m = file;
  m[map_at + 1] = (uint8_t)((NLEV << 4) | (m[map_at + 1] & 15));
  if (!expect(m, "level of the map")) return false;
  m = file;
  m[map_at - 1] ^= 1;  // the map's length word
  if (!expect(m, "map length")) return false;
  m = file;
  m.push_back(0);
  if (!expect(m, "left over")) return false;
  if (cells & 1) {
    m = file;
    m[len - 1] |= 1;
    if (!expect(m, "padding nibble")) return false;
  }
  if (!expect(file, "above 16", 17)) return false;
  m = file;
  m[12 + 8 + 3] = 4;
  if (!expect(m, "n_strings")) return false;
  // truncation at every offset is refused
  for (size_t n = 0; n < len; ++n) {
    const char* err = nullptr;
    if (!probe(file, n, &err)) return false;
    if (err == nullptr) {
      std::printf("a file truncated to %zu of %zu bytes was accepted\n", n, len);
      return false;
    }
  }
  for (int i = 0; i < 4000; ++i) {
    m = file;
    m[rnd() % len] = (uint8_t)rnd();
    if (!probe(m, len)) return false;
  }
  for (int i = 0; i < 4000; ++i) {
    m = file;
    const size_t at = rnd() % (len - 3);
    const uint32_t v = (i & 1) ? rnd() : rnd() % 4096;
    m[at] = (uint8_t)(v >> 24);
    m[at + 1] = (uint8_t)(v >> 16);
    m[at + 2] = (uint8_t)(v >> 8);
    m[at + 3] = (uint8_t)v;
    if (!probe(m, len)) return false;
  }
  return true;
}

int main() {
  const bool ok = sweep(100, 150, 3, 301, 17) && sweep(120, 200, 5, 40, 9) && sweep(1, 1, 0, 0, 0) &&
                  sweep(64, 4097, 5, 0, 5) && sweep(1080, 1920, 5, 1500, 0);
  std::printf("refused %ld, accepted %ld\n", refused, accepted);
  if (!ok || refused == 0 || accepted == 0) {
    std::printf("container_roi_check FAILED\n");
    return 1;
  }
  std::printf("container_roi_check ok\n");
  return 0;
}
