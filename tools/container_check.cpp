// Host sanitizer check of the bitstream container (mlic_amd/csrc/container.cpp): a seeded mutation sweep of
// valid files through container_parse, every input in a heap block of exactly its size so that AddressSanitizer
// sees any read outside [data, data + n).  Build and run from the repository root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Imlic_amd/csrc \
//       tools/container_check.cpp mlic_amd/csrc/container.cpp -o /tmp/container_check && /tmp/container_check
//
// Exit status 0 and a final "container_check ok" line mean: every truncation of each file, 4000 single-byte and
// 4000 four-byte overwrites per file were each either refused with a message or parsed to in-bounds offsets, and
// the sanitizers reported nothing.
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

// parse a copy that owns exactly n bytes; returns false on a contract violation
static bool probe(const std::vector<uint8_t>& file, size_t n, bool vbr) {
  std::unique_ptr<uint8_t[]> buf(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(buf.get(), file.data(), n);
  ContainerInfo c;
  std::memset(&c, 0xee, sizeof c);
  const char* err = container_parse(n ? buf.get() : nullptr, n, vbr, 8, (uint64_t)1 << 28, &c);
  if (err) {
    ++refused;
    if (!*err) {
      std::printf("refusal without a message\n");
      return false;
    }
    return true;
  }
  ++accepted;
  const bool ok = c.y_off <= n && c.y_len <= n - c.y_off && c.z_off <= n && c.z_len <= n - c.z_off &&
                  c.y_off + c.y_len + 4 == c.z_off && c.z_off + c.z_len == n && c.H > 0 && c.W > 0 &&
                  c.hz == (c.H + 63) / 64 && c.wz == (c.W + 63) / 64 && (uint64_t)c.hz * c.wz * 4096 <= ((uint64_t)1 << 28) &&
                  (vbr ? (c.level >= 0 && c.level < 8) : c.level == -1);
  if (!ok) std::printf("accepted a file with out-of-contract fields\n");
  return ok;
}

static bool sweep(uint32_t H, uint32_t W, int level, size_t y_len, size_t z_len) {
  const bool vbr = level >= 0;
  std::vector<uint8_t> y(y_len), z(z_len);
  for (auto& v : y) v = (uint8_t)rnd();
  for (auto& v : z) v = (uint8_t)rnd();
  size_t len = 0;
  if (container_write(H, W, level, (H + 63) / 64, (W + 63) / 64, y.data(), y_len, z.data(), z_len, nullptr, 0, &len) ||
      len != container_bytes(y_len, z_len, vbr)) {
    std::printf("size query failed\n");
    return false;
  }
  std::vector<uint8_t> file(len);
  if (container_write(H, W, level, (H + 63) / 64, (W + 63) / 64, y.data(), y_len, z.data(), z_len, file.data(), len, &len)) {
    std::printf("write failed\n");
    return false;
  }
  if (len && container_write(H, W, level, 1, 1, y.data(), y_len, z.data(), z_len, file.data(), len - 1, &len) == nullptr) {
    std::printf("a short buffer was not refused\n");
    return false;
  }
  // round trip
  ContainerInfo c;
  if (container_parse(file.data(), len, vbr, 8, (uint64_t)1 << 28, &c) != nullptr || c.H != H || c.W != W ||
      c.level != (vbr ? level : -1) || c.y_len != y_len || c.z_len != z_len ||
      (y_len && std::memcmp(file.data() + c.y_off, y.data(), y_len) != 0) ||
      (z_len && std::memcmp(file.data() + c.z_off, z.data(), z_len) != 0)) {
    std::printf("round trip failed\n");
    return false;
  }
  // the other model kind reading this file must be refused or stay in bounds as well
  if (!probe(file, len, !vbr)) return false;
  for (size_t n = 0; n <= len; ++n)
    if (!probe(file, n, vbr)) return false;
  std::vector<uint8_t> m;
  for (int i = 0; i < 4000; ++i) {
    m = file;
    m[rnd() % len] = (uint8_t)rnd();
    if (!probe(m, len, vbr)) return false;
  }
  for (int i = 0; i < 4000; ++i) {
    m = file;
    const size_t at = rnd() % (len - 3);
    // half the words small (plausible sizes and lengths), half arbitrary
    const uint32_t v = (i & 1) ? rnd() : rnd() % 4096;
    m[at] = (uint8_t)(v >> 24);
    m[at + 1] = (uint8_t)(v >> 16);
    m[at + 2] = (uint8_t)(v >> 8);
    m[at + 3] = (uint8_t)v;
    if (!probe(m, len, vbr)) return false;
  }
  return true;
}

int main() {
  const bool ok = sweep(100, 150, -1, 301, 17) && sweep(100, 150, 3, 301, 17) && sweep(1, 1, -1, 0, 0) &&
                  sweep(64, 4097, 0, 0, 5) && sweep(1080, 1920, 7, 1500, 0);
  std::printf("refused %ld, accepted %ld\n", refused, accepted);
  if (!ok || refused == 0 || accepted == 0) {
    std::printf("container_check FAILED\n");
    return 1;
  }
  std::printf("container_check ok\n");
  return 0;
}
