// Host sanitizer check of the layered container (mlic_amd/csrc/container.cpp: container_layered_bytes,
// container_write_layered, container_parse_layered): write, parse, the truncation sweep against the layout, each
// listed refusal by its message, and a byte-flip and overwrite sweep over the header, every input in a heap block
// of exactly its size so that AddressSanitizer sees any read outside [data, data + n).
// Build and run from the repository root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       -Imlic_amd/csrc \
//       tools/container_layered_check.cpp mlic_amd/csrc/container.cpp -o /tmp/container_layered_check && \
//       /tmp/container_layered_check
//
// Exit status 0 and a final "container_layered_check ok" line mean: each file round-trips (every header field, z
// and every layer's bytes; container_layered_bytes equals the written length), container_parse refuses it with
// and without a level word, every prefix of it parses with allow_truncated to exactly the layer count the layout
// gives (and is refused when cut before the end of z), without allow_truncated only the whole file parses, each
// listed refusal gives its own message, every single-bit flip and every byte and 32-bit overwrite of the header
// was either refused with a message or parsed to in-bounds, ordered strings, and the sanitizers reported nothing.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "container.h"

using namespace mlic;

static long refused = 0, accepted = 0;
static const uint32_t NLEV = 6;
static const uint64_t MAXPIX = (uint64_t)1 << 28;

// a copy in a heap block of exactly n bytes (n = 0: a one-byte block whose byte is never to be read)
static std::unique_ptr<uint8_t[]> exact(const uint8_t* p, size_t n) {
  std::unique_ptr<uint8_t[]> b(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(b.get(), p, n);
  return b;
}

struct File {
  uint32_t H, W, hz, wz, S;
  int32_t level;
  std::vector<uint8_t> z;
  std::vector<std::vector<uint8_t>> layers;
  std::vector<uint8_t> bytes;
  size_t z_end = 0;               // the first byte after the z string
  std::vector<size_t> layer_end;  // the first byte after layer k
};

static bool build(File& f) {
  std::vector<const uint8_t*> ptrs;
  std::vector<size_t> lens;
  for (auto& l : f.layers) {
    ptrs.push_back(l.empty() ? nullptr : l.data());
    lens.push_back(l.size());
  }
  size_t len = 0;
  const char* err = container_write_layered(f.H, f.W, f.level, f.hz, f.wz, f.z.data(), f.z.size(), ptrs.data(),
                                            lens.data(), f.S, nullptr, 0, &len);
  if (err) return std::printf("size query refused: %s\n", err), false;
  if (len != container_layered_bytes(f.z.size(), lens.data(), f.S, f.level >= 0))
    return std::printf("container_layered_bytes differs from the writer's length\n"), false;
  f.bytes.assign(len, 0xee);
  if (len > 0 && container_write_layered(f.H, f.W, f.level, f.hz, f.wz, f.z.data(), f.z.size(), ptrs.data(), lens.data(),
                                         f.S, f.bytes.data(), len - 1, &len) == nullptr)
    return std::printf("a buffer one byte short was accepted\n"), false;
  err = container_write_layered(f.H, f.W, f.level, f.hz, f.wz, f.z.data(), f.z.size(), ptrs.data(), lens.data(), f.S,
                                f.bytes.data(), f.bytes.size(), &len);
  if (err || len != f.bytes.size()) return std::printf("write refused: %s\n", err ? err : "length"), false;
  f.z_end = 16 + (f.level >= 0 ? 4 : 0) + 8 + 4 + f.z.size();
  size_t at = f.z_end;
  f.layer_end.clear();
  for (auto& l : f.layers) f.layer_end.push_back(at += 4 + l.size());
  if (at != len) return std::printf("the layout's length differs from the writer's\n"), false;
  return true;
}

// what a successful parse must satisfy whatever the bytes were
static bool in_bounds(const LayeredInfo& c, size_t n) {
  if (c.S < 1 || c.S > LAYERED_MAX_S || c.layers_present > c.S) return false;
  if (c.z_off > n || c.z_len > n - c.z_off) return false;
  size_t prev = c.z_off + c.z_len;
  for (uint32_t k = 0; k < c.layers_present; ++k) {
    if (c.layer_off[k] != prev + 4) return false;
    if (c.layer_off[k] > n || c.layer_len[k] > n - c.layer_off[k]) return false;
    prev = c.layer_off[k] + c.layer_len[k];
  }
  return c.layers_present < c.S || prev == n;
}

static bool round_trip(const File& f) {
  auto d = exact(f.bytes.data(), f.bytes.size());
  const size_t n = f.bytes.size();
  LayeredInfo c{};
  for (int trunc = 0; trunc < 2; ++trunc) {
    const char* err = container_parse_layered(d.get(), n, NLEV, MAXPIX, trunc != 0, &c);
    if (err) return std::printf("whole file refused: %s\n", err), false;
    if (c.H != f.H || c.W != f.W || c.hz != f.hz || c.wz != f.wz || c.level != (f.level >= 0 ? f.level : -1) ||
        c.S != f.S || c.layers_present != f.S || !in_bounds(c, n))
      return std::printf("header fields differ after the round trip\n"), false;
    if (c.z_len != f.z.size() || (c.z_len && std::memcmp(d.get() + c.z_off, f.z.data(), c.z_len) != 0))
      return std::printf("z differs after the round trip\n"), false;
    for (uint32_t k = 0; k < f.S; ++k)
      if (c.layer_len[k] != f.layers[k].size() ||
          (c.layer_len[k] && std::memcmp(d.get() + c.layer_off[k], f.layers[k].data(), c.layer_len[k]) != 0))
        return std::printf("layer %u differs after the round trip\n", k), false;
  }
  ContainerInfo p{};
  for (int vbr = 0; vbr < 2; ++vbr)
    if (container_parse(d.get(), n, vbr != 0, NLEV, MAXPIX, &p) == nullptr)
      return std::printf("container_parse accepted a layered file\n"), false;
  return true;
}

static bool truncation_sweep(const File& f) {
  for (size_t n = 0; n <= f.bytes.size(); ++n) {
    auto d = exact(f.bytes.data(), n);
    LayeredInfo c{};
    uint32_t want = 0;
    for (size_t e : f.layer_end) want += e <= n ? 1 : 0;
    const char* err = container_parse_layered(d.get(), n, NLEV, MAXPIX, true, &c);
    if (n < f.z_end) {
      if (err == nullptr) return std::printf("a cut at %zu, before the end of z, was accepted\n", n), false;
    } else {
      if (err) return std::printf("a cut at %zu was refused: %s\n", n, err), false;
      if (c.layers_present != want || !in_bounds(c, n))
        return std::printf("a cut at %zu gives %u layers, the layout %u\n", n, c.layers_present, want), false;
    }
    err = container_parse_layered(d.get(), n, NLEV, MAXPIX, false, &c);
    if ((err == nullptr) != (n == f.bytes.size()))
      return std::printf("without allow_truncated a cut at %zu was %s\n", n, err ? "refused" : "accepted"), false;
    (err ? refused : accepted)++;
  }
  return true;
}

static bool expect(const std::vector<uint8_t>& bytes, bool trunc, const char* part) {
  auto d = exact(bytes.data(), bytes.size());
  LayeredInfo c{};
  const char* err = container_parse_layered(d.get(), bytes.size(), NLEV, MAXPIX, trunc, &c);
  if (err == nullptr || std::strstr(err, part) == nullptr)
    return std::printf("expected a refusal with \"%s\", got %s\n", part, err ? err : "acceptance"), false;
  return true;
}

static void put32(std::vector<uint8_t>& b, size_t at, uint32_t v) {
  for (int i = 0; i < 4; ++i) b[at + i] = (uint8_t)(v >> (24 - 8 * i));
}

static bool refusals(const File& f) {  // f: a VBR file with at least two layers
  const size_t lv = 16, hz = 20, zl = 28;
  std::vector<uint8_t> b;
  auto with = [&](size_t at, uint8_t v) { b = f.bytes; b[at] = v; return b; };
  auto with32 = [&](size_t at, uint32_t v) { b = f.bytes; put32(b, at, v); return b; };
  bool ok = expect(with(0, 'X'), true, "bad magic") && expect(with(4, 1), true, "unknown version") &&
            expect(with(5, 2), true, "unknown flags") && expect(with(6, 0), true, "S is not in 1..32") &&
            expect(with(6, 33), true, "S is not in 1..32") && expect(with(7, 1), true, "reserved byte") &&
            expect(with32(8, 0), true, "H or W is zero") && expect(with32(12, 0), true, "H or W is zero") &&
            expect(with32(lv, NLEV), true, "level is not below n_levels") &&
            expect(with32(hz, f.hz + 1), true, "h_z, w_z are not") &&
            expect(with32(zl, 0x7fffffffu), true, "the z length runs past the end") &&
            expect(with32(f.z_end, 0x7fffffffu), false, "a layer length runs past the end");
  if (!ok) return false;
  b = f.bytes;
  b.push_back(0);
  if (!expect(b, true, "bytes left over") || !expect(b, false, "bytes left over")) return false;
  b = f.bytes;
  b.resize(f.layer_end[0] + 2);
  if (!expect(b, false, "truncated before a layer length")) return false;
  b = f.bytes;
  b.resize(10);
  if (!expect(b, true, "truncated header")) return false;
  // a size beyond max_pixels: 16448 x 16448 pads to more than 2^28 pixels
  b = f.bytes;
  put32(b, 8, 16448);
  put32(b, 12, 16448);
  put32(b, hz, 257);
  put32(b, hz + 4, 257);
  if (!expect(b, true, "exceeds max_pixels")) return false;
  // S larger than the layers that follow: a whole file by its bytes, but layers are missing
  b = f.bytes;
  b[6] = (uint8_t)(f.S + 1);
  if (!expect(b, false, "truncated before a layer length")) return false;
  LayeredInfo c{};
  auto d = exact(b.data(), b.size());
  if (container_parse_layered(d.get(), b.size(), NLEV, MAXPIX, true, &c) != nullptr || c.layers_present != f.S)
    return std::printf("S + 1 with allow_truncated: the S whole layers expected\n"), false;
  if (container_parse_layered(d.get(), b.size(), NLEV, MAXPIX, true, nullptr) == nullptr)
    return std::printf("null info accepted\n"), false;
  return true;
}

// every single-bit flip, and every byte and 32-bit overwrite with a set of telling values, over the header and
// the first length words: refused with a message, or parsed in bounds
static bool mutation_sweep(const File& f) {
  const size_t head = f.z_end + 8 < f.bytes.size() ? f.z_end + 8 : f.bytes.size();
  const uint32_t words[] = {0u, 1u, 2u, 0x7fffffffu, 0x80000000u, 0xffffffffu, (uint32_t)f.bytes.size(),
                            (uint32_t)f.bytes.size() - 1, 64u, 65u};
  auto check = [&](const std::vector<uint8_t>& b) {
    auto d = exact(b.data(), b.size());
    for (int trunc = 0; trunc < 2; ++trunc) {
      LayeredInfo c{};
      const char* err = container_parse_layered(d.get(), b.size(), NLEV, MAXPIX, trunc != 0, &c);
      if (err == nullptr && !in_bounds(c, b.size())) return false;
      if (err != nullptr && err[0] == 0) return false;
      (err ? refused : accepted)++;
    }
    return true;
  };
  for (size_t at = 0; at < head; ++at) {
    for (int bit = 0; bit < 8; ++bit) {
      std::vector<uint8_t> b = f.bytes;
      b[at] ^= (uint8_t)(1u << bit);
      if (!check(b)) return std::printf("bit %d of byte %zu: a parse out of bounds\n", bit, at), false;
    }
    for (uint32_t v : {0u, 1u, 32u, 33u, 127u, 128u, 255u}) {
      std::vector<uint8_t> b = f.bytes;
      b[at] = (uint8_t)v;
      if (!check(b)) return std::printf("byte %zu = %u: a parse out of bounds\n", at, v), false;
    }
    if (at + 4 <= f.bytes.size())
      for (uint32_t v : words) {
        std::vector<uint8_t> b = f.bytes;
        put32(b, at, v);
        if (!check(b)) return std::printf("word at %zu = %u: a parse out of bounds\n", at, v), false;
      }
  }
  return true;
}

static File make(uint32_t H, uint32_t W, int32_t level, uint32_t S, const std::vector<size_t>& lens, size_t zlen) {
  File f;
  f.H = H;
  f.W = W;
  f.hz = (H + 63) / 64;
  f.wz = (W + 63) / 64;
  f.S = S;
  f.level = level;
  f.z.resize(zlen);
  for (size_t i = 0; i < zlen; ++i) f.z[i] = (uint8_t)(0xa0 + i);
  for (uint32_t k = 0; k < S; ++k) {
    std::vector<uint8_t> l(lens[k % lens.size()]);
    for (size_t i = 0; i < l.size(); ++i) l[i] = (uint8_t)(17 * k + i + 1);
    f.layers.push_back(l);
  }
  return f;
}

int main() {
  std::vector<File> files;
  files.push_back(make(120, 200, -1, 4, {0, 1, 5, 9}, 3));
  files.push_back(make(120, 200, 3, 4, {0, 1, 5, 9}, 3));
  files.push_back(make(1, 1, -1, 1, {7}, 0));
  files.push_back(make(64, 65, 5, 10, {12, 0, 33, 8, 8, 0, 0, 100, 1, 2}, 40));
  files.push_back(make(1088, 1920, 0, 32, {3, 0}, 11));
  for (File& f : files) {
    if (!build(f) || !round_trip(f) || !truncation_sweep(f) || !mutation_sweep(f)) {
      std::printf("file %u x %u, S = %u, level %d failed\n", f.H, f.W, f.S, f.level);
      return 1;
    }
  }
  if (!refusals(files[1])) return 1;
  // the writer's own refusals
  size_t len = 0;
  const size_t one = 1;
  const uint8_t byte = 0;
  const uint8_t* ptr = &byte;
  if (container_write_layered(64, 64, -1, 1, 1, nullptr, 0, &ptr, &one, 0, nullptr, 0, &len) == nullptr ||
      container_write_layered(64, 64, -1, 1, 1, nullptr, 0, &ptr, &one, 33, nullptr, 0, &len) == nullptr ||
      container_write_layered(64, 64, -1, 1, 1, nullptr, 0, &ptr, &one, 1, nullptr, 0, nullptr) == nullptr ||
      container_layered_bytes(0, &one, 0, false) != 0 || container_layered_bytes(0, &one, 33, false) != 0) {
    std::printf("the writer accepted S outside 1..32 or a null len\n");
    return 1;
  }
  std::printf("%ld refused, %ld accepted\ncontainer_layered_check ok\n", refused, accepted);
  return 0;
}
