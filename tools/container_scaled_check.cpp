// Host sanitizer check of the scaled container (mlic_amd/csrc/container.cpp: container_write_scaled /
// container_parse_scaled) and of the resampler's tables (mlic_amd/csrc/resample_table.h): write, parse, each listed
// refusal by its message, the truncation sweep and a seeded mutation sweep, every input in a heap block of exactly
// its size so that AddressSanitizer sees any read outside [data, data + n); the tables' windows stay inside the
// input and under the tap bound at every ratio tried.  Build and run from the repository root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       -Imlic_amd/csrc \
//       tools/container_scaled_check.cpp mlic_amd/csrc/container.cpp -o /tmp/container_scaled_check && /tmp/container_scaled_check
//
// Exit status 0 and a final "container_scaled_check ok" line mean: each file round-trips (display size, filter,
// flags, the inner file's bytes and its parse), the per-image and tiled parsers refuse it, every truncation is
// refused, each listed refusal gives its own message, 4000 single-byte and 4000 four-byte overwrites per file were
// each either refused with a message or parsed to in-bounds fields within the ratio range, the tables are sound,
// and the sanitizers reported nothing.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "container.h"
#include "resample_table.h"

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

// every window inside [0, Li), 1 <= n <= the bound, weights finite and summing to 1, zeros behind the row
static bool tables_ok() {
  int most = 0;
  for (int filter = 0; filter < RESAMPLE_FILTERS; ++filter)
    for (int Li = 1; Li <= 130; ++Li)
      for (int Lo = 1; Lo <= 130; ++Lo) {
        int taps = -1;
        const char* err = resample_table(filter, Li, Lo, nullptr, nullptr, nullptr, 0, &taps);
        const bool legal = Lo <= 8 * Li && Li <= 8 * Lo;
        if ((err == nullptr) != legal) return std::printf("ratio check wrong at %d -> %d\n", Li, Lo), false;
        if (!legal) continue;
        // exactly-sized heap blocks: a write outside them is a sanitizer report
        std::unique_ptr<int32_t[]> start(new int32_t[Lo]), count(new int32_t[Lo]);
        std::unique_ptr<float[]> w(new float[(size_t)Lo * taps]);
        int taps2 = -1;
        if (resample_table(filter, Li, Lo, start.get(), count.get(), w.get(), taps, &taps2) != nullptr || taps2 != taps)
          return std::printf("fill failed at %d -> %d\n", Li, Lo), false;
        if (taps > 1 && resample_table(filter, Li, Lo, start.get(), count.get(), w.get(), taps - 1, &taps2) == nullptr)
          return std::printf("a short stride was accepted at %d -> %d\n", Li, Lo), false;
        if (taps < 1 || taps > RESAMPLE_MAX_TAPS) return std::printf("tap bound broken at %d -> %d\n", Li, Lo), false;
        if (Li >= Lo && taps > 2 * resample_filter_radius(filter) * 8 + 1) return false;
        if (Li <= Lo && taps > 2 * resample_filter_radius(filter) + 1)
          return std::printf("upscale tap bound broken at %d -> %d\n", Li, Lo), false;
        most = taps > most ? taps : most;
        for (int o = 0; o < Lo; ++o) {
          const int n = count[o];
          if (n < 1 || n > taps || start[o] < 0 || start[o] + n > Li) return std::printf("window outside the input\n"), false;
          if (o > 0 && (start[o] < start[o - 1] || start[o] + n < start[o - 1] + count[o - 1]))
            return std::printf("windows not monotonic at %d -> %d\n", Li, Lo), false;
          double sum = 0;
          for (int j = 0; j < taps; ++j) {
            const float v = w[(size_t)o * taps + j];
            if (!std::isfinite(v) || (j >= n && v != 0.0f)) return std::printf("bad weight\n"), false;
            sum += v;
          }
          if (std::fabs(sum - 1.0) > 1e-5) return std::printf("weights sum to %g at %d -> %d\n", sum, Li, Lo), false;
          if (Li == Lo && (n != 1 || start[o] != o || w[(size_t)o * taps] != 1.0f)) return std::printf("identity\n"), false;
        }
      }
  int taps = 0;
  if (resample_table(0, 8000, 1000, nullptr, nullptr, nullptr, 0, &taps) != nullptr || taps > RESAMPLE_MAX_TAPS) return false;
  if (resample_table(3, 8, 8, nullptr, nullptr, nullptr, 0, &taps) == nullptr ||
      resample_table(-1, 8, 8, nullptr, nullptr, nullptr, 0, &taps) == nullptr ||
      resample_table(0, 0, 8, nullptr, nullptr, nullptr, 0, &taps) == nullptr ||
      resample_table(0, 8, 8, nullptr, nullptr, nullptr, 0, nullptr) == nullptr)
    return std::printf("a bad table request was accepted\n"), false;
  std::printf("largest table row: %d taps\n", most);
  return true;
}

// parse a copy that owns exactly n bytes; *err_out = the refusal (or null); false on a contract violation
static bool probe(const std::vector<uint8_t>& file, size_t n, const char** err_out = nullptr, uint64_t max_pixels = MAXPIX) {
  std::unique_ptr<uint8_t[]> buf(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(buf.get(), file.data(), n);
  ScaledInfo s;
  std::memset(&s, 0xee, sizeof s);
  const char* err = container_parse_scaled(n ? buf.get() : nullptr, n, NLEV, max_pixels, &s);
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
  const ContainerInfo& c = s.inner;
  const size_t len = s.inner_len;
  bool ok = s.H > 0 && s.W > 0 && (uint64_t)s.H * s.W <= max_pixels && s.filter <= 2 && s.inner_off == SCALED_HEADER &&
            len == n - SCALED_HEADER && c.H > 0 && c.W > 0 && (uint64_t)c.H <= 8 * (uint64_t)s.H &&
            (uint64_t)s.H <= 8 * (uint64_t)c.H && (uint64_t)c.W <= 8 * (uint64_t)s.W && (uint64_t)s.W <= 8 * (uint64_t)c.W &&
            c.y_off <= len && c.y_len <= len - c.y_off && c.z_off <= len && c.z_len <= len - c.z_off &&
            (s.vbr ? c.level >= 0 && (uint32_t)c.level < NLEV : c.level == -1);
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

static bool same(const uint8_t* p, const std::vector<uint8_t>& v) {  // an empty vector's data() may be null
  return v.empty() || std::memcmp(p, v.data(), v.size()) == 0;
}

static bool sweep(uint32_t H, uint32_t W, uint32_t h, uint32_t w, int level, uint32_t filter) {
  const bool vbr = level >= 0;
  std::vector<uint8_t> y(rnd() % 40), z(rnd() % 9);
  for (auto& v : y) v = (uint8_t)rnd();
  for (auto& v : z) v = (uint8_t)rnd();
  size_t ilen = 0;
  container_write(h, w, level, (h + 63) / 64, (w + 63) / 64, y.data(), y.size(), z.data(), z.size(), nullptr, 0, &ilen);
  std::vector<uint8_t> inner(ilen);
  if (container_write(h, w, level, (h + 63) / 64, (w + 63) / 64, y.data(), y.size(), z.data(), z.size(), inner.data(), ilen,
                      &ilen))
    return std::printf("inner write failed\n"), false;
  size_t len = 0;
  if (container_write_scaled(H, W, vbr, filter, nullptr, ilen, nullptr, 0, &len) || len != SCALED_HEADER + ilen)
    return std::printf("size query failed\n"), false;
  std::vector<uint8_t> file(len);
  if (container_write_scaled(H, W, vbr, filter, inner.data(), ilen, file.data(), len - 1, &len) == nullptr ||
      container_write_scaled(0, W, vbr, filter, inner.data(), ilen, file.data(), len, &len) == nullptr ||
      container_write_scaled(H, 0, vbr, filter, inner.data(), ilen, file.data(), len, &len) == nullptr ||
      container_write_scaled(H, W, vbr, 3, inner.data(), ilen, file.data(), len, &len) == nullptr ||
      container_write_scaled(H, W, vbr, filter, inner.data(), 0, file.data(), len, &len) == nullptr ||
      container_write_scaled(H, W, vbr, filter, nullptr, ilen, file.data(), len, &len) == nullptr ||
      container_write_scaled(H, W, vbr, filter, inner.data(), ilen, file.data(), len, nullptr) == nullptr)
    return std::printf("a short buffer, a zero size, a bad filter, an empty or null inner file or a null len was not "
                       "refused by the writer\n"), false;
  if (container_write_scaled(H, W, vbr, filter, inner.data(), ilen, file.data(), file.size(), &len) || len != file.size())
    return std::printf("write failed\n"), false;
  ScaledInfo s;
  if (container_parse_scaled(file.data(), len, NLEV, MAXPIX, &s) != nullptr || s.H != H || s.W != W || s.filter != filter ||
      s.vbr != vbr || s.inner_off != SCALED_HEADER || s.inner_len != ilen ||
      std::memcmp(file.data() + s.inner_off, inner.data(), ilen) != 0 || s.inner.H != h || s.inner.W != w ||
      s.inner.level != (vbr ? level : -1) || s.inner.y_len != y.size() || s.inner.z_len != z.size() ||
      !same(file.data() + s.inner_off + s.inner.y_off, y) || !same(file.data() + s.inner_off + s.inner.z_off, z) || !is_scaled_file(file.data(), len))
    return std::printf("round trip failed\n"), false;
  // the other parsers keep refusing a scaled file
  ContainerInfo c;
  TiledInfo t;
  size_t mo = 0, ml = 0;
  if (container_parse(file.data(), len, false, 0, MAXPIX, &c) == nullptr ||
      container_parse(file.data(), len, true, NLEV, MAXPIX, &c) == nullptr ||
      container_parse_roi(file.data(), len, NLEV, MAXPIX, &c, &mo, &ml) == nullptr ||
      container_parse_tiled(file.data(), len, (uint64_t)1 << 32, &t) == nullptr)
    return std::printf("another parser accepted a scaled file\n"), false;
  // the listed refusals, each by its message
  std::vector<uint8_t> m = file;
  m[0] = 'X';
  if (!expect(m, "magic")) return false;
  m = file, m[3] = 'T';
  if (!expect(m, "magic")) return false;
  m = file, m[4] = 1;
  if (!expect(m, "version")) return false;
  m = file, m[5] |= 2;
  if (!expect(m, "flags")) return false;
  m = file, m[6] = 3;
  if (!expect(m, "filter")) return false;
  m = file, m[7] = 1;
  if (!expect(m, "reserved")) return false;
  m = file, put32at(m, 8, 0);
  if (!expect(m, "H or W is zero")) return false;
  m = file, put32at(m, 12, 0);
  if (!expect(m, "H or W is zero")) return false;
  if (!expect(file, "max_pixels", (uint64_t)H * W - 1)) return false;
  m = file, put32at(m, 8, 8 * h + 1);
  if (!expect(m, "ratio")) return false;
  m = file, put32at(m, 12, 8 * w + 1);
  if (!expect(m, "ratio")) return false;
  if (h > 8) {
    m = file, put32at(m, 8, (h - 1) / 8);
    if (!expect(m, "ratio")) return false;
  }
  if (w > 8) {
    m = file, put32at(m, 12, (w - 1) / 8);
    if (!expect(m, "ratio")) return false;
  }
  m = file, put32at(m, 8, 8 * h), put32at(m, 12, (w + 7) / 8);  // both ends of the range are legal
  {
    const char* err = nullptr;
    if (!probe(m, m.size(), &err) || err != nullptr) return std::printf("ratio 8 or 1/8 refused: %s\n", err ? err : ""), false;
  }
  // the inner file's own refusals come through
  m = file, m[5] ^= 1;  // the flag no longer matches the inner file's header
  if (!expect(m, "container_parse")) return false;
  m = file, put32at(m, SCALED_HEADER, 0);
  if (!expect(m, "container_parse: H or W is zero")) return false;
  m = file, put32at(m, SCALED_HEADER + (vbr ? 12 : 8), 7);
  if (!expect(m, "h_z, w_z")) return false;
  if (vbr) {
    m = file, put32at(m, SCALED_HEADER + 8, NLEV);
    if (!expect(m, "level")) return false;
  }
  m = file, m.push_back(0);
  if (!expect(m, "left over")) return false;
  {
    std::vector<uint8_t> head(file.begin(), file.begin() + SCALED_HEADER - 1);
    if (!expect(head, "truncated header")) return false;
    head.assign(file.begin(), file.begin() + SCALED_HEADER);
    if (!expect(head, "container_parse: truncated header")) return false;
  }
  for (size_t n = 0; n < len; ++n) {
    const char* err = nullptr;
    if (!probe(file, n, &err)) return false;
    if (err == nullptr) return std::printf("a file truncated to %zu of %zu bytes was accepted\n", n, len), false;
  }
  const size_t head = SCALED_HEADER + 40 < len ? SCALED_HEADER + 40 : len;
  for (int i = 0; i < 4000; ++i) {
    m = file;
    m[rnd() % ((i & 3) ? head : len)] = (uint8_t)rnd();  // mostly the two headers
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
  const bool ok = tables_ok() && sweep(100, 150, 50, 75, -1, 0) && sweep(100, 150, 50, 75, 3, 1) &&
                  sweep(1080, 1920, 540, 960, -1, 2) && sweep(17, 33, 130, 257, 5, 0) && sweep(9, 9, 9, 9, 0, 1) &&
                  sweep(2160, 3840, 270, 480, -1, 0);
  std::printf("refused %ld, accepted %ld\n", refused, accepted);
  if (!ok || refused == 0 || accepted == 0) {
    std::printf("container_scaled_check FAILED\n");
    return 1;
  }
  std::printf("container_scaled_check ok\n");
  return 0;
}
