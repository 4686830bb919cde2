// Host sanitizer check of the residual container (mlic_amd/csrc/container.cpp: container_write_residual /
// container_parse_residual) and of the integer definitions (mlic_amd/csrc/residual.h): write, parse, each listed
// refusal by its message, the truncation sweep and a seeded mutation sweep, every input in a heap block of exactly
// its size so that AddressSanitizer sees any read outside [data, data + n); the quantiser's bound over all
// 256 x 256 x 128 cases, the division-free quotient against the division, the class sizes.  Build and run from the
// repository root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       -Imlic_amd/csrc \
//       tools/container_residual_check.cpp mlic_amd/csrc/container.cpp -o /tmp/container_residual_check && /tmp/container_residual_check
//
// Exit status 0 and a final "container_residual_check ok" line mean: each file round-trips (size, tau, flags,
// digest, tables, the inner file's bytes and its parse, the residual string), the per-image, ROI, tiled, scaled and
// layered parsers refuse it, every truncation is refused, each listed refusal gives its own message, 4000
// single-byte and 4000 four-byte overwrites per file were each either refused with a message or parsed to in-bounds
// fields, the definitions hold, and the sanitizers reported nothing.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "container.h"
#include "residual.h"

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

static bool definitions_ok() {
  for (int tau = 0; tau <= RES_MAX_TAU; ++tau) {
    const uint32_t magic = residual_magic(2 * tau + 1);
    for (int n = 0; n < 512; ++n)
      if (residual_div(n, magic) != n / (2 * tau + 1)) return std::printf("quotient wrong at %d / %d\n", n, 2 * tau + 1), false;
    for (int x = 0; x < 256; ++x)
      for (int b = 0; b < 256; ++b) {
        const int q = residual_quant(x, b, tau), rec = residual_rec(b, q, tau);
        const int e = x > rec ? x - rec : rec - x;
        if (e > tau || q < -255 || q > 255 || (tau == 0 && rec != x))
          return std::printf("bound broken at x %d base %d tau %d\n", x, b, tau), false;
        const int bin = residual_bin(q);
        if (bin < 0 || bin >= RES_BINS || ((q < -63 || q > 63) != (bin == RES_ESCAPE_BIN))) return std::printf("bin\n"), false;
      }
  }
  int sizes[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int a = 0; a < 256; ++a) {
    const int k = residual_class(a);
    if (k < 0 || k > 7) return std::printf("class out of range\n"), false;
    ++sizes[k];
  }
  const int want[8] = {2, 2, 4, 8, 16, 32, 64, 128};
  for (int k = 0; k < 8; ++k)
    if (sizes[k] != want[k]) return std::printf("class %d has %d members\n", k, sizes[k]), false;
  if ((RES_DIGEST_K & 1) == 0) return false;
  return true;
}

// parse a copy that owns exactly n bytes; *err_out = the refusal (or null); false on a contract violation
static bool probe(const std::vector<uint8_t>& file, size_t n, const char** err_out = nullptr, uint64_t max_pixels = MAXPIX) {
  std::unique_ptr<uint8_t[]> buf(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(buf.get(), file.data(), n);
  ResidualInfo s;
  std::memset(&s, 0xee, sizeof s);
  const char* err = container_parse_residual(n ? buf.get() : nullptr, n, NLEV, max_pixels, &s);
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
  bool ok = s.H > 0 && s.W > 0 && (uint64_t)s.H * s.W <= max_pixels && s.tau <= 127 && s.inner_off <= n &&
            len >= 1 && len <= n - s.inner_off && s.res_off <= n && s.res_len <= n - s.res_off &&
            s.res_off + s.res_len == n && s.inner_off + len + 4 == s.res_off && c.H == s.H && c.W == s.W &&
            c.y_off <= len && c.y_len <= len - c.y_off && c.z_off <= len && c.z_len <= len - c.z_off &&
            (s.vbr ? c.level >= 0 && (uint32_t)c.level < NLEV : c.level == -1);
  for (uint32_t k = 0; ok && k < RESIDUAL_CTX; ++k) {
    if (s.m[k] == RESIDUAL_ABSENT) continue;
    const size_t cnt = 2 * (size_t)s.m[k] + 2;
    ok = s.m[k] <= RESIDUAL_MAX_M && s.freq_off[k] <= n && 2 * cnt <= n - s.freq_off[k] && s.freq_off[k] + 2 * cnt <= s.inner_off;
    uint32_t sum = 0;
    for (size_t j = 0; ok && j < cnt; ++j) {
      const uint32_t f = ((uint32_t)buf[s.freq_off[k] + 2 * j] << 8) | buf[s.freq_off[k] + 2 * j + 1];
      ok = f >= 1;
      sum += f;
    }
    ok = ok && sum == 65536;
  }
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

// seeded tables: context k absent when bit k of `absent` is set; frequencies >= 1 summing to 65536
static void make_tables(uint32_t absent, uint8_t* m, std::vector<uint16_t>& freq) {
  freq.assign(RESIDUAL_CTX * 128, 0);
  for (uint32_t k = 0; k < RESIDUAL_CTX; ++k) {
    if (absent >> k & 1) {
      m[k] = RESIDUAL_ABSENT;
      continue;
    }
    m[k] = (uint8_t)(k == 0 ? 0 : k == 1 ? 63 : rnd() % 64);
    const uint32_t cnt = 2 * (uint32_t)m[k] + 2;
    uint32_t left = 65536 - cnt;
    for (uint32_t j = 0; j < cnt; ++j) {
      const uint32_t extra = j + 1 == cnt ? left : rnd() % (left / 2 + 1);
      freq[k * 128 + j] = (uint16_t)(1 + extra);
      left -= extra;
    }
  }
}

static bool sweep(uint32_t H, uint32_t W, int level, uint32_t tau, uint32_t absent) {
  const bool vbr = level >= 0;
  std::vector<uint8_t> y(rnd() % 40), z(rnd() % 9), res(rnd() % 50);
  for (auto& v : y) v = (uint8_t)rnd();
  for (auto& v : z) v = (uint8_t)rnd();
  for (auto& v : res) v = (uint8_t)rnd();
  const uint64_t digest = ((uint64_t)rnd() << 32) | rnd();
  size_t ilen = 0;
  container_write(H, W, level, (H + 63) / 64, (W + 63) / 64, y.data(), y.size(), z.data(), z.size(), nullptr, 0, &ilen);
  std::vector<uint8_t> inner(ilen);
  if (container_write(H, W, level, (H + 63) / 64, (W + 63) / 64, y.data(), y.size(), z.data(), z.size(), inner.data(), ilen,
                      &ilen))
    return std::printf("inner write failed\n"), false;
  uint8_t m[RESIDUAL_CTX];
  std::vector<uint16_t> freq;
  make_tables(absent, m, freq);
  size_t tables = 0;
  for (uint32_t k = 0; k < RESIDUAL_CTX; ++k) tables += 1 + (m[k] == RESIDUAL_ABSENT ? 0 : 2 * (2 * (size_t)m[k] + 2));
  size_t len = 0;
  if (container_write_residual(H, W, vbr, tau, digest, m, nullptr, nullptr, ilen, nullptr, res.size(), nullptr, 0, &len) ||
      len != RESIDUAL_HEADER + tables + 4 + ilen + 4 + res.size())
    return std::printf("size query failed\n"), false;
  std::vector<uint8_t> file(len);
  std::vector<uint16_t> bad = freq;
  uint8_t badm[RESIDUAL_CTX];
  std::memcpy(badm, m, sizeof badm);
  uint32_t first = 0;
  while (m[first] == RESIDUAL_ABSENT) ++first;
  badm[first] = 64;
  bad[first * 128] = 0;
  std::vector<uint16_t> bad2 = freq;
  bad2[first * 128] = (uint16_t)(bad2[first * 128] + 1);
  const uint8_t* rp = res.empty() ? nullptr : res.data();
  if (container_write_residual(H, W, vbr, tau, digest, m, freq.data(), inner.data(), ilen, rp, res.size(), file.data(), len - 1, &len) == nullptr ||
      container_write_residual(0, W, vbr, tau, digest, m, freq.data(), inner.data(), ilen, rp, res.size(), file.data(), len, &len) == nullptr ||
      container_write_residual(H, 0, vbr, tau, digest, m, freq.data(), inner.data(), ilen, rp, res.size(), file.data(), len, &len) == nullptr ||
      container_write_residual(H, W, vbr, 128, digest, m, freq.data(), inner.data(), ilen, rp, res.size(), file.data(), len, &len) == nullptr ||
      container_write_residual(H, W, vbr, tau, digest, badm, freq.data(), inner.data(), ilen, rp, res.size(), file.data(), len, &len) == nullptr ||
      container_write_residual(H, W, vbr, tau, digest, m, bad.data(), inner.data(), ilen, rp, res.size(), file.data(), len, &len) == nullptr ||
      container_write_residual(H, W, vbr, tau, digest, m, bad2.data(), inner.data(), ilen, rp, res.size(), file.data(), len, &len) == nullptr ||
      container_write_residual(H, W, vbr, tau, digest, nullptr, freq.data(), inner.data(), ilen, rp, res.size(), file.data(), len, &len) == nullptr ||
      container_write_residual(H, W, vbr, tau, digest, m, nullptr, inner.data(), ilen, rp, res.size(), file.data(), len, &len) == nullptr ||
      container_write_residual(H, W, vbr, tau, digest, m, freq.data(), inner.data(), 0, rp, res.size(), file.data(), len, &len) == nullptr ||
      container_write_residual(H, W, vbr, tau, digest, m, freq.data(), nullptr, ilen, rp, res.size(), file.data(), len, &len) == nullptr ||
      container_write_residual(H, W, vbr, tau, digest, m, freq.data(), inner.data(), ilen, rp, res.size(), file.data(), len, nullptr) == nullptr)
    return std::printf("a short buffer, a zero size, a bad tau, m or frequency, an empty or null inner file or a null "
                       "argument was not refused by the writer\n"), false;
  if (container_write_residual(H, W, vbr, tau, digest, m, freq.data(), inner.data(), ilen, rp, res.size(), file.data(),
                               file.size(), &len) || len != file.size())
    return std::printf("write failed\n"), false;
  ResidualInfo s;
  if (container_parse_residual(file.data(), len, NLEV, MAXPIX, &s) != nullptr || s.H != H || s.W != W || s.tau != tau ||
      s.vbr != vbr || s.digest != digest || s.inner_len != ilen || s.res_len != res.size() ||
      std::memcmp(file.data() + s.inner_off, inner.data(), ilen) != 0 ||
      (!res.empty() && std::memcmp(file.data() + s.res_off, res.data(), res.size()) != 0) || s.inner.H != H ||
      s.inner.W != W || s.inner.level != (vbr ? level : -1) || s.inner.y_len != y.size() || s.inner.z_len != z.size() ||
      !is_residual_file(file.data(), len) || std::memcmp(s.m, m, sizeof m) != 0)
    return std::printf("round trip failed\n"), false;
  for (uint32_t k = 0; k < RESIDUAL_CTX; ++k) {
    if (m[k] == RESIDUAL_ABSENT) continue;
    for (uint32_t j = 0; j < 2 * (uint32_t)m[k] + 2; ++j) {
      const uint32_t f = ((uint32_t)file[s.freq_off[k] + 2 * j] << 8) | file[s.freq_off[k] + 2 * j + 1];
      if (f != freq[k * 128 + j]) return std::printf("a frequency did not round-trip\n"), false;
    }
  }
  // the other parsers keep refusing a residual file
  ContainerInfo c;
  TiledInfo t;
  ScaledInfo sc;
  LayeredInfo la;
  size_t mo = 0, ml = 0;
  if (container_parse(file.data(), len, false, 0, MAXPIX, &c) == nullptr ||
      container_parse(file.data(), len, true, NLEV, MAXPIX, &c) == nullptr ||
      container_parse_roi(file.data(), len, NLEV, MAXPIX, &c, &mo, &ml) == nullptr ||
      container_parse_tiled(file.data(), len, (uint64_t)1 << 32, &t) == nullptr ||
      container_parse_scaled(file.data(), len, NLEV, MAXPIX, &sc) == nullptr ||
      container_parse_layered(file.data(), len, NLEV, MAXPIX, false, &la) == nullptr ||
      container_parse_layered(file.data(), len, NLEV, MAXPIX, true, &la) == nullptr)
    return std::printf("another parser accepted a residual file\n"), false;
  // the listed refusals, each by its message
  const size_t tab0 = RESIDUAL_HEADER;  // context 0's m byte
  const size_t inner_at = RESIDUAL_HEADER + tables + 4, res_at = inner_at + ilen + 4;
  std::vector<uint8_t> mm = file;
  mm[0] = 'X';
  if (!expect(mm, "magic")) return false;
  mm = file, mm[3] = 'S';
  if (!expect(mm, "magic")) return false;
  mm = file, mm[4] = 1;
  if (!expect(mm, "version")) return false;
  mm = file, mm[5] |= 2;
  if (!expect(mm, "flags")) return false;
  mm = file, mm[6] = 128;
  if (!expect(mm, "tau above 127")) return false;
  mm = file, mm[7] = 23;
  if (!expect(mm, "n_ctx")) return false;
  mm = file, put32at(mm, 8, 0);
  if (!expect(mm, "H or W is zero")) return false;
  mm = file, put32at(mm, 12, 0);
  if (!expect(mm, "H or W is zero")) return false;
  if (!expect(file, "max_pixels", (uint64_t)H * W - 1)) return false;
  {
    size_t at = tab0;  // the first table that is present
    for (uint32_t k = 0; k < first; ++k) at += 1;
    mm = file, mm[at] = 64;
    if (!expect(mm, "an m outside 0..63")) return false;
    mm = file, mm[at] = 254;
    if (!expect(mm, "an m outside 0..63")) return false;
    mm = file, mm[at + 1] = 0, mm[at + 2] = 0;
    if (!expect(mm, "a zero frequency")) return false;
    mm = file, mm[at + 2] = (uint8_t)(mm[at + 2] ^ 1);
    if (!expect(mm, mm[at + 1] == 0 && mm[at + 2] == 0 ? "a zero frequency" : "do not sum to 65536")) return false;
  }
  mm = file, put32at(mm, inner_at - 4, (uint32_t)(len - inner_at + 1));
  if (!expect(mm, "the inner length runs past the end")) return false;
  mm = file, put32at(mm, inner_at - 4, 0);
  if (!expect(mm, "")) return false;  // an empty inner file, or what follows no longer parses: refused either way
  mm = file, put32at(mm, res_at - 4, (uint32_t)res.size() + 1);
  if (!expect(mm, "the residual length runs past the end")) return false;
  mm = file, mm.push_back(0);
  if (!expect(mm, "left over")) return false;
  // the inner file's own refusals come through
  mm = file, mm[5] ^= 1;  // the flag no longer matches the inner file's header
  if (!expect(mm, "container_parse")) return false;
  mm = file, put32at(mm, inner_at, 0);
  if (!expect(mm, "container_parse: H or W is zero")) return false;
  mm = file, put32at(mm, inner_at, H + 1);
  if (!expect(mm, "")) return false;  // h_z may or may not still fit: refused by one message or the other
  mm = file, put32at(mm, inner_at + 4, W == 64 ? 63 : ((W + 63) / 64 * 64 == W ? W - 1 : W + 1));
  if (!expect(mm, "is not the outer one")) return false;
  if (vbr) {
    mm = file, put32at(mm, inner_at + 8, NLEV);
    if (!expect(mm, "level")) return false;
  }
  {
    std::vector<uint8_t> head(file.begin(), file.begin() + RESIDUAL_HEADER - 1);
    if (!expect(head, "truncated header")) return false;
    head.assign(file.begin(), file.begin() + RESIDUAL_HEADER);
    if (!expect(head, "truncated before a table's m")) return false;
    head.assign(file.begin(), file.begin() + inner_at - 5);
    if (!expect(head, "truncated")) return false;
    head.assign(file.begin(), file.begin() + inner_at - 1);
    if (!expect(head, "truncated before the inner length")) return false;
    head.assign(file.begin(), file.begin() + res_at - 1);
    if (!expect(head, "truncated before the residual length")) return false;
  }
  for (size_t n = 0; n < len; ++n) {
    const char* err = nullptr;
    if (!probe(file, n, &err)) return false;
    if (err == nullptr) return std::printf("a file truncated to %zu of %zu bytes was accepted\n", n, len), false;
  }
  for (int i = 0; i < 4000; ++i) {
    mm = file;
    mm[rnd() % ((i & 3) == 1 ? RESIDUAL_HEADER : len)] = (uint8_t)rnd();
    if (!probe(mm, len)) return false;
  }
  for (int i = 0; i < 4000; ++i) {
    mm = file;
    const size_t at = (i & 3) == 1 ? inner_at - 4 + rnd() % 24 : rnd() % (len - 3);
    put32at(mm, at < len - 3 ? at : len - 4, (i & 1) ? rnd() : rnd() % 4096);
    if (!probe(mm, len)) return false;
  }
  return true;
}

int main() {
  const bool ok = definitions_ok() && sweep(100, 150, -1, 0, 0) && sweep(100, 150, 3, 1, 0x00ff00) &&
                  sweep(1080, 1920, -1, 2, 0xfffffc) && sweep(17, 33, 5, 127, 0x555555) && sweep(1, 1, 0, 7, 0xaaaaaa) &&
                  sweep(64, 64, -1, 3, 0x7ffffe);
  std::printf("refused %ld, accepted %ld\n", refused, accepted);
  if (!ok || refused == 0 || accepted == 0) {
    std::printf("container_residual_check FAILED\n");
    return 1;
  }
  std::printf("container_residual_check ok\n");
  return 0;
}
