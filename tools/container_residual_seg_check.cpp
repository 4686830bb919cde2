// Host sanitizer check of the segmented residual container (mlic_amd/csrc/container.cpp:
// container_write_residual_seg / container_parse_residual_seg) and of the segment capacity bound
// (mlic_amd/csrc/residual_seg.h) against the host rANS coder (mlic_amd/csrc/rans.cpp).  Every parsed input sits in
// a heap block of exactly its size, so AddressSanitizer sees any read outside [data, data + n).  Build and run from
// the repository root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       -Imlic_amd/csrc tools/container_residual_seg_check.cpp mlic_amd/csrc/container.cpp mlic_amd/csrc/rans.cpp \
//       -o /tmp/container_residual_seg_check && /tmp/container_residual_seg_check
//
// Exit status 0 and a final "container_residual_seg_check ok" line mean: plain and VBR files round-trip (every
// field, the index, the segments' bytes), every truncation is refused, each listed refusal gives its own message, the
// other parsers refuse the file and this one refuses theirs, 4000 single-byte and 4000 four-byte overwrites per file
// were each either refused with a message or parsed to in-bounds fields; and the capacity bound holds: over
// adversarial segments (every sample an escape with three nibbles, under tables whose coded symbols have frequency
// 1; also mixed and all-cheap segments) of 1..65536 samples the coder never writes more than n + 2 words, which is
// within the n + RES_SEG_SLACK words the file allows, and each such segment decodes back to its symbols consuming
// exactly its words and ending at the state 2^31.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "container.h"
#include "rans.h"

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
static const int SLACK = 4;  // residual_seg.h RES_SEG_SLACK (that header needs no HIP, but keep this program to two)

// ------------------------------------------------------------------------------------ the capacity bound
// tables in the file's form: context 0 has m = 0 (symbols 0 and the escape), the escape with frequency 1;
// context 1 has m = 63 with the escape and both outermost symbols at frequency 1
static CdfTables adversarial_tables() {
  CdfTables t;
  t.n = 2;
  t.stride = 129;
  t.cdf.assign(2 * 129, 0);
  t.length = {3, 129};
  t.offset = {0, -63};
  int32_t* a = t.cdf.data();
  a[1] = 65535;
  a[2] = 65536;
  int32_t* b = t.cdf.data() + 129;
  // 128 symbols: index 0 and 126 (q = -63, 63) and 127 (the escape) have frequency 1, index 63 takes the rest
  int32_t c = 0;
  for (int j = 0; j < 128; ++j) {
    b[j] = c;
    c += (j == 63) ? 65536 - 127 : 1;
  }
  b[128] = 65536;
  t.prepare();
  return t;
}

static bool bound_holds(const CdfTables& t, const std::vector<int32_t>& sym, const std::vector<int32_t>& ctx, const char* what) {
  const int64_t n = (int64_t)sym.size();
  const std::string s = rans_encode(sym.data(), ctx.data(), n, t);
  const int64_t words = (int64_t)s.size() / 4;
  if (s.size() % 4 || words < 2 || words > n + 2 || words > n + SLACK) {
    std::printf("%s: %lld samples took %lld words\n", what, (long long)n, (long long)words);
    return false;
  }
  RansDecoderState d;
  d.set_max_bypass(3);
  d.set_stream(reinterpret_cast<const uint8_t*>(s.data()), s.size());
  std::vector<int32_t> back((size_t)n);
  if (!d.decode(ctx.data(), n, t, back.data()) || back != sym) return std::printf("%s: decode differs\n", what), false;
  const RansDecoderState::Mark mk = d.mark();
  if (mk.pos != (size_t)words || mk.state != (1ull << 31)) {
    std::printf("%s: %zu of %lld words consumed, state %llx\n", what, mk.pos, (long long)words, (unsigned long long)mk.state);
    return false;
  }
  return true;
}

static bool capacity_ok() {
  const CdfTables t = adversarial_tables();
  const int64_t sizes[] = {1, 2, 3, 7, 255, 256, 257, 4096, 65535, 65536};
  for (int64_t n : sizes) {
    std::vector<int32_t> sym((size_t)n), ctx((size_t)n);
    // every sample the costliest escape: q = -255 in the m = 0 context (raw 509, three nibbles, symbol frequency 1)
    for (int64_t i = 0; i < n; ++i) sym[i] = -255, ctx[i] = 0;
    if (!bound_holds(t, sym, ctx, "all -255 escapes, m = 0")) return false;
    for (int64_t i = 0; i < n; ++i) sym[i] = 255, ctx[i] = 0;  // raw 508
    if (!bound_holds(t, sym, ctx, "all +255 escapes, m = 0")) return false;
    for (int64_t i = 0; i < n; ++i) sym[i] = (i & 1) ? -255 : 255, ctx[i] = 1;  // raw 383 / 382 under m = 63
    if (!bound_holds(t, sym, ctx, "all escapes, m = 63")) return false;
    for (int64_t i = 0; i < n; ++i) sym[i] = (i & 1) ? -63 : 63, ctx[i] = 1;  // frequency-1 symbols, no escape
    if (!bound_holds(t, sym, ctx, "frequency-1 symbols")) return false;
    for (int64_t i = 0; i < n; ++i) sym[i] = 0, ctx[i] = (int32_t)(i & 1);  // the cheapest symbols
    if (!bound_holds(t, sym, ctx, "cheapest symbols")) return false;
    for (int rep = 0; rep < 4; ++rep) {
      for (int64_t i = 0; i < n; ++i) {
        ctx[i] = (int32_t)(rnd() & 1);
        const uint32_t r = rnd() % 8;
        sym[i] = r < 5 ? (int32_t)(rnd() % 511) - 255 : r == 5 ? 0 : (rnd() & 1 ? -255 : 255);
      }
      if (!bound_holds(t, sym, ctx, "mixed")) return false;
    }
  }
  return true;
}

// ------------------------------------------------------------------------------------------ the container
struct Made {
  std::vector<uint8_t> file, inner, segs;
  std::vector<uint32_t> seg_bytes;
  uint8_t m[24];
  std::vector<uint16_t> freq;
  uint32_t H, W, seg_len, n_seg;
  bool vbr;
};

static bool make(uint32_t H, uint32_t W, uint32_t seg_len, bool vbr, Made* out) {
  Made& f = *out;
  f.H = H, f.W = W, f.seg_len = seg_len, f.vbr = vbr;
  f.n_seg = (uint32_t)((3ull * H * W + seg_len - 1) / seg_len);
  f.freq.assign(24 * 128, 0);
  for (int k = 0; k < 24; ++k) {
    f.m[k] = k % 5 == 4 ? RESIDUAL_ABSENT : (uint8_t)(k % 3 == 0 ? 0 : k);
    if (f.m[k] == RESIDUAL_ABSENT) continue;
    const int cnt = 2 * f.m[k] + 2;
    for (int j = 0; j < cnt; ++j) f.freq[k * 128 + j] = 1;
    f.freq[k * 128 + f.m[k]] = (uint16_t)(65536 - (cnt - 1));
  }
  const uint8_t y[5] = {1, 2, 3, 4, 5}, z[3] = {9, 8, 7};
  size_t len = 0;
  const uint32_t hz = (H + 63) / 64, wz = (W + 63) / 64;
  if (container_write(H, W, vbr ? 3 : -1, hz, wz, y, 5, z, 3, nullptr, 0, &len)) return false;
  f.inner.resize(len);
  if (container_write(H, W, vbr ? 3 : -1, hz, wz, y, 5, z, 3, f.inner.data(), len, &len)) return false;
  f.seg_bytes.resize(f.n_seg);
  f.segs.clear();
  for (uint32_t k = 0; k < f.n_seg; ++k) {
    const uint64_t left = 3ull * H * W - (uint64_t)k * seg_len;
    const uint64_t n = left < seg_len ? left : seg_len;
    f.seg_bytes[k] = 8 + 4 * (uint32_t)(rnd() % (n / 8 + 1));
    for (uint32_t j = 0; j < f.seg_bytes[k]; ++j) f.segs.push_back((uint8_t)rnd());
  }
  if (const char* e = container_write_residual_seg(H, W, vbr, 3, 0x0123456789abcdefull, f.m, f.freq.data(), seg_len,
                                                   f.n_seg, f.seg_bytes.data(), f.inner.data(), f.inner.size(),
                                                   f.segs.data(), f.segs.size(), nullptr, 0, &len))
    return std::printf("size query: %s\n", e), false;
  f.file.assign(len, 0xEE);
  if (const char* e = container_write_residual_seg(H, W, vbr, 3, 0x0123456789abcdefull, f.m, f.freq.data(), seg_len,
                                                   f.n_seg, f.seg_bytes.data(), f.inner.data(), f.inner.size(),
                                                   f.segs.data(), f.segs.size(), f.file.data(), len, &len))
    return std::printf("write: %s\n", e), false;
  return len == f.file.size();
}

// parse a copy that owns exactly n bytes; false on a contract violation
static bool probe(const std::vector<uint8_t>& file, size_t n, const char** err_out = nullptr, ResidualSegInfo* info = nullptr,
                  uint64_t max_pixels = MAXPIX) {
  std::unique_ptr<uint8_t[]> buf(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(buf.get(), file.data(), n);
  ResidualSegInfo s;
  std::memset(&s, 0xee, sizeof s);
  const char* err = container_parse_residual_seg(n ? buf.get() : nullptr, n, NLEV, max_pixels, &s);
  if (err_out) *err_out = err;
  if (err) {
    ++refused;
    if (!*err) return std::printf("refusal without a message\n"), false;
    return true;
  }
  ++accepted;
  if (info) *info = s;
  const uint64_t N = 3ull * s.H * s.W;
  bool ok = s.H > 0 && s.W > 0 && (uint64_t)s.H * s.W <= max_pixels && s.tau <= 127 && s.seg_len >= 256 &&
            s.seg_len <= 65536 && (uint64_t)s.n_seg == (N + s.seg_len - 1) / s.seg_len && s.inner_off <= n &&
            s.inner_len >= 1 && s.inner_len <= n - s.inner_off && s.res_off == s.inner_off + s.inner_len + 4 &&
            s.index_off == s.res_off && s.res_len <= n - s.res_off && s.res_off + s.res_len == n &&
            s.data_off == s.index_off + 4 * (size_t)s.n_seg && s.data_off + s.data_len == n && s.inner.H == s.H &&
            s.inner.W == s.W;
  uint64_t sum = 0;
  for (uint32_t k = 0; ok && k < s.n_seg; ++k) {
    const uint8_t* p = buf.get() + s.index_off + 4 * (size_t)k;
    const uint32_t v = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
    const uint64_t left = N - (uint64_t)k * s.seg_len, cnt = left < s.seg_len ? left : s.seg_len;
    ok = v % 4 == 0 && v >= 8 && v <= 4 * (cnt + SLACK);
    sum += v;
  }
  ok = ok && sum == s.data_len;
  for (uint32_t k = 0; ok && k < RESIDUAL_CTX; ++k) {
    if (s.m[k] == RESIDUAL_ABSENT) continue;
    const size_t cnt = 2 * (size_t)s.m[k] + 2;
    ok = s.m[k] <= RESIDUAL_MAX_M && s.freq_off[k] + 2 * cnt <= s.inner_off;
  }
  if (!ok) std::printf("accepted a file with out-of-contract fields\n");
  return ok;
}

static bool expect(const std::vector<uint8_t>& file, const char* word, uint64_t max_pixels = MAXPIX) {
  const char* err = nullptr;
  if (!probe(file, file.size(), &err, nullptr, max_pixels)) return false;
  if (!err || !std::strstr(err, word)) {
    std::printf("expected a refusal with \"%s\", got %s\n", word, err ? err : "acceptance");
    return false;
  }
  return true;
}

static std::vector<uint8_t> with32(std::vector<uint8_t> f, size_t at, uint32_t v) {
  f[at] = (uint8_t)(v >> 24), f[at + 1] = (uint8_t)(v >> 16), f[at + 2] = (uint8_t)(v >> 8), f[at + 3] = (uint8_t)v;
  return f;
}

static bool container_ok() {
  const struct {
    uint32_t H, W, L;
    bool vbr;
  } shapes[] = {{1, 1, 256, false}, {17, 23, 256, true}, {64, 96, 257, false}, {40, 50, 4096, true}, {30, 30, 65536, false}};
  for (const auto& sh : shapes) {
    Made f;
    if (!make(sh.H, sh.W, sh.L, sh.vbr, &f)) return false;
    ResidualSegInfo s;
    const char* err = nullptr;
    if (!probe(f.file, f.file.size(), &err, &s) || err) return std::printf("round trip refused: %s\n", err ? err : "?"), false;
    bool same = s.H == f.H && s.W == f.W && s.tau == 3 && s.vbr == f.vbr && s.digest == 0x0123456789abcdefull &&
                s.seg_len == f.seg_len && s.n_seg == f.n_seg && s.inner_len == f.inner.size() &&
                s.data_len == f.segs.size() && !std::memcmp(s.m, f.m, 24) &&
                !std::memcmp(f.file.data() + s.inner_off, f.inner.data(), f.inner.size()) &&
                !std::memcmp(f.file.data() + s.data_off, f.segs.data(), f.segs.size()) &&
                s.inner.level == (f.vbr ? 3 : -1) && is_residual_seg_file(f.file.data(), f.file.size()) &&
                !is_residual_file(f.file.data(), f.file.size());
    for (uint32_t k = 0; same && k < f.n_seg; ++k) {
      const uint8_t* p = f.file.data() + s.index_off + 4 * (size_t)k;
      same = ((((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3])) == f.seg_bytes[k];
    }
    if (!same) return std::printf("round trip differs\n"), false;
    for (size_t n = 0; n < f.file.size(); ++n) {  // every truncation
      if (!probe(f.file, n, &err)) return false;
      if (!err) return std::printf("a truncation to %zu bytes was accepted\n", n), false;
    }
    // the other parsers refuse it, and this one theirs
    ContainerInfo ci;
    TiledInfo ti;
    ScaledInfo si;
    LayeredInfo li;
    ResidualInfo r1;
    const uint8_t* d = f.file.data();
    const size_t n = f.file.size();
    if (!container_parse(d, n, false, NLEV, MAXPIX, &ci) || !container_parse(d, n, true, NLEV, MAXPIX, &ci) ||
        !container_parse_tiled(d, n, MAXPIX, &ti) || !container_parse_scaled(d, n, NLEV, MAXPIX, &si) ||
        !container_parse_layered(d, n, NLEV, MAXPIX, false, &li) || !container_parse_layered(d, n, NLEV, MAXPIX, true, &li) ||
        !container_parse_residual(d, n, NLEV, MAXPIX, &r1))
      return std::printf("another parser accepted an MLR2 file\n"), false;
    std::vector<uint8_t> as1 = f.file;
    as1[3] = '1';
    if (!expect(as1, "bad magic") || !expect(f.inner, "bad magic")) return false;
    // each refusal by its message
    const size_t seg_at = s.inner_off - 12, res_at = s.res_off - 4, idx = s.index_off;
    std::vector<uint8_t> g = f.file;
    g[4] = 1;
    if (!expect(g, "unknown version")) return false;
    g = f.file, g[5] = 2;
    if (!expect(g, "unknown flags")) return false;
    g = f.file, g[6] = 128;
    if (!expect(g, "tau above 127")) return false;
    g = f.file, g[7] = 23;
    if (!expect(g, "n_ctx is not 24")) return false;
    if (!expect(with32(f.file, 8, 0), "H or W is zero")) return false;
    if (f.H * f.W > 1 && !expect(f.file, "exceeds max_pixels", (uint64_t)f.H * f.W - 1)) return false;
    g = f.file, g[24] = 64;
    if (!expect(g, "an m outside 0..63")) return false;
    g = f.file, g[25] = 0, g[26] = 0;
    if (!expect(g, "a zero frequency")) return false;
    g = f.file, g[26] ^= 1;
    if (!expect(g, "do not sum to 65536")) return false;
    if (!expect(with32(f.file, seg_at, 255), "seg_len outside 256..65536") ||
        !expect(with32(f.file, seg_at, 65537), "seg_len outside 256..65536") ||
        !expect(with32(f.file, seg_at + 4, f.n_seg + 1), "n_seg is not ceil") ||
        !expect(with32(f.file, seg_at + 8, 0), "an empty inner file") ||
        !expect(with32(f.file, seg_at + 8, (uint32_t)n), "the inner length runs past the end") ||
        !expect(with32(f.file, res_at, (uint32_t)s.res_len + 4), "the residual length runs past the end") ||
        !expect(with32(f.file, idx, f.seg_bytes[0] + 2), "not a multiple of 4") ||
        !expect(with32(f.file, idx, 4), "a segment length below 8") ||
        !expect(with32(f.file, idx, 4 * (65536 + SLACK) + 4), "above the capacity bound") ||
        !expect(with32(f.file, idx, f.seg_bytes[0] + 4), "not 4 n_seg + the segment lengths"))
      return false;
    g = f.file;
    g.push_back(0);
    if (!expect(g, "bytes left over")) return false;
    g = f.file, g[5] ^= 1;  // the flag no longer matches the inner file
    if (!expect(g, "container_parse")) return false;
    // seeded overwrites: refused with a message or parsed to in-bounds fields, never a read outside the block
    for (int it = 0; it < 4000; ++it) {
      g = f.file;
      g[rnd() % g.size()] = (uint8_t)rnd();
      if (!probe(g, g.size())) return false;
      g = f.file;
      const size_t at = rnd() % (g.size() - 3);
      const uint32_t v = (rnd() & 3) ? rnd() % 70000 : rnd();
      if (!probe(with32(g, at, v), g.size())) return false;
    }
    // the writer's refusals
    size_t len = 0;
    std::vector<uint32_t> sb = f.seg_bytes;
    std::vector<uint8_t> out(f.file.size());
    auto wr = [&](uint32_t L, uint32_t ns, const std::vector<uint32_t>& b, size_t segs_len) {
      return container_write_residual_seg(f.H, f.W, f.vbr, 3, 1, f.m, f.freq.data(), L, ns, b.data(), f.inner.data(),
                                          f.inner.size(), f.segs.data(), segs_len, out.data(), out.size(), &len);
    };
    const char* e = wr(255, f.n_seg, sb, f.segs.size());
    if (!e || !std::strstr(e, "seg_len outside")) return std::printf("writer: seg_len\n"), false;
    e = wr(f.seg_len, f.n_seg + 1, sb, f.segs.size());
    if (!e || !std::strstr(e, "n_seg is not ceil")) return std::printf("writer: n_seg\n"), false;
    sb[0] += 2;
    e = wr(f.seg_len, f.n_seg, sb, f.segs.size());
    if (!e || !std::strstr(e, "not a multiple of 4")) return std::printf("writer: multiple\n"), false;
    sb[0] = 4;
    e = wr(f.seg_len, f.n_seg, sb, f.segs.size());
    if (!e || !std::strstr(e, "below 8")) return std::printf("writer: below 8\n"), false;
    sb[0] = 4 * (65536 + SLACK) + 4;
    e = wr(f.seg_len, f.n_seg, sb, f.segs.size());
    if (!e || !std::strstr(e, "above the capacity bound")) return std::printf("writer: bound\n"), false;
    sb = f.seg_bytes;
    e = wr(f.seg_len, f.n_seg, sb, f.segs.size() - 4);
    if (!e || !std::strstr(e, "do not sum")) return std::printf("writer: sum\n"), false;
  }
  return true;
}

int main() {
  if (!capacity_ok()) return 1;
  if (!container_ok()) return 1;
  std::printf("%ld refused, %ld accepted\ncontainer_residual_seg_check ok\n", refused, accepted);
  return 0;
}
