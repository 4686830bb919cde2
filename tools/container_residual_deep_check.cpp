// Host sanitizer check of the deep residual layer's host code: the integer definitions of
// mlic_amd/csrc/residual16.h and the "MLR3" container (mlic_amd/csrc/container.cpp: container_write_residual_deep /
// container_parse_residual_deep).  Every parsed input sits in a heap block of exactly its size, so AddressSanitizer
// sees any read outside [data, data + n).  Build and run from the repository root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       -Imlic_amd/csrc tools/container_residual_deep_check.cpp mlic_amd/csrc/container.cpp mlic_amd/csrc/rans.cpp \
//       -o /tmp/container_residual_deep_check && /tmp/container_residual_deep_check
//
// Exit status 0 and a final "container_residual_deep_check ok" line mean: the multiply-shift division equals the true
// division for every n in 0..2^16+126 and every step 1, 3, .., 255; for every depth 9..16, a sweep of (x, base, tau)
// keeps |x - rec| <= tau and rec = x at tau 0; split then join is the identity for every q in +-maxv and every shift,
// lo is in 0..2^s-1 and |hi| <= 255 exactly when the fit condition holds; the shift rule gives its hand-computed
// cases; files round-trip (every field, the plane's bytes), every truncation at every byte is refused, every listed
// refusal gives its own message, the other parsers refuse the file, and every single-byte corruption of the header
// (all 256 values of each byte up to the first table) and 4000 seeded overwrites per file are each either refused
// with a message or parsed to in-bounds fields.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "container.h"
#include "residual16.h"

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

// ------------------------------------------------------------------------------------------ the integers
static bool division_ok() {
  for (int tau = 0; tau <= RES_MAX_TAU; ++tau) {
    const int step = 2 * tau + 1;
    const uint32_t magic = residual16_magic(step);
    for (uint32_t n = 0; n <= 65535u + 127u; ++n)
      if (residual16_div(n, magic) != n / (uint32_t)step) return std::printf("division: n %u step %d\n", n, step), false;
  }
  return true;
}

static bool one_bound(int x, int base, int tau, int depth) {
  const int maxv = (1 << depth) - 1;
  const int q = residual16_quant(x, base, tau, residual16_magic(2 * tau + 1));
  const int rec = residual16_rec(base, q, tau, maxv);
  const int e = x > rec ? x - rec : rec - x, aq = q < 0 ? -q : q;
  if (e > tau || aq > maxv || (tau == 0 && rec != x)) {
    std::printf("bound: x %d base %d tau %d depth %d: q %d rec %d\n", x, base, tau, depth, q, rec);
    return false;
  }
  return true;
}

static bool bound_ok() {
  const int taus[] = {0, 1, 2, 3, 63, 126, 127};
  for (int depth = RES16_MIN_DEPTH; depth <= RES16_MAX_DEPTH; ++depth) {
    const int maxv = (1 << depth) - 1;
    for (int tau : taus) {
      const int step = 2 * tau + 1;
      const int edge[] = {0, 1, tau, step, maxv / 2, maxv - 1, maxv};
      for (int x : edge)
        for (int b : edge)
          if (!one_bound(x, b, tau, depth)) return false;
      for (int it = 0; it < 20000; ++it)
        if (!one_bound((int)(rnd() % (uint32_t)(maxv + 1)), (int)(rnd() % (uint32_t)(maxv + 1)), tau, depth)) return false;
    }
  }
  for (int x = 0; x < 512; ++x)  // depth 9, exhaustively
    for (int b = 0; b < 512; ++b)
      for (int tau : {0, 1, 2, 127})
        if (!one_bound(x, b, tau, 9)) return false;
  return true;
}

static bool split_ok() {
  for (int depth = RES16_MIN_DEPTH; depth <= RES16_MAX_DEPTH; ++depth) {
    const int maxv = (1 << depth) - 1;
    for (int s = 0; s <= residual16_max_shift(depth); ++s) {
      for (int q = -maxv; q <= maxv; ++q) {
        const int hi = residual16_hi(q, s), lo = residual16_lo(q, s);
        if (lo < 0 || lo >= (1 << s) || residual16_join(hi, lo, s) != q)
          return std::printf("split: q %d s %d: hi %d lo %d\n", q, s, hi, lo), false;
      }
      // |hi| <= 255 for every |q| <= M exactly when M fits: the worst is hi of -M
      for (int M = 0; M <= maxv; ++M) {
        const int h = residual16_hi(-M, s), h2 = residual16_hi(M, s);
        const bool within = -h <= RES16_MAX_HI && h2 <= RES16_MAX_HI;
        if (within != residual16_fits((uint32_t)M, s)) return std::printf("fit: M %d s %d\n", M, s), false;
      }
    }
    if (!residual16_fits((uint32_t)maxv, residual16_max_shift(depth))) return std::printf("d - 7 does not fit\n"), false;
  }
  return true;
}

static bool shift_ok() {
  const uint64_t N = 3 * 100 * 100;
  const struct {
    int depth;
    uint64_t N;
    uint32_t mq;
    uint64_t sq;
    int want;
  } cases[] = {
      {10, N, 0, 0, 0},                   // a perfect base
      {10, N, 255, 8 * N, 0},             // both conditions met with equality at s = 0
      {10, N, 256, 8 * N, 1},             // (256 + 1) >> 1 = 128 fits at 1
      {10, N, 255, 8 * N + 1, 1},         // the sum pushes it to 1
      {12, N, 4095, 40 * N, 5},           // fit: (4095 + 31) >> 5 = 128; the sum allows s >= 3
      {16, N, 65535, 600 * N, 9},         // only d - 7 fits the largest q
      {16, N, 2000, 600 * N, 7},          // fit from 3, the sum from 7 (8 * 128 = 1024 >= 600)
      {16, N, 100, 16385 * N, 9},         // nothing meets the sum condition (8 * 512 = 4096): d - 7
      {9, N, 511, 511 * N, 2},            // d - 7 = 2: nothing meets the sum (8 * 4 = 32), so d - 7
      {16, 3ull << 32, 65535, 3ull << 40, 9},
  };
  for (const auto& c : cases) {
    const int s = residual16_shift(c.depth, c.N, c.mq, c.sq);
    if (s != c.want)
      return std::printf("shift: depth %d mq %u sq %llu: %d, expected %d\n", c.depth, c.mq, (unsigned long long)c.sq, s, c.want), false;
  }
  return true;
}

// ------------------------------------------------------------------------------------------ the container
struct Made {
  std::vector<uint8_t> file, inner, segs, lo;
  std::vector<uint32_t> seg_bytes;
  uint8_t m[24];
  std::vector<uint16_t> freq;
  uint32_t H, W, seg_len, n_seg, depth, shift;
  bool vbr;
};

static const char* write(const Made& f, uint32_t depth, uint32_t shift, size_t lo_len, uint8_t* out, size_t cap, size_t* len) {
  return container_write_residual_deep(f.H, f.W, f.vbr, 3, depth, shift, 0x0123456789abcdefull, f.m, f.freq.data(),
                                       f.seg_len, f.n_seg, f.seg_bytes.data(), f.inner.data(), f.inner.size(),
                                       f.segs.data(), f.segs.size(), f.lo.data(), lo_len, out, cap, len);
}

static bool make(uint32_t H, uint32_t W, uint32_t seg_len, bool vbr, uint32_t depth, uint32_t shift, Made* out) {
  Made& f = *out;
  f.H = H, f.W = W, f.seg_len = seg_len, f.vbr = vbr, f.depth = depth, f.shift = shift;
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
  f.lo.assign((size_t)(8 * residual16_plane_words(H, W, (int)shift)), 0);
  for (auto& b : f.lo) b = (uint8_t)rnd();
  f.lo.push_back(0);  // data() of an empty plane stays a valid pointer
  const size_t lo_len = f.lo.size() - 1;
  if (const char* e = write(f, depth, shift, lo_len, nullptr, 0, &len)) return std::printf("size query: %s\n", e), false;
  f.file.assign(len, 0xEE);
  if (const char* e = write(f, depth, shift, lo_len, f.file.data(), len, &len)) return std::printf("write: %s\n", e), false;
  return len == f.file.size();
}

// parse a copy that owns exactly n bytes; false on a contract violation
static bool probe(const std::vector<uint8_t>& file, size_t n, const char** err_out = nullptr, ResidualDeepInfo* info = nullptr,
                  uint64_t max_pixels = MAXPIX) {
  std::unique_ptr<uint8_t[]> buf(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(buf.get(), file.data(), n);
  ResidualDeepInfo d;
  std::memset(&d, 0xee, sizeof d);
  const char* err = container_parse_residual_deep(n ? buf.get() : nullptr, n, NLEV, max_pixels, &d);
  if (err_out) *err_out = err;
  if (err) {
    ++refused;
    if (!*err) return std::printf("refusal without a message\n"), false;
    return true;
  }
  ++accepted;
  if (info) *info = d;
  const ResidualSegInfo& s = d.seg;
  const uint64_t N = 3ull * s.H * s.W;
  bool ok = s.H > 0 && s.W > 0 && (uint64_t)s.H * s.W <= max_pixels && s.tau <= 127 && s.seg_len >= 256 &&
            s.seg_len <= 65536 && (uint64_t)s.n_seg == (N + s.seg_len - 1) / s.seg_len && s.inner_off <= n &&
            s.inner_len >= 1 && s.inner_len <= n - s.inner_off && s.res_off == s.inner_off + s.inner_len + 4 &&
            s.index_off == s.res_off && s.res_len <= n - s.res_off && s.data_off == s.index_off + 4 * (size_t)s.n_seg &&
            s.data_off + s.data_len == s.res_off + s.res_len && s.inner.H == s.H && s.inner.W == s.W &&
            d.depth >= 9 && d.depth <= 16 && d.shift <= d.depth - 7 && d.lo_off == s.data_off + s.data_len + 4 &&
            d.lo_len == 8 * residual16_plane_words(s.H, s.W, (int)d.shift) && d.lo_off + d.lo_len == n;
  if (!ok) std::printf("accepted a file with out-of-contract fields\n");
  return ok;
}

static bool expect(const std::vector<uint8_t>& file, const char* word, uint64_t max_pixels = MAXPIX) {
  const char* err = nullptr;
  if (!probe(file, file.size(), &err, nullptr, max_pixels)) return false;
  if (!err || !std::strstr(err, word) || !std::strstr(err, "container_parse")) {
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
    uint32_t H, W, L, depth, shift;
    bool vbr;
  } shapes[] = {{1, 1, 256, 9, 0, false}, {17, 23, 256, 10, 3, true}, {5, 130, 257, 16, 9, false}, {40, 64, 4096, 12, 1, true}};
  for (const auto& sh : shapes) {
    Made f;
    if (!make(sh.H, sh.W, sh.L, sh.vbr, sh.depth, sh.shift, &f)) return false;
    ResidualDeepInfo d;
    const char* err = nullptr;
    if (!probe(f.file, f.file.size(), &err, &d) || err) return std::printf("round trip refused: %s\n", err ? err : "?"), false;
    const ResidualSegInfo& s = d.seg;
    const size_t lo_len = f.lo.size() - 1;
    const bool same = s.H == f.H && s.W == f.W && s.tau == 3 && s.vbr == f.vbr && s.digest == 0x0123456789abcdefull &&
                      s.seg_len == f.seg_len && s.n_seg == f.n_seg && s.inner_len == f.inner.size() &&
                      s.data_len == f.segs.size() && !std::memcmp(s.m, f.m, 24) && d.depth == f.depth &&
                      d.shift == f.shift && d.lo_len == lo_len &&
                      !std::memcmp(f.file.data() + s.inner_off, f.inner.data(), f.inner.size()) &&
                      !std::memcmp(f.file.data() + s.data_off, f.segs.data(), f.segs.size()) &&
                      (lo_len == 0 || !std::memcmp(f.file.data() + d.lo_off, f.lo.data(), lo_len)) &&
                      is_residual_deep_file(f.file.data(), f.file.size()) &&
                      !is_residual_seg_file(f.file.data(), f.file.size()) && !is_residual_file(f.file.data(), f.file.size());
    if (!same) return std::printf("round trip differs\n"), false;
    for (size_t n = 0; n < f.file.size(); ++n) {  // every truncation, at every byte
      if (!probe(f.file, n, &err)) return false;
      if (!err) return std::printf("a truncation to %zu bytes was accepted\n", n), false;
    }
    // the other parsers refuse it, and this one theirs
    ContainerInfo ci;
    TiledInfo ti;
    ScaledInfo si;
    LayeredInfo li;
    ResidualInfo r1;
    ResidualSegInfo r2;
    const uint8_t* p = f.file.data();
    const size_t n = f.file.size();
    if (!container_parse(p, n, false, NLEV, MAXPIX, &ci) || !container_parse(p, n, true, NLEV, MAXPIX, &ci) ||
        !container_parse_tiled(p, n, MAXPIX, &ti) || !container_parse_scaled(p, n, NLEV, MAXPIX, &si) ||
        !container_parse_layered(p, n, NLEV, MAXPIX, false, &li) || !container_parse_layered(p, n, NLEV, MAXPIX, true, &li) ||
        !container_parse_residual(p, n, NLEV, MAXPIX, &r1) || !container_parse_residual_seg(p, n, NLEV, MAXPIX, &r2))
      return std::printf("another parser accepted an MLR3 file\n"), false;
    std::vector<uint8_t> g = f.file;
    g[3] = '2';
    if (!expect(g, "bad magic") || !expect(f.inner, "bad magic")) return false;
    // each refusal by its message
    const size_t ds_at = s.inner_off - 14, seg_at = s.inner_off - 12, res_at = s.res_off - 4, idx = s.index_off;
    const size_t lo_at = d.lo_off - 4;
    g = f.file, g[4] = 1;
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
    g = f.file, g[ds_at] = 8;
    if (!expect(g, "depth outside 9..16")) return false;
    g = f.file, g[ds_at] = 17;
    if (!expect(g, "depth outside 9..16")) return false;
    g = f.file, g[ds_at + 1] = (uint8_t)(f.depth - 6);
    if (!expect(g, "shift outside 0..depth - 7")) return false;
    if (f.shift != 1) {
      g = f.file, g[ds_at + 1] = 1;  // a legal shift that no longer matches the plane
      if (!expect(g, "lo_len is not")) return false;
    }
    if (!expect(with32(f.file, seg_at, 255), "seg_len outside 256..65536") ||
        !expect(with32(f.file, seg_at + 4, f.n_seg + 1), "n_seg is not ceil") ||
        !expect(with32(f.file, seg_at + 8, 0), "an empty inner file") ||
        !expect(with32(f.file, seg_at + 8, (uint32_t)n), "the inner length runs past the end") ||
        !expect(with32(f.file, res_at, (uint32_t)n), "the residual length runs past the end") ||
        !expect(with32(f.file, idx, f.seg_bytes[0] + 2), "not a multiple of 4") ||
        !expect(with32(f.file, idx, 4), "a segment length below 8") ||
        !expect(with32(f.file, idx, 4 * (65536 + RESIDUAL_SEG_SLACK) + 4), "above the capacity bound") ||
        !expect(with32(f.file, idx, f.seg_bytes[0] + 4), "not 4 n_seg + the segment lengths") ||
        !expect(with32(f.file, lo_at, (uint32_t)lo_len + 8), "lo_len is not"))
      return false;
    g = f.file;
    g.push_back(0);
    if (!expect(g, "bytes left over after the low-bit plane")) return false;
    if (lo_len) {
      g = f.file;
      g.pop_back();
      if (!expect(g, "truncated inside the low-bit plane")) return false;
    }
    g = f.file;
    g.resize(lo_at + 2);
    if (!expect(g, "truncated before the low-bit plane's length")) return false;
    g = f.file, g[5] ^= 1;  // the flag no longer matches the inner file
    if (!expect(g, "container_parse")) return false;
    // every single-byte corruption of the header, then seeded overwrites anywhere
    for (size_t at = 0; at < RESIDUAL_HEADER + 1; ++at)
      for (int v = 0; v < 256; ++v) {
        g = f.file, g[at] = (uint8_t)v;
        if (!probe(g, g.size())) return false;
      }
    for (size_t at = ds_at; at < ds_at + 14; ++at)  // depth, shift, seg_len, n_seg, inner_len
      for (int v = 0; v < 256; ++v) {
        g = f.file, g[at] = (uint8_t)v;
        if (!probe(g, g.size())) return false;
      }
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
    std::vector<uint8_t> out(f.file.size() + 64);
    const char* e = write(f, 8, 0, lo_len, out.data(), out.size(), &len);
    if (!e || !std::strstr(e, "depth outside 9..16")) return std::printf("writer: depth\n"), false;
    e = write(f, f.depth, f.depth - 6, lo_len, out.data(), out.size(), &len);
    if (!e || !std::strstr(e, "shift outside")) return std::printf("writer: shift\n"), false;
    e = write(f, f.depth, f.shift, lo_len + 8, out.data(), out.size(), &len);
    if (!e || !std::strstr(e, "lo_len is not") || !std::strstr(e, "container_write_residual_deep"))
      return std::printf("writer: lo_len\n"), false;
  }
  return true;
}

int main() {
  if (!division_ok() || !bound_ok() || !split_ok() || !shift_ok()) return 1;
  if (!container_ok()) return 1;
  std::printf("%ld refused, %ld accepted\ncontainer_residual_deep_check ok\n", refused, accepted);
  return 0;
}
