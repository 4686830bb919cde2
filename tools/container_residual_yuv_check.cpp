// Host sanitizer check of the Y'CbCr residual layer's host code: the integer definitions of
// mlic_amd/csrc/residual_yuv.h, the "MLR4" container (mlic_amd/csrc/container.cpp: container_write_residual_yuv /
// container_parse_residual_yuv) and the host segment coders for a given N (mlic_amd/csrc/residual_seg.cpp).  Every
// parsed input sits in a heap block of exactly its size, so AddressSanitizer sees any read outside [data, data + n).
// Build and run from the repository root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan \
//       -Imlic_amd/csrc tools/container_residual_yuv_check.cpp mlic_amd/csrc/container.cpp mlic_amd/csrc/rans.cpp \
//       mlic_amd/csrc/residual_seg.cpp -o /tmp/container_residual_yuv_check && /tmp/container_residual_yuv_check
//
// Exit status 0 and a final "container_residual_yuv_check ok" line mean: the frame geometry (N, offsets, groups, plane
// words) equals a brute-force count for a sweep of sizes and the three subsamplings; the bound |x - rec| <= tau holds
// at depths 8, 10 and 16 with rec = x at tau 0 and the depth-8 values are residual.h's; files round-trip (every
// field, the plane's bytes), every truncation at every byte is refused, every listed refusal gives its own message,
// the other parsers refuse the file and this one theirs, 4000 seeded overwrites per file are each either refused
// with a message or parsed to in-bounds fields; and the _host_n coders round-trip all-escape segments at N = 3,
// 6 * 256 + 1 and a frame's N within the capacity bound, give the H, W entries' bytes at N = 3 H W, and refuse a
// flipped byte.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "container.h"
#include "residual_yuv.h"

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
static const int SUBS[3][2] = {{1, 1}, {2, 1}, {2, 2}};

// ------------------------------------------------------------------------------------------ the integers
static bool geometry_ok() {
  const int sizes[] = {1, 2, 3, 63, 64, 65, 127, 128, 129, 261, 514};
  for (const auto& sub : SUBS)
    for (int H : sizes)
      for (int W : sizes) {
        const ResYuvGeom g = residual_yuv_geom(H, W, sub[0], sub[1]);
        int64_t n = 0, groups = 0;
        for (int p = 0; p < 3; ++p) {
          int64_t h = 0, w = 0;
          for (int y = 0; y < H; y += p ? sub[1] : 1) ++h;  // a chroma row per sub_y luma rows, the last partial
          for (int x = 0; x < W; x += p ? sub[0] : 1) ++w;
          if (g.h[p] != h || g.w[p] != w || g.off[p] != n || g.rowbase[p] != groups)
            return std::printf("geometry: %d x %d sub %d %d plane %d\n", H, W, sub[0], sub[1], p), false;
          n += h * w;
          int64_t G = 0;
          for (int64_t x = 0; x < w; x += 64) ++G;
          if (g.G[p] != G) return std::printf("groups: %d x %d plane %d\n", H, W, p), false;
          groups += h * G;
        }
        if (g.N != n || g.groups != groups) return std::printf("N: %d x %d\n", H, W), false;
        for (int s = 0; s <= 9; ++s)
          if (residual_yuv_plane_words((uint64_t)H, (uint64_t)W, sub[0], sub[1], s) != (uint64_t)(groups * s))
            return std::printf("plane words: %d x %d s %d\n", H, W, s), false;
      }
  if (residual_yuv_max_shift(8) != 0 || residual_yuv_max_shift(9) != 2 || residual_yuv_max_shift(16) != 9) return false;
  if (!residual_yuv_sub_ok(1, 1) || !residual_yuv_sub_ok(2, 1) || !residual_yuv_sub_ok(2, 2) || residual_yuv_sub_ok(1, 2) ||
      residual_yuv_sub_ok(0, 1) || residual_yuv_sub_ok(3, 1))
    return std::printf("sub_ok\n"), false;
  if (residual_yuv_shift(8, 1000, 255, 100000) != 0) return std::printf("shift at depth 8\n"), false;
  if (residual_yuv_shift(10, 1000, 1023, 1000) != residual16_shift(10, 1000, 1023, 1000)) return false;
  return true;
}

static bool bound_ok() {
  const int depths[] = {8, 10, 16}, taus[] = {0, 1, 2, 127};
  for (int depth : depths) {
    const int maxv = (1 << depth) - 1;
    for (int tau : taus) {
      const uint32_t magic = residual16_magic(2 * tau + 1);
      for (int it = 0; it < 40000; ++it) {
        const int x = it < 8 ? (it & 1 ? maxv : 0) : (int)(rnd() % (uint32_t)(maxv + 1));
        const int b = it < 8 ? (it & 2 ? maxv : 0) : (int)(rnd() % (uint32_t)(maxv + 1));
        const int q = residual16_quant(x, b, tau, magic), rec = residual16_rec(b, q, tau, maxv);
        const int e = x > rec ? x - rec : rec - x;
        if (e > tau || (tau == 0 && rec != x)) return std::printf("bound: x %d base %d tau %d depth %d\n", x, b, tau, depth), false;
        if (depth == 8 && (q != residual_quant(x, b, tau) || rec != residual_rec(b, q, tau)))
          return std::printf("depth 8 differs from residual.h: x %d base %d tau %d\n", x, b, tau), false;
      }
    }
  }
  // a sample of a word: LSB-aligned words above maxv read as maxv, MSB-aligned words drop their low bits
  if (residual_yuv_sample(1023, 0, 1023) != 1023 || residual_yuv_sample(40000, 0, 1023) != 1023 ||
      residual_yuv_sample(0xFFC0, 6, 1023) != 1023 || residual_yuv_sample(0x0047, 6, 1023) != 1 ||
      residual_yuv_sample(200, 0, 255) != 200)
    return std::printf("sample of a word\n"), false;
  if (residual_yuv_context(2, 1023, 10) != 16 + 7 || residual_yuv_context(1, 3, 8) != 8 + 1) return false;
  return true;
}

// ------------------------------------------------------------------------------------------ the container
struct Made {
  std::vector<uint8_t> file, inner, segs, lo;
  std::vector<uint32_t> seg_bytes;
  uint8_t m[24];
  std::vector<uint16_t> freq;
  uint32_t H, W, seg_len, depth, shift, sub_x, sub_y, matrix, flags;
  bool vbr;
};

static bool make(uint32_t H, uint32_t W, uint32_t seg_len, bool vbr, uint32_t depth, uint32_t shift, uint32_t sub_x,
                 uint32_t sub_y, uint32_t matrix, uint32_t flags, Made* out) {
  Made& d = *out;
  d.H = H, d.W = W, d.seg_len = seg_len, d.vbr = vbr, d.depth = depth, d.shift = shift;
  d.sub_x = sub_x, d.sub_y = sub_y, d.matrix = matrix, d.flags = flags;
  const uint8_t y[3] = {1, 2, 3}, z[1] = {9};
  size_t len = 0;
  const uint32_t hz = (H + 63) / 64, wz = (W + 63) / 64;
  const int32_t level = vbr ? 2 : -1;
  if (container_write(H, W, level, hz, wz, y, 3, z, 1, nullptr, 0, &len)) return std::printf("inner size\n"), false;
  d.inner.assign(len, 0);
  if (container_write(H, W, level, hz, wz, y, 3, z, 1, d.inner.data(), len, &len)) return std::printf("inner\n"), false;
  d.freq.assign(24 * 128, 0);
  for (int k = 0; k < 24; ++k) {
    d.m[k] = k % 5 == 4 ? RESIDUAL_ABSENT : (uint8_t)(k % 4);
    if (d.m[k] == RESIDUAL_ABSENT) continue;
    const int cnt = 2 * d.m[k] + 2;
    for (int j = 0; j < cnt; ++j) d.freq[k * 128 + j] = 1;
    d.freq[k * 128] = (uint16_t)(65536 - (cnt - 1));
  }
  const ResYuvGeom g = residual_yuv_geom(H, W, (int)sub_x, (int)sub_y);
  const uint64_t n_seg = (uint64_t)residual_n_seg(g.N, (int)seg_len);
  d.seg_bytes.clear();
  d.segs.clear();
  for (uint64_t k = 0; k < n_seg; ++k) {
    const uint32_t v = 8 + 4 * (rnd() % 3);
    d.seg_bytes.push_back(v);
    for (uint32_t i = 0; i < v; ++i) d.segs.push_back((uint8_t)rnd());
  }
  d.lo.assign((size_t)(8 * g.groups * shift), 0);
  for (auto& v : d.lo) v = (uint8_t)rnd();
  const char* err = container_write_residual_yuv(H, W, vbr, 5, depth, shift, sub_x, sub_y, matrix, flags,
                                                 0x0123456789abcdefull, d.m, d.freq.data(), seg_len, (uint32_t)n_seg,
                                                 d.seg_bytes.data(), d.inner.data(), d.inner.size(), d.segs.data(),
                                                 d.segs.size(), d.lo.data(), d.lo.size(), nullptr, 0, &len);
  if (err) return std::printf("size query: %s\n", err), false;
  d.file.assign(len, 0);
  err = container_write_residual_yuv(H, W, vbr, 5, depth, shift, sub_x, sub_y, matrix, flags, 0x0123456789abcdefull, d.m,
                                     d.freq.data(), seg_len, (uint32_t)n_seg, d.seg_bytes.data(), d.inner.data(),
                                     d.inner.size(), d.segs.data(), d.segs.size(), d.lo.data(), d.lo.size(),
                                     d.file.data(), len, &len);
  if (err || len != d.file.size()) return std::printf("write: %s\n", err ? err : "length"), false;
  return true;
}

// parse the first n bytes of `file` from a heap block of exactly n bytes
static bool probe(const std::vector<uint8_t>& file, size_t n, const char** err_out = nullptr,
                  ResidualYuvInfo* info = nullptr, uint64_t max_pixels = MAXPIX) {
  std::unique_ptr<uint8_t[]> block(new uint8_t[n ? n : 1]);
  if (n) std::memcpy(block.get(), file.data(), n);
  ResidualYuvInfo y;
  const char* err = container_parse_residual_yuv(block.get(), n, NLEV, max_pixels, &y);
  if (err_out) *err_out = err;
  if (err) {
    ++refused;
    return false;
  }
  ++accepted;
  const ResidualSegInfo& s = y.deep.seg;
  // what was parsed lies inside the file
  if (s.inner_off + s.inner_len > n || s.res_off + s.res_len > n || s.index_off + 4 * (size_t)s.n_seg > n ||
      s.data_off + s.data_len > n || y.deep.lo_off + y.deep.lo_len > n) {
    std::printf("parsed fields run past the end\n");
    std::exit(1);
  }
  if (info) *info = y;
  return true;
}

static bool expect(const std::vector<uint8_t>& file, const char* word, uint64_t max_pixels = MAXPIX) {
  const char* err = nullptr;
  if (probe(file, file.size(), &err, nullptr, max_pixels)) return std::printf("accepted, wanted: %s\n", word), false;
  if (std::strstr(err, "container_parse_residual_yuv: ") != err && std::strstr(word, "container_parse:") == nullptr)
    return std::printf("message without the entry's name: %s\n", err), false;
  if (std::strstr(err, word) == nullptr) return std::printf("got \"%s\", wanted \"%s\"\n", err, word), false;
  return true;
}

static std::vector<uint8_t> with8(std::vector<uint8_t> f, size_t at, uint8_t v) {
  f[at] = v;
  return f;
}
static std::vector<uint8_t> with32(std::vector<uint8_t> f, size_t at, uint32_t v) {
  for (int i = 0; i < 4; ++i) f[at + i] = (uint8_t)(v >> (24 - 8 * i));
  return f;
}

static bool container_ok() {
  const struct {
    uint32_t H, W, L, depth, shift, sx, sy, matrix, flags;
    bool vbr;
  } cases[] = {{17, 70, 256, 8, 0, 2, 2, 1, 2, false},   {17, 70, 256, 10, 3, 2, 2, 2, 2, true},
               {19, 131, 300, 16, 9, 2, 1, 0, 1, false}, {5, 64, 65536, 12, 0, 1, 1, 1, 3, false},
               {1, 1, 256, 9, 2, 2, 2, 0, 0, true}};
  for (const auto& c : cases) {
    Made d;
    if (!make(c.H, c.W, c.L, c.vbr, c.depth, c.shift, c.sx, c.sy, c.matrix, c.flags, &d)) return false;
    ResidualYuvInfo y;
    if (!probe(d.file, d.file.size(), nullptr, &y)) return std::printf("a written file is refused\n"), false;
    const ResidualSegInfo& s = y.deep.seg;
    if (!is_residual_yuv_file(d.file.data(), d.file.size()) || is_residual_deep_file(d.file.data(), d.file.size()))
      return std::printf("magic\n"), false;
    if (s.H != c.H || s.W != c.W || s.tau != 5 || s.vbr != c.vbr || s.digest != 0x0123456789abcdefull ||
        s.seg_len != c.L || s.n_seg != d.seg_bytes.size() || y.deep.depth != c.depth || y.deep.shift != c.shift ||
        y.sub_x != c.sx || y.sub_y != c.sy || y.matrix != c.matrix || y.full_range != ((c.flags & 1) != 0) ||
        y.site_left != ((c.flags & 2) != 0))
      return std::printf("fields differ\n"), false;
    if (s.inner_len != d.inner.size() || std::memcmp(d.file.data() + s.inner_off, d.inner.data(), d.inner.size()) ||
        s.data_len != d.segs.size() || std::memcmp(d.file.data() + s.data_off, d.segs.data(), d.segs.size()) ||
        y.deep.lo_len != d.lo.size() || (d.lo.size() && std::memcmp(d.file.data() + y.deep.lo_off, d.lo.data(), d.lo.size())) ||
        y.deep.lo_off + y.deep.lo_len != d.file.size())
      return std::printf("strings differ\n"), false;
    for (size_t k = 0; k < d.seg_bytes.size(); ++k) {
      const uint8_t* p = d.file.data() + s.index_off + 4 * k;
      if ((((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]) != d.seg_bytes[k])
        return std::printf("index differs\n"), false;
    }
    for (size_t n = 0; n < d.file.size(); ++n)  // every truncation
      if (probe(d.file, n)) return std::printf("a truncation to %zu of %zu bytes is accepted\n", n, d.file.size()), false;
    std::vector<uint8_t> more = d.file;
    more.push_back(0);
    if (!expect(more, "bytes left over after the low-bit plane")) return false;
    // the other parsers refuse it, and this one theirs
    ContainerInfo ci;
    ResidualInfo ri;
    ResidualSegInfo si;
    ResidualDeepInfo di;
    if (!container_parse(d.file.data(), d.file.size(), false, NLEV, MAXPIX, &ci) ||
        !container_parse(d.file.data(), d.file.size(), true, NLEV, MAXPIX, &ci) ||
        !container_parse_residual(d.file.data(), d.file.size(), NLEV, MAXPIX, &ri) ||
        !container_parse_residual_seg(d.file.data(), d.file.size(), NLEV, MAXPIX, &si) ||
        !container_parse_residual_deep(d.file.data(), d.file.size(), NLEV, MAXPIX, &di))
      return std::printf("another parser accepts an MLR4 file\n"), false;
    if (!expect(d.inner, "container_parse_residual_yuv: ")) return false;
    for (int it = 0; it < 4000; ++it) {  // seeded overwrites: refused with a message, or parsed in bounds
      std::vector<uint8_t> f = d.file;
      const int cnt = 1 + (int)(rnd() % 3);
      for (int k = 0; k < cnt; ++k) f[rnd() % f.size()] = (uint8_t)rnd();
      const char* err = nullptr;
      if (!probe(f, f.size(), &err) && (err == nullptr || !*err)) return std::printf("a refusal without a message\n"), false;
    }
  }
  // every listed refusal, by message
  Made d;
  if (!make(17, 70, 256, false, 10, 3, 2, 2, 1, 2, &d)) return false;
  ResidualYuvInfo y;
  probe(d.file, d.file.size(), nullptr, &y);
  const ResidualSegInfo& s = y.deep.seg;
  const size_t ds = s.inner_off - 18;  // depth, shift, sub_x, sub_y, matrix, flags, then seg_len, n_seg, inner_len
  const std::vector<uint8_t>& f = d.file;
  if (!expect(with8(f, 3, '3'), "bad magic (not a Y'CbCr residual file)") || !expect(with8(f, 4, 1), "unknown version") ||
      !expect(with8(f, 5, 2), "unknown flags") || !expect(with8(f, 6, 128), "tau above 127") ||
      !expect(with8(f, 7, 23), "n_ctx is not 24") || !expect(with32(f, 8, 0), "H or W is zero") ||
      !expect(with8(f, 24, 64), "an m outside 0..63") || !expect(with8(f, ds, 7), "depth outside 8..16") ||
      !expect(with8(f, ds, 17), "depth outside 8..16") || !expect(with8(f, ds, 8), "shift must be 0 at depth 8") ||
      !expect(with8(f, ds + 1, 4), "shift outside 0..depth - 7") || !expect(with8(f, ds + 1, 2), "lo_len is not") ||
      !expect(with8(f, ds + 2, 1), "sub_x, sub_y is not one of") || !expect(with8(f, ds + 3, 3), "sub_x, sub_y is not one of") ||
      !expect(with8(f, ds + 3, 1), "n_seg is not ceil(N / seg_len)") || !expect(with8(f, ds + 4, 3), "matrix outside 0..2") ||
      !expect(with8(f, ds + 5, 4), "reserved flag bits are set") || !expect(with32(f, ds + 6, 255), "seg_len outside 256..65536") ||
      !expect(with32(f, ds + 10, s.n_seg + 1), "n_seg is not ceil(N / seg_len)") ||
      !expect(with32(f, ds + 14, 0), "an empty inner file") || !expect(with32(f, s.index_off, 6), "not a multiple of 4") ||
      !expect(with32(f, s.index_off, 4), "a segment length below 8") ||
      !expect(with32(f, s.index_off, d.seg_bytes[0] + 4), "not 4 n_seg + the segment lengths") ||
      !expect(with32(f, y.deep.lo_off - 4, (uint32_t)y.deep.lo_len + 8), "lo_len is not") ||
      !expect(std::vector<uint8_t>(f.begin(), f.end() - 1), "truncated inside the low-bit plane") ||
      !expect(std::vector<uint8_t>(f.begin(), f.begin() + (long)y.deep.lo_off - 2), "truncated before the low-bit plane's length") ||
      !expect(std::vector<uint8_t>(f.begin(), f.begin() + (long)ds + 3), "truncated before depth, shift and the frame's fields") ||
      !expect(std::vector<uint8_t>(f.begin(), f.begin() + 10), "truncated header") ||
      !expect(f, "exceeds max_pixels", 17 * 70 - 1))
    return false;
  Made e;  // BT.2020 at depth 8: the writer refuses it, and so does the parser for a file patched to say so
  if (!make(17, 70, 256, false, 8, 0, 2, 2, 1, 0, &e)) return false;
  probe(e.file, e.file.size(), nullptr, &y);
  if (!expect(with8(e.file, y.deep.seg.inner_off - 18 + 4, 2), "matrix 2 (BT.2020) at depth 8")) return false;
  size_t len = 0;
  const char* err = container_write_residual_yuv(17, 70, false, 5, 8, 0, 2, 2, 2, 0, 1, e.m, e.freq.data(), 256,
                                                 (uint32_t)e.seg_bytes.size(), e.seg_bytes.data(), e.inner.data(),
                                                 e.inner.size(), e.segs.data(), e.segs.size(), nullptr, 0, nullptr, 0, &len);
  if (!err || !std::strstr(err, "container_write_residual_yuv: matrix 2 (BT.2020) at depth 8")) return std::printf("writer: bt2020\n"), false;
  err = container_write_residual_yuv(17, 70, false, 5, 8, 1, 2, 2, 1, 0, 1, e.m, e.freq.data(), 256, (uint32_t)e.seg_bytes.size(),
                                     e.seg_bytes.data(), e.inner.data(), e.inner.size(), e.segs.data(), e.segs.size(),
                                     nullptr, 0, nullptr, 0, &len);
  if (!err || !std::strstr(err, "shift must be 0 at depth 8")) return std::printf("writer: shift at depth 8\n"), false;
  return true;
}

// ------------------------------------------------------------------------------------------ the coders for a given N
// the file's form of tables under which every sample is the costliest escape: context k has m = 0 (the symbol 0 and
// the escape), the escape with frequency 1
static void escape_tables(std::vector<uint8_t>* m, std::vector<uint16_t>* freq) {
  m->assign(24, 0);
  freq->assign(24 * 128, 0);
  for (int k = 0; k < 24; ++k) {
    (*freq)[k * 128] = 65535;
    (*freq)[k * 128 + 1] = 1;
  }
}

static bool coder_round_trip(int64_t N, int L, const char* what) {
  std::vector<uint8_t> m;
  std::vector<uint16_t> freq;
  escape_tables(&m, &freq);
  std::vector<int16_t> sym((size_t)N), back((size_t)N, 7);
  std::vector<uint8_t> ctx((size_t)N);
  for (int64_t i = 0; i < N; ++i) sym[i] = (i & 1) ? -255 : 255, ctx[i] = (uint8_t)(i % 24);
  const int64_t n_seg = residual_n_seg(N, L);
  residual_seg_check_n(what, 1, N, L, n_seg);
  std::vector<uint32_t> seg_bytes((size_t)n_seg);
  uint64_t len = 0;
  residual_seg_encode_host_n(what, sym.data(), ctx.data(), 1, N, m.data(), freq.data(), L, n_seg, nullptr, 0,
                             seg_bytes.data(), &len);
  uint64_t sum = 0;
  for (int64_t k = 0; k < n_seg; ++k) {
    const int64_t n = residual_seg_samples(N, L, k);
    if (seg_bytes[k] % 4 || seg_bytes[k] < 8 || seg_bytes[k] > 4 * (uint64_t)(n + 2))
      return std::printf("%s: segment %lld of %lld samples took %u bytes\n", what, (long long)k, (long long)n, seg_bytes[k]), false;
    sum += seg_bytes[k];
  }
  if (sum != len) return std::printf("%s: lengths\n", what), false;
  std::unique_ptr<uint8_t[]> out(new uint8_t[len]);  // exactly the bytes: a write or read past them is seen
  std::vector<uint32_t> again((size_t)n_seg);
  uint64_t len2 = 0;
  residual_seg_encode_host_n(what, sym.data(), ctx.data(), 1, N, m.data(), freq.data(), L, n_seg, out.get(), len,
                             again.data(), &len2);
  if (len2 != len || again != seg_bytes) return std::printf("%s: the second pass differs\n", what), false;
  residual_seg_lengths_check(what, seg_bytes.data(), &len, len, 1, N, L, n_seg);
  residual_seg_decode_host_n(what, out.get(), len, &len, seg_bytes.data(), ctx.data(), 1, N, m.data(), freq.data(), L,
                             n_seg, back.data());
  if (back != sym) return std::printf("%s: decode differs\n", what), false;
  return true;
}

// a flipped byte is refused, and the refusal names the segment.  The tables are skewed with frequencies that are no
// powers of two and the symbols have no escapes: under flat power-of-two tables, as in an escape's bypass nibbles,
// rANS is plain bit packing and a flip only changes a value, which no check can see.
static bool flip_refused(int64_t N, int L, const char* what) {
  static const uint16_t f8[8] = {1000, 3000, 12000, 40000, 6000, 2000, 1500, 36};  // q = -3..3 and the escape
  std::vector<uint8_t> m(24, 3);
  std::vector<uint16_t> freq(24 * 128, 0);
  for (int k = 0; k < 24; ++k)
    for (int j = 0; j < 8; ++j) freq[k * 128 + j] = f8[j];
  std::vector<int16_t> sym((size_t)N), back((size_t)N);
  std::vector<uint8_t> ctx((size_t)N);
  for (int64_t i = 0; i < N; ++i) sym[i] = (int16_t)((int)(rnd() % 7) - 3), ctx[i] = (uint8_t)(rnd() % 24);
  const int64_t n_seg = residual_n_seg(N, L);
  std::vector<uint32_t> seg_bytes((size_t)n_seg);
  uint64_t len = 0;
  residual_seg_encode_host_n(what, sym.data(), ctx.data(), 1, N, m.data(), freq.data(), L, n_seg, nullptr, 0,
                             seg_bytes.data(), &len);
  std::unique_ptr<uint8_t[]> out(new uint8_t[len]);
  residual_seg_encode_host_n(what, sym.data(), ctx.data(), 1, N, m.data(), freq.data(), L, n_seg, out.get(), len,
                             seg_bytes.data(), &len);
  residual_seg_decode_host_n(what, out.get(), len, &len, seg_bytes.data(), ctx.data(), 1, N, m.data(), freq.data(), L,
                             n_seg, back.data());
  if (back != sym) return std::printf("%s: decode differs\n", what), false;
  out[len - seg_bytes[(size_t)n_seg - 1] / 2 - 1] ^= 0x08;  // inside the last segment
  try {
    residual_seg_decode_host_n(what, out.get(), len, &len, seg_bytes.data(), ctx.data(), 1, N, m.data(), freq.data(), L,
                               n_seg, back.data());
    return std::printf("%s: a flipped byte is accepted\n", what), false;
  } catch (const std::runtime_error& e) {
    const std::string want = "segment " + std::to_string(n_seg - 1) + ": ";
    if (std::string(e.what()).find(want) == std::string::npos) return std::printf("%s: %s\n", what, e.what()), false;
  }
  return true;
}

static bool refuses(int64_t N, int L, int64_t n_seg, const char* word) {
  try {
    residual_seg_check_n("check_n", 1, N, L, n_seg);
  } catch (const std::runtime_error& e) {
    if (std::strstr(e.what(), word)) return true;
    return std::printf("check_n: got \"%s\", wanted \"%s\"\n", e.what(), word), false;
  }
  return std::printf("check_n accepts N %lld L %d n_seg %lld\n", (long long)N, L, (long long)n_seg), false;
}

static bool coders_ok() {
  if (!coder_round_trip(3, 256, "N = 3") || !coder_round_trip(6 * 256 + 1, 256, "N = 6 * 256 + 1") ||
      !coder_round_trip(residual_yuv_geom(19, 261, 2, 2).N, 256, "a 4:2:0 frame") ||
      !coder_round_trip(residual_yuv_geom(19, 261, 2, 2).N, 4096, "a 4:2:0 frame, L = 4096") ||
      !coder_round_trip(65536 + 5, 65536, "L = 65536"))
    return false;
  if (!flip_refused(3, 256, "flip, N = 3") || !flip_refused(6 * 256 + 1, 256, "flip, N = 6 * 256 + 1") ||
      !flip_refused(residual_yuv_geom(19, 261, 2, 2).N, 4096, "flip, a 4:2:0 frame"))
    return false;
  if (!refuses(0, 256, 0, "N must be positive") || !refuses(RES_SEG_MAX_N + 1, 65536, 8193, "N is above 2^29") ||
      !refuses(1000, 255, 4, "outside 256..65536") || !refuses(1000, 256, 3, "is not ceil(N / seg_len) = 4"))
    return false;
  // at N = 3 H W the H, W entry gives the same bytes
  const int H = 7, W = 45;
  const int64_t N = 3 * H * W, n_seg = residual_n_seg(N, 256);
  std::vector<uint8_t> m;
  std::vector<uint16_t> freq;
  escape_tables(&m, &freq);
  std::vector<int16_t> sym((size_t)N);
  std::vector<uint8_t> ctx((size_t)N);
  for (int64_t i = 0; i < N; ++i) sym[i] = (int16_t)((int)(rnd() % 511) - 255), ctx[i] = (uint8_t)(rnd() % 24);
  const size_t cap = 4 * (size_t)(N + 4 * n_seg);
  std::vector<uint8_t> a(cap, 0), b(cap, 0);
  std::vector<uint32_t> sa((size_t)n_seg), sb((size_t)n_seg);
  uint64_t la = 0, lb = 0;
  residual_seg_encode_host(sym.data(), ctx.data(), 1, H, W, m.data(), freq.data(), 256, n_seg, a.data(), cap, sa.data(), &la);
  residual_seg_encode_host_n("n", sym.data(), ctx.data(), 1, N, m.data(), freq.data(), 256, n_seg, b.data(), cap, sb.data(), &lb);
  if (la != lb || sa != sb || a != b) return std::printf("the N entry differs from the H, W entry\n"), false;
  return true;
}

int main() {
  try {
    if (!geometry_ok() || !bound_ok() || !container_ok() || !coders_ok()) return 1;
  } catch (const std::exception& e) {
    std::printf("exception: %s\n", e.what());
    return 1;
  }
  std::printf("%ld inputs refused, %ld accepted\ncontainer_residual_yuv_check ok\n", refused, accepted);
  return 0;
}
