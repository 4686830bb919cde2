// Segmented residual strings, host side (residual_seg.h has the definitions): argument checks shared by the host and
// device entries, the kernels' tables, and the host coder, which is the oracle of residual_coder.hip.
#include "residual_seg.h"

#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "rans.h"

namespace mlic {

namespace {
[[noreturn]] void fail(const char* what, const std::string& msg) {
  throw std::runtime_error(std::string("mlic: ") + what + ": " + msg);
}

// rans.cpp's tables of one image: an absent context gets a two-symbol placeholder that nothing is coded with
CdfTables coder_tables(const uint8_t* m, const uint16_t* freq) {
  CdfTables t;
  t.n = RES_CTX;
  t.stride = RES_CDF_STRIDE;
  t.cdf.assign((size_t)RES_CTX * RES_CDF_STRIDE, 0);
  t.length.assign(RES_CTX, 3);
  t.offset.assign(RES_CTX, 0);
  for (int k = 0; k < RES_CTX; ++k) {
    int32_t* c = t.cdf.data() + (size_t)k * RES_CDF_STRIDE;
    if (m[k] == RES_ABSENT) {
      c[1] = 32768;
      c[2] = 65536;
      continue;
    }
    const int cnt = 2 * m[k] + 2;
    for (int j = 0; j < cnt; ++j) c[j + 1] = c[j] + freq[k * RES_BINS + j];
    t.length[k] = cnt + 1;
    t.offset[k] = -(int32_t)m[k];
  }
  t.prepare();
  return t;
}

// the first sample of a segment that the tables cannot code, or -1
int64_t first_uncodable(const int16_t* sym, const uint8_t* ctx, int64_t n, const uint8_t* m, bool* range) {
  for (int64_t i = 0; i < n; ++i) {
    if (ctx[i] >= RES_CTX || m[ctx[i]] == RES_ABSENT) {
      *range = false;
      return i;
    }
    if (sym && (sym[i] < -RES_MAX_Q || sym[i] > RES_MAX_Q)) {
      *range = true;
      return i;
    }
  }
  return -1;
}
}  // namespace

namespace {
void seg_len_check(const char* what, int64_t N, int seg_len, int64_t n_seg, const char* of) {
  if (seg_len < RES_SEG_MIN || seg_len > RES_SEG_MAX)
    fail(what, "the segment length " + std::to_string(seg_len) + " is outside 256..65536");
  if (n_seg != residual_n_seg(N, seg_len))
    fail(what, "n_seg " + std::to_string(n_seg) + " is not ceil(" + of + " / seg_len) = " +
                   std::to_string(residual_n_seg(N, seg_len)));
}
}  // namespace

void residual_seg_check(const char* what, int B, int H, int W, int seg_len, int64_t n_seg) {
  if (B < 1) fail(what, "B must be positive");
  if (H < 1 || W < 1) fail(what, "H and W must be positive");
  const int64_t N = 3 * (int64_t)H * W;
  if (N > RES_SEG_MAX_N) fail(what, "the image has more than 2^29 samples");
  seg_len_check(what, N, seg_len, n_seg, "3 H W");
}

void residual_seg_check_n(const char* what, int B, int64_t N, int seg_len, int64_t n_seg) {
  if (B < 1) fail(what, "B must be positive");
  if (N < 1) fail(what, "N must be positive");
  if (N > RES_SEG_MAX_N) fail(what, "N is above 2^29 samples");
  seg_len_check(what, N, seg_len, n_seg, "N");
}

void residual_seg_tables_check(const char* what, const uint8_t* m, const uint16_t* freq, int B) {
  if (m == nullptr) fail(what, "null m");
  if (freq == nullptr) fail(what, "null frequencies");
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < RES_CTX; ++k) {
      const uint8_t mk = m[b * RES_CTX + k];
      if (mk == RES_ABSENT) continue;
      if (mk > RES_MAX_M) fail(what, "an m outside 0..63");
      uint32_t sum = 0;
      for (int j = 0; j < 2 * mk + 2; ++j) {
        const uint16_t f = freq[((size_t)b * RES_CTX + k) * RES_BINS + j];
        if (f == 0) fail(what, "a zero frequency");
        sum += f;
      }
      if (sum != 65536) fail(what, "a table's frequencies do not sum to 65536");
    }
}

void residual_seg_lengths_check(const char* what, const uint32_t* seg_bytes, const uint64_t* data_len, size_t stride,
                                int B, int64_t N, int seg_len, int64_t n_seg) {
  if (seg_bytes == nullptr) fail(what, "null segment lengths");
  if (data_len == nullptr) fail(what, "null data lengths");
  for (int b = 0; b < B; ++b) {
    uint64_t sum = 0;
    for (int64_t k = 0; k < n_seg; ++k) {
      const uint32_t v = seg_bytes[(size_t)b * n_seg + k];
      const std::string where = "image " + std::to_string(b) + ", segment " + std::to_string(k) + ": ";
      if (v % 4) fail(what, where + "a length that is not a multiple of 4");
      if (v < RES_SEG_MIN_BYTES) fail(what, where + "a length below 8");
      if (v > residual_seg_cap_bytes(residual_seg_samples(N, seg_len, k)))
        fail(what, where + "a length above the capacity bound of its samples");
      sum += v;
    }
    if (sum != data_len[b])
      fail(what, "image " + std::to_string(b) + ": the segment lengths sum to " + std::to_string(sum) +
                     ", the data length is " + std::to_string(data_len[b]));
    if (data_len[b] > stride) fail(what, "image " + std::to_string(b) + ": the data length exceeds the stride");
  }
}

void residual_seg_enc_table(const uint8_t* m, const uint16_t* freq, ResSegEncTable* t) {
  std::memset(t, 0, sizeof(*t));
  const CdfTables c = coder_tables(m, freq);
  for (int k = 0; k < RES_CTX; ++k) {
    t->m[k] = m[k];
    if (m[k] == RES_ABSENT) continue;
    for (int j = 0; j < 2 * m[k] + 2; ++j) {
      const EncSym& e = c.enc[(size_t)k * RES_CDF_STRIDE + j];
      const uint32_t start = (uint32_t)c.cdf[(size_t)k * RES_CDF_STRIDE + j];
      t->rec[k * RES_BINS + j] = ResEncRec{e.rcp_freq, e.freq | (start << 16), e.rcp_shift};
    }
  }
  for (int k = RES_CTX; k < 32; ++k) t->m[k] = RES_ABSENT;
}

void residual_seg_dec_table(const uint8_t* m, const uint16_t* freq, ResSegDecTable* t) {
  std::memset(t, 0, sizeof(*t));
  for (int k = 0; k < 32; ++k) t->m[k] = k < RES_CTX ? m[k] : RES_ABSENT;
  for (int k = 0; k < RES_CTX; ++k) {
    uint32_t* c = t->cdf[k];
    const int cnt = m[k] == RES_ABSENT ? 0 : 2 * m[k] + 2;
    for (int j = 0; j < cnt; ++j) c[j + 1] = c[j] + freq[k * RES_BINS + j];
    for (int j = cnt + 1; j <= RES_CDF_STRIDE; ++j) c[j] = 65536;
    int s = 0;
    for (int b = 0; b < (1 << RES_SEG_LUT_BITS); ++b) {
      const uint32_t lo = (uint32_t)b << (16 - RES_SEG_LUT_BITS);
      while (s + 1 < cnt && c[s + 1] <= lo) ++s;
      t->lut[k][b] = (uint8_t)s;
    }
  }
}

void residual_seg_encode_host(const int16_t* sym, const uint8_t* ctx, int B, int H, int W, const uint8_t* m,
                              const uint16_t* freq, int seg_len, int64_t n_seg, uint8_t* out, size_t cap,
                              uint32_t* seg_bytes, uint64_t* len) {
  residual_seg_encode_host_n("residual_encode_segments_host", sym, ctx, B, 3 * (int64_t)H * W, m, freq, seg_len, n_seg,
                             out, cap, seg_bytes, len);
}

void residual_seg_encode_host_n(const char* what, const int16_t* sym, const uint8_t* ctx, int B, int64_t N,
                                const uint8_t* m, const uint16_t* freq, int seg_len, int64_t n_seg, uint8_t* out,
                                size_t cap, uint32_t* seg_bytes, uint64_t* len) {
  for (int b = 0; b < B; ++b) {
    const uint8_t* mb = m + (size_t)b * RES_CTX;
    const CdfTables t = coder_tables(mb, freq + (size_t)b * RES_CTX * RES_BINS);
    uint64_t total = 0;
    for (int64_t k = 0; k < n_seg; ++k) {
      const int64_t n = residual_seg_samples(N, seg_len, k);
      const int16_t* s = sym + (size_t)b * N + k * seg_len;
      const uint8_t* c = ctx + (size_t)b * N + k * seg_len;
      bool range = false;
      const int64_t bad = first_uncodable(s, c, n, mb, &range);
      if (bad >= 0)
        fail(what, "image " + std::to_string(b) + ", segment " + std::to_string(k) + ": " +
                       residual_seg_reason(range ? RES_SEG_RANGE : RES_SEG_CONTEXT));
      RansEncoder e(n);
      e.put_reverse(s, c, n, t);
      const std::string bytes = e.flush();
      if (bytes.size() > residual_seg_cap_bytes(n))
        fail(what, "image " + std::to_string(b) + ", segment " + std::to_string(k) + ": above the capacity bound");
      seg_bytes[(size_t)b * n_seg + k] = (uint32_t)bytes.size();
      if (out != nullptr) {
        if (total + bytes.size() > cap)
          fail(what, "image " + std::to_string(b) + ", segment " + std::to_string(k) + ": " +
                         residual_seg_reason(RES_SEG_OVERFLOW));
        std::memcpy(out + (size_t)b * cap + total, bytes.data(), bytes.size());
      }
      total += bytes.size();
    }
    len[b] = total;
  }
}

void residual_seg_decode_host(const uint8_t* data, size_t stride, const uint64_t* data_len, const uint32_t* seg_bytes,
                              const uint8_t* ctx, int B, int H, int W, const uint8_t* m, const uint16_t* freq,
                              int seg_len, int64_t n_seg, int16_t* sym) {
  residual_seg_decode_host_n("residual_decode_segments_host", data, stride, data_len, seg_bytes, ctx, B,
                             3 * (int64_t)H * W, m, freq, seg_len, n_seg, sym);
}

void residual_seg_decode_host_n(const char* what, const uint8_t* data, size_t stride, const uint64_t* data_len,
                                const uint32_t* seg_bytes, const uint8_t* ctx, int B, int64_t N, const uint8_t* m,
                                const uint16_t* freq, int seg_len, int64_t n_seg, int16_t* sym) {
  (void)data_len;
  for (int b = 0; b < B; ++b) {
    const uint8_t* mb = m + (size_t)b * RES_CTX;
    const CdfTables t = coder_tables(mb, freq + (size_t)b * RES_CTX * RES_BINS);
    size_t off = 0;
    for (int64_t k = 0; k < n_seg; ++k) {
      const int64_t n = residual_seg_samples(N, seg_len, k);
      const uint8_t* c = ctx + (size_t)b * N + k * seg_len;
      int16_t* q = sym + (size_t)b * N + k * seg_len;
      const uint32_t nb = seg_bytes[(size_t)b * n_seg + k];
      const std::string where = "image " + std::to_string(b) + ", segment " + std::to_string(k) + ": ";
      bool range = false;
      if (first_uncodable(nullptr, c, n, mb, &range) >= 0) fail(what, where + residual_seg_reason(RES_SEG_CONTEXT));
      RansDecoderState d;
      d.set_max_bypass(RES_MAX_NB);
      d.set_stream(data + (size_t)b * stride + off, nb);
      uint32_t reason = 0;
      try {
        if (!d.decode(c, n, t, q, RES_MAX_Q)) reason = RES_SEG_RANGE;
      } catch (const std::runtime_error& e) {
        reason = std::strstr(e.what(), "bypass") ? RES_SEG_BYPASS : RES_SEG_SYMBOL;
      }
      if (!reason)
        for (int64_t i = 0; i < n; ++i)
          if (q[i] < -RES_MAX_Q) reason = RES_SEG_RANGE;  // the narrow range is [-nlim - 1, nlim]
      const RansDecoderState::Mark mk = d.mark();
      if (!reason && mk.pos != nb / 4) reason = RES_SEG_WORDS;
      if (!reason && mk.state != (1ull << 31)) reason = RES_SEG_STATE;
      if (reason) fail(what, where + residual_seg_reason(reason));
      off += nb;
    }
  }
}

}  // namespace mlic
