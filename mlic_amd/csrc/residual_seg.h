// Segmented residual strings (DESIGN.md section 5 "Residual coding", "Segments"): the integer definitions shared by
// the host coder (residual_seg.cpp), the kernels (residual_coder.hip), the C ABI (capi.cpp) and the file
// (container.cpp).  Host and device, no HIP call.
//
// The N = 3 H W samples of an image, in residual.h's canonical order, are cut into n_seg = ceil(N / L) segments:
// segment k is [k L, min((k + 1) L, N)), L in 256..65536.  Segments ignore row and channel boundaries.  A segment's
// bytes are exactly mlic::rans_encode (rans.cpp) of its symbols and contexts under the image's 24 tables: 64-bit
// state from 2^31, 32-bit words, 16-bit frequencies, |q| > m escaped through 4-bit bypass nibbles, two words of flush.
// The contexts read the base picture alone and the tables are static, so segments code and decode independently.
// A decoder that has decoded a whole segment has consumed exactly its words and holds the state 2^31 again (the
// encoder started there and rANS is a bijection on the state): both decoders check that per segment.
//
// Capacity.  Let w be the words written and x the state, and I = 32 w + log2 x.  The coder starts at I = 31.  An emit
// with frequency f first renormalises when x >= 2^47 f (one word out, x >>= 32: I does not grow, and x >= 2^15 f is
// left), then takes x to floor(x / f) 2^16 + x mod f + start < (x / f + 1) 2^16 = x (2^16 / f) (1 + f / x), so I
// grows by less than 16 - log2 f + log2(1 + 2^-15).  With |q| <= 255 and max_value = 2 m + 1 the raw escape value is
// at most 510, so nb <= 3 and a sample is at most five emits: the symbol (f >= 1: 16 bits), nb and three nibbles
// (f = 2^12: 4 bits each), 32 bits and 5 log2(1 + 2^-15) < 2.3e-4 more.  At the end x >= 2^31, so
//     32 w + 31 <= I <= 31 + n (32 + 2.3e-4),   w <= n + n 7.2e-6 < n + 1   for n <= 65536,
// that is w <= n, and with the flush a segment of n samples is at most n + 2 words.  RES_SEG_SLACK = 4 is what the
// file and the entries allow; tools/container_residual_seg_check.cpp asserts the bound over all-escape segments under
// tables with frequency-1 entries.  The kernels do not rely on it: every store is checked against the segment's size.
#ifndef MLIC_RESIDUAL_SEG_H
#define MLIC_RESIDUAL_SEG_H
#include <cstddef>
#include <cstdint>

#include "residual.h"

namespace mlic {

constexpr int RES_SEG_MIN = 256;
constexpr int RES_SEG_MAX = 65536;
constexpr int RES_SEG_SLACK = 4;      // words a segment may take beyond one per sample, flush included
constexpr int RES_SEG_MIN_BYTES = 8;  // the flush alone
constexpr int RES_MAX_Q = 255;
constexpr int RES_MAX_NB = 3;         // bypass nibbles of a raw value <= 510
constexpr int64_t RES_SEG_MAX_N = (int64_t)1 << 29;  // so that an image's bytes and 16 n_seg stay below 2^32

MLIC_RES_HD inline int64_t residual_n_seg(int64_t N, int L) { return (N + L - 1) / L; }
MLIC_RES_HD inline int64_t residual_seg_samples(int64_t N, int L, int64_t k) {
  const int64_t left = N - k * L;
  return left < L ? left : L;
}
MLIC_RES_HD inline uint32_t residual_seg_cap_bytes(int64_t n) { return 4u * (uint32_t)(n + RES_SEG_SLACK); }

// The per-image status word of the kernels: RES_SEG_CLEAN, or (segment << 4) | reason of the smallest bad segment
// (atomicMin).  The entries reset it on the stream.
constexpr uint32_t RES_SEG_CLEAN = 0xFFFFFFFFu;
enum ResSegReason : uint32_t {
  RES_SEG_OVERFLOW = 1,  // encode: the bytes do not fit the capacity
  RES_SEG_CONTEXT = 2,   // a context >= 24 or without a table
  RES_SEG_BYPASS = 3,    // decode: a bypass length above 3
  RES_SEG_SYMBOL = 4,    // decode: a symbol index above max_value
  RES_SEG_RANGE = 5,     // a q outside [-255, 255]
  RES_SEG_STATE = 6,     // decode: the final state is not 2^31
  RES_SEG_WORDS = 7,     // decode: the words consumed are not the segment's
};
inline const char* residual_seg_reason(uint32_t r) {
  switch (r) {
    case RES_SEG_OVERFLOW: return "the bytes do not fit the capacity";
    case RES_SEG_CONTEXT: return "a context without a table";
    case RES_SEG_BYPASS: return "a bypass length above 3";
    case RES_SEG_SYMBOL: return "a symbol index above max_value";
    case RES_SEG_RANGE: return "a symbol outside [-255, 255]";
    case RES_SEG_STATE: return "the final state is not 2^31";
    case RES_SEG_WORDS: return "the words consumed are not the segment's";
  }
  return "unknown";
}

// The tables as the kernels read them, built on the host from the file's form (m[24], freq[24][128]).
// Encoder record of (context, symbol index): ryg_rans' exact reciprocal (rans.cpp make_enc_sym) in 16 bytes;
// cmpl_freq = 2^16 - freq and bias = start (+ 2^16 - 1 for freq 1) follow from freq and start.
struct ResEncRec {
  uint64_t rcp;
  uint32_t freq_start;  // freq | start << 16 (a table has >= 2 symbols, so freq <= 65535)
  uint32_t shift;
};
struct alignas(16) ResSegEncTable {
  ResEncRec rec[RES_CTX * RES_BINS];
  uint8_t m[32];  // m[k], RES_ABSENT without a table
};
constexpr int RES_SEG_LUT_BITS = 10;
struct alignas(16) ResSegDecTable {
  uint32_t cdf[RES_CTX][RES_CDF_STRIDE + 1];        // cdf[k][0 .. 2 m + 2], the rest 65536
  uint8_t lut[RES_CTX][1 << RES_SEG_LUT_BITS];      // the largest s with cdf[s] <= bucket << 6
  uint8_t m[32];
};

// Host side (residual_seg.cpp).  The checks throw std::runtime_error with a message that begins "mlic: <what>: ";
// the device entries call them before any HIP call.  m: [B][24], freq: [B][24][128] (the file's form).
void residual_seg_check(const char* what, int B, int H, int W, int seg_len, int64_t n_seg);
void residual_seg_check_n(const char* what, int B, int64_t N, int seg_len, int64_t n_seg);  // 1 <= N <= RES_SEG_MAX_N
void residual_seg_tables_check(const char* what, const uint8_t* m, const uint16_t* freq, int B);
// each length a multiple of 4, >= 8 and within residual_seg_cap_bytes of its samples; sum = data_len[b] <= stride
void residual_seg_lengths_check(const char* what, const uint32_t* seg_bytes, const uint64_t* data_len, size_t stride,
                                int B, int64_t N, int seg_len, int64_t n_seg);
void residual_seg_enc_table(const uint8_t* m, const uint16_t* freq, ResSegEncTable* t);
void residual_seg_dec_table(const uint8_t* m, const uint16_t* freq, ResSegDecTable* t);
// The host coder: a loop over segments on RansEncoder / RansDecoderState.  Image b's bytes start at out + b cap
// (data + b stride).  encode: out == nullptr asks for len and seg_bytes only; a cap below an image's bytes throws.
// decode: throws naming the image and the first bad segment.
void residual_seg_encode_host(const int16_t* sym, const uint8_t* ctx, int B, int H, int W, const uint8_t* m,
                              const uint16_t* freq, int seg_len, int64_t n_seg, uint8_t* out, size_t cap,
                              uint32_t* seg_bytes, uint64_t* len);
void residual_seg_decode_host(const uint8_t* data, size_t stride, const uint64_t* data_len, const uint32_t* seg_bytes,
                              const uint8_t* ctx, int B, int H, int W, const uint8_t* m, const uint16_t* freq,
                              int seg_len, int64_t n_seg, int16_t* sym);
// The same two for a string of N samples that is not an RGB image's 3 H W (a Y'CbCr frame: residual_yuv.h), with the
// entry's name for the messages; the two above forward here.
void residual_seg_encode_host_n(const char* what, const int16_t* sym, const uint8_t* ctx, int B, int64_t N,
                                const uint8_t* m, const uint16_t* freq, int seg_len, int64_t n_seg, uint8_t* out,
                                size_t cap, uint32_t* seg_bytes, uint64_t* len);
void residual_seg_decode_host_n(const char* what, const uint8_t* data, size_t stride, const uint64_t* data_len,
                                const uint32_t* seg_bytes, const uint8_t* ctx, int B, int64_t N, const uint8_t* m,
                                const uint16_t* freq, int seg_len, int64_t n_seg, int16_t* sym);

}  // namespace mlic
#endif
