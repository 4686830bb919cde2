// The device rANS coder of the segmented residual strings (residual_seg.h has the definitions; DESIGN.md section 5
// "Residual coding", "Segments").  A segment's bytes are exactly rans.cpp's rans_encode of its samples, so the host
// coder is the oracle of both kernels.
//
// Mapping, both kernels: one lane per segment, a workgroup is one wave and owns 64 consecutive segments of one
// image (the tables are per image).  A lane that read sym[k L + j] itself would touch one cache line per sample
// across the wave, so the wave stages chunks of RC_CHUNK samples of its 64 segments through LDS: 32 lanes read 32
// consecutive samples of one segment (sym int16 and ctx uint8, coalesced), two segments per instruction, and put
// them down as one dword per sample in a row of RC_CHUNK + 1 dwords per segment, so that the lanes, each walking
// its own row, hit 64 different banks.
//
// Encoder.  The image's records (ResEncRec, 16 bytes per (context, symbol): ryg_rans' exact reciprocal) sit in LDS:
// 48 KB, read once per wave from L2.  Segments are walked backwards (rANS is LIFO) and a lane's words go out towards
// lower addresses, as RansEncoder::put_reverse does.  The output is made in two passes of the same coder with no host
// round trip between them: a counting pass writes seg_bytes, residual_seg_scan_kernel turns them into offsets (and
// flags an image whose bytes exceed the capacity), and the writing pass puts every word into its final place.  No
// scratch of one word per sample, and the bytes cannot depend on the launch geometry; the price is that the coder's
// arithmetic runs twice.  Every store is checked against the segment's own size.
//
// Decoder.  The image's 24 CDFs and a 1024-bucket first-candidate table per context (built on the host) sit in LDS.
// A lane reads its words forwards from data + seg_off[k]; past seg_bytes[k] it takes zeros.  Decoded q goes back into
// the staged dword and leaves as int16 in canonical order, coalesced.  Anything a well-formed segment cannot hold
// ends the lane's decoding (it writes zeros from there) and goes to the image's status word with atomicMin.
#include "kernels.h"
#include "residual_seg.h"

namespace mlic {

namespace {

constexpr int RC_CHUNK = 32;
constexpr int RC_ROW = RC_CHUNK + 1;
constexpr uint64_t RC_L = 1ull << 31;

// chunk c of the wave's 64 segments -> S (sym in the low half, ctx above it)
__device__ inline void stage_in(uint32_t* S, const int16_t* sym, const uint8_t* ctx, int64_t seg0, int64_t n_seg,
                                int64_t N, int L, int c, int lane) {
  const int j = lane & 31;
  const int idx = c * RC_CHUNK + j;
  for (int r0 = 0; r0 < 64; r0 += 2) {
    const int r = r0 + (lane >> 5);
    const int64_t seg = seg0 + r;
    const int64_t i = seg * L + idx;
    if (seg < n_seg && idx < L && i < N)
      S[r * RC_ROW + j] = (sym ? (uint32_t)(uint16_t)sym[i] : 0u) | ((uint32_t)ctx[i] << 16);
  }
}

template <class T>
__device__ inline void table_to_lds(T* dst, const T* src, int lane) {
  static_assert(sizeof(T) % 16 == 0, "tables are copied as 16-byte pieces");
  const uint4* s = reinterpret_cast<const uint4*>(src);
  uint4* d = reinterpret_cast<uint4*>(dst);
  for (int i = lane; i < (int)(sizeof(T) / 16); i += 64) d[i] = s[i];
}

template <bool WRITE>
__global__ __launch_bounds__(64) void residual_encode_segments_kernel(
    const int16_t* __restrict__ sym, const uint8_t* __restrict__ ctx, int64_t N, int L, int64_t n_seg, int wpi,
    const ResSegEncTable* __restrict__ tabs, uint8_t* __restrict__ out, size_t cap,
    const uint32_t* __restrict__ seg_off, uint32_t* __restrict__ seg_bytes, uint32_t* __restrict__ status) {
  __shared__ ResSegEncTable T;
  __shared__ uint32_t S[64 * RC_ROW];
  const int lane = threadIdx.x;
  const int img = blockIdx.x / wpi;
  const int64_t seg0 = (int64_t)(blockIdx.x % wpi) * 64;
  const int64_t k = seg0 + lane;
  const bool active = k < n_seg;
  if (WRITE && status[img] != RES_SEG_CLEAN) return;  // the counting pass or the scan refused the image: no byte of it
  table_to_lds(&T, tabs + img, lane);
  sym += (size_t)img * N;
  ctx += (size_t)img * N;
  const int n_k = active ? (int)residual_seg_samples(N, L, k) : 0;
  uint64_t x = RC_L;
  uint32_t cnt = 0, p = 0, bad = 0;
  uint32_t* wbase = nullptr;
  if (WRITE && active) {
    p = seg_bytes[(size_t)img * n_seg + k] / 4;
    wbase = reinterpret_cast<uint32_t*>(out + (size_t)img * cap + seg_off[(size_t)img * n_seg + k]);
  }
  auto emit = [&](uint32_t w) {
    if (WRITE) {
      if (p > 0) wbase[--p] = w;
      else bad = RES_SEG_OVERFLOW;
    } else {
      ++cnt;
    }
  };
  auto put_bits = [&](uint32_t val) {  // rans.cpp enc_put_bits with 4 bits: freq 2^12, x_max = 2^59
    if (x >= (1ull << 59)) {
      emit((uint32_t)x);
      x >>= 32;
    }
    x = (x << 4) | val;
  };
  const int nch = (L + RC_CHUNK - 1) / RC_CHUNK;
  for (int c = nch - 1; c >= 0; --c) {
    __syncthreads();
    stage_in(S, sym, ctx, seg0, n_seg, N, L, c, lane);
    __syncthreads();
    for (int j = RC_CHUNK - 1; j >= 0; --j) {
      if (c * RC_CHUNK + j >= n_k || bad) continue;
      const uint32_t v = S[lane * RC_ROW + j];
      const int q = (int)(int16_t)(v & 0xffffu);
      const uint32_t ci = v >> 16;
      const uint32_t mk = ci < (uint32_t)RES_CTX ? T.m[ci] : RES_ABSENT;
      if (mk == RES_ABSENT) {
        bad = RES_SEG_CONTEXT;
        continue;
      }
      if (q < -RES_MAX_Q || q > RES_MAX_Q) {
        bad = RES_SEG_RANGE;
        continue;
      }
      const int mx = 2 * (int)mk + 1;
      int value = q + (int)mk;
      if ((uint32_t)value >= (uint32_t)mx) {  // the escape: raw <= 510, so at most three nibbles, last first
        const uint32_t raw = value < 0 ? (uint32_t)(-2 * value - 1) : (uint32_t)(2 * (value - mx));
        const int nb = raw == 0 ? 0 : raw < 16 ? 1 : raw < 256 ? 2 : 3;
        for (int t = nb; t-- > 0;) put_bits((raw >> (4 * t)) & 15u);
        put_bits((uint32_t)nb);
        value = mx;
      }
      const ResEncRec e = T.rec[ci * RES_BINS + value];  // rans.cpp enc_put_sym
      const uint32_t freq = e.freq_start & 0xffffu, start = e.freq_start >> 16;
      if (x >= ((uint64_t)freq << 47)) {
        emit((uint32_t)x);
        x >>= 32;
      }
      const uint64_t quo = __umul64hi(x, e.rcp) >> e.shift;
      x = x + (start + (freq < 2 ? 65535u : 0u)) + quo * (uint64_t)(65536u - freq);
    }
  }
  if (!active) return;
  if (WRITE) {
    if (!bad && p == 2) {
      wbase[0] = (uint32_t)x;
      wbase[1] = (uint32_t)(x >> 32);
    } else if (!bad) {
      bad = RES_SEG_OVERFLOW;
    }
  } else {
    seg_bytes[(size_t)img * n_seg + k] = 4u * (cnt + 2u);
  }
  if (bad) atomicMin(status + img, ((uint32_t)k << 4) | bad);
}

// seg_off = the exclusive prefix sum of an image's seg_bytes; total; an image whose bytes exceed cap is refused
__global__ __launch_bounds__(256) void residual_seg_scan_kernel(const uint32_t* __restrict__ seg_bytes, int64_t n_seg,
                                                                size_t cap, uint32_t* __restrict__ seg_off,
                                                                unsigned long long* __restrict__ total,
                                                                uint32_t* __restrict__ status) {
  __shared__ uint32_t sc[256];
  __shared__ uint32_t running;
  const int img = blockIdx.x, t = threadIdx.x;
  seg_bytes += (size_t)img * n_seg;
  seg_off += (size_t)img * n_seg;
  if (t == 0) running = 0;
  __syncthreads();
  for (int64_t base = 0; base < n_seg; base += 256) {
    const int64_t i = base + t;
    const uint32_t v = i < n_seg ? seg_bytes[i] : 0u;
    sc[t] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const uint32_t a = t >= d ? sc[t - d] : 0u;
      __syncthreads();
      sc[t] += a;
      __syncthreads();
    }
    const uint32_t off = running + sc[t] - v;
    if (i < n_seg) {
      seg_off[i] = off;
      if ((size_t)off + v > cap) atomicMin(status + img, ((uint32_t)i << 4) | RES_SEG_OVERFLOW);
    }
    __syncthreads();
    if (t == 255) running += sc[255];
    __syncthreads();
  }
  if (t == 0) total[img] = running;
}

__global__ __launch_bounds__(64) void residual_decode_segments_kernel(
    const uint8_t* __restrict__ data, size_t stride, const uint32_t* __restrict__ seg_off,
    const uint32_t* __restrict__ seg_bytes, const uint8_t* __restrict__ ctx, int64_t N, int L, int64_t n_seg, int wpi,
    const ResSegDecTable* __restrict__ tabs, int16_t* __restrict__ sym, uint32_t* __restrict__ status) {
  __shared__ ResSegDecTable T;
  __shared__ uint32_t S[64 * RC_ROW];
  const int lane = threadIdx.x;
  const int img = blockIdx.x / wpi;
  const int64_t seg0 = (int64_t)(blockIdx.x % wpi) * 64;
  const int64_t k = seg0 + lane;
  const bool active = k < n_seg;
  table_to_lds(&T, tabs + img, lane);
  sym += (size_t)img * N;
  ctx += (size_t)img * N;
  const int n_k = active ? (int)residual_seg_samples(N, L, k) : 0;
  const uint32_t nw = active ? seg_bytes[(size_t)img * n_seg + k] / 4 : 0u;
  const uint32_t* w =
      active ? reinterpret_cast<const uint32_t*>(data + (size_t)img * stride + seg_off[(size_t)img * n_seg + k]) : nullptr;
  uint32_t pos = 0, bad = 0;
  auto get_word = [&]() -> uint32_t {  // never outside the segment: zeros past its end, and the count shows it
    const uint32_t v = pos < nw ? w[pos] : 0u;
    ++pos;
    return v;
  };
  uint64_t x = get_word();
  x |= (uint64_t)get_word() << 32;
  auto get_bits = [&]() -> uint32_t {  // rans.cpp's bypass read of 4 bits
    const uint32_t v = (uint32_t)x & 15u;
    x >>= 4;
    if (x < RC_L) x = (x << 32) | get_word();
    return v;
  };
  const int nch = (L + RC_CHUNK - 1) / RC_CHUNK;
  for (int c = 0; c < nch; ++c) {
    __syncthreads();
    stage_in(S, nullptr, ctx, seg0, n_seg, N, L, c, lane);
    __syncthreads();
    for (int j = 0; j < RC_CHUNK; ++j) {
      if (c * RC_CHUNK + j >= n_k) break;
      int q = 0;
      if (!bad) {
        const uint32_t ci = S[lane * RC_ROW + j] >> 16;
        const uint32_t mk = ci < (uint32_t)RES_CTX ? T.m[ci] : RES_ABSENT;
        if (mk == RES_ABSENT) {
          bad = RES_SEG_CONTEXT;
        } else {
          const uint32_t mx = 2 * mk + 1;
          const uint32_t cum = (uint32_t)x & 0xffffu;
          uint32_t s = T.lut[ci][cum >> (16 - RES_SEG_LUT_BITS)];
          while (s < mx && T.cdf[ci][s + 1] <= cum) ++s;
          const uint32_t start = T.cdf[ci][s], freq = T.cdf[ci][s + 1] - start;
          if (s > mx || cum - start >= freq) {
            bad = RES_SEG_SYMBOL;
          } else {
            x = (uint64_t)freq * (x >> 16) + cum - start;
            if (x < RC_L) x = (x << 32) | get_word();
            int value = (int)s;
            if (s == mx) {
              const uint32_t nb = get_bits();
              if (nb > (uint32_t)RES_MAX_NB) {
                bad = RES_SEG_BYPASS;
              } else {
                uint32_t raw = 0;
                for (uint32_t t = 0; t < nb; ++t) raw |= get_bits() << (4 * t);
                value = (int)(raw >> 1);
                value = (raw & 1u) ? -value - 1 : value + (int)mx;
              }
            }
            q = value - (int)mk;
            if (!bad && (q < -RES_MAX_Q || q > RES_MAX_Q)) bad = RES_SEG_RANGE;
            if (bad) q = 0;
          }
        }
      }
      S[lane * RC_ROW + j] = (uint32_t)(uint16_t)(int16_t)q;
    }
    __syncthreads();
    {  // the chunk's q, coalesced
      const int j = lane & 31;
      const int idx = c * RC_CHUNK + j;
      for (int r0 = 0; r0 < 64; r0 += 2) {
        const int r = r0 + (lane >> 5);
        const int64_t seg = seg0 + r;
        const int64_t i = seg * L + idx;
        if (seg < n_seg && idx < L && i < N) sym[i] = (int16_t)(S[r * RC_ROW + j] & 0xffffu);
      }
    }
  }
  if (!active) return;
  if (!bad && pos != nw) bad = RES_SEG_WORDS;
  if (!bad && x != RC_L) bad = RES_SEG_STATE;
  if (bad) atomicMin(status + img, ((uint32_t)k << 4) | bad);
}

unsigned seg_grid(int B, int64_t n_seg, int* wpi, const char* what) {
  const int64_t w = (n_seg + 63) / 64;
  if (w * B > 0x7fffffffLL) throw Error(std::string("mlic: ") + what + ": batch too large for one launch");
  *wpi = (int)w;
  return (unsigned)(w * B);
}

}  // namespace

void residual_encode_segments(const int16_t* sym, const uint8_t* ctx, int B, int64_t N, int L, int64_t n_seg,
                              const ResSegEncTable* tabs, uint8_t* out, size_t cap, uint32_t* seg_off,
                              uint32_t* seg_bytes, uint64_t* total, uint32_t* status, hipStream_t st) {
  int wpi;
  const unsigned blocks = seg_grid(B, n_seg, &wpi, "residual_encode_segments");
  HIP_OK(hipMemsetAsync(status, 0xFF, sizeof(uint32_t) * (size_t)B, st));  // RES_SEG_CLEAN
  hipLaunchKernelGGL(residual_encode_segments_kernel<false>, dim3(blocks), dim3(64), 0, st, sym, ctx, N, L, n_seg, wpi,
                     tabs, out, cap, seg_off, seg_bytes, status);
  hipLaunchKernelGGL(residual_seg_scan_kernel, dim3(B), dim3(256), 0, st, seg_bytes, n_seg, cap, seg_off,
                     reinterpret_cast<unsigned long long*>(total), status);
  hipLaunchKernelGGL(residual_encode_segments_kernel<true>, dim3(blocks), dim3(64), 0, st, sym, ctx, N, L, n_seg, wpi,
                     tabs, out, cap, seg_off, seg_bytes, status);
  HIP_OK(hipGetLastError());
}

void residual_decode_segments(const uint8_t* data, size_t stride, const uint32_t* seg_off, const uint32_t* seg_bytes,
                              const uint8_t* ctx, int B, int64_t N, int L, int64_t n_seg, const ResSegDecTable* tabs,
                              int16_t* sym, uint32_t* status, hipStream_t st) {
  int wpi;
  const unsigned blocks = seg_grid(B, n_seg, &wpi, "residual_decode_segments");
  HIP_OK(hipMemsetAsync(status, 0xFF, sizeof(uint32_t) * (size_t)B, st));  // RES_SEG_CLEAN
  hipLaunchKernelGGL(residual_decode_segments_kernel, dim3(blocks), dim3(64), 0, st, data, stride, seg_off, seg_bytes,
                     ctx, N, L, n_seg, wpi, tabs, sym, status);
  HIP_OK(hipGetLastError());
}

}  // namespace mlic
