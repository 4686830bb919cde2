// Tables of the separable, antialiased polyphase resampler (DESIGN.md section 5 "Scaled coding"; the rule of PIL's
// ImagingResample and of torch's interpolate(antialias=True)).  Host only, plain C++17, no HIP: g++ alone compiles it.
//
// Per axis (input length Li, output length Lo): s = Li / Lo, fs = max(s, 1), support = a * fs with a = 3 (lanczos3),
// 2 (bicubic, Keys a = -0.5), 1 (triangle).  For output o: c = (o + 0.5) s, x0 = max(0, int(c - support + 0.5)),
// x1 = min(Li, int(c + support + 0.5)), n = x1 - x0, w_j = k((j + x0 - c + 0.5) / fs) for j < n, divided by their
// sum; all in double, each weight rounded once to fp32.  Lo == Li is by definition the identity table (n = 1,
// weight 1): sin(pi) is not 0 in floating point, so a computed Lanczos identity would not be exact.
//
// Tap bound.  1/8 <= Lo / Li <= 8 is the allowed ratio, so fs <= 8 and support <= 3 * 8 = 24.  x0 and x1 are the
// truncations of two numbers 2 * support apart, so n <= 2 * support + 1: at most RESAMPLE_MAX_TAPS = 49 taps
// (lanczos3 at ratio 1/8; 33 for bicubic, 17 for triangle), and at most 7 / 5 / 3 when the axis does not shrink.
#ifndef MLIC_RESAMPLE_TABLE_H
#define MLIC_RESAMPLE_TABLE_H
#include <cmath>
#include <cstdint>

namespace mlic {

enum { RESAMPLE_LANCZOS3 = 0, RESAMPLE_BICUBIC = 1, RESAMPLE_TRIANGLE = 2, RESAMPLE_FILTERS = 3 };
constexpr int RESAMPLE_MAX_RATIO = 8;
constexpr int RESAMPLE_MAX_TAPS = 2 * 3 * RESAMPLE_MAX_RATIO + 1;  // 49, see above
constexpr int RESAMPLE_MAX_SIDE = 1 << 24;

inline int resample_filter_radius(int filter) {
  return filter == RESAMPLE_LANCZOS3 ? 3 : filter == RESAMPLE_BICUBIC ? 2 : 1;
}

inline double resample_kernel(int filter, double x) {
  if (filter == RESAMPLE_LANCZOS3) {
    if (!(x >= -3.0 && x < 3.0)) return 0.0;
    auto sinc = [](double t) {
      if (t == 0.0) return 1.0;
      t *= 3.14159265358979323846;
      return std::sin(t) / t;
    };
    return sinc(x) * sinc(x / 3.0);
  }
  x = std::fabs(x);
  if (filter == RESAMPLE_BICUBIC) {
    const double a = -0.5;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
    if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
    return 0.0;
  }
  return x < 1.0 ? 1.0 - x : 0.0;
}

// nullptr when filter, Li, Lo follow the rules
inline const char* resample_axis_check(int filter, int64_t Li, int64_t Lo) {
  if (filter < 0 || filter >= RESAMPLE_FILTERS) return "resample: unknown filter (0 lanczos3, 1 bicubic, 2 triangle)";
  if (Li < 1 || Lo < 1) return "resample: lengths must be positive";
  if (Li > RESAMPLE_MAX_SIDE || Lo > RESAMPLE_MAX_SIDE) return "resample: a length above 2^24";
  if (Lo > RESAMPLE_MAX_RATIO * Li || Li > RESAMPLE_MAX_RATIO * Lo)
    return "resample: the ratio of output to input length must lie in [1/8, 8]";
  return nullptr;
}

// output o's window [*x0, *x0 + n) and the centre; returns n
inline int resample_window(int filter, int Li, int Lo, int o, int* x0, double* centre, double* fs_out) {
  if (Li == Lo) {
    *x0 = o;
    *centre = o + 0.5;
    *fs_out = 1.0;
    return 1;
  }
  const double s = (double)Li / (double)Lo, fs = s > 1.0 ? s : 1.0;
  const double support = resample_filter_radius(filter) * fs, c = (o + 0.5) * s;
  int a = (int)(c - support + 0.5), b = (int)(c + support + 0.5);
  if (a < 0) a = 0;
  if (b > Li) b = Li;
  *x0 = a;
  *centre = c;
  *fs_out = fs;
  return b - a;
}

// *taps = the largest n of the table.  start, count (Lo entries each) and weights (Lo rows of `stride` floats, the
// entries j >= n of a row +0) are filled when all three are given and stride >= *taps; all three null is the size
// query.  Returns nullptr or a static message.
inline const char* resample_table(int filter, int Li, int Lo, int32_t* start, int32_t* count, float* weights, int stride,
                                  int* taps) {
  if (taps == nullptr) return "resample_table: null taps";
  if (const char* err = resample_axis_check(filter, Li, Lo)) return err;
  const bool fill = start != nullptr || count != nullptr || weights != nullptr;
  if (fill && (start == nullptr || count == nullptr || weights == nullptr))
    return "resample_table: start, count and weights go together";
  int most = 0;
  for (int o = 0; o < Lo; ++o) {
    int x0;
    double c, fs;
    const int n = resample_window(filter, Li, Lo, o, &x0, &c, &fs);
    if (n < 1 || n > RESAMPLE_MAX_TAPS) return "resample_table: a tap count outside [1, 49] (internal)";
    if (n > most) most = n;
  }
  *taps = most;
  if (!fill) return nullptr;
  if (stride < most) return "resample_table: stride is below the table's tap count";
  for (int o = 0; o < Lo; ++o) {
    int x0;
    double c, fs;
    const int n = resample_window(filter, Li, Lo, o, &x0, &c, &fs);
    float* w = weights + (int64_t)o * stride;
    start[o] = x0;
    count[o] = n;
    double k[RESAMPLE_MAX_TAPS], sum = 0.0;
    if (Li == Lo) {
      k[0] = sum = 1.0;
    } else {
      for (int j = 0; j < n; ++j) sum += k[j] = resample_kernel(filter, ((double)(j + x0) - c + 0.5) / fs);
    }
    for (int j = 0; j < n; ++j) w[j] = (float)(k[j] / sum);
    for (int j = n; j < stride; ++j) w[j] = 0.0f;
  }
  return nullptr;
}

}  // namespace mlic
#endif
