// keywin_check.cpp — the key window of the max-min round kernels (simgrid_amd/csrc/lmm_keywin.hpp), checked on the
// host: g++ -O2 -std=c++17 keywin_check.cpp (tests/test_keywin.py; host code only, so it also builds under
// -fsanitize=address,undefined).  Prints "ok <checks> <relative code width of the C2 window> <legacy's>".
#include <algorithm>
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../simgrid_amd/csrc/lmm_keywin.hpp"

static long checks = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    checks++;                                     \
    if (!(cond)) {                                \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                   \
      std::printf("\n");                          \
      return 1;                                   \
    }                                             \
  } while (0)

constexpr unsigned kSatKey = 0xFFFEu;  // (lmm_dev.hpp)

// The key before the window: the upper 16 bits of the ratio rounded down to f32 (lmm_dev.hpp's ratio_key as it was).
static unsigned legacy_key(double r) { return (f32_rd_bits(r) >> 16) & 0xFFFFu; }

// Non-negative doubles over everything a ratio or a bound level can be: zero, f64 and f32 denormals, the whole f32
// range, values above it, +inf; with neighbours one ulp apart and exact repeats.
static std::vector<double> sample() {
  std::vector<double> v = {0.0,     4.9e-324, 1e-320,  DBL_MIN, 1e-300, 1e-46,   1.4e-45, 1e-40, FLT_MIN,
                           1e-30,   1e-10,    1e-4,    0.08,    0.4,    1.0,     10.0,    1e10,  1e30,
                           FLT_MAX, 3.5e38,   1e39,    1e300,   DBL_MAX, INFINITY};
  std::mt19937_64 g(12345);
  std::uniform_real_distribution<double> ex(-330.0, 320.0), c2(1e-4, 0.4);
  for (int i = 0; i < 20000; i++)
    v.push_back(std::pow(10.0, ex(g)));
  for (int i = 0; i < 20000; i++)
    v.push_back(c2(g));
  const size_t n = v.size();
  for (size_t i = 0; i < n; i++) {
    v.push_back(std::nextafter(v[i], INFINITY));
    v.push_back(std::nextafter(v[i], 0.0));
    v.push_back(double(float(v[i])));  // exactly an f32 (or +inf)
    v.push_back(v[i]);                 // an exact repeat
  }
  std::sort(v.begin(), v.end());
  return v;
}

int main() {
  const std::vector<double> v = sample();
  // the round-down conversion itself: never above the value, and the next f32 is
  for (double r : v) {
    uint32_t u = f32_rd_bits(r);
    float f;
    std::memcpy(&f, &u, sizeof f);
    CHECK(double(f) <= r, "f32_rd(%a) = %a above it", r, double(f));
    CHECK(!(double(std::nextafterf(f, INFINITY)) <= r) || r == INFINITY, "f32_rd(%a) = %a not the nearest below", r,
          double(f));
  }
  const KeyWin wins[] = {kKeyWinLegacy,
                         key_window(1e-4, 0.4, 1.0),
                         key_window(1e-4, 0.08, 4.0),
                         key_window(1e-30, 1e30, 1.0),
                         key_window(1e-30, 1e30, 64.0),
                         key_window(0.5, 0.5, 1.0),
                         key_window(0.0, INFINITY, 1.0),
                         key_window(4.9e-324, 1e-320, 2.0),
                         KeyWin{0x3F800000u, 0},
                         KeyWin{0x00000001u, 31},
                         KeyWin{0x7F800000u, 3}};
  for (const KeyWin w : wins) {
    CHECK(w.shift >= 0 && w.shift < 32, "shift %d", w.shift);
    unsigned prev = 0;
    for (size_t i = 0; i < v.size(); i++) {
      const unsigned c = key_code(v[i], w);
      CHECK(c < kSatKey && c <= kKeyTop, "code %#x of %a not below kSatKey (base %#x shift %d)", c, v[i], w.base, w.shift);
      CHECK(c >= prev, "not monotone at %a: %#x after %#x (base %#x shift %d)", v[i], c, prev, w.base, w.shift);
      if (i && v[i] == v[i - 1])
        CHECK(c == prev, "equal inputs %a, codes %#x and %#x", v[i], prev, c);
      prev = c;
    }
    // both clamps
    uint32_t below = w.base ? w.base - 1 : 0;
    CHECK(key_code_bits(below, w) == 0 && key_code_bits(w.base, w) == 0, "below the base not code 0");
    CHECK(key_code(INFINITY, w) == std::min<uint64_t>(kKeyTop, (uint64_t(0x7F800000u) - std::min(w.base, 0x7F800000u)) >> w.shift),
          "+inf");
  }
  // {0, 16} is the key the engines had
  CHECK(kKeyWinLegacy.base == 0 && kKeyWinLegacy.shift == 16, "legacy window {%u, %d}", kKeyWinLegacy.base,
        kKeyWinLegacy.shift);
  for (double r : v)
    CHECK(key_code(r, KeyWin{0u, 16}) == legacy_key(r), "legacy key of %a: %#x, window {0, 16}: %#x", r, legacy_key(r),
          key_code(r, KeyWin{0u, 16}));
  // the C2 range plus headroom, [1e-4, 0.4]: the largest relative width of a code inside the window, against legacy's
  const KeyWin c2 = key_window(1e-4, 0.4, 1.0);
  CHECK(key_code(1e-4, c2) == 0 && key_code(0.4, c2) <= kKeyTop && key_code(0.4, c2) > kKeyTop / 2,
        "C2 window {%#x, %d}: codes %#x..%#x", c2.base, c2.shift, key_code(1e-4, c2), key_code(0.4, c2));
  auto width = [&](KeyWin w) {  // max over the sample in [1e-4, 0.4] of (upper end of r's code - lower end) / lower end
    double worst = 0;
    for (double r : v) {
      if (r < 1e-4 || r > 0.4)
        continue;
      const uint32_t b = f32_rd_bits(r);
      const uint32_t lo = w.base + (((b - w.base) >> w.shift) << w.shift), hi = lo + (1u << w.shift);
      float fl, fh;
      std::memcpy(&fl, &lo, 4);
      std::memcpy(&fh, &hi, 4);
      worst = std::max(worst, (double(fh) - double(fl)) / double(fl));
    }
    return worst;
  };
  const double wc2 = width(c2), wleg = width(kKeyWinLegacy);
  CHECK(wc2 < wleg, "C2 window's code width %.3g not finer than legacy's %.3g", wc2, wleg);
  CHECK(wleg > 0.0078 && wleg < 0.0079, "legacy width %.6g (2^-7)", wleg);
  // the choice: degenerate windows
  {
    const KeyWin w = key_window(0.5, 0.5, 1.0);
    CHECK(w.shift == 0 && w.base == f32_rd_bits(0.5), "min == max: {%#x, %d}", w.base, w.shift);
    const KeyWin t = key_window(3.0, 3.0000001, 1.0);  // a few f32 steps wide
    CHECK(t.shift == 0 && key_code(3.0000001, t) <= 2, "narrow window {%#x, %d}", t.base, t.shift);
  }
  for (double head : {1.0, 4.0, 1e6, 1e38}) {
    const KeyWin w = key_window(1e-30, 1e30, head);
    const uint32_t top = f32_rd_bits(1e30 * head);
    CHECK(((top - w.base) >> w.shift) <= kKeyTop, "1e-30..1e30 x %g: top code %#x", head, (top - w.base) >> w.shift);
    CHECK(w.shift == 0 || ((top - w.base) >> (w.shift - 1)) > kKeyTop, "shift %d not the smallest", w.shift);
    CHECK(key_code(1e-30, w) == 0 && key_code(1e30, w) > key_code(1.0, w) && key_code(1.0, w) > 0, "codes across the range");
  }
  {  // the smallest shift, over many ranges
    std::mt19937_64 g(7);
    std::uniform_real_distribution<double> ex(-40.0, 38.0);
    for (int i = 0; i < 20000; i++) {
      double a = std::pow(10.0, ex(g)), b = std::pow(10.0, ex(g));
      if (a > b)
        std::swap(a, b);
      const KeyWin w = key_window(a, b, 4.0);
      const uint32_t top = f32_rd_bits(b * 4.0);
      CHECK(w.base == f32_rd_bits(a) && ((top - w.base) >> w.shift) <= kKeyTop, "window of [%a, %a]", a, b);
      CHECK(w.shift == 0 || ((top - w.base) >> (w.shift - 1)) > kKeyTop, "shift %d of [%a, %a] not the smallest", w.shift,
            a, b);
      CHECK(w.shift <= 15, "shift %d", w.shift);
    }
  }
  // nothing alive (lo > hi, the reduction's identities) or a NaN: the legacy window
  CHECK(key_window(INFINITY, 0.0, 4.0).shift == 16 && key_window(INFINITY, 0.0, 4.0).base == 0, "empty range");
  CHECK(key_window(NAN, 1.0, 4.0).shift == 16, "NaN range");
  std::printf("ok %ld %.6g %.6g\n", checks, wc2, wleg);
  return 0;
}
