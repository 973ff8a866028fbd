// lmm_keywin.hpp — the 16-bit keys of the max-min round kernels as codes of a per-solve window over the f32 bits of
// the ratio.  Plain host / device code: the kernels of lmm_maxmin_kernels.hpp make every key through key_code, the
// round engine chooses its window on the device once per solve (mm_key_window), tests/c/keywin_check.cpp checks the
// map and the choice on the host.
//
//   code(r) = min(kKeyTop, (max(bits(f32_rd(r)), base) - base) >> shift)
//
// The bits of a non-negative f32 order like the value, and the round-down conversion, the clamp at both ends and the
// shift are all monotone non-decreasing, so code(a) < code(b) => a < b for ANY window.  The keys are only a prefilter
// (a vote takes the exact lexicographic (ratio, id) minimum among the constraints at the minimal key, and a vote stands
// only while its target's key is strictly below the row's floor), so every target, round and value of a solve is the
// same under every window; a window that fits the solve's ratios badly only sends more rows to the exact compares.
// {0, 16} is the key the engines had before — sign, exponent and the upper 7 mantissa bits of the f32 — and stays the
// window of the persistent and batch engines and of a round-engine solve under LMMHIP_KEY_WINDOW=0.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define LMM_KW_FN __host__ __device__ __forceinline__
#else
#define LMM_KW_FN inline
#endif

#ifndef LMM_KEY_MANT
#define LMM_KEY_MANT 7  // mantissa bits of the legacy key (build knob, measurement)
#endif

struct KeyWin {
  uint32_t base;  // f32 bits of the window's lower end: ratios at or below it take code 0
  int shift;      // f32 bit patterns per code, as a power of two (0..31)
};
// The top live code: strictly below the two keys of a constraint out of the light table (kSatKey 0xFFFE, kDeadKey
// 0xFFFF, lmm_dev.hpp).  +inf and every ratio above the window clamp here.
constexpr unsigned kKeyTop = 0xFFFDu;
constexpr KeyWin kKeyWinLegacy{0u, 23 - LMM_KEY_MANT};

// The bits of r rounded down (toward -inf) to f32.
LMM_KW_FN uint32_t f32_rd_bits(double r) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __float_as_uint(__double2float_rd(r));
#else
  float f = float(r);  // (to nearest: one step down where that rounded up; FLT_MAX for a finite r above it)
  if (double(f) > r)
    f = std::nextafterf(f, -INFINITY);
  uint32_t u;
  std::memcpy(&u, &f, sizeof u);
  return u;
#endif
}

LMM_KW_FN unsigned key_code_bits(uint32_t bits, KeyWin w) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t c = __builtin_elementwise_sub_sat(bits, w.base) >> w.shift;  // (one clamped subtract)
#else
  const uint32_t c = ((bits > w.base ? bits : w.base) - w.base) >> w.shift;
#endif
  return c < kKeyTop ? unsigned(c) : kKeyTop;
}
// r: a non-negative ratio or bound level (+inf included).
LMM_KW_FN unsigned key_code(double r, KeyWin w) { return key_code_bits(f32_rd_bits(r), w); }

// The window of a solve whose initial alive ratios span [lo, hi]: base = bits(f32_rd(lo)), shift the smallest s with
// (bits(f32_rd(hi * headroom)) - base) >> s <= kKeyTop.  Ratios only grow during a solve: the headroom says how far
// above the initial maximum the codes stay distinct (above it they clamp at kKeyTop).  No alive ratio (lo > hi, or a
// NaN): the legacy window.
LMM_KW_FN KeyWin key_window(double lo, double hi, double headroom) {
  if (!(lo <= hi) || !(lo >= 0))
    return kKeyWinLegacy;
  KeyWin w;
  w.base = f32_rd_bits(lo);
  const uint32_t top = f32_rd_bits(hi * headroom);
  const uint32_t span = top > w.base ? top - w.base : 0u;
  w.shift = 0;
  while ((span >> w.shift) > kKeyTop)
    w.shift++;
  return w;
}
