// lmm_cert.hpp — the rules of the max-min certificate, one definition for the host walk (System::check_certificate,
// lmm_system.cpp) and the device pass (cert_cnst / cert_var, lmm_common_kernels.hpp).  Plain host / device code (no
// HIP beyond the function attributes): tests/c/cert_rules_check.cpp replays the comparisons check_certificate wrote
// out before next to these functions.
//
// The certificate of a solved system: it is feasible, and every judged variable (penalty > 0, value > 0) is at its
// own bound or lies on a saturated constraint on which its level value * penalty is the largest.  Every comparison
// below is a fixed expression of fp64 operations, each rounded once (the device code is compiled with
// -ffp-contract=off), so host and device decide alike on the same numbers.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define LMM_CERT_HD __host__ __device__ inline
#else
#define LMM_CERT_HD inline
#endif

namespace lmmcert {

// worst excess when no constraint is judged
constexpr double kNoExcess = -1e300;
// witness codes of a variable that has no constraint to name (= LMMHIP_WIT_*, include/lmm/lmm_hip.h)
constexpr int32_t kWitAtBound = -1, kWitNone = -2, kWitNotJudged = -3;

// A constraint takes part: the "part" test of lmm_solve's init (maxmin.cpp:524).  False for a bound of 0, a negative
// one and NaN.
LMM_CERT_HD bool judged(double b, double prec) { return b > b * prec; }
// The assertion of System::print() (maxmin.cpp:470), and the saturated set as SURVEY.md A.6 compares it.
LMM_CERT_HD bool infeasible(double u, double b, double prec) { return u - b > b * prec; }
LMM_CERT_HD bool saturated(double u, double b, double prec) { return !(b - u > b * prec); }
LMM_CERT_HD double excess(double u, double b) { return (u - b) / b; }
// A variable sits at its own bound.
LMM_CERT_HD bool at_bound(double x, double vb, double prec) {
  const double tol = 1e-9 * vb;
  return vb > 0 && std::fabs(x - vb) <= (prec < tol ? tol : prec);  // (std::max(prec, 1e-9 * vb))
}
// A variable of level x * penalty is among the largest of a constraint whose largest level is `top`.
LMM_CERT_HD bool carries(double level, double top) { return level >= top * (1 - 1e-9); }

}  // namespace lmmcert
